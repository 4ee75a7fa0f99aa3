// rt_temporal.h — the film's temporal accumulation (include/mi355rt.h: rt_film_temporal, rt_film_temporal_moments): carry the previous frame's mean to where
// its surfaces are under the current camera, reject what has become visible, and blend in the new passes.  A pixel's first hit
// (this frame's guides: distance, normal, object id) gives its world point; the previous camera and the closed-form grid map that
// point back to a fractional pixel of the history with two divisions; the four pixels around it are bilinear taps, each kept only
// if the history's guides show the same object at the same squared distance (relative tolerance) under a normal that has not
// turned away, and if its history stands for at least one pass.  What survives is blended with the new sum by pass counts.
// The arithmetic of one pixel (temporal_pixel) is HIP-free, like rt_denoise.h and for the same reason: the kernel below and
// tests/algo/temporal_check.cpp, a CPU program built under AddressSanitizer and UBSan, compile the same text.  Everything here is
// float64 without fused multiply-add (the Makefile's -ffp-contract=off; the CPU program's too), in the header's order; the one
// square root is the normalize of the primary ray, rt_math.h's normalize3_generic, as the guides form that ray.
// Every tap index is range-checked before it is read, whatever the guides, sums or history hold (NaN and Inf included): a
// projection that is not a number inside (-1, w) x (-1, h) is a fresh pixel before any index is formed from it.
// The kernel (hipcc only): one thread per pixel, consecutive threads consecutive y (the fast axis of the layout), a grid capped
// near 8 blocks per CU with a grid-stride loop; under a small camera move neighbouring pixels read neighbouring taps, so the four
// gathers mostly coalesce; 8- and 4-byte accesses, so any plane stride will do; no LDS, no scratch, 64-bit plane offsets.
// rt_film_temporal_moments carries the history's mean of squares through the same taps: the tap loop and the blend are written once,
// as templates over MOMENTS (temporal_taps_of, temporal_pixel_of), and the plain instantiation, which compiles none of the moment
// lines, is handed a null TemporalMomentsArgs that it never reads.
#pragma once
#include <cstdint>

#include "rt_math.h"

#if defined(__HIPCC__)
#define RT_TP_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define RT_TP_HD
#endif

namespace rt {

// One call over a w x h frame.  Cameras and grid travel by value, as in every launch.
struct TemporalArgs {
    const double *sum;          // this frame's sum of n passes, 3 planes
    const float *guides;        // this frame's guides, 8 planes
    const double *hist;         // the previous frame's mean, 3 planes
    const float *hist_len;      // passes each history pixel stands for, 1 plane
    const float *hist_guides;   // the previous frame's guides, 8 planes
    double *out;                // the new mean, 3 planes
    float *out_len;             // the new length plane
    long long sum_stride, guide_stride, hist_stride, hist_guide_stride, out_stride;
    int w, h;
    double n;                   // (double)n
    double px, y0, dy, z0, dz;  // the closed-form grid
    double o[3], R[9];          // the current camera
    double po[3], pR[9];        // the camera the history was rendered with
    double depth_tol, normal_cos, max_history;
};

// What the history gives pixel (x, y): valid (some tap survived), the taps' weighted mean hm and their length L (capped).
struct TemporalTaps {
    bool valid;
    double hm[3], L;
};

// rt_film_temporal_moments: the call above and, beside it, the second moment.  sq is this frame's sum of squares, hist_sq the
// history's MEAN of squares, out_sq the new mean of squares, three planes each.
struct TemporalMomentsArgs {
    TemporalArgs t;
    const double *sq, *hist_sq;
    double *out_sq;
    long long sq_stride, hist_sq_stride, out_sq_stride;
};

RT_TP_HD inline double temporal_snap(double f)
{
    const double r = __builtin_floor(f + 0.5);
    return __builtin_fabs(f - r) <= 0x1p-20 ? r : f;
}

// The history's taps around where pixel (x, y) was.  With MOMENTS the history's mean of squares (three planes at m->hist_sq) is
// weighed through the same taps into hq: after H_k the line Q_k = Q_k + bw * hist_sq[k][q].
template <bool MOMENTS>
RT_TP_HD inline TemporalTaps temporal_taps_of(const TemporalArgs &a, const TemporalMomentsArgs *m, int x, int y, double *hq)
{
    TemporalTaps r{false, {0.0, 0.0, 0.0}, 0.0};
    const long long e = (long long)x * a.h + y;
    const float idp = a.guides[7 * a.guide_stride + e];
    if (idp < 0.0f || a.max_history == 0.0) return r;
    const V3 P{a.px, (double)x * a.dy + a.y0, (double)y * a.dz + a.z0};
    const V3 d = normalize3_generic(V3{a.R[0] * P.x + a.R[1] * P.y + a.R[2] * P.z,
                                       a.R[3] * P.x + a.R[4] * P.y + a.R[5] * P.z,
                                       a.R[6] * P.x + a.R[7] * P.y + a.R[8] * P.z});
    const double t = (double)a.guides[3 * a.guide_stride + e];
    const double u0 = (a.o[0] + t * d.x) - a.po[0], u1 = (a.o[1] + t * d.y) - a.po[1], u2 = (a.o[2] + t * d.z) - a.po[2];
    const double q0 = (a.pR[0] * u0 + a.pR[3] * u1) + a.pR[6] * u2;
    const double q1 = (a.pR[1] * u0 + a.pR[4] * u1) + a.pR[7] * u2;
    const double q2 = (a.pR[2] * u0 + a.pR[5] * u1) + a.pR[8] * u2;
    if (!(q0 > 0.0)) return r;
    const double r2 = (u0 * u0 + u1 * u1) + u2 * u2;
    const double sc = a.px / q0;
    const double fx = temporal_snap((q1 * sc - a.y0) / a.dy), fy = temporal_snap((q2 * sc - a.z0) / a.dz);
    if (!(fx > -1.0 && fx < (double)a.w && fy > -1.0 && fy < (double)a.h)) return r;   // (NaN lands here)
    const double flx = __builtin_floor(fx), fly = __builtin_floor(fy);
    const double ax = fx - flx, ay = fy - fly;
    const int ix = (int)flx, iy = (int)fly;                                           // -1 .. w-1, -1 .. h-1
    const double nx = (double)a.guides[e], ny = (double)a.guides[a.guide_stride + e], nz = (double)a.guides[2 * a.guide_stride + e];
    double W = 0.0, H0 = 0.0, H1 = 0.0, H2 = 0.0, Lh = 0.0, Q0 = 0.0, Q1 = 0.0, Q2 = 0.0;
    for (int ta = 0; ta < 2; ++ta) {
        const int qx = ix + ta;
        for (int tb = 0; tb < 2; ++tb) {
            const int qy = iy + tb;
            const double bw = (ta ? ax : 1.0 - ax) * (tb ? ay : 1.0 - ay);
            if (bw == 0.0 || qx < 0 || qx >= a.w || qy < 0 || qy >= a.h) continue;
            const long long eq = (long long)qx * a.h + qy;
            if (a.hist_guides[7 * a.hist_guide_stride + eq] != idp) continue;
            const double tq = (double)a.hist_guides[3 * a.hist_guide_stride + eq];
            if (!(__builtin_fabs(tq * tq - r2) <= a.depth_tol * r2)) continue;
            const double cn = ((nx * (double)a.hist_guides[eq]) + (ny * (double)a.hist_guides[a.hist_guide_stride + eq])) +
                              (nz * (double)a.hist_guides[2 * a.hist_guide_stride + eq]);
            if (!(cn >= a.normal_cos)) continue;
            const double lq = (double)a.hist_len[eq];
            if (!(lq > 0.0)) continue;
            W = W + bw;
            H0 = H0 + bw * a.hist[eq]; H1 = H1 + bw * a.hist[a.hist_stride + eq]; H2 = H2 + bw * a.hist[2 * a.hist_stride + eq];
            if constexpr (MOMENTS) {
                Q0 = Q0 + bw * m->hist_sq[eq]; Q1 = Q1 + bw * m->hist_sq[m->hist_sq_stride + eq]; Q2 = Q2 + bw * m->hist_sq[2 * m->hist_sq_stride + eq];
            }
            Lh = Lh + bw * lq;
        }
    }
    if (!(W > 0.0)) return r;
    r.valid = true;
    r.hm[0] = H0 / W; r.hm[1] = H1 / W; r.hm[2] = H2 / W;
    if constexpr (MOMENTS) { hq[0] = Q0 / W; hq[1] = Q1 / W; hq[2] = Q2 / W; }
    const double L = Lh / W;
    r.L = L > a.max_history ? a.max_history : L;
    return r;
}

// Pixel (x, y), written to out and out_len; with MOMENTS out_sq receives the second moment blended by the same lengths.
template <bool MOMENTS>
RT_TP_HD inline void temporal_pixel_of(const TemporalArgs &a, const TemporalMomentsArgs *m, int x, int y)
{
    const long long e = (long long)x * a.h + y;
    double hq[3] = {0.0, 0.0, 0.0};
    const TemporalTaps tp = temporal_taps_of<MOMENTS>(a, m, x, y, hq);
    const double s0 = a.sum[e], s1 = a.sum[a.sum_stride + e], s2 = a.sum[2 * a.sum_stride + e];
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    if constexpr (MOMENTS) { q0 = m->sq[e]; q1 = m->sq[m->sq_stride + e]; q2 = m->sq[2 * m->sq_stride + e]; }
    if (!tp.valid) {                                                                  // fresh
        a.out[e] = s0 / a.n; a.out[a.out_stride + e] = s1 / a.n; a.out[2 * a.out_stride + e] = s2 / a.n;
        if constexpr (MOMENTS) {
            m->out_sq[e] = q0 / a.n; m->out_sq[m->out_sq_stride + e] = q1 / a.n; m->out_sq[2 * m->out_sq_stride + e] = q2 / a.n;
        }
        a.out_len[e] = (float)a.n;
        return;
    }
    const double den = tp.L + a.n;
    a.out[e] = (tp.L * tp.hm[0] + s0) / den;
    a.out[a.out_stride + e] = (tp.L * tp.hm[1] + s1) / den;
    a.out[2 * a.out_stride + e] = (tp.L * tp.hm[2] + s2) / den;
    if constexpr (MOMENTS) {
        m->out_sq[e] = (tp.L * hq[0] + q0) / den;
        m->out_sq[m->out_sq_stride + e] = (tp.L * hq[1] + q1) / den;
        m->out_sq[2 * m->out_sq_stride + e] = (tp.L * hq[2] + q2) / den;
    }
    a.out_len[e] = (float)den;
}

RT_TP_HD inline TemporalTaps temporal_taps(const TemporalArgs &a, int x, int y) { return temporal_taps_of<false>(a, nullptr, x, y, nullptr); }
RT_TP_HD inline void temporal_pixel(const TemporalArgs &a, int x, int y) { temporal_pixel_of<false>(a, nullptr, x, y); }

// out and out_len receive temporal_pixel's bits: the same lines.
RT_TP_HD inline TemporalTaps temporal_moments_taps(const TemporalMomentsArgs &m, int x, int y, double *hq) { return temporal_taps_of<true>(m.t, &m, x, y, hq); }
RT_TP_HD inline void temporal_moments_pixel(const TemporalMomentsArgs &m, int x, int y) { temporal_pixel_of<true>(m.t, &m, x, y); }

#if defined(__HIPCC__)

constexpr int TEMPORAL_THREADS = 256;

// w*h <= RT_FILM_MAX_PIXELS = 2^27: pixel indices are 32-bit, plane offsets 64-bit
__global__ __launch_bounds__(TEMPORAL_THREADS) void temporal_kernel(const TemporalArgs a)
{
    const unsigned npx = (unsigned)a.w * (unsigned)a.h, step = gridDim.x * TEMPORAL_THREADS;
    for (unsigned e = blockIdx.x * TEMPORAL_THREADS + threadIdx.x; e < npx; e += step) {
        const unsigned x = e / (unsigned)a.h;
        temporal_pixel(a, (int)x, (int)(e - x * (unsigned)a.h));
    }
}

// the same shape with the second moment: 24 B more read of this frame, 24 B more per surviving tap, 24 B more written
__global__ __launch_bounds__(TEMPORAL_THREADS) void temporal_moments_kernel(const TemporalMomentsArgs m)
{
    const unsigned npx = (unsigned)m.t.w * (unsigned)m.t.h, step = gridDim.x * TEMPORAL_THREADS;
    for (unsigned e = blockIdx.x * TEMPORAL_THREADS + threadIdx.x; e < npx; e += step) {
        const unsigned x = e / (unsigned)m.t.h;
        temporal_moments_pixel(m, (int)x, (int)(e - x * (unsigned)m.t.h));
    }
}

// blocks of a temporal launch over npx pixels: at most 8 per CU, as the film and denoise kernels'
inline unsigned temporal_grid(long long npx, int cu_count)
{
    const long long want = (npx + TEMPORAL_THREADS - 1) / TEMPORAL_THREADS, cap = (long long)cu_count * 8;
    const long long n = want < cap ? want : cap;
    return (unsigned)(n < 1 ? 1 : n);
}

#endif  // __HIPCC__

}  // namespace rt
