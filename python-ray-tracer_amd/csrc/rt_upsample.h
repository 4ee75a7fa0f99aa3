// rt_upsample.h — guided upsampling (include/mi355rt.h: rt_film_upsample): lift a mean that was accumulated and filtered on a coarse
// grid to the display grid along first-hit guides rendered at both resolutions.  An output pixel's place on the coarse grid follows
// from the two closed-form grids alone (no camera: both frames see the same rays' directions, scaled by px); the four coarse pixels
// around it are bilinear taps, each kept only if the coarse guides show the output pixel's object under a normal that has not turned
// away (stage 0).  Where none survives, the 4 x 4 coarse pixels around it are searched for the object, weighted by a rational
// fall-off of their distance (stage 1); where the object is not there at all (it is thinner than a coarse pixel), the plain bilinear
// mean stands in (stage 2).  With demodulation the taps carry colour / albedo of the coarse guides and the result is multiplied by
// the output pixel's own albedo, so texture detail comes from the display-resolution guides.
// The arithmetic of one pixel (upsample_pixel) is HIP-free, like rt_temporal.h and for the same reason: the kernel below and
// tests/algo/upsample_check.cpp, a CPU program built under AddressSanitizer and UBSan, compile the same text.  Everything here is
// float64 without fused multiply-add (the Makefile's -ffp-contract=off; the CPU program's too), in the header's order; no exp(),
// pow() or square root.  Every tap index is range-checked before it is read, whatever the guides and the mean hold (NaN and Inf
// included): the fractional position is clamped into the coarse frame (NaN to 0) before any index is formed from it.
// The kernel (hipcc only): one thread per output pixel, consecutive threads consecutive Y (the fast axis of the layout), a grid
// capped near 8 blocks per CU with a grid-stride loop; neighbouring output pixels share their taps, so most tap loads hit the
// caches; 8- and 4-byte accesses, so any plane stride will do; no LDS, no scratch, 64-bit plane offsets.  Only the lanes whose
// stage 0 found nothing walk the 16 taps of stage 1: that loop sits behind the test and is not unrolled, as the pooled path of
// denoise_var_prepare_len_pixel (rt_denoise_var.h).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RT_UP_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define RT_UP_HD
#endif

namespace rt {

// One call: a wl x hl mean (sum of n) to a w x h frame.  Both grids travel by value.
struct UpsampleArgs {
    const double *lo;           // the coarse sum of n passes (or a mean with n = 1), planes 0..2
    const float *lo_guides;     // the coarse frame's guides, 8 planes
    const float *hi_guides;     // the output frame's guides, 8 planes
    double *out;                // the lifted mean, 3 planes
    float *kind;                // nullptr, or one plane: the stage that wrote each pixel
    long long lo_stride, lo_guide_stride, hi_guide_stride, out_stride;
    int wl, hl, w, h;
    double n;                   // (double)n
    double lo_px, lo_y0, lo_dy, lo_z0, lo_dz;
    double hi_px, hi_y0, hi_dy, hi_z0, hi_dz;
    double normal_cos;
    int demod;
};

RT_UP_HD inline double upsample_snap(double f)
{
    const double r = __builtin_floor(f + 0.5);
    return __builtin_fabs(f - r) <= 0x1p-20 ? r : f;
}

// f into [0, last]: anything that is not >= 0 (NaN included) becomes 0.
RT_UP_HD inline double upsample_clamp(double f, int last)
{
    if (!(f >= 0.0)) f = 0.0;
    if (f > (double)last) f = (double)last;
    return f;
}

RT_UP_HD inline double upsample_albedo(float v)
{
    const double d = (double)v;
    return d > 1.0 ? d : 1.0;
}

// The running sums of a stage.
struct UpsampleSums { double W, A0, A1, A2; };

// Coarse pixel eq with weight wt onto s: the mean, over the coarse albedo where demod.
RT_UP_HD inline void upsample_add(const UpsampleArgs &a, long long eq, double wt, bool demod, UpsampleSums &s)
{
    double v0 = a.lo[eq] / a.n, v1 = a.lo[a.lo_stride + eq] / a.n, v2 = a.lo[2 * a.lo_stride + eq] / a.n;
    if (demod) {
        v0 = v0 / upsample_albedo(a.lo_guides[4 * a.lo_guide_stride + eq]);
        v1 = v1 / upsample_albedo(a.lo_guides[5 * a.lo_guide_stride + eq]);
        v2 = v2 / upsample_albedo(a.lo_guides[6 * a.lo_guide_stride + eq]);
    }
    s.W = s.W + wt;
    s.A0 = s.A0 + wt * v0; s.A1 = s.A1 + wt * v1; s.A2 = s.A2 + wt * v2;
}

// The 2 x 2 bilinear taps around (ix + ax, iy + ay).  GUIDED: stage 0 (the id and normal tests, demodulation as asked); else stage 2.
template <bool GUIDED>
RT_UP_HD inline UpsampleSums upsample_bilinear(const UpsampleArgs &a, long long e, float idp, int ix, int iy, double ax, double ay)
{
    UpsampleSums s{0.0, 0.0, 0.0, 0.0};
    for (int ta = 0; ta < 2; ++ta) {
        const int qx = ix + ta;
        for (int tb = 0; tb < 2; ++tb) {
            const int qy = iy + tb;
            const double bw = (ta ? ax : 1.0 - ax) * (tb ? ay : 1.0 - ay);
            if (bw == 0.0 || qx < 0 || qx >= a.wl || qy < 0 || qy >= a.hl) continue;
            const long long eq = (long long)qx * a.hl + qy;
            if constexpr (GUIDED) {
                if (a.lo_guides[7 * a.lo_guide_stride + eq] != idp) continue;
                if (idp >= 0.0f) {
                    const double cn = (((double)a.hi_guides[e] * (double)a.lo_guides[eq]) +
                                       ((double)a.hi_guides[a.hi_guide_stride + e] * (double)a.lo_guides[a.lo_guide_stride + eq])) +
                                      ((double)a.hi_guides[2 * a.hi_guide_stride + e] * (double)a.lo_guides[2 * a.lo_guide_stride + eq]);
                    if (!(cn >= a.normal_cos)) continue;
                }
            }
            upsample_add(a, eq, bw, GUIDED && a.demod, s);
        }
    }
    return s;
}

// Stage 1: the object's pixels among the 4 x 4 around (fx, fy), no normal test.
RT_UP_HD inline UpsampleSums upsample_search(const UpsampleArgs &a, float idp, int ix, int iy, double fx, double fy)
{
    UpsampleSums s{0.0, 0.0, 0.0, 0.0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int ta = -1; ta <= 2; ++ta) {
        const int qx = ix + ta;
        if (qx < 0 || qx >= a.wl) continue;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int tb = -1; tb <= 2; ++tb) {
            const int qy = iy + tb;
            if (qy < 0 || qy >= a.hl) continue;
            const long long eq = (long long)qx * a.hl + qy;
            if (a.lo_guides[7 * a.lo_guide_stride + eq] != idp) continue;
            const double ex = (double)qx - fx, ey = (double)qy - fy;
            upsample_add(a, eq, 1.0 / (1.0 + (ex * ex + ey * ey)), a.demod != 0, s);
        }
    }
    return s;
}

// Output pixel (X, Y), written to out and, where given, kind.
RT_UP_HD inline void upsample_pixel(const UpsampleArgs &a, int X, int Y)
{
    const long long e = (long long)X * a.h + Y;
    const double sc = a.lo_px / a.hi_px;
    const double fx = upsample_clamp(upsample_snap((((double)X * a.hi_dy + a.hi_y0) * sc - a.lo_y0) / a.lo_dy), a.wl - 1);
    const double fy = upsample_clamp(upsample_snap((((double)Y * a.hi_dz + a.hi_z0) * sc - a.lo_z0) / a.lo_dz), a.hl - 1);
    const double flx = __builtin_floor(fx), fly = __builtin_floor(fy);
    const double ax = fx - flx, ay = fy - fly;
    const int ix = (int)flx, iy = (int)fly;                                           // 0 .. wl-1, 0 .. hl-1
    const float idp = a.hi_guides[7 * a.hi_guide_stride + e];
    float kind = 0.0f;
    bool demod = a.demod != 0;
    UpsampleSums s = upsample_bilinear<true>(a, e, idp, ix, iy, ax, ay);
    if (!(s.W > 0.0)) {
        kind = 1.0f;
        s = upsample_search(a, idp, ix, iy, fx, fy);
        if (!(s.W > 0.0)) {
            kind = 2.0f;
            demod = false;
            s = upsample_bilinear<false>(a, e, idp, ix, iy, ax, ay);
        }
    }
    double r0 = s.A0 / s.W, r1 = s.A1 / s.W, r2 = s.A2 / s.W;
    if (demod) {
        r0 = r0 * upsample_albedo(a.hi_guides[4 * a.hi_guide_stride + e]);
        r1 = r1 * upsample_albedo(a.hi_guides[5 * a.hi_guide_stride + e]);
        r2 = r2 * upsample_albedo(a.hi_guides[6 * a.hi_guide_stride + e]);
    }
    a.out[e] = r0; a.out[a.out_stride + e] = r1; a.out[2 * a.out_stride + e] = r2;
    if (a.kind) a.kind[e] = kind;
}

#if defined(__HIPCC__)

constexpr int UPSAMPLE_THREADS = 256;

// w*h <= RT_FILM_MAX_PIXELS = 2^27: pixel indices are 32-bit, plane offsets 64-bit
__global__ __launch_bounds__(UPSAMPLE_THREADS) void upsample_kernel(const UpsampleArgs a)
{
    const unsigned npx = (unsigned)a.w * (unsigned)a.h, step = gridDim.x * UPSAMPLE_THREADS;
    for (unsigned e = blockIdx.x * UPSAMPLE_THREADS + threadIdx.x; e < npx; e += step) {
        const unsigned x = e / (unsigned)a.h;
        upsample_pixel(a, (int)x, (int)(e - x * (unsigned)a.h));
    }
}

// blocks of an upsample launch over npx output pixels: at most 8 per CU, as the film, denoise and temporal kernels'
inline unsigned upsample_grid(long long npx, int cu_count)
{
    const long long want = (npx + UPSAMPLE_THREADS - 1) / UPSAMPLE_THREADS, cap = (long long)cu_count * 8;
    const long long n = want < cap ? want : cap;
    return (unsigned)(n < 1 ? 1 : n);
}

#endif  // __HIPCC__

}  // namespace rt
