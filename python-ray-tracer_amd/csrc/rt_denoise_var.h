// rt_denoise_var.h — the film's variance-guided a-trous filter (include/mi355rt.h: rt_film_denoise_variance): rt_denoise.h's filter
// with the colour tolerance of every pixel taken from the estimated variance of its mean instead of one global sigma.  A prepare
// pass forms the mean m_0 (three planes) and the variance of the mean v_0 (a fourth plane) from the film's sum and sum of squares;
// each level then filters the four planes: the colour weight of a tap is 1 / (1 + d2 / (kappa^2 vp + var_floor)) with vp the pixel's
// variance (3x3-smoothed within its object when prefilter is set), and the variance is carried on as sum(w^2 v) / (sum w)^2.
// The arithmetic of one pixel (denoise_var_prepare_pixel, denoise_var_pixel and what they call) and the plan of the levels are HIP-free,
// like rt_denoise.h and for the same reason: the kernels below and tests/algo/variance_check.cpp, a CPU program built under
// AddressSanitizer and UBSan, compile the same text.  Everything here is float64 without fused multiply-add, in the header's order; no
// exp(), pow() or sqrt.  The kernels (hipcc only) are shaped like denoise_kernel: one thread per pixel, consecutive threads consecutive
// y, a grid capped near 8 blocks per CU with a grid-stride loop, one launch per level, taps gathered through the caches; 8- and 4-byte
// accesses, so any plane stride will do; no LDS, no scratch, 64-bit plane offsets.
// rt_film_denoise_variance_temporal filters what rt_film_temporal_moments wrote (a mean, a mean of squares and a length per pixel) and
// only its prepare pass is new (denoise_var_prepare_len_pixel, denoise_var_prepare_len_kernel, with the argument struct DenoiseVarLenArgs
// of their own): a pixel whose length reaches spatial_below takes the variance of its own moments, a shorter one pools the moments of
// the 5x5 pixels of its object around it.  Only lanes whose length is short walk the 25 taps; a wave with one such lane pays the whole
// loop once (25 iterations of an id load, a length load and, where both pass, six 8-byte loads, executed for the short lanes with the
// others masked off), a wave without one pays the compare and a branch.  The levels are denoise_var_kernel's, unchanged.
#pragma once
#include <cstdint>

#include "rt_denoise.h"

namespace rt {

constexpr int DENOISE_VAR_PLANES = 4;   // RT_DENOISE_VAR_PLANES: the mean's three planes and the variance

// One launch over a ws x h frame: the prepare pass (sum, sq -> dst) or one level (src -> dst); dst and src have four planes.
struct DenoiseVarArgs {
    const double *sum, *sq;      // the prepare pass's inputs
    const double *src;           // a level's input: (m_i, v_i)
    const float *guides;
    double *dst;
    long long sum_stride, sq_stride, src_stride, guide_stride, dst_stride;
    int ws, h;
    int step;        // 2^i: pixels between taps
    int nsq;         // log2(normal_shin): squarings of the normal's cosine
    int last;        // with demod: the result is multiplied by the pixel's albedo
    int demod;
    int prefilter;
    int copy;        // levels == 0: dst = (sum / n, v_0 without demodulation) and nothing else
    double n, n1;    // (double)n, (double)(n - 1)
    double k2;       // kappa * kappa
    double var_floor;
};

// The plan, shared by rt_film_denoise_variance and the CPU program: write k of levels + 1 (k = 0 the prepare pass, k = i + 1 level i)
// goes to d_out when an even number of writes follow it, else to d_work, so that the last one ends in d_out.
RT_DN_HD inline bool denoise_var_to_out(int levels, int k) { return ((levels - k) & 1) == 0; }

RT_DN_HD inline void denoise_var_level(DenoiseVarArgs &a, int levels, int i)
{
    a.step = 1 << i;
    a.last = i == levels - 1;
}

// the 3x3 smoothing kernel (1/4, 1/2, 1/4) at i = d + 1
RT_DN_HD inline double denoise_var_g(int i) { return i == 1 ? 0.5 : 0.25; }

// r > 0 ? r : 0 (NaN: 0)
RT_DN_HD inline double denoise_var_pos(double r) { return r > 0.0 ? r : 0.0; }

// The colour weight of a tap at squared colour distance d2 under the tolerance den.
RT_DN_HD inline double denoise_var_wc(double d2, double den)
{
    if (den > 0.0) return 1.0 / (1.0 + d2 / den);
    return d2 > 0.0 ? 0.0 : 1.0;
}

// The end of both prepare passes for channel c of element e: the mean m over the albedo and the variance over its square with demod,
// the mean stored; returns the variance, of which the caller stores v_0 = (var_0 + var_1) + var_2.  Per channel, as both passes
// interleave it with their loads: one call for the three channels made denoise_var_prepare_kernel hold every load at once.
RT_DN_HD inline double denoise_var_prepare_store(const float *guides, long long guide_stride, double *dst, long long dst_stride,
                                                 int c, long long e, bool demod, double m, double var)
{
    if (demod) {
        const double al = denoise_albedo(guides[(4 + c) * guide_stride + e]);
        m = m / al;
        var = var / (al * al);
    }
    dst[c * dst_stride + e] = m;
    return var;
}

// Element e of the prepare pass: (m_0, v_0) from the sum and the sum of squares, over the albedo with demod.
RT_DN_HD inline void denoise_var_prepare_pixel(const DenoiseVarArgs &a, long long e)
{
    const bool demod = a.demod && !a.copy;
    double v[3];
    for (int c = 0; c < 3; ++c) {
        const double m = a.sum[c * a.sum_stride + e] / a.n;
        const double r = denoise_var_pos(a.sq[c * a.sq_stride + e] / a.n - m * m);
        v[c] = denoise_var_prepare_store(a.guides, a.guide_stride, a.dst, a.dst_stride, c, e, demod, m, r / a.n1);
    }
    a.dst[3 * a.dst_stride + e] = (v[0] + v[1]) + v[2];
}

// The prepare pass of rt_film_denoise_variance_temporal over a ws x h frame: (mean, msq, len) -> dst, four planes.
struct DenoiseVarLenArgs {
    const double *mean, *msq;    // the temporal mean and mean of squares, three planes each
    const float *len;            // the length plane
    const float *guides;
    double *dst;
    long long mean_stride, msq_stride, guide_stride, dst_stride;
    int ws, h;
    int demod;
    int copy;                    // levels == 0: dst = (mean, v_0 without demodulation)
    double spatial_below;
};

// Pixel (x, y) of that prepare pass: (m_0, v_0) from the pixel's own moments where its length reaches spatial_below, else from the
// moments of its object's pixels in the 5x5 window, weighted by their lengths.
RT_DN_HD inline void denoise_var_prepare_len_pixel(const DenoiseVarLenArgs &a, int x, int y)
{
    const long long e = (long long)x * a.h + y;
    const bool demod = a.demod && !a.copy;
    const double Lp = (double)a.len[e];
    const double m[3] = {a.mean[e], a.mean[a.mean_stride + e], a.mean[2 * a.mean_stride + e]};
    double var[3] = {0.0, 0.0, 0.0};
    if (Lp >= a.spatial_below) {                                                      // own
        for (int c = 0; c < 3; ++c) {
            const double r = denoise_var_pos(a.msq[c * a.msq_stride + e] - m[c] * m[c]);
            var[c] = Lp > 1.0 ? r / (Lp - 1.0) : 0.0;
        }
    } else {                                                                          // pooled (a NaN length lands here)
        const float *const ids = a.guides + 7 * a.guide_stride;
        const float idp = ids[e];
        double SL = 0.0, M[3] = {0.0, 0.0, 0.0}, Q[3] = {0.0, 0.0, 0.0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= a.ws) continue;
            for (int dy = -2; dy <= 2; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= a.h) continue;
                const long long eq = (long long)qx * a.h + qy;
                if (ids[eq] != idp) continue;
                const double lq = (double)a.len[eq];
                if (!(lq > 0.0)) continue;
                SL = SL + lq;
                for (int c = 0; c < 3; ++c) {
                    M[c] = M[c] + lq * a.mean[c * a.mean_stride + eq];
                    Q[c] = Q[c] + lq * a.msq[c * a.msq_stride + eq];
                }
            }
        }
        if (SL > 1.0 && Lp > 0.0)
            for (int c = 0; c < 3; ++c) {
                const double pm = M[c] / SL;
                const double r = denoise_var_pos(Q[c] / SL - pm * pm);
                var[c] = (r / (SL - 1.0)) * (SL / Lp);
            }
    }
    for (int c = 0; c < 3; ++c) var[c] = denoise_var_prepare_store(a.guides, a.guide_stride, a.dst, a.dst_stride, c, e, demod, m[c], var[c]);
    a.dst[3 * a.dst_stride + e] = (var[0] + var[1]) + var[2];
}

// Pixel (x, y) of one level, written to dst.
RT_DN_HD inline void denoise_var_pixel(const DenoiseVarArgs &a, int x, int y)
{
    const long long e = (long long)x * a.h + y;
    const float *const ids = a.guides + 7 * a.guide_stride;
    const double *const m0 = a.src, *const m1 = a.src + a.src_stride, *const m2 = a.src + 2 * a.src_stride, *const var = a.src + 3 * a.src_stride;
    const float idp = ids[e];
    const bool surface = idp >= 0.0f;
    double vp = var[e];
    if (a.prefilter) {
        double gw = 0.0, gv = 0.0;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= a.ws) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= a.h) continue;
                const long long eq = (long long)qx * a.h + qy;
                if (ids[eq] != idp) continue;
                const double t = denoise_var_g(dx + 1) * denoise_var_g(dy + 1);
                gw = gw + t;
                gv = gv + t * var[eq];
            }
        }
        vp = gv / gw;
    }
    const double den = a.k2 * vp + a.var_floor;
    const double nx = (double)a.guides[e], ny = (double)a.guides[a.guide_stride + e], nz = (double)a.guides[2 * a.guide_stride + e];
    const double mp0 = m0[e], mp1 = m1[e], mp2 = m2[e];
    double W = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0, V = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int dx = -2; dx <= 2; ++dx) {
        const int qx = x + a.step * dx;
        if (qx < 0 || qx >= a.ws) continue;
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + a.step * dy;
            if (qy < 0 || qy >= a.h) continue;
            const long long eq = (long long)qx * a.h + qy;
            if (ids[eq] != idp) continue;
            double cn = 1.0;
            if (surface) {
                cn = ((nx * (double)a.guides[eq]) + (ny * (double)a.guides[a.guide_stride + eq])) + (nz * (double)a.guides[2 * a.guide_stride + eq]);
                if (!(cn > 0.0)) continue;
                for (int i = 0; i < a.nsq; ++i) cn = cn * cn;
            }
            const double mq0 = m0[eq], mq1 = m1[eq], mq2 = m2[eq];
            const double e0 = mq0 - mp0, e1 = mq1 - mp1, e2 = mq2 - mp2;
            const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
            const double w = ((denoise_k(dx + 2) * denoise_k(dy + 2)) * cn) * denoise_var_wc(d2, den);
            W = W + w;
            A0 = A0 + w * mq0; A1 = A1 + w * mq1; A2 = A2 + w * mq2;
            V = V + (w * w) * var[eq];
        }
    }
    double r0 = A0 / W, r1 = A1 / W, r2 = A2 / W;
    if (a.last && a.demod) {
        r0 = r0 * denoise_albedo(a.guides[4 * a.guide_stride + e]);
        r1 = r1 * denoise_albedo(a.guides[5 * a.guide_stride + e]);
        r2 = r2 * denoise_albedo(a.guides[6 * a.guide_stride + e]);
    }
    a.dst[e] = r0; a.dst[a.dst_stride + e] = r1; a.dst[2 * a.dst_stride + e] = r2;
    a.dst[3 * a.dst_stride + e] = V / (W * W);
}

#if defined(__HIPCC__)

// ws*h <= RT_FILM_MAX_PIXELS = 2^27: pixel indices are 32-bit, plane offsets 64-bit
__global__ __launch_bounds__(DENOISE_THREADS) void denoise_var_prepare_kernel(const DenoiseVarArgs a)
{
    const unsigned npx = (unsigned)a.ws * (unsigned)a.h, step = gridDim.x * DENOISE_THREADS;
    for (unsigned e = blockIdx.x * DENOISE_THREADS + threadIdx.x; e < npx; e += step) denoise_var_prepare_pixel(a, (long long)e);
}

__global__ __launch_bounds__(DENOISE_THREADS) void denoise_var_prepare_len_kernel(const DenoiseVarLenArgs a)
{
    const unsigned npx = (unsigned)a.ws * (unsigned)a.h, step = gridDim.x * DENOISE_THREADS;
    for (unsigned e = blockIdx.x * DENOISE_THREADS + threadIdx.x; e < npx; e += step) {
        const unsigned x = e / (unsigned)a.h;
        denoise_var_prepare_len_pixel(a, (int)x, (int)(e - x * (unsigned)a.h));
    }
}

__global__ __launch_bounds__(DENOISE_THREADS) void denoise_var_kernel(const DenoiseVarArgs a)
{
    const unsigned npx = (unsigned)a.ws * (unsigned)a.h, step = gridDim.x * DENOISE_THREADS;
    for (unsigned e = blockIdx.x * DENOISE_THREADS + threadIdx.x; e < npx; e += step) {
        const unsigned x = e / (unsigned)a.h;
        denoise_var_pixel(a, (int)x, (int)(e - x * (unsigned)a.h));
    }
}

#endif  // __HIPCC__

}  // namespace rt
