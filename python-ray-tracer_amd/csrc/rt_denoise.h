// rt_denoise.h — the film's edge-stopping a-trous filter (include/mi355rt.h: rt_film_denoise): `levels` iterations of a 5x5 B3-spline
// kernel whose taps are 2^i pixels apart, on the mean of a film sum, each tap weighted by whether it shows the same object as the
// centre (the guides' id), by how far its normal turns away (a power of the cosine, by exact squarings) and by how far its colour
// is from the centre's (a rational weight, no exp()).
// The arithmetic of one pixel of one level (denoise_pixel and what it calls) is HIP-free, like rt_film.h and for the same reason: the
// kernel below and tests/algo/denoise_check.cpp, a CPU program built under AddressSanitizer and UBSan, compile the same text.
// Everything here is float64 without fused multiply-add (the Makefile's -ffp-contract=off; the CPU program's too), in the header's
// order.  The kernel (hipcc only): one thread per pixel, consecutive threads consecutive y (the fast axis of the layout), a grid
// capped near 8 blocks per CU with a grid-stride loop; the 25 taps are gathered through the caches with the centre pixel's guides
// and colour in registers; 8- and 4-byte accesses, so any plane stride will do; no LDS, no scratch, 64-bit plane offsets.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RT_DN_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define RT_DN_HD
#endif

namespace rt {

// One level of the filter over a ws x h frame: src is the film sum (first) or the level before, dst the level's result.
struct DenoiseArgs {
    const double *src;
    const float *guides;
    double *dst;
    long long src_stride, guide_stride, dst_stride;
    int ws, h;
    int step;        // 2^i: pixels between taps
    int nsq;         // log2(normal_shin): squarings of the normal's cosine
    int first;       // src is the sum: a tap's colour is s / n, over its albedo with demod
    int last;        // with demod: the result is multiplied by the pixel's albedo
    int demod;
    int copy;        // levels == 0: dst = src / n and nothing else
    double n;        // (double)n
    double q;        // sigma / 2^i, or 0: no colour weight
};

// The plan of the levels, shared by rt_film_denoise and the CPU program: level i of `levels` (levels == 0: the one level i = 0 that
// writes the mean) reads the sum or the level before and writes d_out when an even number of levels follow it, else d_work, so
// that the last level ends in d_out.
RT_DN_HD inline bool denoise_to_out(int levels, int i) { return levels == 0 || ((levels - 1 - i) & 1) == 0; }

RT_DN_HD inline void denoise_level(DenoiseArgs &a, int levels, int i, double sigma)
{
    a.step = 1 << i;
    a.first = i == 0; a.last = i == levels - 1; a.copy = levels == 0;
    a.q = sigma / (double)(1 << i);                                // a power of two: exact
}

// the B3 spline (1/16, 1/4, 3/8, 1/4, 1/16) at i = d + 2
RT_DN_HD inline double denoise_k(int i) { return i == 2 ? 0.375 : ((i == 1 || i == 3) ? 0.25 : 0.0625); }

// a[c][p] = max((double)albedo_c[p], 1.0)
RT_DN_HD inline double denoise_albedo(float a)
{
    const double v = (double)a;
    return v > 1.0 ? v : 1.0;
}

// m_i[c] of element e: the level before, or on the first level s / n (over the albedo with demod)
RT_DN_HD inline double denoise_value(const DenoiseArgs &a, int c, long long e)
{
    double v = a.src[c * a.src_stride + e];
    if (a.first) {
        v = v / a.n;
        if (a.demod) v = v / denoise_albedo(a.guides[(4 + c) * a.guide_stride + e]);
    }
    return v;
}

// Pixel (x, y) of one level, written to dst.
RT_DN_HD inline void denoise_pixel(const DenoiseArgs &a, int x, int y)
{
    const long long e = (long long)x * a.h + y;
    if (a.copy) {
        for (int c = 0; c < 3; ++c) a.dst[c * a.dst_stride + e] = a.src[c * a.src_stride + e] / a.n;
        return;
    }
    const float idp = a.guides[7 * a.guide_stride + e];
    const bool surface = idp >= 0.0f;
    const double nx = (double)a.guides[e], ny = (double)a.guides[a.guide_stride + e], nz = (double)a.guides[2 * a.guide_stride + e];
    const double mp0 = denoise_value(a, 0, e), mp1 = denoise_value(a, 1, e), mp2 = denoise_value(a, 2, e);
    double W = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0;
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
            if (a.guides[7 * a.guide_stride + eq] != idp) continue;
            double cn = 1.0;
            if (surface) {
                cn = ((nx * (double)a.guides[eq]) + (ny * (double)a.guides[a.guide_stride + eq])) + (nz * (double)a.guides[2 * a.guide_stride + eq]);
                if (!(cn > 0.0)) continue;
                for (int i = 0; i < a.nsq; ++i) cn = cn * cn;
            }
            const double mq0 = denoise_value(a, 0, eq), mq1 = denoise_value(a, 1, eq), mq2 = denoise_value(a, 2, eq);
            double wc = 1.0;
            if (a.q > 0.0) {
                const double e0 = (mq0 - mp0) / a.q, e1 = (mq1 - mp1) / a.q, e2 = (mq2 - mp2) / a.q;
                const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                wc = 1.0 / (1.0 + d2);
            }
            const double w = ((denoise_k(dx + 2) * denoise_k(dy + 2)) * cn) * wc;
            W = W + w;
            A0 = A0 + w * mq0; A1 = A1 + w * mq1; A2 = A2 + w * mq2;
        }
    }
    double r0 = A0 / W, r1 = A1 / W, r2 = A2 / W;
    if (a.last && a.demod) {
        r0 = r0 * denoise_albedo(a.guides[4 * a.guide_stride + e]);
        r1 = r1 * denoise_albedo(a.guides[5 * a.guide_stride + e]);
        r2 = r2 * denoise_albedo(a.guides[6 * a.guide_stride + e]);
    }
    a.dst[e] = r0; a.dst[a.dst_stride + e] = r1; a.dst[2 * a.dst_stride + e] = r2;
}

#if defined(__HIPCC__)

constexpr int DENOISE_THREADS = 256;

// ws*h <= RT_FILM_MAX_PIXELS = 2^27: pixel indices are 32-bit, plane offsets 64-bit
__global__ __launch_bounds__(DENOISE_THREADS) void denoise_kernel(const DenoiseArgs a)
{
    const unsigned npx = (unsigned)a.ws * (unsigned)a.h, step = gridDim.x * DENOISE_THREADS;
    for (unsigned e = blockIdx.x * DENOISE_THREADS + threadIdx.x; e < npx; e += step) {
        const unsigned x = e / (unsigned)a.h;
        denoise_pixel(a, (int)x, (int)(e - x * (unsigned)a.h));
    }
}

// blocks of a denoise launch over npx pixels: at most 8 per CU, as the film kernels'
inline unsigned denoise_grid(long long npx, int cu_count)
{
    const long long want = (npx + DENOISE_THREADS - 1) / DENOISE_THREADS, cap = (long long)cu_count * 8;
    const long long n = want < cap ? want : cap;
    return (unsigned)(n < 1 ? 1 : n);
}

#endif  // __HIPCC__

}  // namespace rt
