// rt_film.h — the film (include/mi355rt.h: rt_film_accumulate, rt_film_accumulate_moments, rt_film_resolve, rt_film_resolve_metered): a
// float64 sum of float32 pass frames in device memory (with the moments entry a float64 sum of their squares beside it), and its
// resolve to a frame (mean, exposure, with the metered entry times the exposure a meter solved on the device, highlight compression,
// display gamma, bytes).
// The arithmetic of one element (film_add, film_add_sq, film_tone, film_clip) is HIP-free, like rt_plan.h and rt_scene.h and for the same
// reason: the kernels below and tests/algo/film_check.cpp and variance_check.cpp, CPU programs built under AddressSanitizer and UBSan,
// compile the same text.  Everything here is evaluated without fused multiply-add (the Makefile's -ffp-contract=off; the CPU program's too).
// The kernels (hipcc only) are memory-bound streams: 16-byte accesses per lane on planes whose base is 16-byte aligned, 8-, 4-
// or 1-byte accesses on planes whose base is not (a caller's plane stride may be odd), a scalar tail for the last npx mod 4
// elements, a grid capped near 8 blocks per CU with a grid-stride loop, no LDS, no scratch, 64-bit plane offsets.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_FILM_HD __host__ __device__
#else
#define RT_FILM_HD
#endif

namespace rt {

// One pass's float32 colour onto the float64 sum.
RT_FILM_HD inline double film_add(double s, float f) { return s + (double)f; }

// One pass's float32 colour, squared, onto the float64 sum of squares (rt_film_accumulate_moments).  The product of two widened
// float32 values is exact in float64: fusing it into the addition could not change the result.
RT_FILM_HD inline double film_add_sq(double q, float f)
{
    const double g = (double)f;
    return q + g * g;
}

// What a resolve evaluates once: n as a double, and the square of white / 255.
struct FilmTone {
    double n, exposure, white, wn2;
    int gamma;
};

RT_FILM_HD inline FilmTone film_tone_of(int64_t n, double exposure, double white, int gamma)
{
    FilmTone t;
    t.n = (double)n; t.exposure = exposure; t.white = white; t.gamma = gamma;
    const double wn = white / 255.0;
    t.wn2 = wn * wn;
    return t;
}

// The sum s of n passes to a display value: mean, exposure, the extended Reinhard curve per channel (white maps to 255), a square
// root for gamma 2.  The comparisons are false for a NaN, which passes through.
RT_FILM_HD inline double film_tone(double s, const FilmTone &t)
{
    double v = (s / t.n) * t.exposure;
    if (t.white > 0.0) {
        const double x = v / 255.0;
        if (x > 0.0) {
            const double y = (x * (1.0 + x / t.wn2)) / (1.0 + x);
            v = y * 255.0;
        }
    }
    if (t.gamma == 2) {
        const double q = v / 255.0;
        if (q > 0.0) v = __builtin_sqrt(q) * 255.0;
    }
    return v;
}

// rt_device.h's clip_color (common.py:52-57): NaN -> 0, round half to even, clamp to 0..255.
RT_FILM_HD inline uint8_t film_clip(double c)
{
    if (!(c == c)) return 0;
    if (c <= -0.5) return 0;
    if (c >= 255.5) return 255;
    const int i = (int)__builtin_rint(c);
    return (uint8_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
}

// rt_film_resolve_metered's exposure: the tone's own (the user's compensation) times the metered one x = state[0], or times 1.0
// where x is not (finite and > 0): a state that no solve has written yet.
RT_FILM_HD inline bool film_exposure_usable(double x) { return x > 0.0 && x <= 1.7976931348623157e308; }
RT_FILM_HD inline double film_metered_exposure(double exposure, double x) { return exposure * (film_exposure_usable(x) ? x : 1.0); }

constexpr int FILM_BATCH = 4;                       // passes one add kernel folds
constexpr size_t FILM_SCRATCH_MAX = 256u << 20;      // bytes of pass frames beyond which passes go one by one

// frames: `nb` (1..FILM_BATCH) float32 pass frames, pass b's plane c at frames[(b*3 + c) * fplane], fplane a multiple of 4 floats
// and frames 16-byte aligned (the library's own scratch): every pass plane is 16-byte aligned.
struct FilmAddArgs {
    double *sum;
    const float *frames;
    long long sum_stride, fplane, npx;
    int nb, reset;
};

// film_add2_kernel: FilmAddArgs with the sum of squares beside the sum; sum and sq are planes of their own stride and alignment
struct FilmAdd2Args {
    double *sum, *sq;
    const float *frames;
    long long sum_stride, sq_stride, fplane, npx;
    int nb, reset;
};

struct FilmResolveArgs {
    const double *sum;
    uint8_t *u8;
    float *f32;
    long long sum_stride, out_stride, npx;
    int h, rgb, hwc;
    FilmTone tone;
};

#if defined(__HIPCC__)

constexpr int FILM_THREADS = 256;

// 16 bytes per lane as the compiler's own vector types: one global_load / global_store _dwordx4 each
typedef double film_d2 __attribute__((ext_vector_type(2)));
typedef float film_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool film_aligned(const void *p, unsigned a) { return ((unsigned long long)p & (a - 1)) == 0; }

// four consecutive doubles: two 16-byte accesses where the plane allows (vec), else four of 8 bytes
__device__ __forceinline__ void film_load4(const double *p, bool vec, double (&v)[4])
{
    if (vec) {
        const film_d2 a = *reinterpret_cast<const film_d2 *>(p), b = *reinterpret_cast<const film_d2 *>(p + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}

__device__ __forceinline__ void film_store4(double *p, bool vec, const double (&v)[4])
{
    if (vec) {
        *reinterpret_cast<film_d2 *>(p) = film_d2{v[0], v[1]};
        *reinterpret_cast<film_d2 *>(p + 2) = film_d2{v[2], v[3]};
    } else {
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}

// sum[c][e] = (reset ? +0.0 : sum[c][e]) + f_0[c][e] + ... + f_{nb-1}[c][e], left to right, and with SQ (Args = FilmAdd2Args) the
// same of the squares into sq[c][e] beside it, each pass element read once for both; the sum's bits do not depend on SQ.
// blockIdx.y is the plane; a thread takes groups of four elements in a grid-stride loop, and the first npx mod 4 threads of block 0
// the elements behind the last group.  A sum plane and a sq plane may differ in alignment.
template <bool SQ, class Args>
__device__ __forceinline__ void film_add_body(const Args &a)
{
    const long long c = blockIdx.y;
    double *const s = a.sum + c * a.sum_stride;
    double *q = nullptr;
    if constexpr (SQ) q = a.sq + c * a.sq_stride;
    const float *const f = a.frames + c * a.fplane;
    const long long pass = 3 * a.fplane;
    const bool vec_s = film_aligned(s, 16), vec_q = SQ && film_aligned(q, 16);
    const long long ngroups = a.npx >> 2, step = (long long)gridDim.x * FILM_THREADS;
    for (long long g = (long long)blockIdx.x * FILM_THREADS + threadIdx.x; g < ngroups; g += step) {
        const long long e = g << 2;
        film_f4 v[FILM_BATCH];
#pragma unroll
        for (int b = 0; b < FILM_BATCH; ++b)
            if (b < a.nb) v[b] = *reinterpret_cast<const film_f4 *>(f + b * pass + e);
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
        if (!a.reset) {
            film_load4(s + e, vec_s, acc);
            if constexpr (SQ) film_load4(q + e, vec_q, sq);
        }
#pragma unroll
        for (int b = 0; b < FILM_BATCH; ++b)
            if (b < a.nb) {
                acc[0] = film_add(acc[0], v[b].x); acc[1] = film_add(acc[1], v[b].y);
                acc[2] = film_add(acc[2], v[b].z); acc[3] = film_add(acc[3], v[b].w);
                if constexpr (SQ) {
                    sq[0] = film_add_sq(sq[0], v[b].x); sq[1] = film_add_sq(sq[1], v[b].y);
                    sq[2] = film_add_sq(sq[2], v[b].z); sq[3] = film_add_sq(sq[3], v[b].w);
                }
            }
        film_store4(s + e, vec_s, acc);
        if constexpr (SQ) film_store4(q + e, vec_q, sq);
    }
    if (blockIdx.x == 0 && (long long)threadIdx.x < (a.npx & 3)) {
        const long long e = (ngroups << 2) + threadIdx.x;
        double acc = a.reset ? 0.0 : s[e], sq = 0.0;
        if constexpr (SQ) sq = a.reset ? 0.0 : q[e];
        for (int b = 0; b < a.nb; ++b) {
            const float x = f[b * pass + e];
            acc = film_add(acc, x);
            if constexpr (SQ) sq = film_add_sq(sq, x);
        }
        s[e] = acc;
        if constexpr (SQ) q[e] = sq;
    }
}

__global__ __launch_bounds__(FILM_THREADS) void film_add_kernel(const FilmAddArgs a) { film_add_body<false>(a); }
__global__ __launch_bounds__(FILM_THREADS) void film_add2_kernel(const FilmAdd2Args a) { film_add_body<true>(a); }

// One pixel's three bytes (the tail, and the image layout): e = (x - x0) h + y.
__device__ __forceinline__ void film_store_u8_pixel(const FilmResolveArgs &a, long long e, double R, double G, double B)
{
    const uint8_t r8 = film_clip(R), g8 = film_clip(G), b8 = film_clip(B);
    const uint8_t c1 = a.rgb ? g8 : b8, c2 = a.rgb ? b8 : g8;
    if (a.hwc) {
        const long long x = e / a.h, y = e - x * a.h;
        uint8_t *px = a.u8 + (y * a.out_stride + x) * 3;
        px[0] = r8; px[1] = c1; px[2] = c2;
    } else {
        a.u8[e] = r8;
        a.u8[a.out_stride + e] = c1;
        a.u8[2 * a.out_stride + e] = c2;
    }
}

__device__ __forceinline__ void film_store_f32x4(float *p, bool vec, const double (&v)[4])
{
    if (vec) *reinterpret_cast<film_f4 *>(p) = film_f4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    else { p[0] = (float)v[0]; p[1] = (float)v[1]; p[2] = (float)v[2]; p[3] = (float)v[3]; }
}

__device__ __forceinline__ void film_store_u8x4(uint8_t *p, bool vec, const double (&v)[4])
{
    const uint8_t b0 = film_clip(v[0]), b1 = film_clip(v[1]), b2 = film_clip(v[2]), b3 = film_clip(v[3]);
    if (vec) *reinterpret_cast<uint32_t *>(p) = (uint32_t)b0 | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16) | ((uint32_t)b3 << 24);
    else { p[0] = b0; p[1] = b1; p[2] = b2; p[3] = b3; }
}

// The resolve (rt_film_resolve.inc: the body of both kernels, as text).  film_resolve_metered_kernel (rt_film_resolve_metered) forms
// its exposure first: the tone's times state[0] (film_metered_exposure), one product formed once.  The state is read through a
// pointer to the constant address space, as the sky block is (rt_device.h: sky_color): the kernel never writes it and the address is
// a kernel argument, so the read is one scalar load and the product is formed on the scalar unit.
typedef __attribute__((address_space(4))) const double film_state_f64;

__global__ __launch_bounds__(FILM_THREADS) void film_resolve_kernel(const FilmResolveArgs a)
{
#include "rt_film_resolve.inc"
}

__global__ __launch_bounds__(FILM_THREADS) void film_resolve_metered_kernel(FilmResolveArgs a, const double *state)
{
    a.tone.exposure = film_metered_exposure(a.tone.exposure, *(film_state_f64 *)(size_t)state);
#include "rt_film_resolve.inc"
}

// blocks along x of a film kernel over `groups` groups of four elements: at most 8 per CU in all (`planes` rows of them)
inline unsigned film_grid(long long groups, int cu_count, int planes)
{
    const long long want = (groups + FILM_THREADS - 1) / FILM_THREADS, cap = (long long)cu_count * 8 / planes;
    const long long n = want < cap ? want : cap;
    return (unsigned)(n < 1 ? 1 : n);
}

#endif  // __HIPCC__

}  // namespace rt
