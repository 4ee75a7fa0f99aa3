// rt_meter.h — the film's meter (include/mi355rt.h: rt_film_meter, rt_film_meter_solve): a histogram of the luminance of a film's mean
// over bins that come from the bits of a float64 (eight per octave over 2^-16 .. 2^24, no log()), and the exposure that maps a
// percentile of it to a key value, adapted from the exposure before.  rt_film_resolve_metered (rt_film.h) multiplies it in.
// The arithmetic of one pixel (meter_luminance, meter_bin, meter_edge), the serial solve (meter_solve) and the phases of the
// histogram kernel (meter_lds_clear, meter_count, meter_flush) are HIP-free, like rt_bloom.h and for the same reason: the kernels
// below and tests/algo/meter_check.cpp, a CPU program built under AddressSanitizer and UBSan, compile the same text.  Everything is
// float64 without fused multiply-add, in the header's order.
//   meter_hist_kernel   shaped like the film streams: 256 threads, film_grid capped at 2 blocks per CU with a grid-stride loop over
//                       groups of four pixels (16-byte loads where a plane's base allows, 8-byte ones where a caller's stride leaves
//                       it misaligned), a scalar tail for npx mod 4.  The first kernel here that combines values across a frame:
//                       uint32 counters in LDS, METER_COPIES private copies per workgroup (one per wave), atomicAdd on LDS; a barrier;
//                       the block's threads add the copies and issue one 64-bit global atomicAdd per non-zero bin.  Counts are
//                       integers: the result does not depend on the order in which lanes or workgroups arrive.  No scratch.
//   meter_solve_kernel  one workgroup: its threads stage the counts in LDS, thread 0 runs meter_solve on them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/mi355rt.h"
#include "rt_film.h"

#if defined(__HIPCC__)
#define RT_MT_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define RT_MT_HD
#endif

namespace rt {

constexpr int METER_LO = -16, METER_OCTAVES = 40, METER_SUB = 8;        // RT_METER_LO, RT_METER_OCTAVES, RT_METER_SUB
constexpr int METER_BINS = METER_OCTAVES * METER_SUB + 3;               // RT_METER_BINS: nothing, below, the octaves, above
constexpr int METER_STATE_DOUBLES = 4;                                  // RT_METER_STATE_DOUBLES
constexpr int METER_K0 = (1023 + METER_LO) * METER_SUB;                 // 8056: the exponent and three mantissa bits of 2^METER_LO
static_assert(METER_SUB == 8, "a bin is the exponent and the top three mantissa bits: u >> 49");
static_assert(METER_LO == RT_METER_LO && METER_OCTAVES == RT_METER_OCTAVES && METER_SUB == RT_METER_SUB && METER_BINS == RT_METER_BINS &&
              METER_STATE_DOUBLES == RT_METER_STATE_DOUBLES && METER_BINS == 323 && METER_K0 == 8056, "rt_meter.h restates the header's constants");

constexpr int METER_THREADS = 256;

// Private copies of the counters in a workgroup's LDS: thread t counts into copy t / (METER_THREADS / METER_COPIES).  4 is one per
// wave.  Measured (tools/meter_bench.py, profiles/meter_bench.json, DESIGN.md: Metering): builds with -DRT_METER_COPIES=1, 4 and 8 on
// rendered films and on a constant frame, where every lane hits one counter.  The constant frame is not slower than a rendered film
// with any of the three (x0.66 to x0.97 of it), and the three builds differ by less than the rounds' spread: the starting point stays.
#ifndef RT_METER_COPIES
#define RT_METER_COPIES 4
#endif
constexpr int METER_COPIES = RT_METER_COPIES;
static_assert(METER_COPIES >= 1 && METER_COPIES <= METER_THREADS && METER_THREADS % METER_COPIES == 0, "whole groups of threads share a copy");
constexpr int METER_LDS_WORDS = METER_COPIES * METER_BINS;
constexpr size_t METER_LDS_BYTES = (size_t)METER_LDS_WORDS * sizeof(uint32_t);

RT_MT_HD inline double meter_luminance(double m0, double m1, double m2) { return (0.2126 * m0 + 0.7152 * m1) + 0.0722 * m2; }

RT_MT_HD inline uint64_t meter_bits(double y)
{
    uint64_t u;
    memcpy(&u, &y, sizeof u);
    return u;
}

// The bin of a luminance: 0 for what has none (zero, negative, NaN), 1 below 2^-16, 322 at or above 2^24 (+Inf included).
RT_MT_HD inline int meter_bin(double y)
{
    if (!(y > 0.0)) return 0;
    const int64_t k = (int64_t)(meter_bits(y) >> 49) - METER_K0;
    return k < 0 ? 1 : (k >= METER_OCTAVES * METER_SUB ? METER_BINS - 1 : 2 + (int)k);
}

// The lower edge of bin b (2 <= b <= 322): (1 + j/8) * 2^E, exact.
RT_MT_HD inline double meter_edge(int b)
{
    const uint64_t u = (uint64_t)(b - 2 + METER_K0) << 49;
    double y;
    memcpy(&y, &u, sizeof y);
    return y;
}

RT_MT_HD inline double meter_clamp(double v, const rt_meter &mt)
{
    return v < mt.min_exposure ? mt.min_exposure : (v > mt.max_exposure ? mt.max_exposure : v);
}

// The header's solve, serially.  Both walks over the counts have a fixed trip count (b is one more than the number of bins whose
// running count is at most r: the running count never falls), so the loads do not wait for one another.
RT_MT_HD inline void meter_solve(const uint64_t *hist, const rt_meter &mt, double *state)
{
    uint64_t N = 0;
    for (int i = 1; i < METER_BINS; ++i) N += hist[i];
    const double prev = state[0];
    const bool usable = film_exposure_usable(prev);
    if (N == 0) {
        state[0] = usable ? prev : meter_clamp(1.0, mt);
        state[1] = 0.0; state[2] = 0.0; state[3] = 0.0;
        return;
    }
    uint64_t r = (uint64_t)(mt.percentile * (double)N);
    if (r > N - 1) r = N - 1;
    int b = 1;
    uint64_t C = 0, below = 0;
    for (int i = 1; i < METER_BINS - 1; ++i) {          // (C_322 = N > r: bin 322 is never counted as "at most r")
        C += hist[i];
        if (C <= r) { b = i + 1; below = C; }
    }
    double Ym;
    if (b == 1) Ym = meter_edge(2);
    else if (b == METER_BINS - 1) Ym = meter_edge(METER_BINS - 1);
    else {
        const double lo = meter_edge(b), hi = meter_edge(b + 1);
        Ym = lo + (hi - lo) * ((double)(r - below) / (double)hist[b]);
    }
    const double t = meter_clamp(mt.key / Ym, mt);
    state[0] = (usable && mt.rate < 1.0) ? meter_clamp(prev + (t - prev) * mt.rate, mt) : t;
    state[1] = Ym; state[2] = (double)N; state[3] = (double)b;
}

struct MeterHistArgs {
    const double *sum;
    unsigned long long *hist;
    long long sum_stride, npx;
    double n;            // (double)n
};

// One count into a workgroup's LDS: an atomic on the device, where the threads of a copy run at once.
RT_MT_HD inline void meter_lds_add(uint32_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, 1u);
#else
    *p += 1u;
#endif
}

RT_MT_HD inline void meter_hist_add(unsigned long long *p, unsigned long long v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

// four consecutive doubles (rt_film.h: film_load4 on the device; the CPU program reads them one by one)
RT_MT_HD inline void meter_load4(const double *p, bool vec, double (&v)[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
    film_load4(p, vec, v);
#else
    (void)vec;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
#endif
}

RT_MT_HD inline bool meter_aligned16(const void *p) { return ((unsigned long long)(uintptr_t)p & 15) == 0; }

RT_MT_HD inline void meter_count_pixel(uint32_t *copy, double s0, double s1, double s2, double n)
{
    meter_lds_add(copy + meter_bin(meter_luminance(s0 / n, s1 / n, s2 / n)));
}

// The kernel's phases for thread `tid` of `nthreads` of workgroup `block` of `nblocks`; lds is METER_LDS_WORDS uint32.  A barrier
// stands between the phases.
RT_MT_HD inline void meter_lds_clear(uint32_t *lds, int tid, int nthreads)
{
    for (int i = tid; i < METER_LDS_WORDS; i += nthreads) lds[i] = 0u;
}

// count: the thread's groups of four pixels in a grid-stride loop, and for the first npx mod 4 threads of workgroup 0 the pixels
// behind the last group, into the thread's copy.  A workgroup counts at most 2^27 pixels: a uint32 counter cannot overflow.
RT_MT_HD inline void meter_count(const MeterHistArgs &a, uint32_t *lds, int tid, int nthreads, long long block, long long nblocks)
{
    uint32_t *const copy = lds + (tid / (nthreads / METER_COPIES)) * METER_BINS;
    const double *const s0 = a.sum, *const s1 = a.sum + a.sum_stride, *const s2 = a.sum + 2 * a.sum_stride;
    const bool v0 = meter_aligned16(s0), v1 = meter_aligned16(s1), v2 = meter_aligned16(s2);
    const long long ngroups = a.npx >> 2, step = nblocks * nthreads;
    for (long long g = block * nthreads + tid; g < ngroups; g += step) {
        const long long e = g << 2;
        double R[4], G[4], B[4];
        meter_load4(s0 + e, v0, R);
        meter_load4(s1 + e, v1, G);
        meter_load4(s2 + e, v2, B);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 4; ++i) meter_count_pixel(copy, R[i], G[i], B[i], a.n);
    }
    if (block == 0 && (long long)tid < (a.npx & 3)) {
        const long long e = (ngroups << 2) + tid;
        meter_count_pixel(copy, s0[e], s1[e], s2[e], a.n);
    }
}

// flush: thread t adds the copies of bins t, t + nthreads, ... and adds what is not zero to the counts in memory.
RT_MT_HD inline void meter_flush(const MeterHistArgs &a, const uint32_t *lds, int tid, int nthreads)
{
    for (int b = tid; b < METER_BINS; b += nthreads) {
        uint32_t c = 0u;
        for (int k = 0; k < METER_COPIES; ++k) c += lds[k * METER_BINS + b];
        if (c) meter_hist_add(a.hist + b, (unsigned long long)c);
    }
}

#if defined(__HIPCC__)

// Workgroups per CU at the grid's cap.  Every workgroup ends with up to one global atomic per bin, so fewer, longer-running workgroups
// pay fewer of them; more of them hide more of the loads' latency.  A measurement (tools/meter_bench.py --lib on builds with 8, 4, 2
// and 1, profiles/meter_bench.json, DESIGN.md: Metering): at film_grid's own 8 a 1080p film's 2 025 workgroups of 1 024 pixels each
// end with some 160 atomics each and the call takes 0.047 ms; at 2 it takes 0.020 ms, at 2160p 0.039 against 0.058 ms, at 4320p 0.144
// against 0.153 ms; at 1 the 4320p frame is the slowest of the four (0.159 ms).  So 2.
#ifndef RT_METER_BLOCKS_PER_CU
#define RT_METER_BLOCKS_PER_CU 2
#endif
static_assert(RT_METER_BLOCKS_PER_CU == 1 || RT_METER_BLOCKS_PER_CU == 2 || RT_METER_BLOCKS_PER_CU == 4 || RT_METER_BLOCKS_PER_CU == 8, "a divisor of film_grid's 8");
inline unsigned meter_grid(long long groups, int cu_count) { return film_grid(groups, cu_count, 8 / RT_METER_BLOCKS_PER_CU); }

__global__ __launch_bounds__(METER_THREADS) void meter_hist_kernel(const MeterHistArgs a)
{
    __shared__ uint32_t lds[METER_LDS_WORDS];
    const int tid = (int)threadIdx.x;
    meter_lds_clear(lds, tid, METER_THREADS);
    __syncthreads();
    meter_count(a, lds, tid, METER_THREADS, (long long)blockIdx.x, (long long)gridDim.x);
    __syncthreads();
    meter_flush(a, lds, tid, METER_THREADS);
}

// reset: the counts to zero, on the stream, before the histogram kernel
__global__ __launch_bounds__(METER_THREADS) void meter_clear_kernel(unsigned long long *hist)
{
    for (int b = (int)threadIdx.x; b < METER_BINS; b += METER_THREADS) hist[b] = 0ull;
}

constexpr int METER_SOLVE_THREADS = 64;

// The launch is this kernel's cost: one wave stages the 323 counts in LDS (six loads per lane, in flight together), lane 0 solves.
__global__ __launch_bounds__(METER_SOLVE_THREADS) void meter_solve_kernel(const unsigned long long *hist, const rt_meter mt, double *state)
{
    __shared__ uint64_t counts[METER_BINS];
    for (int b = (int)threadIdx.x; b < METER_BINS; b += METER_SOLVE_THREADS) counts[b] = hist[b];
    __syncthreads();
    if (threadIdx.x == 0) meter_solve(counts, mt, state);
}

#endif  // __HIPCC__

}  // namespace rt
