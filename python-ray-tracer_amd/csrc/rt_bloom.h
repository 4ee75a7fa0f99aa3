// rt_bloom.h — the film's bloom (include/mi355rt.h: rt_film_bloom): what is brighter than a threshold is scaled by its brightest
// channel (the glow keeps the pixel's hue), blurred by `levels` iterations of the separable B3-spline a-trous kernel the denoisers
// use, without any edge-stopping, and the mean of the levels times `strength` is added to the film's mean, in linear colour.
// The arithmetic of one element (bloom_bright, bloom_tap, bloom_x_pixel, bloom_y_pixel), the plan of the launches (bloom_plan) and
// the phases of the tile kernel (bloom_tile_load, _xpass, _ypass) are HIP-free, like rt_denoise.h and for the same reason: the kernels
// below and tests/algo/bloom_check.cpp, a CPU program built under AddressSanitizer and UBSan, compile the same text.  Everything is
// float64 without fused multiply-add, in the header's order.
// Two forms of one level, bit-identical:
//   gather  bloom_x_kernel (b_i -> t) and bloom_y_kernel (t -> b_{i+1}, out += wl * b_{i+1}): one thread per pixel, consecutive threads
//           consecutive y, a grid capped near 8 blocks per CU with a grid-stride loop, the 5 taps gathered through the caches; no LDS;
//   tile    bloom_tile_kernel: one workgroup per BLOOM_TX x BLOOM_TY tile and channel: the tile of b_i and a halo of 2*step
//           on every side staged in LDS, t formed in LDS for the tile's columns and the y halo, b_{i+1} and the out update from LDS.
//           t never goes to memory.  Lanes run along y in the loads, the LDS reads and writes and the stores: a wave's 8-byte LDS
//           accesses are consecutive addresses, which the LDS serves without a bank conflict for any row pitch.
// 8-byte accesses everywhere (a caller's stride may leave a plane only 8-byte aligned), 32-bit pixel indices, 64-bit plane offsets,
// every index range-checked before it is read, no scratch.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_BL_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define RT_BL_HD
#endif

namespace rt {

constexpr int BLOOM_MAX_LEVELS = 8;     // RT_BLOOM_MAX_LEVELS
constexpr int BLOOM_NO_TILES = 1;       // RT_BLOOM_NO_TILES

// The tile: BLOOM_TX columns (x, the slow axis) by BLOOM_TY rows (y, the fast axis: a wave covers one column's 64 rows).  The LDS
// of one workgroup holds one channel: b with its halo, (TX + 2H) x (TY + 2H), and t, TX x (TY + 2H), H = 2 * step, sized for the
// largest step the kernel is built for: 48 x 80 + 32 x 80 doubles = 51200 bytes, three workgroups (12 waves) per CU of 160 KiB.
constexpr int BLOOM_TX = 32, BLOOM_TY = 64;
constexpr int BLOOM_TILE_BUILT_STEP = 4;                       // the largest step bloom_tile_kernel is instantiated for
constexpr int BLOOM_TILE_HALO = 2 * BLOOM_TILE_BUILT_STEP;
constexpr int BLOOM_LDS_B = (BLOOM_TX + 2 * BLOOM_TILE_HALO) * (BLOOM_TY + 2 * BLOOM_TILE_HALO);
constexpr int BLOOM_LDS_T = BLOOM_TX * (BLOOM_TY + 2 * BLOOM_TILE_HALO);
constexpr int BLOOM_LDS_DOUBLES = BLOOM_LDS_B + BLOOM_LDS_T;
constexpr size_t BLOOM_LDS_BYTES = (size_t)BLOOM_LDS_DOUBLES * sizeof(double);

// The largest step (1, 2, 4; 0: none) whose level runs as a tile.  A measurement, not a guess (tools/bloom_bench.py --per-level,
// profiles/bloom_bench.json, DESIGN.md: Bloom): a tiled level costs x0.63 to x0.78 of a gathered one at steps 1, 2 and 4 on all three
// standing workloads, by far more than the rounds' spread (under 3 %), so 4, the largest step measured and built.  Larger steps are
// not measured: their halo (2 * step on every side of a 32 x 64 tile) would exceed the tile itself.
#ifndef RT_BLOOM_TILE_MAX_STEP
#define RT_BLOOM_TILE_MAX_STEP 4
#endif
constexpr int BLOOM_TILE_MAX_STEP = RT_BLOOM_TILE_MAX_STEP;
static_assert(BLOOM_TILE_MAX_STEP <= BLOOM_TILE_BUILT_STEP, "the tile kernel's LDS is sized for steps up to BLOOM_TILE_BUILT_STEP");

// One launch of a bloom call.  src and dst name work-plane sets (0: planes 0..2 of d_work, 1: planes 3..5; -1: none).
enum BloomKind { BLOOM_BRIGHT = 0, BLOOM_X = 1, BLOOM_Y = 2, BLOOM_TILE = 3 };
struct BloomLaunch {
    int kind;
    int level;      // -1 for the bright pass
    int step;       // 1 << level
    int src, dst;   // the set read (-1: the sum) and the set written (-1: none: levels == 0, or a last level that stores no b)
    int out;        // 1: the launch writes (bright) or updates (y, tile) out
};
struct BloomPlan {
    int count;
    BloomLaunch l[1 + 2 * BLOOM_MAX_LEVELS];
};

// The plan: the bright pass writes out = m and b_0 into set 0; level i reads b_i from the current set `cur`.  Gathered: x writes t
// into the other set, y reads t and writes b_{i+1} back into cur (nothing reads b_i any more).  Tiled: one launch reads cur and
// writes b_{i+1} into the other set (other workgroups still read b_i's halos), which becomes cur.  The last level stores no b.
// max_step: BLOOM_TILE_MAX_STEP for rt_film_bloom; the CPU program also walks the plans of every other choice.
RT_BL_HD inline BloomPlan bloom_plan(int levels, int flags, int max_step = BLOOM_TILE_MAX_STEP)
{
    BloomPlan p;
    p.count = 0;
    p.l[p.count++] = {BLOOM_BRIGHT, -1, 0, -1, levels > 0 ? 0 : -1, 1};
    int cur = 0;
    for (int i = 0; i < levels; ++i) {
        const int step = 1 << i;
        const bool last = i == levels - 1;
        if (step <= max_step && !(flags & BLOOM_NO_TILES)) {
            p.l[p.count++] = {BLOOM_TILE, i, step, cur, last ? -1 : 1 - cur, 1};
            cur = 1 - cur;
        } else {
            p.l[p.count++] = {BLOOM_X, i, step, cur, 1 - cur, 0};
            p.l[p.count++] = {BLOOM_Y, i, step, 1 - cur, last ? -1 : cur, 1};
        }
    }
    return p;
}

// One launch over a ws x h frame.
struct BloomArgs {
    const double *src;   // the sum (bright), b_i (x, tile) or t (y)
    double *dst;         // b_0 (bright; NULL with levels == 0), t (x), b_{i+1} (y, tile; NULL: not stored)
    double *out;         // bright: written; y, tile: out = out + wl * b_{i+1}; x: not used
    long long src_stride, dst_stride, out_stride;
    int ws, h;
    int step;
    int reserved;
    double n;            // (double)n
    double threshold;
    double wl;           // strength / (double)levels
};

// the B3 spline (1/16, 1/4, 3/8, 1/4, 1/16) at i = d + 2
RT_BL_HD inline double bloom_k(int i) { return i == 2 ? 0.375 : ((i == 1 || i == 3) ? 0.25 : 0.0625); }

// Element e of the bright pass: out = m, and b_0 when the call has levels.
RT_BL_HD inline void bloom_bright(const BloomArgs &a, long long e)
{
    const double m0 = a.src[e] / a.n, m1 = a.src[a.src_stride + e] / a.n, m2 = a.src[2 * a.src_stride + e] / a.n;
    a.out[e] = m0; a.out[a.out_stride + e] = m1; a.out[2 * a.out_stride + e] = m2;
    if (!a.dst) return;
    double mx = m0 > m1 ? m0 : m1;
    mx = mx > m2 ? mx : m2;
    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
    if (mx > a.threshold) {
        const double g = (mx - a.threshold) / mx;
        b0 = m0 > 0.0 ? m0 * g : 0.0;
        b1 = m1 > 0.0 ? m1 * g : 0.0;
        b2 = m2 > 0.0 ? m2 * g : 0.0;
    }
    a.dst[e] = b0; a.dst[a.dst_stride + e] = b1; a.dst[2 * a.dst_stride + e] = b2;
}

// Five taps `step` positions apart along one axis: p points at the centre element, `pitch` is the distance in elements between
// neighbours along the axis, pos the centre's coordinate on it and len the axis' length.  A tap outside [0, len) is skipped.
RT_BL_HD inline double bloom_tap(const double *p, long long pitch, int pos, int len, int step)
{
    double T = 0.0;
    for (int d = -2; d <= 2; ++d) {
        const long long q = (long long)pos + (long long)step * d;
        if (q < 0 || q >= len) continue;
        T = T + bloom_k(d + 2) * p[(long long)step * d * pitch];
    }
    return T;
}

// The level's accumulate into out.
RT_BL_HD inline void bloom_accumulate(double *out, double wl, double B) { *out = *out + wl * B; }

// Pixel (x, y) of the x pass: t = the taps of b_i along x.
RT_BL_HD inline void bloom_x_pixel(const BloomArgs &a, int x, int y)
{
    const long long e = (long long)x * a.h + y;
    for (int c = 0; c < 3; ++c) a.dst[c * a.dst_stride + e] = bloom_tap(a.src + c * a.src_stride + e, a.h, x, a.ws, a.step);
}

// Pixel (x, y) of the y pass: b_{i+1} = the taps of t along y, stored unless the level is the last, and added into out.
RT_BL_HD inline void bloom_y_pixel(const BloomArgs &a, int x, int y)
{
    const long long e = (long long)x * a.h + y;
    for (int c = 0; c < 3; ++c) {
        const double B = bloom_tap(a.src + c * a.src_stride + e, 1, y, a.h, a.step);
        if (a.dst) a.dst[c * a.dst_stride + e] = B;
        bloom_accumulate(a.out + c * a.out_stride + e, a.wl, B);
    }
}

// The tile kernel's phases for the tile whose first pixel is (x0, y0) and channel c: `tid` of `nthreads` threads does its share;
// lds is BLOOM_LDS_DOUBLES doubles: b (with halo, pitch P = BLOOM_TY + 2H) then t (pitch P).  A barrier stands between the phases.
// Consecutive tid are consecutive y in every phase.  No address outside the frame is formed, and no pass reads an LDS element that
// stands for a position outside it.
RT_BL_HD inline int bloom_tile_halo(int step) { return 2 * step; }
RT_BL_HD inline int bloom_tile_pitch(int step) { return BLOOM_TY + 4 * step; }

// load: b_i of the tile and its halo, memory -> lds b.
RT_BL_HD inline void bloom_tile_load(const BloomArgs &a, double *lds, int tid, int nthreads, int x0, int y0, int c)
{
    const int H = bloom_tile_halo(a.step), P = bloom_tile_pitch(a.step), count = (BLOOM_TX + 2 * H) * P;
    const double *src = a.src + c * a.src_stride;
    // Outside the frame the nearest pixel inside stands in (an address that exists), and no pass reads the copy.  Without a branch,
    // and with a trip count that does not depend on the thread, the loop unrolls into one batch of loads and one of LDS writes.
    const auto element = [&](int i) {
        const int lx = i / P, ly = i - lx * P;
        int gx = x0 - H + lx, gy = y0 - H + ly;
        gx = gx < 0 ? 0 : (gx >= a.ws ? a.ws - 1 : gx);
        gy = gy < 0 ? 0 : (gy >= a.h ? a.h - 1 : gy);
        lds[i] = src[(long long)gx * a.h + gy];
    };
    const int full = count / nthreads;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < full; ++k) element(tid + k * nthreads);
    if (tid + full * nthreads < count) element(tid + full * nthreads);
}

// x pass: t for the tile's columns and every row of the y halo, lds b -> lds t.
RT_BL_HD inline void bloom_tile_xpass(const BloomArgs &a, double *lds, int tid, int nthreads, int x0, int y0, int c)
{
    (void)c;
    const int H = bloom_tile_halo(a.step), P = bloom_tile_pitch(a.step), count = BLOOM_TX * P;
    double *t = lds + BLOOM_LDS_B;
    for (int i = tid; i < count; i += nthreads) {
        const int lx = i / P, ly = i - lx * P;
        const int gx = x0 + lx, gy = y0 - H + ly;
        if (gx >= a.ws || gy < 0 || gy >= a.h) continue;
        t[i] = bloom_tap(lds + (lx + H) * P + ly, P, gx, a.ws, a.step);
    }
}

// y pass and store: b_{i+1} from lds t, stored unless the level is the last, and added into out.
RT_BL_HD inline void bloom_tile_ypass(const BloomArgs &a, double *lds, int tid, int nthreads, int x0, int y0, int c)
{
    const int H = bloom_tile_halo(a.step), P = bloom_tile_pitch(a.step);
    const double *t = lds + BLOOM_LDS_B;
    for (int i = tid; i < BLOOM_TX * BLOOM_TY; i += nthreads) {
        const int lx = i / BLOOM_TY, ly = i - lx * BLOOM_TY;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= a.ws || gy >= a.h) continue;
        const long long e = (long long)gx * a.h + gy;
        const double B = bloom_tap(t + lx * P + ly + H, 1, gy, a.h, a.step);
        if (a.dst) a.dst[c * a.dst_stride + e] = B;
        bloom_accumulate(a.out + c * a.out_stride + e, a.wl, B);
    }
}

// tiles of a frame along x and y
RT_BL_HD inline int bloom_tiles_x(int ws) { return (ws + BLOOM_TX - 1) / BLOOM_TX; }
RT_BL_HD inline int bloom_tiles_y(int h) { return (h + BLOOM_TY - 1) / BLOOM_TY; }

#if defined(__HIPCC__)

constexpr int BLOOM_THREADS = 256;

// ws*h <= RT_FILM_MAX_PIXELS = 2^27: pixel indices are 32-bit, plane offsets 64-bit
__global__ __launch_bounds__(BLOOM_THREADS) void bloom_bright_kernel(const BloomArgs a)
{
    const unsigned npx = (unsigned)a.ws * (unsigned)a.h, stride = gridDim.x * BLOOM_THREADS;
    for (unsigned e = blockIdx.x * BLOOM_THREADS + threadIdx.x; e < npx; e += stride) bloom_bright(a, (long long)e);
}

__global__ __launch_bounds__(BLOOM_THREADS) void bloom_x_kernel(const BloomArgs a)
{
    const unsigned npx = (unsigned)a.ws * (unsigned)a.h, stride = gridDim.x * BLOOM_THREADS;
    for (unsigned e = blockIdx.x * BLOOM_THREADS + threadIdx.x; e < npx; e += stride) {
        const unsigned x = e / (unsigned)a.h;
        bloom_x_pixel(a, (int)x, (int)(e - x * (unsigned)a.h));
    }
}

__global__ __launch_bounds__(BLOOM_THREADS) void bloom_y_kernel(const BloomArgs a)
{
    const unsigned npx = (unsigned)a.ws * (unsigned)a.h, stride = gridDim.x * BLOOM_THREADS;
    for (unsigned e = blockIdx.x * BLOOM_THREADS + threadIdx.x; e < npx; e += stride) {
        const unsigned x = e / (unsigned)a.h;
        bloom_y_pixel(a, (int)x, (int)(e - x * (unsigned)a.h));
    }
}

// One level in one launch: workgroup (b, c) does tile (b / tiles_y, b % tiles_y) of channel c (the channels share nothing, and three
// times the workgroups fill the CUs' last round better); STEP fixes the halo and the pitch at compile time.
// At most 2^27 / (32 * 64) = 65536 tiles at full tiles; a thin frame has more, part-filled, tiles: bloom_tile_blocks.
template <int STEP>
__global__ __launch_bounds__(BLOOM_THREADS) void bloom_tile_kernel(BloomArgs a)
{
    __shared__ double lds[BLOOM_LDS_DOUBLES];
    a.step = STEP;
    const unsigned tiles_y = (unsigned)bloom_tiles_y(a.h);
    const unsigned tx = blockIdx.x / tiles_y, ty = blockIdx.x - tx * tiles_y;
    const int x0 = (int)(tx * BLOOM_TX), y0 = (int)(ty * BLOOM_TY), tid = (int)threadIdx.x, c = (int)blockIdx.y;
    bloom_tile_load(a, lds, tid, BLOOM_THREADS, x0, y0, c);
    __syncthreads();
    bloom_tile_xpass(a, lds, tid, BLOOM_THREADS, x0, y0, c);
    __syncthreads();
    bloom_tile_ypass(a, lds, tid, BLOOM_THREADS, x0, y0, c);
}

// blocks of a gather launch over npx pixels: at most 8 per CU, as the film kernels'
inline unsigned bloom_grid(long long npx, int cu_count)
{
    const long long want = (npx + BLOOM_THREADS - 1) / BLOOM_THREADS, cap = (long long)cu_count * 8;
    const long long n = want < cap ? want : cap;
    return (unsigned)(n < 1 ? 1 : n);
}

// workgroups of a tile launch: one per tile (ws*h <= 2^27 and ws, h >= 1: at most 2^27 / 32 + ... tiles, far below 2^31)
inline unsigned bloom_tile_blocks(int ws, int h) { return (unsigned)((long long)bloom_tiles_x(ws) * bloom_tiles_y(h)); }

#endif  // __HIPCC__

}  // namespace rt
