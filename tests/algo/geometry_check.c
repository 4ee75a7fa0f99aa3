/* The launch geometry of the library (python-ray-tracer_amd/csrc/rt_geometry.h) under UndefinedBehaviorSanitizer, on the
 * boundary shapes of include/mi355rt.h: frames of exactly 2^31 pixels, frames one or two pixels thin up to the longest side
 * accepted and their transposes, (2w-1)(2h-1) on both sides of 2^31 (the lattice switch of RT_AA_REFERENCE), column slabs at
 * odd x0 near w, and sequences of n frames at frames_per_launch up to n.  For every shape this replays what mi355rt.hip does
 * with the header's results — rt_render_sequence's launches, dispatch()'s column slabs and frame batches, the lattice launch,
 * rt_render's chunks and copies — and checks, with the int arithmetic the kernel (rt_device.h: render_kernel,
 * aa_resolve_kernel) does on the same values:
 *   every dispatch is at most 2^32 - 1 work-items, and its workgroup index fits an int;
 *   the tiles of each dispatch cover its columns x [0, h) exactly once, the slabs [x0, x1) and the batches [0, n) likewise;
 *   every value handed to an int (KParams, the feedback key, a lane's x, y and parked offset) fits it, and every 2-D copy
 *   pitch fits RT_GEO_MAX_PITCH;
 *   the shapes beyond the limits are refused.
 * Any sanitizer report aborts the run (exit != 0).  tests/test_algorithms.py builds and runs it. */
#include "../../python-ray-tracer_amd/csrc/rt_geometry.h"
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); exit(1); } } while (0)

static long long n_dispatch, n_shapes;

static int as_int(long long v, const char *what)
{
    CHECK(v >= INT_MIN && v <= INT_MAX, "%s = %lld does not fit an int", what, v);
    return (int)v;
}

/* The kernel's index arithmetic for the last lane of the last tile of a dispatch (the largest x, y and offset it forms), in
 * int as rt_device.h forms it: x = x0 + tx*8 + (lane>>3), y = ty*8 + (lane&7), parked offset (x - x0)*h + y of a lane inside
 * the frame. */
static void kernel_indices(int x0, int x1, int h, int tiles_y, int ntiles)
{
    const int tile = ntiles - 1;
    const int tx = tile / tiles_y, ty = tile - tx * tiles_y;
    const int x = x0 + tx * RT_GEO_TILE + 7, y = ty * RT_GEO_TILE + 7;
    CHECK(x >= x1 - 1 && y >= h - 1, "last tile ends at (%d, %d) inside [%d, %d) x [0, %d)", x, y, x0, x1, h);
    const int off = (x1 - 1 - x0) * h + (h - 1);   /* the frame's last pixel */
    CHECK(off >= 0, "parked offset %d", off);
}

/* One dispatch of dispatch(): nframes frames of columns [x0, x1), workgroups of wpw tiles. */
static void one_dispatch(long long x0, long long x1, long long h, long long wpw, long long nframes)
{
    const rt_geo_plan g = rt_geo_plan_of(x0, x1, h, wpw, nframes);
    CHECK(g.nslabs == 1 && g.frames_per_dispatch == nframes, "dispatch of [%lld,%lld) x %lld, %lld frames is not one dispatch", x0, x1, h, nframes);
    CHECK(g.tiles_x * RT_GEO_TILE >= x1 - x0 && (g.tiles_x - 1) * RT_GEO_TILE < x1 - x0, "tiles_x %lld for %lld columns", g.tiles_x, x1 - x0);
    CHECK(g.tiles_y * RT_GEO_TILE >= h && (g.tiles_y - 1) * RT_GEO_TILE < h, "tiles_y %lld for %lld rows", g.tiles_y, h);
    CHECK(g.blocks * wpw >= g.ntiles && (g.blocks - 1) * wpw < g.ntiles, "blocks %lld for %lld tiles", g.blocks, g.ntiles);
    const long long items = g.blocks * nframes * 64 * wpw;
    CHECK(items <= RT_GEO_MAX_ITEMS, "%lld work-items in one dispatch ([%lld,%lld) x %lld, %lld frames, wpw %lld)", items, x0, x1, h, nframes, wpw);
    as_int(g.blocks * nframes - 1, "largest workgroup index");
    as_int(g.blocks * wpw, "tiles of the dispatch");
    const int ix0 = as_int(x0, "x0"), ix1 = as_int(x1, "x1"), ih = as_int(h, "h");
    const int tiles_y = as_int(g.tiles_y, "tiles_y"), ntiles = as_int(g.ntiles, "ntiles");
    as_int(g.blocks, "bpf");
    kernel_indices(ix0, ix1, ih, tiles_y, ntiles);
    ++n_dispatch;
}

/* dispatch(): column slabs, or batches of frames, then one_dispatch each. */
static void dispatch(long long x0, long long x1, long long h, long long wpw, long long nframes)
{
    const rt_geo_plan g = rt_geo_plan_of(x0, x1, h, wpw, nframes);
    CHECK(g.frames_per_dispatch >= 1 && g.nslabs >= 1 && g.slab_tiles >= 1, "plan of [%lld,%lld) x %lld", x0, x1, h);
    if (g.nslabs > 1) {
        long long covered = x0;
        for (long long s = 0; s < g.nslabs; ++s) {
            const long long sx0 = x0 + s * g.slab_tiles * RT_GEO_TILE;
            const long long sx1 = sx0 + g.slab_tiles * RT_GEO_TILE < x1 ? sx0 + g.slab_tiles * RT_GEO_TILE : x1;
            CHECK(sx0 == covered && sx1 > sx0, "slab %lld of [%lld,%lld): [%lld,%lld) after %lld", s, x0, x1, sx0, sx1, covered);
            for (long long f = 0; f < nframes; ++f) one_dispatch(sx0, sx1, h, wpw, 1);
            covered = sx1;
        }
        CHECK(covered == x1, "slabs of [%lld,%lld) end at %lld", x0, x1, covered);
        return;
    }
    long long covered = 0;
    for (long long f = 0; f < nframes; f += g.frames_per_dispatch) {
        const long long nf = nframes - f < g.frames_per_dispatch ? nframes - f : g.frames_per_dispatch;
        one_dispatch(x0, x1, h, wpw, nf);
        covered += nf;
    }
    CHECK(covered == nframes, "batches cover %lld of %lld frames", covered, nframes);
}

/* launch(): the lattice path of RT_AA_REFERENCE (aa == 1) or the pixel path, for a launch of nframes frames. */
static void launch(long long w, long long h, long long x0, long long x1, long long wpw, long long nframes, int aa)
{
    as_int(rt_geo_tiles(h), "tiles_y"); as_int(rt_geo_tiles(x1 - x0) * rt_geo_tiles(h), "ntiles");
    long long l0, l1;
    if (aa && rt_geo_lattice(w, h, x0, x1, &l0, &l1)) {
        const long long LW = 2 * w - 1, LH = 2 * h - 1;
        CHECK(l0 >= 0 && l1 <= LW && l0 < l1 && l0 <= 2 * x0 && l1 > 2 * (x1 - 1), "lattice columns [%lld,%lld) for [%lld,%lld)", l0, l1, x0, x1);
        as_int(LW, "lattice w"); as_int(LH, "lattice h");
        for (long long f = 0; f < nframes && f < 2; ++f) dispatch(l0, l1, LH, wpw, 1);   /* (frame by frame: every one alike) */
        /* aa_resolve_kernel: one thread per pixel, workgroups of 256; pixel (x, y) reads lattice column 2x - l0 */
        const long long npx = (x1 - x0) * h;
        CHECK((npx + 255) / 256 * 256 <= RT_GEO_MAX_ITEMS, "aa_resolve_kernel: %lld work-items", (npx + 255) / 256 * 256);
        as_int(2 * (x1 - 1) - l0, "resolve column");
        as_int(2 * (h - 1), "resolve row");
        return;
    }
    dispatch(x0, x1, h, wpw, nframes);
}

/* rt_render's chunks and copies of [x0, x1) (planar, uint8 and float32). */
static void render_copies(long long x0, long long x1, long long h, int nch)
{
    const long long npx = (x1 - x0) * h, tiles = rt_geo_tiles(x1 - x0);
    if (nch < 2 || npx < (1ll << 19) || tiles < 4ll * nch) return;             /* one launch, one 1-D copy per output */
    long long prev = x0;
    for (int c = 0; c <= nch; ++c) {
        const long long cx = rt_geo_chunk_x(x0, x1, nch, c);
        as_int(cx, "chunk column");
        CHECK(c == 0 ? cx == x0 : (cx > prev && (cx == x1 || (cx - x0) % RT_GEO_TILE == 0)), "chunk edge %d of [%lld,%lld): %lld after %lld", c, x0, x1, cx, prev);
        prev = cx;
    }
    CHECK(prev == x1, "chunks of [%lld,%lld) end at %lld", x0, x1, prev);
    for (long long eb = 1; eb <= 4; eb += 3) {
        if (rt_geo_copy_2d(npx, eb)) CHECK(npx * eb <= RT_GEO_MAX_PITCH, "pitch %lld", npx * eb);
        else CHECK(npx * eb > RT_GEO_MAX_PITCH && 3 * npx * eb <= (long long)(SIZE_MAX >> 1), "plane copies of %lld bytes", npx * eb);
    }
}

/* One shape: rt_render_sequence's launches of fpl frames (0: 8), in every AA path and workgroup size, and rt_render. */
static void shape(long long w, long long h, long long x0, long long x1, long long n, long long fpl)
{
    CHECK(rt_geo_frame_ok(w, h), "frame %lld x %lld refused", w, h);
    CHECK(0 <= x0 && x0 < x1 && x1 <= w, "slab [%lld,%lld) of %lld", x0, x1, w);
    const long long per = fpl > 0 ? fpl : 8;
    for (long long wpw = 2; wpw <= 4; wpw += 2)
        for (int aa = 0; aa <= 1; ++aa) {
            long long covered = 0;
            for (long long i = 0; i < n; i += per) {
                const long long nf = n - i < per ? n - i : per;
                launch(w, h, x0, x1, wpw, nf, aa);
                covered += nf;
            }
            CHECK(covered == n, "launches cover %lld of %lld frames", covered, n);
        }
    for (int nch = 1; nch <= 8; ++nch) render_copies(x0, x1, h, nch);
    ++n_shapes;
}

static void frame(long long w, long long h)
{
    shape(w, h, 0, w, 1, 0);
    /* slabs near w, at odd and even x0 */
    for (long long d = 1; d <= 17; d += 4) if (d <= w) shape(w, h, w - d, w, 1, 0);
    if (w >= 13) shape(w, h, w - 13, w - 1, 1, 0);
    if (w > 2) shape(w, h, 1, w - 1, 1, 0);
}

int main(void)
{
    const long long M = RT_GEO_MAX_PIXELS;
    /* w*h = 2^31 exactly, in every aspect with a power-of-two side */
    for (long long w = 8; w <= M / 4; w *= 2) frame(w, M / w);
    frame(65536, 32768);
    /* thin frames, h = 1, 2 up to the longest side accepted, and their transposes */
    const long long thin[] = { (1ll << 29) + 8, (1ll << 29) + 9, 1ll << 30, (1ll << 30) + 1, RT_GEO_MAX_W - 1, RT_GEO_MAX_W };
    for (int i = 0; i < 6; ++i)
        for (long long h = 1; h <= 2; ++h)
            if (thin[i] * h <= M) frame(thin[i], h);
    const long long tall[] = { (1ll << 26) + 1, (1ll << 28) + 8, RT_GEO_MAX_H - 1, RT_GEO_MAX_H };
    for (int i = 0; i < 4; ++i)
        for (long long w = 1; w <= 2; ++w) frame(w, tall[i]);
    frame(4, RT_GEO_MAX_H); frame(3, RT_GEO_MAX_H);
    /* (2w-1)(2h-1) just below and just above 2^31; lattice sides at the limit */
    frame(23170, 23170); frame(23171, 23171); frame(23170, 23171);
    frame(46340, 11585); frame(46341, 11585);
    frame((1ll << 30) - 4, 1); frame((1ll << 30) - 3, 1); frame(1ll << 30, 1);
    frame(1, (1ll << 28) - 16); frame(1, (1ll << 28) - 15);
    /* sequences: n frames at frames_per_launch up to n */
    shape(32768, 16384, 0, 32768, 8, 0);                 /* 8 frames of 2^29 pixels at the default */
    shape(32768, 16384, 0, 32768, 16, 16);
    shape(7680, 4320, 0, 7680, 131, 131);
    shape(7680, 4320, 0, 7680, 262, 0);
    shape(7680, 4320, 0, 7680, 1000, 1000);
    shape(7680, 4320, 1, 7679, 131, 131);
    shape(65536, 32768, 0, 65536, 3, 3);
    shape((1ll << 29) + 8, 2, 0, (1ll << 29) + 8, 3, 3);
    shape(1920, 1080, 0, 1920, 100000, 100000);
    shape(1, 1, 0, 1, 1 << 20, 1 << 20);
    shape(1, 1, 0, 1, INT_MAX / 1024, 0);
    shape(64, 64, 0, 64, 50000, INT_MAX);
    /* refused: a side beyond the limits, or more than 2^31 pixels */
    const long long bad[][2] = { { RT_GEO_MAX_W + 1, 1 }, { INT_MAX, 1 }, { 1, RT_GEO_MAX_H + 1 }, { 2, (1ll << 29) + 8 }, { 1, INT_MAX },
                                 { 65536, 32769 }, { 46341, 46341 }, { (1ll << 30) + 1, 2 }, { 0, 1 }, { 1, 0 }, { INT_MAX, INT_MAX } };
    for (int i = 0; i < (int)(sizeof bad / sizeof bad[0]); ++i) CHECK(!rt_geo_frame_ok(bad[i][0], bad[i][1]), "%lld x %lld accepted", bad[i][0], bad[i][1]);
    /* every accepted frame's one tile column fits one dispatch at either workgroup size */
    for (long long wpw = 2; wpw <= 4; wpw += 2) {
        const rt_geo_plan g = rt_geo_plan_of(0, 1, RT_GEO_MAX_H, wpw, 1);
        CHECK(g.items <= RT_GEO_MAX_ITEMS, "one tile column of h = %lld: %lld work-items", RT_GEO_MAX_H, g.items);
    }
    printf("shapes=%lld dispatches=%lld ok\n", n_shapes, n_dispatch);
    return 0;
}
