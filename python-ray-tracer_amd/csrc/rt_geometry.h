/*
 * rt_geometry.h — the host-side launch arithmetic of mi355rt.hip in one place: frame limits, tiles, workgroups, work-items
 * per dispatch, column slabs, frames per dispatch, the lattice-or-per-pixel choice of RT_AA_REFERENCE, rt_render's chunk
 * columns and its copy pitches.  Pure functions on 64-bit integers, no HIP: the library calls them, and
 * tests/algo/geometry_check.c runs them under UndefinedBehaviorSanitizer on the boundary shapes of include/mi355rt.h.
 * Valid C99 and C++.
 */
#ifndef RT_GEOMETRY_H
#define RT_GEOMETRY_H

#include <stdint.h>

#define RT_GEO_TILE 8                            /* tiles are 8x8 pixels, one wavefront each (rt_layout.h: TILE) */
#define RT_GEO_MAX_PIXELS (1ll << 31)            /* w*h of a frame */
#define RT_GEO_MAX_W ((1ll << 31) - 8)           /* the kernel forms x0 + 8 tx + 7 (up to w + 6) as a signed int */
#define RT_GEO_MAX_H ((1ll << 29) - 32)          /* one column of tiles, ceil(h/8) <= 2^26 - 4, in whole workgroups of up to
                                                    four tiles, is at most 2^32 - 256 work-items: one dispatch */
#define RT_GEO_MAX_ITEMS 0xFFFFFFFFll            /* work-items of one dispatch: the HSA packet's grid size is 32 bits */
#define RT_GEO_MAX_PITCH 0x7FFFFFFFll            /* largest row pitch (bytes) rt_render hands to a 2-D copy */

/* 1 if a frame of w x h pixels is accepted (rt_set_raygen, rt_set_pixel_loc): 1 <= w <= 2^31 - 8, 1 <= h <= 2^29 - 32 and
 * w*h <= 2^31. */
static inline int rt_geo_frame_ok(long long w, long long h)
{
    return w >= 1 && h >= 1 && w <= RT_GEO_MAX_W && h <= RT_GEO_MAX_H && w * h <= RT_GEO_MAX_PIXELS;
}

static inline long long rt_geo_tiles(long long n) { return (n + RT_GEO_TILE - 1) / RT_GEO_TILE; }

/* RT_AA_REFERENCE on the closed-form grid renders the (2w-1) x (2h-1) half-pixel lattice when that lattice is itself a frame
 * the kernel can address (fewer than 2^31 samples, sides within the frame limits); otherwise nine taps per pixel.  The lattice
 * columns of pixel columns [x0, x1) are [*l0, *l1), *l1 exclusive.  (For an accepted frame.) */
static inline int rt_geo_lattice(long long w, long long h, long long x0, long long x1, long long *l0, long long *l1)
{
    const long long LW = 2 * w - 1, LH = 2 * h - 1;
    *l0 = 2 * x0 - 1 > 0 ? 2 * x0 - 1 : 0;
    *l1 = 2 * x1 < LW ? 2 * x1 : LW;
    return LW * LH < RT_GEO_MAX_PIXELS && LW <= RT_GEO_MAX_W && LH <= RT_GEO_MAX_H;
}

/* One launch of the render kernel over columns [x0, x1) of a frame h high, nframes frames, workgroups of wpw tiles (64 wpw
 * work-items).  It goes out as dispatches of at most RT_GEO_MAX_ITEMS work-items: a frame that exceeds that alone is cut into
 * nslabs column slabs of slab_tiles tile columns (the last one narrower; slab s starts at column x0 + 8 s slab_tiles), one
 * dispatch per slab and frame; otherwise up to frames_per_dispatch frames share one dispatch. */
typedef struct rt_geo_plan {
    long long tiles_x, tiles_y, ntiles;   /* of [x0, x1) x [0, h) */
    long long blocks;                     /* workgroups per frame */
    long long items;                      /* work-items per frame, blocks * 64 wpw */
    long long slab_tiles, nslabs;         /* tile columns per slab; slabs per frame (1: the whole range) */
    long long frames_per_dispatch;        /* 1 when nslabs > 1 */
} rt_geo_plan;

static inline rt_geo_plan rt_geo_plan_of(long long x0, long long x1, long long h, long long wpw, long long nframes)
{
    rt_geo_plan g;
    g.tiles_x = rt_geo_tiles(x1 - x0);
    g.tiles_y = rt_geo_tiles(h);
    g.ntiles = g.tiles_x * g.tiles_y;
    g.blocks = (g.ntiles + wpw - 1) / wpw;
    g.items = g.blocks * 64 * wpw;
    const long long max_blocks = RT_GEO_MAX_ITEMS / (64 * wpw);   /* workgroups of one dispatch */
    if (g.items > RT_GEO_MAX_ITEMS) {
        const long long max_cols = max_blocks * wpw / g.tiles_y;  /* >= 1 for h <= RT_GEO_MAX_H */
        g.nslabs = (g.tiles_x + max_cols - 1) / max_cols;
        g.slab_tiles = (g.tiles_x + g.nslabs - 1) / g.nslabs;     /* equal widths, at most max_cols */
        g.frames_per_dispatch = 1;
    } else {
        g.nslabs = 1;
        g.slab_tiles = g.tiles_x;
        g.frames_per_dispatch = max_blocks / g.blocks < nframes ? max_blocks / g.blocks : nframes;
    }
    return g;
}

/* rt_render's column chunks: nch chunks of [x0, x1), the first and the last half as wide as the others, edges on tile
 * columns.  Chunk c is [rt_geo_chunk_x(.., c), rt_geo_chunk_x(.., c + 1)). */
static inline long long rt_geo_chunk_x(long long x0, long long x1, long long nch, long long c)
{
    const long long num = (c == 0) ? 0 : (c == nch ? 2 * (nch - 1) : 2 * c - 1);   /* of 2 (nch - 1) half-units */
    const long long x = x0 + rt_geo_tiles(x1 - x0) * num / (2 * (nch - 1)) * RT_GEO_TILE;
    return x < x1 ? x : x1;
}

/* rt_render copies a chunk's three planes (pitch: one plane, npx elements of elem_bytes) as one 2-D copy when the pitch is
 * at most RT_GEO_MAX_PITCH bytes, else plane by plane. */
static inline int rt_geo_copy_2d(long long npx, long long elem_bytes) { return npx * elem_bytes <= RT_GEO_MAX_PITCH; }

#endif /* RT_GEOMETRY_H */
