// rt_guides.h — the first-hit guides (include/mi355rt.h: rt_render_guides): what the pinhole camera's RT_AA_NONE primary ray of a
// pixel hits first, as eight float32 planes — normal, distance, albedo, object id.  One kernel beside the render kernels, which it
// does not touch: it stages the packed scene and the float32 cull tables into LDS as render_kernel does, forms the ray with pixel_P
// and primary_dir, and asks closest_hit, the render kernels' own query with their culls, for the exact closest hit.  Normal, hit
// point and texel index are formed as trace_bounce forms them for the first trace.  Shared with the render kernels through
// rt_device.h: tile_xy, hit_slot, plane_base (and pixel_P, primary_dir, closest_hit, sphere_hot, sphere_orig, texel_of).  Still
// written out here as render_kernel and trace_bounce have them, because moving them into a shared function changed instruction
// streams of the render kernels or of this one (Denoiser: Guides): the two staging copies, the Lds view, the lane's
// pixel, the normal.  One wave per 8x8 tile laid out as in render_kernel, four waves per workgroup, tiles in plain order: no
// dispatch-order feedback, no parked state, no per-thread LDS slots.
// MODE is closest_hit's (rt_plan.h: plan_guides picks it as plan_launch would for the scene): 0 float64 sphere records in LDS,
// 1 none (sphere_hot widens the float32 table), 2 the lane-owned traversal of a clustered scene.
#pragma once
#include "rt_device.h"

#pragma clang fp contract(off)

namespace rt {

constexpr int GUIDE_PLANES = 8;
constexpr int GUIDE_WPW = 4;

// p: scene, ftab, pixel_loc, the grid, the camera, x0, x1, tiles_y (+ magic), ntiles, S, P, L, NC, anchors, plane_codes, extent2,
// floor_anch, lanes_primary as for a render launch; out_f32 / plane_stride the guides; lens.tex and lens.texels where textured != 0.
template <int MODE>
__global__ __launch_bounds__(64 * GUIDE_WPW) void guides_kernel(const KParams p, const int textured)
{
    constexpr int WG_THREADS = 64 * GUIDE_WPW;
    constexpr bool NOREC = MODE >= 1;
    const int nrec = (int)lds_doubles(NOREC ? 0 : p.S, p.P, p.L);             // MODE 1 / 2: planes and lights only (sphere_hot)
    const double *rec_src = p.scene + (NOREC ? (size_t)p.S * SPH_STRIDE : 0);
    float *sph32 = reinterpret_cast<float *>(lds_raw + nrec);                 // (nrec is a multiple of 4 doubles: 16-byte aligned)
    const TableLayout tl = table_layout(p.S, p.NC, p.anchors, p.P);
    const bool LANES = MODE >= 2 && p.anchors > 0;                            // (render_kernel: no origin-form cluster spheres then)
    const size_t ntab = LANES ? tl.total_lanes : tl.total;
    {
        for (int i = threadIdx.x; i < nrec; i += WG_THREADS) lds_raw[i] = rec_src[i];
        const int nf4 = (int)(ntab / 4);
        const f4 *src = reinterpret_cast<const f4 *>(p.ftab);
        f4 *dst = reinterpret_cast<f4 *>(sph32);
        for (int i = threadIdx.x; i < nf4; i += WG_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Lds lds{sph32, sph32 + tl.tab, LANES ? nullptr : sph32 + tl.csph32, sph32 + tl.ctab, sph32 + tl.cbox, sph32 + tl.gbox,
                  sph32 + tl.gtab, nullptr, p.NC, __builtin_amdgcn_readfirstlane(wave), MODE < 2, MODE >= 2, false, RT_DEFER_DIRECTION != 0 && MODE < 2, nullptr};
    const int tile = __builtin_amdgcn_readfirstlane((int)blockIdx.x * GUIDE_WPW + wave);
    if (tile >= p.ntiles) return;                                             // whole wave, after the barrier
    int tx, ty;
    tile_xy(p, tile, tx, ty);
    const int x = p.x0 + tx * TILE + (lane >> 3);
    const int y = ty * TILE + (lane & 7);
    const bool inb = (x < p.x1) && (y < p.h);
    const int xc = inb ? x : p.x0, yc = inb ? y : 0;                          // keep addresses valid for idle lanes

    const V3 o{p.cam_o[0], p.cam_o[1], p.cam_o[2]};
    const V3 d = primary_dir(p, pixel_P(p, xc, yc));
    double t = 999.0;
    int idx = -1, type = HIT_NONE;
    if (inb) closest_hit<Query<MODE>>(lds, p, o, d, 0, t, idx, type);               // (anchor 0: the camera, as the first trace)
    if (!inb) return;

    float g[GUIDE_PLANES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1.0f};
    if (type != HIT_NONE) {
        const V3 Pt{o.x + t * d.x, o.y + t * d.y, o.z + t * d.z};             // trace.py:60
        const int plb = plane_base<NOREC>(p.S);
        V3 N;
        const double *col;                                                    // the object's own colour (float32 widened)
        double id;
        if (type == HIT_SPHERE) {
            const SphHot s = sphere_hot<NOREC>(lds, idx);
            N = normalize3(V3{Pt.x - s.x, Pt.y - s.y, Pt.z - s.z});           // common.py:94-101
            col = (NOREC ? p.scene : lds.recs()) + idx * SPH_STRIDE + 4;
            id = sphere_orig<NOREC>(lds, p, idx);
        } else {
            const double *r = lds.recs() + plb + idx * PL_STRIDE;
            N = V3{r[6], r[7], r[8]};                                         // float32-renormalised, host-side
            col = r + 12;
            id = (double)(p.S + idx);
        }
        g[0] = (float)N.x; g[1] = (float)N.y; g[2] = (float)N.z;
        g[3] = (float)t;
        if (textured) {                                                       // the first trace's texel (an untextured object's is its colour)
            const unsigned ti = texel_of(p, hit_slot(type, idx, p.S), Pt);
            const f4 tc = reinterpret_cast<const f4 *>(p.lens.texels)[ti];
            g[4] = tc[0]; g[5] = tc[1]; g[6] = tc[2];
        } else { g[4] = (float)col[0]; g[5] = (float)col[1]; g[6] = (float)col[2]; }
        g[7] = (float)id;
    }
    float *out = p.out_f32 + ((long long)(x - p.x0) * p.h + y);
#pragma unroll
    for (int c = 0; c < GUIDE_PLANES; ++c) out[(long long)c * p.plane_stride] = g[c];
}

}  // namespace rt
