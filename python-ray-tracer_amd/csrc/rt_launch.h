// rt_launch.h — the kernels' argument (rt_kparams.h: rt::KParams) as the host builds it, and what an entry point refuses before it
// touches the device.  From the view (camera, ray grid, lens), the scene's layout (rt_scene.h), the planned family (rt_plan.h) and
// rt_params:
//   * the reach bound behind extent2, floor_anch and facing_tau (reach_of);
//   * the part of KParams a render launch and a guides launch share (frame_part), and what each adds (render_part, guides_part);
//   * the lattice launch's pair of RT_AA_REFERENCE (lattice_pair), a frame of a sequence (frame_params), a column slab of a frame
//     beyond one dispatch (slab_params), and the fields of one dispatch (dispatch_part);
//   * the entry checks, as functions that return a code and the rt_last_error text (check_*), each entry's in its own order.
// HIP-free, like rt_plan.h and for the same reason: pure arithmetic, testable where there is no GPU.  mi355rt.hip keeps the HIP
// calls, the buffers and the caches, and hands in the device pointers; tests/algo/launch_check.cpp walks these functions over a table
// of views, scenes and slabs under AddressSanitizer and UBSan and compares every field with the recorded one.
#pragma once
#include "rt_kparams.h"
#include "rt_facing.h"
#include "rt_plan.h"

#include <cmath>
#include <cstring>

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace rt {

// What the rt_set_camera, rt_set_lens, rt_set_raygen and rt_set_pixel_loc entries leave behind.
struct View {
    double cam_o[3] = {0, 0, 0}, cam_R[9] = {0};
    int w = 0, h = 0;
    double px = 0, y0 = 0, dy = 0, z0 = 0, dz = 0;
    double lens_a = 0.0, lens_f = 1.0;   // rt_set_lens: aperture (0: the pinhole camera) and focus distance
    bool have_cam = false, have_grid = false, explicit_grid = false;
};

// Every ray origin of a launch lies within reach = |cam| (+ the aperture: primary rays start on the lens, |L - cam| <= a) +
// 999 (depth + 1) + the scene's extent of the world origin.  aperture is 0 for a launch whose family has no lens, and for the guides
// (depth 0: every ray starts at the camera).  Sets k.extent2 and k.floor_anch (part of the cull tables' cache key) and returns the
// reach, which rt_facing_tau takes.
inline double reach_of(KParams &k, const double cam_o[3], double aperture, int depth, double extent2)
{
    double cam2 = cam_o[0] * cam_o[0] + cam_o[1] * cam_o[1] + cam_o[2] * cam_o[2];
    if (aperture > 0.0) { const double e = std::sqrt(cam2) + aperture; cam2 = e * e; }
    k.extent2 = (float)(1.0001 * (cam2 > extent2 ? cam2 : extent2));
    const double reach = std::sqrt(cam2) + 999.0 * (depth + 1) + std::sqrt(extent2);
    k.floor_anch = (float)(0x1p-39 * reach * reach);
    return reach;
}

// What a render launch and a guides launch share: k zeroed, then the scene (`scene`: the current scene buffer) and its counts, the
// frame, the grid (`pixel_loc`: the explicit grid's buffer) and the camera, by value, and the reach values.  Returns the reach.
inline double frame_part(KParams &k, const View &v, const SceneLayout &lay, const double *scene, const double *pixel_loc, int lanes_primary,
                         int x0, int x1, double aperture, int depth)
{
    std::memset(&k, 0, sizeof k);
    k.scene = scene;
    k.nframes = 1;
    k.pixel_loc = v.explicit_grid ? pixel_loc : nullptr;
    k.w = v.w; k.h = v.h; k.x0 = x0; k.x1 = x1;
    k.S = lay.S; k.P = lay.P; k.L = lay.L; k.NC = lay.NC; k.plane_codes = lay.plane_codes;
    k.lanes_primary = lanes_primary;
    k.tiles_y = (int)rt_geo_tiles(v.h);
    k.px = v.px; k.y0 = v.y0; k.dy = v.dy; k.z0 = v.z0; k.dz = v.dz;
    std::memcpy(k.cam_o, v.cam_o, sizeof k.cam_o);
    std::memcpy(k.cam_R, v.cam_R, sizeof k.cam_R);
    k.anchors = anchors_of(lay);
    return reach_of(k, v.cam_o, aperture, depth, lay.extent2);
}

// A guides launch (rt_guides.h) over columns [x0, x1): the frame part of rays that start at the camera and go no further than the
// first hit (no lens, depth 0), three float planes of plane_stride elements, and for a textured scene its texture block and texels.
inline void guides_part(KParams &k, const View &v, const SceneLayout &lay, const double *scene, const double *pixel_loc, const float *texels,
                        int lanes_primary, int x0, int x1, void *d_guides, long long plane_stride)
{
    frame_part(k, v, lay, scene, pixel_loc, lanes_primary, x0, x1, 0.0, 0);
    k.out_f32 = (float *)d_guides;
    k.plane_stride = plane_stride;
    if (lay.T > 0) { k.lens.tex = lay.tex_off; k.lens.texels = texels; }
}

// A render launch of family `fam` (plan_launch) over columns [x0, x1): the frame part, rt_params, the outputs, and the union —
// refl_pow first; a lens (aperture > 0; check_params: the scene has a material table) runs the lens kernels, which read no refl_pow:
// the lens travels in its place, by value with this launch.  The texture kernels read no refl_pow either: the 6-column material
// block, the texture block and the texel array (`texels`: the current scene buffer's) travel in its place; the lighting kernels are
// texture kernels and the sky kernels lighting kernels.
inline void render_part(KParams &k, const View &v, const SceneLayout &lay, Family fam, const rt_params *p, const double *scene,
                        const double *pixel_loc, const float *texels, int lanes_primary, int x0, int x1, void *d_u8, void *d_f32,
                        long long plane_stride, unsigned *tile_cycles)
{
    const bool lens = has_lens(fam);
    const double reach = frame_part(k, v, lay, scene, pixel_loc, lanes_primary, x0, x1, lens ? v.lens_a : 0.0, p->depth);
    k.out_u8 = (uint8_t *)d_u8;
    k.out_f32 = (float *)d_f32;
    k.tile_cycles = tile_cycles;
    k.plane_stride = plane_stride;
    k.depth = p->depth;
    k.aa = p->aa_mode; k.u8_rgb = (p->flags & RT_FLAG_U8_RGB) ? 1 : 0; k.u8_hwc = (p->flags & RT_FLAG_U8_HWC) ? 1 : 0;
    k.spp = p->spp; k.seed = p->seed;
    k.ntiles = (int)(rt_geo_tiles(x1 - x0) * k.tiles_y);      // (rt_geo_frame_ok: below 2^28)
    k.amb = p->amb; k.lamb = p->lamb;
    std::memcpy(k.refl_pow, p->refl_pow, sizeof k.refl_pow);
    if (lens) { k.lens.aperture = v.lens_a; k.lens.focus = v.lens_f; k.lens.mat = lay.lens_mat; }
    if (has_tex(fam)) { k.lens.mat = lay.lens_mat; k.lens.tex = lay.tex_off; k.lens.texels = texels; }
    if (has_lit(fam)) k.lens.lit = lay.lit_off;
    if (has_sky(fam)) k.lens.sky = lay.sky_off;
    // the facing certificate's margin (rt_facing.h): the same reach bounds |light - Pt|; a family without a material table reads the
    // wave-uniform p.lamb (MS::mat is has_mat(family) in the kernels), the others look at the lane's own coefficient
    k.facing_tau = rt_facing_tau(reach, has_mat(fam) ? 0.0 : p->lamb);
}

// RT_AA_REFERENCE on the closed-form grid: kl renders lattice columns [li0, li1) of the (2w-1) x (2h-1) half-pixel lattice of k's
// frame as float64 samples into `lat`, and k, for aa_resolve_kernel, learns where they are.
inline void lattice_pair(KParams &k, KParams &kl, long long li0, long long li1, double *lat)
{
    const long long LW = 2ll * k.w - 1, LH = 2ll * k.h - 1;
    kl = k;
    kl.aa = 0; kl.lattice = 1; kl.out_u8 = nullptr; kl.out_f32 = nullptr; kl.out_f64 = lat; kl.tile_cycles = nullptr;   // (rt_set_tile_stats: pixel launches only)
    kl.w = (int)LW; kl.h = (int)LH; kl.x0 = (int)li0; kl.x1 = (int)li1; kl.plane_stride = 0;
    kl.tiles_y = (int)rt_geo_tiles(LH);
    kl.ntiles = (int)(rt_geo_tiles(li1 - li0) * kl.tiles_y);
    k.out_f64 = lat; k.lat_x0 = (int)li0; k.lat_h = (int)LH;
}

// Frame fr of a sequence: the outputs + fr * frame_stride elements.
inline KParams frame_params(const KParams &k, int fr, long long frame_stride)
{
    KParams kf = k;
    if (kf.out_u8) kf.out_u8 += (size_t)fr * frame_stride;
    if (kf.out_f32) kf.out_f32 += (size_t)fr * frame_stride;
    return kf;
}

// Column slab s of the launch k that g = rt_geo_plan_of(k.x0, k.x1, k.h, ...) cuts into g.nslabs dispatches: its columns, its
// tiles, and every output from its first column on.
inline KParams slab_params(const KParams &k, const rt_geo_plan &g, long long s)
{
    const long long sx0 = k.x0 + s * g.slab_tiles * TILE, sx1 = std::min<long long>(k.x1, sx0 + g.slab_tiles * TILE);
    const long long dx = sx0 - k.x0;
    KParams ks = k;
    ks.x0 = (int)sx0; ks.x1 = (int)sx1; ks.ntiles = (int)(rt_geo_tiles(sx1 - sx0) * k.tiles_y);
    if (ks.out_u8) ks.out_u8 += k.u8_hwc ? 3 * dx : dx * k.h;       // (element [c, x, y] of rt_render_device)
    if (ks.out_f32) ks.out_f32 += dx * k.h;
    if (ks.out_f64) ks.out_f64 += 3 * dx * k.h;                      // (lattice samples, [column - x0][row][3])
    if (ks.tile_cycles) ks.tile_cycles += dx / TILE * k.tiles_y;
    return ks;
}

// What one dispatch of `grid` workgroups per frame sets just before it goes out.
inline void dispatch_part(KParams &k, int nframes, unsigned grid, long long frame_stride, const OrderShape &os)
{
    k.nframes = nframes; k.bpf = (int)grid; k.frame_stride = frame_stride; k.order_tiles = os.otiles ? 1 : 0;
    div_magic((unsigned)k.bpf, k.bpf_magic, k.bpf_shift);
    div_magic((unsigned)k.tiles_y, k.tiles_y_magic, k.tiles_y_shift);
    k.seq_offset = os.seq_offset;
}

// An entry check's answer: RT_OK, or the code and the rt_last_error text ("entry: msg" where the refusal names its entry:
// rt_film_launch.h).
struct Refusal {
    int code = RT_OK;
    const char *msg = nullptr;
    const char *entry = nullptr;
};

// What every launch needs before anything else: a scene, a camera, a ray grid.
inline Refusal check_state(bool have_scene, const View &v)
{
    if (!have_scene) return {RT_ERR_STATE, "rt_set_scene has not been called"};
    if (!v.have_cam) return {RT_ERR_STATE, "rt_set_camera has not been called"};
    if (!v.have_grid) return {RT_ERR_STATE, "rt_set_raygen / rt_set_pixel_loc has not been called"};
    return {};
}

inline Refusal check_columns(const View &v, int x0, int x1)
{
    if (x0 < 0 || x1 > v.w || x0 >= x1) return {RT_ERR_BAD_ARG, "column range must satisfy 0 <= x0 < x1 <= w"};
    return {};
}

// Every entry that renders with rt_params.
inline Refusal check_params(bool have_scene, const View &v, const SceneLayout &lay, const rt_params *p, int x0, int x1)
{
    if (!p) return {RT_ERR_BAD_ARG, "params is NULL"};
    Refusal r = check_state(have_scene, v);
    if (r.code != RT_OK) return r;
    if (p->depth < 0 || p->depth > RT_MAX_DEPTH) return {RT_ERR_BAD_ARG, "depth outside 0..RT_MAX_DEPTH"};
    if (p->aa_mode != RT_AA_NONE && p->aa_mode != RT_AA_REFERENCE && p->aa_mode != RT_AA_STOCHASTIC)
        return {RT_ERR_BAD_ARG, "unknown aa_mode"};
    if (p->aa_mode == RT_AA_STOCHASTIC) {
        if (p->spp < 1 || p->spp > RT_MAX_SPP) return {RT_ERR_BAD_ARG, "spp outside 1..RT_MAX_SPP"};
        if (v.explicit_grid) return {RT_ERR_STATE, "RT_AA_STOCHASTIC needs the closed-form ray grid (rt_set_raygen)"};
    }
    r = check_columns(v, x0, x1);
    if (r.code != RT_OK) return r;
    if (lay.M > 0 && (p->flags & RT_FLAG_COUNT_RAYS))
        return {RT_ERR_BAD_ARG, "RT_FLAG_COUNT_RAYS is not available for a scene with materials"};
    if (v.lens_a > 0.0 && lay.M == 0)
        return {RT_ERR_STATE, "a lens with aperture > 0 needs a scene with a material table (M >= 1)"};
    return {};
}

// rt_render_device (n == 1) and rt_render_sequence: n frames of columns [x0, x1) into device memory, frame_stride elements apart.
inline Refusal check_device_outputs(const View &v, const rt_params *p, int x0, int x1, int n, const void *d_u8, const void *d_f32,
                                    int64_t plane_stride, int64_t frame_stride)
{
    if (!d_u8 && !d_f32) return {RT_ERR_BAD_ARG, "both output pointers are NULL"};
    if (p->flags & RT_FLAG_U8_HWC) {
        if (d_f32) return {RT_ERR_BAD_ARG, "RT_FLAG_U8_HWC re-uses plane_stride as the image row pitch: render the float32 buffer in a separate call"};
        if (plane_stride < (int64_t)(x1 - x0)) return {RT_ERR_BAD_ARG, "row pitch smaller than the slab width"};
        if (n > 1 && frame_stride < 3 * plane_stride * v.h) return {RT_ERR_BAD_ARG, "frame_stride smaller than one image"};
    } else {
        if (plane_stride < (int64_t)(x1 - x0) * v.h) return {RT_ERR_BAD_ARG, "plane_stride smaller than the slab"};
        if (n > 1 && frame_stride < 3 * plane_stride) return {RT_ERR_BAD_ARG, "frame_stride smaller than three planes"};
    }
    return {};
}

// rt_render and rt_render_begin: the uint8 image's staging plane is pitched like an image, the float32 planes are not.
inline Refusal check_host_hwc(const rt_params *p, const void *out_f32)
{
    if (!(p->flags & RT_FLAG_U8_HWC) || !out_f32) return {};
    return {RT_ERR_BAD_ARG, "RT_FLAG_U8_HWC: request the uint8 image and the float32 buffer in separate calls"};
}

}  // namespace rt
