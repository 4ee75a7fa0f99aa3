// rt_kparams.h — rt::KParams, the one argument of every render, table, guides and resolve kernel: plain data, so it needs no HIP.
// rt_device.h includes it for the kernels; rt_launch.h fills it on the host.
#pragma once
#include <stdint.h>

namespace rt {

struct KParams {
    const double *scene;       // packed records: S spheres, then P planes, then L lights
    const double *pixel_loc;   // explicit (3,w,h) grid or nullptr (closed-form ray generation)
    uint8_t *out_u8;           // or nullptr
    float *out_f32;            // or nullptr
    unsigned *tile_cycles;     // or nullptr: per-tile wave cycles of this launch (rt_set_tile_stats)
    unsigned *cost;            // or nullptr: scheduler feedback — a measuring launch stores every tile block's cost (wave cycles / 4,
                               // summed over the block's waves); order_kernel turns them into the next launches' dispatch order
    const unsigned *order;     // or nullptr: workgroup -> tile-block permutation from a measured launch's costs (XCD-affine, longest
                               // first inside every XCD); order + bpf: the same XCD assignment in plain tile order, which all but the
                               // last frame of a multi-frame launch use (order_kernel)
    int order_tiles;           // 1 (four-wave kernels): `order` and `cost` are per TILE — workgroup b's wave w renders tile
                               // order[b WPW + w], so that a workgroup's waves can be tiles of equal cost (they end together and
                               // hand their slots back together); 0: per tile block (WPW consecutive tiles)
    int seq_offset;            // bpf (x WPW with order_tiles), or 0 to dispatch every frame of a multi-frame launch longest-first (MI355RT_SEQ_ORDER=0)
    int nframes, bpf;          // frames rendered by this launch (rt_render_sequence) and workgroups per frame: workgroup b renders
                               // block order[b % bpf] of frame b / bpf into the outputs + (b / bpf) * frame_stride elements
    long long frame_stride;
    const float *ftab;         // the float32 cull tables of this scene / camera / depth, built once by tables_kernel
    unsigned long long *ray_counts;   // counting instantiation only (RT_FLAG_COUNT_RAYS): {closest, shadow issued, shadow skipped, hits}
    double *out_f64;           // lattice instantiation: float64 (R,G,B) per lattice sample, [column - x0][row][3]; aa_resolve_kernel reads it
    int lattice;               // 1: the "frame" is the (2w-1) x (2h-1) half-pixel lattice of the pixel grid (w, h, x0, x1 are lattice units)
    int lat_x0, lat_h;         // aa_resolve_kernel: first lattice column in out_f64, lattice rows
    long long plane_stride;    // elements between colour planes of the output
    int w, h, x0, x1;
    int S, P, L, depth;
    int NC;                    // sphere clusters (0 = flat)
    unsigned plane_codes;      // axis codes of planes 0..3, one signed byte each: 0 = general normal, +-(axis+1) = exactly
                               // axis-aligned unit normal.  A kernel argument lives in an SGPR, so the plane tests of
                               // the usual scenes (a floor, a wall) branch on the scalar unit without touching the VALU
    int aa, u8_rgb, tiles_y, ntiles;
    unsigned tiles_y_magic, tiles_y_shift, bpf_magic, bpf_shift;   // div_magic() of tiles_y and bpf (the host fills them)
    int anchors, spp;          // L+1 if the anchored cull table is in use, else 0; samples per pixel (stochastic AA)
    unsigned seed;             // jitter hash seed (stochastic AA)
    int u8_hwc;                // uint8 frame interleaved as [y][x][3] (an image), row pitch = plane_stride pixels
    int lanes_primary;         // MODE 2: lane-owned traversal for the primary rays and their shadow rays too (else from bounce 1 on)
    float extent2, floor_anch; // max squared distance of camera / lights / sphere surfaces from the world origin;
                               // launch-constant floor of the anchored cull (host: 2^-39 (|cam| + 999(depth+1) + extent)²)
    double px, y0, dy, z0, dz;
    double cam_o[3];
    double cam_R[9];
    double amb, lamb;
    double facing_tau;         // margin of the facing certificate (rt_facing.h; host: rt_facing_tau of the floor_anch reach): a light whose
                               // (light - Pt).N is below -facing_tau on every live lane of a wave is skipped before its direction is formed
    union {
        double refl_pow[16];   // kernels without a material table: refl ** (b+1) (the MAT kernels weigh bounces with the table)
        struct {               // LENS kernels (MAT kernels: refl_pow is unused there), rt_set_lens
            double aperture;   // lens radius a > 0
            double focus;      // distance f of the plane of focus along R e_x
            long long mat;     // offset (doubles) in `scene` of the material block with rows of 6 (mat_offset, or a padded copy)
            // TEX kernels (rt_set_scene_textures with a textured object; lens or not, they read `mat` too):
            long long tex;     // offset (doubles) in `scene` of the texture block (tex_doubles)
            const float *texels;   // 16 B per entry: {R,G,B, texture id or -1} float32 of the S + P object slots, then {R,G,B,-} of the scene's texels
            // LIT kernels (rt_set_scene_lighting with a coloured light or a specular row; they are TEX kernels too):
            long long lit;     // offset (doubles) in `scene` of the lighting block (lit_doubles)
            // SKY kernels (rt_set_scene_sky with a sky that is not black; they are LIT kernels too):
            long long sky;     // offset (doubles) in `scene` of the sky block (SKY_DOUBLES)
        } lens;
    };
};

}  // namespace rt
