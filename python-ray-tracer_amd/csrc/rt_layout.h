// rt_layout.h — the layout of the scene buffer, shared by the host's scene packer (rt_scene.h) and the render kernels
// (rt_device.h): record strides, the feature families and the sizes and offsets of the buffer's blocks.
// HIP-free: hipcc and a plain C++17 host compiler both take it (tests/algo/scene_pack_check.cpp builds the packer without
// HIP), so nothing here may name a HIP type or builtin.
#pragma once
#include <stddef.h>

// __host__ __device__ under HIP, nothing for a host compiler
#ifdef __HIPCC__
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

namespace rt {

constexpr int SPH_STRIDE = 8;      // doubles per sphere record: cx,cy,cz,r2, R,G,B, caller's index
constexpr int PL_STRIDE = 16;      // ox,oy,oz,nx,ny,nz, Nx,Ny,Nz, bNx,bNy,bNz, R,G,B, axis code (0 general, +-1/2/3 = +-e_x/y/z)
constexpr int LT_STRIDE = 4;       // x,y,z,pad
constexpr int CL_STRIDE = 4;       // cluster bounding sphere: cx,cy,cz,R2 (global memory only; LDS holds the float32 tables)
constexpr int CLUSTER = 8;         // spheres per cluster
#ifndef RT_CLUSTER_MIN
#define RT_CLUSTER_MIN 20   // measured (median-split clusters) against the flat scene: 16 spheres +3 % (the two-wave kernels, flat
                            // scenes only, are faster there), 25 -7 %, 36 -20 %, 49 -17 %, 64 -13 %
#endif
constexpr int CLUSTER_MIN = RT_CLUSTER_MIN;   // scenes with at most this many spheres stay flat
constexpr int SUPER = 8;           // clusters per group of clusters (one more box each: the lane-owned traversal skips whole groups)
constexpr int TEX_STRIDE = 20;     // doubles per texture record: origin[3], axis[3][3], n[3], 1/n[3], base, pad
constexpr int SKY_DOUBLES = 24;    // the sky block (rt_device.h: sky_color has its layout)

// The feature family of a render kernel (its last template argument).  Each family's kernels are the twins of the family before
// it with one more feature; LENS and LENS_SOFT are the lens twins of SCAT and SOFT.  The host derives a launch's family from its
// scene and lens (mi355rt.hip: family_of) and runs that family's kernels.
// TEX_*: the texture twins of SCAT, SOFT, LENS and LENS_SOFT (rt_set_scene_textures with a textured object): the hit's colour is a
// texel chosen at the hit point (texel_of).  They are appended: tools/isa_compare.py matches kernels by the family's number.
// LIT_*: the lighting twins of the four TEX families (rt_set_scene_lighting with a light that is not (1, 1, 1) or a row with
// spec > 0): every light has a colour and a hit a Blinn-Phong highlight (trace_bounce).  Appended too, for the same reason.
// SKY_*: the sky twins of the four LIT families (rt_set_scene_sky with a sky that is not black): a trace that finds nothing
// returns sky_color(d) in place of (0, 0, 0) (trace_bounce).  Appended too, for the same reason.
enum class Family { PLAIN, MAT, REFR, SCAT, SOFT, LENS, LENS_SOFT, TEX_SCAT, TEX_SOFT, TEX_LENS, TEX_LENS_SOFT,
                    LIT_SCAT, LIT_SOFT, LIT_LENS, LIT_LENS_SOFT, SKY_SCAT, SKY_SOFT, SKY_LENS, SKY_LENS_SOFT };
constexpr int FAMILIES = 19;
RT_HD constexpr bool has_mat(Family f) { return f != Family::PLAIN; }
RT_HD constexpr bool has_refr(Family f) { return f >= Family::REFR; }
RT_HD constexpr bool has_scat(Family f) { return f >= Family::SCAT; }
RT_HD constexpr bool has_soft(Family f) { return f == Family::SOFT || f == Family::LENS_SOFT || f == Family::TEX_SOFT || f == Family::TEX_LENS_SOFT || f == Family::LIT_SOFT || f == Family::LIT_LENS_SOFT || f == Family::SKY_SOFT || f == Family::SKY_LENS_SOFT; }
RT_HD constexpr bool has_lens(Family f) { return f == Family::LENS || f == Family::LENS_SOFT || f == Family::TEX_LENS || f == Family::TEX_LENS_SOFT || f == Family::LIT_LENS || f == Family::LIT_LENS_SOFT || f == Family::SKY_LENS || f == Family::SKY_LENS_SOFT; }
RT_HD constexpr bool has_tex(Family f) { return f >= Family::TEX_SCAT; }
RT_HD constexpr bool has_lit(Family f) { return f >= Family::LIT_SCAT; }
RT_HD constexpr bool has_sky(Family f) { return f >= Family::SKY_SCAT; }
RT_HD constexpr int table_cols(Family f) { return has_scat(f) ? 6 : (has_refr(f) ? 5 : 3); }   // doubles per material row its kernels read

RT_HD inline int pad4(int n) { return (n + 3) & ~3; }
RT_HD inline int supers(int NC) { return (NC + SUPER - 1) / SUPER; }   // groups of SUPER clusters

// The packed float64 records at the head of the scene buffer (and of a render kernel's LDS image): S spheres, P planes, L lights.
RT_HD inline size_t lds_doubles(int S, int P, int L) { return (size_t)S * SPH_STRIDE + (size_t)P * PL_STRIDE + (size_t)L * LT_STRIDE; }
// The material block of a scene with materials, behind the packed records (and the cluster records and one spare double):
// M, then the M x table_cols(f) table {amb, lamb, refl} (5 columns, refraction kernels: {amb, lamb, refl, trans, ior}; 6, scatter
// kernels and their twins: ..., rough), then S + P int32
// material ids of the slots (padded to a double), and (has_soft(f): a scene of the area-light kernels) its shadow_samples n.  Material
// kernels stage it at the end of their LDS image.
RT_HD inline size_t mat_offset(int S, int P, int L, int NC) { return lds_doubles(S, P, L) + (size_t)(NC + supers(NC)) * CL_STRIDE + 1; }
RT_HD inline size_t mat_doubles(int M, int S, int P, Family f) { return M > 0 ? 1 + (size_t)table_cols(f) * M + ((size_t)S + P + 1) / 2 + (has_soft(f) ? 1 : 0) : 0; }
// The texture block of a scene with a textured object (KParams::lens.tex): T, then the T records of TEX_STRIDE doubles (texel_of).
RT_HD inline size_t tex_doubles(int T) { return T > 0 ? 1 + (size_t)TEX_STRIDE * T : 0; }
// The lighting block of a scene that runs the LIT kernels (KParams::lens.lit): {e_r, e_g, e_b, -} per light (LT_STRIDE doubles),
// then {spec / n, log2(shin)} per object slot (S spheres in slot order, then P planes).
RT_HD inline size_t lit_doubles(int S, int P, int L) { return (size_t)LT_STRIDE * L + 2 * ((size_t)S + P); }

}  // namespace rt
