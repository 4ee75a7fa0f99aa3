// rt_layout.h — the layout of the scene buffer and of a render kernel's LDS image, shared by the host's scene packer
// (rt_scene.h), its launch plan (rt_plan.h) and the render kernels (rt_device.h): record strides, the feature families, the
// sizes and offsets of the buffer's blocks, the float32 tables and the LDS image's size (table_layout, lds_bytes), the tile
// size, the build-time knobs both sides read (RT_CLUSTER_MIN, RT_MAX_CULL_TABLE_BYTES, RT_W_*) and div_magic.
// HIP-free: hipcc and a plain C++17 host compiler both take it (tests/algo/scene_pack_check.cpp and launch_plan_check.cpp
// build the packer and the plan without HIP), so nothing here may name a HIP type or builtin.
#pragma once
#include <stddef.h>

// __host__ __device__ under HIP, nothing for a host compiler
#ifdef __HIPCC__
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

// waves/SIMD the LDS-parked, parked AA and lane-owned kernels are compiled for (render_kernel's __launch_bounds__; rt_plan.h's
// parking rule reads RT_W_LANES)
#ifndef RT_W_PARK
#define RT_W_PARK 7
#endif
#ifndef RT_W_AAPARK
#define RT_W_AAPARK 7   // 72 VGPRs with a few spills (76 B/lane of scratch) still beat 5 waves/SIMD without: -9 %
#endif
#ifndef RT_W_LANES
#define RT_W_LANES 4    // lane-owned traversal (clustered scenes: the LDS image bounds the occupancy at about 4 anyway) wants registers
#endif

namespace rt {

constexpr int TILE = 8;            // 8x8 pixels per wavefront
// Tiles (wavefronts) per workgroup: a template parameter of the kernel, chosen per scene by the host.  Small
// workgroups start and retire at a finer grain (C2: 2 waves beat 4 by 3 %); every workgroup stages its own copy
// of the scene and its cull tables, so bigger scenes want bigger workgroups (C4: 4 waves beat 2 by 24 %, C5 by 69 %).
constexpr int TILE_ORDER_MIN_WPW = 4;   // workgroups of this many waves or more may be dispatched tile by tile (render_kernel, dispatch)
constexpr int BOX_STRIDE = 8;      // floats per cluster box: lo.xyz, -, hi.xyz, - (two ds_read_b128)
constexpr int CULL_STRIDE = 4;     // floats per (anchor, sphere) cull entry: Lx,Ly,Lz, tau (one ds_read_b128)
#ifndef RT_MAX_CULL_TABLE_BYTES
#define RT_MAX_CULL_TABLE_BYTES (40 * 1024)
#endif
constexpr int MAX_CULL_TABLE_BYTES = RT_MAX_CULL_TABLE_BYTES;   // anchored cull table budget per workgroup (LDS)
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
// scene and lens (rt_plan.h: family_of) and runs that family's kernels.
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

// sphere slots in the float32 tables: whole clusters when the scene is clustered, else a multiple of 4
RT_HD inline int padS(int S, int NC) { return NC > 0 ? NC * CLUSTER : pad4(S); }

// LDS image: [float64 records][per-thread slots 6|9 x 256 doubles][256 int32 pixel offsets][float32 sphere table S x 4][cull table anchors x S x CULL_STRIDE]
RT_HD constexpr int lds_slots(bool aa, bool park, bool mode2, Family f) { return (park ? ((aa && !mode2) ? 9 : 6) : 0) + (has_mat(f) ? 3 : 0) + (has_refr(f) ? 4 : 0) + (has_scat(f) ? 2 : 0) + (has_soft(f) ? 1 : 0); }   // x workgroup-size doubles (MODE 2: the tap sums stay in registers; MAT: + W, lamb, refl; REFR: + Q, eta; SCAT: + rough, key; SOFT: + light key)
RT_HD inline int lds_offset_words(bool park, int wgt) { return park ? wgt : 0; }    // + one int32 per thread: the pixel offset
// The float32 tables of a scene, offsets in floats (every one a multiple of 4):
//   sph32 | anchored table | cluster anchored table | cluster boxes | group boxes | group anchored table | cluster sph32 | colours
// (colours: {R,G,B,-} of the S spheres, padded to Sp entries, then of the P planes — exact, the scene is float32; only
// the MODE 1 kernels, which keep no float64 sphere records, stage and read them: `total_col` floats instead of `total`)
// The lane-owned traversal never reads the clusters' origin-form spheres (it tests boxes), so its kernels stage — and
// reserve LDS for — everything but that last table (`lanes`): config 5's image stays under the 4-workgroups-per-CU line.
struct TableLayout { size_t tab, ctab, cbox, gbox, gtab, csph32, total_lanes, total, col32, total_col; };
RT_HD inline TableLayout table_layout(int S, int NC, int anchors, int P = 0)
{
    const size_t Sp = padS(S, NC), NCp = pad4(NC), NG = supers(NC), NGp = pad4((int)NG);
    TableLayout t;
    size_t o = 4 * Sp;
    t.tab = o;    o += (size_t)anchors * Sp * CULL_STRIDE;
    t.ctab = o;   o += (size_t)anchors * NCp * CULL_STRIDE;
    t.cbox = o;   o += NCp * BOX_STRIDE;
    t.gbox = o;   o += NG * BOX_STRIDE;
    t.gtab = o;   o += (size_t)anchors * NGp * CULL_STRIDE;
    t.total_lanes = o;
    t.csph32 = o; o += 4 * NCp;
    t.total = o;
    t.col32 = o;  o += 4 * (Sp + (size_t)pad4(P));
    t.total_col = o;
    return t;
}
// What a two-wave render kernel reads of that layout, in 32-bit arithmetic.  The plan sends two-wave workgroups flat scenes only
// (rt_plan.h: plan_launch, NC == 0) and they are MODE 0 kernels, so the cluster tables and the colour table are empty and never
// read: what is left is `tab` and `total`, and total == total_lanes.  ng > 0 (the small-scene twins; rt_plan.h: cull_groups
// guarantees pad4(S) == 4 ng and anchors == L + 1): `tab` is a constant and `total` one multiply-add of L.
// tests/algo/fixed_path_check.cpp compares both forms with table_layout over every scene the twins are sent, and the plan's
// case grid for a clustered scene in a two-wave shape.
struct FlatLayout { unsigned tab, total; };
RT_HD inline FlatLayout flat_layout(int ng, int S, int L, int anchors)
{
    if (ng > 0) return FlatLayout{16u * (unsigned)ng, 16u * (unsigned)ng * (unsigned)L + 32u * (unsigned)ng};
    const unsigned Sp = (unsigned)pad4(S);
    return FlatLayout{4u * Sp, 4u * Sp + (unsigned)anchors * Sp * CULL_STRIDE};
}
RT_HD inline size_t table_floats(int S, int NC, int anchors, bool lanes = false, bool col = false, int P = 0)
{
    const TableLayout t = table_layout(S, NC, anchors, P);
    return col ? t.total_col : (lanes ? t.total_lanes : t.total);
}
// mode2: the kernels of the large clustered scenes (lane-owned traversal) stage no float64 sphere records (sphere_hot)
// (TEX kernels keep their twins' image, unread parts included: they take every colour from KParams::lens.texels, so the MODE 1
// colour table and the colours of the float64 records are dead weight in theirs — the price of sharing the twins' layout.)
// f, M: the kernels' family and the scene's material count (their image holds the material block, mat_doubles)
RT_HD inline size_t lds_bytes(int S, int P, int L, int NC, int anchors, bool aa, bool park, int wgt, bool lanes = false, bool mode2 = false, bool norec = false,
                              Family f = Family::PLAIN, int M = 0)
{
    return (lds_doubles((mode2 || norec) ? 0 : S, P, L) + (size_t)lds_slots(aa, park, mode2, f) * wgt +
            mat_doubles(M, S, P, f)) * sizeof(double) +
           ((size_t)lds_offset_words(park, wgt) + table_floats(S, NC, anchors, lanes, norec, P)) * sizeof(float) + 16   // + workgroup cost/arrival words
#ifdef RT_REGION_STATS
           + (size_t)(wgt / 64) * 32 * sizeof(unsigned)
#endif
           ;
}

// Division of n < 2^31 by a launch constant d without the backend's 20-instruction sequence (v_rcp_iflag_f32 and two
// correction steps, on the VECTOR unit even for wave-uniform operands): q = mulhi(n, M) >> sh with M = floor(2^(31+l) / d) + 1,
// l = ceil(log2 d), sh = l - 1 — exact because n d < 2^(31+l) (Granlund-Montgomery); d = 1 passes n through.  Every wave
// divides its tile index by the tiles per column, and in multi-frame launches its block index by the blocks per frame,
// twice: 31 of the headline kernel's vector instructions (and as many scalar ones) per wave, C2 -1.5 %, C4 -1.7 %.
// tests/test_host_helpers.py checks the formula exhaustively on small ranges and on random operands.
RT_HD inline void div_magic(unsigned d, unsigned &M, unsigned &sh)
{
    if (d <= 1u) { M = 0u; sh = 0u; return; }
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    M = (unsigned)((1ull << (31 + l)) / d + 1ull);
    sh = l - 1u;
}

}  // namespace rt
