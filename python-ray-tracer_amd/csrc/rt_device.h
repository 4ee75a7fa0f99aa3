// rt_device.h — the render kernel for gfx950 (CDNA4): one wavefront per 8x8 pixel tile.
//
// What it computes is the reference's `render` kernel and everything it inlines
// (/root/reference/src/ray_tracing/: kernels.py:6-73, trace.py:7-133, common.py, intersections.py),
// in IEEE float64 with separate multiply/add roundings (this file is compiled with
// -ffp-contract=off), so results are bit-identical to the reference's Python arithmetic.
//
// How it is organised is not the reference's one-thread-per-pixel translation:
//   * a 64-lane wavefront owns an 8x8 tile (8 consecutive y per x-row = the contiguous
//     direction of the (3,w,h) frame); the 2 or 4 waves of a workgroup take tiles consecutive in y;
//   * the scene (float64-widened sphere/plane/light/material records, packed by the host: rt_scene.h) and its float32 cull
//     tables (built once per scene/camera by tables_kernel) are copied once per workgroup into LDS and read
//     with wave-uniform (broadcast) ds_reads;
//   * every scene query normalises its direction ONCE (the reference re-normalises per sphere,
//     intersections.py:13 — same value every time), with an exact two-fma shortcut for
//     already-unit vectors, and works on the quadratic scaled by 1/4 (exact in binary FP); the wave-uniform
//     queries do so only once their cull has left a sphere to test (rt_cull.h: the cull reads the incoming direction);
//   * closest-hit keeps the smallest positive numerator and divides once per query;
//   * shadow queries are any-hit: no sqrt/divide unless a decision is within rounding reach,
//     the sphere loop exits as soon as a wave ballot says every live lane is occluded, and
//     lanes whose Lambert term is not positive (result unused, trace.py:101) do not query;
//   * a conservative float32 pre-test ("cull") per sphere decides, for the whole wave, whether the
//     float64 test can change anything; only spheres some lane might hit get the float64 test.
//     The cull never decides a hit and never feeds a value into the result — it only skips
//     float64 evaluations whose outcome (a miss) it has certified with an explicit error margin;
//   * the kernel is bound by VALU instruction issue (0.79 of the bound priced with measured cycles per instruction class on the
//     headline config: float64 4.1-4.2 cycles, 32-bit 2.2, lane masks 4.1-4.2; profiles/r03_valu_prices.json) with the CU's single
//     scalar ALU as the second bound, so both instruction counts are what the code below economises: lane masks
//     come straight from compares, the cull's mask is built with s_cmp + s_addc, table entries are one
//     ds_read_b128 at an immediate offset of a VGPR-pinned base, wave-uniform facts travel in SGPRs;
//   * no MFMA: there is no dense contraction on this path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rt_kparams.h"  // rt::KParams, the kernels' argument (the host fills it: rt_launch.h)
#include "rt_math.h"     // V3, the seeded bodies of normalize3 / div_inrange / sqrt_inrange / renormalize_unit, the counter hashes, clip_color
#include "rt_cull.h"     // the float32 cull's certificates (RayF, cull_anchored, cull_origin, anchored_tau, CULL_K_*) and the guard for culling on the incoming direction
#include "rt_facing.h"   // the facing certificate of the point-light loop (trace_bounce) and its margin
#include "rt_layout.h"   // record strides, rt::Family, block sizes and offsets, the LDS image's arithmetic (lds_bytes, table_layout, ...), TILE, div_magic:
                         // shared with the host's scene packer (rt_scene.h) and launch plan (rt_plan.h)

#pragma clang fp contract(off)

// Build-time knobs (A/B builds for tools/ab_bench.py); the defaults are the measured best on MI355X:
//   RT_FAST_NORMALIZE   shared-reciprocal normalize instead of sqrt + three divisions (C2 -10 %)
//   RT_FAST_DIVSQRT     0 = the backend's full f64 division / sqrt in the scene queries (div_inrange, sqrt_inrange)
// and, with their defaults in rt_layout.h (the host's launch plan reads them too):
//   RT_CLUSTER_MIN      sphere count above which the scene is stored in clusters of 8
//   RT_MAX_CULL_TABLE_BYTES  LDS budget of a workgroup's anchored cull table
//   RT_W_PARK, RT_W_AAPARK, RT_W_LANES  waves/SIMD the LDS-parked, parked AA and lane-owned variants are compiled for
// and two measurement builds: RT_REGION_STATS (tools/region_stats.py) and RT_LANE_STATS (tools/lane_stats.py).
#ifndef RT_FAST_DIVSQRT
#define RT_FAST_DIVSQRT 1
#endif
#ifndef RT_FAST_NORMALIZE
#define RT_FAST_NORMALIZE 1
#endif
#ifndef RT_FACING_SKIP
#define RT_FACING_SKIP 1     // 0: the point-light loops without the facing certificate (A/B builds)
#endif
#ifndef RT_DEFER_DIRECTION
#define RT_DEFER_DIRECTION 1 // 0: every scene query forms its float64 direction R before its cull (A/B builds); 1: the wave-uniform queries
#endif                       //    form R only when the cull leaves a sphere (closest_spheres, any_spheres_masks; rt_cull.h)
#ifndef RT_DEFER_SHADOW
#define RT_DEFER_SHADOW 1    // 0: only closest_hit defers, any_hit_masks keeps the former order (A/B builds)
#endif

namespace rt {

constexpr int TABLE_THREADS = 256; // tables_kernel's workgroup

__device__ __forceinline__ int div_by(int n, int d, unsigned M, unsigned sh)
{
    return d == 1 ? n : (int)(__umulhi((unsigned)n, M) >> sh);
}

// The four exact-arithmetic shortcuts: rt_math.h has their derivations and their bodies (which the CPU checks of tests/algo run);
// here are the build switches, the wave-uniform guards and the hardware's seeds.
__device__ __forceinline__ V3 normalize3(const V3 &v)
{
#if RT_FAST_NORMALIZE == 0
    return normalize3_generic(v);
#else
    const double nn = v.x * v.x + v.y * v.y + v.z * v.z;
    const double cmin = __builtin_fmin(__builtin_fmin(__builtin_fabs(v.x), __builtin_fabs(v.y)), __builtin_fabs(v.z));
    const bool ok = (cmin >= NORMALIZE_MIN_COMPONENT) && (nn <= NORMALIZE_MAX_NN);   // NaNs fail both
    if (__builtin_amdgcn_ballot_w64(!ok) != 0ull) return normalize3_generic(v);
    return normalize3_seeded(v, nn, __builtin_amdgcn_rsq(nn));
#endif
}
__device__ __forceinline__ double div_inrange(double a, double b)
{
#if RT_FAST_DIVSQRT == 0
    return a / b;
#else
    return div_seeded(a, b, __builtin_amdgcn_rcp(b));
#endif
}
__device__ __forceinline__ double sqrt_inrange(double x)      // x >= 0 (or NaN)
{
#if RT_FAST_DIVSQRT == 0
    return __builtin_sqrt(x);
#else
    return sqrt_seeded(x, __builtin_amdgcn_rsq(x));
#endif
}
__device__ __forceinline__ V3 renormalize_unit(const V3 &d)
{
    const double nn = d.x * d.x + d.y * d.y + d.z * d.z;
    const double e = nn - 1.0;                                     // exact
    if (__builtin_amdgcn_ballot_w64(!(__builtin_fabs(e) < UNIT_WINDOW)) != 0ull) return normalize3_generic(d);
    return renormalize_unit_fast(d, e);
}

enum { HIT_NONE = 0, HIT_SPHERE = 1, HIT_PLANE = 2 };

// A per-lane V3 that lives either in LDS (PARK: slot `slot` of the per-thread area, [component][thread] so
// consecutive lanes hit consecutive banks) or in registers.  Parking long-lived values (the running colour,
// the incoming direction during the light loop, the AA tap sums) is what takes the kernel from 5 to 7
// waves/SIMD; the compiler would otherwise spill them to scratch, i.e. to HBM.  volatile + explicit LDS
// address space: a real ds_read/ds_write round trip through ONE 32-bit address (without volatile the stores
// are forwarded and the values stay in VGPRs; without the address space the accesses become flat).
// Scenes whose LDS image is too large for 6+ workgroups per CU run the register variant (host picks).
typedef __attribute__((address_space(3))) double lds_f64;
// REMAT (MODE 3 = MODE 2 with this; the AA kernels of the large clustered scenes, which run at 128 VGPRs with the most spills,
// take it: config 5 at 4 spp -1.5 %, while the 1 spp kernels lose 0.3 % with it): the slot's address is not kept in a
// register between accesses but re-derived at each one from the wave's index (a scalar) and the lane's number (two v_mbcnt,
// volatile so that the compiler does not hoist and keep them): three instructions per access, one VGPR less across the whole
// bounce.
__device__ __forceinline__ unsigned fresh_lane()
{
    unsigned l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
template <bool PARK, int WGT, bool REMAT = false> struct Park3 {
    volatile lds_f64 *p;
    volatile lds_f64 *sbase;       // REMAT: the slot's first word of this wave (scalar)
    V3 v;
    __device__ __forceinline__ Park3(double *base, int slot, int wave = 0)
        : p(REMAT ? nullptr : (volatile lds_f64 *)base + slot * 3 * WGT + threadIdx.x),
          sbase(REMAT ? (volatile lds_f64 *)base + slot * 3 * WGT + wave * 64 : nullptr), v{0.0, 0.0, 0.0} {}
    __device__ __forceinline__ volatile lds_f64 *at() const { if constexpr (REMAT) return sbase + fresh_lane(); else return p; }
    __device__ __forceinline__ void set(const V3 &a)
    {
        if constexpr (PARK) { volatile lds_f64 *q = at(); q[0] = a.x; q[WGT] = a.y; q[2 * WGT] = a.z; } else v = a;
    }
    __device__ __forceinline__ V3 get() const
    {
        if constexpr (PARK) { volatile lds_f64 *q = at(); return V3{q[0], q[WGT], q[2 * WGT]}; } else return v;
    }
};


// Per-object materials (MAT kernels, rt_set_scene_materials): where a sample finds the hit object's coefficients and keeps
// its running reflection weight W.  An empty struct, and every use a no-op, in the kernels of scenes without materials (PLAIN).
// Three per-thread LDS slots from WSLOT on (lds_slots) hold W, and the Lambert coefficient and reflectivity of the lane's current
// hit, copied there from the table entry once per hit: no VGPR holds a coefficient or the entry's address across the light
// loop (with them in registers seven of the 22 material kernels spilled more than their default twins).  The slots are addressed
// off the same base as the parked colour (an immediate offset) or, FRESH (register variants, REMAT), re-derived from the lane's
// number.  The table and the ids are wave-uniform LDS byte addresses, kept scalar until a hit reads them (see opaque()).
// REFR (refraction kernels, rt_set_scene_materials_ex with a transparent row): rows of 5, {amb, lamb, refl, trans, ior}, and four
// more slots: REFL then holds the hit's continuation weight c (trans for a transparent hit, refl otherwise), Q the unbiased hit
// point moved BIAS against the outward normal (P - BIAS*N, the far side of the surface) and ETA what the continuation after the
// light loop is: 0 a reflection, ior > 0 a refraction through a sphere, -1 a pass through a plane.
// SCAT (scatter kernels, rt_set_scene_materials_scatter with a rough row; REFR too): rows of 6, {amb, lamb, refl, trans, ior,
// rough}, and two more slots: ROUGH, the hit's roughness, and KEY, the sample's pre-hashed key (scatter_key), written once per
// sample and read by the scatter after the light loop (scatter_continue).
// SOFT (area-light kernels, rt_set_scene_area_lights with a radius > 0; SCAT too): one more slot, LKEY, the sample's pre-hashed
// light key (soft_key), read inside the light loop where each shadow sample's point on its light is formed (soft_light_point);
// nsh is the scene's shadow_samples n (the last double of the material block).
// LENS (depth-of-field kernels, rt_set_lens with an aperture > 0; SCAT too): no slot; the primary ray does not start at the
// camera, so trace 0's closest-hit query takes the origin form of the cull (trace_bounce).
// TEX (texture kernels, rt_set_scene_textures with a textured object; SCAT too, and SOFT / LENS as their twins): no slot and no
// LDS: texture records, ids and texels are read from global memory where a hit needs them (texel_of).
// LIT (lighting kernels, rt_set_scene_lighting; TEX too): no slot and no LDS either: the lights' colours and the hit's spec / n
// and log2(shin) are read from the scene's lighting block in global memory inside the light loop (trace_bounce, lit_doubles).
// SKY (sky kernels, rt_set_scene_sky; LIT too): no slot and no LDS: the lanes of a trace that missed read the scene's sky block
// from global memory through wave-uniform addresses (sky_color, SKY_DOUBLES).
template <Family F, int WSLOT, bool FRESH> struct MatState {
    static constexpr bool mat = has_mat(F), refr = has_refr(F), scat = has_scat(F), soft = has_soft(F), lens = has_lens(F), tex = has_tex(F), lit = has_lit(F), sky = has_sky(F);
    static constexpr int COLS = table_cols(F);   // doubles per table row
    unsigned tab;              // LDS: M x {amb, lamb, refl} (REFR: M x {amb, lamb, refl, trans, ior}; SCAT: ..., rough)
    unsigned ids;              // LDS: the material of every slot (S spheres in slot order, then P planes)
    int nsh;                   // SOFT: shadow samples per light (1 otherwise, unused)
    enum { W = 0, LAMB = 1, REFL = 2, QX = 3, QY = 4, QZ = 5, ETA = 6, ROUGH = 7, KEY = 8, LKEY = 9 };
    template <int WGT, int k> __device__ __forceinline__ volatile lds_f64 *at(const double *acc, int wave) const
    {
        if constexpr (FRESH) return (volatile lds_f64 *)acc + (WSLOT + k) * WGT + wave * 64 + fresh_lane();
        else return (volatile lds_f64 *)acc + (WSLOT + k) * WGT + threadIdx.x;
    }
    __device__ __forceinline__ volatile const lds_f64 *entry(int slot) const   // the material of slot `slot`
    {
        unsigned t = tab, i = ids;
        asm volatile("" : "+s"(t), "+s"(i));
        typedef __attribute__((address_space(3))) const int lds_ci32;
        const int m = ((lds_ci32 *)(size_t)i)[slot];
        return (volatile const lds_f64 *)(size_t)t + COLS * m;
    }
};
// SLOT(X): this lane's slot X, for a function that has the MatState as `ms`, the Lds view as `lds` and the workgroup's size as WGT.
// The address is formed at every use (at): the slots are volatile and FRESH re-derives the lane, so no pointer is kept between uses.
#define SLOT(X) (*ms.template at<WGT, MS::X>(lds.acc, lds.wave))
template <int WSLOT, bool FRESH> struct MatState<Family::PLAIN, WSLOT, FRESH> {
    static_assert(!has_mat(Family::PLAIN), "MS::mat is has_mat(family) on both sides: the host folds p.lamb into facing_tau by the same predicate");
    static constexpr bool mat = false, refr = false, scat = false, soft = false, lens = false, tex = false, lit = false, sky = false;
};

// ---------------------------------------------------------------------------------------------
// Conservative float32 cull.  For a ray (o, R) and sphere (c, r2) the reference computes, in
// float64, D = s² - a·(|L|² - r2) with L = o - c, s = L·R, and reports a miss when D < 0, or when
// s >= 0 and |L|² - r2 >= 0 ("behind", see below).  D is r2 minus the squared distance from c to
// the ray's LINE, so it may be evaluated from any point A of the line: D = (A-c)·R)² - |A-c|² + r2.
//
//  * anchored form — every primary ray passes through the camera and every shadow ray through its
//    light, so with A = camera/light the vector A-c, w = r2-|A-c|² and the error margin are
//    constants per (anchor, sphere): a table built once per workgroup in LDS (from float64), and
//    the per-ray work is s' = (A-c)·R32 (3 ops) and ONE compare, |s'| < tau, with
//    tau = sqrt(|A-c|² - r2 - margin - floor) rounded down (D' = s'² + r2 - |A-c|² < -margin - floor);
//  * origin form — for reflection rays, and for the sphere a shadow ray starts on, L = o32 - c is
//    formed per lane; it also certifies "behind" (s > e_s and |L|²-r2 > e_c).
//
// Error budget, u = 2^-24, Λ = |A-c| or |L|: inputs rounded to float32 (relative u each), three
// roundings in each dot product, one in the final fma:
//     anchored: |D' - D| <= u(13Λ² + 2 r2)               margin used: 32u(Λ² + r2)
//     origin:   |D' - D| <= u(19Λ² + 2|o|² + 2 r2)       margin used: 64u(Λ² + |o|² + r2)
//               |s' - s| <= u(|o| + 5Λ)                  margin used:  8u(1 + Λ² + |o|²)
//               |c' - c| <= u(7Λ² + |o|² + r2)           margin used: 64u(Λ² + |o|² + r2)
// plus, in all of them, floor = 2^-40(|o|² + extent²) >= the float64 rounding of the reference's own
// D (<= 2^-50 of its operands) and the distance by which a float64 direction misses its anchor.  The anchored
// form uses a launch constant for it: every ray origin lies within |cam| + 999(depth+1) of the world origin
// (each segment of a path is shorter than the far limit), so floor_anch = 2^-39(|cam| + 999(depth+1) + extent)²
// bounds it for every query of the launch.
// A sphere is skipped only if EVERY live lane holds a certificate; NaNs certify nothing.
// ---------------------------------------------------------------------------------------------
// (the CULL_K_* constants and the certificates' arithmetic — make_rayf_dir, add_origin, anchored_tau, cull_anchored, cull_origin —
// are in rt_cull.h, HIP-free, with the bound for culling on the incoming direction)

// The workgroup's dynamic LDS.  Its base is a link-time constant: reading the float64 records through this symbol (and
// not through a pointer carried in a struct) lets every record access be a ds_read at an immediate offset of the slot
// index — as a carried pointer the base sat in a scalar register that was spilled and re-read (v_readlane + v_mov)
// 33 times in the bundle kernels.
extern __shared__ double lds_raw[];

struct Lds {
    __device__ __forceinline__ const double *recs() const { return lds_raw; }     // float64 records
    const float *sph32;    // Sp x {cx,cy,cz,r2}
    const float *tab;      // anchors x Sp x CULL_STRIDE
    const float *csph32;   // NCp x {cx,cy,cz,R2}: cluster bounding spheres, origin form
    const float *ctab;     // anchors x NCp x CULL_STRIDE: cluster bounding spheres, anchored form
    const float *cbox;     // NCp x BOX_STRIDE: cluster bounding boxes (rounded outward), for rays without an anchor
    const float *gbox;     // supers(NC) x BOX_STRIDE: boxes around groups of SUPER clusters
    const float *gtab;     // anchors x pad4(supers(NC)) x CULL_STRIDE: the groups' bounding spheres, anchored form
    const float *col32;    // (Sp + planes) x {R,G,B,-}: colours (MODE 1 kernels only; nullptr otherwise)
    int NC;
    int wave;              // this wave's index in its workgroup (scalar)
    bool pairs;            // a compile-time constant per kernel: the wave-uniform cull keeps two table entries in flight (cull4)
    bool groups;           // a compile-time constant per kernel: test a chunk's group of clusters before its clusters (MODE 2 kernels)
    bool trim;             // a compile-time constant per kernel: the instruction trims measured on the two-wave kernels without a material
                           // table — shadow queries keep their occlusion flag as one scalar lane mask (any_hit_masks), and a plane with
                           // normal -e_i is tested without negating den and num (plane_den_num)
    bool defer;            // a compile-time constant per kernel: the wave-uniform queries form their float64 direction behind their cull
                           // (closest_spheres, any_spheres_masks).  Not in the lane-owned kernels, whose queries need R before the traversal,
                           // and not in the parked 9-tap kernels (AA && PARK), which run at 72 VGPRs with 68 to 92 B/lane of scratch already:
                           // the PLAIN ones gain 4 to 8 B/lane with it
#ifdef RT_REGION_STATS
    unsigned *reg;         // measurement build: 32 words per wave — cycles per code region [0, 24), bounce class [30], last stamp [31]
#endif
    double *acc;           // 6 (9 with AA) x workgroup-size doubles, [slot][thread] (consecutive lanes -> consecutive banks):
                           // slots 0-2 the running colour of the current sample, 3-5 the incoming direction
                           // during the light loop, 6-8 (AA kernel only) the tap sums — kept out of VGPRs that would stay
                           // live across every query of every bounce (registers decide occupancy here)
};

#ifdef RT_REGION_STATS
// Measurement build only (hipcc -DRT_REGION_STATS, tools/region_stats.py): where a wave's cycles go.  RT_MARK(id) adds the
// shader-clock cycles since the wave's previous mark to region `id` (+ 12 for bounces 2 and later); all active lanes write
// the same values to the wave's words.  Regions: 0 re-normalise (closest), 1 closest: cluster bounds, 2 closest: cluster
// loop (float32 sphere tests + float64 tests), 3 closest: planes + select, 4 hit point / normal, 5 light direction + Lambert,
// 6 re-normalise (shadow), 7 shadow: cluster bounds, 8 shadow: cluster loop, 9 shadow: planes, 10 reflection, 11 the rest.
__device__ __forceinline__ void region_mark(unsigned *reg, int id)
{
    volatile unsigned *r = reg + (threadIdx.x >> 6) * 32;
    const unsigned now = (unsigned)__builtin_amdgcn_s_memtime();
    const unsigned last = r[31], c = r[30];
    r[id + c] = r[id + c] + (now - last);
    r[31] = now;
}
#define RT_MARK(id) region_mark(lds.reg, id)
#else
#define RT_MARK(id)
#endif

// Table entries are read through a 32-bit LDS address that is pinned in a VGPR (the empty asm): the index is
// wave-uniform, and left to itself the compiler forms every entry's address on the scalar unit and moves it
// into a VGPR for its ds_read — one extra VALU instruction per sphere.  With the base in a VGPR the entries of
// a group are immediate offsets of one 16-byte ds_read_b128 each.
typedef __attribute__((address_space(3))) const f4 lds_cf4;
__device__ __forceinline__ lds_cf4 *pin_lds(const float *generic)
{
    unsigned a = (unsigned)(size_t)(__attribute__((address_space(3))) const float *)generic;
    asm volatile("" : "+v"(a));
    return (lds_cf4 *)(size_t)a;
}

// Phase 1 of a scene query: one bit per sphere of the chunk [k0, k0+n), set when SOME live lane holds
// no certificate.  Straight-line float32 work with no dependence between spheres; the mask is
// wave-uniform (it is built from ballots), so phase 2 — the float64 test — runs only for set bits.
// self: the sphere a shadow ray starts on (-1: none), certified by the origin form's "behind" test.
// Lane masks of the cull are produced by the compares themselves (inline asm, one VALU instruction each, result in
// an SGPR pair, zero for inactive lanes), combined on the scalar unit and pushed into the accumulator with
// s_cmp + s_addc:  acc = 2 acc + (some live lane holds no certificate).  Going through bool and a ballot instead
// costs a v_cndmask and a v_cmp per sphere whenever the predicate is more than a single compare, and
// compare + select + shift + or is four scalar instructions where two do.  Each CU has ONE scalar ALU for its four
// SIMDs and this kernel keeps it well over half busy, so scalar instructions are not free here.
// All of these are "not ..." compares: an unordered operand (NaN) yields 1 = no certificate.
typedef unsigned long long lanemask;
__device__ __forceinline__ lanemask m_nlt_abs(float a, float b)   // !(|a| < b)
{
    lanemask m; asm volatile("v_cmp_nlt_f32_e64 %0, |%1|, %2" : "=s"(m) : "v"(a), "v"(b)); return m;
}
__device__ __forceinline__ lanemask m_nlt_neg(float a, float b)   // !(a < -b)
{
    lanemask m; asm volatile("v_cmp_nlt_f32_e64 %0, %1, -%2" : "=s"(m) : "v"(a), "v"(b)); return m;
}
__device__ __forceinline__ lanemask m_ngt(float a, float b)       // !(a > b)
{
    lanemask m; asm volatile("v_cmp_ngt_f32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b)); return m;
}
__device__ __forceinline__ lanemask m_ne(int a, int b)            // a != b
{
    lanemask m; asm volatile("v_cmp_ne_u32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "s"(b)); return m;
}
__device__ __forceinline__ unsigned push_any(unsigned acc, lanemask m)
{
    asm volatile("s_cmp_lg_u64 %1, 0\n\ts_addc_u32 %0, %0, %0" : "+s"(acc) : "s"(m) : "scc");
    return acc;
}

// logarithmic cost key for the dispatch-order feedback: monotone in c, < 1024
__device__ __forceinline__ int order_bucket(unsigned c)
{
    if (c < 32u) return (int)c;
    const int msb = 31 - __builtin_clz(c);
    return ((msb - 4) << 5) | (int)((c >> (msb - 5)) & 31u);
}
// dispatch-order feedback (order_kernel)
constexpr int ORDER_THREADS = 1024, ORDER_BUCKETS = 1024, ORDER_XCDS = 8;


// ---------------------------------------------------------------------------------------------
// Slab test of a ray without an anchor (o, R) against a cluster's bounding box, float32, conservative: a certificate
// that the reference reports a miss for EVERY sphere in the box.
//   exact geometry: if the half-line o + tR, t >= 0, stays at least d outside the box, it stays d outside every sphere
//   in it, so the reference's D = r2 - (distance to the line)^2 < -d^2 (or both roots lie behind the origin by d): its own
//   float64 rounding (<= 2^-40 (|o|^2 + extent^2), the `floor` of the sphere certificates) cannot turn that into a hit
//   once d >= 2^-20 sqrt(|o|^2 + extent^2);
//   float32 ray: o and R rounded to float32 move a point of the ray at parameter t by at most 2^-24 (|o| + t), and every t
//   that matters is below |o| + extent;
//   both are covered by growing the box by m = 2^-18 (extent + |o|_1) on every side — done on the ray instead: the lower
//   faces are tested from o + m, the upper ones from o - m;
//   float32 arithmetic: a face's parameter is t = fma(face, inv, c), inv = rcp(R_i) (1 ulp; measured 0.88), c = -(o_i +- m) inv rounded:
//   t carries a relative error below 2^-21 and an absolute one below 2^-23 |c|; c is moved by 2^-21 |c| in the direction
//   that lowers the near parameter and raises the far one, and the final comparison allows 2^-18 relative.
//   R_i = 0 is replaced by +-2^-40 (a change of direction far below the float32 rounding already covered).
// Miss certificate: tfar < max(tnear (1 - 2^-18), 0).  NaN operands never certify (the caller opens everything).
// 17 VALU instructions per box, as many as the bounding-SPHERE test it replaces, for a bound several times tighter around
// flat or elongated clusters.
// ---------------------------------------------------------------------------------------------
struct RayBox { F3 inv, clo, chi; bool sane; };
__device__ __forceinline__ float vmin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float vmax3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ void raybox_axis(float o, float R, float m, float &inv, float &clo, float &chi)
{
    const float Rs = __builtin_fabsf(R) < 0x1p-40f ? __builtin_copysignf(0x1p-40f, R) : R;
    inv = __builtin_amdgcn_rcpf(Rs);
    const float a = -((o + m) * inv), b = -((o - m) * inv);     // lower faces from o + m, upper faces from o - m
    const float da = __builtin_fabsf(a) * 0x1p-21f, db = __builtin_fabsf(b) * 0x1p-21f;
    // inv > 0: the lower face is the near one (its parameter goes down, the upper face's up); inv < 0: the other way round
    clo = inv > 0.0f ? a - da : a + da;
    chi = inv > 0.0f ? b + db : b - db;
}
__device__ __forceinline__ RayBox make_raybox(const RayF &q, float extent2)   // q with its origin (add_origin)
{
    RayBox rb;
    const float m = 0x1p-18f * (__builtin_sqrtf(extent2) + (__builtin_fabsf(q.o.x) + __builtin_fabsf(q.o.y) + __builtin_fabsf(q.o.z)));
    raybox_axis(q.o.x, q.R.x, m, rb.inv.x, rb.clo.x, rb.chi.x);
    raybox_axis(q.o.y, q.R.y, m, rb.inv.y, rb.clo.y, rb.chi.y);
    raybox_axis(q.o.z, q.R.z, m, rb.inv.z, rb.clo.z, rb.chi.z);
    const float chk = (q.o.x + q.o.y + q.o.z) + (q.R.x + q.R.y + q.R.z);
    rb.sane = (chk == chk) && __builtin_fabsf(chk) < 0x1p100f;                // no NaN, no infinity among the six
    return rb;
}
__device__ __forceinline__ bool box_open(const f4 lo, const f4 hi, const RayBox &rb)   // true = NO certificate
{
    const float ax = __builtin_fmaf(lo[0], rb.inv.x, rb.clo.x), bx = __builtin_fmaf(hi[0], rb.inv.x, rb.chi.x);
    const float ay = __builtin_fmaf(lo[1], rb.inv.y, rb.clo.y), by = __builtin_fmaf(hi[1], rb.inv.y, rb.chi.y);
    const float az = __builtin_fmaf(lo[2], rb.inv.z, rb.clo.z), bz = __builtin_fmaf(hi[2], rb.inv.z, rb.chi.z);
    const float tn = vmax3(vmin(ax, bx), vmin(ay, by), vmin(az, bz));
    const float tf = vmin3(vmax(ax, bx), vmax(ay, by), vmax(az, bz));
    return !(tf < vmax(tn * (1.0f - 0x1p-18f), 0.0f));
}

// Certificates of 4 consecutive table entries -> 4 mask bits (bit u set = some live lane has no certificate).
// The tables are padded with entries that always certify a miss (tau = +inf, r2 = -inf), so groups of 4 need no
// bounds handling and use immediate LDS offsets.
// Returns 16 acc + bits (entries are visited from the highest to the lowest).
// PAIRS: two entries are read before either is tested — one LDS round trip per two tests instead of one per test, for four more
// live VGPRs.  The wave-uniform kernels take it (config 4 -2.7 %, 36 ... 144 spheres -3 ... -5 %, 16 spheres -3 %, the headline -0.6 %,
// the 9-tap kernels -0.7 ... -2.6 %); the lane-owned kernels, which run
// this cull for their primary rays at 128 VGPRs with spills, lose 0.8 % with it and keep one entry in flight.
template <bool ANCH, bool SELF, bool PAIRS>
__device__ __forceinline__ unsigned cull4(lds_cf4 *base, const RayF &q, int jsel, unsigned acc)
{
    static_assert(CULL_STRIDE == 4, "one 16-byte entry per (anchor, sphere)");
    f4 pending = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int u = 3; u >= 0; --u) {
        f4 e;
        if constexpr (PAIRS) {
            if (u & 1) {
                asm volatile("" ::: "memory");
                e = base[u];
                f4 enext = base[u - 1];
                asm volatile("" : "+v"(e), "+v"(enext));      // both loaded before either is used
                pending = enext;
            } else e = pending;
        } else {
            asm volatile("" ::: "memory");                    // one entry in flight (registers decide occupancy)
            e = base[u];
        }
        lanemask open;                                        // live lanes without a certificate for this entry
        if constexpr (ANCH) {
            const float sd = __builtin_fmaf(e[2], q.R.z, __builtin_fmaf(e[1], q.R.y, e[0] * q.R.x));
            open = m_nlt_abs(sd, e[3]);                       // cull_anchored()
        } else {                                              // cull_origin()
            const float lx = q.o.x - e[0], ly = q.o.y - e[1], lz = q.o.z - e[2];
            const float sd = __builtin_fmaf(lz, q.R.z, __builtin_fmaf(ly, q.R.y, lx * q.R.x));
            const float ll = __builtin_fmaf(lz, lz, __builtin_fmaf(ly, ly, lx * lx));
            const float cc = ll - e[3];
            const float D = __builtin_fmaf(sd, sd, -cc);
            const float mg = __builtin_fmaf(CULL_K_ORIGIN, ll + e[3], q.mgq);
            const float es = __builtin_fmaf(CULL_K_S, ll, q.esq);
            open = m_nlt_neg(D, mg) & (m_ngt(sd, es) | m_ngt(cc, mg));
        }
        if constexpr (SELF) open &= m_ne(jsel, u);            // the sphere this lane's shadow ray starts on
        acc = push_any(acc, open);
    }
    return acc;
}

// Phase 1 of a scene query for the chunk of spheres [k0, k0+n), k0 a multiple of 64: one bit per sphere, set
// when SOME live lane holds no certificate.  Clustered scenes first test the (up to 8) bounding spheres of the
// chunk's clusters and only open the clusters some lane might hit.  Everything here is wave-uniform control
// flow on scalar masks.
// NG > 0 (the small-scene kernels: render_kernel's last template argument; rt_plan.h: cull_groups picks them): the scene is flat and
// has at most 4 NG spheres, so its table rows are exactly NG groups of four (padS(S, 0) = pad4(S) = 4 NG), k0 is 0 and n is S.  The
// cull is then NG chained cull4 calls, highest group first, as the clustered branch chains `hi` into `lohi`: no loop, no shift by a
// register, no pointer advance, immediate LDS offsets.  The same compares on the same entries in the same order.
template <bool ANCH, bool SELF, int NG = 0>
__device__ __forceinline__ unsigned long long cull_mask_t(const Lds &lds, int S, int anchor, int k0, int n,
                                                          const RayF &q, int selfj)
{
    if constexpr (NG > 0) {
        lds_cf4 *sbase = pin_lds(ANCH ? lds.tab + (size_t)anchor * (4 * NG) * CULL_STRIDE : lds.sph32);
        unsigned m = 0u;
#pragma unroll
        for (int g = NG - 1; g >= 0; --g)
            m = lds.pairs ? cull4<ANCH, SELF, true>(sbase + 4 * g, q, selfj - 4 * g, m) : cull4<ANCH, SELF, false>(sbase + 4 * g, q, selfj - 4 * g, m);
        return m;
    }
    unsigned long long mask = 0ull;
    const int Sp = padS(S, lds.NC);
    lds_cf4 *sbase = pin_lds(ANCH ? lds.tab + ((size_t)anchor * Sp + k0) * CULL_STRIDE : lds.sph32 + 4 * k0);
    if (lds.NC > 0) {
        const int NCp = pad4(lds.NC), c0 = k0 / CLUSTER, nc = (n + CLUSTER - 1) / CLUSTER;
        if (ANCH && lds.groups) {                                             // the chunk's 8 clusters are one group: is any lane's ray near it at all?
                                                                              // (the kernels of the large scenes only: 196 spheres -3 %, 256 -4 %; 36-100 spheres +0.4..+1.6 %)
            static_assert(CLUSTER * SUPER == 64, "a 64-sphere chunk is one group of clusters");
            const f4 ge = *pin_lds(lds.gtab + ((size_t)anchor * pad4(supers(lds.NC)) + (k0 >> 6)) * CULL_STRIDE);
            const float gs = __builtin_fmaf(ge[2], q.R.z, __builtin_fmaf(ge[1], q.R.y, ge[0] * q.R.x));
            if (m_nlt_abs(gs, ge[3]) == 0ull) return 0ull;
        }
        // (the clusters' BOXES, which the lane-owned traversal tests for rays without an anchor, were tried here too: the
        // extra live values cost the wave-uniform kernels more in spills than the tighter bound saves: 36-100 spheres
        // +9..+20 %)
        lds_cf4 *cbase = pin_lds(ANCH ? lds.ctab + ((size_t)anchor * NCp + c0) * CULL_STRIDE : lds.csph32 + 4 * c0);
        unsigned cm = 0;
        for (int j = 0; j < nc; j += 4) cm |= (lds.pairs ? cull4<ANCH, false, true>(cbase + j, q, -1, 0u) : cull4<ANCH, false, false>(cbase + j, q, -1, 0u)) << j;
        while (cm) {                                                          // clusters some lane might hit
            const int c = __builtin_ctz(cm);
            cm &= cm - 1u;
            const int jb = c * CLUSTER;
            const unsigned hi = lds.pairs ? cull4<ANCH, SELF, true>(sbase + jb + 4, q, selfj - jb - 4, 0u) : cull4<ANCH, SELF, false>(sbase + jb + 4, q, selfj - jb - 4, 0u);
            const unsigned lohi = lds.pairs ? cull4<ANCH, SELF, true>(sbase + jb, q, selfj - jb, hi) : cull4<ANCH, SELF, false>(sbase + jb, q, selfj - jb, hi);
            mask |= (unsigned long long)lohi << jb;
        }
    } else {
        const int npad = pad4(n);
        for (int j = 0; j < npad; j += 4) mask |= (unsigned long long)(lds.pairs ? cull4<ANCH, SELF, true>(sbase + j, q, selfj - j, 0u) : cull4<ANCH, SELF, false>(sbase + j, q, selfj - j, 0u)) << j;
    }
    return mask;
}

// dir: the float32 direction the certificates read — float32(R), or float32(d) of a wave inside the unit window (rt_cull.h)
// NG > 0 (cull_mask_t): one chunk, k0 = 0 and n = S, so a sphere index is in the chunk's window exactly when it is one (self >= 0).
template <int NG = 0>
__device__ __forceinline__ unsigned long long cull_mask(const Lds &lds, int S, int anchor, int k0, int n,
                                                        const V3 &o, const F3 &dir, float extent2, int self)
{
    RayF q = make_rayf_dir(dir);
    if (anchor >= 0) {
        const bool cand = NG > 0 ? self >= 0 : (self >= k0 && self < k0 + n);  // per lane
        if (__builtin_amdgcn_ballot_w64(cand) != 0ull) {                                         // only shadow rays leaving a sphere
            add_origin(q, o, extent2);
            const float *cs = lds.sph32 + 4 * self;
            const bool self_culled = cand ? cull_origin(f4{cs[0], cs[1], cs[2], cs[3]}, q) : false;
            if (__builtin_amdgcn_ballot_w64(self_culled) != 0ull)
                return cull_mask_t<true, true, NG>(lds, S, anchor, k0, n, q, self_culled ? self - k0 : -1);
        }
        return cull_mask_t<true, false, NG>(lds, S, anchor, k0, n, q, -1);
    }
    add_origin(q, o, extent2);
    return cull_mask_t<false, false, NG>(lds, S, anchor, k0, n, q, -1);
}

template <int NG = 0>
__device__ __forceinline__ unsigned long long cull_mask(const Lds &lds, int S, int anchor, int k0, int n,
                                                        const V3 &o, const V3 &R, float extent2, int self)
{
    return cull_mask<NG>(lds, S, anchor, k0, n, o, cull_dir32(R), extent2, self);
}

// ---------------------------------------------------------------------------------------------
// Sphere test, intersections.py:6-38, restated on the quadratic divided by 4.
//   reference:  b = 2s, disc = b*b - (4a)*c, num = -b -/+ sqrt(disc), t = num / (2a)
//   here:       D = s*s - a*c,  q = sqrt(D),  n = -s -/+ q,           t = n / a
// Scaling by powers of two commutes with every rounding involved (no overflow/underflow at
// scene magnitudes): disc = 4D, sqrt(disc) = 2q, num = 2n, t identical bit for bit.
// "Behind" rule: if s >= 0 and c >= 0 then D <= fl(s*s), so q <= s and both numerators are <= 0:
// the reference returns a miss, and so do we without evaluating the sqrt.
// ---------------------------------------------------------------------------------------------

// intersections.py:52 and :59-61 for one plane record: den = d.n and num = (p0 - o).n.  A plane whose stored
// normal is exactly +-e_i (the reference's ground plane is (0,0,1)) has den = +-d_i and num = +-(p0_i - o_i)
// bit for bit — the other two products are +-0 and add nothing — so 8 of the 13 operations are skipped under a
// wave-uniform branch on the record's axis code (set by the host).
// axis code of plane k from the kernel argument (planes 4.. use the general formula, which is exact for them too)
// A wave-uniform kernel argument made opaque at its point of use: the value stays where it is (a scalar register), but
// what is derived from it (a comparison, a select) is re-derived there with scalar instructions instead of being hoisted
// out of the bounce loop into scalar registers the kernel does not have — hoisted values come back as v_readlane, a VALU
// slot each, at every use.
__device__ __forceinline__ int opaque(int x)
{
    asm volatile("" : "+s"(x));
    return x;
}

// The kernels whose once-per-tile path (render_kernel's prologue, pixel_P, trace_bounce's light base, store_pixel) is compiled in
// its trimmed form; the others keep the general one, instruction for instruction.  The trims are worth a few dozen scalar
// instructions per wave, which only a kernel on its instruction-issue bound feels, and every one of them moves the register
// allocation of the kernels it touches (tools/isa_compare.py: applied everywhere, more than half of the library's kernels
// gained a spilled scalar or vector register): so they go to the kernels they were measured on and cost nothing anywhere else.
// RT_TRIM_*: build-time overrides, for measuring a wider choice (profiles/fixed_path_items.txt has the ones tried).
#ifndef RT_TRIM_PATH
#define RT_TRIM_PATH(WPW, GROUND, NG) ((NG) > 0)       // prologue (layout, cost words, frame index), light base, facing margin
#endif
#ifndef RT_TRIM_RAY
#define RT_TRIM_RAY(WPW, GROUND, NG) ((NG) > 0)        // pixel_P: px as a scalar value
#endif
#ifndef RT_TRIM_STORE
#define RT_TRIM_STORE(WPW, GROUND, NG) ((NG) > 0)      // store_pixel: the straight-line clip, one address stepped from plane to plane
#endif
#ifndef RT_TRIM_RESOLVE
#define RT_TRIM_RESOLVE false                          // aa_resolve_kernel's store_pixel
#endif

// What a kernel's scene queries are compiled for, as one type handed down from the kernel (render_kernel's MODE, GROUND and NG;
// guides_kernel's MODE) through sample and trace_bounce to closest_hit, any_hit, any_hit_masks, plane_code and plane_count: a
// further axis of specialisation is a member here, not a parameter of each of them.
template <int MODE_, bool GROUND_ = false, int NG_ = 0>
struct Query {
    static constexpr int MODE = MODE_;          // 0: wave-uniform cull; 1: the same without float64 sphere records in LDS (sphere_hot); 2: lane-owned traversal of a clustered scene, also without; 3: 2 with re-derived park addresses (Park3)
    static constexpr bool GROUND = GROUND_;     // the one plane is the z-up ground (below)
    static constexpr int NG = NG_;              // > 0: the scene's spheres are that many cull groups of four (cull_mask_t)
    template <int WPW> static constexpr bool trim() { return RT_TRIM_PATH(WPW, GROUND_, NG_); }   // (above)
    static_assert(NG == 0 || (NG <= 2 && GROUND && MODE == 0), "small-scene kernels are wave-uniform (MODE 0) ground-plane kernels of one or two cull groups");
};

// GROUND (the ground-plane kernels: render_kernel's last template argument; rt_plan.h: ground_plane picks them): the scene has
// exactly one plane and its stored normal is (0,0,1), the reference's ground.  The queries then take P as 1 (plane_count) and the axis
// code as +3: no loop over the planes, no decode of the packed codes, no chain of wave-uniform branches on the code, and the one
// record at a fixed address.  The arithmetic is plane_den_num's z-branch, unchanged.  A template argument, not a flag in Lds like
// trim and defer: the feature kernels call the queries from lambdas, which are simplified before they are inlined, and a flag read
// through `lds` there is folded too late to leave their instruction streams as they were.
template <class Q> __device__ __forceinline__ int plane_code(const KParams &p, int k)
{
    if constexpr (Q::GROUND) return 3;
    // the decoded code and the booleans derived from it are loop-invariant, and the compiler hoists them out of the bounce
    // loop — into scalar registers it does not have: they come back as v_readlane (a VALU slot each) at every use.
    // Re-deriving them from the one kernel-argument word costs scalar instructions only.
    unsigned c = p.plane_codes;
    asm volatile("" : "+s"(c));
    return k < 4 ? (int)(signed char)(c >> (8 * k)) : 0;
}

// The number of planes a query tests: the kernel argument, opaque (above), or the constant 1 of the ground-plane kernels.
template <class Q> __device__ __forceinline__ int plane_count(const KParams &p)
{
    if constexpr (Q::GROUND) return 1;
    else return opaque(p.P);
}

// The cull anchor of a query: the caller's where the launch has anchored tables, else none.
// (NG > 0: anchored tables are part of the predicate, rt_plan.h: cull_groups)
template <class Q> __device__ __forceinline__ int cull_anchor(const KParams &p, int anchor)
{
    return (Q::NG > 0 || opaque(p.anchors) > 0) ? anchor : -1;
}

// no_negate (Lds::trim): for a normal -e_i both den and num are negated, and everything a query does with the pair is the same for
// (-den, -num) as for (den, num) — |den| < 0.001, |num| against |den|, whether the signs agree, and the quotient bit for bit
// (IEEE division, and div_inrange: rcp is odd and each of its steps negates exactly, and a zero quotient has IEEE's sign in both).
// Leaving the negation out saves two v_xor and two v_cndmask per test, for either sign of the code.
// tests/algo/plane_sign_check.cpp restates it (with div_inrange as rt_math.h has it).
__device__ __forceinline__ void plane_den_num(const double *__restrict__ g, int code, const V3 &o, const V3 &d, double &den, double &num,
                                              bool no_negate = false)
{
    if (code == 0) {
        const V3 n{g[3], g[4], g[5]};
        den = dot3(d, n);
        const V3 LP{g[0] - o.x, g[1] - o.y, g[2] - o.z};
        num = dot3(LP, n);
    } else {
        const int a = code < 0 ? -code : code;
        double dc, lp;
        if (a == 1)      { dc = d.x; lp = g[0] - o.x; }
        else if (a == 2) { dc = d.y; lp = g[1] - o.y; }
        else             { dc = d.z; lp = g[2] - o.z; }
        if (code > 0 || no_negate) { den = dc; num = lp; } else { den = -dc; num = -lp; }
    }
}

// What a sphere test reads of sphere slot k: centre and r*r.  F32 (the kernels of the large clustered scenes, MODE 2): from
// the float32 table the cull already keeps in LDS, widened on use — the scene IS float32 (scene.py:18) and r*r is a float32
// product (intersections.py:21), so the widening is exact; those kernels stage no float64 sphere records at all (config 5:
// 16 KB of LDS, which is what lets their long-lived state be parked in LDS instead of spilling to scratch), and read a hit
// sphere's colour and caller's index from the packed scene in global memory, at the point of use.
struct SphHot { double x, y, z, r2; };
template <bool F32> __device__ __forceinline__ SphHot sphere_hot(const Lds &lds, int k)
{
    if constexpr (F32) {
        const f4 c = *(lds_cf4 *)(size_t)(unsigned)(size_t)(__attribute__((address_space(3))) const float *)(lds.sph32 + 4 * k);
        return SphHot{(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
    } else {
        const double *g = lds.recs() + k * SPH_STRIDE;
        return SphHot{g[0], g[1], g[2], g[3]};
    }
}
template <bool F32> __device__ __forceinline__ double sphere_orig(const Lds &lds, const KParams &p, int k)   // the caller's index of slot k
{
    if constexpr (F32) return p.scene[(size_t)k * SPH_STRIDE + 7]; else return lds.recs()[k * SPH_STRIDE + 7];
}

// intersections.py:6-38 for the sphere in slot k (float64), on the quadratic divided by 4 (see above), feeding the
// closest-hit selection: bestn = numerator of the current winner, bidx its slot.
template <bool F32>
__device__ __forceinline__ void sphere_closest(const Lds &lds, const KParams &p, int k, const V3 &o, const V3 &R, double a,
                                               double &bestn, int &bidx)
{
    const SphHot g = sphere_hot<F32>(lds, k);
    const V3 Lv{o.x - g.x, o.y - g.y, o.z - g.z};            // :16
    const double s = dot3(Lv, R);                             // b/2
    const double cc = dot3(Lv, Lv) - g.r2;                    // :21 (r2 = float32 r*r, widened)
    const double D = s * s - a * cc;                          // disc/4
    if (D >= 0.0 && !(s >= 0.0 && cc >= 0.0)) {
        const double q = sqrt_inrange(D);
        double n = -s - q;                                    // :28
        if (!(n > 0.0)) n = -s + q;                           // :33
        // The reference compares the rounded quotients t = n/a with a strict `best > t`, in ascending caller
        // index (trace.py:26): the smallest t wins and, among equal t, the lowest index.  Division by the
        // common a > 0 and rounding are monotone, so numerators order the quotients — except that two
        // numerators within a couple of ulp of each other may round to the SAME quotient, where the index
        // decides.  Numerators further apart than a relative 2^-50 have different quotients in the same
        // order (the gap is four ulp); for closer ones (equal included) both quotients are formed and the
        // reference's rule is applied literally.  Wave-uniform branch, practically never taken.
        // Slots are visited in any order (clustered scenes permute them): the records keep the caller's index, which is
        // looked up only here, for the two spheres of a tie.
        if (n > 0.0) {
            bool take = n < bestn;
            const bool close = __builtin_fabs(n - bestn) < bestn * 0x1p-50;   // false while bestn = +inf (bidx = -1)
            if (__builtin_amdgcn_ballot_w64(close) != 0ull) {
                if (close) {
                    const double tq = n / a, tb = bestn / a;                  // :31 / :36
                    take = tq < tb || (tq == tb && sphere_orig<F32>(lds, p, k) < sphere_orig<F32>(lds, p, bidx));
                }
            }
            if (take) { bestn = n; bidx = k; }
        }
    }
}

// the same sphere for a shadow (any-hit) query: does it report 0 < t < 999?
template <bool F32>
__device__ __forceinline__ bool sphere_any(const Lds &lds, int k, const V3 &o, const V3 &R, double a, bool a_sane)
{
    const SphHot g = sphere_hot<F32>(lds, k);
    const V3 Lv{o.x - g.x, o.y - g.y, o.z - g.z};
    const double s = dot3(Lv, R);
    const double cc = dot3(Lv, Lv) - g.r2;
    const double D = s * s - a * cc;
    if (D >= 0.0 && !(s >= 0.0 && cc >= 0.0)) {
        // s < 0: the larger numerator n2 = -s + q is positive, so a positive root exists and
        // the reference's t is at most n2/a.  n2 <= 998 (from -s < 499, q <= 499) and a within
        // 1e-6 of 1 give t < 999: occluded, decided without sqrt or divide.
        if (s < 0.0 && -s < 499.0 && D < 249001.0 && a_sane) return true;
        const double q = __builtin_sqrt(D);                   // origin inside the sphere, or a far hit: exact path (rare: the generic forms — with the in-range ones here the headline kernel's register allocation tips, +2.4 %)
        double n = -s - q;
        if (!(n > 0.0)) n = -s + q;
        if (n > 0.0) {
            const double t = n / a;
            if (999.0 > t && t > 0.0) return true;
        }
    }
    return false;
}

// The lanes of a scalar lane mask, back as a per-lane bool (one v_cndmask; only where a rare per-lane path is entered).
__device__ __forceinline__ bool lane_of(lanemask m)
{
    unsigned x; asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(x) : "s"(m)); return x != 0u;
}
__device__ __forceinline__ lanemask lanes_where(bool c) { return __builtin_amdgcn_ballot_w64(c); }   // of a plain compare: the v_cmp itself

// sphere_any for the whole wave at once: the live lanes for which the sphere reports 0 < t < 999, as a lane mask.  The same
// compares, each written straight into a scalar register pair and combined on the scalar unit: as nested per-lane conditions
// every level is an exec-mask region (s_and_saveexec, a branch, s_or exec) and the bool that leaves them a v_cndmask + v_cmp
// pair at every use.  D >= 0 rules out a NaN s (it would have made D a NaN), so under it !(s >= 0) is s < 0.
// a_sane: the lanes whose a is within 1e-6 of 1.  The exact path (origin inside the sphere, a far hit) is entered by the
// wave only if some lane needs it.
template <bool F32>
__device__ __forceinline__ lanemask sphere_any_mask(const Lds &lds, int k, const V3 &o, const V3 &R, double a, lanemask a_sane)
{
    const SphHot g = sphere_hot<F32>(lds, k);
    const V3 Lv{o.x - g.x, o.y - g.y, o.z - g.z};
    const double s = dot3(Lv, R);
    const double cc = dot3(Lv, Lv) - g.r2;
    const double D = s * s - a * cc;
    const lanemask dpos = lanes_where(D >= 0.0), sneg = lanes_where(s < 0.0);
    const lanemask cand = dpos & (sneg | lanes_where(!(cc >= 0.0)));          // D >= 0 && !(s >= 0 && cc >= 0)
    const lanemask fast = dpos & sneg & lanes_where(-s < 499.0) & lanes_where(D < 249001.0) & a_sane;   // see sphere_any
    lanemask hit = fast;
    const lanemask slow = cand & ~fast;
    if (slow != 0ull) {
        bool h = false;
        if (lane_of(slow)) {
            const double q = __builtin_sqrt(D);
            double n = -s - q;
            if (!(n > 0.0)) n = -s + q;
            if (n > 0.0) {
                const double t = n / a;
                h = 999.0 > t && t > 0.0;
            }
        }
        hit |= lanes_where(h);
    }
    return hit;
}


// ---------------------------------------------------------------------------------------------
// Lane-owned traversal of clustered scenes (more than CLUSTER_MIN spheres; the LANES instantiations).
// The wave-uniform cull above opens a cluster for the WHOLE wave as soon as one lane's ray might reach it, and gives
// every sphere of an opened cluster its per-ray float32 test and — if one lane lacks a certificate — its float64
// test for all lanes.  That is the right trade while the 64 rays travel together (primary rays, first shadow rays).
// After a few bounces they do not: every lane's ray opens its own 2-4 clusters, the union over the wave approaches
// ALL of them, and a wave with 20 rays left pays for hundreds of sphere tests none of its rays needs (measured on
// config 5: 3x the instructions per wave at bounce 8 compared with bounce 2).
// Here each lane keeps its own candidates: phase 1 tests the cluster bounds in a wave-uniform loop as before but
// leaves one bit per cluster IN THE LANE; then the wave loops while any lane has a cluster left, every lane taking
// ITS next cluster (per-lane LDS addresses: each lane reads the table entries and records of its own spheres),
// running the 8 float32 tests into a per-lane survivor mask, and looping again over its own survivors for the
// float64 test.  Iterations = the MAXIMUM over the lanes of their own counts, not the size of the union.
// Same certificates, same float64 arithmetic, same tie rule (explicit caller's index), any visiting order.
// ---------------------------------------------------------------------------------------------
template <bool ANCH>
__device__ __forceinline__ bool lane_open(const f4 e, const RayF &q)          // true = this lane holds NO certificate
{
    if constexpr (ANCH) {
        const float sd = __builtin_fmaf(e[2], q.R.z, __builtin_fmaf(e[1], q.R.y, e[0] * q.R.x));
        return !(__builtin_fabsf(sd) < e[3]);                                 // cull_anchored()
    } else return !cull_origin(e, q);
}
__device__ __forceinline__ lds_cf4 *lds_f4(const float *generic)             // per-lane LDS address of a table entry
{
    return (lds_cf4 *)(size_t)(unsigned)(size_t)(__attribute__((address_space(3))) const float *)generic;
}

// One bit per cluster bound of the block [cb, cb + nc), nc <= 32: set where THIS lane's ray lacks a certificate.
// Anchored rays: the bounding spheres' table of the anchor (a dot product and a compare each); the others: the boxes.
template <bool ANCH>
__device__ __forceinline__ unsigned lane_cluster_bits(const Lds &lds, int anchor, int cb, int nc, const RayF &q, float extent2)
{
    unsigned cm = 0u;
    if constexpr (ANCH) {
        const int NCp = pad4(lds.NC), NGp = pad4(supers(lds.NC));
        lds_cf4 *base = pin_lds(lds.ctab + ((size_t)anchor * NCp + cb) * CULL_STRIDE);
        lds_cf4 *gbase = pin_lds(lds.gtab + ((size_t)anchor * NGp + cb / SUPER) * CULL_STRIDE);
        for (int c0 = 0; c0 < nc; c0 += SUPER) {                             // a group no lane's ray comes near is skipped whole
            if (__builtin_amdgcn_ballot_w64(lane_open<true>(gbase[c0 / SUPER], q)) == 0ull) continue;
            const int c1 = c0 + SUPER < nc ? c0 + SUPER : nc;
            for (int c = c0; c < c1; c += 4) {                                // tables are padded to a multiple of 4
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    asm volatile("" ::: "memory");
                    const f4 e = base[c + u];
                    cm |= lane_open<true>(e, q) ? (1u << (c + u)) : 0u;
                }
            }
        }
    } else {
        const RayBox rb = make_raybox(q, extent2);
        lds_cf4 *base = pin_lds(lds.cbox + (size_t)cb * BOX_STRIDE);
        lds_cf4 *gbase = pin_lds(lds.gbox + (size_t)(cb / SUPER) * BOX_STRIDE);
        static_assert(SUPER == 8, "a group's clusters are one byte of the mask");
        for (int c0 = 0; c0 < nc; c0 += SUPER) {                             // a group no lane's ray enters is skipped whole
            const bool gopen = box_open(gbase[2 * (c0 / SUPER)], gbase[2 * (c0 / SUPER) + 1], rb) || !rb.sane;
            if (__builtin_amdgcn_ballot_w64(gopen) == 0ull) continue;
            const int c1 = c0 + SUPER < nc ? c0 + SUPER : nc;
            for (int c = c0; c < c1; c += 2) {                                // (an even number of boxes is stored)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    asm volatile("" ::: "memory");
                    const f4 lo = base[2 * (c + u)], hi = base[2 * (c + u) + 1];
                    cm |= box_open(lo, hi, rb) ? (1u << (c + u)) : 0u;
                }
            }
        }
        if (!rb.sane) cm = ~0u;
    }
    return cm & (nc >= 32 ? ~0u : ((1u << nc) - 1u));                         // (padding, and what a NaN ray opened of it)
}

// the survivors among the (up to 8) spheres of the lane's own cluster, first slot kb
template <bool ANCH>
__device__ __forceinline__ unsigned lane_sphere_bits(const Lds &lds, int S, int anchor, int kb, const RayF &q)
{
    const int Sp = padS(S, lds.NC);
    lds_cf4 *sb = lds_f4(ANCH ? lds.tab + ((size_t)anchor * Sp + kb) * CULL_STRIDE : lds.sph32 + 4 * kb);
    unsigned sm = 0u;
#pragma unroll
    for (int j = 0; j < CLUSTER; ++j) sm |= lane_open<ANCH>(sb[j], q) ? (1u << j) : 0u;
    const int nv = S - kb;                                                    // slots past the last sphere are padding
    return nv >= CLUSTER ? sm : (sm & ((1u << nv) - 1u));
}

// A per-lane count of the lane-owned traversal (clusters or spheres a lane opened) for the measurement build
// (hipcc -DRT_LANE_STATS, tools/lane_stats.py); empty, and every use a no-op, in the product build, as RT_MARK is.
#ifdef RT_LANE_STATS
// counters behind the per-tile cycles (p.tile_cycles[ntiles + base ..]): calls, sum of the
// per-wave maximum, sum of ceil(total / 64), sum of the totals
__device__ __forceinline__ void lane_stats(const KParams &p, int base, unsigned v)
{
    if (!p.tile_cycles) return;
    unsigned mx = v, sum = v;
    for (int d = 32; d >= 1; d >>= 1) { const unsigned m2 = __shfl_xor(mx, d), s2 = __shfl_xor(sum, d); mx = m2 > mx ? m2 : mx; sum += s2; }
    if ((threadIdx.x & 63) == __builtin_ctzll(__builtin_amdgcn_ballot_w64(true))) {
        unsigned *c = p.tile_cycles + p.ntiles + base;
        atomicAdd(c + 0, 1u); atomicAdd(c + 1, mx); atomicAdd(c + 2, (sum + 63u) >> 6); atomicAdd(c + 3, sum);
    }
}
struct LaneCount {
    unsigned n;
    __device__ __forceinline__ LaneCount(unsigned v = 0u) : n(v) {}
    __device__ __forceinline__ void set(unsigned v) { n = v; }
    __device__ __forceinline__ void report(const KParams &p, int base) const { lane_stats(p, base, n); }
};
#else
struct LaneCount {
    __device__ __forceinline__ LaneCount(unsigned = 0u) {}
    __device__ __forceinline__ void set(unsigned) {}
    __device__ __forceinline__ void report(const KParams &, int) const {}
};
#endif
template <bool ANCH>
__device__ __forceinline__ void lanes_closest(const Lds &lds, const KParams &p, int anchor, const V3 &o, const V3 &R, double a,
                                              double &bestn, int &bidx)
{
    RayF q = make_rayf_dir(R);
    if constexpr (!ANCH) add_origin(q, o, p.extent2);
    for (int cb = 0; cb < lds.NC; cb += 32) {
        const int nc = lds.NC - cb < 32 ? lds.NC - cb : 32;
        unsigned cm = lane_cluster_bits<ANCH>(lds, anchor, cb, nc, q, p.extent2);
        RT_MARK(1);
        LaneCount(__builtin_popcount(cm)).report(p, 0);
        while (__builtin_amdgcn_ballot_w64(cm != 0u) != 0ull) {
            LaneCount smc;
            if (cm != 0u) {
                const int kb = (cb + __builtin_ctz(cm)) * CLUSTER;
                cm &= cm - 1u;
                unsigned sm = lane_sphere_bits<ANCH>(lds, p.S, anchor, kb, q);
                smc.set(__builtin_popcount(sm));
                while (__builtin_amdgcn_ballot_w64(sm != 0u) != 0ull) {
                    if (sm != 0u) {
                        const int k = kb + __builtin_ctz(sm);
                        sm &= sm - 1u;
                        sphere_closest<true>(lds, p, k, o, R, a, bestn, bidx);
                    }
                }
            }
            smc.report(p, 4);
        }
        RT_MARK(2);
    }
}

// any-hit: self = the sphere slot this lane's shadow ray starts on (-1: none); its own miss is certified by the
// origin form's "behind" test where that holds (as in cull_mask)
template <bool ANCH>
__device__ __forceinline__ bool lanes_any(const Lds &lds, const KParams &p, int anchor, const V3 &o, const V3 &R, double a, int self)
{
    const bool a_sane = (a > 0.999999 && a < 1.000001);
    RayF q = make_rayf_dir(R);
    bool self_culled = false;
    if constexpr (ANCH) {
        if (__builtin_amdgcn_ballot_w64(self >= 0) != 0ull) {
            add_origin(q, o, p.extent2);
            if (self >= 0) { const float *cs = lds.sph32 + 4 * self; self_culled = cull_origin(f4{cs[0], cs[1], cs[2], cs[3]}, q); }
        }
    } else add_origin(q, o, p.extent2);
    bool occ = false;
    for (int cb = 0; cb < lds.NC; cb += 32) {
        if (cb > 0 && __builtin_amdgcn_ballot_w64(!occ) == 0ull) break;   // (nothing is occluded before the first block)
        const int nc = lds.NC - cb < 32 ? lds.NC - cb : 32;
        unsigned cm = lane_cluster_bits<ANCH>(lds, anchor, cb, nc, q, p.extent2);
        RT_MARK(7);
        if (occ) cm = 0u;
        LaneCount(__builtin_popcount(cm)).report(p, 8);
        while (__builtin_amdgcn_ballot_w64(cm != 0u) != 0ull) {
            LaneCount smc;
            if (cm != 0u) {
                const int kb = (cb + __builtin_ctz(cm)) * CLUSTER;
                cm &= cm - 1u;
                unsigned sm = lane_sphere_bits<ANCH>(lds, p.S, anchor, kb, q);
                if (self_culled && self >= kb && self < kb + CLUSTER) sm &= ~(1u << (self - kb));
                smc.set(__builtin_popcount(sm));
                while (__builtin_amdgcn_ballot_w64(sm != 0u) != 0ull) {
                    if (sm != 0u) {
                        const int k = kb + __builtin_ctz(sm);
                        sm &= sm - 1u;
                        if (sphere_any<true>(lds, k, o, R, a, a_sane)) { occ = true; sm = 0u; cm = 0u; }
                    }
                }
            }
            smc.report(p, 12);
        }
        RT_MARK(8);
    }
    return occ;
}

// The sphere part of a wave-uniform scene query whose float64 direction is DEFERRED (rt_cull.h has the guard and the bound): the
// caller has formed e = |d|² - 1 and the wave's window ballot, and calls one of two instantiations under that wave-uniform branch.
//   IN_WINDOW: every live lane has |e| < UNIT_WINDOW.  The cull reads float32(d); R = renormalize_unit_fast(d, e) — the very call
//              renormalize_unit would have made — a = R.R (and the shadow query's a_sane) are formed under the wave-uniform `if (mask)`
//              of a chunk, in front of its first float64 test, and live in that block only (carried round the chunk loop they cost
//              the headline kernel scratch; a scene above 64 spheres forms them once per chunk with an open sphere: the same values).
//              A query whose cull leaves no sphere never forms them.
//   otherwise: the former order, R = normalize3_generic(d) first and the cull on float32(R).
// Two bodies and not one with selects: `in_window ? renormalize_unit_fast(d, e) : normalize3_generic(d)` compiles to six to twelve
// v_cndmask per query in the path every query takes, more than the deferral saves.
// closest_spheres returns R.R for the query's one division (read only with bidx >= 0, which implies an open chunk).
// A value made opaque where it stands: what is computed from the result stays behind this point.  R is the same in every chunk,
// so the compiler otherwise moves it (and a, and a_sane) out of the chunk loop as loop-invariant — to in front of the cull.
__device__ __forceinline__ double pinned_here(double x)
{
    asm volatile("" : "+v"(x));
    return x;
}
// The trim of a small-scene kernel's 32-bit mask (NG > 0: 1 <= S <= 4 NG <= 8): the padding slots certify themselves, except to a
// NaN ray, which must not send one to the float64 test (it would read a plane record as a sphere).
__device__ __forceinline__ unsigned small_mask(unsigned long long m, int S) { return (unsigned)m & ((1u << S) - 1u); }

// The chunk of spheres that one cull_mask call of a wave-uniform query answers for, and so the shape of the query's sphere walk
// `for (int k0 = 0; k0 < C::end(S); k0 += 64)`: 64 spheres and a 64-bit mask, or (NG > 0, the small-scene kernels) all of the
// scene's at most eight in one chunk and a 32-bit mask: one trip with k0 = 0.  A walk says so with `if constexpr (NG > 0) break;`
// at the end of its body: the increment is then unreachable and no loop is formed at all.  Left to the bound alone the one-trip
// loop is deleted only after its invariants (the trim's `~(-1 << S)`) have been hoisted in front of the cull, and the small-scene
// kernels come out with other instruction counts and, one of them, other resource lines.
template <int NG> struct Chunk {
    using mask_t = typename std::conditional<(NG > 0), unsigned, unsigned long long>::type;
    static __device__ __forceinline__ int end(int S) { return NG > 0 ? 1 : S; }
    // the chunk's spheres, of the `left` = S - k0 from its first one on
    static __device__ __forceinline__ int count(int left) { return (NG > 0 || left < 64) ? left : 64; }
    // padding slots certify themselves, except to a NaN ray
    static __device__ __forceinline__ mask_t trim(unsigned long long m, int n)
    {
        if constexpr (NG > 0) return small_mask(m, n);
        else return m & ((n == 64) ? ~0ull : ((1ull << n) - 1ull));
    }
    static __device__ __forceinline__ int first(mask_t m)
    {
        if constexpr (NG > 0) return __builtin_ctz(m);
        else return __builtin_ctzll(m);
    }
};

template <bool F32, bool IN_WINDOW, int NG = 0>
__device__ __forceinline__ double closest_spheres(const Lds &lds, const KParams &p, int S, int canchor, const V3 &o, const V3 &d, double e,
                                                  double &bestn, int &bidx)
{
    double a = 1.0;
    V3 Rg{0.0, 0.0, 0.0};
    if constexpr (!IN_WINDOW) { Rg = normalize3_generic(d); a = dot3(Rg, Rg); }
    using C = Chunk<NG>;
    for (int k0 = 0; k0 < C::end(S); k0 += 64) {
      const int n = C::count(S - k0);
      // the float32 ray is rebuilt per chunk so that it is not live during the float64 phase
      typename C::mask_t mask = C::trim(cull_mask<NG>(lds, S, canchor, k0, n, o, cull_dir32(IN_WINDOW ? d : Rg), p.extent2, -1), n);
      RT_MARK(1);
      if (mask) {
        V3 R = Rg;
        if constexpr (IN_WINDOW) { R = renormalize_unit_fast(d, pinned_here(e)); a = dot3(R, R); }
        do {                                                  // spheres some live lane might hit, ascending
          const int k = k0 + C::first(mask);
          mask &= mask - 1;
          sphere_closest<F32>(lds, p, k, o, R, a, bestn, bidx);
        } while (mask);
      }
      RT_MARK(2);
      if constexpr (NG > 0) break;                             // (Chunk: one trip)
    }
    return a;
}
// any_hit_masks' sphere loop the same way: the lanes some sphere occludes.
template <bool IN_WINDOW, int NG = 0>
__device__ __forceinline__ lanemask any_spheres_masks(const Lds &lds, const KParams &p, int S, int canchor, const V3 &o, const V3 &d, double e,
                                                      int self, lanemask live)
{
    lanemask occ = 0ull;
    V3 Rg{0.0, 0.0, 0.0};
    if constexpr (!IN_WINDOW) Rg = normalize3_generic(d);
    using C = Chunk<NG>;
    for (int k0 = 0; k0 < C::end(S); k0 += 64) {
      if (k0 > 0 && (live & ~occ) == 0ull) break;
      const int n = C::count(S - k0);
      typename C::mask_t mask = C::trim(cull_mask<NG>(lds, S, canchor, k0, n, o, cull_dir32(IN_WINDOW ? d : Rg), p.extent2, self), n);
      RT_MARK(7);
      if (mask) {
        V3 R = Rg;
        if constexpr (IN_WINDOW) R = renormalize_unit_fast(d, pinned_here(e));
        const double a = dot3(R, R);
        const lanemask a_sane = lanes_where(a > 0.999999) & lanes_where(a < 1.000001);
        do {
          const int k = k0 + C::first(mask);
          mask &= mask - 1;
          occ |= sphere_any_mask<false>(lds, k, o, R, a, a_sane);
          if (mask && (live & ~occ) == 0ull) break;
        } while (mask);
      }
      RT_MARK(8);
      if constexpr (NG > 0) break;                             // (Chunk: one trip)
    }
    return occ;
}

// trace.py:7-41, closest hit.  R = normalize(d) and a = R.R are computed once per query.
// anchor: index into the cull table of a point every live lane's ray passes through (0 = camera),
// or -1 for rays with no common anchor (reflections).
template <class Q>
__device__ __forceinline__ void closest_hit(const Lds &lds, const KParams &p, const V3 &o, const V3 &d, int anchor,
                                            double &t_out, int &idx_out, int &type_out)
{
    constexpr int MODE = Q::MODE, NG = Q::NG;
    using C = Chunk<NG>;
    const int P = plane_count<Q>(p);
    const int S = p.S;
    // Lds::defer: R and a are formed in front of the first float64 sphere test, not in front of the cull (closest_spheres).
    constexpr bool F32 = MODE >= 1;                           // sphere records: the float32 LDS table (see sphere_hot)
    double bestn = __builtin_inf();
    int bidx = -1;
    double aq;                                                // R.R, for the one division below
    if (MODE < 2 && lds.defer) {
        const double e = unit_excess(d);
        const bool in_window = cull_reads_d(__builtin_amdgcn_ballot_w64(outside_unit_window(e)));   // wave-uniform
        RT_MARK(0);
        const int canchor = cull_anchor<Q>(p, anchor);
        if (in_window) aq = closest_spheres<F32, true, NG>(lds, p, S, canchor, o, d, e, bestn, bidx);
        else aq = closest_spheres<F32, false, NG>(lds, p, S, canchor, o, d, e, bestn, bidx);
    } else {
    const V3 R = renormalize_unit(d);                         // R == normalize(d), intersections.py:13
    const double a = dot3(R, R);
    RT_MARK(0);
    const int canchor = cull_anchor<Q>(p, anchor);
    // lane-owned traversal for the rays without a common anchor (bounce 1 on), where the wave's rays have parted;
    // the primary rays of a tile travel together: the wave-uniform cull below is cheaper for them
    if (MODE >= 2 && lds.NC > 0 && (canchor < 0 || p.lanes_primary)) {
        if (canchor >= 0) lanes_closest<true>(lds, p, canchor, o, R, a, bestn, bidx);
        else lanes_closest<false>(lds, p, -1, o, R, a, bestn, bidx);
    } else if constexpr (NG > 0) {                            // one chunk, all of it (Chunk)
      // This walk alone keeps a copy for the one chunk: written as the loop below with a break at its end, like the other three
      // walks, the loop's variables stand in front of `idx` and `type` in this function, the compiler promotes those two to
      // registers in the other order, and all six small-scene kernels come out with two v_cndmask swapped and other register
      // names.  Two of the six then measured 0.2 and 0.3 % over what two builds of the parent differ by
      // (profiles/kernel_twin_bench.json); with the copy every kernel is its parent's, instruction for instruction.
      typename C::mask_t mask = C::trim(cull_mask<NG>(lds, S, canchor, 0, S, o, R, p.extent2, -1), S);
      RT_MARK(1);
      while (mask) {
        const int k = C::first(mask);
        mask &= mask - 1;
        sphere_closest<F32>(lds, p, k, o, R, a, bestn, bidx);
      }
      RT_MARK(2);
    } else
    for (int k0 = 0; k0 < C::end(S); k0 += 64) {
      const int n = C::count(S - k0);
      // the float32 ray is rebuilt per chunk so that it is not live during the float64 phase
      typename C::mask_t mask = C::trim(cull_mask<NG>(lds, S, canchor, k0, n, o, R, p.extent2, -1), n);
      RT_MARK(1);
      while (mask) {                                          // spheres some live lane might hit, ascending
        const int k = k0 + C::first(mask);
        mask &= mask - 1;
        sphere_closest<F32>(lds, p, k, o, R, a, bestn, bidx);
      }
      RT_MARK(2);
    }
    aq = a;
    }
    double best = 999.0;                                      // trace.py:17
    int idx = -1, type = HIT_NONE;
    if (bidx >= 0) {
        const double t = div_inrange(bestn, aq);              // :31 / :36, once per query
        if (best > t && t > 0.0) { best = t; idx = bidx; type = HIT_SPHERE; }
    }
    const double *pl = lds.recs() + (F32 ? 0 : opaque(p.S) * SPH_STRIDE);
    for (int k = 0; k < P; ++k) {                             // intersections.py:41-68
        const double *g = pl + k * PL_STRIDE;
        double den, num;
        plane_den_num(g, plane_code<Q>(p, k), o, d, den, num, lds.trim);   // :52, :59-61
        if (!(__builtin_fabs(den) < 0.001)) {                 // :55
            const double t = div_inrange(num, den);           // :63
            if (best > t && t > 0.0) { best = t; idx = k; type = HIT_PLANE; }
        }
    }
    t_out = best; idx_out = idx; type_out = type;
    RT_MARK(3);
}

// any_hit's sphere and plane loops with the occlusion flag as ONE lane mask in a scalar register pair (Lds::trim: the
// two-wave kernels without a material table): "is any live lane still unoccluded" is then two scalar instructions wherever
// it is asked, no test runs under a per-lane condition, and the flag becomes a per-lane bool once, at the end.  Same compares
// on the same values as any_hit's loops below; a lane that is already occluded is tested again (its answer can only stay).
template <class Q>
__device__ __forceinline__ bool any_hit_masks(const Lds &lds, const KParams &p, const V3 &o, const V3 &d, int anchor, int self)
{
    constexpr int NG = Q::NG;
    using C = Chunk<NG>;
    const int P = plane_count<Q>(p);
    const int S = p.S;
    const lanemask live = lanes_where(true);
    lanemask occ;
    if (RT_DEFER_SHADOW != 0 && lds.defer) {   // R, a and a_sane in front of the first float64 test, not in front of the cull (any_spheres_masks)
        const double e = unit_excess(d);
        const bool in_window = cull_reads_d(__builtin_amdgcn_ballot_w64(outside_unit_window(e)));   // wave-uniform
        RT_MARK(6);
        const int canchor = cull_anchor<Q>(p, anchor);
        if (in_window) occ = any_spheres_masks<true, NG>(lds, p, S, canchor, o, d, e, self, live);
        else occ = any_spheres_masks<false, NG>(lds, p, S, canchor, o, d, e, self, live);
    } else {
    const V3 R = renormalize_unit(d);                         // R == normalize(d), intersections.py:13
    const double a = dot3(R, R);
    RT_MARK(6);
    const int canchor = cull_anchor<Q>(p, anchor);
    const lanemask a_sane = lanes_where(a > 0.999999) & lanes_where(a < 1.000001);
    occ = 0ull;
    for (int k0 = 0; k0 < C::end(S); k0 += 64) {
      if (k0 > 0 && (live & ~occ) == 0ull) break;
      const int n = C::count(S - k0);
      typename C::mask_t mask = C::trim(cull_mask<NG>(lds, S, canchor, k0, n, o, R, p.extent2, self), n);
      RT_MARK(7);
      while (mask) {
        const int k = k0 + C::first(mask);
        mask &= mask - 1;
        occ |= sphere_any_mask<false>(lds, k, o, R, a, a_sane);
        if (mask && (live & ~occ) == 0ull) break;
      }
      RT_MARK(8);
      if constexpr (NG > 0) break;                             // (Chunk: one trip)
    }
    }
    const double *pl = lds.recs() + opaque(p.S) * SPH_STRIDE;
    for (int k = 0; k < P; ++k) {
        if ((live & ~occ) == 0ull) break;
        const double *g = pl + k * PL_STRIDE;
        double den, num;
        plane_den_num(g, plane_code<Q>(p, k), o, d, den, num, true);
        const double an = __builtin_fabs(num), ad = __builtin_fabs(den);
        // the signs agree (any_hit: num > 0 && den > 0 || num < 0 && den < 0) where the sign bits do and neither is zero; den is
        // not zero under !(|den| < 0.001); a NaN num fails |num| > 0, a NaN den every test of the quotient below
        int sx = (int)(__builtin_bit_cast(unsigned long long, num) >> 32) ^ (int)(__builtin_bit_cast(unsigned long long, den) >> 32);
        asm("" : "+v"(sx));                                                   // (a 32-bit compare of the high words' xor, not a 64-bit one of both words')
        const lanemask ahead = lanes_where(!(ad < 0.001)) & lanes_where(sx >= 0) & lanes_where(an > 0.0);   // t = num/den > 0
        const lanemask sure = lanes_where(an < 998.0 * ad);                   // t < 999 for certain (see any_hit)
        occ |= ahead & sure;
        const lanemask edge = ahead & ~sure & ~occ;
        if (edge != 0ull) {                                                   // far along a grazing ray: the rounded quotient decides
            bool h = false;
            if (lane_of(edge) && !(an > 1000.0 * ad)) { const double t = num / den; h = 999.0 > t && t > 0.0; }
            occ |= lanes_where(h);
        }
    }
    RT_MARK(9);
    return lane_of(occ);
}

// trace.py:92-96: the shadow query only asks "does anything report 0 < t < 999" (any hit).
// Called with the lanes that need the answer active; returns true if occluded.
// anchor = cull-table index of the light the ray points at; self = index of the sphere the ray
// starts on (-1: a plane), whose miss is certified by the origin-form "behind" test.
// NG > 0: only the two-wave kernels without a material table (Lds::trim) have small-scene twins, so any_hit_masks answers for them.
template <class Q>
__device__ __forceinline__ bool any_hit(const Lds &lds, const KParams &p, const V3 &o, const V3 &d, int anchor, int self, bool lanes = true)
{
    constexpr int MODE = Q::MODE;
    if (MODE == 0 && lds.trim) return any_hit_masks<Q>(lds, p, o, d, anchor, self);
    const int P = plane_count<Q>(p);
    const int S = p.S;
    const V3 R = renormalize_unit(d);                         // R == normalize(d), intersections.py:13
    const double a = dot3(R, R);
    RT_MARK(6);
    const bool a_sane = (a > 0.999999 && a < 1.000001);
    bool occ = false;
    const int canchor = (opaque(p.anchors) > 0) ? anchor : -1;
    if (MODE >= 2 && lds.NC > 0 && lanes) {
        occ = (canchor >= 0) ? lanes_any<true>(lds, p, canchor, o, R, a, self) : lanes_any<false>(lds, p, -1, o, R, a, self);
    } else
    for (int k0 = 0; k0 < S; k0 += 64) {
      // "is any live lane still unoccluded" compiles to a v_cndmask + v_cmp pair (the bool lives as a lane mask that may hold
      // stale bits of inactive lanes): asked only where the answer can be no and skipping pays — not before the first chunk,
      // not before the first sphere of the first chunk, not before a plane (an empty exec mask skips a plane's test anyway)
      if (k0 > 0 && __builtin_amdgcn_ballot_w64(!occ) == 0ull) break;
      const int n = (S - k0 < 64) ? S - k0 : 64;
      unsigned long long mask = cull_mask(lds, S, canchor, k0, n, o, R, p.extent2, self);
      mask &= (n == 64) ? ~0ull : ((1ull << n) - 1ull);
      RT_MARK(7);
      while (mask) {
        const int k = k0 + __builtin_ctzll(mask);
        mask &= mask - 1ull;
        if (!occ) occ = sphere_any<(MODE >= 1)>(lds, k, o, R, a, a_sane);
        if (mask && __builtin_amdgcn_ballot_w64(!occ) == 0ull) break;   // every live lane already occluded (only if spheres remain)
      }
      RT_MARK(8);
    }
    const double *pl = lds.recs() + (MODE >= 1 ? 0 : opaque(p.S) * SPH_STRIDE);
    for (int k = 0; k < P; ++k) {
        if (!occ) {
            const double *g = pl + k * PL_STRIDE;
            double den, num;
            plane_den_num(g, plane_code<Q>(p, k), o, d, den, num);
            if (!(__builtin_fabs(den) < 0.001)) {
                const double an = __builtin_fabs(num), ad = __builtin_fabs(den);
                const bool same_sign = (num > 0.0 && den > 0.0) || (num < 0.0 && den < 0.0);
                if (same_sign) {
                    // t = num/den > 0.  t < 999 is certain when |num| < 998|den| and impossible when
                    // |num| > 1000|den|; only in between is the rounded quotient needed.
                    if (an < 998.0 * ad) occ = true;
                    else if (!(an > 1000.0 * ad)) { const double t = num / den; if (999.0 > t && t > 0.0) occ = true; }
                }
            }
        }
    }
    RT_MARK(9);
    return occ;
}

// Per-lane ray counters of the counting instantiation (rt_get_stats); empty, and every call a no-op, otherwise.
template <bool COUNT> struct RayCount {
    __device__ __forceinline__ void closest(bool) {}
    __device__ __forceinline__ void hit(bool) {}
    __device__ __forceinline__ void shadow(bool, bool) {}
};
template <> struct RayCount<true> {
    unsigned n_closest = 0, n_issued = 0, n_skipped = 0, n_hit = 0;
    __device__ __forceinline__ void closest(bool alive) { n_closest += alive ? 1u : 0u; }      // trace.py:53
    __device__ __forceinline__ void hit(bool alive) { n_hit += alive ? 1u : 0u; }
    // trace.py:92 issues a shadow query per light and hit; the kernel traces it only where its answer is used (k > 0)
    __device__ __forceinline__ void shadow(bool alive, bool traced) { n_issued += (alive && traced) ? 1u : 0u; n_skipped += (alive && !traced) ? 1u : 0u; }
};

// Candidate t of the hashed points in the cube [-1, 1)^3 for the hash key `key`: its components are the counters t | {0, 1, 2}
// (q_c = (h >> 8) 2^-23 + 2^-24 - 1, and q.q, are exact).  soft_light_point and scatter_continue take the first of eight that is
// inside the unit ball; their counter layouts and what they do with it differ.
__device__ __forceinline__ V3 hash_unit3(unsigned key, unsigned t)
{
    return V3{hash_unit(key, t), hash_unit(key, t | 1u), hash_unit(key, t | 2u)};
}

// Shadow sample point Q of a light record g = {cx, cy, cz, rho} for the hash key `key` (soft_key with t = b << 15 | m << 9 |
// i << 5 folded in): the first of eight hashed candidates q in the unit ball (hash_unit3, as scatter_continue's), Q = c + rho*q (float64,
// no fused multiply-add: -ffp-contract=off), or c itself if none of the eight is inside.
__device__ __forceinline__ V3 soft_light_point(unsigned key, const double *g)
{
#pragma unroll 1
    for (int j = 0; j < 8; ++j) {
        const unsigned t = (unsigned)j << 2;
        const V3 c = hash_unit3(key, t);
        if (dot3(c, c) < 1.0) { const double rho = g[3]; return V3{g[0] + rho * c.x, g[1] + rho * c.y, g[2] + rho * c.z}; }
    }
    return V3{g[0], g[1], g[2]};
}

// The mirror direction d - 2(d.N)N of common.py:113-120.  |d - 2(d.N)N| = 1 up to rounding for unit d, N: the exact unit-vector
// path applies (renormalize_unit falls back to sqrt-and-divide by itself otherwise).
__device__ __forceinline__ V3 mirror_dir(const V3 &d, const V3 &N)
{
    const double c2 = -2.0 * dot3(d, N);
    return renormalize_unit(V3{d.x + c2 * N.x, d.y + c2 * N.y, d.z + c2 * N.z});
}

// The direction of shadow sample i of light m (record g) in trace b, from the biased hit point Pt: the sample's key is the light
// key of the lane's sample (lkey: its LKEY slot, read by the caller at every sample: no VGPR holds it across the light loop) with
// b, m and i folded in, its point on the light soft_light_point's.  common.py:84-91.
__device__ __forceinline__ V3 soft_light_dir(unsigned lkey, int b, int m, int i, const double *g, const V3 &Pt)
{
    const unsigned key = lkey ^ (((unsigned)b << 15) | ((unsigned)m << 9) | ((unsigned)i << 5));
    const V3 Q = soft_light_point(key, g);
    return normalize3(V3{Q.x - Pt.x, Q.y - Pt.y, Q.z - Pt.z});
}

// The scatter of a SCAT kernel's hit on a rough surface (rough > 0, trace b < depth), in place of the mirror direction R:
// the first of eight hashed candidates q in the unit ball (hash_unit3, counters b << 5 | j << 2 | c), then
// D = normalize(R + rough*q) (R itself if none of the eight is inside).  Returns false if D leaves on the other side of the
// surface from R (or either is on it, or NaN): the path ends after this trace (absorption).
template <int WGT, class MS>
__device__ __forceinline__ bool scatter_continue(const Lds &lds, const MS &ms, const V3 &N, int b, double rough, V3 &nd)
{
    const unsigned key = (unsigned)SLOT(KEY);
    const V3 R = nd;
    bool found = false;
    V3 q{0.0, 0.0, 0.0};
#pragma unroll 1
    for (int j = 0; j < 8 && !found; ++j) {
        const unsigned t = ((unsigned)b << 5) | ((unsigned)j << 2);
        const V3 c = hash_unit3(key, t);
        if (dot3(c, c) < 1.0) { q = c; found = true; }
    }
    if (found) nd = normalize3(V3{R.x + rough * q.x, R.y + rough * q.y, R.z + rough * q.z});   // linear_comb(R, q, 1.0, rough)
    const double sR = dot3(R, N), sD = dot3(nd, N);
    return (sR > 0.0 && sD > 0.0) || (sR < 0.0 && sD < 0.0);
}

// The continuation of a REFR kernel's hit (MatState: ETA, Q), in place of trace.py:105-110.  d: the incoming direction,
// N: the outward normal at the hit, Pt = P + BIAS*N (:82-83).  float64 throughout, in the order rt_set_scene_materials_ex
// documents (mi355rt.h): c = d.N; entering (c < 0): eta = 1/ior, ci = -c, n = N; leaving: eta = ior, ci = c, n = -N.
//   sphere, k = 1 - eta^2 (1 - ci^2) >= 0:  T = normalize(eta d + (eta ci - sqrt(k)) n), from P - BIAS*n
//   sphere, k < 0 (total internal reflection):  the reflection, from P + BIAS*n
//   plane (thin sheet, ior ignored):  d, from P - BIAS*n
// and the next origin is that point + BIAS * the new direction.  P - BIAS*n is Q entering and Pt leaving, P + BIAS*n the
// other way round (-BIAS*n = -+bN exactly: negation is exact).
// SCAT: a reflection off a rough surface is scattered (scatter_continue; sb: the trace index, -1 for the last trace, whose
// continuation is never used); returns false where the path ends (absorption).  Otherwise always true.
template <int WGT, class MS>
__device__ __forceinline__ bool refract_continue(const Lds &lds, const MS &ms, const V3 &N, const V3 &Pt, V3 &o, V3 &d, int sb = -1)
{
    const double eta_slot = SLOT(ETA);
    V3 nd;
    bool from_q = false, reflect = true;
    if (eta_slot != 0.0) {
        const double c = dot3(d, N);
        const bool enter = c < 0.0;
        from_q = enter;
        if (eta_slot < 0.0) { nd = d; reflect = false; }                     // a transparent plane
        else {
            const double eta = enter ? 1.0 / eta_slot : eta_slot;
            const double ci = enter ? -c : c;
            const double k = 1.0 - (eta * eta) * (1.0 - ci * ci);
            if (k >= 0.0) {
                const double cn = eta * ci - __builtin_sqrt(k);
                const V3 n = enter ? N : V3{-N.x, -N.y, -N.z};
                // |T| = 1 up to rounding for unit d, N (renormalize_unit falls back to sqrt-and-divide otherwise)
                nd = renormalize_unit(V3{eta * d.x + cn * n.x, eta * d.y + cn * n.y, eta * d.z + cn * n.z});
                reflect = false;
            } else from_q = !enter;                                           // total internal reflection: stays on the incoming side
        }
    }
    bool keep = true;
    if (reflect) {
        nd = mirror_dir(d, N);
        if constexpr (MS::scat) {                                             // (a transparent row is never rough)
            const double rough = SLOT(ROUGH);
            if (rough > 0.0 && sb >= 0) keep = scatter_continue<WGT>(lds, ms, N, sb, rough, nd);
        }
    }
    V3 b = Pt;
    if (from_q) b = V3{SLOT(QX), SLOT(QY), SLOT(QZ)};
    o = V3{b.x + 0.0002 * nd.x, b.y + 0.0002 * nd.y, b.z + 0.0002 * nd.z};
    d = nd;
    return keep;
}

// The texel a TEX kernel's hit takes its colour from (rt_set_scene_textures, mi355rt.h): the entry of KParams::lens.texels for the
// object in slot `slot` (spheres in slot order, then planes) hit at the unbiased point Pt.  The slot's own entry holds its colour
// and, in the fourth float, its texture id k (-1: none — the entry is then the answer).  With a texture, its record
// r = {origin[3], axis[3][3], n[3], 1/n[3], base} (TEX_STRIDE doubles in the scene buffer's texture block, KParams::lens.tex; read
// per lane from global memory: a wave's hits share a few records, which stay in the cache) gives, per axis a:
// g = ((d.x*U.x) + (d.y*U.y)) + d.z*U.z with d = Pt - origin (float64, no fused multiply-add), f = floor(g) clamped to
// [-2^30, 2^30 - 1] (NaN: -2^30), j = f mod n; entry base + (j_2*ny + j_1)*nx + j_0 (base = S + P + first).
// Nothing of this is staged in LDS: the images of a family's kernels, and with them every choice the dispatcher makes from
// their sizes (workgroups per CU, parking), are those of the family's twin.
// f mod n without an integer division (20 instructions on the vector unit, three times per hit): q = floor(f * rn) with
// rn = RN(1/n) (the host's division, rt_scene.h: texture_block), j = f - n*q, and one correction step into [0, n).  Exact for integral |f| <= 2^30 and
// 1 <= n <= 4096:  n*q < 2^43 and f - n*q are integers below 2^53, so neither rounds;  f*rn is within 2^-52 |f/n| <= 2^-22 of f/n
// (rn within 2^-53 relative, one more rounding);  a quotient f/n that is not an integer is at least 1/n >= 2^-12 from the
// nearest one, so its floor is the true floor and 0 <= j < n;  an integral quotient k may come out as k or k - 1, j as 0 or n:
// the correction maps n to 0.  (The other direction, j < 0, cannot occur; it is corrected too, for one compare and one add.)
// An axis with n = 1 needs no case of its own: j = f - floor(f) = 0 whatever g is.
// tests/test_textures.py replays this against integer arithmetic on dimensions 3, 5, 7 and 4096 and coordinates on exact multiples.
__host__ __device__ inline double texel_wrap(double g, double n, double rn)
{
    double f = __builtin_floor(g);
    f = f >= -0x1p30 ? f : -0x1p30;                                           // (a NaN fails the compare)
    f = f > 0x1p30 - 1.0 ? 0x1p30 - 1.0 : f;
    double j = f - n * __builtin_floor(f * rn);
    if (j < 0.0) j += n;
    if (j >= n) j -= n;
    return j;
}
__device__ __forceinline__ unsigned texel_of(const KParams &p, int slot, const V3 &Pt)
{
    const int k = (int)p.lens.texels[4 * (size_t)slot + 3];
    unsigned ti = (unsigned)slot;
    if (k >= 0) {
        const double *r = p.scene + (size_t)p.lens.tex + 1 + TEX_STRIDE * k;
        const V3 dd{Pt.x - r[0], Pt.y - r[1], Pt.z - r[2]};
        const double j0 = texel_wrap(((dd.x * r[3]) + (dd.y * r[4])) + (dd.z * r[5]), r[12], r[15]);
        const double j1 = texel_wrap(((dd.x * r[6]) + (dd.y * r[7])) + (dd.z * r[8]), r[13], r[16]);
        const double j2 = texel_wrap(((dd.x * r[9]) + (dd.y * r[10])) + (dd.z * r[11]), r[14], r[17]);
        ti = (unsigned)(r[18] + ((j2 * r[13] + j1) * r[12] + j0));            // (integers below 2^53: exact)
    }
    return ti;
}

// The sky (rt_set_scene_sky, mi355rt.h): the colour of a trace with direction d that found nothing, float64 without fused
// multiply-add in the header's order.  k is the scene's sky block (SKY_DOUBLES 8-byte words), which the host (rt_scene.h: sky_block) lays out for this
// function:
//   0..2 up | 3..5 horizon | 6..8 zenith - horizon | 9..11 nadir - horizon | 12 log2(sharp), an int64 | 13..15 sun_dir |
//   16 sun_cos | 17..19 sun_rgb | 20..22 halo_rgb | 23 log2(halo_shin), an int64
// (the two differences are float64 subtractions, the same bits wherever they are formed).  The block is read through a pointer
// to the constant address space: the kernel never writes the scene buffer and the address is made of kernel arguments alone, so
// every read is an s_load into SGPRs and no VGPR holds a constant of the sky; the two counts are integers so that the squaring
// loops run on the scalar unit.  Both gradient differences are loaded and the value is selected, not the address.
typedef __attribute__((address_space(4))) const double sky_f64;
typedef __attribute__((address_space(4))) const long long sky_i64;
__device__ __forceinline__ V3 sky_color(const double *block, const V3 &d)
{
    sky_f64 *k = (sky_f64 *)(size_t)block;
    const double h = dot3(d, V3{k[0], k[1], k[2]});
    const bool below = h < 0.0;
    const double a = below ? -h : h;
    double one = 1.0;
    asm volatile("" : "+s"(one));                             // (a scalar 1.0 made here: see DESIGN.md, Sky)
    double t = a > 1.0 ? one : a;
    const int nsharp = (int)((sky_i64 *)k)[12];
    if (nsharp > 0) {                                                         // (wave-uniform: a scalar branch)
        double q = 1.0 - t;
#pragma unroll 1
        for (int i = 0; i < nsharp; ++i) q = q * q;
        t = 1.0 - q;
    }
    const double zx = k[6], zy = k[7], zz = k[8], nx = k[9], ny = k[10], nz = k[11];
    V3 g{k[3] + t * (below ? nx : zx), k[4] + t * (below ? ny : zy), k[5] + t * (below ? nz : zz)};
    const double s = dot3(d, V3{k[13], k[14], k[15]});
    if (s > 0.0) {
        double q = s;
        const int nhalo = (int)((sky_i64 *)k)[23];
#pragma unroll 1
        for (int i = 0; i < nhalo; ++i) q = q * q;
        g = V3{g.x + k[20] * q, g.y + k[21] * q, g.z + k[22] * q};
    }
    if (s >= k[16]) g = V3{g.x + k[17], g.y + k[18], g.z + k[19]};
    return g;
}

// The set-up of a hit (type, idx).  trace_bounce and guides_kernel (rt_guides.h) share the first two.
// hit_slot: the object's slot in the tables that list spheres in slot order, then planes (material ids, texels, lighting rows).
// plane_base: where the planes' records start in the LDS records.  MODE 1 / 2 kernels (NOREC) keep no float64 sphere records in
// LDS (sphere_hot): the planes' and lights' records start at 0.
// hit_normal: the outward normal N at the unbiased hit point Pt and BIAS*N, trace.py:63-71.  (guides_kernel forms N in the branch
// that also picks its colour and id: with the normal in a call of its own its instruction stream changes.)
__device__ __forceinline__ int hit_slot(int type, int idx, int S) { return (type == HIT_SPHERE) ? idx : S + idx; }
template <bool NOREC> __device__ __forceinline__ int plane_base(int S) { return NOREC ? 0 : S * SPH_STRIDE; }
template <bool NOREC>
__device__ __forceinline__ void hit_normal(const Lds &lds, int type, int idx, int plb, const V3 &Pt, V3 &N, V3 &bN)
{
    if (type == HIT_SPHERE) {                                                 // :63-66
        const SphHot g = sphere_hot<NOREC>(lds, idx);
        N = normalize3(V3{Pt.x - g.x, Pt.y - g.y, Pt.z - g.z});               // common.py:94-101
        bN = V3{0.0002 * N.x, 0.0002 * N.y, 0.0002 * N.z};
    } else {                                                                  // :68-71
        const double *g = lds.recs() + plb + idx * PL_STRIDE;
        N = V3{g[6], g[7], g[8]};                                             // float32-renormalised, host-side
        bN = V3{g[9], g[10], g[11]};                                          // BIAS*N as the reference rounds it
    }
}

// trace.py:44-112.  On entry `alive` lanes carry a ray (o,d); on exit `alive` is false for lanes
// that missed (the reference's 404 sentinels), rgb is this bounce's colour, (o,d) the next ray.
// MS::mat: ambient_int and lambert_int are the hit object's material coefficients; its reflectivity is left in the REFL slot (alive lanes).
// b: the trace index (0: the primary ray); SCAT kernels scatter off rough surfaces with it, and clear `alive` where a scattered
// path ends (absorption) after this trace's colour.
template <bool PARK, int WGT, bool COUNT, class Q, class MS>
__device__ __forceinline__ void trace_bounce(const Lds &lds, const KParams &p, bool &alive, int anchor,
                                             V3 &o, V3 &d, V3 &rgb, RayCount<COUNT> &cnt, MS &ms, int b = 0)
{
    constexpr int MODE = Q::MODE;
    constexpr bool NOREC = MODE >= 1;         // no float64 sphere records in LDS (sphere_hot)
    // The wave-level skip of back-facing point lights (rt_facing.h) is compiled out of the lane-owned kernels (MODE 2) of every
    // family: they run at 128 VGPRs with scratch already, and the skip adds 4 to 8 bytes of it per lane there (DESIGN.md §4,
    // "Back-facing lights").  Their light loops are the former ones.
    constexpr bool FACING_SKIP = RT_FACING_SKIP != 0 && MODE != 2;
    const int S = p.S, P = p.P, L = opaque(p.L);
    rgb = V3{0.0, 0.0, 0.0};
    double t = 999.0; int idx = -1, type = HIT_NONE;
    cnt.closest(alive);
    RT_MARK(11);
    // (LENS: a primary ray starts on the lens, not at the camera: no anchor for its closest hit.  `anchor` itself still says
    // which trace this is for the shadow rays below.)
    if (alive) closest_hit<Q>(lds, p, o, d, MS::lens ? -1 : anchor, t, idx, type);   // :53 (idle lanes masked off)
    // SKY: the lanes that entered alive and missed return the sky's colour for their direction instead of (0, 0, 0); they end
    // as before.  d is still in registers here, parked kernels included (the hit lanes park it below), so it is neither held
    // longer nor read back; the branch is skipped when no lane of the wave missed (s_cbranch_execz).
    if constexpr (MS::sky) {
        if (alive && type == HIT_NONE) rgb = sky_color(p.scene + (size_t)p.lens.sky, d);
    }
    alive = alive && (type != HIT_NONE);                                      // :56-57
    cnt.hit(alive);
    if (alive) {
        V3 Pt{o.x + t * d.x, o.y + t * d.y, o.z + t * d.z};                   // :60 (1.0*o is exact)
        // PARK: the object's colour is re-read from its LDS record where it is used (volatile: at the point of
        // use) instead of being held in 6 VGPRs across the shadow queries
        // MODE 1 / 2 kernels keep no float64 sphere records in LDS (plane_base), and a
        // hit sphere's colour comes from the packed scene in global memory — through one flat pointer that serves both cases
        const int plb = plane_base<NOREC>(NOREC ? 0 : opaque(S));            // (opaque only where S is used)
        const int coff = (type == HIT_SPHERE) ? idx * SPH_STRIDE + 4 : plb + idx * PL_STRIDE + 12;
        volatile const lds_f64 *colp = (volatile const lds_f64 *)lds.recs() + coff;
        volatile const double *colf = (NOREC && type == HIT_SPHERE) ? p.scene + coff : lds.recs() + coff;
        // MODE 1: one float32 LDS table holds the spheres' and the planes' colours (exact: the scene is float32)
        typedef __attribute__((address_space(3))) float lds_f32;
        volatile const lds_f32 *col1 = nullptr;
        if constexpr (MODE == 1) col1 = (volatile const lds_f32 *)lds.col32 + 4 * ((type == HIT_SPHERE) ? idx : (int)padS(S, lds.NC) + idx);
        // TEX: the colour is a float32 texel in global memory (the object's own colour is one too: texel_of), chosen here from the
        // unbiased Pt.  What stays live across the shadow queries is its 32-bit index; parked kernels read the texel again at
        // each point of use (an L2 hit), as they re-read a record's colour
        unsigned texi = 0u;
        if constexpr (MS::tex) texi = texel_of(p, hit_slot(type, idx, S), Pt);
        auto texel = [&](int c) -> double { return (double)((volatile const float *)p.lens.texels)[4 * (size_t)texi + c]; };
        V3 colr{0.0, 0.0, 0.0};
        if constexpr (!PARK && MS::tex) {                                      // register variants: the 16-byte entry, one aligned load
            const f4 tc = reinterpret_cast<const f4 *>(p.lens.texels)[texi];
            colr = V3{(double)tc[0], (double)tc[1], (double)tc[2]};
        }
        else if constexpr (!PARK) colr = (MODE == 1) ? V3{(double)col1[0], (double)col1[1], (double)col1[2]} : V3{colf[0], colf[1], colf[2]};
        auto col = [&](int c) -> double {
            if constexpr (PARK && MS::tex) return texel(c);
            else if constexpr (PARK && MODE == 1) return (double)col1[c];
            else if constexpr (PARK && NOREC) return colf[c];
            else if constexpr (PARK) return colp[c];
            else return c == 0 ? colr.x : (c == 1 ? colr.y : colr.z);
        };
        auto lambert_add = [&](double k, const V3 &e) {                     // :101, rgb += (k * e) * col, e the light's colour
            rgb = V3{rgb.x + (k * e.x) * col(0), rgb.y + (k * e.y) * col(1), rgb.z + (k * e.z) * col(2)};
        };
        volatile const lds_f64 *mp = nullptr;
        V3 N, bN;
        hit_normal<NOREC>(lds, type, idx, plb, Pt, N, bN);
        if constexpr (MS::mat) {
            // the object's entry of the LDS material table (looked up after the normal: its address is live only here);
            // Lambert coefficient and reflectivity go to the lane's slots
            mp = ms.entry((type == HIT_SPHERE) ? idx : S + idx);              // (hit_slot, spelled out: through the call the two terms of the entry's address swap in the add)
            SLOT(LAMB) = mp[1];
            if constexpr (MS::refr) {
                // a transparent hit: its weight is trans, and Q = P - BIAS*N (the unbiased P is gone after :82-83) is kept for
                // the continuation; a plane's BIAS*N is its stored bN, rounded as the reference rounds it
                const double tr = mp[3];
                const bool glass = tr > 0.0;
                SLOT(REFL) = glass ? tr : mp[2];
                SLOT(ETA) = glass ? ((type == HIT_SPHERE) ? mp[4] : -1.0) : 0.0;
                if (glass) {
                    SLOT(QX) = Pt.x - bN.x;
                    SLOT(QY) = Pt.y - bN.y;
                    SLOT(QZ) = Pt.z - bN.z;
                }
                if constexpr (MS::scat) SLOT(ROUGH) = mp[5];
            } else
            SLOT(REFL) = mp[2];
            const double amb = mp[0];
            rgb = V3{0.0 + amb * col(0), 0.0 + amb * col(1), 0.0 + amb * col(2)};   // :77 as the reference rounds it (+0 for a negative amb)
        } else
        rgb = V3{p.amb * col(0), p.amb * col(1), p.amb * col(2)};             // :77 (0 + amb*col)
        Pt = V3{Pt.x + bN.x, Pt.y + bN.y, Pt.z + bN.z};                       // :82-83
        const int self = (type == HIT_SPHERE) ? idx : -1;
        Park3<PARK, WGT, MODE == 3> dpark(lds.acc, 1, lds.wave);      // the incoming direction is only needed again for the reflection
        dpark.set(d);
        RT_MARK(4);

        constexpr bool TRIM = Q::template trim<WGT / 64>();                  // (RT_TRIM_PATH)
        const double *lt = lds.recs() + plb + ((TRIM && Q::GROUND) ? 1 : opaque(P)) * PL_STRIDE;   // (TRIM: plane_count, not the opaque argument)
        if constexpr (MS::lit) {
        // LIT (rt_set_scene_lighting, mi355rt.h): light m has a colour e_m and the hit a Blinn-Phong highlight of strength spec / n
        // and exponent shin.  e_m, spec / n and log2(shin) come from the scene's lighting block in global memory (lit_doubles): e_m
        // by a wave-uniform address, the hit's pair by its slot, the one 32-bit value this keeps live across the shadow queries.
        // The shadow query is asked when the Lambert term (k > 0) or the highlight (spec > 0 and Ld.N > 0) wants it; spec > 0 is
        // read off the stored spec / n, which gives the same bytes where the quotient underflows to 0 (mi355rt.h).  Ld is not
        // held across the query either: a lane that is lit and whose hit has spec > 0 forms it again, the same way from the same operands (the soft key
        // comes from its slot again, the light's record through an opaque index: again()), and reads -d for the half vector back from dpark.
        const unsigned lslot = (unsigned)(hit_slot(type, idx, S));
        auto lit_row = [&]() { return (volatile const double *)(p.scene + (size_t)p.lens.lit + (size_t)LT_STRIDE * L) + 2 * (size_t)lslot; };
        auto again = [](int m) { asm volatile("" : "+v"(m)); return m; };   // the light's index, opaque: what is read through it is read again
        auto point_Ld = [&](int m) {
            const double *g = lt + m * LT_STRIDE;
            return normalize3(V3{g[0] - Pt.x, g[1] - Pt.y, g[2] - Pt.z});     // common.py:84-91
        };
        auto soft_Ld = [&](int m, int i) { return soft_light_dir((unsigned)SLOT(LKEY), b, m, i, lt + m * LT_STRIDE, Pt); };
        auto lit_add = [&](int m, double k, auto &&form_Ld) {                 // light m, not occluded
            const double *e = p.scene + (size_t)p.lens.lit + LT_STRIDE * m;
            const double er = e[0], eg = e[1], eb = e[2];
            if (k > 0.0) lambert_add(k, V3{er, eg, eb});
            volatile const double *lr = lit_row();
            const double spec = lr[0];
            if (spec > 0.0) {                                                 // (Ld again only for a hit that can have a highlight)
              const V3 Ld = form_Ld();
              if (dot3(Ld, N) > 0.0) {
                const V3 dd = dpark.get();
                const V3 H = normalize3(V3{Ld.x - dd.x, Ld.y - dd.y, Ld.z - dd.z});   // Ld + (-d); a zero sum: NaN, no highlight
                const double s = dot3(N, H);
                if (s > 0.0) {
                    double q = s;
                    const int nsq = (int)lr[1];
#pragma unroll 1
                    for (int i = 0; i < nsq; ++i) q = q * q;                  // s ** shin, log2(shin) squarings
                    const double a = spec * q;
                    rgb = V3{rgb.x + a * er, rgb.y + a * eg, rgb.z + a * eb};
                }
              }
            }
        };
        for (int m = 0; m < L; ++m) {
            if constexpr (MS::soft) {
#pragma unroll 1
                for (int i = 0; i < ms.nsh; ++i) {
                    const V3 Ld = soft_Ld(m, i);
                    const double cN = dot3(Ld, N);
                    const double k = SLOT(LAMB) * cN;   // :99
                    RT_MARK(5);
                    if (k > 0.0 || (lit_row()[0] > 0.0 && cN > 0.0)) {
                        const bool occluded = any_hit<Q>(lds, p, Pt, Ld, -1, self, true);
                        if (!occluded) lit_add(m, k, [&]() { return soft_Ld(again(m), i); });
                    }
                }
            } else {
                if constexpr (FACING_SKIP) {                                  // (rt_facing.h: neither k > 0 nor cN > 0 on any live lane)
                    const double *g = lt + m * LT_STRIDE;
                    const bool cert = rt_facing_certified_lamb(g[0] - Pt.x, g[1] - Pt.y, g[2] - Pt.z, N.x, N.y, N.z, p.facing_tau,
                                                               SLOT(LAMB));
                    if (__builtin_amdgcn_ballot_w64(!cert) == 0ull) { RT_MARK(5); continue; }
                }
                const V3 Ld = point_Ld(m);
                const double cN = dot3(Ld, N);
                const double k = SLOT(LAMB) * cN;       // :99
                RT_MARK(5);
                if (k > 0.0 || (lit_row()[0] > 0.0 && cN > 0.0)) {
                    const bool occluded = any_hit<Q>(lds, p, Pt, Ld, 1 + m, self, anchor != 0 || p.lanes_primary);
                    if (!occluded) lit_add(m, k, [&]() { return point_Ld(again(m)); });
                }
            }
        }
        } else
        if constexpr (MS::soft) {
        // SOFT: the lights array of :86 is the L*n shadow sample points Q, (m, i) m-major (soft_light_point), and lamb (the
        // table's, host-divided by n) is lamb_b / n.  The rays do not pass through a light's centre: the shadow query takes the
        // origin form of the cull (no anchor; the lane-owned kernels' lanes_any<false>), never the light-anchored tables.
        for (int m = 0; m < L; ++m) {
            const double *g = lt + m * LT_STRIDE;
#pragma unroll 1
            for (int i = 0; i < ms.nsh; ++i) {
                // (the key is re-read from its slot per sample: no VGPR holds it across the light loop)
                const V3 Ld = soft_light_dir((unsigned)SLOT(LKEY), b, m, i, g, Pt);
                const double k = SLOT(LAMB) * dot3(Ld, N);   // :99
                RT_MARK(5);
                if (k > 0.0) {
                    const bool occluded = any_hit<Q>(lds, p, Pt, Ld, -1, self, true);
                    if (!occluded) lambert_add(k, V3{1.0, 1.0, 1.0});
                }
            }
        }
        } else {
        // (TRIM: the certificate's margin, read from the argument segment once per trace and held in a scalar pair across the
        // lights: read where it is used, it is loaded again, and waited for, on every light)
        double ftau = p.facing_tau;
        if constexpr (FACING_SKIP && TRIM) asm volatile("" : "+s"(ftau));
        for (int m = 0; m < L; ++m) {                                         // :86-102
            const double *g = lt + m * LT_STRIDE;
            const V3 v{g[0] - Pt.x, g[1] - Pt.y, g[2] - Pt.z};
            double lamb;
            if constexpr (MS::mat) lamb = SLOT(LAMB); else lamb = p.lamb;
            if constexpr (FACING_SKIP) {
                // The facing certificate (rt_facing.h): where every live lane of the wave has v.N < -facing_tau (and no negative lamb:
                // per lane with a material table, folded into facing_tau by the host otherwise), no lane's k will be positive, so
                // the wave goes to the next light without normalising v.  One lane without the certificate: today's code for all.
                bool cert;
                if constexpr (MS::mat) cert = rt_facing_certified_lamb(v.x, v.y, v.z, N.x, N.y, N.z, TRIM ? ftau : p.facing_tau, lamb);
                else cert = rt_facing_certified(v.x, v.y, v.z, N.x, N.y, N.z, TRIM ? ftau : p.facing_tau);
                if (__builtin_amdgcn_ballot_w64(!cert) == 0ull) {
                    cnt.shadow(true, false);
                    RT_MARK(5);
                    continue;
                }
            }
            const V3 Ld = normalize3(v);                                      // common.py:84-91
            const double k = lamb * dot3(Ld, N);                              // :99
            // :92-102 — the shadow query's answer is only used when k > 0; it has no other effect,
            // so lanes with k <= 0 (light behind the surface) do not ask.
            cnt.shadow(true, k > 0.0);
            RT_MARK(5);
            if (k > 0.0) {
                // (the shadow rays of the primary hits still travel together: wave-uniform cull unless p.lanes_primary)
                const bool occluded = any_hit<Q>(lds, p, Pt, Ld, 1 + m, self, anchor != 0 || p.lanes_primary);
                if (!occluded) lambert_add(k, V3{1.0, 1.0, 1.0});
            }
        }
        }
        d = dpark.get();
        if constexpr (MS::scat) {
            alive = refract_continue<WGT>(lds, ms, N, Pt, o, d, b < p.depth ? b : -1);   // (alive is true here)
        } else if constexpr (MS::refr) {
            refract_continue<WGT>(lds, ms, N, Pt, o, d);
        } else {
        const V3 Rd = mirror_dir(d, N);
        o = V3{Pt.x + 0.0002 * Rd.x, Pt.y + 0.0002 * Rd.y, Pt.z + 0.0002 * Rd.z};   // :110
        d = Rd;
        }
        RT_MARK(10);
    }
}


// trace.py:115-133.  Bounce 0 rays all start at the camera (cull anchor 0; LENS kernels: on the lens, none); later bounces have none.
// MS::mat (per-object materials): bounce b >= 1 is weighted with W_b = ((refl_0 * refl_1) * ...) * refl_{b-1}, the reflectivities
// of the surfaces the ray was reflected off, in place of p.refl_pow[b-1].  W stops changing where the path ends: the missed
// bounce adds W*0, as the reference's does, and the ones after it add the same again (no change).
// SCAT: key is the sample's scatter_key, kept in its slot for the scatter.  SOFT: lkey is its soft_key, kept in its slot for
// the light loop.
template <bool PARK, int WGT, bool COUNT, class Q, class MS>
__device__ __forceinline__ V3 sample(const Lds &lds, const KParams &p, bool alive, V3 o, V3 d, RayCount<COUNT> &cnt, MS &ms,
                                     unsigned key = 0u, unsigned lkey = 0u)
{
    constexpr int MODE = Q::MODE;
    Park3<PARK, WGT, MODE == 3> acc(lds.acc, 0, lds.wave);           // the running colour
    acc.set(V3{0.0, 0.0, 0.0});
    if constexpr (MS::mat) SLOT(W) = 1.0;
    if constexpr (MS::scat) SLOT(KEY) = (double)key;
    if constexpr (MS::soft) SLOT(LKEY) = (double)lkey;
    for (int b = 0; b <= p.depth; ++b) {
        if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;                                   // wave-uniform exit
        if constexpr (COUNT) {                                                // lane utilisation per bounce: waves entering, lanes alive
            const unsigned long long am = __builtin_amdgcn_ballot_w64(alive);
            if ((threadIdx.x & 63u) == 0u && p.ray_counts) {
                atomicAdd(&p.ray_counts[4 + 2 * b], 1ull);
                atomicAdd(&p.ray_counts[5 + 2 * b], (unsigned long long)__builtin_popcountll(am));
            }
        }
        V3 rgb;
#ifdef RT_REGION_STATS
        ((volatile unsigned *)lds.reg)[(threadIdx.x >> 6) * 32 + 30] = b >= 2 ? 12u : 0u;
#endif
        trace_bounce<PARK, WGT, COUNT, Q, MS>(lds, p, alive, b == 0 ? 0 : -1, o, d, rgb, cnt, ms, b);
        if (b == 0) acc.set(rgb);                                             // :120
        else {                                                                // :131 (a missed bounce adds pow*0; SKY: W * sky(d))
            double wgt;
            if constexpr (MS::mat) wgt = SLOT(W); else wgt = p.refl_pow[b - 1];
            const V3 a = acc.get();
            acc.set(V3{a.x + wgt * rgb.x, a.y + wgt * rgb.y, a.z + wgt * rgb.z});
        }
        if constexpr (MS::mat) {                                              // W_{b+1} = W_b * refl_b (W_1 = 1 * refl_0 = refl_0)
            if (alive) {
                volatile lds_f64 *w = &SLOT(W);                              // (one read-modify-write of one slot)
                *w = *w * SLOT(REFL);
            }
        }
    }
    return acc.get();
}

template <bool SCALAR_PX = false>
__device__ __forceinline__ V3 pixel_P(const KParams &p, int x, int y)
{
    // (SCALAR_PX, RT_TRIM_RAY: p.px as a value in scalar registers.  Left as a read of the argument segment, it is merged with the
    // table's first load into one per-lane flat load through a select of the two addresses — a vector memory round trip at the
    // head of every wave)
    double px = p.px;
    if constexpr (SCALAR_PX) asm("" : "+s"(px));
    if (p.pixel_loc) {                                                        // kernels.py:19
        const size_t wh = (size_t)p.w * p.h, o = (size_t)x * p.h + y;
        return V3{p.pixel_loc[o], p.pixel_loc[wh + o], p.pixel_loc[2 * wh + o]};
    }
    return V3{SCALAR_PX ? px : p.px, (double)x * p.dy + p.y0, (double)y * p.dz + p.z0};   // scene/camera.py:18-26
}

// Lattice point (i, j) of the half-pixel lattice of the closed-form grid: even indices are pixel centres, odd ones
// the reference's midpoints 0.5 Pa + 0.5 Pb of the two neighbouring centres (kernels.py:43-50: c1*a + c2*b, two
// products and one sum per component; either operand order gives the same bits).  The first component is
// 0.5 px + 0.5 px = px exactly.
__device__ __forceinline__ V3 lattice_P(const KParams &p, int i, int j)
{
    const double ya = (double)(i >> 1) * p.dy + p.y0, yb = (double)((i + 1) >> 1) * p.dy + p.y0;
    const double za = (double)(j >> 1) * p.dz + p.z0, zb = (double)((j + 1) >> 1) * p.dz + p.z0;
    return V3{p.px, (i & 1) ? 0.5 * ya + 0.5 * yb : ya, (j & 1) ? 0.5 * za + 0.5 * zb : za};
}

__device__ __forceinline__ V3 primary_dir(const KParams &p, const V3 &P)
{
    const V3 v{p.cam_R[0] * P.x + p.cam_R[1] * P.y + p.cam_R[2] * P.z,       // kernels.py:22, common.py:40-49
               p.cam_R[3] * P.x + p.cam_R[4] * P.y + p.cam_R[5] * P.z,
               p.cam_R[6] * P.x + p.cam_R[7] * P.y + p.cam_R[8] * P.z};
    return normalize3(v);                                                     // kernels.py:23
}

// The thin-lens primary ray (o, d) of sample (X, Y, s) through the pixel point P (rt_set_lens, mi355rt.h), float64 without
// fused multiply-add: v = R P as primary_dir forms it, the focal point F = O + (f / P.x) v (linear_comb(O, v, 1.0, f / P.x);
// 1.0*O is exact), u the first of eight hashed candidates in the unit disk (u_c and u.u exact) or (0, 0),
// o = (O + (a u0) ey) + (a u1) ez with ey, ez the columns 1 and 2 of R, d = normalize(F - o).
__device__ __forceinline__ void lens_ray(const KParams &p, unsigned x, unsigned y, unsigned s, const V3 &P, V3 &o, V3 &d)
{
    const V3 v{p.cam_R[0] * P.x + p.cam_R[1] * P.y + p.cam_R[2] * P.z,
               p.cam_R[3] * P.x + p.cam_R[4] * P.y + p.cam_R[5] * P.z,
               p.cam_R[6] * P.x + p.cam_R[7] * P.y + p.cam_R[8] * P.z};
    const double t = p.lens.focus / P.x;
    const V3 F{p.cam_o[0] + t * v.x, p.cam_o[1] + t * v.y, p.cam_o[2] + t * v.z};
    const unsigned key = lens_key(x, y, s, p.seed);
    double u0 = 0.0, u1 = 0.0;
#pragma unroll 1
    for (int j = 0; j < 8; ++j) {
        const unsigned tj = (unsigned)j << 1;
        const double c0 = hash_unit(key, tj);
        const double c1 = hash_unit(key, tj | 1u);
        if (c0 * c0 + c1 * c1 < 1.0) { u0 = c0; u1 = c1; break; }
    }
    const double a0 = p.lens.aperture * u0, a1 = p.lens.aperture * u1;
    o = V3{(p.cam_o[0] + a0 * p.cam_R[1]) + a1 * p.cam_R[2], (p.cam_o[1] + a0 * p.cam_R[4]) + a1 * p.cam_R[5],
           (p.cam_o[2] + a0 * p.cam_R[7]) + a1 * p.cam_R[8]};
    d = normalize3(V3{F.x - o.x, F.y - o.y, F.z - o.z});                     // common.py:28-32 of vector_difference(o, F)
}

// kernels.py:69-73: clip and store one pixel; off = (x - x0) h + y.
// fo = element offset of this launch's frame (rt_render_sequence; 0 for a single frame)
// TRIM (RT_TRIM_STORE): the clip as straight-line code (clip_color), and the three planes through one per-lane address stepped by
// the scalar stride; else the clip with its branches (clip_color_branches: the same bytes) and every plane's base formed with
// 64-bit scalar adds before the lane's offset goes on.
template <bool TRIM = false>
__device__ __forceinline__ void store_pixel(const KParams &p, long long off, long long fo, double R, double G, double B)
{
    if (p.out_u8) {                                                           // common.py:60-63
        const uint8_t r8 = TRIM ? clip_color(R) : clip_color_branches(R), g8 = TRIM ? clip_color(G) : clip_color_branches(G),
                      b8 = TRIM ? clip_color(B) : clip_color_branches(B);
        const uint8_t c1 = p.u8_rgb ? g8 : b8, c2 = p.u8_rgb ? b8 : g8;
        uint8_t *o8 = p.out_u8 + fo;
        if (p.u8_hwc) {                                                       // image layout: row y, column x, 3 bytes
            const long long xr = off / p.h, yy = off - xr * p.h;
            uint8_t *px = o8 + (yy * p.plane_stride + xr) * 3;
            px[0] = r8; px[1] = c1; px[2] = c2;
        } else {
            if constexpr (TRIM) {
                uint8_t *q = o8 + off;
                q[0] = r8;
                q += p.plane_stride; q[0] = c1;
                q += p.plane_stride; q[0] = c2;
            } else {
                o8[off] = r8;
                o8[p.plane_stride + off] = c1;
                o8[2 * p.plane_stride + off] = c2;
            }
        }
    }
    if (p.out_f32) {
        float *o32 = p.out_f32 + fo;
        if constexpr (TRIM) {
            float *q = o32 + off;
            q[0] = (float)R;
            q += p.plane_stride; q[0] = (float)G;
            q += p.plane_stride; q[0] = (float)B;
        } else {
            o32[off] = (float)R;
            o32[p.plane_stride + off] = (float)G;
            o32[2 * p.plane_stride + off] = (float)B;
        }
    }
}

// The float32 cull tables (exact sphere table for the origin form; {A-c, tau} per anchor and sphere; the same two
// for the cluster bounding spheres), in the order and layout the render kernel keeps them in LDS.  They depend on
// the scene, the camera position (anchor 0) and floor_anch only, so the host runs this once per change of those
// (one workgroup, a few microseconds) and every render workgroup copies the result.
__global__ __launch_bounds__(TABLE_THREADS) void tables_kernel(const KParams p, float *__restrict__ out)
{
    const int nrec = (int)lds_doubles(p.S, p.P, p.L);
    const int Sp = padS(p.S, p.NC), NCp = pad4(p.NC);
    const TableLayout tl = table_layout(p.S, p.NC, p.anchors, p.P);
    float *sph32 = out;
    float *tab = out + tl.tab;                         // anchors x Sp entries
    float *csph32 = out + tl.csph32;
    float *ctab = out + tl.ctab;                       // anchors x NCp entries
    const double *rec = p.scene;
    const float NINF = -__builtin_inff();
    for (int k = threadIdx.x; k < Sp; k += TABLE_THREADS) {   // exact: the scene is float32
        const double *g = rec + k * SPH_STRIDE;
        const bool real = k < p.S;
        sph32[4 * k + 0] = real ? (float)g[0] : 0.0f; sph32[4 * k + 1] = real ? (float)g[1] : 0.0f;
        sph32[4 * k + 2] = real ? (float)g[2] : 0.0f; sph32[4 * k + 3] = real ? (float)g[3] : NINF;
    }
    float *col32 = out + tl.col32;
    for (int k = threadIdx.x; k < Sp + pad4(p.P); k += TABLE_THREADS) {   // colours of spheres and planes (MODE 1 kernels)
        const double *g = k < p.S ? rec + k * SPH_STRIDE + 4 : rec + p.S * SPH_STRIDE + (k - Sp) * PL_STRIDE + 12;
        const bool real = k < p.S || (k >= Sp && k - Sp < p.P);
        for (int c = 0; c < 3; ++c) col32[4 * k + c] = real ? (float)g[c] : 0.0f;
        col32[4 * k + 3] = 0.0f;
    }
    const double *lt = rec + p.S * SPH_STRIDE + p.P * PL_STRIDE;
    for (int e = threadIdx.x; e < p.anchors * Sp; e += TABLE_THREADS) {
        const int a = e / Sp, k = e - a * Sp;
        float *t = tab + (size_t)e * CULL_STRIDE;
        if (k >= p.S) { t[0] = t[1] = t[2] = 0.0f; t[3] = -NINF; continue; }   // padding: always culled
        const double *g = rec + k * SPH_STRIDE;
        const double ax = a ? lt[(a - 1) * LT_STRIDE + 0] : p.cam_o[0];
        const double ay = a ? lt[(a - 1) * LT_STRIDE + 1] : p.cam_o[1];
        const double az = a ? lt[(a - 1) * LT_STRIDE + 2] : p.cam_o[2];
        const double lx = ax - g[0], ly = ay - g[1], lz = az - g[2];
        const double ll = lx * lx + ly * ly + lz * lz;
        t[0] = (float)lx; t[1] = (float)ly; t[2] = (float)lz;
        t[3] = anchored_tau(ll, g[3], p.floor_anch);
    }
    // the same two tables for the cluster bounding spheres (float64 records after the lights; rounding the
    // centre to float32 is covered by rounding R2 up)
    const double *cl = rec + nrec;
    for (int c = threadIdx.x; c < NCp; c += TABLE_THREADS) {
        const bool real = c < p.NC;
        const double *g = cl + (real ? c : 0) * CL_STRIDE;
        csph32[4 * c + 0] = real ? (float)g[0] : 0.0f; csph32[4 * c + 1] = real ? (float)g[1] : 0.0f;
        csph32[4 * c + 2] = real ? (float)g[2] : 0.0f;
        csph32[4 * c + 3] = real ? (float)(g[3] * (1.0 + 0x1p-20)) : NINF;
    }
    for (int e = threadIdx.x; e < p.anchors * NCp; e += TABLE_THREADS) {
        const int a = e / NCp, c = e - a * NCp;
        float *t = ctab + (size_t)e * CULL_STRIDE;
        if (c >= p.NC) { t[0] = t[1] = t[2] = 0.0f; t[3] = -NINF; continue; }
        const double *g = cl + c * CL_STRIDE;
        const double ax = a ? lt[(a - 1) * LT_STRIDE + 0] : p.cam_o[0];
        const double ay = a ? lt[(a - 1) * LT_STRIDE + 1] : p.cam_o[1];
        const double az = a ? lt[(a - 1) * LT_STRIDE + 2] : p.cam_o[2];
        const double lx = ax - g[0], ly = ay - g[1], lz = az - g[2];
        const double ll = lx * lx + ly * ly + lz * lz;
        t[0] = (float)lx; t[1] = (float)ly; t[2] = (float)lz;
        t[3] = anchored_tau(ll, g[3], p.floor_anch);
    }
    // bounding boxes of the clusters' spheres (radius = sqrt of the float32 r*r the reference tests against, a little
    // more), every face rounded outward to float32
    float *cbox = out + tl.cbox;
    for (int c = threadIdx.x; c < NCp; c += TABLE_THREADS) {
        double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
        for (int k = c * CLUSTER; k < (c + 1) * CLUSTER && k < p.S; ++k) {
            const double *g = rec + k * SPH_STRIDE;
            const double rad = __builtin_sqrt(g[3]) * (1.0 + 0x1p-20) + 1e-30;
            for (int i = 0; i < 3; ++i) { lo[i] = __builtin_fmin(lo[i], g[i] - rad); hi[i] = __builtin_fmax(hi[i], g[i] + rad); }
        }
        float *b = cbox + (size_t)c * BOX_STRIDE;
        for (int i = 0; i < 3; ++i) {                  // a float is within 2^-24 |x| of x: step 2^-22 |x| outward first
            b[i] = (float)(lo[i] - (__builtin_fabs(lo[i]) * 0x1p-22 + 1e-30));
            b[4 + i] = (float)(hi[i] + (__builtin_fabs(hi[i]) * 0x1p-22 + 1e-30));
        }
        b[3] = 0.0f; b[7] = 0.0f;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < supers(p.NC); g += TABLE_THREADS) {       // the union of the group's (outward-rounded) boxes
        float *b = out + tl.gbox + (size_t)g * BOX_STRIDE;
        for (int i = 0; i < 3; ++i) { b[i] = __builtin_inff(); b[4 + i] = -__builtin_inff(); }
        for (int c = g * SUPER; c < (g + 1) * SUPER && c < p.NC; ++c)
            for (int i = 0; i < 3; ++i) {
                b[i] = __builtin_fminf(b[i], cbox[(size_t)c * BOX_STRIDE + i]);
                b[4 + i] = __builtin_fmaxf(b[4 + i], cbox[(size_t)c * BOX_STRIDE + 4 + i]);
            }
        b[3] = 0.0f; b[7] = 0.0f;
    }
    // the anchored table of the groups' bounding spheres (float64 records behind the clusters')
    const int NG = supers(p.NC), NGp = pad4(NG);
    const double *gr = cl + (size_t)p.NC * CL_STRIDE;
    for (int e = threadIdx.x; e < p.anchors * NGp; e += TABLE_THREADS) {
        const int a = e / NGp, g = e - a * NGp;
        float *t = out + tl.gtab + (size_t)e * CULL_STRIDE;
        if (g >= NG) { t[0] = t[1] = t[2] = 0.0f; t[3] = -NINF; continue; }
        const double *c = gr + g * CL_STRIDE;
        const double ax = a ? lt[(a - 1) * LT_STRIDE + 0] : p.cam_o[0];
        const double ay = a ? lt[(a - 1) * LT_STRIDE + 1] : p.cam_o[1];
        const double az = a ? lt[(a - 1) * LT_STRIDE + 2] : p.cam_o[2];
        const double lx = ax - c[0], ly = ay - c[1], lz = az - c[2];
        const double ll = lx * lx + ly * ly + lz * lz;
        t[0] = (float)lx; t[1] = (float)ly; t[2] = (float)lz;
        t[3] = anchored_tau(ll, c[3], p.floor_anch);
    }
}

// The MatState of a workgroup's material block matl (staged: M, table, ids) with W in the per-thread slot wslot.
// SOFT: nsh is the scene's shadow_samples (the block's last double).
template <Family F, int WSLOT, bool FRESH>
__device__ __forceinline__ MatState<F, WSLOT, FRESH> mat_state(double *matl, int M, int nsh = 1)
{
    typedef __attribute__((address_space(3))) double lds_d;
    typedef MatState<F, WSLOT, FRESH> MS;
    if constexpr (MS::mat) return MS{(unsigned)(size_t)(lds_d *)(matl + 1), (unsigned)(size_t)(lds_d *)(matl + 1 + MS::COLS * M), nsh};
    else return {};
}

// One wave per 8x8 tile, tiles consecutive in y: tile -> (tx, ty).  render_kernel and guides_kernel (rt_guides.h).
__device__ __forceinline__ void tile_xy(const KParams &p, int tile, int &tx, int &ty)
{
    tx = div_by(tile, p.tiles_y, p.tiles_y_magic, p.tiles_y_shift);
    ty = tile - tx * p.tiles_y;
}

// AA = false: aliasing off — instantiated separately so that the common case does not carry the tap loop's
// live state (registers decide occupancy here).
// F: the kernel's feature family (Family; PLAIN has none of these features).
// MAT: the scene has a material table (per-object shading coefficients, rt_set_scene_materials).
// REFR (with MAT): the table has transparent rows (rt_set_scene_materials_ex): refraction continuations (refract_continue).
// SCAT (with REFR): the table has rough rows (rt_set_scene_materials_scatter): scattered reflections (scatter_continue).
// SOFT (with SCAT): a light has a radius (rt_set_scene_area_lights): n shadow samples per light (soft_light_point).
// LENS (with SCAT, and LENS_SOFT with SOFT): the camera has an aperture (rt_set_lens): thin-lens primary rays (lens_ray).
// GROUND: the ground-plane twin (plane_code) of a PLAIN kernel that does not count rays; false: the generic kernel.
// NG: the cull groups of a small-scene twin (cull_mask_t) of a two-wave ground-plane twin: the scene is flat, has 4 NG - 3 to 4 NG spheres
// and anchored tables; 0: the kernel for any scene.
template <bool AA, bool PARK, int WPW, bool COUNT = false, bool LAT = false, int MODE = 0, Family F = Family::PLAIN, bool GROUND = false, int NG = 0>
__global__ __launch_bounds__(64 * WPW, MODE >= 2 ? RT_W_LANES : (AA ? (PARK ? RT_W_AAPARK : 4) : (PARK ? RT_W_PARK : 5))) void render_kernel(const KParams p)
{
    constexpr int WG_THREADS = 64 * WPW, WAVES_PER_WG = WPW;
    constexpr bool M2 = MODE >= 2;
    constexpr bool NOREC = MODE >= 1;
    using Q = Query<MODE, GROUND, NG>;        // what the scene queries below are compiled for
    constexpr bool TRIM = Q::template trim<WPW>(), TRIM_RAY = RT_TRIM_RAY(WPW, GROUND, NG), TRIM_STORE = RT_TRIM_STORE(WPW, GROUND, NG);   // (above Query)
    static_assert(NG == 0 || (WPW == 2 && !COUNT && F == Family::PLAIN), "small-scene twins: of PLAIN's two-wave kernels");
    constexpr bool MAT = has_mat(F), SCAT = has_scat(F), SOFT = has_soft(F), LENS = has_lens(F), TEX = has_tex(F);
    const int nrec = (int)lds_doubles(NOREC ? 0 : p.S, p.P, p.L);             // MODE 1 / 2: planes and lights only (sphere_hot)
    const double *rec_src = p.scene + (NOREC ? (size_t)p.S * SPH_STRIDE : 0);
    double *accum = lds_raw + nrec;
    int *offw = reinterpret_cast<int *>(accum + lds_slots(AA, PARK, M2, F) * WG_THREADS);
    float *sph32 = reinterpret_cast<float *>(offw + lds_offset_words(PARK, WG_THREADS));
    // TRIM: two-wave kernels are sent flat scenes only and are MODE 0 (rt_plan.h: plan_launch), so of the layout they read `tab`
    // and `total` alone: flat_layout forms those two in a few 32-bit scalar instructions (a small-scene twin: `tab` is a constant
    // and `total` one multiply-add of L) where table_layout's 64-bit chain through p.NC costs every workgroup about 45.  The
    // cluster and colour tables are empty there and their pointers never read (Lds::NC is the constant 0).
    static_assert(WPW != 2 || MODE == 0, "two-wave kernels: wave-uniform cull over float64 records (flat_layout)");
    TableLayout tl;
    if constexpr (WPW == 2 && TRIM) {
        const FlatLayout fl = flat_layout(NG, p.S, p.L, p.anchors);
        tl = TableLayout{fl.tab, 0, 0, 0, 0, 0, fl.total, fl.total, 0, 0};
    } else tl = table_layout(p.S, p.NC, p.anchors, p.P);
    // the lane-owned kernels leave the clusters' origin-form spheres in global memory: with anchored tables in place the only
    // rays without an anchor are the reflections, and those test boxes
    const bool LANES = MODE >= 2 && p.anchors > 0;
    float *tab = sph32 + tl.tab;                       // anchors x Sp entries
    float *csph32 = LANES ? nullptr : sph32 + tl.csph32;
    float *ctab = sph32 + tl.ctab;                     // anchors x NCp entries
    float *cbox = sph32 + tl.cbox;                     // NCp boxes
    const size_t ntab = MODE == 1 ? tl.total_col : (LANES ? tl.total_lanes : tl.total);
    unsigned *wgstat = reinterpret_cast<unsigned *>(sph32 + ntab);   // {cycles, waves done}
    if ((!TRIM || p.cost) && threadIdx.x == 0) { wgstat[0] = 0u; wgstat[1] = 0u; }   // (read by measuring launches only, below: TRIM leaves them alone in the others)
    {   // stage the packed scene and its float32 cull tables once per workgroup: two straight copies.  (The tables
        // used to be computed here, by every workgroup: 3 % of the frame's VALU instructions and a second barrier.)
        for (int i = threadIdx.x; i < nrec; i += WG_THREADS) lds_raw[i] = rec_src[i];
        const int nf4 = (int)(ntab / 4);
        const f4 *src = reinterpret_cast<const f4 *>(p.ftab);
        f4 *dst = reinterpret_cast<f4 *>(sph32);
        for (int i = threadIdx.x; i < nf4; i += WG_THREADS) dst[i] = src[i];
    }
    // MAT: the material block (mat_offset) behind the workgroup words (and the region counters of the measurement build)
#ifdef RT_REGION_STATS
    double *matl = reinterpret_cast<double *>(wgstat + 4 + WPW * 32);
#else
    double *matl = reinterpret_cast<double *>(wgstat + 4);
#endif
    int nmat = 0, nsh = 1;
    if constexpr (MAT) {
        // (LENS, TEX: the block with rows of 6 the host names, a padded copy behind the scene's own for a table of 3 or 5 columns)
        const double *msrc = p.scene + ((LENS || TEX) ? (size_t)p.lens.mat : mat_offset(p.S, p.P, p.L, p.NC));
        nmat = (int)msrc[0];
        const int nm = (int)mat_doubles(nmat, p.S, p.P, F);
        for (int i = threadIdx.x; i < nm; i += WG_THREADS) matl[i] = msrc[i];
        if constexpr (SOFT) nsh = (int)msrc[nm - 1];
    }
    __syncthreads();
    // two-wave workgroups serve the small flat scenes only (the host sends every clustered scene to workgroups of 4): with
    // NC a constant 0 there, none of the cluster code is compiled into those kernels (the headline kernel sits in a narrow
    // register optimum)
#ifdef RT_REGION_STATS
    const Lds lds{sph32, tab, csph32, ctab, cbox, sph32 + tl.gbox, sph32 + tl.gtab, MODE == 1 ? sph32 + tl.col32 : nullptr, WPW == 2 ? 0 : p.NC, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), MODE < 2, MODE >= 2, WPW == 2 && !MAT, RT_DEFER_DIRECTION != 0 && MODE < 2 && !(AA && PARK), wgstat + 4, accum};
    for (int i = threadIdx.x & 63; i < 32; i += 64) lds.reg[(threadIdx.x >> 6) * 32 + i] = 0u;
    if ((threadIdx.x & 63) == 0) lds.reg[(threadIdx.x >> 6) * 32 + 31] = (unsigned)__builtin_amdgcn_s_memtime();
#else
    const Lds lds{sph32, tab, csph32, ctab, cbox, sph32 + tl.gbox, sph32 + tl.gtab, MODE == 1 ? sph32 + tl.col32 : nullptr, WPW == 2 ? 0 : p.NC, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), MODE < 2, MODE >= 2, WPW == 2 && !MAT, RT_DEFER_DIRECTION != 0 && MODE < 2 && !(AA && PARK), accum};
#endif

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // Longest-first dispatch: the hardware hands out workgroups in blockIdx order, so blockIdx indexes a
    // permutation of the tile blocks sorted by the cycles they took in the previous launch (order_kernel).
    // Any permutation renders every tile exactly once; only the length of the launch's tail depends on it.
    // A launch may carry several frames of the same scene and camera (rt_render_sequence): workgroups [f bpf, (f+1) bpf)
    // render frame f, each frame in the same order, so one frame's last workgroups run beside the next frame's first.
    // Only the LAST frame of a launch decides how raggedly the launch ends, so only it is dispatched longest-first; the
    // frames before it run every XCD's blocks in tile order, neighbours in y back to back on the XCD that owns their group:
    // the 128-byte lines they share are completed in that L2 within microseconds.
    int bid = (int)blockIdx.x;
    const unsigned *ord = p.order;
    int frame = 0;                                                            // of a multi-frame launch (TRIM: one scalar register until the store)
    if (p.nframes > 1) {
        frame = div_by(bid, p.bpf, p.bpf_magic, p.bpf_shift);
        bid -= frame * p.bpf;
        if (ord && frame < p.nframes - 1) ord += p.seq_offset;
    }
    // Four-wave kernels may dispatch TILE by tile (p.order_tiles): a workgroup holds its LDS image and — by the time three of its
    // waves have ended — three idle wave slots until its last wave ends, so its waves should be tiles of EQUAL cost, not
    // neighbours (measured on config 5: 3.26 of 4 wave slots per SIMD occupied on average with neighbours).
    const bool by_tile = WPW >= TILE_ORDER_MIN_WPW && p.order_tiles;
    const int block = by_tile ? bid : (ord ? (int)ord[bid] : bid);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int tile_v = by_tile ? (ord ? (int)ord[bid * WAVES_PER_WG + wave_u] : bid * WAVES_PER_WG + wave_u) : block * WAVES_PER_WG + wave;
    // (wave-uniform, but loaded through a vector register: as a scalar it does not occupy a VGPR until the cost is recorded
    // at the end — the MODE 1 kernel spilled it, 8 bytes of scratch written per lane; the two-wave kernels keep their register
    // allocation as it is)
    const int tile = WPW >= TILE_ORDER_MIN_WPW ? __builtin_amdgcn_readfirstlane(tile_v) : tile_v;
    if (tile >= p.ntiles) return;                                             // whole wave, after the barriers
    const unsigned long long t_begin = (p.tile_cycles || p.cost) ? __builtin_amdgcn_s_memtime() : 0ull;
    int tx, ty;
    tile_xy(p, tile, tx, ty);
    const int x = p.x0 + tx * TILE + (lane >> 3);
    const int y = ty * TILE + (lane & 7);
    bool inb = (x < p.x1) && (y < p.h);
    // LAT: of the lattice, only pixel centres (even, even) and the points inside the outermost centres are ever summed
    if constexpr (LAT) inb = inb && ((((x | y) & 1) == 0) || (x >= 1 && x <= p.w - 2 && y >= 1 && y <= p.h - 2));
    const int xc = inb ? x : p.x0, yc = inb ? y : 0;                          // keep addresses valid for idle lanes
    // PARK: the pixel's output offset waits in LDS instead of staying live (or being spilled to scratch)
    // across the whole trace; -1 marks lanes outside the frame.
    typedef __attribute__((address_space(3))) int lds_i32;
    // (REMAT kernels re-derive it at the end from the tile, a scalar, and the lane's number instead: see Park3)
    constexpr bool OFF_REMAT = PARK && MODE == 3;
    volatile lds_i32 *offp = OFF_REMAT ? nullptr : (volatile lds_i32 *)offw + threadIdx.x;
    if constexpr (PARK && !OFF_REMAT) *offp = inb ? (x - p.x0) * p.h + y : -1;   // w*h <= 2^31 (checked by the host)

    const V3 o{p.cam_o[0], p.cam_o[1], p.cam_o[2]};                           // kernels.py:16
    RayCount<COUNT> cnt;
    constexpr int WSLOT = lds_slots(AA, PARK, M2, Family::PLAIN);            // MAT: the slot of W
    auto ms = mat_state<F, WSLOT, !PARK || MODE == 3>(matl, nmat, nsh);
    // SCAT: the scatter key of a sample is (X, Y, s) on the half-pixel lattice, pixel centres at (2x, 2y), absolute columns
    // (the lattice kernels' own coordinates); s the stochastic sample, else 0
    // SOFT: the light key (soft_key) of the same (X, Y, s)
    // LENS: the primary ray is lens_ray's for the same (X, Y, s); its origin is the lane's own
    const unsigned sseed = SCAT ? p.seed : 0u;
    double R, G, B;
    if constexpr (!AA) {
        unsigned key = 0u, lkey = 0u;
        if constexpr (SCAT) key = LAT ? scatter_key((unsigned)xc, (unsigned)yc, 0u, sseed) : scatter_key(2u * xc, 2u * yc, 0u, sseed);
        if constexpr (SOFT) lkey = LAT ? soft_key((unsigned)xc, (unsigned)yc, 0u, sseed) : soft_key(2u * xc, 2u * yc, 0u, sseed);
        const V3 P0 = LAT ? lattice_P(p, xc, yc) : pixel_P<TRIM_RAY>(p, xc, yc);
        V3 ro = o, rd;
        if constexpr (LENS) lens_ray(p, LAT ? (unsigned)xc : 2u * xc, LAT ? (unsigned)yc : 2u * yc, 0u, P0, ro, rd);
        else rd = primary_dir(p, P0);
        const V3 c = sample<PARK, WG_THREADS, COUNT, Q, decltype(ms)>(lds, p, inb, ro, rd, cnt, ms, key, lkey);   // kernels.py:19-26
        R = c.x; G = c.y; B = c.z;
    } else {
        // kernels.py:26-65 as ONE loop: tap 0 is the centre sample, taps 1-8 the half-pixel neighbours (only
        // if some lane of the wave is interior).  One inlined copy of sample(); the tap sums live in LDS when
        // PARK.  The same loop serves the build-defined stochastic mode (p.aa == 2): p.spp jittered samples.
        const bool stoch = (p.aa == 2);
        const bool interior = !stoch && inb && x >= 1 && x <= p.w - 2 && y >= 1 && y <= p.h - 2;
        const int ntaps = stoch ? p.spp : ((__builtin_amdgcn_ballot_w64(interior) != 0ull) ? 9 : 1);
        // neighbour offsets (dx,dy)+1 packed 2 bits each, in the order of kernels.py:53:
        // left, right, top(y+1), bottom(y-1), top-left, top-right, bottom-left, bottom-right
        constexpr unsigned NBX = 0x8858u, NBY = 0x0A25u;
        Park3<PARK && !M2, WG_THREADS> taps(lds.acc, 2);
#pragma unroll 1
        for (int tap = 0; tap < ntaps; ++tap) {
            const V3 Pp = pixel_P<TRIM_RAY>(p, xc, yc);                       // :19
            V3 Pt = Pp;
            unsigned key = 0u, lkey = 0u;
            unsigned lx = 2u * xc, ly = 2u * yc;                              // LENS: the sample's (X, Y)
            if constexpr (SCAT) key = scatter_key(2u * xc, 2u * yc, stoch ? (unsigned)tap : 0u, sseed);
            if constexpr (SOFT) lkey = soft_key(2u * xc, 2u * yc, stoch ? (unsigned)tap : 0u, sseed);
            if (stoch) {
                const unsigned hh = jitter_hash((unsigned)xc, (unsigned)yc, (unsigned)tap, p.seed);
                const double u = (double)(hh & 0xFFFFu) * 0x1p-16 + (0x1p-17 - 0.5);
                const double v = (double)(hh >> 16) * 0x1p-16 + (0x1p-17 - 0.5);
                Pt = V3{Pp.x, Pp.y + u * p.dy, Pp.z + v * p.dz};
            } else if (tap) {
                const int k = tap - 1;
                const int ddx = (int)((NBX >> (2 * k)) & 3u) - 1, ddy = (int)((NBY >> (2 * k)) & 3u) - 1;
                const V3 Pn = pixel_P<TRIM_RAY>(p, interior ? x + ddx : xc, interior ? y + ddy : yc);
                Pt = V3{0.5 * Pp.x + 0.5 * Pn.x, 0.5 * Pp.y + 0.5 * Pn.y, 0.5 * Pp.z + 0.5 * Pn.z};   // :43-50
                if constexpr (SCAT) key = scatter_key((unsigned)(2 * xc + ddx), (unsigned)(2 * yc + ddy), 0u, sseed);
                if constexpr (SOFT) lkey = soft_key((unsigned)(2 * xc + ddx), (unsigned)(2 * yc + ddy), 0u, sseed);
                if constexpr (LENS) { lx = (unsigned)(2 * xc + ddx); ly = (unsigned)(2 * yc + ddy); }
            }
            V3 ro = o, rd;
            if constexpr (LENS) lens_ray(p, lx, ly, stoch ? (unsigned)tap : 0u, Pt, ro, rd);
            else rd = primary_dir(p, Pt);
            const V3 s = sample<PARK, WG_THREADS, COUNT, Q, decltype(ms)>(lds, p, (tap && !stoch) ? interior : inb, ro, rd, cnt, ms, key, lkey);   // :26 / :56
            if (tap == 0) taps.set(s);
            else if (stoch) { const V3 a = taps.get(); taps.set(V3{a.x + s.x, a.y + s.y, a.z + s.z}); }
            else if (interior) { const V3 a = taps.get(); taps.set(V3{a.x + s.x, a.y + s.z, a.z + s.y}); }   // :58-60 (G += B_s; B += G_s)
        }
        { const V3 a = taps.get(); R = a.x; G = a.y; B = a.z; }
        if (stoch) { const double n = (double)p.spp; R = R / n; G = G / n; B = B / n; }
        else if (interior) { R = R / 9; G = G / 9; B = B / 9; }               // :63-65
    }

    long long off;
    if constexpr (OFF_REMAT) {
        const int l2 = (int)fresh_lane();
        const int x2 = p.x0 + tx * TILE + (l2 >> 3), y2 = ty * TILE + (l2 & 7);
        bool inb2 = (x2 < p.x1) && (y2 < p.h);
        if constexpr (LAT) inb2 = inb2 && ((((x2 | y2) & 1) == 0) || (x2 >= 1 && x2 <= p.w - 2 && y2 >= 1 && y2 <= p.h - 2));
        off = inb2 ? (long long)((x2 - p.x0) * p.h + y2) : -1ll;
    } else if constexpr (PARK) off = *offp; else off = inb ? (long long)(x - p.x0) * p.h + y : -1ll;   // (int32 -1 sign-extends)
    if (off >= 0) {
        if constexpr (LAT) {                                                  // one float64 (R,G,B) per lattice sample
            double *q = p.out_f64 + off * 3;
            q[0] = R; q[1] = G; q[2] = B;
        } else {
            // the frame index is formed again here (a wave-uniform division) instead of being carried through the trace, except
            // by the TRIM kernels, which have the scalar register for it (frame 0 of a single-frame launch: offset 0)
            long long fo;
            if constexpr (TRIM) fo = (long long)frame * p.frame_stride;
            else fo = opaque(p.nframes) > 1 ? (long long)div_by((int)blockIdx.x, p.bpf, p.bpf_magic, p.bpf_shift) * p.frame_stride : 0ll;
            store_pixel<TRIM_STORE>(p, off, fo, R, G, B);
        }
    }
#ifdef RT_REGION_STATS
    RT_MARK(11);
    if (p.tile_cycles && (threadIdx.x & 63) < 24)                            // behind the per-tile cycles: 24 region counters (cycles / 64)
        atomicAdd(p.tile_cycles + p.ntiles + 16 + (threadIdx.x & 63), lds.reg[(threadIdx.x >> 6) * 32 + (threadIdx.x & 63)] >> 6);
#endif
    if constexpr (COUNT) {                                                    // rt_get_stats: one atomic per wave and counter
        unsigned v[4] = {cnt.n_closest, cnt.n_issued, cnt.n_skipped, cnt.n_hit};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v[c] += __shfl_down(v[c], d);
            if ((threadIdx.x & 63) == 0 && p.ray_counts) atomicAdd(&p.ray_counts[c], (unsigned long long)v[c]);
        }
    }
    if ((p.tile_cycles || p.cost) && (threadIdx.x & 63) == 0) {               // timing only; never feeds a pixel
        const unsigned cyc = (unsigned)(__builtin_amdgcn_s_memtime() - t_begin);
        if (p.tile_cycles) p.tile_cycles[tile] = cyc;
        if (p.cost) {
            if (by_tile) p.cost[tile] = cyc >> 2;                             // per tile
            else {
                // the block's cost = sum over its waves; the wave that finishes last stores it
                const int expected = (p.ntiles - block * WAVES_PER_WG < WAVES_PER_WG) ? p.ntiles - block * WAVES_PER_WG : WAVES_PER_WG;
                atomicAdd(&wgstat[0], cyc >> 2);
                if ((int)atomicAdd(&wgstat[1], 1u) == expected - 1) p.cost[block] = atomicAdd(&wgstat[0], 0u);
            }
        }
    }
}

// RT_AA_REFERENCE, second half (kernels.py:29-65): pixel (x,y) sums the lattice samples around its centre (2x, 2y) in the
// reference's order — centre, left, right, top (y+1), bottom (y-1), top-left, top-right, bottom-left, bottom-right,
// with G += B_s and B += G_s — and divides by 9; frame-border pixels keep their centre sample.  p describes the PIXEL
// frame (w, h, x0, x1, outputs); p.out_f64 / lat_x0 / lat_h the lattice samples.  One thread per pixel, y fastest.
__global__ __launch_bounds__(256) void aa_resolve_kernel(const KParams p)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)(p.x1 - p.x0) * p.h) return;
    const int xr = (int)(idx / p.h), y = (int)(idx - (long long)xr * p.h), x = p.x0 + xr;
    const double *c = p.out_f64 + ((size_t)(2 * x - p.lat_x0) * p.lat_h + 2 * y) * 3;
    double R = c[0], G = c[1], B = c[2];
    if (x >= 1 && x <= p.w - 2 && y >= 1 && y <= p.h - 2) {
        constexpr unsigned NBX = 0x8858u, NBY = 0x0A25u;                      // (dx,dy)+1, 2 bits each, in the order of kernels.py:53
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int ddx = (int)((NBX >> (2 * k)) & 3u) - 1, ddy = (int)((NBY >> (2 * k)) & 3u) - 1;
            const double *s = c + ((long long)ddx * p.lat_h + ddy) * 3;
            R += s[0]; G += s[2]; B += s[1];                                  // :58-60
        }
        R = R / 9; G = G / 9; B = B / 9;                                      // :63-65
    }
    store_pixel<RT_TRIM_RESOLVE>(p, idx, 0ll, R, G, B);
}

// Builds the dispatch order of the following launches from the block costs a measuring launch stored: longest-first WITHIN
// every XCD, and XCD-affine.
//
// The dispatcher hands workgroup i to XCD i mod 8, and every XCD has its own L2.  A two-wave workgroup writes 16-pixel runs
// of the output planes (16 B of a uint8 plane, 64 B of a float32 plane); the rest of each 128-byte line belongs to its
// neighbours in y.  When those run on other XCDs every fragment of the line is written back on its own (round 2: WRITE_SIZE
// 41 MB per 1080p frame for 31 MB of pixels); written by one XCD, the line is completed in that L2 and leaves it once.
// So WHICH XCD renders a block is decided for GROUPS of 2^gshift consecutive blocks (y runs fastest: neighbours in y), and
// WHEN it renders it block by block:
//   1. the groups are sorted by decreasing mean block cost (counting sort, 1024 logarithmic buckets) and dealt to the XCDs
//      in serpentine order — rank r goes to XCD r mod 8 in even rows of eight and 7 - r mod 8 in odd ones — so every XCD
//      gets the same number of groups and nearly the same total cost;
//   2. every XCD's blocks are sorted by decreasing cost of their own (a second counting sort, per XCD), and the XCD's j-th
//      block takes position 8 j + xcd of the order.  Round 2's XCD-affine order sorted whole groups (a coarser order: +6..14 %
//      on one stream); here the order inside an XCD is as fine as the plain longest-first order.
// The groups that do not fill a row of eight and the short group at the end of the frame share the positions behind those
// rows, longest first.  The output is a permutation of [0, nblocks) by construction; any permutation renders the same frame.
//   3. a second permutation, order[nblocks ..], keeps the XCD assignment of step 1 but runs every XCD's blocks in plain tile
//      order (group after group, the blocks of a group back to back).  All but the last frame of a multi-frame launch use
//      it: in the middle of a launch every CU is busy whatever the order, and blocks that share output lines then follow
//      each other on their XCD within microseconds (step 2's order scatters a group's blocks over the XCD's whole list:
//      measured 37 MB of writes per headline frame instead of 41 for 31 MB of pixels; tile order inside the XCD: see
//      profiles/r03_order_group_sweep.txt).
// gtmp: nblocks / 2^gshift + 1 words, btmp: nblocks words of scratch; order: 2 nblocks words.
// wshift > 0: the items are TILES and a workgroup takes 2^wshift consecutive positions of the order (KParams::order_tiles):
// XCD x's t-th item then sits at position ((8 (t >> wshift) + x) << wshift) + (t mod 2^wshift) — its (t >> wshift)-th workgroup —
// and sorting an XCD's tiles by cost makes every workgroup four tiles of (nearly) equal cost.  nvalid: items that exist (the
// last workgroup's missing tiles cost nothing).  gshift counts items (>= wshift).
__global__ __launch_bounds__(ORDER_THREADS) void order_kernel(const unsigned *__restrict__ cost, unsigned *__restrict__ gtmp,
                                                               unsigned *__restrict__ btmp, unsigned *__restrict__ order, int nblocks, int gshift,
                                                               int wshift, int nvalid)
{
    const unsigned wm = (1u << wshift) - 1u;
    auto place = [&](unsigned x, unsigned t, unsigned tail_) -> unsigned {
        return x < (unsigned)ORDER_XCDS ? ((((unsigned)ORDER_XCDS * (t >> wshift) + x) << wshift) | (t & wm)) : tail_ + t;
    };
    auto cost_of = [&](int it) -> unsigned { return it < nvalid ? cost[it] : 0u; };
    __shared__ unsigned hist[(ORDER_XCDS + 1) * ORDER_BUCKETS];     // [class][bucket]; class ORDER_XCDS = the leftover blocks
    __shared__ unsigned scan[ORDER_THREADS / 64];
    static_assert(ORDER_THREADS == ORDER_BUCKETS, "thread i owns bucket 1023 - i");
    const int i = threadIdx.x, lane = i & 63, wv = i >> 6;
    const int gb = 1 << gshift;
    const int full = nblocks >> gshift;                 // groups of gb blocks; a shorter one may follow
    const int rows = full / ORDER_XCDS;                 // rows of eight groups: one group per XCD each
    // in place: hist[c][b] (counts per bucket) -> exclusive offsets in descending bucket order, for classes [0, nc)
    auto scan_classes = [&](int nc) {
        for (int c = 0; c < nc; ++c) {
            __syncthreads();
            const unsigned v = hist[c * ORDER_BUCKETS + ORDER_BUCKETS - 1 - i];
            unsigned incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            if (lane == 63) scan[wv] = incl;            // wave totals
            __syncthreads();
            unsigned base = 0;
            for (int w = 0; w < wv; ++w) base += scan[w];
            hist[c * ORDER_BUCKETS + ORDER_BUCKETS - 1 - i] = base + incl - v;
        }
        __syncthreads();
    };
    for (int k = i; k < (ORDER_XCDS + 1) * ORDER_BUCKETS; k += ORDER_THREADS) hist[k] = 0u;
    __syncthreads();
    // 1. groups by mean block cost
    for (int g = i; g < full; g += ORDER_THREADS) {
        unsigned long long sum = 0;
        for (int k = 0; k < gb; ++k) sum += cost_of((g << gshift) + k);
        const unsigned mean = (unsigned)(sum >> gshift);
        const int bkt = order_bucket(mean);
        gtmp[g] = ((unsigned)bkt << 20) | atomicAdd(&hist[bkt], 1u);
    }
    scan_classes(1);
    for (int g = i; g < full; g += ORDER_THREADS) {
        const unsigned s = gtmp[g];
        const int r = (int)(hist[s >> 20] + (s & 0xFFFFFu));                 // rank among the groups, most expensive first
        const int q = r / ORDER_XCDS, c = r - q * ORDER_XCDS;
        gtmp[g] = q < rows ? (unsigned)((q & 1) ? ORDER_XCDS - 1 - c : c) : (unsigned)ORDER_XCDS;
    }
    __syncthreads();
    const unsigned tail = (unsigned)(ORDER_XCDS * rows * gb);                // first position behind the rows
    {   // 3. the same XCD assignment in tile order: thread i owns the groups [i per, (i + 1) per); for every class an exclusive
        // scan over the threads of how many of its groups they own gives each group its rank within its class
        unsigned *seq = order + nblocks;
        const int per = (full + ORDER_THREADS - 1) / ORDER_THREADS;
        const int g0 = i * per < full ? i * per : full, g1 = g0 + per < full ? g0 + per : full;
        unsigned base[ORDER_XCDS + 1];
        for (int c = 0; c <= ORDER_XCDS; ++c) {
            unsigned v = 0;
            for (int g = g0; g < g1; ++g) v += gtmp[g] == (unsigned)c ? 1u : 0u;
            unsigned incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            __syncthreads();
            if (lane == 63) scan[wv] = incl;
            __syncthreads();
            unsigned b0 = 0;
            for (int w = 0; w < wv; ++w) b0 += scan[w];
            base[c] = b0 + incl - v;
        }
        for (int g = g0; g < g1; ++g) {
            const unsigned c = gtmp[g];
            unsigned jg = 0;
#pragma unroll
            for (int cc = 0; cc <= ORDER_XCDS; ++cc) if (c == (unsigned)cc) jg = base[cc]++;
            for (int k = 0; k < gb; ++k) {
                const unsigned j = jg * (unsigned)gb + (unsigned)k;
                seq[place(c, j, tail)] = (unsigned)((g << gshift) + k);
            }
        }
        for (int b = (full << gshift) + i; b < nblocks; b += ORDER_THREADS) seq[b] = (unsigned)b;    // the short group: last, in place
    }
    __syncthreads();
    for (int k = i; k < (ORDER_XCDS + 1) * ORDER_BUCKETS; k += ORDER_THREADS) hist[k] = 0u;
    __syncthreads();
    // 2. blocks by their own cost, per XCD
    for (int b = i; b < nblocks; b += ORDER_THREADS) {
        const int g = b >> gshift;
        const unsigned x = g < full ? gtmp[g] : (unsigned)ORDER_XCDS;
        const int bkt = order_bucket(cost_of(b));
        btmp[b] = ((unsigned)bkt << 22) | atomicAdd(&hist[x * ORDER_BUCKETS + bkt], 1u);                  // items < 2^22 (host)
    }
    scan_classes(ORDER_XCDS + 1);
    for (int b = i; b < nblocks; b += ORDER_THREADS) {
        const int g = b >> gshift;
        const unsigned s = btmp[b], x = g < full ? gtmp[g] : (unsigned)ORDER_XCDS;
        const unsigned j = hist[x * ORDER_BUCKETS + (s >> 22)] + (s & 0x3FFFFFu);
        order[place(x, j, tail)] = (unsigned)b;
    }
}

}  // namespace rt
