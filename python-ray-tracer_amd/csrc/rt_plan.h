// rt_plan.h — everything about a launch of the render kernel that is decided before a HIP call: the feature family, which of the
// family's kernels runs (its shape: workgroup size, lane-owned or wave-uniform, MODE 1 or not, parked or not), with how much
// dynamic LDS, and the shape of the dispatch order (group shift, tile or block items, seq_offset).
// HIP-free, like rt_geometry.h and rt_scene.h and for the same reason: a pure choice on the scene's layout, the MI355RT_* knobs,
// the AA mode and the flags, testable where there is no GPU.  The plan names the kernel completely: family, shape and twin (the
// ground-plane or small-scene instantiation of that shape), so the row and column of the one table of kernels' addresses that
// mi355rt.hip keeps (KERNELS, built from row_kernels and SHAPES).  mi355rt.hip launches what the plan says;
// tests/algo/launch_plan_check.cpp walks the plan over a table of scenes and knobs under AddressSanitizer and UBSan and compares
// it with the recorded choice.
#pragma once
#include "rt_layout.h"
#include "rt_scene.h"
#include "rt_geometry.h"

#include <algorithm>
#include <cstddef>

namespace rt {

// The knobs that steer the choice (rt_create fills them from the environment).
struct PlanKnobs {
    int lanes_min_spheres = 161;      // MI355RT_LANES_MINS: the lane-owned traversal from that size on
    int f32_records = 1;              // MI355RT_F32_RECORDS: four-wave wave-uniform kernels keep no float64 sphere records in LDS (MODE 1)
    size_t wpw2_max_image = 4608;     // MI355RT_WPW2_MAX_IMAGE: flat scenes whose LDS image is at most this many bytes run two-wave workgroups
    int lanes_park = 1;               // MI355RT_LANES_PARK=0: register variants of the lane-owned kernels (A/B; with workgroups of equal-cost tiles the
                                      // parked variants win: config 5 6.88 against 7.16 ms — with neighbouring tiles they lost, 8.20 against 7.95)
    int order_group = -1;             // MI355RT_ORDER_GROUP: log2 of the blocks per XCD-affine dispatch group (0..6; 0 = every block on its
                                      // own; default -1 = groups of 16 tiles)
    int order_tiles = 1;              // MI355RT_ORDER_TILES=0: the four-wave kernels' dispatch order per block of four neighbouring tiles (A/B)
    int seq_order = -1;               // MI355RT_SEQ_ORDER: 1 / 0 = all but the last frame of a multi-frame launch in the XCD's tile order / every
                                      // frame longest-first; default -1 = tile order for the two-wave kernels (small flat scenes: headline
                                      // 0.1050 ms either way, writes 31.8 instead of 38.7 MB per frame), longest-first for the four-wave ones
                                      // (config 4: 0.734 against 0.785 ms — runs of cheap sky tiles starve the dispatcher in tile order)
    int ground_plane = 1;             // MI355RT_GROUND_PLANE=0: scenes with the reference's single z-up ground plane run the generic kernels
                                      // too (A/B, and the tests that compare the twins with them)
    int small_scene = 1;              // MI355RT_SMALL_SCENE=0: scenes of at most eight spheres run the ground-plane twins compiled for any sphere
                                      // count (A/B, and the tests that compare the small-scene twins with them)
};

// The feature family of a launch: which render kernels it runs, and how many per-thread slots and material columns those
// have.  From the scene (rt::SceneLayout: M materials in a table of mat_cols columns, soft_n shadow samples per light, ...) and the
// lens aperture.
inline Family family_of(const SceneLayout &s, double lens_a)
{
    using F = Family;
    const bool lens = lens_a > 0.0, soft = s.soft_n > 0;
    if (s.M <= 0) return F::PLAIN;
    if (s.sky)                                                       // (rt_scene.h: a sky only with M >= 1; it sets lit too)
        return lens ? (soft ? F::SKY_LENS_SOFT : F::SKY_LENS) : (soft ? F::SKY_SOFT : F::SKY_SCAT);
    if (s.lit)                                                       // (rt_scene.h: lit only with M >= 1; textured or not)
        return lens ? (soft ? F::LIT_LENS_SOFT : F::LIT_LENS) : (soft ? F::LIT_SOFT : F::LIT_SCAT);
    if (s.T > 0)                                                     // (rt_scene.h: T > 0 only with a textured object, and M >= 1)
        return lens ? (soft ? F::TEX_LENS_SOFT : F::TEX_LENS) : (soft ? F::TEX_SOFT : F::TEX_SCAT);
    if (lens) return soft ? F::LENS_SOFT : F::LENS;                  // (check_params: a lens needs a material table)
    return block_family(s.M, s.mat_cols, soft);                      // SOFT, SCAT, REFR or MAT: the family of the scene's own material block
}

// The shape of a launch (plan_launch): render_kernel's first six template arguments.
struct Shape {
    bool aa, park;
    int wpw;
    bool count, lat;
    int mode;    // 0: wave-uniform cull; 1: the same without float64 sphere records in LDS; 2: lane-owned traversal; 3: its AA + parked variant
    constexpr bool operator==(const Shape &o) const
    {
        return aa == o.aa && park == o.park && wpw == o.wpw && count == o.count && lat == o.lat && mode == o.mode;
    }
};

// Every shape plan_launch can produce.
constexpr Shape SHAPES[] = {
    // wave-uniform cull, workgroups of 2 or 4 (flat scenes up to rt::CLUSTER_MIN spheres may take 2), with AA or without, register
    // or parked variant; MODE 1: workgroups of 4 without AA that keep no float64 sphere records in LDS (rt_device.h: sphere_hot)
    {false, false, 2, false, false, 0}, {false, true, 2, false, false, 0}, {true, false, 2, false, false, 0}, {true, true, 2, false, false, 0},
    {false, false, 4, false, false, 0}, {false, true, 4, false, false, 0}, {true, false, 4, false, false, 0}, {true, true, 4, false, false, 0},
    {false, false, 4, false, false, 1}, {false, true, 4, false, false, 1},
    // the same over the half-pixel lattice (RT_AA_REFERENCE on the closed-form grid: no AA of their own)
    {false, false, 2, false, true, 0}, {false, true, 2, false, true, 0}, {false, false, 4, false, true, 0}, {false, true, 4, false, true, 0},
    {false, false, 4, false, true, 1}, {false, true, 4, false, true, 1},
    // lane-owned traversal (MODE 2, clustered scenes from lanes_min_spheres spheres on), workgroups of 4; with AA and parked: MODE 3
    {false, false, 4, false, false, 2}, {false, true, 4, false, false, 2}, {true, false, 4, false, false, 2}, {true, true, 4, false, false, 3},
    {false, false, 4, false, true, 2}, {false, true, 4, false, true, 2},
    // rt_get_stats: the register variants with workgroups of 4 carry the ray counters
    {false, false, 4, true, false, 0}, {true, false, 4, true, false, 0}, {false, false, 4, true, true, 0},
};
constexpr int NSHAPES = sizeof SHAPES / sizeof SHAPES[0];
constexpr int shape_index(const Shape &s)    // in SHAPES, or -1
{
    for (int i = 0; i < NSHAPES; ++i)
        if (SHAPES[i] == s) return i;
    return -1;
}

// A family has one render kernel per shape, except
//  * the counting shapes, which PLAIN alone has (check_params refuses RT_FLAG_COUNT_RAYS for a scene with materials), and
//  * the parked wave-uniform shapes (MODE 0 and 1) from REFR on, which the parking rule never picks (the static_assert below).
// So PLAIN has 25 kernels, MAT 22 and every later family (the four texture, the four lighting and the four sky families included) 14.  Nothing else names a render kernel of a family other than
// PLAIN, so the kernels a family does not have are not compiled.
constexpr bool has_kernel(Family f, const Shape &s)
{
    return (!s.count || f == Family::PLAIN) && !(has_refr(f) && s.park && s.mode < 2);
}

// The ground-plane twins (rt_device.h: GROUND): kernels of the PLAIN family that do not count rays have a second
// instantiation, compiled for a scene whose only plane has the stored normal (0,0,1): the reference's ground, which every
// BASELINE workload has.  ground_plane says whether a launch is of such a scene, has_ground_kernel whether its shape has a twin;
// a launch for which both hold runs the twin.  The choice is a dimension of its own: the plan's family, shape, index and LDS size
// do not depend on it (a twin stages the same LDS image as its generic kernel).
// `code0`: plane 0's axis code, the low byte of SceneLayout::plane_codes (+3: exactly +e_z).
// Six of PLAIN's 22 shapes that do not count rays have no twin: measured against the parent's kernel of the same shape
// (profiles/ground_plane_shapes.txt), theirs gained 0.3 to 1.1 %, which is within what register allocation alone moves these
// kernels by; the other 16 gained 2.4 to 5.8 %.  All six are register variants (park = false).  A launch of one of them runs the
// generic kernel whatever ground_plane says.
constexpr Shape NO_GROUND_TWIN[] = {
    {false, false, 2, false, false, 0}, {true, false, 2, false, false, 0},      // two-wave register variants, without AA and with
    {false, false, 4, false, false, 1}, {false, false, 4, false, true, 1},      // MODE 1 register variants
    {false, false, 4, false, false, 2}, {false, false, 4, false, true, 2},      // lane-owned register variants without an AA mode of their own
};
constexpr bool has_ground_kernel(Family f, const Shape &s)
{
    if (f != Family::PLAIN || s.count) return false;
    for (const Shape &n : NO_GROUND_TWIN)
        if (n == s) return false;
    return true;
}

inline bool ground_plane(const SceneLayout &lay, const PlanKnobs &kn, Family fam, int flags)
{
    const int code0 = (int)(signed char)(lay.plane_codes & 0xffu);
    return kn.ground_plane != 0 && fam == Family::PLAIN && !(flags & RT_FLAG_COUNT_RAYS) && lay.P == 1 && code0 == 3;
}

// The small-scene twins (rt_device.h: NG, render_kernel's last template argument): two-wave ground-plane twins have further
// instantiations compiled for a flat scene of at most eight spheres, whose cull-table rows are one or two groups of four: the
// queries run no chunk loop and no loop over the groups.  A dimension of its own beside ground_plane, like it: the plan's family,
// shape, index and LDS size do not depend on it (the twins stage the same LDS image).
// cull_groups: the groups (1: 1 to 4 spheres, 2: 5 to 8) a launch's kernel may be compiled for, or 0: the launch is of a scene
// with the ground plane (ground_plane), flat, with 1 to 8 spheres and the anchored tables of all its lights (`anchors`: the launch's,
// anchors_of(lay) or 0).  has_small_kernel: the shape has such twins; a launch for which both hold runs one.
// Three shapes were candidates, the two-wave parked ground twins (every two-wave register variant runs the generic kernel or is
// LDS-bound); SMALL_TWIN names the ones whose twins gained more than register allocation alone moves these kernels by
// (profiles/small_scene_shapes.txt).
constexpr int SMALL_MAX_GROUPS = 2;
constexpr Shape SMALL_TWIN[] = {
    {false, true, 2, false, false, 0},      // the headline kernel
    {true, true, 2, false, false, 0},       // with AA
    {false, true, 2, false, true, 0},       // over the half-pixel lattice
};
constexpr bool has_small_kernel(Family f, const Shape &s)
{
    if (!has_ground_kernel(f, s)) return false;
    for (const Shape &k : SMALL_TWIN)
        if (k == s) return true;
    return false;
}

inline int cull_groups(const SceneLayout &lay, const PlanKnobs &kn, Family fam, int flags, int anchors)
{
    if (!ground_plane(lay, kn, fam, flags) || kn.small_scene == 0) return 0;
    if (lay.NC != 0 || lay.S < 1 || lay.S > 4 * SMALL_MAX_GROUPS || anchors != lay.L + 1) return 0;
    return (lay.S + 3) / 4;
}

// The twin of family fam's kernel of shape s that a launch runs (LaunchPlan names it): both predicates above with the shape's say.
// `flags` and `anchors` are the launch's, as plan_launch has them.
struct Twin {
    bool ground;    // the ground-plane twin
    int groups;     // > 0: of that twin, the small-scene twin for so many cull groups
};
inline Twin twin_of(const SceneLayout &lay, const PlanKnobs &kn, Family fam, const Shape &s, int flags, int anchors)
{
    return Twin{ground_plane(lay, kn, fam, flags) && has_ground_kernel(fam, s),
                has_small_kernel(fam, s) ? cull_groups(lay, kn, fam, flags, anchors) : 0};
}

// The render kernels stand in one table (mi355rt.hip: KERNELS) of ROWS rows of NSHAPES: a row per family, then the ground-plane
// twins' row, then a row of small-scene twins per number of cull groups.
constexpr int GROUND_ROW = FAMILIES, ROWS = FAMILIES + 1 + SMALL_MAX_GROUPS;
struct Row {
    Family family;
    bool ground;
    int groups;
};
constexpr Row row_kernels(int row)
{
    return row < FAMILIES ? Row{(Family)row, false, 0} : Row{Family::PLAIN, true, row - GROUND_ROW};
}
constexpr int row_of(Family fam, const Twin &t) { return t.groups > 0 ? GROUND_ROW + t.groups : (t.ground ? GROUND_ROW : (int)fam); }
// Whether the table has a kernel of shape s in that row: has_kernel, has_ground_kernel and has_small_kernel are its cases.
constexpr bool row_has_kernel(int row, const Shape &s)
{
    const Row r = row_kernels(row);
    return r.groups > 0 ? has_small_kernel(r.family, s) : (r.ground ? has_ground_kernel(r.family, s) : has_kernel(r.family, s));
}

// The parking rule of the wave-uniform kernels (plan_launch): their state parks in LDS while PARK_WAVES wavefronts per CU still
// fit their workgroups' LDS images.
constexpr int PARK_WAVES = 24;
constexpr size_t CU_LDS = 160 * 1024;

// A kernel a family does not have (counting kernels aside) is one that no scene lets park: its per-thread slots, pixel offsets
// and workgroup words alone (rt::lds_bytes of an empty scene) take more than CU_LDS at PARK_WAVES wavefronts.  For REFR without
// AA that is 13 slots: 13 840 B x 12 workgroups of 2 = 166 080 B and 27 664 B x 6 workgroups of 4 = 165 984 B against 163 840 B.
constexpr bool missing_kernels_never_park()
{
    for (int fi = 0; fi < FAMILIES; ++fi)
        for (const Shape &s : SHAPES) {
            const Family f = (Family)fi;
            if (s.count || has_kernel(f, s)) continue;
            const size_t wgt = 64 * s.wpw;
            const size_t least = lds_slots(s.aa, true, s.mode >= 2, f) * wgt * sizeof(double) +
                                 wgt * sizeof(int) + 16;
            if (!s.park || s.mode >= 2 || least * (PARK_WAVES / s.wpw) <= CU_LDS) return false;
        }
    return true;
}
static_assert(missing_kernels_never_park(), "the parking rule can pick a render kernel that is not compiled");

// anchored cull table (camera + one anchor per light) if it fits its LDS budget, else origin-form culling only
inline int anchors_of(const SceneLayout &lay)
{
    const size_t table = (size_t)(lay.L + 1) * (padS(lay.S, lay.NC) + pad4(lay.NC)) * CULL_STRIDE * sizeof(float);
    return (table <= (size_t)MAX_CULL_TABLE_BYTES) ? lay.L + 1 : 0;
}

// The dynamic LDS of family f's kernel of shape s over a scene: lane-owned kernels (MODE 2 and 3) with anchored tables leave the
// clusters' origin-form spheres out of LDS, and they and the MODE 1 kernels the float64 sphere records.
inline size_t lds_bytes(const SceneLayout &lay, int anchors, Family f, const Shape &s)
{
    const bool lanes = s.mode >= 2;
    return lds_bytes(lay.S, lay.P, lay.L, lay.NC, anchors, s.aa, s.park, 64 * s.wpw, lanes && anchors > 0, lanes, s.mode == 1, f, lay.M);
}

struct LaunchPlan {
    Family family;
    Shape shape;
    int index;      // of shape in SHAPES
    size_t lds;     // dynamic LDS bytes of the launch
    Twin twin;      // which twin of that kernel runs (twin_of): a dimension of its own, nothing above depends on it
    int row() const { return row_of(family, twin); }   // the kernel is KERNELS[row()][index]
};

// Chooses the kernel instantiation for a launch: `aa`: the launch has an AA mode of its own (a lattice launch has none), `flags`:
// rt_params.flags, `lattice`: it renders the half-pixel lattice of RT_AA_REFERENCE, `anchors`: anchors_of(lay).
// Workgroup size: 2 tiles (wavefronts) for scenes whose LDS image (records + cull tables) is small, 4 otherwise
// (every workgroup stages its own copy; rt_layout.h has the measurements).
// Kernel variant: state parked in LDS (7 waves/SIMD, no scratch) while at least PARK_WAVES wavefronts per CU still
// fit their workgroups' LDS images; otherwise the register variant (its occupancy is then LDS-bound anyway).
// The kernel is the family's of the launch's shape, or the twin of it that twin_of names (mi355rt.hip: KERNELS).
inline LaunchPlan plan_launch(const SceneLayout &lay, const PlanKnobs &kn, double lens_a, bool aa, int flags, bool lattice, int anchors)
{
    const Family fam = family_of(lay, lens_a);
    const bool count = (flags & RT_FLAG_COUNT_RAYS) != 0;
    const size_t image = lds_doubles(lay.S, lay.P, lay.L) * sizeof(double) + table_floats(lay.S, lay.NC, anchors) * sizeof(float);
    // Scenes with more than rt::CLUSTER_MIN spheres are clustered (rt_set_scene) and culled cluster by cluster; from 161
    // spheres on with the lane-owned traversal and its groups of clusters (rt_device.h, MODE 2; compiled for 128 VGPRs,
    // 4 waves/SIMD).  Measured against the plain wave-uniform cull of the same clusters
    // (profiles/r02_variant_thresholds.txt): 256 spheres -25 %, 196 spheres -4 % (depth 3) .. -9 % (depth 8), 169 -8 %,
    // but 144 +6 %, 100 +17 %.
    // (Round 2's bundle pre-cull, MODE 1/3, lost against these clusters at every measured size and was removed in round 3:
    // profiles/r02_variant_thresholds.txt.)
    const bool lanes = lay.NC > 0 && lay.S >= kn.lanes_min_spheres && !count && !(flags & RT_FLAG_NO_BUNDLES);
    const int wpw = (image <= kn.wpw2_max_image && !count && lay.NC == 0) ? 2 : 4;   // flat scenes only (up to rt::CLUSTER_MIN spheres); measured at 1080p, depth 3 on flat scenes: 2 wins up to 25 spheres (4.1 KB), 4 from 36 (5.4 KB)
    auto bytes = [&](bool park, int mode) { return lds_bytes(lay, anchors, fam, Shape{aa, park, wpw, count, lattice, mode}); };
    // MODE 1 (wave-uniform cull, four-wave workgroups, no float64 sphere records in LDS: sphere_hot widens the float32 table
    // and a hit's colour comes from global memory) where the smaller image lets a CU hold one workgroup more — the parked
    // variant runs 7 per CU if they fit and needs 6, the register variant 5.  Config 4 (64 spheres): 6 -> 7 workgroups, -5 %;
    // 100 spheres: register variant at 5 -> parked at 6, -7 %; where the count stays (36, 49, 144 spheres) it costs 0...2 %
    // (four conversions per sphere test), and the AA kernels lose 1.5 % with it: those keep MODE 0.
    // The feature family picks the twins of these variants: their LDS images hold the material block too
    // (rt::mat_doubles: rows of rt::table_cols, the lens kernels' from rt::SceneLayout::lens_mat), and their parked variants the
    // family's per-thread slots (rt::lds_slots).
    auto per_cu = [&](int mode) {
        const size_t lp = bytes(true, mode);
        if (lp * 6 <= CU_LDS) return (int)std::min<size_t>(7, CU_LDS / lp);
        return (int)std::min<size_t>(5, CU_LDS / bytes(false, mode));
    };
    const bool norec = !lanes && !count && !aa && wpw == 4 && kn.f32_records && per_cu(1) > per_cu(0);
    const int mode = lanes ? 2 : (norec ? 1 : 0);
    const size_t lds_park = bytes(true, mode);
    // (lane-owned kernels are compiled for 4 waves per SIMD = 4 workgroups per CU: parked state while those still fit)
    const bool park = !count && (lanes ? (lds_park * RT_W_LANES <= CU_LDS && kn.lanes_park) : lds_park * (PARK_WAVES / wpw) <= CU_LDS);
    LaunchPlan pl;
    pl.family = fam;
    pl.shape = Shape{aa, park, wpw, count, lattice, lanes && aa && park ? 3 : mode};
    pl.lds = park ? lds_park : bytes(false, mode);
    pl.index = shape_index(pl.shape);
    pl.twin = twin_of(lay, kn, fam, pl.shape, flags, anchors);
    return pl;
}

// rt_render_guides (rt_guides.h: guides_kernel): the table mode of its closest_hit and the dynamic LDS of its four-wave workgroups.
// The mode is the one plan_launch gives a launch of the same scene without a material table, AA or flags (0, 1 or 2: what keeps
// the LDS image of a scene of RT_MAX_SPHERES small); the image is that of the register variant of that mode: no per-thread slots,
// no pixel offsets, no material block.
struct GuidesPlan {
    int mode;
    size_t lds;
};

inline GuidesPlan plan_guides(const SceneLayout &lay, const PlanKnobs &kn, int anchors)
{
    SceneLayout l = lay;
    l.M = 0; l.soft_n = 0; l.T = 0; l.lit = false; l.sky = false;
    const LaunchPlan pl = plan_launch(l, kn, 0.0, false, 0, false, anchors);
    GuidesPlan g;
    g.mode = pl.shape.mode >= 2 ? 2 : pl.shape.mode;
    g.lds = lds_bytes(l, anchors, Family::PLAIN, Shape{false, false, 4, false, false, g.mode});
    return g;
}

// The shape of the dispatch order of a planned launch over the grid g (rt_geo_plan_of with the plan's workgroup size; one dispatch).
struct OrderShape {
    bool feedback;   // the launch dispatches in a measured order (and may measure)
    int gshift;      // log2 of the blocks per XCD-affine group
    int wshift;      // log2 of the workgroup's waves
    bool otiles;     // the order's items are tiles, not blocks
    unsigned items;  // entries of one permutation
    int code;        // the workgroup size, + 32 lane-owned, + 64 tile items: what of the kernel's shape an order depends on (the feedback key)
    int seq_offset;  // KParams::seq_offset
};

inline OrderShape order_shape(const LaunchPlan &pl, const PlanKnobs &kn, int flags, const rt_geo_plan &g)
{
    const int wpw = pl.shape.wpw;
    const unsigned grid = (unsigned)g.blocks;
    OrderShape o;
    // Scheduler feedback (longest-first dispatch): a launch files its tile blocks by cost and dispatches in the
    // order built from the previous measured launch of the same range, depth and AA mode.
    // RT_FLAG_NO_FEEDBACK renders in plain tile order.  Any order renders every tile exactly once.
    o.feedback = !(flags & RT_FLAG_NO_FEEDBACK) && grid > 1 && grid < (1u << 20);
    // XCD-affine block groups (rt::order_kernel): runs of 2^gshift consecutive blocks (neighbours in y, which share 128-byte
    // lines of the output planes) are rendered by ONE XCD, so that its L2 completes those lines before they leave for HBM;
    // inside every XCD the order is block-level longest-first.  Default: groups of 16 tiles.  MI355RT_ORDER_GROUP overrides
    // (0 = every block on its own: round 2's order, 1.39x the algorithmic write traffic on the headline frame).
    o.gshift = kn.order_group >= 0 ? kn.order_group : (wpw == 2 ? 3 : 2);
    // Four-wave kernels: the order's items are TILES, not blocks of four neighbouring tiles (rt_device.h: KParams::order_tiles) —
    // a workgroup's four waves are then tiles of equal cost, end together and free their slots together.
    o.otiles = wpw >= TILE_ORDER_MIN_WPW && kn.order_tiles && o.feedback;
    o.wshift = wpw == 4 ? 2 : 1;
    o.items = o.otiles ? grid * (unsigned)wpw : grid;
    o.code = wpw + (pl.shape.mode >= 2 ? 32 : 0) + (o.otiles ? 64 : 0);
    o.seq_offset = (kn.seq_order < 0 ? wpw == 2 : kn.seq_order != 0) ? (int)o.items : 0;
    return o;
}

}  // namespace rt
