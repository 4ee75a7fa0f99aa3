/* fixed_path_check.cpp — what the render kernels' once-per-tile path takes for granted (rt_device.h: render_kernel's prologue and
 * store_pixel), checked on the CPU against the general forms.  It compiles rt_math.h, rt_layout.h and rt_plan.h as the kernel does.
 *   fixed_path_check clip     rt::clip_color (rt_math.h), the straight-line clip of the trimmed kernels, and rt::clip_color_branches, the
 *                             clip of the others, against the rule written out below — NaN -> 0,
 *                             c <= -0.5 -> 0, c >= 255.5 -> 255, else rint(c) clamped to 0..255 — on +-0, +-inf, quiet and signalling
 *                             NaNs of both signs, denormals, k + 0.5 and both of its neighbours for k = -2..257, and 10^7 seeded random
 *                             bit patterns: equal bytes throughout.  Prints "clip <operands> ok".
 *   fixed_path_check layout   rt::flat_layout (rt_layout.h), the two fields of the table layout a two-wave kernel reads, against
 *                             rt::table_layout(S, NC, anchors, P): in its constant form (ng > 0) over every scene with cull_groups > 0
 *                             (S = 1..8, L = 0..RT_MAX_LIGHTS, packed by the library's packer), in its flat form (ng = 0) over those
 *                             and every flat scene up to rt::CLUSTER_MIN spheres; and rt::lds_bytes against the image's size formed
 *                             from flat_layout's total.  Prints "layout <scenes> ok".
 *   fixed_path_check plan     over the case grid of launch_plan_check.cpp (knob rows, sphere counts, planes, lights, families, AA
 *                             modes, flags): no plan sends a scene with NC > 0 to a two-wave shape, and no two-wave shape is other
 *                             than MODE 0.  Prints "plan <cases> <two-wave cases> ok".
 * Built with AddressSanitizer and UBSan by tests/test_fixed_path.py. */
#include "../../python-ray-tracer_amd/csrc/rt_math.h"
#include "../../python-ray-tracer_amd/csrc/rt_layout.h"
#include "../../python-ray-tracer_amd/csrc/rt_plan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;

/* ---- clip ---- */

static double from_bits(uint64_t b) { double d; std::memcpy(&d, &b, sizeof d); return d; }
static uint64_t to_bits(double d) { uint64_t b; std::memcpy(&b, &d, sizeof b); return b; }

/* the rule, on the bit pattern where a NaN is concerned: no arithmetic touches one */
static uint8_t clip_rule(double c)
{
    const uint64_t b = to_bits(c), mag = b & 0x7fffffffffffffffull;
    if (mag > 0x7ff0000000000000ull) return 0;          /* NaN, quiet or signalling */
    if (c <= -0.5) return 0;
    if (c >= 255.5) return 255;
    const double r = std::nearbyint(c);                 /* round half to even (the default rounding mode) */
    const int i = (int)r;
    return (uint8_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
}

static long clip_one(double c)
{
    const uint8_t want = clip_rule(c), got = rt::clip_color(c), old = rt::clip_color_branches(c);
    if ((want != got || want != old) && failures < 20) {
        std::fprintf(stderr, "clip_color(%a = 0x%016llx) = %d, clip_color_branches = %d, the rule gives %d\n", c, (unsigned long long)to_bits(c),
                     (int)got, (int)old, (int)want);
        ++failures;
    }
    return 1;
}

static int check_clip()
{
    long n = 0;
    const uint64_t specials[] = {
        0x0000000000000000ull, 0x8000000000000000ull,                         /* +-0 */
        0x7ff0000000000000ull, 0xfff0000000000000ull,                         /* +-inf */
        0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff8000000000001ull, 0xfffc0000deadbeefull,   /* quiet NaNs */
        0x7ff0000000000001ull, 0xfff0000000000001ull, 0x7ff4000000000000ull, 0xfff7ffffffffffffull,   /* signalling NaNs */
        0x0000000000000001ull, 0x8000000000000001ull, 0x000fffffffffffffull, 0x800fffffffffffffull,   /* denormals */
        0x0010000000000000ull, 0x8010000000000000ull, 0x7fefffffffffffffull, 0xffefffffffffffffull,   /* smallest normals, largest finite */
    };
    for (uint64_t b : specials) n += clip_one(from_bits(b));
    for (int k = -2; k <= 257; ++k) {
        const double t = (double)k + 0.5;
        n += clip_one(t);
        n += clip_one(std::nextafter(t, -INFINITY));
        n += clip_one(std::nextafter(t, INFINITY));
        n += clip_one((double)k);
    }
    uint64_t s = 0x9E3779B97F4A7C15ull;                                       /* splitmix64, seeded */
    for (long i = 0; i < 10000000; ++i) {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        /* every fourth pattern as it is (any exponent, NaNs included); the others with the exponent folded into 2^-4 .. 2^11,
         * either sign, where the rule's branches meet */
        const uint64_t b = (i & 3) == 0 ? z : ((z & 0x800fffffffffffffull) | ((uint64_t)(1019 + (z >> 52) % 16) << 52));
        n += clip_one(from_bits(b));
    }
    if (!failures) std::printf("clip %ld ok\n", n);
    return failures ? 1 : 0;
}

/* ---- layout ---- */

/* S spheres, L lights and the ground plane, through the library's packer (as small_scene_check.cpp builds them) */
static rt::PackedScene scene(int S, int L)
{
    const int P = 1;
    std::vector<float> sph(7 * (size_t)S + 1), lights(3 * (size_t)L + 1), planes(9 * (size_t)P);
    for (int k = 0; k < S; ++k) {
        sph[0 * S + k] = 6.0f + (float)(k % 5); sph[1 * S + k] = (float)k - 1.0f; sph[2 * S + k] = 0.5f; sph[3 * S + k] = 0.5f;
        sph[4 * S + k] = sph[5 * S + k] = sph[6 * S + k] = 200.0f;
    }
    for (int m = 0; m < L; ++m) { lights[0 * L + m] = -2.0f + (float)m; lights[1 * L + m] = 3.0f; lights[2 * L + m] = 6.0f; }
    planes[0] = 0.0f; planes[1] = 0.0f; planes[2] = -1.0f;
    planes[3] = 0.0f; planes[4] = 0.0f; planes[5] = 1.0f;
    planes[6] = planes[7] = planes[8] = 120.0f;
    rt::SceneDesc d;
    d.spheres = sph.data(); d.lights = lights.data(); d.planes = planes.data();
    d.S = S; d.L = L; d.P = P;
    const rt::PlanKnobs kn;
    return rt::pack_scene(d, rt::CLUSTER_MIN, kn.lanes_min_spheres);
}

/* the LDS image of a PLAIN kernel of shape s, formed from the flat layout's total (rt_layout.h: lds_bytes, two-wave MODE 0) */
static size_t image_from_flat(const rt::SceneLayout &lay, const rt::Shape &s, unsigned total)
{
    const int wgt = 64 * s.wpw;
    return (rt::lds_doubles(lay.S, lay.P, lay.L) + (size_t)rt::lds_slots(s.aa, s.park, false, rt::Family::PLAIN) * wgt) * sizeof(double) +
           ((size_t)rt::lds_offset_words(s.park, wgt) + total) * sizeof(float) + 16;
}

static void layout_case(const rt::SceneLayout &lay, int anchors, int ng, const char *what)
{
    const rt::TableLayout t = rt::table_layout(lay.S, lay.NC, anchors, lay.P);
    const rt::FlatLayout f = rt::flat_layout(ng, lay.S, lay.L, anchors);
    /* a two-wave kernel is MODE 0: it reads `tab`, and stages and puts its workgroup words behind `total` (== total_lanes, flat) */
    if (f.tab != t.tab || f.total != t.total || t.total != t.total_lanes) {
        std::fprintf(stderr, "%s S=%d L=%d anchors=%d ng=%d: flat_layout {%u, %u}, table_layout {%zu, %zu (lanes %zu)}\n", what, lay.S, lay.L,
                     anchors, ng, f.tab, f.total, t.tab, t.total, t.total_lanes);
        ++failures;
    }
    for (const rt::Shape &s : rt::SHAPES) {
        if (s.wpw != 2) continue;
        if (rt::lds_bytes(lay, anchors, rt::Family::PLAIN, s) != image_from_flat(lay, s, f.total)) {
            std::fprintf(stderr, "%s S=%d L=%d: lds_bytes is not the image formed from flat_layout\n", what, lay.S, lay.L);
            ++failures;
        }
    }
}

static int check_layout()
{
    const rt::PlanKnobs kn;
    long scenes = 0;
    for (int S = 1; S <= rt::CLUSTER_MIN; ++S)
        for (int L = 0; L <= RT_MAX_LIGHTS; ++L) {
            const rt::PackedScene ps = scene(S, L);
            if (ps.status != RT_OK) { std::fprintf(stderr, "S=%d L=%d: pack_scene: %s\n", S, L, ps.error.c_str()); return 1; }
            const rt::SceneLayout &lay = ps.layout;
            if (lay.NC != 0) { std::fprintf(stderr, "S=%d: the packer clustered a scene of at most CLUSTER_MIN spheres\n", S); return 1; }
            const rt::Family fam = rt::family_of(lay, 0.0);
            const int anchors = rt::anchors_of(lay);
            const int g = rt::cull_groups(lay, kn, fam, 0, anchors);
            if ((S <= 4 * rt::SMALL_MAX_GROUPS) != (g > 0)) { std::fprintf(stderr, "S=%d L=%d: cull_groups %d\n", S, L, g); ++failures; }
            if (g > 0) layout_case(lay, anchors, g, "small-scene form");
            layout_case(lay, anchors, 0, "flat form");
            layout_case(lay, 0, 0, "flat form, no anchored table");
            ++scenes;
        }
    if (!failures) std::printf("layout %ld ok\n", scenes);
    return failures ? 1 : 0;
}

/* ---- plan: launch_plan_check.cpp's case grid ---- */

/* cluster_min, lanes_min_spheres, f32_records, lanes_park, wpw2_max_image, order_group, order_tiles, seq_order */
static const int KNOBS[][8] = {
    {rt::CLUSTER_MIN, 161, 1, 1, 4608, -1, 1, -1},
    {20, 161, 1, 1, 0, -1, 1, -1},
    {100000, 100000, 1, 1, 0, -1, 1, -1},
    {100000, 100000, 1, 1, 10000000, -1, 1, -1},
    {100000, 100000, 0, 1, 0, -1, 1, -1},
    {100000, 100000, 1, 1, 4608, -1, 1, -1},
    {20, 30, 1, 1, 4608, -1, 1, -1},
    {20, 30, 1, 0, 4608, -1, 1, -1},
    {20, 100000, 1, 1, 4608, -1, 1, -1},
    {20, 100000, 0, 1, 4608, -1, 1, -1},
    {20, 161, 1, 1, 4608, 0, 1, -1},
    {20, 161, 1, 1, 4608, -1, 0, -1},
    {20, 161, 1, 1, 4608, -1, 1, 0},
    {20, 161, 1, 1, 4608, -1, 1, 1},
};
static const int SPHERES[] = {0, 1, 8, 16, 20, 21, 25, 36, 64, 100, 144, 160, 161, 256, 400};

static rt::SceneLayout layout_of(rt::Family f, int S, int P, int L, int cluster_min)
{
    rt::SceneLayout lay;
    lay.S = S; lay.P = P; lay.L = L;
    lay.NC = S > cluster_min ? (S + rt::CLUSTER - 1) / rt::CLUSTER : 0;       /* the packer's rule */
    lay.M = rt::has_mat(f) ? 4 : 0;
    lay.mat_cols = rt::table_cols(f);
    lay.soft_n = rt::has_soft(f) ? 2 : 0;
    lay.T = rt::has_tex(f) && !rt::has_lit(f) ? 1 : 0;
    lay.lit = rt::has_lit(f);
    lay.sky = rt::has_sky(f);
    return lay;
}

static int check_plan()
{
    long cases = 0, two = 0;
    for (const auto &row : KNOBS) {
        rt::PlanKnobs kn;
        kn.lanes_min_spheres = row[1]; kn.f32_records = row[2]; kn.lanes_park = row[3];
        kn.wpw2_max_image = (size_t)row[4]; kn.order_group = row[5]; kn.order_tiles = row[6]; kn.seq_order = row[7];
        for (int S : SPHERES) for (int P : {0, 2}) for (int L : {1, 3}) for (int fi = 0; fi < rt::FAMILIES; ++fi) {
            const rt::Family f = (rt::Family)fi;
            const rt::SceneLayout lay = layout_of(f, S, P, L, row[0]);
            const double lens_a = rt::has_lens(f) ? 0.05 : 0.0;
            const int anchors = rt::anchors_of(lay);
            for (int am = 0; am < 3; ++am) for (int cnt = 0; cnt < (f == rt::Family::PLAIN ? 2 : 1); ++cnt) for (int nb = 0; nb < 2; ++nb) {
                const int flags = (cnt ? RT_FLAG_COUNT_RAYS : 0) | (nb ? RT_FLAG_NO_BUNDLES : 0);
                const rt::LaunchPlan pl = rt::plan_launch(lay, kn, lens_a, am == 1, flags, am == 2, anchors);
                ++cases;
                if (pl.shape.wpw != 2) continue;
                ++two;
                if (lay.NC != 0 || pl.shape.mode != 0) {
                    std::fprintf(stderr, "S=%d P=%d L=%d family %d aa %d flags %d: a two-wave shape with NC = %d, mode %d\n", S, P, L, fi, am, flags,
                                 lay.NC, pl.shape.mode);
                    ++failures;
                }
            }
        }
    }
    for (const rt::Shape &s : rt::SHAPES)                                   /* ... and the table has no two-wave shape of another mode */
        if (s.wpw == 2 && s.mode != 0) { std::fprintf(stderr, "SHAPES: a two-wave shape of mode %d\n", s.mode); ++failures; }
    if (!failures) std::printf("plan %ld %ld ok\n", cases, two);
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    if (!std::strcmp(argv[1], "clip")) return check_clip();
    if (!std::strcmp(argv[1], "layout")) return check_layout();
    if (!std::strcmp(argv[1], "plan")) return check_plan();
    return 2;
}
