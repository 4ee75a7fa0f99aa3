/* small_scene_check.cpp — rt::cull_groups (rt_plan.h), the choice between a two-wave ground-plane kernel and its small-scene twin
 * compiled for one or two cull groups (rt_device.h: NG), on scenes packed by the library's own packer (rt_scene.h), with the anchors
 * rt::anchors_of gives them, as a launch has them.
 * Prints one line per case, "<name> <groups>", and checks beside it that the choice changes nothing else of the plan: plan_launch's
 * family, shape, index and LDS bytes do not read the knob, and the twin the plan names (LaunchPlan::twin) has cull_groups where
 * has_small_kernel(shape), else 0, and ground_plane && has_ground_kernel(shape), for each of the three AA modes.  Then the shapes
 * that have such twins (has_small_kernel), one line each.
 *   small_scene_check          the table of tests/test_small_scene.py
 *   small_scene_check lights   one case, for a build with -DRT_MAX_CULL_TABLE_BYTES=2048: 8 spheres and 16 lights, whose anchored
 *                              table (17 rows of 128 bytes) is over that budget, so that anchors_of returns 0.  With the product's
 *                              budget of 40 KiB and RT_MAX_LIGHTS = 64 no scene of at most eight spheres gets there.
 * Built with AddressSanitizer and UBSan by tests/test_small_scene.py, which holds the expected answers. */
#include "../../python-ray-tracer_amd/csrc/rt_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

struct Normal { float x, y, z; };

/* S spheres in front of the camera, L lights, and planes through (0, 0, -1) with the given stored normals; `materials`: a table of
 * one row of three columns (the MAT family) */
static rt::PackedScene scene(int S, const std::vector<Normal> &normals, bool materials = false, int L = 3)
{
    const int P = (int)normals.size();
    std::vector<float> sph(7 * (size_t)S + 1), lights(3 * (size_t)L), planes(9 * (size_t)P + 1);
    for (int k = 0; k < S; ++k) {
        sph[0 * S + k] = 6.0f + (float)(k % 5); sph[1 * S + k] = (float)k - 1.0f; sph[2 * S + k] = 0.5f; sph[3 * S + k] = 0.5f;
        sph[4 * S + k] = sph[5 * S + k] = sph[6 * S + k] = 200.0f;
    }
    for (int m = 0; m < L; ++m) { lights[0 * L + m] = -2.0f + (float)m; lights[1 * L + m] = 3.0f; lights[2 * L + m] = 6.0f; }
    for (int k = 0; k < P; ++k) {
        planes[0 * P + k] = 0.0f; planes[1 * P + k] = 0.0f; planes[2 * P + k] = -1.0f;
        planes[3 * P + k] = normals[k].x; planes[4 * P + k] = normals[k].y; planes[5 * P + k] = normals[k].z;
        planes[6 * P + k] = planes[7 * P + k] = planes[8 * P + k] = 120.0f;
    }
    static const double table[3] = {0.1, 0.6, 0.3};
    std::vector<int32_t> smat(S + 1, 0), pmat(P + 1, 0);
    rt::SceneDesc d;
    d.spheres = sph.data(); d.lights = lights.data(); d.planes = P ? planes.data() : nullptr;
    d.S = S; d.L = L; d.P = P;
    if (materials) { d.materials = table; d.M = 1; d.ncols = 3; d.sphere_material = smat.data(); d.plane_material = pmat.data(); }
    const rt::PlanKnobs kn;
    return rt::pack_scene(d, rt::CLUSTER_MIN, kn.lanes_min_spheres);
}

static int failures = 0;

static void report(const char *name, const rt::PackedScene &ps, int flags = 0, int small_knob = 1, int ground_knob = 1, int want_anchors = -1)
{
    if (ps.status != RT_OK) { std::fprintf(stderr, "%s: pack_scene: %s\n", name, ps.error.c_str()); ++failures; return; }
    rt::PlanKnobs on, off;
    on.small_scene = small_knob; on.ground_plane = ground_knob;
    off.small_scene = 0; off.ground_plane = ground_knob;
    const rt::SceneLayout &lay = ps.layout;
    const rt::Family fam = rt::family_of(lay, 0.0);
    const int anchors = rt::anchors_of(lay);
    if (want_anchors >= 0 && anchors != want_anchors) { std::fprintf(stderr, "%s: anchors_of = %d, the case wants %d\n", name, anchors, want_anchors); ++failures; }
    const int g = rt::cull_groups(lay, on, fam, flags, anchors);
    for (int am = 0; am < 3; ++am) {
        const rt::LaunchPlan a = rt::plan_launch(lay, on, 0.0, am == 1, flags, am == 2, anchors);
        const rt::LaunchPlan b = rt::plan_launch(lay, off, 0.0, am == 1, flags, am == 2, anchors);
        if (a.family != b.family || !(a.shape == b.shape) || a.index != b.index || a.lds != b.lds) {
            std::fprintf(stderr, "%s: the plan depends on the knob\n", name); ++failures;
        }
        /* the twin the plan names is the predicate's answer where the shape has small-scene twins, else none */
        if (a.twin.groups != (rt::has_small_kernel(a.family, a.shape) ? g : 0) || b.twin.groups != 0) {
            std::fprintf(stderr, "%s: aa mode %d: the plan's cull groups are not cull_groups where has_small_kernel\n", name, am); ++failures;
        }
        if (a.twin.ground != (rt::ground_plane(lay, on, fam, flags) && rt::has_ground_kernel(a.family, a.shape)) || a.twin.ground != b.twin.ground) {
            std::fprintf(stderr, "%s: aa mode %d: the plan's twin is not ground_plane && has_ground_kernel\n", name, am); ++failures;
        }
        /* the table rows of a scene with groups are exactly those groups of four, and it plans a wave-uniform shape (whether a
         * two-wave one, which alone has the twins, is the LDS image's business: 64 lights make it a four-wave one) */
        if (g > 0 && (a.shape.mode >= 2 || (int)rt::padS(lay.S, lay.NC) != 4 * g)) {
            std::fprintf(stderr, "%s: %d groups, but mode %d padS %d\n", name, g, a.shape.mode, (int)rt::padS(lay.S, lay.NC)); ++failures;
        }
    }
    if (rt::cull_groups(lay, off, fam, flags, anchors)) { std::fprintf(stderr, "%s: groups with the knob off\n", name); ++failures; }
    if (g < 0 || g > rt::SMALL_MAX_GROUPS) { std::fprintf(stderr, "%s: %d groups\n", name, g); ++failures; }
    std::printf("%s %d\n", name, g);
}

int main(int argc, char **argv)
{
    const Normal up{0, 0, 1};
    if (argc > 1 && !std::strcmp(argv[1], "lights")) {
        report("s8_many_lights", scene(8, {up}, false, 16), 0, 1, 1, 0);
        report("s8_few_lights", scene(8, {up}, false, 14), 0, 1, 1, 15);      /* 15 rows of 128 bytes: inside the budget */
        return failures ? 1 : 0;
    }
    report("s0", scene(0, {up}));
    report("s1", scene(1, {up}));
    report("s4", scene(4, {up}));
    report("s5", scene(5, {up}));
    report("s8", scene(8, {up}));
    report("s9", scene(9, {up}));
    report("s21_clustered", scene(21, {up}));
    report("s8_tilted", scene(8, {Normal{0.0f, 0.6f, 0.8f}}));
    report("s8_two_planes", scene(8, {up, up}));
    report("s8_materials", scene(8, {up}, true));
    report("s8_count_rays", scene(8, {up}), RT_FLAG_COUNT_RAYS);
    report("s8_small_knob_off", scene(8, {up}), 0, 0, 1);
    report("s8_ground_knob_off", scene(8, {up}), 0, 1, 0);
    report("s8_64_lights", scene(8, {up}, false, RT_MAX_LIGHTS), 0, 1, 1, RT_MAX_LIGHTS + 1);   /* the most lights a scene can have: still anchored */
    /* the twins there are: "twin <aa> <park> <wpw> <lat> <mode>" per shape that has them; all are two-wave ground-plane twins */
    for (int fi = 0; fi < rt::FAMILIES; ++fi)
        for (const rt::Shape &s : rt::SHAPES) {
            const bool t = rt::has_small_kernel((rt::Family)fi, s);
            if (t && (!rt::has_ground_kernel((rt::Family)fi, s) || s.wpw != 2 || s.mode != 0)) {
                std::fprintf(stderr, "a small-scene twin of a kernel that is no two-wave ground-plane twin\n"); ++failures;
            }
            if (t) std::printf("twin %d%d%d%d%d 1\n", (int)s.aa, (int)s.park, s.wpw, (int)s.lat, s.mode);
        }
    return failures ? 1 : 0;
}
