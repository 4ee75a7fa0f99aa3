/* The library's launch plan (python-ray-tracer_amd/csrc/rt_plan.h: which render kernel a launch runs, with how much LDS, in what
 * shape of dispatch order) without HIP, over a table of scenes, knobs, AA modes and flags.  Built with AddressSanitizer and
 * UndefinedBehaviorSanitizer and run by tests/test_algorithms.py, which compares what this writes with tests/golden/launch_plan.npz.
 *
 *   launch_plan_check OUT      writes int32 arrays to OUT: the knob rows (NKNOBS x 8), then per case its 8 coordinates
 *                              {knob row, S, P, L, family, AA (0 off, 1 on, 2 the lattice), RT_FLAG_COUNT_RAYS, RT_FLAG_NO_BUNDLES}
 *                              and its 13 results {family, the shape's aa, park, wpw, count, lat, mode, its index in SHAPES, LDS
 *                              bytes, anchors, gshift, the order's code, seq_offset != 0}
 * and prints "cases=N kernels=K table=T ok": K the (family, shape) pairs has_kernel admits, T the (row, shape) pairs of the whole
 * table of render kernels (row_has_kernel: the families' rows, the ground-plane twins' and the small-scene twins').  The order's
 * shape is that of a 32 x 24 frame (12 tiles: 3 or 6 workgroups, so feedback and tile-order items are live).  It fails if a case
 * plans a row and shape the table has no kernel for, or an LDS size that is not lds_bytes of the picked shape. */
#include "../../python-ray-tracer_amd/csrc/rt_plan.h"

#include <cstdint>
#include <cstdio>
#include <vector>

/* cluster_min, lanes_min_spheres, f32_records, lanes_park, wpw2_max_image, order_group, order_tiles, seq_order */
static const int KNOBS[][8] = {
    {rt::CLUSTER_MIN, 161, 1, 1, 4608, -1, 1, -1},       /* the defaults (main checks that they are PlanKnobs') */
    {20, 161, 1, 1, 0, -1, 1, -1},
    {100000, 100000, 1, 1, 0, -1, 1, -1},
    {100000, 100000, 1, 1, 10000000, -1, 1, -1},
    {100000, 100000, 0, 1, 0, -1, 1, -1},
    {100000, 100000, 1, 1, 4608, -1, 1, -1},
    {20, 30, 1, 1, 4608, -1, 1, -1},
    {20, 30, 1, 0, 4608, -1, 1, -1},
    {20, 100000, 1, 1, 4608, -1, 1, -1},
    {20, 100000, 0, 1, 4608, -1, 1, -1},
    {20, 161, 1, 1, 4608, 0, 1, -1},                     /* the order knobs, one at a time */
    {20, 161, 1, 1, 4608, -1, 0, -1},
    {20, 161, 1, 1, 4608, -1, 1, 0},
    {20, 161, 1, 1, 4608, -1, 1, 1},
};
static const int NKNOBS = sizeof KNOBS / sizeof KNOBS[0];
static const int SPHERES[] = {0, 1, 8, 16, 20, 21, 25, 36, 64, 100, 144, 160, 161, 256, 400};

/* a layout that family_of maps to f: M = 4 where the family has a table */
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

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const rt::PlanKnobs def;
    if (def.lanes_min_spheres != KNOBS[0][1] || def.f32_records != KNOBS[0][2] || def.lanes_park != KNOBS[0][3] ||
        def.wpw2_max_image != (size_t)KNOBS[0][4] || def.order_group != KNOBS[0][5] || def.order_tiles != KNOBS[0][6] ||
        def.seq_order != KNOBS[0][7]) {
        std::fprintf(stderr, "knob row 0 is not the defaults\n");
        return 1;
    }
    std::vector<int32_t> out;
    for (const auto &row : KNOBS) out.insert(out.end(), row, row + 8);
    long cases = 0;
    for (int kr = 0; kr < NKNOBS; ++kr) {
        rt::PlanKnobs kn;
        kn.lanes_min_spheres = KNOBS[kr][1]; kn.f32_records = KNOBS[kr][2]; kn.lanes_park = KNOBS[kr][3];
        kn.wpw2_max_image = (size_t)KNOBS[kr][4]; kn.order_group = KNOBS[kr][5]; kn.order_tiles = KNOBS[kr][6]; kn.seq_order = KNOBS[kr][7];
        for (int S : SPHERES) for (int P : {0, 2}) for (int L : {1, 3}) for (int fi = 0; fi < rt::FAMILIES; ++fi) {
            const rt::Family f = (rt::Family)fi;
            const rt::SceneLayout lay = layout_of(f, S, P, L, KNOBS[kr][0]);
            const double lens_a = rt::has_lens(f) ? 0.05 : 0.0;
            if (rt::family_of(lay, lens_a) != f) { std::fprintf(stderr, "family_of: not family %d\n", fi); return 1; }
            const int anchors = rt::anchors_of(lay);
            for (int am = 0; am < 3; ++am) for (int cnt = 0; cnt < (f == rt::Family::PLAIN ? 2 : 1); ++cnt) for (int nb = 0; nb < 2; ++nb) {
                const int flags = (cnt ? RT_FLAG_COUNT_RAYS : 0) | (nb ? RT_FLAG_NO_BUNDLES : 0);
                const rt::LaunchPlan pl = rt::plan_launch(lay, kn, lens_a, am == 1, flags, am == 2, anchors);
                if (pl.family != f || pl.index < 0 || !(rt::SHAPES[pl.index] == pl.shape) || !rt::row_has_kernel(pl.row(), pl.shape)) {
                    std::fprintf(stderr, "knobs %d S=%d P=%d L=%d family %d aa %d flags %d: no kernel of the picked shape\n", kr, S, P, L, fi, am, flags);
                    return 1;
                }
                if (pl.lds != rt::lds_bytes(lay, anchors, f, pl.shape)) {
                    std::fprintf(stderr, "knobs %d S=%d P=%d L=%d family %d aa %d flags %d: LDS bytes are not the picked shape's\n", kr, S, P, L, fi, am, flags);
                    return 1;
                }
                const rt::OrderShape os = rt::order_shape(pl, kn, flags, rt_geo_plan_of(0, 32, 24, pl.shape.wpw, 1));
                const int32_t rec[21] = {kr, S, P, L, fi, am, cnt, nb,
                                         (int)pl.family, pl.shape.aa, pl.shape.park, pl.shape.wpw, pl.shape.count, pl.shape.lat, pl.shape.mode,
                                         pl.index, (int32_t)pl.lds, anchors, os.gshift, os.code, os.seq_offset != 0};
                out.insert(out.end(), rec, rec + 21);
                ++cases;
            }
        }
    }
    int kernels = 0;
    for (int fi = 0; fi < rt::FAMILIES; ++fi)
        for (const rt::Shape &s : rt::SHAPES) kernels += rt::has_kernel((rt::Family)fi, s);
    int table = 0;                          /* ... and of every row: the families', the ground-plane twins', the small-scene twins' */
    for (int row = 0; row < rt::ROWS; ++row)
        for (const rt::Shape &s : rt::SHAPES) table += rt::row_has_kernel(row, s);
    FILE *fo = std::fopen(argv[1], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(int32_t), out.size(), fo) != out.size() || std::fclose(fo) != 0) return 1;
    std::printf("cases=%ld kernels=%d table=%d ok\n", cases, kernels, table);
    return 0;
}
