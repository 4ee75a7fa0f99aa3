"""The CPU side of the device harness of the kernels' exact-arithmetic primitives (tests/algo/device_math_kat.hip, driven on a GPU
by tests/test_gpu_device_math.py): the operand classes of tests/device_math_cases.py hold what their names say, the harness
cross-compiles for gfx950 with the library's own flags, its `host` mode (rt_math.h / rt_cull.h / rt_facing.h run on the host, no
HIP call) agrees bit for bit with the numpy references on 10^5 operands per class, and the property checkers of the dispatch order
and of the box test accept a valid construction and reject planted faults."""
import os
import subprocess

import numpy as np
import pytest

import device_math_cases as dm
from conftest import REPO

CSRC = os.path.join(REPO, "python-ray-tracer_amd", "csrc")
KAT = os.path.join(REPO, "tests", "algo", "build", "device_math_kat")


@pytest.fixture(scope="module")
def kat():
    """The harness, cross-compiled by the library's Makefile (its HIPCC and FLAGS, warnings as errors); make rebuilds it only when it
    is missing or older than its source or the headers."""
    res = subprocess.run(["make", "-C", CSRC, "kat"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert os.path.exists(KAT) and os.path.exists(KAT + "_generic")
    return KAT


def _host(kat, tmp_path, name, cols):
    src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
    n = dm.write_operands(src, cols)
    res = subprocess.run([kat, "host", name, src, dst], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return dm.read_results(dst, name, n)


def test_harness_cross_compiles_with_the_library_flags(kat):
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(HIPCC) $(FLAGS) -Werror -o $@ $(KAT_SRC)" in makefile
    assert "$(HIPCC) $(FLAGS) -Werror -DRT_FAST_NORMALIZE=0 -DRT_FAST_DIVSQRT=0 -o $@ $(KAT_SRC)" in makefile
    # the binaries land in tests/algo/build/, which .gitignore's `build/` (no leading slash: a directory of that name at any depth)
    # covers; read from the file itself, since the tree need not be a git checkout
    rules = [ln.strip() for ln in open(os.path.join(REPO, ".gitignore")) if ln.strip() and not ln.startswith("#")]
    assert os.path.basename(os.path.dirname(KAT)) == "build" and "build/" in rules and "!build/" not in rules
    assert "KAT_DIR := ../../tests/algo/build" in makefile


def test_division_classes():
    c = dm.division_cases()
    a, b = c.cols()
    assert all(v > 0 for v in c.counts().values()) and c.n <= 1 << 22
    assert dm.division_in_range(a, b).all()
    s = c.where["near_one"]
    k = (b[s] - 1.0) * 2.0 ** 52
    assert set(np.arange(-16, 17)) <= set(k.astype(int)) and np.all(np.abs(k) <= 16) and np.all(k == np.rint(k))
    s = c.where["plane_t"]
    assert np.abs(b[s]).min() == 0.001 and np.abs(b[s]).max() == 2.0 ** 128 and (b[s] < 0).any() and (b[s] > 0).any()
    s = c.where["mantissa_sweep"]
    mant, e = np.frexp(np.abs(b[s]))
    assert np.unique(mant).size == 1 << 20 and np.allclose(np.diff(np.sort(mant)), 2.0 ** -21, rtol=1e-9)
    assert set(e - 1) == set(range(-9, 129)) and np.abs(b[s]).min() >= 0.001
    s = c.where["zero_numerators"]
    assert np.all(a[s] == 0) and np.signbit(a[s]).any() and not np.signbit(a[s]).all()
    o = dm.division_out_of_range_cases()
    oa, ob = o.cols()
    assert all(v > 0 for v in o.counts().values())
    for name, s in o.where.items():
        if name != "specials":
            assert not dm.division_in_range(oa[s], ob[s]).any(), name
    s = o.where["exponent_difference"]
    assert np.all(np.abs(np.frexp(oa[s])[1] - np.frexp(ob[s])[1]) > 640) and (np.abs(np.frexp(oa[s])[1] - np.frexp(ob[s])[1]) > 768).any()
    s = o.where["denormal_numerators"]
    assert np.all(np.abs(oa[s]) < 2.0 ** -1022) and np.all(oa[s] != 0)
    assert np.isinf(oa).any() and np.isnan(ob).any() and (ob == 0).any()


def test_square_root_classes():
    c = dm.sqrt_cases()
    x, = c.cols()
    assert all(v > 0 for v in c.counts().values()) and dm.sqrt_in_range(x).all()
    z = x[c.where["zeros"]]
    assert np.all(z == 0) and np.signbit(z).any() and not np.signbit(z).all()
    # a square g² of a double g, scaled by an even power of two, has an exactly representable root that squares back to it
    r = np.sqrt(x[c.where["squares"]])
    assert np.all(r * r == x[c.where["squares"]])
    for name, steps in (("squares_1_step", 1), ("squares_2_steps", 2)):
        v = x[c.where[name]]
        r = np.sqrt(v)
        sq = r * r                                                           # within two ulps of a square, on either side
        d = np.rint((v - sq) / np.spacing(v))
        assert np.all(np.abs(d) <= steps + 1) and (d > 0).any() and (d < 0).any(), name
    # every fifth row from the third is the double nearest to a midpoint's square: neighbouring radicands have roots 0.35 to 0.71 ulp
    # apart (ulp(x) / 2r), so its root lies within 0.36 ulp of the midpoint (long double resolves 2^-11 ulp); the other rows
    # are one and two radicands further from their midpoints, on either side
    mid = x[c.where["near_midpoints"]]
    r = np.sqrt(mid.astype(np.longdouble)) / np.spacing(np.sqrt(mid)).astype(np.longdouble)
    frac = (r - np.floor(r))[2::5]
    assert np.all(np.abs(frac - 0.5) <= 0.36), float(np.abs(frac - 0.5).max())
    s = x[c.where["exponent_sweep"]]
    assert s.min() == dm.IN_RANGE_MIN and set(np.frexp(s)[1] - 1) >= set(range(-600, 300))
    assert np.isnan(x[c.where["nan"]]).all()
    o = dm.sqrt_out_of_range_cases()
    ox, = o.cols()
    assert all(v > 0 for v in o.counts().values()) and not dm.sqrt_in_range(ox).any()
    assert np.isinf(ox[o.where["infinity"]]).all() and np.all(ox[o.where["denormals"]] < 2.0 ** -1022)


def test_normalize_classes():
    c = dm.normalize_cases()
    x, y, z = c.cols()
    assert all(v > 0 and v % 64 == 0 for v in c.counts().values()) and c.n <= 1 << 22
    ok = dm.normalize_guard(x, y, z)
    waves = ok[: c.n - c.n % 64].reshape(-1, 64)
    for name in ("float32_differences", "magnitudes", "min_component_exact", "nn_exact_max", "inside_tail"):
        assert ok[c.where[name]].all(), name                                 # whole waves inside the guard: the seeded path runs
    assert waves.all(axis=1).sum() > 10000
    for name in ("min_component_below", "nn_above_max"):
        assert not ok[c.where[name]].any(), name
    s = c.where["float32_differences"]
    mags = np.frexp(np.abs(x[c.where["magnitudes"]]))[1]
    assert mags.min() <= -190 and mags.max() >= 189
    s = c.where["min_component_exact"]
    cmin = np.minimum(np.minimum(np.abs(x[s]), np.abs(y[s])), np.abs(z[s]))
    assert np.all(cmin == dm.NORMALIZE_MIN_COMPONENT)
    s = c.where["min_component_below"]
    cmin = np.minimum(np.minimum(np.abs(x[s]), np.abs(y[s])), np.abs(z[s]))
    assert np.all(cmin == np.nextafter(dm.NORMALIZE_MIN_COMPONENT, 0.0))
    with np.errstate(all="ignore"):
        nn = x * x + y * y + z * z
    assert np.all(nn[c.where["nn_exact_max"]] == dm.NORMALIZE_MAX_NN)
    assert np.all(nn[c.where["nn_above_max"]] == np.nextafter(dm.NORMALIZE_MAX_NN, np.inf))
    s = c.where["specials"]
    for pred in (np.isnan, np.isinf, lambda v: (v == 0) & np.signbit(v), lambda v: (v == 0) & ~np.signbit(v)):
        assert pred(x[s]).any() and pred(y[s]).any() and pred(z[s]).any()
    s = c.where["one_lane_outside"]
    assert np.all(ok[s].reshape(-1, 64).sum(axis=1) == 63)                   # exactly one lane fails the ballot
    assert set(np.argmin(ok[s].reshape(-1, 64), axis=1)) == set(range(64))


def test_renormalize_classes():
    c = dm.renormalize_cases()
    x, y, z = c.cols()
    assert all(v > 0 and v % 64 == 0 for v in c.counts().values())
    e = dm.unit_excess(x, y, z)
    W = dm.UNIT_WINDOW
    assert np.all(np.abs(e[c.where["unit"]]) < 2.0 ** -50)
    s = e[c.where["scaled"]]
    assert s.min() < -0.9 * W and s.max() > 0.9 * W and np.all(np.abs(s) < 1.01 * W)
    assert (np.abs(s) < W).sum() > 100000 and (np.abs(s) >= W).sum() > 0
    for name, want in (("window_exact_above", W), ("window_inside_above", W - 2.0 ** -52), ("window_outside_above", W + 2.0 ** -52),
                       ("window_exact_below", -W), ("window_inside_below", -W + 2.0 ** -53), ("window_outside_below", -W - 2.0 ** -53)):
        assert np.all(e[c.where[name]] == want), name
    s = c.where["one_nan_lane"]
    inside = (np.abs(e[s]) < W).reshape(-1, 64)
    assert np.all(inside.sum(axis=1) == 63) and np.all(np.isnan(e[s]).reshape(-1, 64).sum(axis=1) == 1)
    assert set(np.argmin(inside, axis=1)) == set(range(64))


def test_launch_shapes_keep_every_class():
    for c in (dm.division_cases(), dm.sqrt_cases(), dm.normalize_cases(), dm.renormalize_cases()):
        last = list(c.where)[-1]
        for shape in ("full", "tail"):
            n = dm.shape_rows(c.n, shape)
            assert n % 64 == (37 if shape == "tail" else 0) and c.where[last].start < n <= c.n


SCALE = 4        # 2^18 / 4 = 65 536 to 2^20 / 4 rows per bulk class: 10^5 per class and more in the sum of a function's classes


def test_host_mode_agrees_with_the_numpy_references(kat, tmp_path):
    """rt_math.h's seeded bodies on the host, with seeds up to 2^-24 off, against a / b, np.sqrt and the separately rounded normalize:
    the references the GPU test compares the device with are the kernel's arithmetic."""
    rng = np.random.default_rng(21)
    a, b = dm.division_cases(scale=SCALE).cols()
    got = _host(kat, tmp_path, "div_seeded", (a, b, dm._noisy(rng, 1.0 / b)))
    assert a.size >= 5 * 10 ** 5 and dm.bit_mismatches(got[0], dm.ref_div(a, b)).size == 0
    x, = dm.sqrt_cases(scale=SCALE).cols()
    with np.errstate(all="ignore"):
        got = _host(kat, tmp_path, "sqrt_seeded", (x, dm._noisy(rng, 1.0 / np.sqrt(x))))
    assert x.size >= 4 * 10 ** 5 and dm.bit_mismatches(got[0], dm.ref_sqrt(x)).size == 0
    vx, vy, vz = dm.normalize_cases(scale=SCALE).cols()
    want = dm.ref_normalize(vx, vy, vz)
    got = _host(kat, tmp_path, "normalize3_generic", (vx, vy, vz))
    assert all(dm.bit_mismatches(g, w).size == 0 for g, w in zip(got, want))
    ok = dm.normalize_guard(vx, vy, vz)
    with np.errstate(all="ignore"):
        nn = (vx * vx + vy * vy + vz * vz)[ok]
    got = _host(kat, tmp_path, "normalize3_seeded", (vx[ok], vy[ok], vz[ok], nn, dm._noisy(rng, 1.0 / np.sqrt(nn))))
    assert ok.sum() >= 10 ** 5 and all(dm.bit_mismatches(g, w[ok]).size == 0 for g, w in zip(got, want))
    dx, dy, dz = dm.renormalize_cases(scale=SCALE).cols()
    e = dm.unit_excess(dx, dy, dz)
    inw = np.abs(e) < dm.UNIT_WINDOW
    want = dm.ref_normalize(dx[inw], dy[inw], dz[inw])
    got = _host(kat, tmp_path, "renormalize_unit_fast", (dx[inw], dy[inw], dz[inw], e[inw]))
    assert inw.sum() >= 10 ** 5 and all(dm.bit_mismatches(g, w).size == 0 for g, w in zip(got[:3], want))
    c = dm.clip_operands(rng)
    got = _host(kat, tmp_path, "clip_color", (c,))
    assert np.array_equal(got[0], dm.ref_clip(c))


def test_order_bucket_restatement():
    c = np.concatenate([np.arange(0, 4096), 2 ** np.arange(5, 32) - 1, 2 ** np.arange(5, 32), [0xFFFFFFFF]]).astype(np.uint64)
    want = [int(v) if v < 32 else ((int(v).bit_length() - 1 - 4) << 5) | ((int(v) >> (int(v).bit_length() - 1 - 5)) & 31) for v in c]
    b = dm.order_bucket(c)
    assert np.array_equal(b, want) and b.max() < 1024 and np.all(np.diff(dm.order_bucket(np.sort(c))) >= 0)


ORDER_SMALL = [nb for nb in dm.ORDER_NBLOCKS if nb <= 16200]


@pytest.mark.parametrize("nblocks", ORDER_SMALL + [(1 << 20) - 1])
def test_order_checker_accepts_a_valid_order(nblocks):
    shapes = dm.order_shapes(nblocks) if nblocks <= 16200 else [(0, 0, nblocks), (4, 2, nblocks - 3)]
    for g, w, nv in shapes:
        for kind in dm.ORDER_COSTS:
            cost = dm.order_costs(kind, nv)
            order = dm.valid_order(nblocks, g, w, nv, cost)
            assert dm.order_violations(order, nblocks, g, w, nv, cost) == [], (nblocks, g, w, nv, kind)


def test_order_checker_rejects_planted_faults():
    nb, g, w = 1000, 2, 0
    cost = dm.order_costs("increasing", nb)
    good = dm.valid_order(nb, g, w, nb, cost)
    assert dm.order_violations(good, nb, g, w, nb, cost) == []
    dup = good.copy(); dup[5] = dup[6]
    assert any("permutation" in v for v in dm.order_violations(dup, nb, g, w, nb, cost))
    dup2 = good.copy(); dup2[nb + 5] = dup2[nb + 6]
    assert any("second half is no permutation" in v for v in dm.order_violations(dup2, nb, g, w, nb, cost))
    split = good.copy(); split[[0, 1]] = split[[1, 0]]                        # positions 0 and 1 are XCD 0's and XCD 1's first items
    assert any("split over two XCD classes" in v for v in dm.order_violations(split, nb, g, w, nb, cost))
    asc = good.copy()
    mine = np.arange(0, 8 * (nb >> g) // 8 * 4, 8)[: (nb >> g) // 8 * 4]     # XCD 0's positions in the rows region
    asc[mine] = asc[mine][::-1]
    assert any("increases along XCD 0" in v for v in dm.order_violations(asc, nb, g, w, nb, cost))
    seq = good.copy(); seq[nb + np.array([0, 8])] = seq[nb + np.array([8, 0])]
    assert any("tile order" in v for v in dm.order_violations(seq, nb, g, w, nb, cost))
    tail = good.copy(); tail[[8, nb - 1]] = tail[[nb - 1, 8]]
    assert dm.order_violations(tail, nb, g, w, nb, cost) != []


def test_raybox_families_and_checker():
    hit = dm.raybox_hitting_rays()
    assert hit[0].size > 200000 and dm.provably_enters(hit).all()
    R = np.array(hit[3:6])
    assert (R == 0).any(axis=0).sum() > 10000 and ((R == 0).sum(axis=0) == 2).sum() > 10000
    assert ((R != 0) & (np.abs(R) < 2.0 ** -40)).any(axis=0).sum() > 10000
    ext = np.sqrt(hit[6])
    o, lo, hi = np.array(hit[0:3]), np.array(hit[7:10]), np.array(hit[10:13])
    assert (np.all((o > lo) & (o < hi), axis=0)).sum() > 1000 and (np.any((o < lo) | (o > hi), axis=0)).sum() > 100000
    # the float32 restatement with a correctly rounded reciprocal certifies none of them ...
    ref = dm.raybox_reference(hit)
    assert dm.raybox_false_certificates(hit, ref).size == 0 and ref.sum() == 0
    # ... and the checker finds a planted certificate
    planted = ref.copy(); planted[[3, 77777]] = 1
    assert list(dm.raybox_false_certificates(hit, planted)) == [3, 77777]
    miss = dm.raybox_missing_rays()
    assert miss[0].size > 100000 and np.all(np.abs(np.array(miss[3:6])) >= 2.0 ** -4) and not dm.provably_enters(miss).any()
    assert dm.raybox_reference(miss).all()                                    # the family is certifiable: the reference certifies all of it
    # 1 ulp of error in the reciprocal, either way, is inside the test's budget
    for step in (np.inf, -np.inf):
        assert dm.raybox_reference(miss, rcp=lambda r: np.nextafter(np.float32(1.0) / r, np.float32(step))).all()
        assert dm.raybox_reference(hit, rcp=lambda r: np.nextafter(np.float32(1.0) / r, np.float32(step))).sum() == 0
    sp = dm.raybox_special_rays()
    ref = dm.raybox_reference(sp)
    assert ref[-1] == 1 and ref[:-1].sum() == 0 and ext.min() > 0
