"""The render kernels' exact-arithmetic primitives on the device, one by one, against IEEE: tests/algo/device_math_kat.hip (a
stand-alone program that includes rt_device.h) runs as a child process on the operand classes of tests/device_math_cases.py, and the
results are compared with numpy float64 references as bit patterns.  What the frames' parity tests only touch on the operands their
scenes happen to produce is run here at the guards, at hard-to-round operands, on denormals and in waves where one lane fails a
ballot; the accuracy of the hardware's seed instructions, which the CPU checks of tests/algo assume, is measured; and
rt::order_kernel's own output is checked against the properties its comment promises.

MI355RT_DEVICE_MATH_OUT: a directory that receives device_math_seeds.json (profiles/ has the committed measurement) and
device_math_counts.json (operands per mode and class)."""
import json
import os
import subprocess

import numpy as np
import pytest

import device_math_cases as dm
from conftest import REPO

pytestmark = pytest.mark.gpu

CSRC = os.path.join(REPO, "python-ray-tracer_amd", "csrc")
BUILD = os.path.join(REPO, "tests", "algo", "build")
SOURCES = [os.path.join(REPO, "tests", "algo", "device_math_kat.hip")] + [
    os.path.join(CSRC, h) for h in ("rt_device.h", "rt_cull.h", "rt_facing.h", "rt_kparams.h", "rt_layout.h", "rt_math.h", "Makefile")]
TIME_LIMIT = 60          # seconds per invocation: each is milliseconds of GPU work on at most 2^22 operands


class Harness:
    def __init__(self, tmp):
        self.tmp, self.dead, self.counts = tmp, None, {}
        newest = max(os.path.getmtime(p) for p in SOURCES)
        exes = [os.path.join(BUILD, "device_math_kat"), os.path.join(BUILD, "device_math_kat_generic")]
        if not all(os.path.exists(e) and os.path.getmtime(e) >= newest for e in exes):
            subprocess.check_call(["make", "-C", CSRC, "-B", "kat"])
        self.fast, self.generic = exes

    def run(self, jobs, generic=False):
        """jobs: lists of harness arguments (one job each).  A harness that died of a signal, aborted, met a HIP error or ran into its
        time limit is not started again: every later test of the module fails here."""
        if self.dead:
            pytest.fail("the device harness is not started again after " + self.dead)
        args = [self.generic if generic else self.fast]
        for k, j in enumerate(jobs):
            args += (["--"] if k else []) + [str(a) for a in j]
        try:
            res = subprocess.run(args, capture_output=True, text=True, timeout=TIME_LIMIT)
        except subprocess.TimeoutExpired:
            self.dead = f"a time-out ({args[1:3]})"
            pytest.fail("device harness: " + self.dead)
        if res.returncode < 0 or res.returncode in (2, 134, 139):      # a signal, an abort, or the harness's own exit on a HIP error
            self.dead = f"exit status {res.returncode} ({args[1:3]}): {res.stderr[-400:]}"
            pytest.fail("device harness: " + self.dead)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout

    def dev(self, name, shape, cols, generic=False, tag=""):
        """Run one function on the device in one launch shape; returns its result words."""
        return self.dev_many([(name, shape, cols)], generic, tag)[0]

    def dev_many(self, runs, generic=False, tag=""):
        jobs, outs = [], []
        for k, (name, shape, cols) in enumerate(runs):
            src, dst = self.tmp / f"{name}{tag}{k}.in", self.tmp / f"{name}{tag}{k}.out"
            n = dm.write_operands(src, cols)
            jobs.append(["dev", name, shape, src, dst])
            outs.append((dst, name, n))
        self.run(jobs, generic)
        res = [dm.read_results(*o) for o in outs]
        for (src, _, _), j in zip(outs, jobs):
            os.remove(j[3]); os.remove(src)
        return res

    def count(self, mode, classes):
        self.counts.setdefault(mode, {}).update(classes)


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    h = Harness(tmp_path_factory.mktemp("device_math"))
    yield h
    out = os.environ.get("MI355RT_DEVICE_MATH_OUT")
    if out:
        with open(os.path.join(out, "device_math_counts.json"), "w") as f:
            json.dump(h.counts, f, indent=1)


def _trim(cols, n):
    return tuple(c[:n] for c in cols)


def _three_shapes(kat, name, cols, want, generic):
    """Function `name` on cols in the three launch shapes against the float64 columns `want`: zero bit mismatches on live lanes,
    the sentinel on the dead lanes of the divergent call."""
    n = cols[0].size
    nf, nt = dm.shape_rows(n, "full"), dm.shape_rows(n, "tail")
    full, tail, odd = kat.dev_many([(name, "full", _trim(cols, nf)), (name, "tail", _trim(cols, nt)), (name, "odd", _trim(cols, nf))], generic)
    for shape, got, rows in (("full", full, nf), ("tail", tail, nt)):
        for k, w in enumerate(want):
            bad = dm.bit_mismatches(got[k], w[:rows])
            assert bad.size == 0, (name, shape, k, bad.size, [(c[bad[0]].hex() if np.isfinite(c[bad[0]]) else c[bad[0]]) for c in cols],
                                   dm.as_f64(got[k])[bad[0]].hex(), w[bad[0]])
    lanes = np.arange(nf) % 64
    for k, w in enumerate(want):
        assert np.all(odd[k][lanes % 2 == 0] == dm.SENTINEL), (name, "a dead lane's result was written")
        live = np.flatnonzero(lanes % 2 == 1)
        bad = dm.bit_mismatches(odd[k][live], w[:nf][live])
        assert bad.size == 0, (name, "odd", k, bad.size, [c[live[bad[0]]] for c in cols])
    return nf + nt + nf // 2


# ---- the seeds -------------------------------------------------------------------------------------------------------------------
def test_seed_instructions_are_as_accurate_as_the_cpu_checks_assume(kat, tmp_path):
    """v_rcp_f64 and v_rsq_f64 on every in-range denominator, radicand and |v|²: relative error at most 2^-24 against long double,
    the level of the stand-in seeds of tests/algo/{normalize,renorm,divsqrt,cull_direction}_check.cpp.  v_rcp_f32 on what
    raybox_axis feeds it: at most 1 ulp, raybox_axis's budget.  The maxima and the operands that attain them go to
    device_math_seeds.json."""
    b, x, f = dm.seed_operands()
    b, x, f = b[: dm.shape_rows(b.size, "full")], x[: dm.shape_rows(x.size, "full")], f[: dm.shape_rows(f.size, "full")]
    rcp, rsq, rcpf = kat.dev_many([("seed_rcp", "full", (b,)), ("seed_rsq", "full", (x,)), ("seed_rcpf", "full", (f,))])
    rcp, rsq, rcpf = dm.as_f64(rcp[0]), dm.as_f64(rsq[0]), dm.as_f32(rcpf[0])
    e_rcp, k_rcp = dm.seed_error(rcp, b.astype(np.longdouble))
    e_rsq, k_rsq = dm.seed_error(rsq, np.sqrt(x.astype(np.longdouble)))
    ulps = dm.rcpf_ulps(f.astype(np.float32), rcpf)
    k_f = int(np.argmax(ulps))
    report = {"rcp_f64": {"operands": int(b.size), "max_relative_error": e_rcp, "log2": float(np.log2(e_rcp)), "at": float(b[k_rcp]).hex()},
              "rsq_f64": {"operands": int(x.size), "max_relative_error": e_rsq, "log2": float(np.log2(e_rsq)), "at": float(x[k_rsq]).hex()},
              "rcp_f32": {"operands": int(f.size), "max_ulps": float(ulps[k_f]), "at": float(f[k_f]).hex()}}
    print(json.dumps(report))
    for d in (str(tmp_path), os.environ.get("MI355RT_DEVICE_MATH_OUT")):
        if d:
            with open(os.path.join(d, "device_math_seeds.json"), "w") as fh:
                json.dump(report, fh, indent=1)
    kat.count("seeds", {"rcp_f64": int(b.size), "rsq_f64": int(x.size), "rcp_f32": int(f.size)})
    assert np.isfinite(rcp).all() and np.isfinite(rsq).all() and np.isfinite(rcpf).all()
    assert e_rcp <= 2.0 ** -24, report
    assert e_rsq <= 2.0 ** -24, report
    assert ulps[k_f] <= 1.0, report


# ---- the four wrappers, fast and generic builds -------------------------------------------------------------------------------------
BUILDS = [pytest.param(False, id="fast"), pytest.param(True, id="generic")]


@pytest.mark.parametrize("generic", BUILDS)
def test_div_inrange(kat, generic):
    c = dm.division_cases()
    a, b = c.cols()
    rows = _three_shapes(kat, "div_inrange", (a, b), (dm.ref_div(a, b),), generic)
    o = dm.division_out_of_range_cases()
    oa, ob = o.cols()
    oa, ob = np.resize(oa, dm.shape_rows(oa.size, "full") + 64), np.resize(ob, dm.shape_rows(ob.size, "full") + 64)
    got = kat.dev("div_inrange", "full", (oa, ob), generic, "oor")
    want = dm.ref_div(oa, ob)
    if generic:
        assert dm.bit_mismatches(got[0], want).size == 0                      # the backend's division is IEEE everywhere
    t = dm.as_f64(got[0])
    bad = np.flatnonzero(dm.hit_of_t(t) != dm.hit_of_t(want))
    assert bad.size == 0, (oa[bad[:5]], ob[bad[:5]], t[bad[:5]], want[bad[:5]])
    kat.count("div_inrange" + ("_generic" if generic else ""), {"rows_run": rows + oa.size, **c.counts(), **{"out_of_range_" + k: v for k, v in o.counts().items()}})


@pytest.mark.parametrize("generic", BUILDS)
def test_sqrt_inrange(kat, generic):
    c = dm.sqrt_cases()
    x, = c.cols()
    rows = _three_shapes(kat, "sqrt_inrange", (x,), (dm.ref_sqrt(x),), generic)
    o = dm.sqrt_out_of_range_cases()
    ox, = o.cols()
    ox = np.resize(ox, dm.shape_rows(ox.size, "full") + 64)
    got = kat.dev("sqrt_inrange", "full", (ox,), generic, "oor")
    want = dm.ref_sqrt(ox)
    if generic:
        assert dm.bit_mismatches(got[0], want).size == 0
    q = dm.as_f64(got[0])
    for s in dm.ROOT_S:
        bad = np.flatnonzero(dm.hit_of_root(q, s) != dm.hit_of_root(want, s))
        assert bad.size == 0, (s, ox[bad[:5]], q[bad[:5]], want[bad[:5]])
    kat.count("sqrt_inrange" + ("_generic" if generic else ""), {"rows_run": rows + ox.size, **c.counts(), **{"out_of_range_" + k: v for k, v in o.counts().items()}})


@pytest.mark.parametrize("generic", BUILDS)
def test_normalize3(kat, generic):
    """Bit equality on every class: outside the guard the wrapper takes the generic path for the whole wave, which is IEEE."""
    c = dm.normalize_cases()
    v = c.cols()
    want = dm.ref_normalize(*v)
    rows = _three_shapes(kat, "normalize3", v, want, generic)
    if generic:                                                               # the backend's own sqrt and divisions, called directly
        n = dm.shape_rows(v[0].size, "full")
        got = kat.dev("normalize3_generic", "full", _trim(v, n), generic)
        assert all(dm.bit_mismatches(g, w[:n]).size == 0 for g, w in zip(got[:3], want))
        rows += n
    kat.count("normalize3" + ("_generic" if generic else ""), {"rows_run": rows, **c.counts()})


@pytest.mark.parametrize("generic", BUILDS)
def test_renormalize_unit(kat, generic):
    c = dm.renormalize_cases()
    v = c.cols()
    rows = _three_shapes(kat, "renormalize_unit", v, dm.ref_normalize(*v), generic)
    kat.count("renormalize_unit" + ("_generic" if generic else ""), {"rows_run": rows, **c.counts()})


# ---- host against device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dm.HOST_FUNCTIONS)
def test_hip_free_functions_agree_between_host_and_device(kat, name):
    """Every RT_MATH_FN function of rt_math.h, rt_cull.h and rt_facing.h, evaluated on the device and on the host by the same
    binary and compared bit for bit inside it, on 2^20 rows of operands."""
    cols = dm.hostdev_operands(name)
    src, dst = kat.tmp / (name + ".hd.in"), kat.tmp / (name + ".hd.out")
    n = dm.write_operands(src, cols)
    out = kat.run([["hostdev", name, src, dst]])
    assert n >= 10 ** 6 and f"hostdev {name} evals={n} mismatches=0" in out, out
    got = dm.read_results(dst, name, n)
    os.remove(src); os.remove(dst)
    if name == "clip_color":
        assert np.array_equal(got[0], dm.ref_clip(cols[0]))
    if name == "normalize3_generic":                                          # the device's lowering of sqrt and / is IEEE
        assert all(dm.bit_mismatches(g, w).size == 0 for g, w in zip(got[:3], dm.ref_normalize(*cols)))
    kat.count("hostdev", {name: n})


# ---- the cluster box test -----------------------------------------------------------------------------------------------------------
def test_raybox_certifies_no_ray_that_enters_the_box(kat):
    hit = dm.raybox_hitting_rays()
    n = dm.shape_rows(hit[0].size, "full")
    hit = _trim(hit, n)
    sp = dm.raybox_special_rays()
    sp = tuple(np.resize(c, 64) for c in sp)
    got, gsp = kat.dev_many([("raybox", "full", hit), ("raybox", "full", sp)])
    assert set(np.unique(got[0])) <= {0, 1}
    bad = dm.raybox_false_certificates(hit, got[0])
    assert bad.size == 0, [c[bad[0]] for c in hit]
    nsp = dm.raybox_special_rays()[0].size
    assert np.all(gsp[0][: nsp - 1] == 0) and gsp[0][nsp - 1] == 1           # NaN / inf never certify; the finite ray they spoil does
    assert np.all(gsp[2][: nsp - 1] == 0)
    kat.count("raybox", {"hitting": n, "specials": nsp})


def test_raybox_certifies_the_rays_that_miss_by_a_margin(kat):
    miss = dm.raybox_missing_rays()
    assert dm.raybox_reference(miss).all()                                    # (tests/test_device_math_cases.py has the argument)
    n = dm.shape_rows(miss[0].size, "full")
    miss = _trim(miss, n)
    got = kat.dev("raybox", "full", miss)
    bad = np.flatnonzero(got[0] != 1)
    assert bad.size == 0, (bad.size, [c[bad[0]] for c in miss])
    kat.count("raybox", {"missing": n})


# ---- the dispatch order -------------------------------------------------------------------------------------------------------------
def _order_cases(nblocks):
    if nblocks <= 16200:
        return [(nblocks, g, w, nv, dm.order_costs(kind, nv)) for g, w, nv in dm.order_shapes(nblocks) for kind in dm.ORDER_COSTS]
    # 2^20 - 1 items (8 MB of order each): equal costs, which put every rank into one bucket and run the 20-bit group counter
    # (gshift 0) and the per-XCD item counters to their ends, at both ends of the shape range and with the tile items' short last
    # workgroup; the other costs at the two shapes that differ most
    shapes = [(0, 0, nblocks), (1, 0, nblocks), (6, 0, nblocks), (2, 2, nblocks), (2, 2, nblocks - 3), (6, 2, nblocks - 3)]
    cases = [(nblocks, g, w, nv, dm.order_costs("equal", nv)) for g, w, nv in shapes]
    return cases + [(nblocks, g, w, nv, dm.order_costs(kind, nv)) for g, w, nv in ((0, 0, nblocks), (4, 2, nblocks - 3)) for kind in dm.ORDER_COSTS[1:]]


@pytest.mark.parametrize("nblocks", dm.ORDER_NBLOCKS)
def test_order_kernel_output_has_the_promised_properties(kat, nblocks):
    cases = _order_cases(nblocks)
    src, dst = kat.tmp / f"order{nblocks}.in", kat.tmp / f"order{nblocks}.out"
    dm.write_order_cases(src, cases)
    out = kat.run([["order", src, dst]])
    assert f"order cases={len(cases)}" in out
    orders = dm.read_order_results(dst, cases)
    os.remove(src); os.remove(dst)
    for (nb, g, w, nv, cost), order in zip(cases, orders):
        assert dm.order_violations(order, nb, g, w, nv, cost) == [], (nb, g, w, nv)
    kat.count("order", {str(nblocks): len(cases)})
