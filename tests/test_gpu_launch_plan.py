"""The library launches what its plan says: cases of tests/golden/launch_plan.npz (the table test_algorithms.py walks through
python-ray-tracer_amd/csrc/rt_plan.h on the CPU), taken by their coordinates, rendered with MI355RT_LOG_KERNELS=1; every
render_kernel<...> line the library logs must name the fixture row's family and shape.  This ties the wiring (the KERNELS table's
indexing, the MI355RT_* knobs reaching the plan) to the table; what the kernels compute is the other GPU tests' business."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, raygen_closed_form
from feature_gpu import KERNEL_LINE
from test_algorithms import LAUNCH_PLAN_COORDS, LAUNCH_PLAN_ROW

pytestmark = pytest.mark.gpu

PLAIN, MAT, SCAT, SOFT = 0, 1, 3, 4                                      # rt::Family numbers
KNOB_ENV = ("MI355RT_CLUSTER_MINS", "MI355RT_LANES_MINS", "MI355RT_F32_RECORDS", "MI355RT_LANES_PARK", "MI355RT_WPW2_MAX_IMAGE",
            "MI355RT_ORDER_GROUP", "MI355RT_ORDER_TILES", "MI355RT_SEQ_ORDER")
# name: the case's coordinates in the table (knob row, S, P, L, family, AA, RT_FLAG_COUNT_RAYS, RT_FLAG_NO_BUNDLES), and what the
# case is there for: fields of the fixture's row
CASES = {
    "plain_s1":        ((0, 1, 2, 1, PLAIN, 0, 0, 0), dict(wpw=2, park=1, mode=0)),
    "plain_s64":       ((0, 64, 2, 3, PLAIN, 0, 0, 0), dict(wpw=4, mode=1)),        # (with three lights: one workgroup more per CU)
    "plain_s256":      ((0, 256, 2, 1, PLAIN, 0, 0, 0), dict(aa=0, mode=2)),
    "plain_s256_aa":   ((0, 256, 2, 1, PLAIN, 1, 0, 0), dict(aa=1, mode=3)),
    "plain_s36_flat":  ((5, 36, 2, 3, PLAIN, 0, 0, 0), dict(wpw=4, mode=0)),      # (MI355RT_CLUSTER_MINS=100000)
    "mat_s8":          ((0, 8, 2, 1, MAT, 0, 0, 0), dict(wpw=2)),
    "scat_s64":        ((0, 64, 2, 1, SCAT, 0, 0, 0), dict(wpw=4)),
    "soft_s256":       ((0, 256, 2, 1, SOFT, 0, 0, 0), dict(mode=2)),
    "plain_s8_count":  ((0, 8, 2, 1, PLAIN, 0, 1, 0), dict(count=1, wpw=4, park=0)),
}


def _scene(S, P, L, family):
    """Random spheres in front of the camera, P planes, L lights, and the arguments that make the scene one of `family`: a table
    of M = 4 rows of 3 columns (MAT), 6 with a rough row (SCAT), and a light radius > 0 (SOFT)."""
    rng = np.random.default_rng(1000 * S + family)
    spheres = np.empty((7, S), np.float32)
    spheres[0] = rng.uniform(4.0, 20.0, S)
    spheres[1:3] = rng.uniform(-5.0, 5.0, (2, S))
    spheres[3] = rng.uniform(0.3, 0.8, S)
    spheres[4:7] = rng.uniform(20.0, 250.0, (3, S))
    lights = np.array([[-2.0, 3.0, 6.0], [0.0, 5.0, -4.0], [3.0, 2.0, 8.0]], np.float32)[:, :L]
    planes = np.array([[0, 0], [0, 0], [-6, 6], [0, 0], [0, 0], [1, -1], [120, 60], [120, 60], [120, 200]], np.float32)[:, :P]
    kw = {}
    if family != PLAIN:
        table = np.tile(np.array([0.1, 0.6, 0.3, 0.0, 1.0, 0.0]), (4, 1))
        if family != MAT:
            table[2, 5] = 0.3
        kw["materials"] = (table if family != MAT else table[:, :3], np.arange(S) % 4, np.arange(P) % 4)
    if family == SOFT:
        kw.update(light_radius=np.full(L, 0.4, np.float32), shadow_samples=2)
    return spheres, lights, planes, kw


@pytest.mark.parametrize("name", list(CASES))
def test_launch_runs_the_planned_kernel(monkeypatch, capfd, name):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    fx = np.load(os.path.join(GOLDEN, "launch_plan.npz"))
    coords, expect = CASES[name]
    at = np.flatnonzero((fx["coords"] == np.array(coords, np.int32)).all(axis=1))
    assert at.size == 1, (name, coords)
    c, row = dict(zip(LAUNCH_PLAN_COORDS, coords)), dict(zip(LAUNCH_PLAN_ROW, (int(v) for v in fx["rows"][at[0]])))
    assert row["family"] == c["family"] and all(row[k] == v for k, v in expect.items()), (name, row)
    for key, value in zip(KNOB_ENV, fx["knobs"][c["knobs"]]):
        if value >= 0:                                                   # (-1: the order knobs' defaults)
            monkeypatch.setenv(key, str(int(value)))
        else:
            monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    monkeypatch.setenv("MI355RT_CHUNKS", "1")                            # one launch over the whole 32 x 24 frame: 12 tiles
    spheres, lights, planes, kw = _scene(c["S"], c["P"], c["L"], c["family"])
    w, h = 32, 24
    capfd.readouterr()
    with pkg.Renderer(0) as r:
        r.set_scene(spheres, lights, planes, **kw)
        r.set_camera(np.zeros(3), np.eye(3))
        r.set_raygen(w, h, *raygen_closed_form(w, h, 60.0))
        flags = (L.RT_FLAG_COUNT_RAYS if c["count"] else 0) | (L.RT_FLAG_NO_BUNDLES if c["no_bundles"] else 0) | \
                (L.RT_FLAG_AA_PER_PIXEL if c["aa"] == 1 else 0)          # (AA 1: a launch with an AA mode of its own, no lattice)
        u8, _ = r.render(0.1, 0.6, 0.4, 1, 1 if c["aa"] else 0, u8=True, flags=flags)
    names = [tuple(int(v) for v in n) for n in KERNEL_LINE.findall(capfd.readouterr().err)]
    want = tuple(row[k] for k in ("aa", "park", "wpw", "count", "lat", "mode", "family"))
    print(f"{name}: planned {want}, launched {names}")
    assert names and all(n == want for n in names), (name, want, names)
    assert u8.any()
