"""Transparent materials (refraction) without a GPU: the C-ABI entry point, Material / Scene.generate_materials with the new
fields, the refraction fixtures (tests/golden/refraction_*.npz, tools/gen_refraction_golden.py) and the generator's pure
Snell step."""
import glob
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO

CASES = {"default_64_d4", "tir_48_d6", "window_48_d3", "inside_32_d4", "overlap_48_d5", "aa_48_d2", "stoch_40x24_spp3_seed7",
         "c4_s64_d5_sub32", "c5_s256_d8_sub96"}


def refraction_cases():
    return sorted(os.path.basename(p)[len("refraction_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "refraction_*.npz")))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_refraction_golden", os.path.join(REPO, "tools", "gen_refraction_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_ctypes_and_library_declare_the_entry_point():
    from python_ray_tracer_amd import _lib
    src = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    assert re.search(r"int\s+rt_set_scene_materials_ex\s*\(", src)
    assert "rt_set_scene_materials_ex" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["rt_set_scene_materials_ex"]
    assert len(args) == 13
    assert _lib.RT_ABI_VERSION == 7
    lib = _lib.load()
    assert hasattr(lib, "rt_set_scene_materials_ex")


def test_material_fields_and_validation():
    from python_ray_tracer_amd.scene import Material
    m = Material(0.1, 0.6, 0.3)
    assert m.transparency == 0.0 and m.ior == 1.0 and not m.transparent
    g = Material(0.0, 0.0, 0.0, transparency=0.9, ior=1.5)
    assert g.transparent and g.key5() == (0.0, 0.0, 0.0, 0.9, 1.5)
    for kw in (dict(transparency=-0.1), dict(transparency=float("nan")), dict(ior=0.0), dict(ior=-1.5), dict(ior=float("inf"))):
        with pytest.raises(ValueError):
            Material(0.0, 0.5, 0.0, **kw)
    with pytest.raises(ValueError):                               # one continuation: reflection or transmission, not both
        Material(0.0, 0.5, 0.2, transparency=0.5, ior=1.5)


def test_generate_materials_opaque_is_unchanged_and_glass_widens():
    from python_ray_tracer_amd.scene import Scene, Sphere, Plane, Light, Material
    mirror, matte = Material(0.0, 0.2, 0.9), Material(0.1, 0.7, 0.0)
    spheres = [Sphere([0, 0, 1], 1.0, [255, 0, 0], material=matte), Sphere([2, 0, 1], 0.5, [0, 255, 0]),
               Sphere([4, 0, 1], 0.5, [0, 0, 255], material=Material(0.1, 0.7, 0.0, transparency=0.0, ior=1.7))]
    planes = [Plane([0, 0, 0], [0, 0, 1], [125, 125, 125], material=mirror)]
    s = Scene([Light([1, 2, 3])], spheres, planes)
    table, sid, pid = s.generate_materials(Material(0.0, 0.6, 0.3))
    # all opaque: the 3-column table of before (an ior of an opaque material changes nothing and is not a column)
    assert table.shape == (3, 3) and table.tolist() == [[0.1, 0.7, 0.0], [0.0, 0.6, 0.3], [0.0, 0.2, 0.9]]
    assert sid.tolist() == [0, 1, 0] and pid.tolist() == [2]
    glass, diamond = Material(0.0, 0.0, 0.0, 0.9, 1.5), Material(0.0, 0.0, 0.0, 0.9, 2.4)
    spheres[1].material = glass
    spheres.append(Sphere([6, 0, 1], 0.5, [9, 9, 9], material=diamond))
    spheres.append(Sphere([8, 0, 1], 0.5, [9, 9, 9], material=Material(0.0, 0.0, 0.0, 0.9, 1.5)))
    table, sid, pid = Scene([Light([1, 2, 3])], spheres, planes).generate_materials(Material(0.0, 0.6, 0.3))
    assert table.dtype == np.float64 and table.shape == (5, 5)
    # dedup keys include transparency and ior: the ior-1.7 opaque row is its own row now, equal glass rows share one
    assert table.tolist() == [[0.1, 0.7, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.9, 1.5], [0.1, 0.7, 0.0, 0.0, 1.7],
                              [0.0, 0.0, 0.0, 0.9, 2.4], [0.0, 0.2, 0.9, 0.0, 1.0]]
    assert sid.tolist() == [0, 1, 2, 3, 1] and pid.tolist() == [4]


def test_refraction_fixtures_are_complete():
    cases = refraction_cases()
    assert CASES <= set(cases)
    for c in cases:
        path = os.path.join(GOLDEN, f"refraction_{c}.npz")
        assert os.path.getsize(path) < 1 << 20, c
        g = np.load(path)
        M = g["materials"].shape[0]
        t = g["materials"]
        assert t.shape == (M, 5) and t.dtype == np.float64 and np.isfinite(t).all(), c
        assert (t[:, 3] >= 0).all() and (t[:, 4] > 0).all() and (t[t[:, 3] > 0, 2] == 0).all(), c
        assert (t[:, 3] > 0).any(), c
        assert g["sphere_material"].shape == (g["spheres"].shape[1],) and g["plane_material"].shape == (g["planes"].shape[1],)
        for ids in (g["sphere_material"], g["plane_material"]):
            assert ids.dtype == np.int32 and ((ids >= 0) & (ids < M)).all()
        assert g["rgb64"].shape == g["u8"].shape == (len(g["coords"]), 3)
        assert g["rgb64"].dtype == np.float64 and g["u8"].dtype == np.uint8 and np.isfinite(g["rgb64"]).all()
        for k in ("n_refract", "n_tir", "n_pass"):
            assert 0 <= int(g[k]) <= len(g["coords"]), (c, k)
        if int(g["aa"]) == 2:
            assert int(g["spp"]) > 0


def test_refraction_fixtures_cover_the_events():
    for c in refraction_cases():
        g = np.load(os.path.join(GOLDEN, f"refraction_{c}.npz"))
        assert int(g["n_refract"]) > 0, c
    assert int(np.load(os.path.join(GOLDEN, "refraction_tir_48_d6.npz"))["n_tir"]) > 0
    assert int(np.load(os.path.join(GOLDEN, "refraction_window_48_d3.npz"))["n_pass"]) > 0
    g = np.load(os.path.join(GOLDEN, "refraction_inside_32_d4.npz"))
    o, sp = g["cam_origin"], g["spheres"]
    inside = ((sp[0:3] - o[:, None]) ** 2).sum(axis=0) < sp[3].astype(np.float64) ** 2
    assert (inside & (g["materials"][g["sphere_material"], 3] > 0)).any(), "the camera is inside a glass sphere"


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return tuple(float(x) for x in v / np.linalg.norm(v))


def test_refract_obeys_snells_law():
    gen = _generator()
    rng = np.random.default_rng(11)
    n_tir = n_ref = 0
    for _ in range(4000):
        d, N = _unit(rng.normal(size=3)), _unit(rng.normal(size=3))
        ior = float(rng.choice([rng.uniform(0.4, 3.0), 1.5, 2.4, 1.0]))
        T, n, enter = gen.refract(d, N, ior)
        c = float(np.dot(d, N))
        assert enter == (c < 0)
        assert n == (N if enter else (-N[0], -N[1], -N[2]))
        eta = 1.0 / ior if enter else ior
        sin_i = math.sqrt(max(0.0, 1.0 - c * c))
        if T is None:
            n_tir += 1
            assert eta * sin_i > 1.0 - 1e-12                          # TIR exactly where eta sin(theta_i) > 1
            continue
        n_ref += 1
        assert eta * sin_i <= 1.0 + 1e-12
        T = np.array(T)
        assert abs(np.linalg.norm(T) - 1.0) < 1e-14
        cos_t = float(np.dot(T, -np.array(n)))                         # the refracted ray continues on the far side
        assert cos_t >= -1e-12
        sin_t = math.sqrt(max(0.0, 1.0 - cos_t * cos_t))
        assert abs(eta * sin_i - sin_t) < 1e-12
        assert abs(float(np.dot(T, np.cross(d, N)))) < 1e-12           # coplanar with d and N
    assert n_tir > 100 and n_ref > 1000
    # ior 1 leaves the direction unchanged (up to rounding), and a normal incidence is not bent
    T, _, _ = gen.refract(_unit([1, 2, -3]), _unit([0, 0, 1]), 1.0)
    assert np.allclose(T, _unit([1, 2, -3]), atol=1e-15)
    T, _, _ = gen.refract((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 1.5)
    assert T == (0.0, 0.0, -1.0)


def test_refract_critical_angle():
    gen = _generator()
    ior = 1.5
    crit = math.asin(1.0 / ior)
    N = (0.0, 0.0, 1.0)
    for ang, tir in ((crit - 1e-6, False), (crit + 1e-6, True)):
        d = (math.sin(ang), 0.0, math.cos(ang))                       # leaving the glass (d.N > 0)
        T, n, enter = gen.refract(d, N, ior)
        assert not enter and (T is None) == tir
