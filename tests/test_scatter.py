"""Rough materials (scatter) without a GPU: the C-ABI entry point, Material / Scene.generate_materials with roughness, the
scatter fixtures (tests/golden/scatter_*.npz, tools/gen_scatter_golden.py) and the generator's pure hash and ball step."""
import glob
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO

CASES = {"default_64_d4", "grazing_48_d3", "inside_32_d4", "aa_48_d2", "stoch_40x24_spp3_seed7", "c4_s64_d5_sub32",
         "c5_s256_d8_sub96"}


def scatter_cases():
    return sorted(os.path.basename(p)[len("scatter_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "scatter_*.npz")))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_scatter_golden", os.path.join(REPO, "tools", "gen_scatter_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_ctypes_and_library_declare_the_entry_point():
    from python_ray_tracer_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    assert re.search(r"int rt_set_scene_materials_scatter\(", hdr)
    assert "0x5CA77E12" in hdr
    assert "rt_set_scene_materials_scatter" in L.PROTOTYPES
    src = open(os.path.join(REPO, "python-ray-tracer_amd", "csrc", "mi355rt.hip")).read()
    assert re.search(r"^int rt_set_scene_materials_scatter\(", src, re.M)


def test_hash_restatement_fixed_values():
    gen = _generator()
    assert gen.hash32(0, 0, 0, 0) == 0x77F37AEA
    assert gen.hash32(2, 4, 0, 7) == 0x7662FE93
    assert gen.hash32(7679, 4319, 511, 0xFFFFFFFF) == 0x45155F2B
    assert gen.hash32(96, 48, (2 * 16 + 15) * 32 + 31, 22 ^ 0x5CA77E12) == 0xD5BD22FC


def test_candidates_are_exact_and_in_range():
    """q_c = (h >> 8) 2^-23 + 2^-24 - 1 is a multiple of 2^-24 in (-1, 1); q.q is exact (48-bit squares, a 50-bit sum)."""
    from fractions import Fraction
    gen = _generator()
    inside = 0
    for X, Y, s, b in ((0, 0, 0, 0), (129, 64, 2, 3), (7679, 4319, 63, 15)):
        for j in range(8):
            q = gen.candidate(X, Y, s, b, j, 7)
            for c in q:
                assert -1.0 < c < 1.0 and (c * 2 ** 24).is_integer()
            exact = sum(Fraction(c) * Fraction(c) for c in q)
            assert Fraction((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) == exact
            inside += exact < 1
    assert 0 < inside < 24
    q = gen.ball_point(129, 64, 2, 3, 7)
    assert q is not None and (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2] < 1.0


def test_hash_key_bits_are_disjoint():
    """((s*16 + b)*8 + j)*4 + c == s << 9 | b << 5 | j << 2 | c for b <= 15: the kernel folds s into its pre-hashed key."""
    for s in (0, 1, 5, 63):
        for b in range(16):
            for j in range(8):
                for c in range(3):
                    assert ((s * 16 + b) * 8 + j) * 4 + c == (s << 9) | (b << 5) | (j << 2) | c


def test_material_roughness_rules():
    from python_ray_tracer_amd.scene import Material
    m = Material(0.0, 0.3, 0.8, roughness=0.25)
    assert m.rough and m.key6() == (0.0, 0.3, 0.8, 0.0, 1.0, 0.25)
    assert not Material(0.0, 0.3, 0.8).rough
    Material(0.0, 0.3, 0.8, roughness=1.0)
    for bad in (-0.1, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Material(0.0, 0.3, 0.8, roughness=bad)
    with pytest.raises(ValueError):
        Material(0.0, 0.0, 0.0, transparency=0.9, ior=1.5, roughness=0.1)
    Material(0.0, 0.0, 0.0, transparency=0.9, ior=1.5, roughness=0.0)


def test_generate_materials_widths():
    from python_ray_tracer_amd.scene import Material, Scene
    s = Scene.default_scene()
    default = Material(0.05, 0.8, 0.0)
    t, sid, pid = s.generate_materials(default)
    assert t.shape[1] == 3
    s.spheres[0].material = Material(0.0, 0.0, 0.0, transparency=0.9, ior=1.5)
    assert s.generate_materials(default)[0].shape[1] == 5
    s.spheres[1].material = Material(0.0, 0.4, 0.8, roughness=0.3)
    s.planes[0].material = Material(0.0, 0.3, 0.7, roughness=0.3)
    t, sid, pid = s.generate_materials(default)
    assert t.shape[1] == 6 and t.dtype == np.float64
    assert tuple(t[sid[1]]) == (0.0, 0.4, 0.8, 0.0, 1.0, 0.3)
    assert tuple(t[sid[0]]) == (0.0, 0.0, 0.0, 0.9, 1.5, 0.0)
    assert tuple(t[pid[0]]) == (0.0, 0.3, 0.7, 0.0, 1.0, 0.3)
    assert tuple(t[sid[2]]) == (0.05, 0.8, 0.0, 0.0, 1.0, 0.0)
    assert len({tuple(r) for r in t}) == t.shape[0]


def test_fixture_set_and_invariants():
    cases = set(scatter_cases())
    assert cases >= CASES
    absorbed = fallback = 0
    for case in cases:
        g = np.load(os.path.join(GOLDEN, f"scatter_{case}.npz"))
        t = g["materials"]
        assert t.ndim == 2 and t.shape[1] == 6 and t.dtype == np.float64
        assert np.isfinite(t).all() and (t[:, 5] >= 0).all() and (t[:, 5] <= 1).all()
        assert not ((t[:, 3] > 0) & (t[:, 5] > 0)).any()
        assert (t[:, 5] > 0).any()
        assert int(g["sphere_material"].max()) < t.shape[0] and int(g["plane_material"].max()) < t.shape[0]
        assert g["u8"].shape == (len(g["coords"]), 3) and g["rgb64"].shape == (len(g["coords"]), 3)
        assert int(g["n_scatter"]) > 0, case
        assert 0 <= int(g["seed"]) <= 0xFFFFFFFF
        absorbed += int(g["n_absorbed"])
        fallback += int(g["n_fallback"])
    assert absorbed > 0 and fallback > 0
    g = np.load(os.path.join(GOLDEN, "scatter_grazing_48_d3.npz"))
    assert int(g["n_absorbed"]) > 0 and int(g["n_fallback"]) > 0 and (g["materials"][:, 5] == 1.0).any()
    g = np.load(os.path.join(GOLDEN, "scatter_default_64_d4.npz"))
    t = g["materials"]
    assert ((t[:, 5] == 0) & (t[:, 3] == 0)).any() and (t[:, 3] > 0).any()


def test_renderer_routes_six_columns_to_the_scatter_symbol():
    src = open(os.path.join(REPO, "python-ray-tracer_amd", "renderer.py")).read()
    assert "rt_set_scene_materials_scatter" in src
