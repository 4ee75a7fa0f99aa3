"""Area lights (soft shadows) without a GPU: the C-ABI entry point, Light(radius=) and Renderer.set_scene's checks, the
soft_* fixtures (tests/golden/soft_*.npz, tools/gen_soft_shadow_golden.py) and the generator's pure light sampler."""
import glob
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

CASES = {"default_64_d4", "aa_48_d2", "stoch_40x24_spp3_seed7", "mixed_32_n16_d2", "glass_rough_48_d4", "rim_48_d2",
         "c4_s64_d5_sub32", "c5_s256_d8_sub96"}


def soft_cases():
    return sorted(os.path.basename(p)[len("soft_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "soft_*.npz")))


def _generator():
    tools = os.path.join(REPO, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    spec = importlib.util.spec_from_file_location("gen_soft_shadow_golden", os.path.join(tools, "gen_soft_shadow_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _jitter_hash(x, y, s, seed):
    """rt_device.h jitter_hash, restated on Python integers."""
    M = 0xFFFFFFFF
    h = (seed ^ 0x9E3779B9) & M
    h = ((h ^ x) * 0x85EBCA6B) & M; h ^= h >> 13
    h = ((h ^ y) * 0xC2B2AE35) & M; h ^= h >> 16
    h = ((h ^ s) * 0x27D4EB2F) & M; h ^= h >> 15
    h = (h * 0x165667B1) & M; h ^= h >> 13
    return h


def test_header_ctypes_and_library_declare_the_entry_point():
    from python_ray_tracer_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    assert re.search(r"int rt_set_scene_area_lights\(", hdr)
    assert re.search(r"#define RT_MAX_SHADOW_SAMPLES 16\b", hdr)
    assert "0x50F7117E" in hdr and "0x50F7117E" != "0x5CA77E12"
    assert "rt_set_scene_area_lights" in L.PROTOTYPES and L.RT_MAX_SHADOW_SAMPLES == 16
    src = open(os.path.join(REPO, "python-ray-tracer_amd", "csrc", "mi355rt.hip")).read()
    assert re.search(r"^int rt_set_scene_area_lights\(", src, re.M)
    dev = open(os.path.join(REPO, "python-ray-tracer_amd", "csrc", "rt_math.h")).read()
    assert "0x50F7117Eu" in dev


def test_hash_layout_is_the_bit_pattern():
    """t = ((((s*32 + b)*64 + m)*16 + i)*8 + j)*4 + c is s << 20 | b << 15 | m << 9 | i << 5 | j << 2 | c: injective, < 2^26."""
    for s, b, m, i, j, c in ((0, 0, 0, 0, 0, 0), (63, 16, 63, 15, 7, 3), (5, 3, 2, 9, 1, 2), (1, 16, 0, 0, 7, 0)):
        t = ((((s * 32 + b) * 64 + m) * 16 + i) * 8 + j) * 4 + c
        assert t == (s << 20) | (b << 15) | (m << 9) | (i << 5) | (j << 2) | c and t < 2 ** 26


def test_light_candidates_restate_the_device_hash():
    gen = _generator()
    assert gen.SOFT_SALT == 0x50F7117E
    for X, Y, s, b, m, i, j, seed in ((0, 0, 0, 0, 0, 0, 0, 0), (129, 64, 2, 3, 1, 5, 4, 7), (7679, 4319, 63, 16, 63, 15, 7, 0xFFFFFFFF)):
        q = gen.light_candidate(X, Y, s, b, m, i, j, seed)
        t = (s << 20) | (b << 15) | (m << 9) | (i << 5) | (j << 2)
        for c in range(3):
            h = _jitter_hash(X, Y, t | c, seed ^ 0x50F7117E)
            assert q[c] == (h >> 8) * 2.0 ** -23 + (2.0 ** -24 - 1.0)
            assert -1.0 < q[c] < 1.0 and (q[c] * 2 ** 24).is_integer()


def test_light_point_hand_cases():
    gen = _generator()
    c = (2.5, -2.0, 3.0)
    assert gen.light_point(4, 6, 0, 0, 0, 0, 1, c, 0.0) == c                     # radius 0: the centre (c + 0*q)
    inside = 0
    for X in range(0, 40, 3):
        for i in range(4):
            Q = gen.light_point(X, 7, 1, 2, 1, i, 9, c, 0.5)
            d = np.array(Q) - np.array(c)
            assert np.dot(d, d) < 0.25 * (1 + 1e-12)
            inside += 1
            # the first candidate inside the ball, and c + rho*q with the products rounded separately
            for j in range(8):
                q = gen.light_candidate(X, 7, 1, 2, 1, i, j, 9)
                if (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2] < 1.0:
                    assert Q == tuple(c[k] + 0.5 * q[k] for k in range(3))
                    break
            else:
                assert Q == c
    assert inside == 56
    # different sample indices, traces, lights and shadow samples give different points
    pts = {gen.light_point(10, 12, s, b, m, i, 3, c, 0.5) for s in (0, 1) for b in (0, 1) for m in (0, 1) for i in (0, 1)}
    assert len(pts) == 16


def test_soft_lights_order_is_light_major():
    gen = _generator()
    lights = np.array([[0.0, 5.0], [1.0, 6.0], [2.0, 7.0]], dtype=np.float32)
    Qs = gen.soft_lights(lights, np.array([0.3, 0.0]), 3, (8, 10, 0, 5), 2)
    assert Qs.shape == (3, 6) and Qs.dtype == np.float64
    for m in range(2):
        for i in range(3):
            assert tuple(Qs[:, m * 3 + i]) == gen.light_point(8, 10, 0, 2, m, i, 5, tuple(float(v) for v in lights[:, m]),
                                                              (0.3, 0.0)[m])
    assert (Qs[:, 3:] == lights[:, 1:2].astype(np.float64)).all()


def test_light_validation():
    from python_ray_tracer_amd.scene.scene import Light, Scene
    assert Light([1, 2, 3]).radius == 0.0
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), 1e39):
        with pytest.raises(ValueError):
            Light([1, 2, 3], radius=bad)
    sc = Scene([Light([1, 2, 3], radius=0.5), Light([0, 0, 5])], [], [])
    r = sc.get_light_radii()
    assert r.dtype == np.float32 and r.tolist() == [0.5, 0.0]
    assert sc.get_lights().shape == (3, 2)


def test_set_scene_needs_a_table_for_area_lights():
    """Renderer.set_scene refuses a radius > 0 without a material table before it reaches the library."""
    from python_ray_tracer_amd import renderer as R
    r = R.Renderer.__new__(R.Renderer)                  # no device needed: the check comes first
    sp, li, pl = np.zeros((7, 1), np.float32), np.zeros((3, 2), np.float32), np.zeros((9, 0), np.float32)
    with pytest.raises(ValueError, match="material table"):
        r.set_scene(sp, li, pl, light_radius=[0.5, 0.0])
    with pytest.raises(ValueError, match="material table"):
        r.set_scene(sp, li, pl, light_radius=[float("nan"), 0.0])
    with pytest.raises(ValueError, match="radii"):
        r.set_scene(sp, li, pl, materials=(np.ones((1, 3)), [0], []), light_radius=[0.5])


def test_fixtures_present_and_have_penumbrae():
    assert set(soft_cases()) >= CASES
    for case in soft_cases():
        path = os.path.join(GOLDEN, f"soft_{case}.npz")
        assert os.path.getsize(path) <= 150 * 1024
        g = np.load(path)
        assert g["n_penumbra"] > 0, case
        r, n = g["light_radius"], int(g["shadow_samples"])
        assert r.dtype == np.float32 and r.shape == (g["lights"].shape[1],) and (r > 0).any()
        assert 1 <= n <= 16
        assert g["u8"].shape == (len(g["coords"]), 3)
    assert int(np.load(os.path.join(GOLDEN, "soft_mixed_32_n16_d2.npz"))["shadow_samples"]) == 16
    assert (np.load(os.path.join(GOLDEN, "soft_mixed_32_n16_d2.npz"))["light_radius"] == 0).any()


def test_rim_fixture_differs_from_its_point_light_render():
    """The rim case: a small sphere beside light 0's centre.  Rays to the ball's points hit it where the lines through the
    centre miss it (n_anchor_miss: a light-anchored cull table would have certified those rays unoccluded), so the frame
    differs from the same scene with point lights."""
    g = np.load(os.path.join(GOLDEN, "soft_rim_48_d2.npz"))
    assert g["n_anchor_miss"] > 0
    differ = (g["u8"] != g["u8_point"]).any(axis=1)
    assert differ.sum() > 50
