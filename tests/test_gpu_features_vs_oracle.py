"""The feature kernels (rt_device.h MAT, REFR, SCAT, SOFT and LENS) against the CPU oracle's restatement of include/mi355rt.h
(oracle/rt_oracle.c orc_render_ex, pinned to every pixel of the feature fixtures by tests/test_oracle_features.py): full frames,
uint8 and float32, bit for bit.  Every feature kernel through the dispatcher's environment overrides, seeded random scenes of
every feature together, the scene-size limits, depth 16, spp 64, the typed bias, a lens on a non-planar explicit grid, and
every entry point.  Each case checks that its feature is live: the oracle's frame changes when that feature is turned off."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, raygen_closed_form
from closest_hit_scenes import size_limit_arrays
from feature_gpu import (ENVS, ENVS_IDS, ENVS_KEYS, FAMILIES, IGNORED, MODES, family_scene, oracle_modes, same as _same,
                         same_pixels as _same_pixels)

sys.path.insert(0, os.path.join(REPO, "tools"))
import feature_scenes as fs  # noqa: E402

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# Every feature kernel.  The (scene, environment) pairs of feature_gpu.ENVS: between them the dispatcher picks every
# instantiation it can pick (flat or clustered, sphere count, LDS image, parked or register state): all 22 MAT kernels and 14 of
# each REFR, SCAT, SOFT and LENS set (a kernel trace of this module shows the 92).  Each family runs on the scene with a seeded
# random table (feature_gpu.family_scene), in AA modes 0, 1 (the lattice and RT_FLAG_AA_PER_PIXEL) and 2, and every setting is
# compared with the oracle.
@pytest.mark.parametrize("case, env", ENVS, ids=ENVS_IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_every_feature_kernel_vs_oracle(monkeypatch, oracle, family, case, env):
    import python_ray_tracer_amd as pkg
    for k in ENVS_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = family_scene(family, case)
    refs, n_live = oracle_modes(oracle, family, case)
    assert n_live >= 20, f"{family} on {case}: the feature changes only {n_live} pixels"
    r = pkg.Renderer(0)
    try:
        for (aa, flags, spp), (r8, r32) in zip(MODES, refs):
            u8, f32 = fs.gpu_frame(r, {**sc, "aa": aa, "flags_aa": flags, "spp": max(spp, 1)})
            _same(f"{family} {case} {env} aa={aa} flags={flags}", u8, f32, r8, r32)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------------
# Seeded random scenes with every feature together (tools/feature_scenes.py), each kind of bias at least twice.  Every feature
# is live in each: turning it off changes at least 5 pixels of the oracle's frame.
RANDOM_SEEDS = [0, 1, 6, 7, 11, 12, 14, 15, 16, 18, 19, 22, 25, 26, 30, 44, 47, 49, 50, 53, 57, 62, 80, 113, 116, 138, 141, 154]


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_feature_scene_vs_oracle(renderer, oracle, seed):
    sc = fs.draw(seed)
    r8, r32 = fs.oracle_frame(oracle, sc)
    lv = fs.live(oracle, sc, r8)
    assert min(lv.values()) >= 5, (sc["kind"], lv)
    try:
        u8, f32 = fs.gpu_frame(renderer, sc)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same(f"seed {seed} ({sc['kind']}, S={sc['spheres'].shape[1]}, depth {sc['depth']}, aa {sc['aa']})", u8, f32, r8, r32)


# ---------------------------------------------------------------------------------------------------------------------
# The gaps of the fixtures: many lights with radii, the scene-size limits, depth 16, spp 64, the typed bias, a non-planar grid.

def _check_full(renderer, oracle, sc, what, min_live=("soft",), **kw):
    r8, r32 = fs.oracle_frame(oracle, sc)
    lv = fs.live(oracle, sc, r8)
    for f in min_live:
        assert lv[f] >= 5, (what, lv)
    try:
        u8, f32 = fs.gpu_frame(renderer, sc, **kw)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same(what, u8, f32, r8, r32)


@pytest.mark.parametrize("NL", [9, 33, 64])
def test_many_area_lights(renderer, oracle, NL):
    """L up to 64 (the key's light index m < 64) with mixed zero and nonzero radii, n = 3."""
    sc = fs.draw(11, w=48, h=32)
    rng = np.random.default_rng(NL)
    li = rng.uniform(-4, 6, (3, NL)).astype(np.float32)
    li[2] = np.abs(li[2]) + 2.0
    li *= np.float32(fs.draw(11)["spheres"][3].mean() / 0.7)
    rad = (rng.uniform(0.1, 0.8, NL) * (rng.uniform(size=NL) < 0.6)).astype(np.float32)
    rad[NL - 1] = 0.6
    sc.update(lights=li, radius=rad * np.float32(sc["spheres"][3].mean()), n=3, depth=3, aa=0)
    _check_full(renderer, oracle, sc, f"{NL} area lights", min_live=("soft", "lens"))


def test_scene_size_limits_sampled(renderer, oracle):
    """M = 256 rows with ids over every row, S = 1024, P = 64, L = 64 with radii, a lens: sampled pixels (render_pixels)."""
    rng = np.random.default_rng(1024)
    S, P, NL, M = 1024, 64, 64, 256
    sp, pl, li, table, sid, pid = size_limit_arrays(rng, S, P, NL, M)      # (the generator limit_scene shares: closest_hit_scenes.py)
    assert set(sid.tolist()) == set(range(M))
    w, h = 256, 160
    sc = dict(kind="limits", w=w, h=h, spheres=sp, lights=li, planes=pl, table=table, sid=sid, pid=pid,
              radius=(rng.uniform(0.1, 0.6, NL) * (np.arange(NL) % 3 != 0)).astype(np.float32), n=2, lens=(0.05, 6.0),
              cam_origin=np.zeros(3), cam_rot=np.eye(3), fov=60.0, raygen=raygen_closed_form(w, h, 60.0), depth=3, aa=0,
              flags_aa=0, spp=1, hseed=77, typed=0)
    co = np.stack([rng.integers(0, w, 300), rng.integers(0, h, 300)], axis=1).astype(np.int32)
    kw = fs.oracle_kwargs(sc)
    args = (w, h, co, sc["cam_origin"], sc["cam_rot"], sp, li, pl, 0.0, 0.0, 0.0, sc["depth"], 0)
    r8, r64 = oracle.render_pixels(*args, **kw)
    o8, _ = oracle.render_pixels(*args, **{**kw, "light_radius": np.zeros(NL, np.float32), "lens": None})
    assert (o8 != r8).any(axis=1).sum() >= 10                    # area lights and the lens are live at the sampled pixels
    try:
        u8, f32 = fs.gpu_frame(renderer, sc)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same_pixels("limits", co, u8, f32, r8, r64)


@pytest.mark.parametrize("seed", [4, 14, 31])
def test_depth_16_mirrors_and_glass(renderer, oracle, seed):
    """refl = 1 mirrors, glass and rough rows at depth 16 (the key's bounce field b at its full width): bounces 9 to 16 change
    the oracle's frame (it differs from the same scene at depth 8), and every feature is live."""
    sc = fs.draw(seed, kind="mirror16")
    assert sc["depth"] == 16
    d16, d8 = fs.oracle_frame(oracle, sc)[0], fs.oracle_frame(oracle, {**sc, "depth": 8})[0]
    assert (d16 != d8).any(axis=0).sum() >= 20
    _check_full(renderer, oracle, sc, f"depth 16, seed {seed}", min_live=("materials", "glass", "rough", "soft", "lens"))


def test_spp_64(renderer, oracle):
    """spp 64 on a small frame (the key's sample field s at its full width) with every feature."""
    sc = fs.draw(16, w=20, h=12)
    sc.update(aa=2, spp=64, depth=3)
    _check_full(renderer, oracle, sc, "spp 64", min_live=("glass", "soft", "lens"))


@pytest.mark.parametrize("family", ["mat", "refr", "scat", "soft", "lens_scat", "lens_soft"])
def test_typed_bias_on_each_family(renderer, oracle, family):
    """RT_FLAG_TYPED_BIAS (float64 BIAS*N of a plane hit) on a scene with a glass window and a floor: the trace's biased
    point, the window pass-through and the scatter origin; it must change the float32 frame."""
    sc = fs.draw(49, w=48, h=32, kind="window")                   # (scale 1e-3: BIAS is large against the scene)
    t = np.array(sc["table"])
    if family == "mat":
        sc["table"] = t[:, :3]
    elif family == "refr":
        sc["table"] = t[:, :5]
    sc["pid"] = np.array([3, 2], np.int32)                       # the window glass, the floor rough
    if family not in ("soft", "lens_soft"):
        sc["radius"] = np.zeros_like(sc["radius"])
    if not family.startswith("lens"):
        sc["lens"] = (0.0, 1.0)
    sc.update(depth=4, aa=0, typed=1)
    r8, r32 = fs.oracle_frame(oracle, sc)
    _, u32 = fs.oracle_frame(oracle, {**sc, "typed": 0})
    assert (u32.view(np.uint32) != r32.view(np.uint32)).any(axis=0).sum() >= 5
    try:
        u8, f32 = fs.gpu_frame(renderer, sc)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same(f"typed bias {family}", u8, f32, r8, r32)


@pytest.mark.parametrize("aa, flags", [(0, 0), (1, 0)])
def test_lens_on_a_non_planar_explicit_grid(renderer, oracle, aa, flags):
    """F = O + (f / P.x) v with P.x the explicit grid's own first row, varying per pixel, and the 9-tap midpoints of it."""
    sc = fs.draw(22, w=40, h=28)
    w, h = sc["w"], sc["h"]
    px, y0, dy, z0, dz = sc["raygen"]
    rng = np.random.default_rng(5)
    grid = np.empty((3, w, h))
    grid[0] = px * rng.uniform(0.6, 1.6, (w, h))
    grid[1] = (np.arange(w) * dy + y0)[:, None] + rng.uniform(-0.3, 0.3, (w, h)) * abs(dy)
    grid[2] = (np.arange(h) * dz + z0)[None, :]
    sc.update(aa=aa, flags_aa=flags, depth=3)
    ref = oracle.render(w, h, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], 0.0, 0.0, 0.0, 3, aa,
                        want=("u8", "f32"), **{**fs.oracle_kwargs(sc), "raygen": None, "pixel_loc": grid})
    planar = oracle.render(w, h, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], 0.0, 0.0, 0.0, 3, aa,
                           want=("u8",), **fs.oracle_kwargs(sc))["u8"]
    assert (planar != ref["u8"]).any(axis=0).sum() >= 20
    try:
        renderer.set_scene(sc["spheres"], sc["lights"], sc["planes"], materials=(sc["table"], sc["sid"], sc["pid"]),
                           light_radius=sc["radius"], shadow_samples=sc["n"])
        renderer.set_camera(sc["cam_origin"], sc["cam_rot"])
        renderer.set_lens(*sc["lens"])
        renderer.set_pixel_loc(grid)
        u8, f32 = renderer.render(*IGNORED.values(), 3, aa, u8=True, f32=True, flags=flags, seed=sc["hseed"])
    finally:
        renderer.set_lens(0.0, 1.0)
    _same(f"explicit non-planar grid aa={aa}", u8, f32, ref["u8"], ref["f32"])


# ---------------------------------------------------------------------------------------------------------------------
# Entry points and layout.

def test_chunked_host_path_half_megapixel(renderer, oracle):
    """rt_render on 1024 x 512 (0.52 MP: four column chunks on the host path), sampled pixels against the oracle."""
    sc = fs.draw(12, w=1024, h=512)
    sc.update(raygen=raygen_closed_form(1024, 512, sc["fov"]), aa=1, flags_aa=0, depth=4)
    rng = np.random.default_rng(512)
    co = np.stack([rng.integers(0, 1024, 500), rng.integers(0, 512, 500)], axis=1).astype(np.int32)
    co[:4] = [[0, 0], [1023, 511], [255, 100], [256, 100]]       # the frame's corners and a chunk seam
    args = (1024, 512, co, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], 0.0, 0.0, 0.0, 4, 1)
    r8, r64 = oracle.render_pixels(*args, **fs.oracle_kwargs(sc))
    o8, _ = oracle.render_pixels(*args, **{**fs.oracle_kwargs(sc), "lens": None})
    assert (o8 != r8).any(axis=1).sum() >= 50
    try:
        u8, f32 = fs.gpu_frame(renderer, sc)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same_pixels("rt_render 0.5 MP", co, u8, f32, r8, r64)


def test_render_device_and_odd_column_slabs(renderer, oracle):
    """rt_render_device into a full frame, and slabs [x0, x1) at odd offsets against the oracle on [x0, x1) (X is the absolute
    column of the key)."""
    sc = fs.draw(25, w=53, h=29)
    sc.update(aa=1, flags_aa=0)
    r8, r32 = fs.oracle_frame(oracle, sc)
    lv = fs.live(oracle, sc, r8)
    assert lv["lens"] >= 20 and lv["rough"] >= 20 and lv["soft"] >= 20, lv     # the keyed features, whose key holds X
    w, h = sc["w"], sc["h"]
    try:
        fs.gpu_frame(renderer, sc)
        p = renderer.params(*IGNORED.values(), sc["depth"], sc["aa"], spp=sc["spp"], seed=sc["hseed"])
        d8, d32 = renderer.malloc(3 * w * h), renderer.malloc(12 * w * h)
        try:
            renderer.render_device(p, 0, w, d8, d32, w * h)
            renderer.sync()
            g8, g32 = np.empty((3, w, h), np.uint8), np.empty((3, w, h), np.float32)
            renderer.d2h(g8, d8)
            renderer.d2h(g32, d32)
        finally:
            renderer.free(d8)
            renderer.free(d32)
        _same("rt_render_device", g8, g32, r8, r32)
        for aa, spp in ((1, 1), (2, 3), (0, 1)):
            for x0, x1 in ((1, 52), (7, 20), (33, 53), (17, 18)):
                s8, s32 = fs.oracle_frame(oracle, {**sc, "aa": aa, "spp": spp}, x0=x0, x1=x1)
                u8, f32 = renderer.render(*IGNORED.values(), sc["depth"], aa, x0=x0, x1=x1, u8=True, f32=True, spp=spp, seed=sc["hseed"])
                _same(f"slab [{x0}, {x1}) aa={aa}", u8, f32, s8[:, x0:x1], s32[:, x0:x1])
    finally:
        renderer.set_lens(0.0, 1.0)


def test_render_sequence_per_frame_cameras_with_a_lens(renderer, oracle):
    """rt_render_sequence with cameras != NULL: each frame of its own camera, all through the context's lens."""
    sc = fs.draw(47, w=40, h=24)
    sc.update(aa=0, flags_aa=0)
    w, h, n = sc["w"], sc["h"], 3
    from python_ray_tracer_amd.scene.rotation import euler_rotation
    cams = []
    for i in range(n):
        o = np.asarray(sc["cam_origin"]) + np.array([0.0, 0.1 * i, 0.05 * i]) * float(sc["spheres"][3].mean())
        R = np.asarray(euler_rotation(2.0 * i, -3.0 * i, 5.0 * i), np.float64) @ np.asarray(sc["cam_rot"])
        cams.append(np.concatenate([o, R.reshape(9)]))
    cams = np.array(cams)
    try:
        fs.gpu_frame(renderer, sc)
        p = renderer.params(*IGNORED.values(), sc["depth"], 0, seed=sc["hseed"])
        npx = w * h
        d8, d32 = renderer.malloc(n * 3 * npx), renderer.malloc(n * 12 * npx)
        try:
            renderer.render_sequence(p, 0, w, n, d8, d32, npx, 3 * npx, cams, None, 0)
            renderer.sync()
            g8, g32 = np.empty((n, 3, w, h), np.uint8), np.empty((n, 3, w, h), np.float32)
            renderer.d2h(g8, d8)
            renderer.d2h(g32, d32)
        finally:
            renderer.free(d8)
            renderer.free(d32)
    finally:
        renderer.set_lens(0.0, 1.0)
    prev = None
    for i in range(n):
        c = {**sc, "cam_origin": cams[i, :3], "cam_rot": cams[i, 3:].reshape(3, 3)}
        r8, r32 = fs.oracle_frame(oracle, c)
        assert fs.live(oracle, c, r8)["lens"] >= 5
        _same(f"rt_render_sequence frame {i}", g8[i], g32[i], r8, r32)
        assert prev is None or not np.array_equal(prev, r8)
        prev = r8
