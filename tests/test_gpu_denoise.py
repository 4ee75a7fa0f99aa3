"""The denoiser on the GPU (rt_render_guides, rt_film_denoise; the kernels of rt_guides.h and rt_denoise.h).  Truth is the numpy
restatement of python-ray-tracer_amd/denoise.py, which tests/test_denoise.py holds against the CPU oracle's leaf functions and
against the kernel's own text on the CPU; every comparison here is bit for bit.  The guides on seven stored scenes (8, 64 clustered
and 256 spheres reach every table layout), in a column slab in place, on an explicit grid, under a lens that is ignored, without a
material table and through rt_set_scene_sky; the filter on random finite sums over real guides for five frame sizes, with odd
strides and sentinels between the planes; through Film against the numpy chain; the quality figure; the error paths; two streams;
the example.  And what those scenes do not reach (tests/closest_hit_scenes.py): the guides of the tie scenes under the settings that
run every table mode of the kernel, each mode named by the library's MI355RT_LOG_KERNELS line; at the scene-size limits with
textures; textured clustered scenes; an empty scene; the filter at six levels, on synthetic guides and sums, on a frame with more
pixels than its grid has threads, and with planes more than 2^32 bytes apart."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, raygen_closed_form
import closest_hit_scenes as chs
from feature_gpu import IGNORED
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_closest_hit_scenes import limit_guides
from test_denoise import GUIDE_SCENES, guide_scene, guides_truth
from test_film import same_bits

from python_ray_tracer_amd import Film, denoise as D, film as F
from python_ray_tracer_amd import _lib as L

pytestmark = pytest.mark.gpu


def _read(r, d, shape, dtype=np.float64):
    a = np.empty(shape, dtype)
    r.d2h(a, d)
    return a


def _set_guide_scene(r, name, lens=None):
    g, w, h, tex = guide_scene(name)
    if tex is not None:
        r.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]), textures=tex)
    else:
        r.set_scene(g["spheres"], g["lights"], g["planes"])
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(*(lens or (0.0, 1.0)))
    r.set_raygen(w, h, *raygen_closed_form(w, h, float(g["fov"])))
    return g, w, h


def _guides(r, w, h, x0=0, x1=None, fill=None, stride=None):
    """rt_render_guides of columns [x0, x1) into a buffer of `stride` elements per plane pre-filled with NaN: (8, stride)."""
    x1 = w if x1 is None else x1
    stride = (x1 - x0) * h if stride is None else stride
    d = r.malloc(4 * 8 * stride)
    try:
        r.h2d(d, np.full(8 * stride, np.nan, np.float32))
        r.render_guides(x0, x1, d, stride)
        r.sync()
        return _read(r, d, (8, stride), np.float32)
    finally:
        r.free(d)


# ---------------------------------------------------------------------------------------------------------------------
# Symbols

def test_symbols_present():
    lib = L.load()
    assert hasattr(lib, "rt_render_guides") and hasattr(lib, "rt_film_denoise") and lib.rt_abi_version() == 7


# ---------------------------------------------------------------------------------------------------------------------
# Guides

@pytest.mark.parametrize("name", GUIDE_SCENES)
def test_guides_match_the_reference(rend, name):
    g, w, h = _set_guide_scene(rend, name)
    want = guides_truth(name)
    stride = w * h + 5                                            # (planes apart by more than the frame: the gap stays NaN)
    got = _guides(rend, w, h, stride=stride)
    bad = np.argwhere(got[:, :w * h].reshape(8, w, h).view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (name, len(bad), bad[:5], got[:, :w * h].reshape(8, w, h)[tuple(bad[0])], want[tuple(bad[0])])
    assert np.isnan(got[:, w * h:]).all()


def test_guides_column_slab_in_place(rend):
    g, w, h = _set_guide_scene(rend, "odd_37x29")
    want = guides_truth("odd_37x29")
    d = rend.malloc(4 * 8 * w * h)
    try:
        rend.h2d(d, np.full(8 * w * h, -777.0, np.float32))
        rend.render_guides(5, 22, d + 4 * 5 * h, w * h)
        rend.sync()
        got = _read(rend, d, (8, w, h), np.float32)
    finally:
        rend.free(d)
    assert same_bits(np.ascontiguousarray(got[:, 5:22]), np.ascontiguousarray(want[:, 5:22]))
    assert (got[:, :5] == -777.0).all() and (got[:, 22:] == -777.0).all()


def test_guides_on_an_explicit_grid(rend):
    g, w, h = _set_guide_scene(rend, "odd_37x29")
    rng = np.random.default_rng(2)
    px, y0, dy, z0, dz = raygen_closed_form(w, h, float(g["fov"]))
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="ij")
    loc = np.stack([np.full((w, h), px), xs * dy + y0, ys * dz + z0]) + rng.uniform(-0.004, 0.004, (3, w, h))   # not separable
    rend.set_pixel_loc(loc)
    want = D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h, pixel_loc=loc)
    got = _guides(rend, w, h).reshape(8, w, h)
    assert same_bits(got, want) and not same_bits(want, np.array(guides_truth("odd_37x29")))


def test_guides_ignore_a_lens_and_need_no_material_table(rend):
    """The textured scene (a material table) under an aperture: the sharp image's guides.  The frame_* scenes of
    test_guides_match_the_reference have no material table."""
    g, w, h = _set_guide_scene(rend, "texture_default_64_d4", lens=(0.2, 2.5))
    assert same_bits(_guides(rend, w, h).reshape(8, w, h), np.array(guides_truth("texture_default_64_d4")))


def test_guides_of_a_sky_scene(rend):
    g = np.load(os.path.join(GOLDEN, "sky_default_64_d4.npz"))
    w, h = 24, 40
    rend.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]),
                   light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]), light_rgb=g["light_rgb"], sky=g["sky"])
    rend.set_camera(g["cam_origin"], g["cam_rot"])
    rg = (2.4, 1.0, -2.0 / (w - 1), 2.2, -3.0 / (h - 1))           # (a grid that looks above the horizon: sky pixels)
    rend.set_raygen(w, h, *rg)
    want = D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h, raygen=rg)
    assert same_bits(_guides(rend, w, h).reshape(8, w, h), want)
    assert (want[7] < 0).any() and (want[7] >= 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# The guides in every table mode (MI355RT_LOG_KERNELS names the mode), at the scene-size limits, textured, of nothing

GUIDES_LINE = re.compile(r"mi355rt: guides_kernel<(\d+)>")
_MODES_SEEN = {}                                                  # setting -> (mode, clustered, S, lights)


def _knob_renderer(monkeypatch, knobs):
    """A context of its own under `knobs` that logs its kernels."""
    import python_ray_tracer_amd as pkg
    for k in chs.KNOB_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    return pkg.Renderer(0)


def _logged_modes(capfd):
    return [int(m) for m in GUIDES_LINE.findall(capfd.readouterr().err)]


def _same_guides(what, got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _run_guides_setting(name, monkeypatch, capfd):
    if name in _MODES_SEEN:
        return _MODES_SEEN[name]
    S, lights, knobs, clustered, mode, _, _ = chs.SETTINGS[name]
    with _knob_renderer(monkeypatch, knobs) as r:
        for case, reverse in [(c, rev) for c in range(chs.TIE_CASES) for rev in (False, True)]:
            sc = chs.tie_scene(case, S, 7, reverse, lights)
            r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
            r.set_camera(sc["cam_origin"], sc["cam_rot"])
            r.set_pixel_loc(sc["pixel_loc"])
            want = D.guides_reference(sc["spheres"], sc["planes"], sc["cam_origin"], sc["cam_rot"], 8, 8, pixel_loc=sc["pixel_loc"])
            assert (want[3] == np.float32(4.0)).all() and np.isin(want[7], sc["tie_at"].astype(np.float32)).all()
            capfd.readouterr()
            got = _guides(r, 8, 8).reshape(8, 8, 8)
            assert _logged_modes(capfd) == [mode], (name, case, reverse)
            _same_guides(f"{name} case {case} reverse={reverse}", got, want)
    _MODES_SEEN[name] = (mode, clustered, S, lights)
    return _MODES_SEEN[name]


@pytest.mark.parametrize("name", list(chs.SETTINGS))
def test_guides_every_table_mode(monkeypatch, capfd, name):
    """The tie scenes (tests/closest_hit_scenes.py: 16 spheres at equal distances at seeded caller indices among fillers) under the
    settings of tests/test_gpu_closest_hit.py, every case in both caller orders.  The id plane is the tie rule seen directly: the
    lowest caller index of the equal distances, whatever the slot.  The distance plane is 4.0 everywhere.  Every case, because the
    packer sorts equal keys by caller index: whether slot order and caller order part for the spheres of a tie depends on the axes
    it splits along, that is on the fillers, which differ from case to case."""
    print(f"{name}: guides_kernel<{_run_guides_setting(name, monkeypatch, capfd)[0]}>")


def test_guides_settings_reach_every_mode(monkeypatch, capfd):
    """Over the module (the settings run here if they have not yet): MODE 0 on a clustered scene and on a flat one, MODE 1 on
    both, MODE 2 at 1024 spheres with three lights (no anchors: origin-form cluster spheres in LDS) and with none (anchored)."""
    seen = {_run_guides_setting(name, monkeypatch, capfd) for name in chs.SETTINGS}
    print(f"guides_kernel (mode, clustered, S, lights) seen: {sorted(seen)}")
    assert {m for m, _, _, _ in seen} == {0, 1, 2}
    assert {(0, True), (0, False), (1, True), (1, False)} <= {(m, c) for m, c, _, _ in seen}
    assert {(2, True, 1024, 3), (2, True, 1024, 0)} <= seen


@pytest.mark.parametrize("n_lights", [3, 1])
def test_guides_at_the_scene_limits(monkeypatch, capfd, n_lights):
    """RT_MAX_SPHERES = 1024 spheres and 64 planes, every third sphere and every plane textured, n_lights lights, in a context of its own.
    Three lights leave no anchored cull table (MODE 2 with the clusters' origin-form spheres in LDS); one light keeps one and plans a dynamic
    LDS image of 66 608 B by plan_guides, above the 64 KiB a kernel gets unasked (tests/test_closest_hit_scenes.py evaluates
    rt_plan.h for both rows): the launch succeeds only if the limit was raised.  All eight planes against guides_reference, then a
    column slab [19, 45) in place."""
    sc = chs.limit_scene(n_lights)
    w, h = sc["w"], sc["h"]
    want = limit_guides(n_lights)
    with _knob_renderer(monkeypatch, {}) as r:
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"], materials=sc["materials"], textures=sc["textures"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        r.set_raygen(w, h, *sc["raygen"])
        capfd.readouterr()
        got = _guides(r, w, h).reshape(8, w, h)
        assert _logged_modes(capfd) == [2]
        _same_guides(f"limit scene L={n_lights}", got, want)
        d = r.malloc(4 * 8 * w * h)
        try:
            r.h2d(d, np.full(8 * w * h, -777.0, np.float32))
            r.render_guides(19, 45, d + 4 * 19 * h, w * h)
            r.sync()
            slab = _read(r, d, (8, w, h), np.float32)
        finally:
            r.free(d)
    _same_guides(f"limit scene L={n_lights} slab", np.ascontiguousarray(slab[:, 19:45]), np.ascontiguousarray(want[:, 19:45]))
    assert (slab[:, :19] == -777.0).all() and (slab[:, 45:] == -777.0).all()


@pytest.mark.parametrize("name, knobs, mode", [("c4_s64_d5_sub32", {}, 1), ("c5_s256_d8_sub96", {}, 2),
                                               ("c4_s64_d5_sub32", {"MI355RT_F32_RECORDS": "0"}, 0)], ids=["s64_mode1", "s256_mode2", "s64_mode0"])
def test_guides_textured_clustered(monkeypatch, capfd, name, knobs, mode):
    """A texel looked up at the hit point of a clustered scene: texel_of(hit_slot(...)) and the albedo go through slot order."""
    g, w, h, _ = guide_scene(name)
    S, P = g["spheres"].shape[1], g["planes"].shape[1]
    tex = chs.textures_for(S, P, S)
    table = np.tile(np.array([0.1, 0.6, 0.3, 0.0, 1.0, 0.0]), (4, 1))
    rg = raygen_closed_form(w, h, float(g["fov"]))
    want = D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h, raygen=rg, textures=tex)
    changed = int((want[4:7] != guides_truth(name)[4:7]).any(axis=0).sum())
    on_sphere = (want[7] >= 0) & (want[7] < S)
    changed_spheres = int(((want[4:7] != guides_truth(name)[4:7]).any(axis=0) & on_sphere).sum())
    print(f"{name}: textures change the albedo of {changed} of {w * h} pixels, {changed_spheres} of them on spheres")
    assert changed >= 100 and changed_spheres >= 30
    with _knob_renderer(monkeypatch, knobs) as r:
        r.set_scene(g["spheres"], g["lights"], g["planes"], materials=(table, np.arange(S) % 4, np.arange(P) % 4), textures=tex)
        r.set_camera(g["cam_origin"], g["cam_rot"])
        r.set_raygen(w, h, *rg)
        capfd.readouterr()
        got = _guides(r, w, h).reshape(8, w, h)
        assert _logged_modes(capfd) == [mode]
    _same_guides(f"{name} textured {knobs}", got, want)


def test_guides_of_an_empty_scene(rend):
    """No sphere, no plane, one light, 9 x 5: every pixel a miss, +0.0f in seven planes and -1.0f in the id plane, bit for bit."""
    w, h = 9, 5
    rend.set_scene(np.zeros((7, 0), np.float32), np.array([[1.0], [2.0], [3.0]], np.float32), np.zeros((9, 0), np.float32))
    rend.set_camera(np.zeros(3), np.eye(3))
    rend.set_raygen(w, h, *raygen_closed_form(w, h, 60.0))
    got = _guides(rend, w, h, stride=w * h + 3)
    assert (got[0:7, :w * h].view(np.uint32) == 0).all() and (got[7, :w * h].view(np.uint32) == np.float32(-1.0).view(np.uint32)).all()
    assert np.isnan(got[:, w * h:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# The filter on uploaded sums

def _soft_fixture():
    return np.load(os.path.join(GOLDEN, "soft_default_64_d4.npz"))


_SOFT_GUIDES = []


def soft_guides():
    """guides_reference of the soft_default_64_d4 frame, once."""
    if not _SOFT_GUIDES:
        g = _soft_fixture()
        w, h = int(g["w"]), int(g["h"])
        a = D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h, raygen=raygen_closed_form(w, h, float(g["fov"])))
        a.setflags(write=False)
        _SOFT_GUIDES.append(a)
    return _SOFT_GUIDES[0]


def _frame_guides(ws, h):
    if (ws, h) == (64, 64):
        return np.array(soft_guides())
    odd = guides_truth("odd_37x29")
    return np.ascontiguousarray(odd if (ws, h) == (37, 29) else odd[:, 10:10 + ws, 12:12 + h])


# (levels, normal_shin, sigma, demodulate, n): levels 0, 1, 2, 5 (both parities of the ping-pong), sigma 0 and > 0, demodulate 0 and 1,
# n 1 and 7
SETTINGS = [(0, 32, 0.0, 0, 7), (0, 1, 4.0, 1, 1), (1, 32, 0.0, 0, 1), (1, 4, 0.125, 1, 7), (2, 32, 16.0, 0, 7), (2, 1024, 0.125, 1, 1),
            (5, 32, 0.125, 1, 7), (5, 2, 0.0, 0, 1), (5, 32, 24.0, 0, 7), (2, 32, 0.0, 1, 7)]


@pytest.mark.parametrize("ws, h", [(1, 1), (1, 7), (5, 1), (37, 29), (64, 64)])
def test_denoise_matches_the_reference(rend, ws, h):
    """Strides larger than ws*h and odd (planes only 8-byte aligned, guide planes 4-byte), a sentinel in the padding of every buffer."""
    rng = np.random.default_rng(ws * 100 + h)
    npx = ws * h
    gd = _frame_guides(ws, h)
    ss, gs, os_, wk = ((npx + k) | 1 for k in (3, 1, 5, 7))       # odd, and larger than the frame
    hg = np.full((8, gs), np.float32(-5.0))
    hg[:, :npx] = gd.reshape(8, -1)
    d_sum, d_g, d_out, d_work = rend.malloc(24 * ss), rend.malloc(32 * gs), rend.malloc(24 * os_), rend.malloc(24 * wk)
    try:
        rend.h2d(d_g, hg)
        for levels, shin, sigma, dem, n in SETTINGS:
            s = rng.uniform(0.0, 300.0, (3, ws, h)) * n * (rng.random((3, ws, h)) < 0.9) - rng.uniform(0.0, 4.0, (3, ws, h))
            hs = np.full((3, ss), -12345.0)
            hs[:, :npx] = s.reshape(3, -1)
            rend.h2d(d_sum, hs)
            rend.h2d(d_out, np.full(3 * os_, -777.0))
            rend.h2d(d_work, np.full(3 * wk, -888.0))
            rend.film_denoise(d_sum, ws, h, n, d_g, d_out, d_work if levels >= 2 else None, levels=levels, normal_shin=shin, sigma=sigma,
                              demodulate=dem, sum_stride=ss, guide_stride=gs, out_stride=os_, work_stride=wk)
            rend.sync()
            got, work = _read(rend, d_out, (3, os_)), _read(rend, d_work, (3, wk))
            want = D.denoise_reference(s, n, gd, levels, shin, sigma, dem)
            what = f"{ws}x{h} levels={levels} shin={shin} sigma={sigma} demodulate={dem} n={n}"
            bad = np.argwhere(got[:, :npx].reshape(3, ws, h).view(np.uint64) != want.view(np.uint64))
            assert bad.size == 0, (what, len(bad), bad[:4], got[:, :npx].reshape(3, ws, h)[tuple(bad[0])], want[tuple(bad[0])])
            assert (got[:, npx:] == -777.0).all() and (work[:, npx:] == -888.0).all(), what
            if levels < 2:
                assert (work == -888.0).all(), what
            assert same_bits(_read(rend, d_sum, (3, ss)), hs), what     # the sum is read only
        assert same_bits(_read(rend, d_g, (8, gs), np.float32), hg)
    finally:
        for p in (d_sum, d_g, d_out, d_work):
            rend.free(p)


def _filter_synthetic(rend, ws, h, settings):
    """rt_film_denoise on synthetic_guides and synthetic_sums (tests/closest_hit_scenes.py) for every setting, with the odd strides
    and the sentinels of test_denoise_matches_the_reference; truth is filtered_truth, finite everywhere
    (tests/test_closest_hit_scenes.py), so equal bits are equal values."""
    npx = ws * h
    gd = chs.synthetic_guides(ws, h, 0)
    ss, gs, os_, wk = ((npx + k) | 1 for k in (3, 1, 5, 7))
    hg = np.full((8, gs), np.float32(-5.0))
    hg[:, :npx] = gd.reshape(8, -1)
    d_sum, d_g, d_out, d_work = rend.malloc(24 * ss), rend.malloc(32 * gs), rend.malloc(24 * os_), rend.malloc(24 * wk)
    try:
        rend.h2d(d_g, hg)
        for setting in settings:
            levels, shin, sigma, dem, n = setting
            s, want = chs.filtered_truth(ws, h, setting)
            hs = np.full((3, ss), -12345.0)
            hs[:, :npx] = s.reshape(3, -1)
            rend.h2d(d_sum, hs)
            rend.h2d(d_out, np.full(3 * os_, -777.0))
            rend.h2d(d_work, np.full(3 * wk, -888.0))
            rend.film_denoise(d_sum, ws, h, n, d_g, d_out, d_work if levels >= 2 else None, levels=levels, normal_shin=shin, sigma=sigma,
                              demodulate=dem, sum_stride=ss, guide_stride=gs, out_stride=os_, work_stride=wk)
            rend.sync()
            got, work = _read(rend, d_out, (3, os_)), _read(rend, d_work, (3, wk))
            what = f"{ws}x{h} levels={levels} shin={shin} sigma={sigma} demodulate={dem} n={n}"
            assert np.isfinite(want).all(), what
            bad = np.argwhere(got[:, :npx].reshape(3, ws, h).view(np.uint64) != want.view(np.uint64))
            assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[:, :npx].reshape(3, ws, h)[tuple(bad[0])], want[tuple(bad[0])])
            assert (got[:, npx:] == -777.0).all() and (work[:, npx:] == -888.0).all(), what
            if levels < 2:
                assert (work == -888.0).all(), what
            assert same_bits(_read(rend, d_sum, (3, ss)), hs), what
        assert same_bits(_read(rend, d_g, (8, gs), np.float32), hg)
    finally:
        for p in (d_sum, d_g, d_out, d_work):
            rend.free(p)


@pytest.mark.parametrize("ws, h", chs.SIX_FRAMES)
def test_denoise_six_levels(rend, ws, h):
    """levels = 6, taps 32 pixels apart, which no other launch of the suite reaches: at normal shininess 1 and 1024, sigma 2 and
    1/8, without and with demodulation.  (The sixth level changes 4206 and 2487 of the 6887 pixels of the 97 x 71 references:
    tests/test_closest_hit_scenes.py.)"""
    _filter_synthetic(rend, ws, h, chs.SIX_LEVELS)


@pytest.mark.parametrize("ws, h", chs.SYNTHETIC_FRAMES)
def test_denoise_synthetic_guides(rend, ws, h):
    """The ten SETTINGS on guides no rendered scene gives: a 1-pixel checkerboard of ids, small blocks, misses, an id above 1024,
    per-pixel random normals, albedos from 0 to 1e30; sums with exact zeros, negatives and eight pixels of 1e200, whose colour
    weight against every other pixel is exactly 0."""
    assert chs.DENOISE_SETTINGS == SETTINGS
    _filter_synthetic(rend, ws, h, SETTINGS)


def test_denoise_loops_past_the_grid_cap(rend):
    """A frame with more pixels than the launch has threads (8 blocks of 256 per CU): the grid-stride loop takes a second turn.
    1031 x 523 = 539 213 pixels against 524 288 on 256 CUs.  (torch is imported with the module, before the library loads: a
    first import of torch after that brings a second HIP runtime into the process, which finds no device.)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == rend.kernel_info()["cu_count"]                  # the number the library sizes the grid by
    ws, h = chs.grid_cap_frame(cus)
    assert ws * h > 8 * 256 * cus
    t0 = time.perf_counter()
    chs.filtered_truth(ws, h, chs.GRID_CAP_SETTING)
    t1 = time.perf_counter()
    _filter_synthetic(rend, ws, h, [chs.GRID_CAP_SETTING])
    print(f"grid cap: {ws} x {h} on {cus} CUs; reference {t1 - t0:.2f} s, device and read-back {time.perf_counter() - t1:.2f} s")


def _put(r, d, byte_offset, host):
    r.h2d(d + byte_offset, np.ascontiguousarray(host))


def _get(r, d, byte_offset, shape, dtype):
    return _read(r, d + byte_offset, shape, dtype)


def test_planes_far_apart(rend):
    """Every plane offset is 64-bit.  The guides of odd_37x29 with plane_stride = 2^28 + 2^26 + 1: plane 7 starts past element 2^31
    and byte 2^33.  Then the 37 x 29 filter at two levels three times, one of sum_stride, out_stride and work_stride 2^28 + 1 each
    time: plane 2 starts past byte 2^32.  One big buffer at a time (9.4 GB, then 4.3 GB), of which only the plane heads are written
    and read, a sentinel before and after each."""
    g, w, h = _set_guide_scene(rend, "odd_37x29")
    npx = w * h
    want = np.array(guides_truth("odd_37x29")).reshape(8, npx)
    stride = 2 ** 28 + 2 ** 26 + 1
    assert 7 * stride > 2 ** 31 and 4 * 7 * stride > 2 ** 33
    t0 = time.perf_counter()
    d = rend.malloc(4 * (7 * stride + npx + 1))
    try:
        for c in range(8):                                        # [sentinel] NaN x npx [sentinel] around every plane head
            _put(rend, d, 4 * (c * stride - (c > 0)), np.concatenate([np.full(int(c > 0), -777.0), np.full(npx, np.nan), [-777.0]]).astype(np.float32))
        rend.render_guides(0, w, d, stride)
        rend.sync()
        for c in range(8):
            got = _get(rend, d, 4 * (c * stride - (c > 0)), (npx + 1 + (c > 0),), np.float32)
            assert got[-1] == -777.0 and (c == 0 or got[0] == -777.0), c
            assert same_bits(np.ascontiguousarray(got[int(c > 0):-1]), want[c]), f"guide plane {c}"
    finally:
        rend.free(d)
    # the filter: demodulate 0, so that the work buffer holds the first level's result as denoise_reference(levels=1) states it
    gd = np.ascontiguousarray(want.reshape(8, w, h))
    s = chs.synthetic_sums(w, h, 3, 5)
    out2, out1 = D.denoise_reference(s, 3, gd, 2, 32, 2.0, 0), D.denoise_reference(s, 3, gd, 1, 32, 2.0, 0)
    assert np.isfinite(out2).all() and np.isfinite(out1).all() and not np.array_equal(out2, out1)
    big = 2 ** 28 + 1
    assert 8 * 2 * big > 2 ** 32
    d_g = rend.malloc(32 * npx)
    try:
        rend.h2d(d_g, gd)
        for which in ("sum", "out", "work"):
            strides = {k: (big if k == which else npx + 3) for k in ("sum", "out", "work")}
            bufs = {k: rend.malloc(8 * (2 * strides[k] + npx + 1)) for k in strides}
            try:
                for c in range(3):
                    _put(rend, bufs["sum"], 8 * c * strides["sum"], np.concatenate([s[c].reshape(-1), [-12345.0]]))
                    _put(rend, bufs["out"], 8 * c * strides["out"], np.full(npx + 1, -777.0))
                    _put(rend, bufs["work"], 8 * c * strides["work"], np.full(npx + 1, -888.0))
                rend.film_denoise(bufs["sum"], w, h, 3, d_g, bufs["out"], bufs["work"], levels=2, normal_shin=32, sigma=2.0, demodulate=0,
                                  sum_stride=strides["sum"], out_stride=strides["out"], work_stride=strides["work"])
                rend.sync()
                for c in range(3):
                    go = _get(rend, bufs["out"], 8 * c * strides["out"], (npx + 1,), np.float64)
                    gw = _get(rend, bufs["work"], 8 * c * strides["work"], (npx + 1,), np.float64)
                    gs_ = _get(rend, bufs["sum"], 8 * c * strides["sum"], (npx + 1,), np.float64)
                    assert go[-1] == -777.0 and gw[-1] == -888.0 and gs_[-1] == -12345.0, (which, c)
                    assert same_bits(np.ascontiguousarray(go[:-1]), np.ascontiguousarray(out2[c].reshape(-1))), f"{which}_stride 2^28 + 1: out plane {c}"
                    assert same_bits(np.ascontiguousarray(gw[:-1]), np.ascontiguousarray(out1[c].reshape(-1))), f"{which}_stride 2^28 + 1: work plane {c}"
                    assert same_bits(np.ascontiguousarray(gs_[:-1]), np.ascontiguousarray(s[c].reshape(-1))), (which, c)
            finally:
                for b in bufs.values():
                    rend.free(b)
    finally:
        rend.free(d_g)
    print(f"planes far apart: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------
# Through Film, and the quality figure

def _soft_scene(r, shadow_samples=None):
    """soft_default_64_d4 under RT_AA_NONE: area lights, the seed drives the light hashes."""
    g = _soft_fixture()
    w, h = int(g["w"]), int(g["h"])
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]),
                light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]) if shadow_samples is None else shadow_samples)
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(0.0, 1.0)
    r.set_raygen(w, h, *raygen_closed_form(w, h, float(g["fov"])))
    return w, h, lambda seed: r.params(**IGNORED, depth=int(g["depth"]), aa=0, seed=seed), int(g["seed"])


def _pass_frames(r, params_of, seed, n, w, h):
    d32 = r.malloc(12 * w * h)
    out = []
    try:
        for i in range(n):
            r.render_device(params_of(seed + i), 0, w, None, d32)
            r.sync()
            out.append(_read(r, d32, (3, w, h), np.float32))
    finally:
        r.free(d32)
    return out


def test_film_guides_denoise_resolve(rend):
    w, h, params_of, seed = _soft_scene(rend)
    frames = _pass_frames(rend, params_of, seed, 4, w, h)
    total = F.accumulate_reference(None, frames)
    with Film(rend) as film:
        film.accumulate(params_of(seed), 4)
        plain8, plain32 = film.resolve(white=400.0, f32=True)
        gd = film.guides()
        assert same_bits(gd, np.array(soft_guides()))
        film.denoise()
        u8, f32 = film.resolve(white=400.0, gamma=2, f32=True, denoised=True)
        den = D.denoise_reference(total, 4, gd, 4, 32, F.DENOISE_SIGMA, 1)
        v = F.tone_reference(den, 1, 1.0, 400.0, 2)
        assert same_bits(f32, v.astype(np.float32)) and np.array_equal(u8, F.clip_reference(v)[[0, 2, 1]])
        again8, again32 = film.resolve(white=400.0, f32=True)     # the plain resolve is what it was
        assert same_bits(again32, plain32) and np.array_equal(again8, plain8)
        assert same_bits(plain32, F.tone_reference(total, 4, 1.0, 400.0, 1).astype(np.float32))
        film.denoise(levels=1, normal_shininess=4, sigma=0.0, demodulate=False)
        _, f32 = film.resolve(u8=False, f32=True, denoised=True)
        assert same_bits(f32, D.denoise_reference(total, 4, gd, 1, 4, 0.0, 0).astype(np.float32))
        film.clear()
        film.accumulate(params_of(seed), 1)
        with pytest.raises(ValueError, match="denoise"):
            film.resolve(denoised=True)


def test_quality_the_filter_helps(rend):
    """soft_default_64_d4 with area lights and ONE shadow sample: truth is the mean of 1024 film passes; RMSE over all pixels and
    channels, linear colour, of the raw 4-pass mean and of its denoised version at Film.denoise's defaults (levels 4, normal
    shininess 32, sigma 1/8, demodulation).  Asserted: the filter helps.  The ratio is a result, printed with the sweep
    (measured on an MI355X: raw 4.33, denoised 3.70, ratio 0.853; DESIGN.md has the table)."""
    w, h, params_of, seed = _soft_scene(rend, shadow_samples=1)
    npx = w * h
    with Film(rend) as truth_film, Film(rend) as film:
        truth_film.accumulate(params_of(1000), 1024)
        film.accumulate(params_of(seed), 4)
        rend.sync()
        truth = _read(rend, truth_film.d_sum, (3, w, h)) / 1024.0
        raw = _read(rend, film.d_sum, (3, w, h)) / 4.0
        rmse = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
        film.denoise()
        rend.sync()
        den = _read(rend, film.d_denoised, (3, w, h))
        print(f"quality: rmse raw {rmse(raw):.4f} denoised {rmse(den):.4f} ratio {rmse(den) / rmse(raw):.4f}")
        for sigma in (1 / 32, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 4.0, 16.0, 64.0):
            film.denoise(sigma=sigma)
            rend.sync()
            print(f"quality: sigma {sigma:g} ratio {rmse(_read(rend, film.d_denoised, (3, w, h))) / rmse(raw):.4f}")
        assert npx == 4096 and rmse(den) < rmse(raw), (rmse(den), rmse(raw))


# ---------------------------------------------------------------------------------------------------------------------
# Error paths

def test_errors_leave_the_outputs_untouched(rend):
    import python_ray_tracer_amd as pkg
    g, w, h = _set_guide_scene(rend, "odd_37x29")
    npx = w * h
    d_g, d_sum, d_out, d_work = rend.malloc(32 * npx), rend.malloc(24 * npx), rend.malloc(24 * npx), rend.malloc(24 * npx)
    nan, inf = float("nan"), float("inf")
    try:
        rend.h2d(d_g, np.full(8 * npx, -777.0, np.float32))
        for what, call in {"NULL buffer": lambda: rend.render_guides(0, w, None, npx),
                           "short plane_stride": lambda: rend.render_guides(0, w, d_g, npx - 1),
                           "x1 > w": lambda: rend.render_guides(0, w + 1, d_g, 2 * npx),
                           "x0 < 0": lambda: rend.render_guides(-1, w, d_g, 2 * npx),
                           "x0 >= x1": lambda: rend.render_guides(5, 5, d_g, npx)}.items():
            with pytest.raises(pkg.RenderError) as e:
                call()
            assert e.value.status == L.RT_ERR_BAD_ARG, what
        with pkg.Renderer(0) as fresh:                            # no scene, then no grid
            d = fresh.malloc(32)
            with pytest.raises(pkg.RenderError) as e:
                fresh.render_guides(0, 1, d, 1)
            assert e.value.status == L.RT_ERR_STATE
            fresh.set_scene(g["spheres"], g["lights"], g["planes"])
            fresh.set_camera(g["cam_origin"], g["cam_rot"])
            with pytest.raises(pkg.RenderError) as e:
                fresh.render_guides(0, 1, d, 1)
            assert e.value.status == L.RT_ERR_STATE
            fresh.free(d)
        rend.sync()
        assert (_read(rend, d_g, (8 * npx,), np.float32) == -777.0).all(), "a refused call touched the guides"
        rend.render_guides(0, w, d_g, npx)
        rend.h2d(d_sum, np.full(3 * npx, 50.0))
        rend.h2d(d_out, np.full(3 * npx, -777.0))
        rend.h2d(d_work, np.full(3 * npx, -888.0))
        ok = dict(levels=2, normal_shin=32, sigma=1.0, demodulate=1)
        den = lambda *a, **kw: rend.film_denoise(*a, **{**ok, **kw})
        bad = {"NULL sum": lambda: den(None, w, h, 1, d_g, d_out, d_work),
               "NULL guides": lambda: den(d_sum, w, h, 1, None, d_out, d_work),
               "NULL out": lambda: den(d_sum, w, h, 1, d_g, None, d_work),
               "n 0": lambda: den(d_sum, w, h, 0, d_g, d_out, d_work),
               "levels -1": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, levels=-1),
               "levels 7": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, levels=7),
               "shin 0": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, normal_shin=0),
               "shin 3": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, normal_shin=3),
               "shin 2048": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, normal_shin=2048),
               "sigma < 0": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, sigma=-1.0),
               "sigma NaN": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, sigma=nan),
               "sigma inf": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, sigma=inf),
               "demodulate 2": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, demodulate=2),
               "reserved 1": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, reserved=1),
               "ws 0": lambda: den(d_sum, 0, h, 1, d_g, d_out, d_work),
               "h 0": lambda: den(d_sum, w, 0, 1, d_g, d_out, d_work),
               "ws*h above RT_FILM_MAX_PIXELS": lambda: den(d_sum, 2 ** 14, 2 ** 13 + 1, 1, d_g, d_out, d_work, sum_stride=2 ** 28,
                                                            guide_stride=2 ** 28, out_stride=2 ** 28, work_stride=2 ** 28),
               "short sum_stride": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, sum_stride=npx - 1),
               "short guide_stride": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, guide_stride=npx - 1),
               "short out_stride": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, out_stride=npx - 1),
               "short work_stride": lambda: den(d_sum, w, h, 1, d_g, d_out, d_work, work_stride=npx - 1),
               "NULL work with two levels": lambda: den(d_sum, w, h, 1, d_g, d_out, None),
               "out is the sum": lambda: den(d_sum, w, h, 1, d_g, d_sum, d_work),
               "work is the sum": lambda: den(d_sum, w, h, 1, d_g, d_out, d_sum),
               "work is out": lambda: den(d_sum, w, h, 1, d_g, d_out, d_out)}
        for what, call in bad.items():
            with pytest.raises(pkg.RenderError) as e:
                call()
            assert e.value.status == L.RT_ERR_BAD_ARG, what
        lib = L.load()                                            # a NULL settings pointer
        assert lib.rt_film_denoise(rend._ctx, d_sum, npx, w, h, 1, d_g, npx, None, d_out, npx, d_work, npx, None) == L.RT_ERR_BAD_ARG
        rend.sync()
        assert (_read(rend, d_out, (3 * npx,)) == -777.0).all() and (_read(rend, d_work, (3 * npx,)) == -888.0).all()
        den(d_sum, w, h, 1, d_g, d_out, d_work)                   # the context is still usable; a constant stays the constant
        den(d_sum, w, h, 1, d_g, d_work, None, levels=1)          # (one level needs no work buffer)
        rend.sync()
        assert np.allclose(_read(rend, d_out, (3 * npx,)), 50.0, rtol=1e-14) and np.allclose(_read(rend, d_work, (3 * npx,)), 50.0, rtol=1e-14)
    finally:
        for p in (d_g, d_sum, d_out, d_work):
            rend.free(p)


# ---------------------------------------------------------------------------------------------------------------------
# Streams

def test_two_streams_their_own_buffers(rend):
    """Guides and filters of two scenes on two streams, queued together: the serial results (scene, camera and grid travel with the
    launches; the cull tables are per stream)."""
    rng = np.random.default_rng(9)
    names = ("odd_37x29", "c5_s256_d8_sub96")
    streams = [rend.stream_create(), rend.stream_create()]
    bufs, sums = [], []
    try:
        for name, st in zip(names, streams):
            g, w, h = _set_guide_scene(rend, name)
            npx = w * h
            s = rng.uniform(0.0, 900.0, (3, w, h))
            d_g, d_sum, d_out, d_work = rend.malloc(32 * npx), rend.malloc(24 * npx), rend.malloc(24 * npx), rend.malloc(24 * npx)
            rend.h2d(d_sum, s)
            bufs.append((d_g, d_sum, d_out, d_work, w, h))
            sums.append(s)
            rend.render_guides(0, w, d_g, npx, st)
            rend.film_denoise(d_sum, w, h, 3, d_g, d_out, d_work, levels=3, normal_shin=32, sigma=2.0, demodulate=1, stream=st)
        for st in streams:
            rend.sync(st)
        for name, s, (d_g, d_sum, d_out, d_work, w, h) in zip(names, sums, bufs):
            gd = np.array(guides_truth(name))
            assert same_bits(_read(rend, d_g, (8, w, h), np.float32), gd), name
            assert same_bits(_read(rend, d_out, (3, w, h)), D.denoise_reference(s, 3, gd, 3, 32, 2.0, 1)), name
    finally:
        for st in streams:
            rend.stream_destroy(st)
        for b in bufs:
            for p in b[:4]:
                rend.free(p)


# ---------------------------------------------------------------------------------------------------------------------
# The example

def test_example_with_denoise_writes_pngs(tmp_path):
    """examples/render_png.py --denoise --guides: four passes of the sky scene with soft shadows, filtered, and the guide images."""
    from PIL import Image
    out, prefix = str(tmp_path / "den.png"), str(tmp_path / "guide")
    log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--sky", "--soft", "--shadow-samples", "1", "--passes", "4",
                                   "--white", "400", "--size", "64x64", "--frames", "2", "--denoise", "--denoise-levels", "3", "--guides", prefix,
                                   "--out", out], text=True)
    assert "wrote" in log and "denoise" in log
    img = np.asarray(Image.open(out))
    assert img.shape == (64, 64, 3) and img.any() and len(np.unique(img)) > 32
    for kind in ("normal", "depth", "albedo", "id"):
        a = np.asarray(Image.open(f"{prefix}_{kind}.png"))
        assert a.shape[:2] == (64, 64) and a.any(), kind
