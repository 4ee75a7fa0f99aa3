"""The sky on the GPU (rt_set_scene_sky, the sky kernels): every sky_* fixture through every entry point, all 56 sky kernels
through the dispatcher's environment overrides with the same bytes and the bytes of the CPU oracle's frames, fixtures against restated scenes (no sky, a black sky, an
unreachable sun, the sun everywhere, a uniform sky over an empty scene, the sky turned upside down), frames in flight across a
change of sky, column slabs, the error paths and the example."""
import ctypes as C

import numpy as np
import pytest

from conftest import raygen_closed_form
# The environment table and helpers are feature_gpu's, so that the sky kernels are held to the same tables as their twins.
from feature_gpu import (BIG, IGNORED, KERNEL_LINE, LIT_FAMILIES, check as _check, column_slabs_are_the_full_frame,
                         family_kernels_same_bytes, fixture_lens, frames as _frames, kw as _kw, lit_scene, render_host as _render_host,
                         run_example, same_frames as _same_frames, set_view, walk_entry_points)
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_sky import CASES, load_sky, packed
from test_lighting import fixture_textures, load_lighting

pytestmark = pytest.mark.gpu
SKY_FAMILIES = {"scatter": 15, "area_lights": 16, "lens": 17, "both": 18}   # rt::Family numbers of the sky kernels


def _mats(g, cols=8):
    return np.ascontiguousarray(g["materials"][:, :cols]), g["sphere_material"], g["plane_material"]


def _scene(r, g, sky="fixture", **kw):
    args = dict(materials=_mats(g), light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]),
                textures=fixture_textures(g), light_rgb=g["light_rgb"], sky=g["sky"] if isinstance(sky, str) else sky)
    args.update(kw)
    r.set_scene(g["spheres"], g["lights"], g["planes"], **args)


def _setup(r, g, explicit=False, **kw):
    return set_view(r, g, lambda r, g: _scene(r, g, **kw), lens=fixture_lens(g), explicit=explicit)


def _black(k):
    k = np.array(k, np.float64)
    for c in (3, 6, 9, 17, 20):
        k[c:c + 3] = 0.0
    return k


# ---------------------------------------------------------------------------------------------------------------------
# The fixtures (gen_lighting_golden's trace with sky_color(d) for a miss, tools/gen_sky_golden.py)

@pytest.mark.parametrize("case", CASES)
def test_fixture_every_entry_point(rend, case):
    g = load_sky(case)
    walk_entry_points(rend, g, _setup, case in BIG, cameras=True, begin_end=True, explicit=case != BIG[1])
    if "sky_b" in g.files:                                      # the same scene under the fixture's second sky
        _setup(rend, g, sky=g["sky_b"])
        u8, f32 = _render_host(rend, g)
        _check(dict(coords=g["coords"], u8=g["u8_b"], rgb64=g["rgb64_b"]), u8, f32, "sky_b")
    _setup(rend, g, sky=None)                                   # no sky: the fixture's u8_plain
    u8, _ = _render_host(rend, g)
    _check(g, u8, None, "without a sky", key="u8_plain")


# ---------------------------------------------------------------------------------------------------------------------
# One scene, the same bytes from every sky kernel (feature_gpu.family_kernels_same_bytes): the lighting table's scene under a
# sky, against its lighting twin without one.


SKY = packed(up=(0.0, 0.6, 0.8), zenith=(30.0, 80.0, 210.0), horizon=(230.0, 210.0, 190.0), nadir=(70.0, 60.0, 50.0), sharp=4.0,
             sun_dir=(0.8, 0.0, 0.6), sun_cos=0.97, sun_rgb=(250.0, 230.0, 180.0), halo_rgb=(120.0, 90.0, 40.0), halo_shin=16.0)


@pytest.mark.parametrize("kind", list(SKY_FAMILIES))
def test_every_sky_kernel_same_bytes(monkeypatch, capfd, oracle, kind):
    def scenes(src, case):
        _, mats, tex, rgb = lit_scene(src, case)                # (tiny: a sky scene without textures)
        lit = dict(materials=mats, textures=tex, light_rgb=rgb)
        return lit, dict(lit, sky=SKY)
    family_kernels_same_bytes(monkeypatch, capfd, oracle, kind, SKY_FAMILIES, load_lighting, (64, 64), "sky", scenes, twins=LIT_FAMILIES)
    assert sorted(SKY_FAMILIES.values()) == [15, 16, 17, 18]


# ---------------------------------------------------------------------------------------------------------------------
# Fixtures against restated scenes

@pytest.mark.parametrize("case", ["aa_48_d2", "everything_48_d4"])
def test_no_sky_and_a_black_sky_are_rt_set_scene_lighting(monkeypatch, capfd, case):
    """sky NULL or a sky with every colour zero: the twin family and its bytes.  An unreachable sun (a black gradient and halo,
    sun_rgb > 0, sun_cos = 2): the sky kernels, and the twin's bytes."""
    import python_ray_tracer_amd as pkg
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    g = load_sky(case)
    kind = "both" if case == "everything_48_d4" else "scatter"
    r = pkg.Renderer(0)
    try:
        _setup(r, g, sky=None)
        ref = _frames(r, g)
        _check(g, ref[0][0] if int(g["aa"]) == 0 else ref[1][0], None, "the twin", key="u8_plain")
        twin = {int(n[6]) for n in KERNEL_LINE.findall(capfd.readouterr().err)}
        assert twin == {LIT_FAMILIES[kind]} and 7 <= LIT_FAMILIES[kind] <= 14
        _scene(r, g, sky=_black(g["sky"]))
        _same_frames(_frames(r, g), ref, "a sky with every colour zero")
        names = KERNEL_LINE.findall(capfd.readouterr().err)
        assert len(names) >= 3 and {int(n[6]) for n in names} == twin, names
        unreachable = _black(g["sky"])
        unreachable[16], unreachable[17:20] = 2.0, (200.0, 150.0, 100.0)
        _scene(r, g, sky=unreachable)
        _same_frames(_frames(r, g), ref, "an unreachable sun")
        names = KERNEL_LINE.findall(capfd.readouterr().err)
        assert len(names) >= 3 and all(int(n[6]) == SKY_FAMILIES[kind] for n in names), names
    finally:
        r.close()


def test_white_lights_without_spec_under_an_unreachable_sun_is_the_materials_frame(monkeypatch, capfd):
    """A scene of the older entry points (white lights, no spec row, no texture) runs SKY_SCAT under a sky, the way it runs
    LIT_SCAT under a coloured light: with an unreachable sun the bytes are those of its own material kernels."""
    import python_ray_tracer_amd as pkg
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    g = load_sky("default_64_d4")
    r = pkg.Renderer(0)
    try:
        _setup(r, g, sky=None, materials=_mats(g, 6), light_rgb=None)
        ref = _frames(r, g)
        _check(g, ref[0][0], None, "the materials frame", key="u8_plain")
        twin = {int(n[6]) for n in KERNEL_LINE.findall(capfd.readouterr().err)}
        assert len(twin) == 1 and 1 <= min(twin) <= 3               # (a material family from before textures, by the table's columns)
        unreachable = _black(g["sky"])
        unreachable[16], unreachable[17:20] = 2.0, (1.0, 1.0, 1.0)
        _scene(r, g, sky=unreachable, materials=_mats(g, 6), light_rgb=None)
        _same_frames(_frames(r, g), ref, "an unreachable sun")
        assert {int(n[6]) for n in KERNEL_LINE.findall(capfd.readouterr().err)} == {15}
    finally:
        r.close()


def test_the_sun_everywhere_is_the_uniform_sky(rend):
    """A black gradient with sun_cos = -2 and sun_rgb = c: 0 + (t * 0) + c = c, the uniform sky c."""
    g = load_sky("events_48_d4")
    c = (61.5, 140.25, 222.0)
    _setup(rend, g, sky=packed(zenith=c, horizon=c, nadir=c))
    ref = _frames(rend, g)
    assert ref[0][0].any()
    sun = _black(g["sky"])
    sun[16], sun[17:20] = -2.0, c
    _scene(rend, g, sky=sun)
    _same_frames(_frames(rend, g), ref, "the sun everywhere")


@pytest.mark.parametrize("depth", [0, 3])
def test_a_uniform_sky_over_an_empty_scene_is_its_colour(rend, depth):
    c = (61.5, 140.25, 222.75)
    sp, pl = np.zeros((7, 0), np.float32), np.zeros((9, 0), np.float32)
    li = np.array([[0.0], [0.0], [5.0]], np.float32)
    none = np.zeros(0, np.int32)
    rend.set_scene(sp, li, pl, materials=(np.array([[0.1, 0.5, 0.3]]), none, none), sky=packed(zenith=c, horizon=c, nadir=c, sharp=8.0))
    g = load_sky("default_64_d4")
    rend.set_camera(g["cam_origin"], g["cam_rot"])
    w, h = 40, 24
    rend.set_raygen(w, h, *raygen_closed_form(w, h, 45.0))
    for aa, spp in ((0, 0), (1, 0), (2, 2)):
        u8, f32 = rend.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], depth, aa, u8=True, f32=True, spp=spp, seed=5)
        # (the stochastic mean is exact too: c has few bits, so c + c is exact and its half is c)
        want32 = np.broadcast_to(np.array(c, np.float32)[:, None, None], (3, w, h)).copy()
        want8 = np.broadcast_to(np.array([round(c[0]), round(c[2]), round(c[1])], np.uint8)[:, None, None], (3, w, h)).copy()
        if aa == 1:
            # the 9-tap mean of kernels.py:52-65 adds a neighbour's blue to green and its green to blue: an interior pixel is
            # (c_r, (c_g + 8 c_b) / 9, (c_b + 8 c_g) / 9); the sums are exact in any order, the quotient is rounded once
            mean = (c[0], (c[1] + 8.0 * c[2]) / 9.0, (c[2] + 8.0 * c[1]) / 9.0)
            want32[:, 1:-1, 1:-1] = np.array(mean, np.float32)[:, None, None]
            want8[:, 1:-1, 1:-1] = np.array([round(mean[0]), round(mean[2]), round(mean[1])], np.uint8)[:, None, None]
        assert (f32 == want32).all(), (aa, f32[:, 1, 1], want32[:, 1, 1])
        assert (u8 == want8).all(), (aa, u8[:, 1, 1], want8[:, 1, 1])        # (planes R, B, G; 61.5 rounds to even, 62)


def test_the_sky_upside_down_is_the_same_gradient(rend):
    """up and sun_dir negated and zenith swapped with nadir, black sun and halo: h changes sign exactly, far swaps with it."""
    g = load_sky("spheres_only_32_d3")
    k = np.array(g["sky"], np.float64)
    k[17:23] = 0.0
    _setup(rend, g, sky=k)
    ref = _frames(rend, g)
    assert ref[0][0].any()
    f = k.copy()
    f[0:3], f[13:16] = -k[0:3], -k[13:16]
    f[3:6], f[9:12] = k[9:12], k[3:6]
    _scene(rend, g, sky=f)
    _same_frames(_frames(rend, g), ref, "upside down")


# ---------------------------------------------------------------------------------------------------------------------
# The ring, slabs, errors, the example

def test_frames_in_flight_keep_their_sky(rend):
    g = load_sky("default_64_d4")
    w, h = _setup(rend, g)
    sky8, _ = _render_host(rend, g)
    _check(g, sky8, None, "sky")
    other = np.array(g["sky"], np.float64)
    other[3:6], other[6:9] = g["sky"][6:9], g["sky"][3:6]
    _scene(rend, g, sky=other)
    other8, _ = _render_host(rend, g)
    assert not np.array_equal(other8, sky8)
    p = rend.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), **_kw(g))
    npx = w * h
    s1, s2 = rend.stream_create(), rend.stream_create()
    bufs = [rend.malloc(3 * npx) for _ in range(6)]
    try:
        # six launches on two streams with a scene change before each: more changes than the ring has buffers
        kinds = ["sky", "other", "plain", "sky", "other", "sky"]
        for i, kind in enumerate(kinds):
            _scene(rend, g, sky=None if kind == "plain" else (g["sky"] if kind == "sky" else other))
            rend.render_device(p, 0, w, bufs[i], None, npx, stream=(s1, s2)[i % 2])
        rend.sync(s1)
        rend.sync(s2)
        for i, kind in enumerate(kinds):
            got = np.empty((3, w, h), np.uint8)
            rend.d2h(got, bufs[i])
            if kind == "other":
                assert np.array_equal(got, other8), f"launch {i}: the other sky"
            else:
                _check(g, got, None, f"launch {i} ({kind})", key="u8" if kind == "sky" else "u8_plain")
    finally:
        for b in bufs:
            rend.free(b)
        rend.stream_destroy(s1)
        rend.stream_destroy(s2)


@pytest.mark.parametrize("aa, spp", [(0, 0), (1, 0), (2, 2)])
def test_column_slab_is_the_full_frame(rend, aa, spp):
    column_slabs_are_the_full_frame(rend, load_sky("everything_48_d4"), _setup, aa, spp, ((9, 41), (33, 48)))


def test_errors_leave_the_previous_scene(rend):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = load_sky("default_64_d4")
    _setup(rend, g)
    nan, inf = float("nan"), float("inf")

    def sky(i, v):
        a = np.array(g["sky"], np.float64)
        a[i] = v
        return dict(sky=a)

    t, sid, pid = _mats(g)
    bad_row = t.copy()
    bad_row[0, 7] = 3.0
    cases = {"up not unit": sky(2, 1.01), "up short": sky(2, 0.99), "sun_dir not unit": sky(13, 1.5), "up nan": sky(0, nan),
             "zenith negative": sky(4, -1.0), "horizon inf": sky(6, inf), "nadir nan": sky(11, nan), "sun_rgb negative": sky(18, -0.5),
             "halo_rgb negative": sky(20, -1e-3), "halo_rgb inf": sky(22, inf), "sun_cos nan": sky(16, nan), "sun_cos inf": sky(16, inf),
             "sharp 3": sky(12, 3.0), "sharp 32": sky(12, 32.0), "sharp 0": sky(12, 0.0), "sharp nan": sky(12, nan),
             "halo_shin 0": sky(23, 0.0), "halo_shin 2048": sky(23, 2048.0), "halo_shin 1.5": sky(23, 1.5),
             # anything rt_set_scene_lighting refuses
             "light_rgb negative": dict(light_rgb=-np.ones((g["lights"].shape[1], 3), np.float32)),
             "shin 3": dict(materials=(bad_row, sid, pid)), "seven columns": dict(materials=(np.ascontiguousarray(t[:, :7]), sid, pid))}
    for what, kw in cases.items():
        with pytest.raises(pkg.RenderError) as e:
            _scene(rend, g, **kw)
        assert e.value.status == L.RT_ERR_BAD_ARG, what
        u8, f32 = _render_host(rend, g)                           # the previous scene stays current
        _check(g, u8, f32, f"after a refused scene ({what})")
    # through the C ABI: a sky without a material table; NULL arrays
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    s, l, p = (np.ascontiguousarray(g[k], np.float32) for k in ("spheres", "lights", "planes"))
    t = np.ascontiguousarray(t, np.float64)
    si, pi = np.ascontiguousarray(sid, np.int32), np.ascontiguousarray(pid, np.int32)
    rad = np.ascontiguousarray(g["light_radius"], np.float32)
    k_ = np.ascontiguousarray(g["sky"], np.float64)

    def call(ctx=rend._ctx, M=t.shape[0], ncols=8, radius=rad.ctypes.data_as(fp), k=k_):
        return rend._lib.rt_set_scene_sky(ctx, s.ctypes.data_as(fp), s.shape[1], l.ctypes.data_as(fp), l.shape[1], p.ctypes.data_as(fp),
                                          p.shape[1], 0, t.ctypes.data_as(C.POINTER(C.c_double)), M, ncols, si.ctypes.data_as(ip),
                                          pi.ctypes.data_as(ip), radius, int(g["shadow_samples"]), None, 0, None, None, None, 0, None,
                                          k.ctypes.data_as(C.POINTER(C.c_double)))

    for what, kw in {"ctx NULL": dict(ctx=None), "light_radius NULL": dict(radius=None), "a sky with M == 0": dict(M=0),
                     "ncols 7": dict(ncols=7)}.items():
        assert call(**kw) == L.RT_ERR_BAD_ARG, what
        u8, f32 = _render_host(rend, g)
        _check(g, u8, f32, f"after a refused scene ({what})")
    with pytest.raises(ValueError):                               # Python: a sky without a material table
        rend.set_scene(g["spheres"], g["lights"], g["planes"], sky=g["sky"])
    with pytest.raises(ValueError):                               # one double too few
        _scene(rend, g, sky=g["sky"][:-1])
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels for a scene with materials
        _render_host(rend, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(rend, g)
    _check(g, u8, f32, "after the refused launch")
    assert call() == L.RT_OK                                      # (the same scene through the C ABI itself, NULL texture arrays)
    u8, f32 = _render_host(rend, g)
    _check(g, u8, f32, "rt_set_scene_sky through the C ABI")


def test_example_with_sky_writes_png(tmp_path):
    """examples/render_png.py --sky: the top row of the picture is sky, not black."""
    _, img = run_example(str(tmp_path / "sky.png"), "64x64", 3, 2, "--sky")
    assert img.shape == (64, 64, 3) and img[0].min() > 0 and img[0, :, 2].min() > 100     # blue all along the top row
