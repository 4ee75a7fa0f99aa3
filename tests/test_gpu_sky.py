"""The sky on the GPU (rt_set_scene_sky, the sky kernels): every sky_* fixture through every entry point, all 56 sky kernels
through the dispatcher's environment overrides with the same bytes and the bytes of the CPU oracle's frames, fixtures against restated scenes (no sky, a black sky, an
unreachable sun, the sun everywhere, a uniform sky over an empty scene, the sky turned upside down), frames in flight across a
change of sky, column slabs, the error paths and the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import REPO, load_frame, raygen_closed_form
# The environment table and helpers are those of the lens, texture and lighting tests, imported and not copied, so that the sky
# kernels are held to the same tables as their twins.
from test_sky import CASES, load_sky, packed
from test_lighting import fixture_textures, load_lighting
from test_gpu_lens import _VARIANTS, _ENV_KEYS as _VARIANT_KEYS, _grid, _lens_materials
from test_gpu_textures import _scene_textures
from test_gpu_features_vs_oracle import _same
from test_gpu_lit_vs_oracle import kernel_table_refs
from test_gpu_lighting import IGNORED, KERNEL_LINE, LIT_FAMILIES, _check, _glossy, _kw, _mats, _render_host, _frames, _same_frames

pytestmark = pytest.mark.gpu
BIG = ("c4_s64_d5_sub32", "c5_s256_d8_sub96")
SKY_FAMILIES = {"scatter": 15, "area_lights": 16, "lens": 17, "both": 18}   # rt::Family numbers of the sky kernels


@pytest.fixture
def rend(renderer):
    """The session's renderer, with the pinhole camera restored afterwards (later tests share it)."""
    yield renderer
    renderer.set_lens(0.0, 1.0)


def _scene(r, g, sky="fixture", **kw):
    args = dict(materials=_mats(g), light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]),
                textures=fixture_textures(g), light_rgb=g["light_rgb"], sky=g["sky"] if isinstance(sky, str) else sky)
    args.update(kw)
    r.set_scene(g["spheres"], g["lights"], g["planes"], **args)


def _setup(r, g, explicit=False, **kw):
    w, h = int(g["w"]), int(g["h"])
    _scene(r, g, **kw)
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(float(g["aperture"]), float(g["focus_distance"]))
    rg = raygen_closed_form(w, h, float(g["fov"]))
    if explicit:
        r.set_pixel_loc(_grid(w, h, rg))
    else:
        r.set_raygen(w, h, *rg)
    return w, h


def _black(k):
    k = np.array(k, np.float64)
    for c in (3, 6, 9, 17, 20):
        k[c:c + 3] = 0.0
    return k


# ---------------------------------------------------------------------------------------------------------------------
# The fixtures (gen_lighting_golden's trace with sky_color(d) for a miss, tools/gen_sky_golden.py)

@pytest.mark.parametrize("case", CASES)
def test_fixture_every_entry_point(rend, case):
    renderer = rend
    g = load_sky(case)
    w, h = _setup(renderer, g)
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "rt_render")
    big = case in BIG
    p = renderer.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), **_kw(g))
    n, npx = 3, w * h
    d8 = renderer.malloc(n * 3 * npx)
    d32 = None if big else renderer.malloc(n * 12 * npx)
    try:
        renderer.render_device(p, 0, w, d8, d32, npx)
        renderer.sync()
        got = np.empty((3, w, h), np.uint8)
        renderer.d2h(got, d8)
        g32 = None
        if d32 is not None:
            g32 = np.empty((3, w, h), np.float32)
            renderer.d2h(g32, d32)
        _check(g, got, g32, "rt_render_device")
        for cams in (None, np.tile(np.concatenate([g["cam_origin"], g["cam_rot"].reshape(9)]), (n, 1))):
            renderer.h2d(d8, np.zeros(n * 3 * npx, np.uint8))
            renderer.render_sequence(p, 0, w, n, d8, d32, npx, 3 * npx, cams, None, 2)   # (cameras=None: launches of 2 frames)
            renderer.sync()
            seq = np.empty((n, 3, w, h), np.uint8)
            renderer.d2h(seq, d8)
            s32 = None
            if d32 is not None:
                s32 = np.empty((n, 3, w, h), np.float32)
                renderer.d2h(s32, d32)
            for i in range(n):
                _check(g, seq[i], None if s32 is None else s32[i], f"rt_render_sequence cameras={cams is not None} frame {i}")
    finally:
        renderer.free(d8)
        if d32 is not None:
            renderer.free(d32)
    if not big:                                                 # rt_render_begin / rt_render_end
        o8, o32 = np.empty((3, w, h), np.uint8), np.empty((3, w, h), np.float32)
        renderer.render_begin(0, IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), o8, o32, **_kw(g))
        renderer.render_end(0)
        _check(g, o8, o32, "rt_render_begin/end")
    if int(g["aa"]) != 2 and case != "c5_s256_d8_sub96":       # stochastic needs the closed-form grid
        _setup(renderer, g, explicit=True)
        u8, f32 = _render_host(renderer, g)
        _check(g, u8, f32, "explicit pixel_loc")
    if int(g["aa"]) == 1:                                       # the per-pixel 9-tap kernel on the closed-form grid
        from python_ray_tracer_amd import _lib as L
        _setup(renderer, g)
        u8, f32 = _render_host(renderer, g, flags=L.RT_FLAG_AA_PER_PIXEL)
        _check(g, u8, f32, "RT_FLAG_AA_PER_PIXEL")
    if "sky_b" in g.files:                                      # the same scene under the fixture's second sky
        _setup(renderer, g, sky=g["sky_b"])
        u8, f32 = _render_host(renderer, g)
        _check(dict(coords=g["coords"], u8=g["u8_b"], rgb64=g["rgb64_b"]), u8, f32, "sky_b")
    _setup(renderer, g, sky=None)                               # no sky: the fixture's u8_plain
    u8, _ = _render_host(renderer, g)
    _check(g, u8, None, "without a sky", key="u8_plain")


# ---------------------------------------------------------------------------------------------------------------------
# One scene, the same bytes from every sky kernel.  test_gpu_lens.py's environment table x the four AA modes reaches all 14
# shapes of a family; MI355RT_LOG_KERNELS makes every launch name its kernel on stderr.

SKY = packed(up=(0.0, 0.6, 0.8), zenith=(30.0, 80.0, 210.0), horizon=(230.0, 210.0, 190.0), nadir=(70.0, 60.0, 50.0), sharp=4.0,
             sun_dir=(0.8, 0.0, 0.6), sun_cos=0.97, sun_rgb=(250.0, 230.0, 180.0), halo_rgb=(120.0, 90.0, 40.0), halo_shin=16.0)


@pytest.mark.parametrize("kind", list(SKY_FAMILIES))
def test_every_sky_kernel_same_bytes(monkeypatch, capfd, oracle, kind):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    soft, lens = kind in ("area_lights", "both"), kind in ("lens", "both")
    w, h = 64, 64
    modes = ((0, 0, 0), (1, 0, 0), (1, L.RT_FLAG_AA_PER_PIXEL, 0), (2, 0, 2))
    seen = set()
    for case in _VARIANTS:
        if case == "tiny":
            g = load_frame("aa_48_d2")
            src = dict(spheres=g["spheres"][:, :1], lights=g["lights"][:, :1], planes=g["planes"][:, :0], fov=g["fov"],
                       cam_origin=g["cam_origin"], cam_rot=g["cam_rot"])
        else:
            src = load_frame(case) if case.startswith("aa_") else load_lighting(case)
        S, P, NL = src["spheres"].shape[1], src["planes"].shape[1], src["lights"].shape[1]
        table, sid, pid = _lens_materials(S, P)
        mats = (_glossy(table), sid, pid)
        radius = np.array([0.5, 0.0, 0.3][:NL], np.float32) if soft else np.zeros(NL, np.float32)
        rgb = np.array([[1.0, 0.7, 0.4], [0.3, 0.5, 1.5], [0.0, 0.3, 0.2]][:NL], np.float32)
        tex = _scene_textures(src) if case != "tiny" else None    # (tiny: a sky scene without textures)
        rg = raygen_closed_form(w, h, float(src["fov"]))
        refs = kernel_table_refs(oracle, src, w, h, modes, "sky", materials=mats, radius=radius, lens=(0.08 if lens else 0.0, 3.0),
                                 textures=tex, light_rgb=rgb, sky=SKY)
        first = plain = None
        for env in _VARIANTS[case]:
            for k in _VARIANT_KEYS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
            r = pkg.Renderer(0)
            try:
                r.set_camera(src["cam_origin"], src["cam_rot"])
                r.set_raygen(w, h, *rg)
                r.set_lens(0.08 if lens else 0.0, 3.0)
                if plain is None:                                 # the lighting twin: the same scene without a sky
                    r.set_scene(src["spheres"], src["lights"], src["planes"], materials=mats, light_radius=radius, shadow_samples=2,
                                textures=tex, light_rgb=rgb)
                    plain = r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, 0, u8=True, seed=3)[0]
                    names = KERNEL_LINE.findall(capfd.readouterr().err)
                    assert names and all(int(n[6]) == LIT_FAMILIES[kind] for n in names), (case, env, names)
                r.set_scene(src["spheres"], src["lights"], src["planes"], materials=mats, light_radius=radius, shadow_samples=2,
                            textures=tex, light_rgb=rgb, sky=SKY)
                outs = [r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, flags=flags, spp=spp, seed=3)
                        for aa, flags, spp in modes]
            finally:
                r.close()
            names = KERNEL_LINE.findall(capfd.readouterr().err)
            assert names and all(int(n[6]) == SKY_FAMILIES[kind] for n in names), (case, env, names)
            seen.update(names)
            for (aa, flags, _), (u8, f32), (r8, r32) in zip(modes, outs, refs):     # every kernel against the CPU oracle
                _same(f"{kind} {case} {env} aa={aa} flags={flags}", u8, f32, r8, r32)
            if first is None:
                first = outs
                assert all(u8.any() for u8, _ in outs)
                assert not np.array_equal(outs[0][0], plain), case      # (the sky shows)
                continue
            for (aa, flags, _), (u8, f32), (r8, r32) in zip(modes, outs, first):
                assert u8.tobytes() == r8.tobytes(), (case, env, aa, flags)
                assert f32.tobytes() == r32.tobytes(), (case, env, aa, flags)
    print(f"{kind}: {len(seen)} kernels: {sorted(seen)}")
    assert len(seen) == 14, f"{kind}: {len(seen)} of the family's 14 kernels ran: {sorted(seen)}"
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
    g = load_sky("everything_48_d4")
    _setup(rend, g)
    full8, full32 = _render_host(rend, g, aa=aa, spp=spp)
    for x0, x1 in ((9, 41), (33, 48)):
        u8, f32 = _render_host(rend, g, aa=aa, spp=spp, x0=x0, x1=x1)
        assert np.array_equal(u8, full8[:, x0:x1]) and np.array_equal(f32, full32[:, x0:x1]), (x0, x1)


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
    import subprocess
    from PIL import Image
    out = str(tmp_path / "sky.png")
    log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--size", "64x64", "--depth", "3",
                                   "--frames", "2", "--sky", "--out", out], text=True)
    assert "wrote" in log
    img = np.asarray(Image.open(out))
    assert img.shape == (64, 64, 3) and img[0].min() > 0 and img[0, :, 2].min() > 100     # blue all along the top row
