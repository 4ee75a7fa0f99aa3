"""Lighting on the GPU (rt_set_scene_lighting, the lighting kernels): every lighting_* fixture through every entry point, all
56 lighting kernels through the dispatcher's environment overrides with the same bytes and the bytes of the CPU oracle's frames, fixtures against restated scenes (white
lights without a spec row, an unused spec row, doubled lights with lamb halved, a black light, a red light), frames in flight
across a scene change, column slabs, the error paths and the example."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import REPO, load_frame, raygen_closed_form
# The environment table and helpers are those of the lens and texture tests, imported and not copied, so that the lighting
# kernels are held to the same tables as their twins.
from test_lighting import CASES, fixture_textures, load_lighting
from test_gpu_lens import _VARIANTS, _ENV_KEYS as _VARIANT_KEYS, _grid, _lens_materials
from test_gpu_textures import _scene_textures
from test_gpu_features_vs_oracle import _same
from test_gpu_lit_vs_oracle import kernel_table_refs

pytestmark = pytest.mark.gpu
IGNORED = dict(amb=7.0, lamb=-3.0, refl=2.0)   # rt_params shading scalars: a material scene must not read them
BIG = ("c4_s64_d5_sub32", "c5_s256_d8_sub96")
TEX_FAMILIES = {"scatter": 7, "area_lights": 8, "lens": 9, "both": 10}      # rt::Family numbers of the texture kernels
LIT_FAMILIES = {"scatter": 11, "area_lights": 12, "lens": 13, "both": 14}   # and of their lighting twins
KERNEL_LINE = re.compile(r"mi355rt: render_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), \(rt::Family\)(\d+)>")


@pytest.fixture
def rend(renderer):
    """The session's renderer, with the pinhole camera restored afterwards (later tests share it)."""
    yield renderer
    renderer.set_lens(0.0, 1.0)


def _mats(g, cols=8):
    return np.ascontiguousarray(g["materials"][:, :cols]), g["sphere_material"], g["plane_material"]


def _scene(r, g, materials=None, light_rgb="fixture", **kw):
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g) if materials is None else materials,
                light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]), textures=fixture_textures(g),
                light_rgb=g["light_rgb"] if isinstance(light_rgb, str) else light_rgb, **kw)


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


def _kw(g):
    return dict(spp=int(g["spp"]) if "spp" in g else 0, seed=int(g["seed"]))


def _pick(g, a, x0=0):
    co = g["coords"]
    return a[:, co[:, 0] - x0, co[:, 1]].T


def _check(g, u8, f32=None, what="", x0=0, key="u8"):
    got = _pick(g, u8, x0)
    assert np.array_equal(got, g[key]), f"{what}: {(got != g[key]).any(axis=1).sum()} of {len(got)} pixels differ (uint8)"
    if f32 is not None:
        a, e = _pick(g, f32, x0), g["rgb64"].astype(np.float32)
        bad = (a.view(np.uint32) != e.view(np.uint32)).any(axis=1)
        assert not bad.any(), (f"{what}: float32 differs at {bad.sum()} of {len(bad)} pixels, e.g. {g['coords'][bad][:4].tolist()}: "
                               f"{a[bad][:4].tolist()} != {e[bad][:4].tolist()}")


def _render_host(r, g, flags=0, aa=None, **kw):
    return r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]) if aa is None else aa, u8=True,
                    f32=True, flags=flags, **{**_kw(g), **kw})


# ---------------------------------------------------------------------------------------------------------------------
# The fixtures (the reference's trace() restated with the two lighting terms, tools/gen_lighting_golden.py)

@pytest.mark.parametrize("case", CASES)
def test_fixture_every_entry_point(rend, case):
    renderer = rend
    g = load_lighting(case)
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
    _setup(renderer, g, materials=_mats(g, 6), light_rgb=None)  # white lights, no spec column: the fixture's u8_plain
    u8, _ = _render_host(renderer, g)
    _check(g, u8, None, "white lights and no spec", key="u8_plain")


# ---------------------------------------------------------------------------------------------------------------------
# One scene, the same bytes from every lighting kernel.  test_gpu_lens.py's environment table x the four AA modes reaches all 14
# shapes of a family; MI355RT_LOG_KERNELS makes every launch name its kernel on stderr.

def _glossy(table):
    """The 6-column table with spec and shin columns: every row glossy, the exponents 1 .. 1024 in turn."""
    t = np.zeros((len(table), 8))
    t[:, :6] = table
    t[:, 6] = [40.0 + 30.0 * (i % 4) for i in range(len(table))]
    t[:, 7] = [float(1 << ((3 * i + 1) % 11)) for i in range(len(table))]
    return t


@pytest.mark.parametrize("kind", list(LIT_FAMILIES))
def test_every_lighting_kernel_same_bytes(monkeypatch, capfd, oracle, kind):
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
        tex = _scene_textures(src) if case != "tiny" else None    # (tiny: a lit scene without textures)
        rg = raygen_closed_form(w, h, float(src["fov"]))
        refs = kernel_table_refs(oracle, src, w, h, modes, "lighting", materials=mats, radius=radius, lens=(0.08 if lens else 0.0, 3.0),
                                 textures=tex, light_rgb=rgb)
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
                if plain is None:
                    r.set_scene(src["spheres"], src["lights"], src["planes"], materials=(table, sid, pid), light_radius=radius,
                                shadow_samples=2, textures=tex)
                    plain = r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, 0, u8=True, seed=3)[0]
                    capfd.readouterr()
                r.set_scene(src["spheres"], src["lights"], src["planes"], materials=mats, light_radius=radius, shadow_samples=2,
                            textures=tex, light_rgb=rgb)
                outs = [r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, flags=flags, spp=spp, seed=3)
                        for aa, flags, spp in modes]
            finally:
                r.close()
            names = KERNEL_LINE.findall(capfd.readouterr().err)
            assert names and all(int(n[6]) == LIT_FAMILIES[kind] for n in names), (case, env, names)
            seen.update(names)
            for (aa, flags, _), (u8, f32), (r8, r32) in zip(modes, outs, refs):     # every kernel against the CPU oracle
                _same(f"{kind} {case} {env} aa={aa} flags={flags}", u8, f32, r8, r32)
            if first is None:
                first = outs
                assert all(u8.any() for u8, _ in outs)
                assert not np.array_equal(outs[0][0], plain), case      # (the lighting shows)
                continue
            for (aa, flags, _), (u8, f32), (r8, r32) in zip(modes, outs, first):
                assert u8.tobytes() == r8.tobytes(), (case, env, aa, flags)
                assert f32.tobytes() == r32.tobytes(), (case, env, aa, flags)
    print(f"{kind}: {len(seen)} kernels: {sorted(seen)}")
    assert len(seen) == 14, f"{kind}: {len(seen)} of the family's 14 kernels ran: {sorted(seen)}"


# ---------------------------------------------------------------------------------------------------------------------
# Fixtures against restated scenes

def _frames(r, g):
    return [_render_host(r, g, aa=aa, spp=spp) for aa, spp in ((0, 0), (1, 0), (2, 2))]


def _same_frames(a, b, what):
    for i, ((u8, f32), (r8, r32)) in enumerate(zip(a, b)):
        assert u8.tobytes() == r8.tobytes() and f32.tobytes() == r32.tobytes(), (what, i)


@pytest.mark.parametrize("case", ["default_64_d4", "everything_48_d4"])
def test_white_lights_without_spec_is_rt_set_scene_textures(monkeypatch, capfd, case):
    """light_rgb NULL or all 1 with no spec row: the twin families and their bytes.  An unused row with spec > 0: the lighting
    kernels, and the twin's bytes."""
    import python_ray_tracer_amd as pkg
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    g = load_lighting(case)
    kind = "both" if case == "everything_48_d4" else "scatter"
    ones = np.ones((g["lights"].shape[1], 3), np.float32)
    m6 = _mats(g, 6)
    m8 = (np.concatenate([m6[0], np.tile([0.0, 64.0], (len(m6[0]), 1))], axis=1), m6[1], m6[2])
    unused = (np.concatenate([m8[0], [[0.1, 0.5, 0.2, 0.0, 1.0, 0.0, 90.0, 16.0]]]), m6[1], m6[2])
    r = pkg.Renderer(0)
    try:
        _setup(r, g, materials=m6, light_rgb=None)                # (no light_rgb and 6 columns: rt_set_scene_textures itself)
        ref = _frames(r, g)
        _check(g, ref[0][0], None, "the twin", key="u8_plain")
        capfd.readouterr()
        for what, mats, rgb in (("NULL, spec 0", m8, None), ("ones, 6 columns", m6, ones), ("ones, spec 0", m8, ones)):
            _scene(r, g, materials=mats, light_rgb=rgb)
            _same_frames(_frames(r, g), ref, what)
        names = KERNEL_LINE.findall(capfd.readouterr().err)
        assert len(names) >= 9 and all(int(n[6]) == TEX_FAMILIES[kind] for n in names), names
        _scene(r, g, materials=unused, light_rgb=None)
        _same_frames(_frames(r, g), ref, "an unused row with spec > 0")
        names = KERNEL_LINE.findall(capfd.readouterr().err)
        assert len(names) >= 3 and all(int(n[6]) == LIT_FAMILIES[kind] for n in names), names
    finally:
        r.close()


def test_doubled_lights_with_lamb_halved_is_the_white_frame(rend):
    """e = (2, 2, 2) and lamb / 2 (both exact): (k/2 * 2) * col = k * col."""
    g = load_lighting("grazing_48_d2")
    t, sid, pid = _mats(g, 6)
    _setup(rend, g, materials=(t, sid, pid), light_rgb=None)
    ref = _frames(rend, g)
    _check(g, ref[0][0], None, "white lights", key="u8_plain")
    half = t.copy()
    half[:, 1] *= 0.5
    _scene(rend, g, materials=(half, sid, pid), light_rgb=np.full((g["lights"].shape[1], 3), 2.0, np.float32))
    _same_frames(_frames(rend, g), ref, "e = 2, lamb / 2")


def test_a_black_light_is_no_light(rend):
    g = load_lighting("default_64_d4")
    _setup(rend, g)
    ref = _frames(rend, g)
    _check(g, ref[0][0], ref[0][1], "the fixture")
    lights = np.concatenate([g["lights"], np.array([[0.5], [0.3], [4.0]], np.float32)], axis=1)
    rend.set_scene(g["spheres"], lights, g["planes"], materials=_mats(g), light_radius=np.append(g["light_radius"], np.float32(0.0)),
                   shadow_samples=int(g["shadow_samples"]), textures=fixture_textures(g),
                   light_rgb=np.concatenate([g["light_rgb"], np.zeros((1, 3), np.float32)]))
    _same_frames(_frames(rend, g), ref, "a trailing light with e = (0, 0, 0)")


def test_a_red_light_lights_the_red_plane_only(rend):
    """e = (1, 0, 0): the red plane is the white-light frame's, the other two are ambient-only."""
    g = load_lighting("default_64_d4")
    m6 = _mats(g, 6)
    NL = g["lights"].shape[1]
    _setup(rend, g, materials=m6, light_rgb=None)
    white = _render_host(rend, g)[1]
    _scene(rend, g, materials=m6, light_rgb=np.tile(np.array([1.0, 0.0, 0.0], np.float32), (NL, 1)))
    red = _render_host(rend, g)[1]
    dark = m6[0].copy()
    dark[:, 1] = 0.0                                              # no Lambert term at all: ambient only
    _scene(rend, g, materials=(dark, m6[1], m6[2]), light_rgb=None)
    amb = _render_host(rend, g)[1]
    assert red[0].tobytes() == white[0].tobytes()
    assert red[1].tobytes() == amb[1].tobytes() and red[2].tobytes() == amb[2].tobytes()
    assert not np.array_equal(white[1], amb[1])


# ---------------------------------------------------------------------------------------------------------------------
# The ring, slabs, errors, the example

def test_frames_in_flight_keep_their_lights(rend):
    g = load_lighting("default_64_d4")
    w, h = _setup(rend, g)
    lit8, _ = _render_host(rend, g)
    _check(g, lit8, None, "lit")
    other_rgb = np.ascontiguousarray(g["light_rgb"][:, ::-1] * np.float32(1.5))
    _scene(rend, g, light_rgb=other_rgb)
    other8, _ = _render_host(rend, g)
    assert not np.array_equal(other8, lit8)
    p = rend.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), **_kw(g))
    npx = w * h
    s1, s2 = rend.stream_create(), rend.stream_create()
    bufs = [rend.malloc(3 * npx) for _ in range(6)]
    try:
        # six launches on two streams with a scene change before each: more changes than the ring has buffers
        kinds = ["lit", "other", "plain", "lit", "other", "lit"]
        for i, kind in enumerate(kinds):
            if kind == "plain":
                _scene(rend, g, materials=_mats(g, 6), light_rgb=None)
            else:
                _scene(rend, g, light_rgb=g["light_rgb"] if kind == "lit" else other_rgb)
            rend.render_device(p, 0, w, bufs[i], None, npx, stream=(s1, s2)[i % 2])
        rend.sync(s1)
        rend.sync(s2)
        for i, kind in enumerate(kinds):
            got = np.empty((3, w, h), np.uint8)
            rend.d2h(got, bufs[i])
            if kind == "other":
                assert np.array_equal(got, other8), f"launch {i}: the other lights"
            else:
                _check(g, got, None, f"launch {i} ({kind})", key="u8" if kind == "lit" else "u8_plain")
    finally:
        for b in bufs:
            rend.free(b)
        rend.stream_destroy(s1)
        rend.stream_destroy(s2)


@pytest.mark.parametrize("aa, spp", [(0, 0), (1, 0), (2, 2)])
def test_column_slab_is_the_full_frame(rend, aa, spp):
    g = load_lighting("everything_48_d4")
    _setup(rend, g)
    full8, full32 = _render_host(rend, g, aa=aa, spp=spp)
    for x0, x1 in ((9, 41), (33, 48)):
        u8, f32 = _render_host(rend, g, aa=aa, spp=spp, x0=x0, x1=x1)
        assert np.array_equal(u8, full8[:, x0:x1]) and np.array_equal(f32, full32[:, x0:x1]), (x0, x1)


def test_errors_leave_the_previous_scene(rend):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = load_lighting("default_64_d4")
    _setup(rend, g)
    nan, inf = float("nan"), float("inf")
    t, sid, pid = _mats(g)

    def rgb(i, c, v):
        a = np.array(g["light_rgb"], np.float32)
        a[i, c] = v
        return dict(light_rgb=a)

    def row(i, c, v):
        a = t.copy()
        a[i, c] = v
        return dict(materials=(a, sid, pid))

    cases = {"e negative": rgb(0, 1, -0.5), "e nan": rgb(1, 0, nan), "e inf": rgb(2, 2, inf),
             "spec negative": row(0, 6, -1.0), "spec nan": row(1, 6, nan), "spec inf": row(1, 6, inf),
             "shin 0": row(0, 7, 0.0), "shin 3": row(2, 7, 3.0), "shin 2048": row(1, 7, 2048.0), "shin 0.5": row(1, 7, 0.5),
             "shin nan": row(0, 7, nan), "shin -2": row(0, 7, -2.0),
             "rough > 1 in a row of 8": row(0, 5, 1.5), "ior 0 in a row of 8": row(0, 4, 0.0),
             "seven columns": dict(materials=(np.ascontiguousarray(t[:, :7]), sid, pid))}
    for what, kw in cases.items():
        with pytest.raises(pkg.RenderError) as e:
            _scene(rend, g, **kw)
        assert e.value.status == L.RT_ERR_BAD_ARG, what
        u8, f32 = _render_host(rend, g)                           # the previous scene stays current
        _check(g, u8, f32, f"after a refused scene ({what})")
    # through the C ABI: 8 columns are refused by the older entry points; lighting without a material table; NULL arrays
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    s, l, p = (np.ascontiguousarray(g[k], np.float32) for k in ("spheres", "lights", "planes"))
    t = np.ascontiguousarray(t, np.float64)
    si, pi = np.ascontiguousarray(sid, np.int32), np.ascontiguousarray(pid, np.int32)
    rad = np.ascontiguousarray(g["light_radius"], np.float32)
    e_ = np.ascontiguousarray(g["light_rgb"], np.float32)

    def call(fn="rt_set_scene_lighting", ctx=rend._ctx, M=t.shape[0], ncols=8, radius=rad.ctypes.data_as(fp), e=e_.ctypes.data_as(fp),
             last=True):
        args = [ctx, s.ctypes.data_as(fp), s.shape[1], l.ctypes.data_as(fp), l.shape[1], p.ctypes.data_as(fp), p.shape[1], 0,
                t.ctypes.data_as(C.POINTER(C.c_double)), M, ncols, si.ctypes.data_as(ip), pi.ctypes.data_as(ip), radius,
                int(g["shadow_samples"]), None, 0, None, None, None, 0]
        return getattr(rend._lib, fn)(*(args + ([e] if last else [])))

    for what, kw in {"ctx NULL": dict(ctx=None), "light_radius NULL": dict(radius=None), "M == 0": dict(M=0),
                     "ncols 7": dict(ncols=7), "ncols 8 through rt_set_scene_textures": dict(fn="rt_set_scene_textures", last=False)}.items():
        assert call(**kw) == L.RT_ERR_BAD_ARG, what
        u8, f32 = _render_host(rend, g)
        _check(g, u8, f32, f"after a refused scene ({what})")
    with pytest.raises(ValueError):                               # Python: light colours without a material table
        rend.set_scene(g["spheres"], g["lights"], g["planes"], light_rgb=g["light_rgb"])
    with pytest.raises(ValueError):                               # one colour too few
        _scene(rend, g, light_rgb=g["light_rgb"][:-1])
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels for a scene with materials
        _render_host(rend, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(rend, g)
    _check(g, u8, f32, "after the refused launch")
    # (the untextured fixture through the C ABI itself, NULL texture arrays: the lit frame)
    g2 = load_lighting("grazing_48_d2")
    _setup(rend, g2)
    u8, f32 = _render_host(rend, g2)
    _check(g2, u8, f32, "an untextured lit scene")


def test_example_with_lights_writes_png(tmp_path):
    """examples/render_png.py --lights: coloured lights and highlights."""
    import subprocess
    from PIL import Image
    outs = {}
    for flag in (["--glass"], ["--lights"]):
        out = str(tmp_path / f"{flag[0].strip('-')}.png")
        log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--size", "64x64", "--depth", "3",
                                       "--frames", "2", "--out", out] + flag, text=True)
        assert "wrote" in log
        outs[flag[0]] = np.asarray(Image.open(out))
    a, b = outs.values()
    assert b.shape == (64, 64, 3) and b.any() and not np.array_equal(a, b)
