"""Lighting on the GPU (rt_set_scene_lighting, the lighting kernels): every lighting_* fixture through every entry point, all
56 lighting kernels through the dispatcher's environment overrides with the same bytes and the bytes of the CPU oracle's frames, fixtures against restated scenes (white
lights without a spec row, an unused spec row, doubled lights with lamb halved, a black light, a red light), frames in flight
across a scene change, column slabs, the error paths and the example."""
import ctypes as C

import numpy as np
import pytest

# The environment table and helpers are feature_gpu's, so that the lighting kernels are held to the same tables as their twins.
from feature_gpu import (BIG, IGNORED, KERNEL_LINE, LIT_FAMILIES, TEX_FAMILIES, check as _check, column_slabs_are_the_full_frame,
                         family_kernels_same_bytes, fixture_lens, frames as _frames, kw as _kw, lit_scene, render_host as _render_host,
                         run_example, same_frames as _same_frames, set_view, walk_entry_points)
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_lighting import CASES, fixture_textures, load_lighting

pytestmark = pytest.mark.gpu


def _mats(g, cols=8):
    return np.ascontiguousarray(g["materials"][:, :cols]), g["sphere_material"], g["plane_material"]


def _scene(r, g, materials=None, light_rgb="fixture", **kw):
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g) if materials is None else materials,
                light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]), textures=fixture_textures(g),
                light_rgb=g["light_rgb"] if isinstance(light_rgb, str) else light_rgb, **kw)


def _setup(r, g, explicit=False, **kw):
    return set_view(r, g, lambda r, g: _scene(r, g, **kw), lens=fixture_lens(g), explicit=explicit)


# ---------------------------------------------------------------------------------------------------------------------
# The fixtures (the reference's trace() restated with the two lighting terms, tools/gen_lighting_golden.py)

@pytest.mark.parametrize("case", CASES)
def test_fixture_every_entry_point(rend, case):
    g = load_lighting(case)
    walk_entry_points(rend, g, _setup, case in BIG, cameras=True, begin_end=True, explicit=case != BIG[1])
    _setup(rend, g, materials=_mats(g, 6), light_rgb=None)      # white lights, no spec column: the fixture's u8_plain
    u8, _ = _render_host(rend, g)
    _check(g, u8, None, "white lights and no spec", key="u8_plain")


# ---------------------------------------------------------------------------------------------------------------------
# One scene, the same bytes from every lighting kernel (feature_gpu.family_kernels_same_bytes): glossy rows and coloured lights
# against the same textured scene with neither.

@pytest.mark.parametrize("kind", list(LIT_FAMILIES))
def test_every_lighting_kernel_same_bytes(monkeypatch, capfd, oracle, kind):
    def scenes(src, case):
        matte, mats, tex, rgb = lit_scene(src, case)            # (tiny: a lit scene without textures)
        return dict(materials=matte, textures=tex), dict(materials=mats, textures=tex, light_rgb=rgb)
    family_kernels_same_bytes(monkeypatch, capfd, oracle, kind, LIT_FAMILIES, load_lighting, (64, 64), "lighting", scenes)


# ---------------------------------------------------------------------------------------------------------------------
# Fixtures against restated scenes

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
    column_slabs_are_the_full_frame(rend, load_lighting("everything_48_d4"), _setup, aa, spp, ((9, 41), (33, 48)))


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
    a, b = (run_example(str(tmp_path / f"{flag.strip('-')}.png"), "64x64", 3, 2, flag)[1] for flag in ("--glass", "--lights"))
    assert b.shape == (64, 64, 3) and b.any() and not np.array_equal(a, b)
