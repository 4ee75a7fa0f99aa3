"""Depth of field on the GPU (rt_set_lens, the lens kernels): every lens_* fixture through every entry point, the large fixtures
on every traversal, all 44 lens kernels through the dispatcher's environment overrides, aperture 0 against the pinhole camera,
a lens closed again and a frame in flight keeping its lens, column slabs, the seed, the error paths and the example."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame, raygen_closed_form
from test_lens import lens_cases

pytestmark = pytest.mark.gpu
IGNORED = dict(amb=7.0, lamb=-3.0, refl=2.0)   # rt_params shading scalars: a material scene must not read them
BIG = ("c4_s64_d5_sub32", "c5_s256_d8_sub96")


@pytest.fixture
def rend(renderer):
    """The session's renderer, with the pinhole camera restored afterwards (later tests share it)."""
    yield renderer
    renderer.set_lens(0.0, 1.0)


def _load(case):
    return np.load(os.path.join(GOLDEN, f"lens_{case}.npz"))


def _mats(g):
    return g["materials"], g["sphere_material"], g["plane_material"]


def _grid(w, h, rg):
    px, y0, dy, z0, dz = rg
    grid = np.empty((3, w, h))
    grid[0] = px
    grid[1] = (np.arange(w) * dy + y0)[:, None]
    grid[2] = (np.arange(h) * dz + z0)[None, :]
    return grid


def _lens(g):
    return float(g["aperture"]), float(g["focus_distance"])


def _setup(r, g, explicit=False, lens=True):
    w, h = int(g["w"]), int(g["h"])
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g), light_radius=g["light_radius"],
                shadow_samples=int(g["shadow_samples"]))
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(*(_lens(g) if lens else (0.0, 1.0)))
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


@pytest.mark.parametrize("case", lens_cases())
def test_fixture_every_entry_point(rend, case):
    renderer = rend
    g = _load(case)
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
    _setup(renderer, g, lens=False)                             # the pinhole camera: the fixture's u8_pinhole
    u8, _ = _render_host(renderer, g)
    _check(g, u8, None, "aperture 0", key="u8_pinhole")


@pytest.mark.parametrize("lanes_mins, records", [("30", "1"), ("30", "0"), ("100000", "1"), ("100000", "0")])
def test_large_fixtures_on_every_traversal(monkeypatch, lanes_mins, records):
    import python_ray_tracer_amd as pkg
    monkeypatch.setenv("MI355RT_LANES_MINS", lanes_mins)
    monkeypatch.setenv("MI355RT_F32_RECORDS", records)
    r = pkg.Renderer(0)
    try:
        for case in BIG:
            g = _load(case)
            _setup(r, g)
            u8, f32 = _render_host(r, g)
            _check(g, u8, f32, f"{case} LANES_MINS={lanes_mins} F32_RECORDS={records}")
    finally:
        r.close()


# test_gpu_soft_shadows.py's environment table: between them these launch every one of the 22 lens kernels of each family
# (rt_device.h LENS: the scatter twins without a light radius, the area-light twins with one).  The frames of one scene must be
# the same bytes in every variant.
_VARIANTS = {
    "c5_s256_d8_sub96": [{}, {"MI355RT_LANES_PARK": "0"}, {"MI355RT_LANES_MINS": "100000"},
                         {"MI355RT_LANES_MINS": "100000", "MI355RT_F32_RECORDS": "0"},
                         {"MI355RT_LANES_MINS": "100000", "MI355RT_CLUSTER_MINS": "100000", "MI355RT_WPW2_MAX_IMAGE": "10000000"}],
    "c4_s64_d5_sub32": [{"MI355RT_LANES_MINS": "100000"}, {"MI355RT_LANES_MINS": "100000", "MI355RT_F32_RECORDS": "0"},
                        {"MI355RT_LANES_MINS": "30"},
                        {"MI355RT_LANES_MINS": "100000", "MI355RT_CLUSTER_MINS": "100000", "MI355RT_WPW2_MAX_IMAGE": "0"}],
    "aa_48_d2": [{}, {"MI355RT_WPW2_MAX_IMAGE": "0"}],
    "tiny": [{}],
}
_ENV_KEYS = sorted({k for vs in _VARIANTS.values() for v in vs for k in v})


def _lens_materials(S, P):
    """matte, mirror-ish, rough and glass spheres; a satin floor"""
    table = np.array([[0.05, 0.6, 0.5, 0.0, 1.0, 0.0], [0.0, 0.4, 0.8, 0.0, 1.0, 0.3], [0.02, 0.6, 0.2, 0.0, 1.0, 0.0],
                      [0.0, 0.5, 0.4, 0.0, 1.0, 0.1], [0.0, 0.1, 0.0, 0.9, 1.5, 0.0]])
    sid = np.array([(1 + (i // 3) % 2) if i % 3 == 0 else (4 if i % 5 == 0 else 0) for i in range(S)], np.int32)
    return table, sid, np.full(P, 3, np.int32)


@pytest.mark.parametrize("soft", [False, True], ids=["scatter", "area_lights"])
@pytest.mark.parametrize("case", list(_VARIANTS))
def test_every_lens_kernel_same_bytes(monkeypatch, case, soft):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    if case == "tiny":
        g = load_frame("aa_48_d2")
        src = dict(spheres=g["spheres"][:, :1], lights=g["lights"][:, :1], planes=g["planes"][:, :0], fov=g["fov"],
                   cam_origin=g["cam_origin"], cam_rot=g["cam_rot"])
    else:
        src = load_frame(case) if case.startswith("aa_") else _load(case)
    S, P, NL = src["spheres"].shape[1], src["planes"].shape[1], src["lights"].shape[1]
    mats = _lens_materials(S, P)
    radius = np.array([0.5, 0.0, 0.3][:NL], np.float32) if soft else np.zeros(NL, np.float32)
    w, h = 160, 96
    rg = raygen_closed_form(w, h, float(src["fov"]))
    modes = ((0, 0, 0), (1, 0, 0), (1, L.RT_FLAG_AA_PER_PIXEL, 0), (2, 0, 2))
    first = pin = None
    for env in _VARIANTS[case]:
        for k in _ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = pkg.Renderer(0)
        try:
            r.set_camera(src["cam_origin"], src["cam_rot"])
            r.set_raygen(w, h, *rg)
            r.set_scene(src["spheres"], src["lights"], src["planes"], materials=mats, light_radius=radius, shadow_samples=2)
            if pin is None:
                pin = r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, 0, u8=True, seed=3)[0]
            r.set_lens(0.08, 3.0)
            outs = [r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, flags=flags, spp=spp, seed=3)
                    for aa, flags, spp in modes]
        finally:
            r.close()
        if first is None:
            first = outs
            assert all(u8.any() for u8, _ in outs)
            assert not np.array_equal(outs[0][0], pin)        # (the lens kernels ran)
            continue
        for (aa, flags, _), (u8, f32), (r8, r32) in zip(modes, outs, first):
            assert u8.tobytes() == r8.tobytes(), (env, aa, flags)
            assert f32.tobytes() == r32.tobytes(), (env, aa, flags)


@pytest.mark.parametrize("kind", ["mat", "refr", "scat", "soft"])
def test_aperture_zero_is_the_pinhole(rend, kind):
    """Aperture 0: the bytes of the same scene without a lens, whatever the focus distance (a MAT, REFR, SCAT and SOFT table)."""
    g = _load("soft_glass_rough_48_d4")
    w, h = _setup(rend, g, lens=False)
    table, sid, pid = _mats(g)
    table = np.array(table)
    if kind == "mat":
        table = table[:, :3]
    elif kind == "refr":
        table = table[:, :5]
    elif kind == "scat":
        assert (table[:, 5] > 0).any()
    rad = g["light_radius"] if kind == "soft" else np.zeros_like(g["light_radius"])
    rend.set_scene(g["spheres"], g["lights"], g["planes"], materials=(table, sid, pid), light_radius=rad, shadow_samples=2)
    for aa, spp in ((0, 0), (1, 0), (2, 3)):
        rend.set_lens(0.0, 1.0)
        ref8, ref32 = rend.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, spp=spp, seed=5)
        for f in (0.5, 2.0, 1e6):
            rend.set_lens(0.0, f)
            u8, f32 = rend.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, spp=spp, seed=5)
            assert u8.tobytes() == ref8.tobytes() and f32.tobytes() == ref32.tobytes(), (aa, f)
        rend.set_lens(0.1, 2.0)                                   # and a lens does differ from it
        u8, _ = rend.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, spp=spp, seed=5)
        assert not np.array_equal(u8, ref8), aa


def test_lens_closed_again_and_a_frame_in_flight_keeps_its_lens(rend):
    g = _load("default_64_d4")
    w, h = _setup(rend, g)
    a, f = _lens(g)
    lens8, _ = _render_host(rend, g)
    _check(g, lens8, None, "lens")
    rend.set_lens(0.0, f)                                         # closed again: the pinhole frame
    u8, _ = _render_host(rend, g)
    _check(g, u8, None, "closed again", key="u8_pinhole")
    rend.set_lens(2 * a, 0.5 * f)
    other8, _ = _render_host(rend, g)
    assert not np.array_equal(other8, lens8)
    # launches queued on two streams, the lens changed between them: each frame keeps the lens it was launched with
    p = rend.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), **_kw(g))
    npx = w * h
    s1, s2 = rend.stream_create(), rend.stream_create()
    bufs = [rend.malloc(3 * npx) for _ in range(3)]
    try:
        rend.set_lens(a, f)
        rend.render_device(p, 0, w, bufs[0], None, npx, stream=s1)
        rend.set_lens(2 * a, 0.5 * f)
        rend.render_device(p, 0, w, bufs[1], None, npx, stream=s2)
        rend.set_lens(0.0, f)
        rend.render_device(p, 0, w, bufs[2], None, npx, stream=s1)
        rend.sync(s1)
        rend.sync(s2)
        got = [np.empty((3, w, h), np.uint8) for _ in range(3)]
        for o, b in zip(got, bufs):
            rend.d2h(o, b)
        _check(g, got[0], None, "in flight, lens")
        assert np.array_equal(got[1], other8), "in flight, the second lens"
        _check(g, got[2], None, "in flight, closed", key="u8_pinhole")
    finally:
        for b in bufs:
            rend.free(b)
        rend.stream_destroy(s1)
        rend.stream_destroy(s2)


@pytest.mark.parametrize("aa, spp", [(0, 0), (1, 0), (2, 2)])
def test_column_slab_is_the_full_frame(rend, aa, spp):
    """X is the absolute column: a slab [x0, x1) is the same columns of the whole frame."""
    g = _load("soft_glass_rough_48_d4")
    _setup(rend, g)
    full8, full32 = _render_host(rend, g, aa=aa, spp=spp)
    for x0, x1 in ((9, 41), (33, 48)):
        u8, f32 = _render_host(rend, g, aa=aa, spp=spp, x0=x0, x1=x1)
        assert np.array_equal(u8, full8[:, x0:x1]) and np.array_equal(f32, full32[:, x0:x1]), (x0, x1)


def test_seed_moves_the_lens_samples(rend):
    """A matte table (no rough row, no area light): only the lens samples depend on the seed.  The same seed gives the same
    bytes, different seeds different ones; without a lens the seed changes nothing."""
    g = _load("default_64_d4")
    _setup(rend, g)
    frames = {s: _render_host(rend, g, seed=s) for s in (1, 2, 0xFFFFFFFF)}
    again = _render_host(rend, g, seed=2)
    assert again[0].tobytes() == frames[2][0].tobytes() and again[1].tobytes() == frames[2][1].tobytes()
    assert not np.array_equal(frames[1][0], frames[2][0]) and not np.array_equal(frames[2][0], frames[0xFFFFFFFF][0])
    rend.set_lens(0.0, 1.0)
    pts = [_render_host(rend, g, seed=s)[1] for s in (1, 2, 0xFFFFFFFF)]
    assert all(p.tobytes() == pts[0].tobytes() for p in pts)


def test_errors(rend):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = _load("default_64_d4")
    _setup(rend, g)
    a, f = _lens(g)
    lib = rend._lib
    for bad in ((-0.1, f), (float("nan"), f), (float("inf"), f), (-float("inf"), f), (a, 0.0), (a, -1.0), (a, float("nan")),
                (a, float("inf"))):
        assert lib.rt_set_lens(rend._ctx, *bad) == L.RT_ERR_BAD_ARG, bad
        u8, f32 = _render_host(rend, g)                           # the previous lens stays
        _check(g, u8, f32, f"after a refused lens {bad}")
    assert lib.rt_set_lens(None, a, f) == L.RT_ERR_BAD_ARG
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels with a lens (nor for a material scene)
        _render_host(rend, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    # a lens on a scalar-only scene: refused at launch, with the lens still set; fine again without it
    rend.set_scene(g["spheres"], g["lights"], g["planes"])
    with pytest.raises(pkg.RenderError) as e:
        rend.render(0.0, 0.6, 0.3, 2, 0, u8=True)
    assert e.value.status == L.RT_ERR_STATE and "material table" in str(e.value)
    rend.set_lens(0.0, f)
    assert rend.render(0.0, 0.6, 0.3, 2, 0, u8=True)[0].any()
    _setup(rend, g)
    u8, f32 = _render_host(rend, g)
    _check(g, u8, f32, "after the refused launches")


def test_example_with_depth_of_field_writes_png(tmp_path):
    """examples/render_png.py --dof A --spp N: the default scene with materials through a thin lens focused on sphere 0."""
    import subprocess
    import sys
    from PIL import Image
    from conftest import REPO
    outs = {}
    for flag in (["--materials", "--spp", "4"], ["--dof", "0.1", "--spp", "4"], ["--dof", "0.1", "--spp", "4", "--focus-on-sphere", "3"]):
        out = str(tmp_path / f"{'_'.join(x.strip('-') for x in flag)}.png")
        log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--size", "160x96", "--depth", "3",
                                       "--frames", "2", "--out", out] + flag, text=True)
        assert "wrote" in log
        outs[" ".join(flag)] = np.asarray(Image.open(out))
    assert "dof=0.1" in log
    a, b, c = outs.values()
    assert b.shape == (96, 160, 3) and b.any()
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
