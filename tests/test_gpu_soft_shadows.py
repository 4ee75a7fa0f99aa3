"""Area lights on the GPU (rt_set_scene_area_lights, the area-light kernels): every soft_* fixture through every entry point,
the large fixtures on every traversal, all 22 area-light kernels through the dispatcher's environment overrides, an all-zero
radius against rt_set_scene_materials_scatter, column slabs, the seed, the error paths and the example."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame, raygen_closed_form
from test_soft_shadows import soft_cases

pytestmark = pytest.mark.gpu
IGNORED = dict(amb=7.0, lamb=-3.0, refl=2.0)   # rt_params shading scalars: a material scene must not read them
BIG = ("c4_s64_d5_sub32", "c5_s256_d8_sub96")


def _load(case):
    return np.load(os.path.join(GOLDEN, f"soft_{case}.npz"))


def _mats(g):
    return g["materials"], g["sphere_material"], g["plane_material"]


def _grid(w, h, rg):
    px, y0, dy, z0, dz = rg
    grid = np.empty((3, w, h))
    grid[0] = px
    grid[1] = (np.arange(w) * dy + y0)[:, None]
    grid[2] = (np.arange(h) * dz + z0)[None, :]
    return grid


def _set(r, g, **kw):
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=kw.pop("materials", _mats(g)),
                light_radius=kw.pop("light_radius", g["light_radius"]), shadow_samples=kw.pop("n", int(g["shadow_samples"])))


def _setup(r, g, explicit=False):
    w, h = int(g["w"]), int(g["h"])
    _set(r, g)
    r.set_camera(g["cam_origin"], g["cam_rot"])
    rg = raygen_closed_form(w, h, float(g["fov"]))
    if explicit:
        r.set_pixel_loc(_grid(w, h, rg))
    else:
        r.set_raygen(w, h, *rg)
    return w, h


def _kw(g):
    return dict(spp=int(g["spp"]) if "spp" in g else 0, seed=int(g["seed"]))


def _check(g, u8, f32=None, what="", x0=0):
    co = g["coords"]
    got = u8[:, co[:, 0] - x0, co[:, 1]].T
    assert np.array_equal(got, g["u8"]), f"{what}: {(got != g['u8']).any(axis=1).sum()} of {len(co)} pixels differ (uint8)"
    if f32 is not None:
        assert np.array_equal(f32[:, co[:, 0] - x0, co[:, 1]].T.view(np.uint32), g["rgb64"].astype(np.float32).view(np.uint32)), \
            f"{what}: float32 differs"


def _render_host(r, g, flags=0, aa=None, **kw):
    return r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]) if aa is None else aa, u8=True,
                    f32=True, flags=flags, **{**_kw(g), **kw})


@pytest.mark.parametrize("case", soft_cases())
def test_fixture_every_entry_point(renderer, case):
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
        renderer.h2d(d8, np.zeros(n * 3 * npx, np.uint8))
        renderer.render_sequence(p, 0, w, n, d8, d32, npx, 3 * npx, None, None, 2)
        renderer.sync()
        seq = np.empty((n, 3, w, h), np.uint8)
        renderer.d2h(seq, d8)
        s32 = None
        if d32 is not None:
            s32 = np.empty((n, 3, w, h), np.float32)
            renderer.d2h(s32, d32)
        for i in range(n):
            _check(g, seq[i], None if s32 is None else s32[i], f"rt_render_sequence frame {i}")
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


def test_rim_fixture_is_not_its_point_light_frame(renderer):
    """The rim case rendered with every radius 0 is the point-light frame the fixture records, not the soft one."""
    g = _load("rim_48_d2")
    _setup(renderer, g)
    _set(renderer, g, light_radius=np.zeros_like(g["light_radius"]))
    u8, _ = _render_host(renderer, g)
    co = g["coords"]
    assert np.array_equal(u8[:, co[:, 0], co[:, 1]].T, g["u8_point"])
    assert not np.array_equal(g["u8_point"], g["u8"])


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


# test_gpu_scatter.py's environment table: between them these launch every one of the 22 area-light kernels (rt_device.h
# SOFT).  The frames of one scene must be the same bytes in every variant.
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


def _soft_materials(S, P):
    """matte, mirror-ish, rough and glass spheres; a satin floor"""
    table = np.array([[0.05, 0.6, 0.5, 0.0, 1.0, 0.0], [0.0, 0.4, 0.8, 0.0, 1.0, 0.3], [0.02, 0.6, 0.2, 0.0, 1.0, 0.0],
                      [0.0, 0.5, 0.4, 0.0, 1.0, 0.1], [0.0, 0.1, 0.0, 0.9, 1.5, 0.0]])
    sid = np.array([(1 + (i // 3) % 2) if i % 3 == 0 else (4 if i % 5 == 0 else 0) for i in range(S)], np.int32)
    return table, sid, np.full(P, 3, np.int32)


@pytest.mark.parametrize("case", list(_VARIANTS))
def test_every_soft_kernel_same_bytes(monkeypatch, case):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    if case == "tiny":
        g = load_frame("aa_48_d2")
        src = dict(spheres=g["spheres"][:, :1], lights=g["lights"][:, :1], planes=g["planes"][:, :0], fov=g["fov"],
                   cam_origin=g["cam_origin"], cam_rot=g["cam_rot"])
    else:
        src = load_frame(case) if case.startswith("aa_") else _load(case)
    S, P, NL = src["spheres"].shape[1], src["planes"].shape[1], src["lights"].shape[1]
    mats = _soft_materials(S, P)
    radius = np.array([0.5, 0.0, 0.3][:NL], np.float32)
    radius[0] = 0.5
    w, h = 160, 96
    rg = raygen_closed_form(w, h, float(src["fov"]))
    modes = ((0, 0, 0), (1, 0, 0), (1, L.RT_FLAG_AA_PER_PIXEL, 0), (2, 0, 2))
    first = None
    for env in _VARIANTS[case]:
        for k in _ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = pkg.Renderer(0)
        try:
            r.set_camera(src["cam_origin"], src["cam_rot"])
            r.set_raygen(w, h, *rg)
            r.set_scene(src["spheres"], src["lights"], src["planes"], materials=mats, light_radius=radius, shadow_samples=3)
            outs = [r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, flags=flags, spp=spp, seed=3)
                    for aa, flags, spp in modes]
        finally:
            r.close()
        if first is None:
            first = outs
            assert all(u8.any() for u8, _ in outs)
            continue
        for (aa, flags, _), (u8, f32), (r8, r32) in zip(modes, outs, first):
            assert u8.tobytes() == r8.tobytes(), (env, aa, flags)
            assert f32.tobytes() == r32.tobytes(), (env, aa, flags)


@pytest.mark.parametrize("case", ["glass_rough_48_d4", "default_64_d4"])
def test_zero_radius_is_the_scatter_path(renderer, case):
    """Every radius 0: the bytes of rt_set_scene_materials_scatter, whatever shadow_samples is."""
    g = _load(case)
    _setup(renderer, g)
    zero = np.zeros_like(g["light_radius"])
    for aa, spp in ((0, 0), (1, 0), (2, 2)):
        renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g))
        ref8, ref32 = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 4, aa, u8=True, f32=True, spp=spp, seed=5)
        for n in (1, 4, 16):
            _set(renderer, g, light_radius=zero, n=n)
            u8, f32 = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 4, aa, u8=True, f32=True, spp=spp, seed=5)
            assert u8.tobytes() == ref8.tobytes() and f32.tobytes() == ref32.tobytes(), (aa, n)
    _set(renderer, g)                                              # and the area lights do differ from it
    u8, _ = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 4, 2, u8=True, f32=True, spp=2, seed=5)
    assert not np.array_equal(u8, ref8)


@pytest.mark.parametrize("aa, spp", [(0, 0), (1, 0), (2, 2)])
def test_column_slab_is_the_full_frame(renderer, aa, spp):
    """X is the absolute column: a slab [x0, x1) is the same columns of the whole frame."""
    g = _load("glass_rough_48_d4")
    w, h = _setup(renderer, g)
    full8, full32 = _render_host(renderer, g, aa=aa, spp=spp)
    for x0, x1 in ((9, 41), (33, 48)):
        u8, f32 = _render_host(renderer, g, aa=aa, spp=spp, x0=x0, x1=x1)
        assert np.array_equal(u8, full8[:, x0:x1]) and np.array_equal(f32, full32[:, x0:x1]), (x0, x1)


def test_seed_changes_only_pixels_that_see_a_light(renderer):
    """With a matte table (no rough row) and depth 0 the seed moves only the shadow sample points: it changes pixels whose hit
    point sees some light for some seed, never misses (the sky); the point-light scene does not depend on the seed at all."""
    g = _load("default_64_d4")
    _setup(renderer, g)
    table, sid, pid = _mats(g)
    seeds = (int(g["seed"]), 1, 2, 0xFFFFFFFF)

    def frame(t, seed):
        _set(renderer, g, materials=(t, sid, pid))
        return renderer.render(0.0, 0.0, 0.0, 0, 0, u8=True, f32=True, seed=seed)

    amb_only = np.array(table, copy=True)
    amb_only[:, 1] = 0.0
    hit_t = np.array(amb_only, copy=True)
    hit_t[:, 0] = 1.0
    _, base32 = frame(amb_only, 1)
    hit = (frame(hit_t, 1)[1] != 0).any(axis=0)                   # (every object has a colour)
    frames = [frame(table, s) for s in seeds]
    lit = np.zeros_like(hit)
    for _, f32 in frames:
        lit |= (f32 != base32).any(axis=0)
    assert lit.any() and (~lit).any()                             # (this view has no sky: the floor fills the background)
    changed = np.zeros_like(hit)
    for u8, f32 in frames[1:]:
        changed |= (u8 != frames[0][0]).any(axis=0)
        assert (f32[:, ~hit] == 0).all()
    assert changed.any() and not (changed & ~hit).any() and not (changed & ~lit).any()
    _set(renderer, g, light_radius=np.zeros_like(g["light_radius"]))
    pts = [renderer.render(0.0, 0.0, 0.0, 0, 0, u8=True, f32=True, seed=s)[1] for s in seeds]
    assert all(p.tobytes() == pts[0].tobytes() for p in pts)


def test_errors_keep_the_previous_scene(renderer):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = _load("default_64_d4")
    _setup(renderer, g)
    table, sid, pid = _mats(g)
    rad = g["light_radius"]
    sp, li, pl = (np.ascontiguousarray(a, np.float32) for a in (g["spheres"], g["lights"], g["planes"]))

    def rv(v, k=1):
        r = np.array(rad, copy=True)
        r[k] = v
        return r

    bad = [dict(light_radius=rv(-0.25)), dict(light_radius=rv(np.nan)), dict(light_radius=rv(np.inf)),
           dict(light_radius=rv(-np.inf)), dict(shadow_samples=0), dict(shadow_samples=17), dict(shadow_samples=-4),
           dict(materials=(np.where(np.arange(np.size(table)).reshape(np.shape(table)) == 2, np.nan, table), sid, pid))]
    for kw in bad:
        with pytest.raises(pkg.RenderError) as e:
            renderer.set_scene(sp, li, pl, **{**dict(materials=_mats(g), light_radius=rad, shadow_samples=4), **kw})
        assert e.value.status == L.RT_ERR_BAD_ARG, kw
        u8, f32 = _render_host(renderer, g)
        _check(g, u8, f32, f"after a refused scene {kw}")
    fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    t = np.ascontiguousarray(table)
    si, pi = np.ascontiguousarray(sid, np.int32), np.ascontiguousarray(pid, np.int32)
    r32 = np.ascontiguousarray(rad, np.float32)
    f = renderer._lib.rt_set_scene_area_lights
    args = (renderer._ctx, sp.ctypes.data_as(fp), sp.shape[1], li.ctypes.data_as(fp), li.shape[1], pl.ctypes.data_as(fp), pl.shape[1], 0)
    M, nc = t.shape[0], t.shape[1]
    assert f(*args, None, 0, 3, None, None, r32.ctypes.data_as(fp), 4) == L.RT_ERR_BAD_ARG              # M == 0 with a radius > 0
    assert f(*args, t.ctypes.data_as(dp), M, nc, si.ctypes.data_as(ip), pi.ctypes.data_as(ip), None, 4) == L.RT_ERR_BAD_ARG   # NULL radii
    assert f(*args, t.ctypes.data_as(dp), M, 4, si.ctypes.data_as(ip), pi.ctypes.data_as(ip), r32.ctypes.data_as(fp), 4) == L.RT_ERR_BAD_ARG
    assert f(None, *args[1:], t.ctypes.data_as(dp), M, nc, si.ctypes.data_as(ip), pi.ctypes.data_as(ip), r32.ctypes.data_as(fp), 4) \
        == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "after refused calls")
    # (radius 0 everywhere without a table is the plain scene: nothing to refuse)
    assert f(*args, None, 0, 3, None, None, np.zeros(li.shape[1], np.float32).ctypes.data_as(fp), 4) == L.RT_OK
    _setup(renderer, g)
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels for area-light scenes
        _render_host(renderer, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "after a refused launch")


def test_example_with_soft_lights_writes_png(tmp_path):
    """examples/render_png.py --soft --spp N: the default scene with lights of radius 0.5, through the Renderer API."""
    import subprocess
    import sys
    from PIL import Image
    from conftest import REPO
    outs = {}
    for flag in (["--materials"], ["--soft", "--spp", "4"]):
        out = str(tmp_path / f"{flag[0][2:]}.png")
        log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--size", "160x96", "--depth", "3",
                                       "--frames", "2", "--out", out] + flag, text=True)
        assert "wrote" in log
        outs[flag[0]] = np.asarray(Image.open(out))
    assert "soft=True" in log
    assert outs["--soft"].shape == (96, 160, 3) and outs["--soft"].any()
    assert not np.array_equal(outs["--soft"], outs["--materials"])
