"""Rough materials on the GPU (rt_set_scene_materials_scatter, the scatter kernels): every scatter_* fixture through every
entry point, the large fixtures on every traversal, all 22 scatter kernels through the dispatcher's environment overrides, an
all-smooth 6-column table against rt_set_scene_materials_ex, column slabs, the seed, the error paths and the example."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame, raygen_closed_form
from test_scatter import scatter_cases

pytestmark = pytest.mark.gpu
IGNORED = dict(amb=7.0, lamb=-3.0, refl=2.0)   # rt_params shading scalars: a material scene must not read them
BIG = ("c4_s64_d5_sub32", "c5_s256_d8_sub96")


def _load(case):
    return np.load(os.path.join(GOLDEN, f"scatter_{case}.npz"))


def _mats(g):
    return g["materials"], g["sphere_material"], g["plane_material"]


def _grid(w, h, rg):
    px, y0, dy, z0, dz = rg
    grid = np.empty((3, w, h))
    grid[0] = px
    grid[1] = (np.arange(w) * dy + y0)[:, None]
    grid[2] = (np.arange(h) * dz + z0)[None, :]
    return grid


def _setup(r, g, explicit=False):
    w, h = int(g["w"]), int(g["h"])
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g))
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


def test_fixtures_have_events():
    assert set(scatter_cases()) >= {"default_64_d4", "aa_48_d2", "stoch_40x24_spp3_seed7", "grazing_48_d3", "inside_32_d4", *BIG}


@pytest.mark.parametrize("case", scatter_cases())
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


# test_gpu_refraction.py's environment table: between them these launch every one of the 22 scatter kernels (rt_device.h
# SCAT).  The frames of one scene must be the same bytes in every variant.
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


def _rough_materials(S, P):
    """every third sphere rough (0.3 and 1.0 alternately), one in five of the others glass; a satin floor"""
    table = np.array([[0.05, 0.6, 0.5, 0.0, 1.0, 0.0], [0.0, 0.4, 0.8, 0.0, 1.0, 0.3], [0.02, 0.2, 0.9, 0.0, 1.0, 1.0],
                      [0.0, 0.3, 0.7, 0.0, 1.0, 0.1], [0.0, 0.1, 0.0, 0.9, 1.5, 0.0]])
    sid = np.array([(1 + (i // 3) % 2) if i % 3 == 0 else (4 if i % 5 == 0 else 0) for i in range(S)], np.int32)
    return table, sid, np.full(P, 3, np.int32)


@pytest.mark.parametrize("case", list(_VARIANTS))
def test_every_scatter_kernel_same_bytes(monkeypatch, case):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    if case == "tiny":
        g = load_frame("aa_48_d2")
        src = dict(spheres=g["spheres"][:, :1], lights=g["lights"][:, :1], planes=g["planes"][:, :0], fov=g["fov"],
                   cam_origin=g["cam_origin"], cam_rot=g["cam_rot"])
    else:
        src = load_frame(case) if case.startswith("aa_") else _load(case)
    S, P = src["spheres"].shape[1], src["planes"].shape[1]
    mats = _rough_materials(S, P)
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
            r.set_scene(src["spheres"], src["lights"], src["planes"], materials=mats)
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


def test_smooth_six_column_table_is_the_refraction_path(renderer):
    """A 6-column table with every rough = 0 renders the bytes of rt_set_scene_materials_ex on its first five columns."""
    g = _load("default_64_d4")
    _setup(renderer, g)
    t6 = np.array(g["materials"], copy=True)
    t6[:, 5] = 0.0
    sid, pid = g["sphere_material"], g["plane_material"]
    for aa, spp in ((0, 0), (1, 0), (2, 2)):
        renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=(np.ascontiguousarray(t6[:, :5]), sid, pid))
        ref8, ref32 = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 4, aa, u8=True, f32=True, spp=spp, seed=5)
        renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=(t6, sid, pid))
        u8, f32 = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 4, aa, u8=True, f32=True, spp=spp, seed=5)
        assert u8.tobytes() == ref8.tobytes() and f32.tobytes() == ref32.tobytes(), aa
    _setup(renderer, g)                                           # and the rough table does differ from it
    u8, _ = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 4, 2, u8=True, f32=True, spp=2, seed=5)
    assert not np.array_equal(u8, ref8)


@pytest.mark.parametrize("aa, spp", [(0, 0), (1, 0), (2, 2)])
def test_column_slab_is_the_full_frame(renderer, aa, spp):
    """X is the absolute column: a slab [x0, x1) is the same columns of the whole frame."""
    g = _load("default_64_d4")
    w, h = _setup(renderer, g)
    full8, full32 = _render_host(renderer, g, aa=aa, spp=spp)
    for x0, x1 in ((9, 41), (33, 64)):
        u8, f32 = _render_host(renderer, g, aa=aa, spp=spp, x0=x0, x1=x1)
        assert np.array_equal(u8, full8[:, x0:x1]) and np.array_equal(f32, full32[:, x0:x1]), (x0, x1)


def test_seed_changes_only_pixels_that_hit_rough_surfaces(renderer):
    """Pixels whose (mirror) path meets no rough surface in traces 0..depth-1 are the smooth table's pixels for every seed.
    The mask of the others is rendered with the same geometry: amb 1 on the rough rows, 0 elsewhere, lamb 0, every opaque
    refl 1 (the weights do not move a ray) and depth - 1."""
    g = _load("default_64_d4")
    _setup(renderer, g)
    table, sid, pid = _mats(g)
    depth = int(g["depth"])
    smooth = np.array(table, copy=True)
    smooth[:, 5] = 0.0
    renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=(smooth, sid, pid))
    ref, _ = _render_host(renderer, g)
    mask_t = np.array(smooth, copy=True)
    mask_t[:, 0] = (table[:, 5] > 0).astype(np.float64)
    mask_t[:, 1] = 0.0
    mask_t[:, 2] = np.where(table[:, 3] > 0, 0.0, 1.0)
    renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=(mask_t, sid, pid))
    _, m32 = renderer.render(0.0, 0.0, 0.0, depth - 1, 0, u8=True, f32=True)
    rough_px = (m32 > 0).any(axis=0)
    assert 0.2 < rough_px.mean() < 1.0
    renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=(table, sid, pid))
    frames = [_render_host(renderer, g, seed=s)[0] for s in (int(g["seed"]), 1, 2, 0xFFFFFFFF)]
    for f in frames:
        assert np.array_equal(f[:, ~rough_px], ref[:, ~rough_px])
    changed = np.zeros_like(rough_px)
    for f in frames[1:]:
        changed |= (f != frames[0]).any(axis=0)
    assert changed.any() and not (changed & ~rough_px).any()
    assert changed.sum() > 0.3 * rough_px.sum()


def test_errors_keep_the_previous_scene(renderer):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = _load("default_64_d4")
    _setup(renderer, g)
    table, sid, pid = _mats(g)
    M = table.shape[0]
    sp, li, pl = (np.ascontiguousarray(a, np.float32) for a in (g["spheres"], g["lights"], g["planes"]))

    def col(c, v, row=1):
        t = np.array(table, copy=True)
        t[row, c] = v
        return t

    glass_row = int(np.nonzero(table[:, 3] > 0)[0][0])
    bad = [
        (col(5, -0.25), sid, pid),                                                    # rough < 0
        (col(5, 1.5), sid, pid),                                                      # rough > 1
        (col(5, np.nan), sid, pid),
        (col(5, np.inf), sid, pid),
        (col(5, 0.5, glass_row), sid, pid),                                           # a rough transparent row
        (col(3, -0.5), sid, pid),                                                     # the rules of 5 columns still hold
        (col(4, 0.0), sid, pid),
        (np.zeros((M, 4)), sid, pid),                                                 # ncols 4 and 7 (Renderer passes the width)
        (np.zeros((M, 7)), sid, pid),
        (table, np.where(np.arange(len(sid)) == 2, M, sid).astype(np.int32), pid),     # id out of range
        (np.zeros((L.RT_MAX_MATERIALS + 1, 6)), sid, pid),
    ]
    for mats in bad:
        with pytest.raises(pkg.RenderError) as e:
            renderer.set_scene(sp, li, pl, materials=mats)
        assert e.value.status == L.RT_ERR_BAD_ARG
        u8, f32 = _render_host(renderer, g)
        _check(g, u8, f32, "after a refused scene")
    fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    t = np.ascontiguousarray(table)
    si, pi = np.ascontiguousarray(sid, np.int32), np.ascontiguousarray(pid, np.int32)
    f = renderer._lib.rt_set_scene_materials_scatter
    args = (renderer._ctx, sp.ctypes.data_as(fp), sp.shape[1], li.ctypes.data_as(fp), li.shape[1], pl.ctypes.data_as(fp), pl.shape[1], 0)
    for ncols in (0, 4, 7, -6):
        assert f(*args, t.ctypes.data_as(dp), M, ncols, si.ctypes.data_as(ip), pi.ctypes.data_as(ip)) == L.RT_ERR_BAD_ARG
    assert f(*args, t.ctypes.data_as(dp), M, 6, None, None) == L.RT_ERR_BAD_ARG          # NULL ids
    assert f(*args, None, M, 6, si.ctypes.data_as(ip), pi.ctypes.data_as(ip)) == L.RT_ERR_BAD_ARG   # NULL table
    assert f(None, *args[1:], t.ctypes.data_as(dp), M, 6, si.ctypes.data_as(ip), pi.ctypes.data_as(ip)) == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "after refused calls")
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels for material scenes
        _render_host(renderer, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "after a refused launch")


def test_example_with_scatter_writes_png(tmp_path):
    """examples/render_png.py --scatter --spp N: brushed spheres and a satin floor, through the Renderer API."""
    import subprocess
    import sys
    from PIL import Image
    from conftest import REPO
    outs = {}
    for flag in (["--materials"], ["--scatter", "--spp", "4"]):
        out = str(tmp_path / f"{flag[0][2:]}.png")
        log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--size", "160x96", "--depth", "3",
                                       "--frames", "2", "--out", out] + flag, text=True)
        assert "wrote" in log
        outs[flag[0]] = np.asarray(Image.open(out))
    assert "scatter=True" in log
    assert outs["--scatter"].shape == (96, 160, 3) and outs["--scatter"].any()
    assert not np.array_equal(outs["--scatter"], outs["--materials"])
