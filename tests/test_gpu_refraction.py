"""Transparent materials on the GPU (rt_set_scene_materials_ex, the refraction kernels): every refraction_* fixture through
every entry point, the large fixtures on every traversal, all 22 refraction kernels through the dispatcher's environment
overrides, an all-opaque 5-column table against rt_set_scene_materials, a window check that does not use the generator,
the error paths, scene changes in flight and the example."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame, raygen_closed_form
from test_refraction import refraction_cases

pytestmark = pytest.mark.gpu
IGNORED = dict(amb=7.0, lamb=-3.0, refl=2.0)   # rt_params shading scalars: a material scene must not read them
BIG = ("c4_s64_d5_sub32", "c5_s256_d8_sub96")


def _load(case):
    return np.load(os.path.join(GOLDEN, f"refraction_{case}.npz"))


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
    return dict(spp=int(g["spp"]) if "spp" in g else 0, seed=int(g["seed"]) if "seed" in g else 1)


def _check(g, u8, f32=None, what=""):
    co = g["coords"]
    got = u8[:, co[:, 0], co[:, 1]].T
    assert np.array_equal(got, g["u8"]), f"{what}: {(got != g['u8']).any(axis=1).sum()} of {len(co)} pixels differ (uint8)"
    if f32 is not None:
        assert np.array_equal(f32[:, co[:, 0], co[:, 1]].T.view(np.uint32), g["rgb64"].astype(np.float32).view(np.uint32)), \
            f"{what}: float32 differs"


def _render_host(r, g, flags=0):
    return r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), u8=True, f32=True, flags=flags, **_kw(g))


@pytest.mark.parametrize("case", refraction_cases())
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
    """The 64- and 256-sphere fixtures (every third sphere glass) on the lane-owned and the wave-uniform kernels, with and
    without float64 sphere records in LDS: refracted rays start inside spheres, clusters and boxes."""
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


# The environment table of test_gpu_materials.py::test_every_material_kernel_is_the_global_path: between them these launch
# every one of the 22 refraction kernels (rt_device.h REFR).  With a glass table the frames of one scene must be the same
# bytes in every variant (there is no global path to compare with).
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


def _glass_materials(S, P):
    """every third sphere glass (ior 1.5 and 2.4 alternately), the others opaque; a mirror floor"""
    table = np.array([[0.05, 0.6, 0.5, 0.0, 1.0], [0.0, 0.1, 0.0, 0.9, 1.5], [0.02, 0.2, 0.0, 0.8, 2.4], [0.0, 0.3, 0.7, 0.0, 1.0]])
    sid = np.array([(1 + (i // 3) % 2) if i % 3 == 0 else 0 for i in range(S)], np.int32)
    return table, sid, np.full(P, 3, np.int32)


@pytest.mark.parametrize("case", list(_VARIANTS))
def test_every_refraction_kernel_same_bytes(monkeypatch, case):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    if case == "tiny":
        g = load_frame("aa_48_d2")
        src = dict(spheres=g["spheres"][:, :1], lights=g["lights"][:, :1], planes=g["planes"][:, :0], fov=g["fov"],
                   cam_origin=g["cam_origin"], cam_rot=g["cam_rot"])
    else:
        src = load_frame(case) if case.startswith("aa_") else _load(case)
    S, P = src["spheres"].shape[1], src["planes"].shape[1]
    mats = _glass_materials(S, P)
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


def test_opaque_five_column_table_is_the_material_path(renderer):
    """A 5-column table with every trans = 0 renders the bytes of rt_set_scene_materials on its first three columns."""
    g = _load("default_64_d4")
    w, h = _setup(renderer, g)
    t5 = np.array(g["materials"], copy=True)
    t5[:, 2] = np.where(t5[:, 3] > 0, 0.25, t5[:, 2])           # the glass rows become reflective ones
    t5[:, 3] = 0.0
    sid, pid = g["sphere_material"], g["plane_material"]
    for aa in (0, 1):
        renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=(np.ascontiguousarray(t5[:, :3]), sid, pid))
        ref8, ref32 = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 4, aa, u8=True, f32=True)
        renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=(t5, sid, pid))
        u8, f32 = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 4, aa, u8=True, f32=True)
        assert u8.tobytes() == ref8.tobytes() and f32.tobytes() == ref32.tobytes(), aa
    # and the glass table does differ from it
    _setup(renderer, g)
    u8, _ = _render_host(renderer, g)
    assert not np.array_equal(u8, ref8)


def test_window_is_transparent():
    """Independent of the generator: a window plane (trans = 1, amb = lamb = 0) between the camera and opaque, non-reflective
    spheres, the lights on the spheres' side, at depth 1 is the frame without the window at depth 0 (the bias shift of the
    continued ray leaves the last bits free: within one uint8 level in at least 99 % of the pixels).  The reference's shadow
    rays do not stop at the light (any hit with t < 999 occludes, trace.py:92-96), so the lights are far out on +x, beyond
    every visible point: no shadow ray, however long, turns towards the window."""
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd.scene import Camera
    g = load_frame("default_128_d3")
    sp = np.ascontiguousarray(g["spheres"][:, :3])               # the spheres at x >= 0.6 (the camera is at x = -2)
    li = np.array([[40.0, 40.0], [-10.0, 10.0], [20.0, 20.0]], np.float32)
    floor = np.ascontiguousarray(g["planes"], np.float32)
    window = np.array([[-1.0], [0.0], [0.0], [1.0], [0.0], [0.0], [200.0], [220.0], [255.0]], np.float32)
    w, h = 128, 96
    cam = Camera(resolution=(w, h), position=[-2, 0, 2.0], euler=[0, -30, 0])
    opaque = [0.05, 0.6, 0.0, 0.0, 1.0]
    with pkg.Renderer(0) as r:
        r.set_camera(cam.position, cam.rotation)
        r.set_raygen(w, h, *cam.raygen())
        r.set_scene(sp, li, floor, materials=(np.array([opaque]), np.zeros(3, np.int32), np.zeros(1, np.int32)))
        ref, _ = r.render(0.0, 0.0, 0.0, 0, 0, u8=True, f32=True)
        r.set_scene(sp, li, np.concatenate([floor, window], axis=1),
                    materials=(np.array([opaque, [0.0, 0.0, 0.0, 1.0, 1.5]]), np.zeros(3, np.int32), np.array([0, 1], np.int32)))
        got, _ = r.render(0.0, 0.0, 0.0, 1, 0, u8=True, f32=True)
        r.set_scene(sp, li, np.concatenate([floor, window], axis=1),
                    materials=(np.array([opaque, [0.0, 0.0, 0.0, 1.0, 1.5]]), np.zeros(3, np.int32), np.array([0, 1], np.int32)))
        at0, _ = r.render(0.0, 0.0, 0.0, 0, 0, u8=True, f32=True)
    assert ref.any() and (ref > 0).any(axis=0).mean() > 0.3
    assert not at0.any(), "at depth 0 the window (amb = lamb = 0) is all the camera sees"
    close = (np.abs(got.astype(int) - ref.astype(int)) <= 1).all(axis=0)
    assert close.mean() >= 0.99, close.mean()


def test_errors_keep_the_previous_scene(renderer):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = _load("default_64_d4")
    _setup(renderer, g)
    table, sid, pid = _mats(g)
    M = table.shape[0]
    sp, li, pl = (np.ascontiguousarray(a, np.float32) for a in (g["spheres"], g["lights"], g["planes"]))

    def col(c, v, row=0):
        t = np.array(table, copy=True)
        t[row, c] = v
        return t

    glass_row = int(np.nonzero(table[:, 3] > 0)[0][0])
    bad = [
        (table, np.where(np.arange(len(sid)) == 2, M, sid).astype(np.int32), pid),     # id out of range
        (table, sid, np.full_like(pid, -1)),
        (np.zeros((L.RT_MAX_MATERIALS + 1, 5)), sid, pid),                             # M > RT_MAX_MATERIALS
        (col(3, -0.5), sid, pid),                                                     # trans < 0
        (col(3, np.nan), sid, pid),
        (col(4, 0.0), sid, pid),                                                      # ior <= 0
        (col(4, -1.5), sid, pid),
        (col(4, np.inf), sid, pid),
        (col(0, np.nan), sid, pid),
        (col(2, 0.5, glass_row), sid, pid),                                           # trans > 0 with refl != 0
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
    f = renderer._lib.rt_set_scene_materials_ex
    args = (renderer._ctx, sp.ctypes.data_as(fp), sp.shape[1], li.ctypes.data_as(fp), li.shape[1], pl.ctypes.data_as(fp), pl.shape[1], 0)
    for ncols in (0, 4, 6, -5):
        assert f(*args, t.ctypes.data_as(dp), M, ncols, si.ctypes.data_as(ip), pi.ctypes.data_as(ip)) == L.RT_ERR_BAD_ARG
    assert f(*args, t.ctypes.data_as(dp), M, 5, None, None) == L.RT_ERR_BAD_ARG          # NULL ids
    assert f(*args, None, M, 5, si.ctypes.data_as(ip), pi.ctypes.data_as(ip)) == L.RT_ERR_BAD_ARG   # NULL table
    assert f(None, *args[1:], t.ctypes.data_as(dp), M, 5, si.ctypes.data_as(ip), pi.ctypes.data_as(ip)) == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "after refused calls")
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels for material scenes
        _render_host(renderer, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "after a refused launch")


def test_glass_and_opaque_scenes_in_flight(renderer):
    """Frames queued with a glass table, then an opaque 3-column table, then the glass table again, on two streams and in a
    sequence: every frame must be its own scene's frame (tables of both widths travel in the launch's scene buffer)."""
    g = _load("default_64_d4")
    w, h = _setup(renderer, g)
    S, P = g["spheres"].shape[1], g["planes"].shape[1]
    B = (np.array([[0.05, 0.6, 0.5]]), np.zeros(S, np.int32), np.zeros(P, np.int32))
    p = renderer.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), 0)
    renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=B)
    refB, _ = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), 0, u8=True, f32=True)
    _setup(renderer, g)
    streams = [renderer.stream_create() for _ in range(2)]
    n, npx = 2, w * h
    bufs = [renderer.malloc(3 * w * h) for _ in range(12)]
    seqs = [renderer.malloc(n * 3 * npx) for _ in range(3)]
    try:
        for i in range(4):
            renderer.render_device(p, 0, w, bufs[i], None, npx, stream=streams[i % 2])
        renderer.render_sequence(p, 0, w, n, seqs[0], None, npx, 3 * npx, None, [streams[0]], 0)
        renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=B)
        for i in range(4, 8):
            renderer.render_device(p, 0, w, bufs[i], None, npx, stream=streams[i % 2])
        renderer.render_sequence(p, 0, w, n, seqs[1], None, npx, 3 * npx, None, [streams[1]], 0)
        renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g))
        for i in range(8, 12):
            renderer.render_device(p, 0, w, bufs[i], None, npx, stream=streams[i % 2])
        renderer.render_sequence(p, 0, w, n, seqs[2], None, npx, 3 * npx, None, [streams[0]], 0)
        for s_ in streams:
            renderer.sync(s_)
        renderer.sync()
        for i in range(12):
            got = np.empty((3, w, h), np.uint8)
            renderer.d2h(got, bufs[i])
            if 4 <= i < 8:
                assert np.array_equal(got, refB), f"frame {i} (opaque table)"
            else:
                _check(g, got, None, f"frame {i} (glass table)")
        for j in range(3):
            seq = np.empty((n, 3, w, h), np.uint8)
            renderer.d2h(seq, seqs[j])
            for i in range(n):
                if j == 1:
                    assert np.array_equal(seq[i], refB), f"sequence {j} frame {i} (opaque table)"
                else:
                    _check(g, seq[i], None, f"sequence {j} frame {i} (glass table)")
    finally:
        for s_ in streams:
            renderer.stream_destroy(s_)
        for b in bufs + seqs:
            renderer.free(b)


def test_example_with_glass_writes_png(tmp_path):
    """examples/render_png.py --glass: two glass spheres over the mirror floor, through the Renderer API."""
    import subprocess
    import sys
    from PIL import Image
    from conftest import REPO
    outs = {}
    for flag in (["--materials"], ["--glass"]):
        out = str(tmp_path / f"{flag[0][2:]}.png")
        log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--size", "160x96", "--depth", "3",
                                       "--frames", "3", "--out", out] + flag, text=True)
        assert "wrote" in log
        outs[flag[0]] = np.asarray(Image.open(out))
    assert "glass=True" in log
    assert outs["--glass"].shape == (96, 160, 3) and outs["--glass"].any()
    assert not np.array_equal(outs["--glass"], outs["--materials"])
