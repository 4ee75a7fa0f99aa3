"""Transparent materials on the GPU (rt_set_scene_materials_ex, the refraction kernels): every refraction_* fixture through
every entry point, the large fixtures on every traversal, all 22 refraction kernels through the dispatcher's environment
overrides, an all-opaque 5-column table against rt_set_scene_materials, a window check that does not use the generator,
the error paths, scene changes in flight and the example."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame
from feature_gpu import (BIG, IGNORED, VARIANTS, aim, check as _check, large_fixtures_on_a_traversal, render_host as _render_host,
                         render_modes, run_example, same_as_first, set_view, variant_renderers, variant_source, walk_entry_points)
from test_refraction import refraction_cases

pytestmark = pytest.mark.gpu


def _load(case):
    return np.load(os.path.join(GOLDEN, f"refraction_{case}.npz"))


def _mats(g):
    return g["materials"], g["sphere_material"], g["plane_material"]


def _setup(r, g, explicit=False):
    return set_view(r, g, lambda r, g: r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g)), explicit=explicit)


@pytest.mark.parametrize("case", refraction_cases())
def test_fixture_every_entry_point(renderer, case):
    walk_entry_points(renderer, _load(case), _setup, case in BIG, cameras=False, begin_end=False, explicit=case != BIG[1])


@pytest.mark.parametrize("lanes_mins, records", [("30", "1"), ("30", "0"), ("100000", "1"), ("100000", "0")])
def test_large_fixtures_on_every_traversal(monkeypatch, lanes_mins, records):
    """The 64- and 256-sphere fixtures (every third sphere glass) on the lane-owned and the wave-uniform kernels, with and
    without float64 sphere records in LDS: refracted rays start inside spheres, clusters and boxes."""
    large_fixtures_on_a_traversal(monkeypatch, lanes_mins, records, _load, _setup)


def _glass_materials(S, P):
    """every third sphere glass (ior 1.5 and 2.4 alternately), the others opaque; a mirror floor"""
    table = np.array([[0.05, 0.6, 0.5, 0.0, 1.0], [0.0, 0.1, 0.0, 0.9, 1.5], [0.02, 0.2, 0.0, 0.8, 2.4], [0.0, 0.3, 0.7, 0.0, 1.0]])
    sid = np.array([(1 + (i // 3) % 2) if i % 3 == 0 else 0 for i in range(S)], np.int32)
    return table, sid, np.full(P, 3, np.int32)


@pytest.mark.parametrize("case", list(VARIANTS))
def test_every_refraction_kernel_same_bytes(monkeypatch, case):
    """feature_gpu.VARIANTS launches every one of the 22 refraction kernels (rt_device.h REFR).  With a glass table the frames of
    one scene must be the same bytes in every variant (there is no global path to compare with)."""
    src = variant_source(case, _load)
    mats = _glass_materials(src["spheres"].shape[1], src["planes"].shape[1])
    first = None
    for env, r in variant_renderers(monkeypatch, case):
        aim(r, src, 160, 96)
        r.set_scene(src["spheres"], src["lights"], src["planes"], materials=mats)
        first = same_as_first(first, render_modes(r), env)


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
    outs = {}
    for flag in (["--materials"], ["--glass"]):
        log, outs[flag[0]] = run_example(str(tmp_path / f"{flag[0][2:]}.png"), "160x96", 3, 3, *flag)
    assert "glass=True" in log
    assert outs["--glass"].shape == (96, 160, 3) and outs["--glass"].any()
    assert not np.array_equal(outs["--glass"], outs["--materials"])
