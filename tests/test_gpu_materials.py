"""Per-object materials on the GPU (rt_set_scene_materials): every materials_* fixture through every entry point, the
kernel variants the dispatcher picks (environment overrides, read at rt_create), uniform tables against the global path,
scene changes in flight and the error paths."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame, raygen_closed_form
from feature_gpu import (BIG, ENVS, ENVS_IDS, IGNORED, MODES, aim, check as _check, kw as _kw, large_fixtures_on_a_traversal,
                         render_host as _render_host, run_example, set_view, variant_source, walk_entry_points)
from test_materials import material_cases

pytestmark = pytest.mark.gpu


def _load(case):
    return np.load(os.path.join(GOLDEN, f"materials_{case}.npz"))


def _mats(g):
    return g["materials"], g["sphere_material"], g["plane_material"]


def _setup(r, g, explicit=False, materials=True):
    return set_view(r, g, lambda r, g: r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g) if materials else None),
                    explicit=explicit)


@pytest.mark.parametrize("case", material_cases())
def test_fixture_every_entry_point(renderer, case):
    walk_entry_points(renderer, _load(case), _setup, case in BIG, cameras=False, begin_end=False, explicit=case != BIG[1])


@pytest.mark.parametrize("lanes_mins, records", [("30", "1"), ("30", "0"), ("100000", "1"), ("100000", "0")])
def test_large_fixtures_on_every_traversal(monkeypatch, lanes_mins, records):
    """The 64- and 256-sphere fixtures (clustered scenes) on the lane-owned (MI355RT_LANES_MINS=30) and the wave-uniform
    (=100000) kernels, with and without float64 sphere records in LDS (MI355RT_F32_RECORDS)."""
    large_fixtures_on_a_traversal(monkeypatch, lanes_mins, records, _load, _setup)


@pytest.mark.parametrize("case", ["default_128_d3", "fov70_48", "tilted_planes_48", "inside_sphere_32", "aa_48_d2", "stoch_48_spp4"])
def test_uniform_table_is_the_global_path(renderer, case):
    """One material (amb, lamb, r) for every object, r in {1/2, 1/4, 0, 1}: the frame must be the global path's with the
    same scalars, byte for byte (uint8 and float32), whatever the launch's own scalars say."""
    g = load_frame(case)
    S, P = g["spheres"].shape[1], g["planes"].shape[1]
    amb, lamb = float(g["amb"]), float(g["lamb"])
    kw = _kw(g)
    for r_ in (0.5, 0.25, 0.0, 1.0):
        _setup(renderer, g, materials=False)
        ref8, ref32 = renderer.render(amb, lamb, r_, int(g["depth"]), int(g["aa"]), u8=True, f32=True, **kw)
        renderer.set_scene(g["spheres"], g["lights"], g["planes"],
                           materials=(np.array([[amb, lamb, r_]]), np.zeros(S, np.int32), np.zeros(P, np.int32)))
        u8, f32 = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), u8=True, f32=True, **kw)
        assert u8.tobytes() == ref8.tobytes(), (case, r_)
        assert f32.tobytes() == ref32.tobytes(), (case, r_)


def test_no_feedback_and_tile_stats_same_bytes(renderer):
    from python_ray_tracer_amd import _lib as L
    g = _load("default_64_d3")
    w, h = _setup(renderer, g)
    ref, _ = _render_host(renderer, g)
    u8, f32 = _render_host(renderer, g, flags=L.RT_FLAG_NO_FEEDBACK)
    _check(g, u8, f32, "RT_FLAG_NO_FEEDBACK")
    ntiles = ((w + 7) // 8) * ((h + 7) // 8)
    stats = renderer.malloc(4 * (ntiles + 64))
    d8 = renderer.malloc(3 * w * h)
    try:
        renderer.set_tile_stats(stats)
        p = renderer.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), 0)
        for _ in range(3):
            renderer.render_device(p, 0, w, d8, None, w * h)
        renderer.sync()
        got = np.empty((3, w, h), np.uint8)
        renderer.d2h(got, d8)
        assert np.array_equal(got, ref)
        cyc = np.empty(ntiles, np.uint32)
        renderer.d2h(cyc, stats)
        assert (cyc > 0).all()
    finally:
        renderer.set_tile_stats(None)
        renderer.free(stats); renderer.free(d8)


def test_scene_changes_in_flight(renderer, oracle):
    """Frames queued with table A on two streams, then table B set and more frames queued: every frame must be its own
    table's frame (the table travels in the launch's scene buffer)."""
    g = _load("default_64_d3")
    w, h = _setup(renderer, g)
    S, P = g["spheres"].shape[1], g["planes"].shape[1]
    B = (np.array([[0.05, 0.6, 0.5]]), np.zeros(S, np.int32), np.zeros(P, np.int32))
    refB = oracle.render(w, h, g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], 0.05, 0.6, 0.5, int(g["depth"]), False,
                         raygen=raygen_closed_form(w, h, float(g["fov"])), want=("u8",))["u8"]
    p = renderer.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), 0)
    streams = [renderer.stream_create() for _ in range(2)]
    bufs = [renderer.malloc(3 * w * h) for _ in range(8)]
    try:
        for i in range(4):
            renderer.render_device(p, 0, w, bufs[i], None, w * h, stream=streams[i % 2])
        renderer.set_scene(g["spheres"], g["lights"], g["planes"], materials=B)
        for i in range(4, 8):
            renderer.render_device(p, 0, w, bufs[i], None, w * h, stream=streams[i % 2])
        for s_ in streams:
            renderer.sync(s_)
        for i in range(8):
            got = np.empty((3, w, h), np.uint8)
            renderer.d2h(got, bufs[i])
            if i < 4:
                _check(g, got, None, f"frame {i} (table A)")
            else:
                assert np.array_equal(got, refB), f"frame {i} (table B)"
    finally:
        for s_ in streams:
            renderer.stream_destroy(s_)
        for b in bufs:
            renderer.free(b)


def test_errors_keep_the_previous_scene(renderer):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = _load("default_64_d3")
    _setup(renderer, g)
    table, sid, pid = _mats(g)
    M = table.shape[0]
    sp, li, pl = (np.ascontiguousarray(a, np.float32) for a in (g["spheres"], g["lights"], g["planes"]))
    bad = [
        (table, np.where(np.arange(len(sid)) == 2, M, sid).astype(np.int32), pid),       # id out of range
        (table, sid, np.full_like(pid, -1)),
        (np.zeros((L.RT_MAX_MATERIALS + 1, 3)), sid, pid),                               # M > RT_MAX_MATERIALS
        (np.where(np.arange(3 * M).reshape(M, 3) == 4, np.nan, table), sid, pid),        # NaN
        (np.where(np.arange(3 * M).reshape(M, 3) == 0, np.inf, table), sid, pid),
    ]
    for mats in bad:
        with pytest.raises(pkg.RenderError) as e:
            renderer.set_scene(sp, li, pl, materials=mats)
        assert e.value.status == L.RT_ERR_BAD_ARG
        u8, f32 = _render_host(renderer, g)
        _check(g, u8, f32, "after a refused scene")
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    t = np.ascontiguousarray(table)
    st = renderer._lib.rt_set_scene_materials(renderer._ctx, sp.ctypes.data_as(fp), sp.shape[1], li.ctypes.data_as(fp), li.shape[1],
                                              pl.ctypes.data_as(fp), pl.shape[1], 0, t.ctypes.data_as(C.POINTER(C.c_double)), M, None, None)
    assert st == L.RT_ERR_BAD_ARG                                 # NULL ids with M > 0
    st = renderer._lib.rt_set_scene_materials(renderer._ctx, sp.ctypes.data_as(fp), sp.shape[1], li.ctypes.data_as(fp), li.shape[1],
                                              pl.ctypes.data_as(fp), pl.shape[1], 0, None, M, None, None)
    assert st == L.RT_ERR_BAD_ARG                                 # NULL table with M > 0
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "after NULL arrays")
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels for material scenes
        _render_host(renderer, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "after a refused launch")


def test_example_with_materials_writes_png(tmp_path):
    """examples/render_png.py --materials: a mirror floor under matte spheres, through the Renderer API."""
    outs = {}
    for flag in ([], ["--materials"]):
        log, outs[bool(flag)] = run_example(str(tmp_path / f"r{len(flag)}.png"), "160x96", 2, 3, *flag)
        assert f"materials={bool(flag)}" in log
    assert outs[True].shape == (96, 160, 3) and outs[True].any() and not np.array_equal(outs[True], outs[False])


def test_begin_end_and_camera_sequence(renderer):
    """rt_render_begin / rt_render_end on two slots, and rt_render_sequence with a camera per frame, on a material scene."""
    g = _load("default_64_d3")
    w, h = _setup(renderer, g)
    outs = [(np.zeros((3, w, h), np.uint8), np.zeros((3, w, h), np.float32)) for _ in range(2)]
    for slot, (o8, o32) in enumerate(outs):
        renderer.render_begin(slot, IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), 0, o8, o32)
    for slot, (o8, o32) in enumerate(outs):
        renderer.render_end(slot)
        _check(g, o8, o32, f"rt_render_begin/end slot {slot}")
    n, npx = 3, w * h
    cams = np.tile(np.concatenate([np.asarray(g["cam_origin"], np.float64).ravel(), np.asarray(g["cam_rot"], np.float64).ravel()]), (n, 1))
    p = renderer.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), 0)
    d8 = renderer.malloc(n * 3 * npx)
    try:
        renderer.render_sequence(p, 0, w, n, d8, None, npx, 3 * npx, cams, None, 0)
        renderer.sync()
        seq = np.empty((n, 3, w, h), np.uint8)
        renderer.d2h(seq, d8)
        for i in range(n):
            _check(g, seq[i], None, f"rt_render_sequence with cameras, frame {i}")
    finally:
        renderer.free(d8)


def test_negative_ambient_keeps_the_sign_of_zero(renderer, oracle):
    """amb < 0 on a colour channel that is 0 (the magenta sphere's G): the reference's 0.0 + amb*col is +0.0, not -0.0.
    Depth 0 and no Lambert term, so the ambient term is the pixel; float32 compared bit for bit with the oracle."""
    g = load_frame("default_128_d3")
    w, h = _setup(renderer, g, materials=False)
    S, P = g["spheres"].shape[1], g["planes"].shape[1]
    renderer.set_scene(g["spheres"], g["lights"], g["planes"],
                       materials=(np.array([[-0.25, 0.0, 0.0]]), np.zeros(S, np.int32), np.zeros(P, np.int32)))
    _, f32 = renderer.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 0, 0, u8=True, f32=True)
    ref = oracle.render(w, h, g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], -0.25, 0.0, 0.0, 0, False,
                        raygen=raygen_closed_form(w, h, float(g["fov"])), want=("f32",))["f32"]
    assert ((f32 == 0) & ~np.signbit(f32) & (np.arange(3)[:, None, None] == 1)).sum() > 100    # magenta pixels, +0 in G
    assert not ((f32 == 0) & np.signbit(f32)).any()
    assert np.array_equal(f32.view(np.uint32), ref.view(np.uint32))


# Every material kernel (22 instantiations, rt_device.h MAT) is launched by one row of feature_gpu.ENVS.  A uniform power-of-two
# table must render the global path's bytes in each of them: plain, the AA lattice, per-pixel AA and stochastic.
@pytest.mark.parametrize("case, env", ENVS, ids=ENVS_IDS)
def test_every_material_kernel_is_the_global_path(monkeypatch, case, env):
    import python_ray_tracer_amd as pkg
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    src = variant_source(case, _load)
    S, P = src["spheres"].shape[1], src["planes"].shape[1]
    amb, lamb, refl = 0.05, 0.6, 0.5
    r = pkg.Renderer(0)
    try:
        aim(r, src, 160, 96)
        for aa, flags, spp in MODES:
            r.set_scene(src["spheres"], src["lights"], src["planes"])
            ref8, ref32 = r.render(amb, lamb, refl, 2, aa, u8=True, f32=True, flags=flags, spp=spp, seed=3)
            r.set_scene(src["spheres"], src["lights"], src["planes"],
                        materials=(np.array([[amb, lamb, refl]]), np.zeros(S, np.int32), np.zeros(P, np.int32)))
            u8, f32 = r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 2, aa, u8=True, f32=True, flags=flags, spp=spp, seed=3)
            assert u8.tobytes() == ref8.tobytes(), (aa, flags)
            assert f32.tobytes() == ref32.tobytes(), (aa, flags)
    finally:
        r.close()
