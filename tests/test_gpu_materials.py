"""Per-object materials on the GPU (rt_set_scene_materials): every materials_* fixture through every entry point, the
kernel variants the dispatcher picks (environment overrides, read at rt_create), uniform tables against the global path,
scene changes in flight and the error paths."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame, raygen_closed_form
from test_materials import material_cases

pytestmark = pytest.mark.gpu
IGNORED = dict(amb=7.0, lamb=-3.0, refl=2.0)   # rt_params shading scalars: a material scene must not read them


def _load(case):
    return np.load(os.path.join(GOLDEN, f"materials_{case}.npz"))


def _mats(g):
    return g["materials"], g["sphere_material"], g["plane_material"]


def _grid(w, h, rg):
    px, y0, dy, z0, dz = rg
    grid = np.empty((3, w, h))
    grid[0] = px
    grid[1] = (np.arange(w) * dy + y0)[:, None]
    grid[2] = (np.arange(h) * dz + z0)[None, :]
    return grid


def _setup(r, g, explicit=False, materials=True):
    w, h = int(g["w"]), int(g["h"])
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g) if materials else None)
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
        # bit for bit, the sign of zero included (the reference's ambient term is 0.0 + amb*col)
        assert np.array_equal(f32[:, co[:, 0], co[:, 1]].T.view(np.uint32), g["rgb64"].astype(np.float32).view(np.uint32)), \
            f"{what}: float32 differs"


def _render_host(r, g, flags=0):
    return r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), u8=True, f32=True, flags=flags, **_kw(g))


BIG = ("c4_s64_d5_sub32", "c5_s256_d8_sub96")


@pytest.mark.parametrize("case", material_cases())
def test_fixture_every_entry_point(renderer, case):
    g = _load(case)
    w, h = _setup(renderer, g)
    u8, f32 = _render_host(renderer, g)
    _check(g, u8, f32, "rt_render")
    # rt_render_device and rt_render_sequence (n = 3, every frame) into device buffers; float32 too for the small frames
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
    """The 64- and 256-sphere fixtures (clustered scenes) on the lane-owned (MI355RT_LANES_MINS=30) and the wave-uniform
    (=100000) kernels, with and without float64 sphere records in LDS (MI355RT_F32_RECORDS)."""
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
    import subprocess
    import sys
    from PIL import Image
    from conftest import REPO
    outs = {}
    for flag in ([], ["--materials"]):
        out = str(tmp_path / f"r{len(flag)}.png")
        log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--size", "160x96", "--depth", "2",
                                       "--frames", "3", "--out", out] + flag, text=True)
        assert "wrote" in log and f"materials={bool(flag)}" in log
        outs[bool(flag)] = np.asarray(Image.open(out))
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


# Every material kernel (22 instantiations, rt_device.h MAT) is launched by one of these: the dispatcher's choice follows the
# scene (flat or clustered, sphere count, LDS image) and the overrides read at rt_create.  A uniform power-of-two table must
# render the global path's bytes in each of them: plain, the AA lattice, per-pixel AA and stochastic.
_VARIANTS = [
    ("c5_s256_d8_sub96", {}),                                                 # lane-owned, parked (MODE 2 / 3)
    ("c5_s256_d8_sub96", {"MI355RT_LANES_PARK": "0"}),                        # lane-owned, registers
    ("c4_s64_d5_sub32", {"MI355RT_LANES_MINS": "100000"}),                    # wave-uniform clusters, 4 waves, parked (MODE 1)
    ("c4_s64_d5_sub32", {"MI355RT_LANES_MINS": "100000", "MI355RT_F32_RECORDS": "0"}),   # ... MODE 0
    ("c5_s256_d8_sub96", {"MI355RT_LANES_MINS": "100000"}),                   # 4 waves, registers (MODE 1)
    ("c5_s256_d8_sub96", {"MI355RT_LANES_MINS": "100000", "MI355RT_F32_RECORDS": "0"}),  # ... MODE 0
    ("aa_48_d2", {}),                                                         # flat, 2 waves, parked (AA: registers)
    ("tiny", {}),                                                             # one sphere, one light: 2 waves, parked AA too
    ("aa_48_d2", {"MI355RT_WPW2_MAX_IMAGE": "0"}),                            # flat, 4 waves, parked (MODE 0)
    ("c4_s64_d5_sub32", {"MI355RT_LANES_MINS": "30"}),                        # lane-owned on a small image: parked (MODE 2 / 3)
    ("c4_s64_d5_sub32", {"MI355RT_LANES_MINS": "100000", "MI355RT_CLUSTER_MINS": "100000",
                         "MI355RT_WPW2_MAX_IMAGE": "0"}),                     # flat 64 spheres, 4 waves (MODE 1 where it saves LDS)
    ("c5_s256_d8_sub96", {"MI355RT_LANES_MINS": "100000", "MI355RT_CLUSTER_MINS": "100000",
                          "MI355RT_WPW2_MAX_IMAGE": "10000000"}),             # flat 256 spheres, 2 waves, registers
]


@pytest.mark.parametrize("case, env", _VARIANTS, ids=[f"{c}-{'-'.join(f'{k[8:]}={v}' for k, v in e.items()) or 'default'}" for c, e in _VARIANTS])
def test_every_material_kernel_is_the_global_path(monkeypatch, case, env):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if case == "tiny":
        g = load_frame("aa_48_d2")
        src = dict(spheres=g["spheres"][:, :1], lights=g["lights"][:, :1], planes=g["planes"][:, :0], fov=g["fov"],
                   cam_origin=g["cam_origin"], cam_rot=g["cam_rot"])
    else:
        src = load_frame(case) if case.startswith("aa_") else _load(case)
    S, P = src["spheres"].shape[1], src["planes"].shape[1]
    w, h = 160, 96
    rg = raygen_closed_form(w, h, float(src["fov"]))
    amb, lamb, refl = 0.05, 0.6, 0.5
    r = pkg.Renderer(0)
    try:
        r.set_camera(src["cam_origin"], src["cam_rot"])
        r.set_raygen(w, h, *rg)
        for aa, flags, spp in ((0, 0, 0), (1, 0, 0), (1, L.RT_FLAG_AA_PER_PIXEL, 0), (2, 0, 2)):
            r.set_scene(src["spheres"], src["lights"], src["planes"])
            ref8, ref32 = r.render(amb, lamb, refl, 2, aa, u8=True, f32=True, flags=flags, spp=spp, seed=3)
            r.set_scene(src["spheres"], src["lights"], src["planes"],
                        materials=(np.array([[amb, lamb, refl]]), np.zeros(S, np.int32), np.zeros(P, np.int32)))
            u8, f32 = r.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 2, aa, u8=True, f32=True, flags=flags, spp=spp, seed=3)
            assert u8.tobytes() == ref8.tobytes(), (aa, flags)
            assert f32.tobytes() == ref32.tobytes(), (aa, flags)
    finally:
        r.close()
