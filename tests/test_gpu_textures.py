"""Textures on the GPU (rt_set_scene_textures, the texture kernels): every texture_* fixture through every entry point, the
large fixtures on every traversal, all 56 texture kernels through the dispatcher's environment overrides with the same bytes and
the bytes of the CPU oracle's frames (which restates the lookup: tests/test_gpu_lit_vs_oracle.py has its edges),
uniform textures against the CPU oracle of the untextured scene (every kernel shape, random scenes, the scene sizes), depth 0
per pixel against the oracle with the texel as the hit object's colour, ids -1 and T == 0 against rt_set_scene_area_lights,
frames in flight across a scene change, column slabs, the error paths and the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import REPO, raygen_closed_form
# The environment tables, scenes and comparisons are feature_gpu's, so that the texture kernels are held to the same tables as
# their twins.
from feature_gpu import (BIG, ENVS, ENVS_IDS, ENVS_KEYS, IGNORED, KERNEL_LINE, MODES, TEX_FAMILIES, check as _check, column_slabs_are_the_full_frame,
                         family_kernels_same_bytes, family_scene, fixture_lens, kw as _kw, large_fixtures_on_a_traversal, lens_materials,
                         oracle_modes, render_host as _render_host, run_example, same as _same, same_pixels as _same_pixels,
                         scene_textures, set_view, walk_entry_points)
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_textures import CASES, fixture_textures, load_texture

sys.path.insert(0, os.path.join(REPO, "tools"))
import feature_scenes as fs  # noqa: E402

from python_ray_tracer_amd.scene import texel_index  # noqa: E402

pytestmark = pytest.mark.gpu


def _mats(g):
    return g["materials"], g["sphere_material"], g["plane_material"]


def _setup(r, g, explicit=False, textured=True):
    def scene(r, g):
        r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g), light_radius=g["light_radius"],
                    shadow_samples=int(g["shadow_samples"]), textures=fixture_textures(g, textured))
    return set_view(r, g, scene, lens=fixture_lens(g), explicit=explicit)


# ---------------------------------------------------------------------------------------------------------------------
# The fixtures (the reference's own trace() on the texel-coloured scene, tools/gen_texture_golden.py)

@pytest.mark.parametrize("case", CASES)
def test_fixture_every_entry_point(rend, case):
    g = load_texture(case)
    walk_entry_points(rend, g, _setup, case in BIG, cameras=True, begin_end=True, explicit=case != BIG[1])
    _setup(rend, g, textured=False)                             # every id -1: the fixture's u8_plain
    u8, _ = _render_host(rend, g)
    _check(g, u8, None, "every texture id -1", key="u8_plain")


@pytest.mark.parametrize("lanes_mins, records", [("30", "1"), ("30", "0"), ("100000", "1"), ("100000", "0")])
def test_large_fixtures_on_every_traversal(monkeypatch, lanes_mins, records):
    large_fixtures_on_a_traversal(monkeypatch, lanes_mins, records, load_texture, _setup)


# ---------------------------------------------------------------------------------------------------------------------
# One scene, the same bytes from every texture kernel (feature_gpu.family_kernels_same_bytes).  (A profiler's kernel trace can
# confirm the list of kernels once, but it is not something every test run can take, and it cannot say which launch picked which
# kernel.)

@pytest.mark.parametrize("kind", list(TEX_FAMILIES))
def test_every_texture_kernel_same_bytes(monkeypatch, capfd, oracle, kind):
    def scenes(src, case):
        mats = lens_materials(src["spheres"].shape[1], src["planes"].shape[1])
        return dict(materials=mats), dict(materials=mats, textures=scene_textures(src))
    family_kernels_same_bytes(monkeypatch, capfd, oracle, kind, TEX_FAMILIES, load_texture, (160, 96), "textures", scenes)


# ---------------------------------------------------------------------------------------------------------------------
# Uniform texture = no texture, against the CPU oracle: every textured object's texels all equal its own colour, so the frame
# must be the oracle's frame of the untextured scene — whatever texel the lookup picks.  This puts every texture kernel shape
# under the existing oracle.

_DIMS = [(1, 1, 1), (2, 2, 1), (3, 5, 1), (2, 2, 2), (1, 1, 7), (5, 1, 3)]


def _uniform_textures(spheres, planes, seed, most=60):
    """Up to `most` objects (the first sphere and every plane among them) get a texture of their own, random dimensions,
    origin and axes, whose texels all equal the object's colour."""
    rng = np.random.default_rng(seed)
    S, P = spheres.shape[1], planes.shape[1]
    scale = float(np.abs(spheres[3]).mean()) if S else 1.0
    objs = list(range(S, S + P)) + ([0] if S else [])
    rest = [i for i in range(1, S)]
    rng.shuffle(rest)
    objs += rest[: max(0, most - len(objs))]
    recs, chunks, first = [], [], 0
    st, pt = np.full(S, -1, np.int32), np.full(P, -1, np.int32)
    for k, o in enumerate(objs):
        dims = _DIMS[int(rng.integers(0, len(_DIMS)))]
        col = spheres[4:7, o] if o < S else planes[6:9, o - S]
        n = dims[0] * dims[1] * dims[2]
        recs.append((rng.uniform(-2, 2, 3) * scale, rng.normal(size=(3, 3)) * rng.choice([0.3, 2.0, 40.0]) / scale, dims, first))
        chunks.append(np.tile(np.asarray(col, np.float32), (n, 1)))
        first += n
        if o < S:
            st[o] = k
        else:
            pt[o - S] = k
    return recs, st, pt, np.concatenate(chunks)


def _gpu_frame(r, sc, textures, **kw):
    r.set_scene(sc["spheres"], sc["lights"], sc["planes"], flags=int(sc["typed"]), materials=(sc["table"], sc["sid"], sc["pid"]),
                light_radius=sc["radius"], shadow_samples=sc["n"], textures=textures)
    r.set_camera(sc["cam_origin"], sc["cam_rot"])
    r.set_lens(*sc["lens"])
    r.set_raygen(sc["w"], sc["h"], *sc["raygen"])
    return r.render(7.0, -3.0, 2.0, sc["depth"], sc["aa"], u8=True, f32=True, flags=sc["flags_aa"], spp=sc["spp"], seed=sc["hseed"], **kw)


@pytest.mark.parametrize("case, env", ENVS, ids=ENVS_IDS)
@pytest.mark.parametrize("family", ("mat", "refr", "scat", "soft", "lens_scat", "lens_soft"))
def test_uniform_texture_every_kernel_vs_oracle(monkeypatch, capfd, oracle, family, case, env):
    """The (scene, environment) table feature_gpu.ENVS: every shape the dispatcher can pick.  A table of 3 or 5
    columns runs the texture twins of the scatter kernels."""
    import python_ray_tracer_amd as pkg
    for k in ENVS_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    sc = family_scene(family, case)
    refs, _ = oracle_modes(oracle, family, case)
    tex = _uniform_textures(sc["spheres"], sc["planes"], len(case))
    want = {"mat": 7, "refr": 7, "scat": 7, "soft": 8, "lens_scat": 9, "lens_soft": 10}[family]
    r = pkg.Renderer(0)
    try:
        for (aa, flags, spp), (r8, r32) in zip(MODES, refs):
            u8, f32 = _gpu_frame(r, {**sc, "aa": aa, "flags_aa": flags, "spp": max(spp, 1)}, tex)
            _same(f"{family} {case} {env} aa={aa} flags={flags}", u8, f32, r8, r32)
    finally:
        r.close()
    names = KERNEL_LINE.findall(capfd.readouterr().err)
    assert names and all(int(n[6]) == want for n in names), names


@pytest.mark.parametrize("seed", [0, 1, 6, 7, 11, 12, 14, 15, 16, 18, 19, 22, 25, 26, 30, 44, 47, 49, 50, 53])
def test_uniform_texture_random_scene_vs_oracle(renderer, oracle, seed):
    """tools/feature_scenes.py's random scenes with every feature (cameras in glass, windows, grazing rough floors, ...)."""
    sc = fs.draw(seed)
    r8, r32 = fs.oracle_frame(oracle, sc)
    tex = _uniform_textures(sc["spheres"], sc["planes"], seed)
    try:
        u8, f32 = _gpu_frame(renderer, sc, tex)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same(f"seed {seed} ({sc['kind']}, S={sc['spheres'].shape[1]}, depth {sc['depth']}, aa {sc['aa']})", u8, f32, r8, r32)


@pytest.mark.parametrize("S", [1, 20, 21, 160, 161, 1024])
@pytest.mark.parametrize("kind", list(TEX_FAMILIES))
def test_uniform_texture_scene_sizes_vs_oracle(renderer, oracle, S, kind):
    """The sizes where the dispatcher changes kernels (flat up to 20 spheres, clustered from 21, lane-owned from 161) and the
    largest scene; the frame of 1024 spheres on sampled pixels (render_pixels)."""
    rng = np.random.default_rng(S)
    side = int(np.ceil(np.sqrt(S)))
    sp = np.zeros((7, S), np.float32)
    ij = np.arange(S)
    sp[0] = 2.0 + 1.1 * (ij // side) + rng.uniform(-0.2, 0.2, S)
    sp[1] = 1.1 * (ij % side - side / 2) + rng.uniform(-0.2, 0.2, S)
    sp[3] = rng.uniform(0.25, 0.5, S)
    sp[2] = sp[3]
    sp[4:7] = rng.integers(0, 256, (3, S))
    pl = np.array([[0], [0], [0], [0], [0], [1], [150], [160], [170]], np.float32)
    li = np.array([[2.0, 6.0], [-3.0, 4.0], [6.0, 9.0]], np.float32)
    soft, lens = kind in ("area_lights", "both"), kind in ("lens", "both")
    table = np.array([[0.05, 0.6, 0.4, 0.0, 1.0, 0.0], [0.0, 0.4, 0.8, 0.0, 1.0, 0.3], [0.0, 0.1, 0.0, 0.9, 1.5, 0.0], [0.02, 0.5, 0.3, 0.0, 1.0, 0.1]])
    w, h = 96, 64
    sc = dict(w=w, h=h, spheres=sp, lights=li, planes=pl, table=table, sid=(ij % 3).astype(np.int32), pid=np.array([3], np.int32),
              radius=np.array([0.4, 0.0] if soft else [0.0, 0.0], np.float32), n=2, lens=(0.05, 4.0) if lens else (0.0, 1.0),
              cam_origin=np.array([-2.0, 0.0, 2.5]), cam_rot=fs._rot([0.0, -25.0, 0.0]), fov=50.0, raygen=fs._raygen(w, h, 50.0),
              depth=3, aa=0, flags_aa=0, spp=1, hseed=S, typed=0)
    tex = _uniform_textures(sp, pl, S)
    try:
        u8, f32 = _gpu_frame(renderer, sc, tex)
    finally:
        renderer.set_lens(0.0, 1.0)
    assert u8.any()
    if S < 1024:
        r8, r32 = fs.oracle_frame(oracle, sc)
        _same(f"S={S} {kind}", u8, f32, r8, r32)
    else:
        co = np.stack([rng.integers(0, w, 400), rng.integers(0, h, 400)], axis=1).astype(np.int32)
        r8, r64 = oracle.render_pixels(w, h, co, sc["cam_origin"], sc["cam_rot"], sp, li, pl, 0.0, 0.0, 0.0, 3, 0,
                                       **fs.oracle_kwargs(sc))
        _same_pixels(f"S={S} {kind}", co, u8, f32, r8, r64)


# ---------------------------------------------------------------------------------------------------------------------
# Depth 0 against the oracle, per pixel: the pixel of the scene in which the hit object (oracle.get_intersection on the
# primary ray) has the colour of the texel texel_index() selects.  An end-to-end check of the lookup without the reference.

@pytest.mark.parametrize("seed", range(8))
def test_depth0_pixels_vs_oracle(renderer, oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    S = int(rng.integers(2, 7))
    sp = np.zeros((7, S), np.float32)
    sp[0] = rng.uniform(1.5, 5.0, S)
    sp[1] = rng.uniform(-2.0, 2.0, S)
    sp[3] = rng.uniform(0.3, 0.9, S)
    sp[2] = sp[3] + rng.uniform(0.0, 0.5, S).astype(np.float32)
    sp[4:7] = rng.integers(0, 256, (3, S))
    pl = np.array([[0], [0], [0], [0.05 * seed], [0.0], [1], [120], [130], [140]], np.float32)
    pl[3:6, 0] /= np.linalg.norm(pl[3:6, 0])
    li = np.array([[2.0, 5.0], [-3.0, 3.0], [6.0, 8.0]], np.float32)
    table = np.array([[0.08, 0.7, 0.3, 0.0, 1.0, 0.0], [0.03, 0.5, 0.0, 0.0, 1.0, 0.0]])
    sid, pid = (np.arange(S) % 2).astype(np.int32), np.array([0], np.int32)
    radius = np.array([0.3, 0.0] if seed % 2 else [0.0, 0.0], np.float32)
    w, h = 64, 40
    cam_o, cam_R = np.array([-2.0, 0.1, 2.0]), fs._rot([3.0 * seed, -25.0, 5.0])
    rg = fs._raygen(w, h, 45.0)
    # two texels and more: dimensions 2..7 along one to three axes, axes neither aligned nor orthogonal, cells of about 0.2
    recs, chunks, first = [], [], 0
    for k in range(S + 1):
        dims = [(2, 1, 1), (2, 2, 1), (3, 5, 1), (2, 2, 2), (1, 1, 7), (5, 3, 2)][int(rng.integers(0, 6))]
        n = dims[0] * dims[1] * dims[2]
        recs.append((rng.uniform(-1, 1, 3), rng.normal(size=(3, 3)) * 3.0, dims, first))
        chunks.append(rng.integers(0, 256, (n, 3)).astype(np.float32))
        first += n
    texels = np.concatenate(chunks)
    st, pt = np.arange(S, dtype=np.int32), np.array([S], np.int32)
    st[rng.integers(0, S)] = -1                                      # one sphere keeps its own colour
    renderer.set_scene(sp, li, pl, materials=(table, sid, pid), light_radius=radius, shadow_samples=2, textures=(recs, st, pt, texels))
    renderer.set_camera(cam_o, cam_R)
    renderer.set_lens(0.0, 1.0)
    renderer.set_raygen(w, h, *rg)
    u8, f32 = renderer.render(7.0, -3.0, 2.0, 0, 0, u8=True, f32=True, seed=seed)
    # the primary rays (kernels.py:19-23) and their hits
    px, y0, dy, z0, dz = rg
    groups = {}
    for x in range(w):
        for y in range(h):
            P = (px, x * dy + y0, y * dz + z0)
            v = [float(cam_R[i, 0]) * P[0] + float(cam_R[i, 1]) * P[1] + float(cam_R[i, 2]) * P[2] for i in range(3)]
            d = oracle.normalize(v)
            t, idx, ty = oracle.get_intersection(cam_o, d, sp, pl)
            k = -1
            if ty in (0, 1):
                k = int(st[idx]) if ty == 0 else int(pt[idx])
            ti = -1
            if k >= 0:
                Pt = np.array([float(cam_o[i]) + t * float(d[i]) for i in range(3)])
                ti = int(texel_index(Pt, recs[k][0], recs[k][1], recs[k][2], recs[k][3]))
            groups.setdefault((ty, idx, ti) if ti >= 0 else None, []).append((x, y))
    assert len(groups) >= 6, "the scene shows too few texels"
    kwargs = dict(raygen=rg, seed=seed, materials=(table, sid, pid), light_radius=radius, shadow_samples=2)
    for key, co in groups.items():
        s2, p2 = sp.copy(), pl.copy()
        if key is not None:
            ty, idx, ti = key
            if ty == 0:
                s2[4:7, idx] = texels[ti]
            else:
                p2[6:9, idx] = texels[ti]
        co = np.array(co, np.int32)
        r8, r64 = oracle.render_pixels(w, h, co, cam_o, cam_R, s2, li, p2, 0.0, 0.0, 0.0, 0, 0, **kwargs)
        _same_pixels(f"seed {seed} group {key}", co, u8, f32, r8, r64)


# ---------------------------------------------------------------------------------------------------------------------
# No textured object: rt_set_scene_area_lights

def test_no_textured_object_is_rt_set_scene_area_lights(monkeypatch, capfd):
    """T == 0, and T > 0 with every id -1 (or NULL id arrays): the bytes of rt_set_scene_area_lights, and no texture kernel."""
    import python_ray_tracer_amd as pkg
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    g = load_texture("everything_48_d4")
    w, h = int(g["w"]), int(g["h"])
    recs, st, pt, texels = fixture_textures(g)
    none = (np.full_like(st, -1), np.full_like(pt, -1))
    r = pkg.Renderer(0)
    try:
        r.set_camera(g["cam_origin"], g["cam_rot"])
        r.set_raygen(w, h, *raygen_closed_form(w, h, float(g["fov"])))
        common = dict(materials=_mats(g), light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]))
        for lens in ((0.0, 1.0), (float(g["aperture"]), float(g["focus_distance"]))):
            r.set_lens(*lens)
            r.set_scene(g["spheres"], g["lights"], g["planes"], **common)
            ref = [_render_host(r, g, aa=aa, spp=spp) for aa, spp in ((0, 0), (1, 0), (2, 2))]
            for textures in (([], *none, np.zeros((0, 3), np.float32)), (recs, *none, texels)):
                r.set_scene(g["spheres"], g["lights"], g["planes"], textures=textures, **common)
                for (aa, spp), (r8, r32) in zip(((0, 0), (1, 0), (2, 2)), ref):
                    u8, f32 = _render_host(r, g, aa=aa, spp=spp)
                    assert u8.tobytes() == r8.tobytes() and f32.tobytes() == r32.tobytes(), (lens, len(textures[0]), aa)
            # NULL id arrays mean all -1
            fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
            s, l, p = (np.ascontiguousarray(g[k], np.float32) for k in ("spheres", "lights", "planes"))
            t, si, pi = (np.ascontiguousarray(a) for a in _mats(g))
            rad = np.ascontiguousarray(g["light_radius"], np.float32)
            tx = np.ascontiguousarray(texels, np.float32)
            from python_ray_tracer_amd import _lib as L
            ra = (L.rt_texture * len(recs))()
            for k, (o, ax, dims, first) in enumerate(recs):
                for a in range(3):
                    ra[k].origin[a], ra[k].dim[a] = float(o[a]), int(dims[a])
                    for i in range(3):
                        ra[k].axis[a][i] = float(ax[a][i])
                ra[k].first = int(first)
            st_ = r._lib.rt_set_scene_textures(r._ctx, s.ctypes.data_as(fp), s.shape[1], l.ctypes.data_as(fp), l.shape[1],
                                               p.ctypes.data_as(fp), p.shape[1], 0, t.ctypes.data_as(C.POINTER(C.c_double)),
                                               t.shape[0], t.shape[1], si.astype(np.int32).ctypes.data_as(ip),
                                               pi.astype(np.int32).ctypes.data_as(ip), rad.ctypes.data_as(fp),
                                               int(g["shadow_samples"]), ra, len(recs), None, None, tx.ctypes.data_as(fp), len(tx))
            assert st_ == L.RT_OK
            u8, f32 = _render_host(r, g, aa=0)
            assert u8.tobytes() == ref[0][0].tobytes() and f32.tobytes() == ref[0][1].tobytes()
    finally:
        r.close()
    names = KERNEL_LINE.findall(capfd.readouterr().err)
    assert len(names) >= 20 and all(int(n[6]) < 7 for n in names), names


# ---------------------------------------------------------------------------------------------------------------------
# The ring, slabs, errors, the example

def test_frames_in_flight_keep_their_textures(rend):
    g = load_texture("default_64_d4")
    w, h = _setup(rend, g)
    recs, st, pt, texels = fixture_textures(g)
    tex8, _ = _render_host(rend, g)
    _check(g, tex8, None, "textured")
    other = (recs, st, pt, (255.0 - texels).astype(np.float32))      # the same textures with inverted texels
    args = dict(materials=_mats(g), light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]))
    rend.set_scene(g["spheres"], g["lights"], g["planes"], textures=other, **args)
    other8, _ = _render_host(rend, g)
    assert not np.array_equal(other8, tex8)
    p = rend.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), **_kw(g))
    npx = w * h
    s1, s2 = rend.stream_create(), rend.stream_create()
    bufs = [rend.malloc(3 * npx) for _ in range(6)]
    try:
        # six launches on two streams with a scene change before each: more changes than the ring has buffers
        kinds = ["tex", "other", "plain", "tex", "other", "tex"]
        for i, kind in enumerate(kinds):
            tx = dict(tex=(recs, st, pt, texels), other=other, plain=fixture_textures(g, False))[kind]
            rend.set_scene(g["spheres"], g["lights"], g["planes"], textures=tx, **args)
            rend.render_device(p, 0, w, bufs[i], None, npx, stream=(s1, s2)[i % 2])
        rend.sync(s1)
        rend.sync(s2)
        for i, kind in enumerate(kinds):
            got = np.empty((3, w, h), np.uint8)
            rend.d2h(got, bufs[i])
            if kind == "other":
                assert np.array_equal(got, other8), f"launch {i}: the inverted texels"
            else:
                _check(g, got, None, f"launch {i} ({kind})", key="u8" if kind == "tex" else "u8_plain")
    finally:
        for b in bufs:
            rend.free(b)
        rend.stream_destroy(s1)
        rend.stream_destroy(s2)


@pytest.mark.parametrize("aa, spp", [(0, 0), (1, 0), (2, 2)])
def test_column_slab_is_the_full_frame(rend, aa, spp):
    column_slabs_are_the_full_frame(rend, load_texture("everything_48_d4"), _setup, aa, spp, ((9, 41), (33, 48)))


def test_errors_leave_the_previous_scene(rend):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = load_texture("default_64_d4")
    _setup(rend, g)
    recs, st, pt, texels = fixture_textures(g)
    args = dict(materials=_mats(g), light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]))
    nan, inf = float("nan"), float("inf")

    def rec(k, origin=None, axes=None, dims=None, first=None):
        o, ax, d, f = recs[k]
        out = list(recs)
        out[k] = (o if origin is None else origin, ax if axes is None else axes, d if dims is None else dims, f if first is None else first)
        return out

    def ids(a, i, v):
        a = np.array(a)
        a[i] = v
        return a

    bad_ax = np.array(recs[1][1])
    bad_ax[2, 1] = nan
    bad_tx = np.array(texels)
    bad_tx[3, 1] = inf
    T = len(recs)
    cases = {
        "sphere id == T": (recs, ids(st, 0, T), pt, texels),
        "sphere id -2": (recs, ids(st, 1, -2), pt, texels),
        "plane id == T": (recs, st, ids(pt, 0, T), texels),
        "dimension 0": (rec(0, dims=(0, 2, 1)), st, pt, texels),
        "dimension 4097": (rec(0, dims=(4097, 1, 1)), st, pt, np.zeros((5000, 3), np.float32)),
        "origin nan": (rec(1, origin=(0.0, nan, 0.0)), st, pt, texels),
        "origin inf": (rec(1, origin=(inf, 0.0, 0.0)), st, pt, texels),
        "axis nan": (rec(1, axes=bad_ax), st, pt, texels),
        "texel inf": (recs, st, pt, bad_tx),
        "texel range past the end": (rec(T - 1, first=len(texels) - 1), st, pt, texels),
        "negative first": (rec(0, first=-1), st, pt, texels),
        "T > RT_MAX_TEXTURES": ([recs[0]] * 65, st, pt, texels),
    }
    for what, tx in cases.items():
        with pytest.raises(pkg.RenderError) as e:
            rend.set_scene(g["spheres"], g["lights"], g["planes"], textures=tx, **args)
        assert e.value.status == L.RT_ERR_BAD_ARG, what
        u8, f32 = _render_host(rend, g)                           # the previous scene stays current
        _check(g, u8, f32, f"after a refused scene ({what})")
    # through the C ABI: NULL arrays, n_texels > RT_MAX_TEXELS, T > 0 with M == 0
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    s, l, p = (np.ascontiguousarray(g[k], np.float32) for k in ("spheres", "lights", "planes"))
    t = np.ascontiguousarray(g["materials"], np.float64)
    si, pi = np.ascontiguousarray(g["sphere_material"], np.int32), np.ascontiguousarray(g["plane_material"], np.int32)
    rad = np.ascontiguousarray(g["light_radius"], np.float32)
    tx = np.ascontiguousarray(texels, np.float32)
    sti, pti = np.ascontiguousarray(st, np.int32), np.ascontiguousarray(pt, np.int32)
    ra = (L.rt_texture * T)()
    for k, (o, ax, dims, first) in enumerate(recs):
        for a in range(3):
            ra[k].origin[a], ra[k].dim[a] = float(o[a]), int(dims[a])
            for i in range(3):
                ra[k].axis[a][i] = float(ax[a][i])
        ra[k].first = int(first)

    def call(ctx=rend._ctx, M=t.shape[0], textures=ra, nT=T, texels_=tx.ctypes.data_as(fp), n=len(tx), radius=rad.ctypes.data_as(fp)):
        return rend._lib.rt_set_scene_textures(ctx, s.ctypes.data_as(fp), s.shape[1], l.ctypes.data_as(fp), l.shape[1],
                                               p.ctypes.data_as(fp), p.shape[1], 0, t.ctypes.data_as(C.POINTER(C.c_double)), M,
                                               t.shape[1], si.ctypes.data_as(ip), pi.ctypes.data_as(ip), radius,
                                               int(g["shadow_samples"]), textures, nT, sti.ctypes.data_as(ip), pti.ctypes.data_as(ip),
                                               texels_, n)

    assert call() == L.RT_OK
    for what, kw in {"ctx NULL": dict(ctx=None), "textures NULL": dict(textures=None), "texels NULL": dict(texels_=None),
                     "n_texels > RT_MAX_TEXELS": dict(n=L.RT_MAX_TEXELS + 1), "n_texels < 0": dict(n=-1), "T < 0": dict(nT=-1),
                     "T > 0 with M == 0": dict(M=0), "light_radius NULL": dict(radius=None)}.items():
        assert call(**kw) == L.RT_ERR_BAD_ARG, what
        u8, f32 = _render_host(rend, g)
        _check(g, u8, f32, f"after a refused scene ({what})")
    ra[1].reserved = 1                                            # the reserved field must be 0
    assert call() == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(rend, g)
    _check(g, u8, f32, "after a refused scene (reserved != 0)")
    ra[1].reserved = 0
    assert call() == L.RT_OK
    with pytest.raises(ValueError):                               # Python: textures without a material table
        rend.set_scene(g["spheres"], g["lights"], g["planes"], textures=(recs, st, pt, texels))
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels for a scene with materials
        _render_host(rend, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    u8, f32 = _render_host(rend, g)
    _check(g, u8, f32, "after the refused launch")


def test_largest_texel_array(rend):
    """RT_MAX_TEXELS texels (four 1024 x 1024 images) in one 4096-wide texture: texels near the end of the array are read."""
    from python_ray_tracer_amd import _lib as L
    n = L.RT_MAX_TEXELS
    texels = np.zeros((n, 3), np.float32)
    texels[:, 0] = np.arange(n) % 251
    texels[n - 1] = (255.0, 1.0, 2.0)
    sp = np.zeros((7, 0), np.float32)
    pl = np.array([[0], [0], [0], [0], [0], [1], [9], [9], [9]], np.float32)
    li = np.array([[0.0], [0.0], [5.0]], np.float32)
    table = np.array([[1.0, 0.0, 0.0]])                               # ambient only: the pixel is the texel
    recs = [((0.0, 0.0, 0.0), np.eye(3) * 64.0, (4096, 1024, 1), 0)]
    rend.set_scene(sp, li, pl, materials=(table, np.zeros(0, np.int32), np.zeros(1, np.int32)), textures=(recs, np.zeros(0, np.int32),
                   np.zeros(1, np.int32), texels))
    rend.set_camera(np.array([0.0, 0.0, 1.0]), fs._rot([0.0, -90.0, 0.0]))
    w, h = 32, 32
    rg = fs._raygen(w, h, 45.0)
    rend.set_raygen(w, h, *rg)
    u8, f32 = rend.render(0.0, 0.0, 0.0, 0, 0, u8=True, f32=True)
    # (floor points just below the grid origin in y wrap to the last rows of the grid)
    px, y0, dy, z0, dz = rg
    cam_R = fs._rot([0.0, -90.0, 0.0])
    hits = top = 0
    for x in range(w):
        for y in range(h):
            P = (px, x * dy + y0, y * dz + z0)
            v = np.array([cam_R[i, 0] * P[0] + cam_R[i, 1] * P[1] + cam_R[i, 2] * P[2] for i in range(3)])
            d = v / np.sqrt((v * v).sum())
            if d[2] >= -1e-3:
                continue
            t = -1.0 / d[2]
            Pt = np.array([0.0, 0.0, 1.0]) + t * d
            g = Pt[:2] * 64.0
            if np.abs(g - np.round(g)).min() < 1e-6:              # (too close to a cell boundary to predict without the exact t)
                continue
            ti = int(texel_index(Pt, recs[0][0], recs[0][1], recs[0][2]))
            assert f32[:, x, y].tolist() == texels[ti].tolist(), (x, y, ti)
            hits += 1
            top = max(top, ti)
    assert hits > 500 and top >= n - 64 * 4096, (hits, top)


def test_example_with_checker_writes_png(tmp_path):
    """examples/render_png.py --checker [--texture IMAGE]: a checkered floor, and an image on it."""
    from PIL import Image
    img = str(tmp_path / "poster.png")
    Image.fromarray(np.random.default_rng(3).integers(0, 256, (12, 16, 3)).astype(np.uint8)).save(img)
    outs = {}
    for flag in (["--materials"], ["--checker"], ["--checker", "--texture", img]):
        out = str(tmp_path / f"{'_'.join(x.strip('-') for x in flag[:2])}{len(flag)}.png")
        _, outs[" ".join(flag)] = run_example(out, "160x96", 3, 2, *flag)
    a, b, c = outs.values()
    assert b.shape == (96, 160, 3) and b.any()
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
