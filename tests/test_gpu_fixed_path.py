"""The render kernels' once-per-tile path (rt_device.h: render_kernel's prologue, pixel_P, store_pixel and rt_math.h's clip_color)
against the CPU oracle, byte for byte, uint8 and float32: what no other parity test pins of it.
  * the clip: a frame without lights at depth 0, whose pixels are exactly amb * colour, with colours 0.5 and 0.25 and ambient
    coefficients that put the values on the clip's ties and on both sides of its bounds (-1.5, -0.5, 0.5, 1.5, 254.5, 255.5, 256.5
    through 0.5; quarter offsets through 0.25), and once with a block of zero vectors in the pixel table (NaN rays);
  * the primary ray from the pixel table and from the closed-form grid, at 1, 4, 5 and 8 spheres (both cull-group counts, both ends);
  * multi-frame launches in the settled dispatch order (three calls of a three-frame sequence behind the two measuring launches),
    light counts 0, 1, 3 and 5, and a 64-light scene, which takes a four-wave kernel (table_layout, not flat_layout).
Every case runs twice, with MI355RT_SMALL_SCENE unset (the small-scene twins, where the scene has them) and 0 (the ground-plane
twins compiled for any sphere count), against one oracle frame per case.  Frames of 37 x 29 and 24 x 40."""
import numpy as np
import pytest

from conftest import load_frame, raygen_closed_form
from feature_gpu import grid as _grid
import ground_plane_scenes as gps

pytestmark = pytest.mark.gpu
KNOBS = ("MI355RT_CLUSTER_MINS", "MI355RT_LANES_MINS", "MI355RT_F32_RECORDS", "MI355RT_LANES_PARK", "MI355RT_WPW2_MAX_IMAGE",
         "MI355RT_ORDER_GROUP", "MI355RT_ORDER_TILES", "MI355RT_SEQ_ORDER", "MI355RT_CHUNKS", "MI355RT_GROUND_PLANE", "MI355RT_SMALL_SCENE")
SMALL = pytest.mark.parametrize("small", [True, False], ids=["small_scene_twins", "MI355RT_SMALL_SCENE=0"])
_REF = {}          # case name -> the oracle's frames, computed once and shared by the two runs of the case


def _renderer(monkeypatch, small):
    import python_ray_tracer_amd as pkg
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if not small:
        monkeypatch.setenv("MI355RT_SMALL_SCENE", "0")
    return pkg.Renderer(0)


def _reference(oracle, name, sc, w, h, amb, lamb, refl, depth, pixel_loc=None):
    if name not in _REF:
        kw = dict(pixel_loc=pixel_loc) if pixel_loc is not None else dict(raygen=raygen_closed_form(w, h, sc["fov"]))
        ref = oracle.render(w, h, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], amb, lamb, refl, depth, False,
                            want=("u8", "f32"), **kw)
        _REF[name] = (ref["u8"].copy(), ref["f32"].copy())
        for a in _REF[name]:
            a.setflags(write=False)
    return _REF[name]


def _same(name, u8, f32, ref):
    assert np.array_equal(u8, ref[0]), (name, int((u8 != ref[0]).any(axis=0).sum()), "uint8 pixels differ")
    assert f32.tobytes() == ref[1].tobytes(), (name, int((f32.view(np.uint32) != ref[1].view(np.uint32)).any(axis=0).sum()), "float32 pixels differ")


def _spheres(S, colours=None):
    """The first S of the eight spheres of the 37 x 29 fixture."""
    sp = np.ascontiguousarray(load_frame("odd_37x29")["spheres"][:, :S]).astype(np.float32)
    assert sp.shape == (7, S)
    if colours is not None:
        sp[4:7] = np.asarray(colours, np.float32)[None, :S]
    return sp


# ---- the clip ----

AMBS = (-3.0, -1.0, 1.0, 3.0, 509.0, 511.0, 513.0, 1021.0, 1023.0)


def _clip_scene():
    sc = gps.fixture_scene("odd_37x29")
    sp = _spheres(8, [0.5, 0.25, 0.5, 0.25, 0.5, 0.5, 0.25, 0.5])
    return dict(sc, spheres=sp, lights=np.zeros((3, 0), np.float32),
                planes=gps.planes_of(gps.GROUND[:6] + (0.25, 0.25, 0.25)))


@SMALL
def test_clip_on_its_ties_and_bounds(monkeypatch, oracle, small):
    sc, w, h = _clip_scene(), 37, 29
    seen = set()
    with _renderer(monkeypatch, small) as r:
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        r.set_raygen(w, h, *raygen_closed_form(w, h, sc["fov"]))
        for amb in AMBS:
            u8, f32 = r.render(amb, 0.6, 0.3, 0, 0, u8=True, f32=True)
            ref = _reference(oracle, f"clip amb={amb}", sc, w, h, amb, 0.6, 0.3, 0)
            _same(f"clip amb={amb}", u8, f32, ref)
            seen |= set(np.unique(f32).tolist())
    # the frames hold what the case is for: amb * 0.5 and amb * 0.25, exactly, of both objects' kinds
    for v in (-1.5, -0.5, 0.5, 1.5, 254.5, 255.5, 256.5, -0.75, -0.25, 0.25, 0.75, 127.25, 127.75, 128.25, 255.25, 255.75):
        assert v in seen, v


@SMALL
def test_clip_of_nan_rays(monkeypatch, oracle, small):
    sc, w, h = _clip_scene(), 37, 29
    grid = _grid(w, h, raygen_closed_form(w, h, sc["fov"]))
    grid[:, 11:21, 9:19] = 0.0                    # zero vectors: NaN directions (crosses tiles; waves with both kinds of lanes)
    with _renderer(monkeypatch, small) as r:
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        r.set_pixel_loc(grid)
        u8, f32 = r.render(511.0, 0.6, 0.3, 0, 0, u8=True, f32=True)
    _same("clip NaN rays", u8, f32, _reference(oracle, "clip NaN rays", sc, w, h, 511.0, 0.6, 0.3, 0, pixel_loc=grid))


# ---- the primary ray ----

@SMALL
@pytest.mark.parametrize("S", [1, 4, 5, 8])
def test_pixel_table_and_closed_form(monkeypatch, oracle, small, S):
    sc, w, h = dict(gps.fixture_scene("odd_37x29"), spheres=_spheres(S)), 37, 29
    amb, lamb, refl = sc["shade"]
    grid = _grid(w, h, raygen_closed_form(w, h, sc["fov"]))
    with _renderer(monkeypatch, small) as r:
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        r.set_pixel_loc(grid)
        t8, t32 = r.render(amb, lamb, refl, 3, 0, u8=True, f32=True)
        r.set_raygen(w, h, *raygen_closed_form(w, h, sc["fov"]))
        c8, c32 = r.render(amb, lamb, refl, 3, 0, u8=True, f32=True)
    _same(f"S={S} pixel table", t8, t32, _reference(oracle, f"S={S} table", sc, w, h, amb, lamb, refl, 3, pixel_loc=grid))
    _same(f"S={S} closed form", c8, c32, _reference(oracle, f"S={S} closed", sc, w, h, amb, lamb, refl, 3))
    assert t8.any() and t8.tobytes() == c8.tobytes() and t32.tobytes() == c32.tobytes()


# ---- multi-frame launches, light counts ----

def _lights(L):
    rng = np.random.default_rng(L)
    base = load_frame("fivelights_32")["lights"].astype(np.float32)
    if L <= base.shape[1]:
        return np.ascontiguousarray(base[:, :L])
    return np.stack([rng.uniform(-3.0, 6.0, L), rng.uniform(-5.0, 5.0, L), rng.uniform(2.0, 7.0, L)]).astype(np.float32)


@SMALL
@pytest.mark.parametrize("L", [0, 1, 3, 5, 64])
def test_sequences_in_the_settled_order(monkeypatch, oracle, small, L):
    """Two single-frame launches (the ones that measure the dispatch order), then three calls of a three-frame rt_render_sequence:
    launches of nframes > 1 in the settled order, which never read the workgroups' cost words.  64 lights: a four-wave kernel."""
    w, h, n = 24, 40, 3
    sc = dict(gps.fixture_scene("portrait_24x40"), lights=_lights(L))
    amb, lamb, refl = (0.05, 0.02, 0.3) if L == 64 else (0.1, 0.3, 0.4)
    ref = _reference(oracle, f"sequence L={L}", sc, w, h, amb, lamb, refl, 2)
    npx = w * h
    with _renderer(monkeypatch, small) as r:
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        r.set_raygen(w, h, *raygen_closed_form(w, h, sc["fov"]))
        for i in range(2):
            u8, f32 = r.render(amb, lamb, refl, 2, 0, u8=True, f32=True)
            _same(f"L={L} measuring launch {i}", u8, f32, ref)
        p = r.params(amb, lamb, refl, 2, 0, 0)
        d8, d32 = r.malloc(n * 3 * npx), r.malloc(n * 12 * npx)
        try:
            for call in range(3):
                r.h2d(d8, np.zeros(n * 3 * npx, np.uint8))
                r.h2d(d32, np.full(n * 3 * npx, -1.0, np.float32))
                r.render_sequence(p, 0, w, n, d8, d32, npx, 3 * npx, None, None, n)
                r.sync()
                u8, f32 = np.empty((n, 3, w, h), np.uint8), np.empty((n, 3, w, h), np.float32)
                r.d2h(u8, d8)
                r.d2h(f32, d32)
                for f in range(n):
                    _same(f"L={L} call {call} frame {f}", u8[f], f32[f], ref)
        finally:
            r.free(d8); r.free(d32)
    assert ref[0].any()
