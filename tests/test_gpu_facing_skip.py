"""The wave-level skip of back-facing point lights (rt_facing.h, trace_bounce's light loops) on the GPU: every frame bit for
bit, uint8 and float32, against the CPU oracle's frame of the same scene.  Frames of 16 x 16 to 24 x 16 pixels are two to six
8 x 8 tiles, one wave each: the smallest in which a wave is wholly skipped, holds certified and uncertified lanes together, or
holds no certified lane.  The camera is at the origin (one test: above it), looks along +x, z is up."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, raygen_closed_form
from feature_gpu import same as _same

sys.path.insert(0, os.path.join(REPO, "tools"))
import feature_scenes as fs  # noqa: E402

pytestmark = pytest.mark.gpu

NO_PLANES = np.zeros((9, 0), np.float32)
FLOOR = np.array([[0, 0, -1.0, 0, 0, 1, 180, 180, 170]], np.float32).T.copy()


def _cols(rows):
    return np.array(rows, np.float32).T.copy()


def _plain(w, h, spheres, lights, planes, *, depth, lamb=0.6, amb=0.1, refl=0.4, cam=(0.0, 0.0, 0.0)):
    return dict(w=w, h=h, spheres=_cols(spheres) if len(spheres) else np.zeros((7, 0), np.float32), lights=_cols(lights), planes=planes,
                depth=depth, lamb=lamb, amb=amb, refl=refl, cam=np.array(cam), rot=np.eye(3), rg=raygen_closed_form(w, h, 60.0))


def _oracle_plain(oracle, sc, want=("u8", "f32")):
    return oracle.render(sc["w"], sc["h"], sc["cam"], sc["rot"], sc["spheres"], sc["lights"], sc["planes"], sc["amb"], sc["lamb"],
                         sc["refl"], sc["depth"], 0, raygen=sc["rg"], want=want)


def _gpu_plain(r, sc, flags=0):
    r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
    r.set_camera(sc["cam"], sc["rot"])
    r.set_lens(0.0, 1.0)
    r.set_raygen(sc["w"], sc["h"], *sc["rg"])
    return r.render(sc["amb"], sc["lamb"], sc["refl"], sc["depth"], 0, u8=True, f32=True, flags=flags)


def _check_plain(renderer, oracle, sc, what):
    ref = _oracle_plain(oracle, sc)
    u8, f32 = _gpu_plain(renderer, sc)
    _same(what, u8, f32, ref["u8"], ref["f32"])
    assert ref["u8"].any(), what
    return ref


def _counted(renderer, oracle, sc):
    """(shadow queries traced, skipped) of the counting kernels, after checking their sum and frame against the oracle's."""
    from python_ray_tracer_amd import _lib as L
    ref = _oracle_plain(oracle, sc, want=("u8", "f32", "counters"))
    renderer.reset_stats()
    u8, f32 = _gpu_plain(renderer, sc, flags=L.RT_FLAG_COUNT_RAYS)
    st = renderer.stats()
    renderer.reset_stats()
    _same("counting kernel", u8, f32, ref["u8"], ref["f32"])
    assert st["closest_queries"] == ref["counters"]["closest"] and st["hits"] == ref["counters"]["hits"]
    assert st["shadow_traced"] + st["shadow_skipped"] == ref["counters"]["shadow"] > 0
    return st["shadow_traced"], st["shadow_skipped"]


# One sphere of angular radius 47 degrees around the view axis (the frame's corners are 39 degrees off it), three lights behind it:
# every hit has every light below its horizon, so every wave skips every light.
def _all_behind(depth, **kw):
    return _plain(16, 16, [[3.0, 0, 0, 2.2, 250, 120, 30]], [[10.0, 3.0, 2.0], [12.0, 0.0, -4.0], [9.0, -5.0, 1.0]], NO_PLANES, depth=depth, **kw)


# A unit sphere over a floor, a light beside it (its terminator runs down the middle of the sphere's disc, through tiles that
# also show lit floor), one behind it and one above the camera: waves with certified and uncertified lanes for the same light.
def _terminator(depth, w=24, h=16, **kw):
    return _plain(w, h, [[4.0, 0, 0, 1.0, 250, 120, 30], [3.0, 1.6, -0.6, 0.4, 40, 200, 90]], [[4.0, 6.0, 0.3], [9.0, -1.0, 0.5], [0.0, 0.0, 3.0]], FLOOR,
                  depth=depth, **kw)


@pytest.mark.parametrize("depth", [0, 1])
def test_every_light_behind_the_only_sphere(renderer, oracle, depth):
    """Every wave skips every light (the counting kernels trace no shadow query at all), and the last trace is the first
    (depth 0) or the second (depth 1)."""
    sc = _all_behind(depth)
    ref = _check_plain(renderer, oracle, sc, f"all lights behind, depth {depth}")
    assert (ref["u8"] != 0).any(axis=0).all()                      # the sphere fills the frame (its ambient term)
    traced, skipped = _counted(renderer, oracle, sc)
    assert traced == 0 and skipped == 3 * 16 * 16


@pytest.mark.parametrize("depth", [0, 1, 3])
def test_terminator_crosses_a_tile(renderer, oracle, depth):
    sc = _terminator(depth)
    _check_plain(renderer, oracle, sc, f"terminator, depth {depth}")


def test_terminator_ray_counters(renderer, oracle):
    """RT_FLAG_COUNT_RAYS: a skipped wave records its live lanes as skipped queries, so traced + skipped is the oracle's count;
    both kinds occur, and in one and the same tile column of the sphere."""
    traced, skipped = _counted(renderer, oracle, _terminator(2))
    assert traced > 100 and skipped > 100
    # one 8 x 16 column slab through the middle of the sphere (two tiles): lit and unlit hits of light 0 side by side
    sc = _terminator(0)
    sc["lights"] = sc["lights"][:, :1]
    ref = _oracle_plain(oracle, sc)["f32"]
    amb_only = _oracle_plain(oracle, {**sc, "lamb": 0.0})["f32"]
    lit = (ref != amb_only).any(axis=0)[8:16]
    assert 10 <= lit.sum() <= lit.size - 10


def test_light_at_the_biased_hit_height(renderer, oracle):
    """A floor z = 0 under a camera at z = 1 and a light at z = float32(0.0002), the height BIAS * N lifts a floor hit to: the
    hit's z is 0 or a few 2^-53 off it, so u = (light - Pt).N is 0 or a rounding error of either sign, nothing is certified, and
    where k comes out positive the (grazing) shadow query is asked as before."""
    pl = np.array([[0, 0, 0, 0, 0, 1, 180, 180, 170]], np.float32).T.copy()
    bias = float(np.float32(0.0002))
    sc = _plain(16, 16, [], [[3.0, 0.5, bias], [2.0, -1.0, 2.0]], pl, depth=1, cam=(0.0, 0.0, 1.0))
    _check_plain(renderer, oracle, sc, "u == 0")
    traced, skipped = _counted(renderer, oracle, sc)
    assert traced > 0


@pytest.mark.parametrize("lamb", [-0.6, 0.0, -0.0])
def test_lamb_not_positive(renderer, oracle, lamb):
    """lamb = -0.6: k > 0 where the light is BEHIND the surface; the certificate never holds (facing_tau is infinite) and those
    hits ask their shadow queries.  lamb = +-0: k is never positive, certified or not."""
    for sc in (_terminator(1, lamb=lamb), _all_behind(1, lamb=lamb)):
        _check_plain(renderer, oracle, sc, f"lamb {lamb}")
    traced, skipped = _counted(renderer, oracle, _all_behind(0, lamb=lamb))
    assert (traced, skipped) == ((3 * 256, 0) if lamb < 0 else (0, 3 * 256))


def _table_scene(table, sid, pid, *, depth=2, light_rgb=None):
    t = _terminator(depth)
    w, h = t["w"], t["h"]
    return dict(kind="facing", w=w, h=h, spheres=t["spheres"], lights=t["lights"], planes=t["planes"], table=np.array(table, np.float64),
                sid=np.array(sid, np.int32), pid=np.array(pid, np.int32), radius=np.zeros(3, np.float32), n=1, lens=(0.0, 1.0),
                cam_origin=t["cam"], cam_rot=t["rot"], fov=60.0, raygen=t["rg"], depth=depth, aa=0, flags_aa=0, spp=1, hseed=5, typed=0,
                textures=None, light_rgb=light_rgb, sky=None)


def _check_table(renderer, oracle, sc, what):
    r8, r32 = fs.oracle_frame(oracle, sc)
    try:
        u8, f32 = fs.gpu_frame(renderer, sc)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same(what, u8, f32, r8, r32)
    return r8


def test_material_table_with_lambert_of_both_signs(renderer, oracle):
    """MAT kernels: the Lambert coefficient is the lane's own.  The large sphere's is negative (lit where the light is behind it:
    no certificate there), the small sphere's zero, the floor's positive, so one wave holds lanes of all three."""
    table = [[0.1, -0.5, 0.3], [0.05, 0.0, 0.5], [0.1, 0.6, 0.2]]
    sc = _table_scene(table, [0, 1], [2])
    r8 = _check_table(renderer, oracle, sc, "lamb of both signs")
    flipped = fs.oracle_frame(oracle, {**sc, "table": np.array([[0.1, 0.5, 0.3]] + table[1:])})[0]
    assert (flipped != r8).any(axis=0).sum() >= 20                 # (the negative coefficient is live)
    _check_table(renderer, oracle, {**sc, "depth": 0}, "lamb of both signs, depth 0")


def test_highlight_on_a_back_lit_sphere(renderer, oracle):
    """LIT kernels: spec > 0 on every object, coloured lights; light 1 is behind the large sphere, whose waves skip it, and light
    0's terminator crosses its tiles: neither the Lambert term nor the highlight may be lost or gained."""
    table = [[0.05, 0.5, 0.3, 0.0, 1.0, 0.0, 150.0, 16.0], [0.05, -0.4, 0.2, 0.0, 1.0, 0.0, 90.0, 4.0], [0.1, 0.6, 0.2, 0.0, 1.0, 0.0, 60.0, 64.0]]
    rgb = np.array([[1.0, 0.7, 0.4], [0.3, 0.5, 1.5], [0.6, 0.9, 0.2]], np.float32)
    sc = _table_scene(table, [0, 1], [2], light_rgb=rgb)
    r8 = _check_table(renderer, oracle, sc, "back-lit highlight")
    off = fs.oracle_frame(oracle, fs.strip(sc, "lighting"))[0]
    assert (off != r8).any(axis=0).sum() >= 20
