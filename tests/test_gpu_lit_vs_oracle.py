"""The texture, lighting and sky kernels (rt_device.h TEX, LIT and SKY) against the CPU oracle's restatement of include/mi355rt.h
(oracle/rt_oracle.c orc_render_ex, pinned to every pixel of the texture_*, lighting_* and sky_* fixtures by
tests/test_oracle_features.py): uint8 and float32, bit for bit, no tolerance anywhere.  (feature_gpu.kernel_table_refs gives the
three test_every_{texture,lighting,sky}_kernel_same_bytes tests the oracle's frames of their scenes.)  Here: seeded random scenes of
tools/feature_scenes.draw_lit, the edges of the texel lookup, of the two lighting terms and of sky(d), and every entry point.
Each case first checks, on the oracle alone, that its feature is live: the oracle's frame changes when the feature is stripped
(at least 20 pixels in the kernel table, at least 5 elsewhere)."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, raygen_closed_form
from feature_gpu import IGNORED, same as _same, same_pixels as _same_pixels

sys.path.insert(0, os.path.join(REPO, "tools"))
import feature_scenes as fs  # noqa: E402

pytestmark = pytest.mark.gpu
SHININESS = fs.SHININESS


# ---------------------------------------------------------------------------------------------------------------------
# Helpers

def _live(oracle, sc, features, r8=None, least=5, coords=None):
    """Assert that each of `features` changes at least `least` pixels of the oracle's frame (or of its sampled pixels)."""
    for f in features:
        if coords is None:
            r8 = fs.oracle_frame(oracle, sc)[0] if r8 is None else r8
            n = int((fs.oracle_frame(oracle, fs.strip(sc, f))[0] != r8).any(axis=0).sum())
        else:
            r8 = fs.oracle_pixels(oracle, sc, coords)[0] if r8 is None else r8
            n = int((fs.oracle_pixels(oracle, fs.strip(sc, f), coords)[0] != r8).any(axis=1).sum())
        assert n >= least, f"{f} changes only {n} pixels of the oracle's frame ({sc['kind']})"


def _check(renderer, oracle, sc, what, features, **kw):
    r8, r32 = fs.oracle_frame(oracle, sc)
    _live(oracle, sc, features, r8)
    try:
        u8, f32 = fs.gpu_frame(renderer, sc, **kw)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same(what, u8, f32, r8, r32)
    return r8, r32


def _check_sampled(renderer, oracle, sc, what, features, co):
    r8, r64 = fs.oracle_pixels(oracle, sc, co)
    _live(oracle, sc, features, r8, coords=co)
    try:
        u8, f32 = fs.gpu_frame(renderer, sc)
    finally:
        renderer.set_lens(0.0, 1.0)
    _same_pixels(what, co, u8, f32, r8, r64)
    return r8, r64


TABLE = np.array([[0.05, 0.6, 0.2, 0.0, 1.0, 0.0, 80.0, 32.0],        # 0 matte
                  [0.0, 0.3, 0.9, 0.0, 1.0, 0.0, 150.0, 256.0],       # 1 mirror
                  [0.02, 0.5, 0.6, 0.0, 1.0, 0.4, 60.0, 8.0],         # 2 rough
                  [0.01, 0.1, 0.0, 0.9, 1.5, 0.0, 200.0, 1024.0],     # 3 glass
                  [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0]])          # 4 flat: the pixel is the object's colour or texel itself
SKY = np.array([0.0, 0.6, 0.8, 30.0, 80.0, 210.0, 230.0, 210.0, 190.0, 70.0, 60.0, 50.0, 4.0, 0.8, 0.0, 0.6, 0.97,
                250.0, 230.0, 180.0, 120.0, 90.0, 40.0, 16.0])


def _base(w=48, h=32, **over):
    """A hand-made scene in feature_scenes' form: a glass, a mirror, a rough and a matte sphere over a floor, three coloured
    lights, the camera at (0, 0, 0.5) looking along +x with z up.  No texture, no sky, no lens until a test adds them."""
    sp = np.array([[4.0, -1.2, 0.6, 0.8, 200, 220, 255], [5.0, 1.2, 0.7, 0.9, 240, 240, 240], [3.2, 0.2, 0.0, 0.4, 250, 120, 30],
                   [6.0, 0.0, 2.0, 0.7, 40, 200, 90]], np.float32).T.copy()
    pl = np.array([[0, 0, -0.5, 0, 0, 1, 180, 180, 170]], np.float32).T.copy()
    li = np.array([[1.0, 2.0, 5.0], [3.0, -3.0, 4.0], [-2.0, 0.0, 3.0]], np.float32).T.copy()
    sc = dict(kind="base", w=w, h=h, spheres=sp, lights=li, planes=pl, table=TABLE.copy(), sid=np.array([3, 1, 2, 0], np.int32),
              pid=np.array([0], np.int32), radius=np.zeros(3, np.float32), n=1, lens=(0.0, 1.0), cam_origin=np.array([0.0, 0.0, 0.5]),
              cam_rot=np.eye(3), fov=60.0, raygen=raygen_closed_form(w, h, 60.0), depth=3, aa=0, flags_aa=0, spp=1, hseed=9, typed=0,
              textures=None, light_rgb=np.array([[1.0, 0.7, 0.4], [0.3, 0.5, 1.5], [0.6, 0.9, 0.2]], np.float32), sky=None)
    sc.update(over)
    return sc


def _one_texture(sc, origin, axes, dims, texels=None, first=0, spheres=True, planes=True, seed=0):
    """The scene with one texture record on its spheres and/or planes; random texels unless given."""
    n = int(dims[0]) * int(dims[1]) * int(dims[2])
    if texels is None:
        texels = np.random.default_rng(seed).integers(0, 256, (first + n, 3)).astype(np.float32)
    S, P = sc["spheres"].shape[1], sc["planes"].shape[1]
    return {**sc, "textures": ([(np.asarray(origin, np.float64), np.asarray(axes, np.float64), tuple(int(v) for v in dims), first)],
                               np.full(S, 0 if spheres else -1, np.int32), np.full(P, 0 if planes else -1, np.int32), texels)}


# ---------------------------------------------------------------------------------------------------------------------
# Seeded random scenes with every feature together (tools/feature_scenes.draw_lit), each kind of bias at least twice.  Textures,
# lighting and the sky are live in each: stripping any of them changes at least 5 pixels of the oracle's frame.
LIT_SEEDS = [1, 4, 6, 7, 11, 12, 14, 15, 16, 18, 19, 21, 22, 25, 26, 36, 44, 45, 47, 50, 60, 62, 65, 76, 77, 88, 113, 116]


def test_lit_seeds_cover_every_kind():
    kinds = [fs.draw_lit(s)["kind"] for s in LIT_SEEDS]
    assert all(kinds.count(k) >= 2 for k in fs.KINDS), {k: kinds.count(k) for k in fs.KINDS}
    assert {fs.draw_lit(s)["sky"][12] for s in LIT_SEEDS} == set(fs.SHARPNESS)
    assert {float(v) for s in LIT_SEEDS for v in fs.draw_lit(s)["table"][:, 7]} == set(SHININESS)
    sc, plain = fs.draw_lit(7), fs.draw(7)                        # draw(seed) is the scene underneath
    assert np.array_equal(sc["spheres"], plain["spheres"]) and np.array_equal(sc["table"][:, :6], plain["table"]) and sc["hseed"] == plain["hseed"]


@pytest.mark.parametrize("seed", LIT_SEEDS)
def test_random_lit_scene_vs_oracle(renderer, oracle, seed):
    sc = fs.draw_lit(seed)
    _check(renderer, oracle, sc, f"seed {seed} ({sc['kind']}, S={sc['spheres'].shape[1]}, depth {sc['depth']}, aa {sc['aa']})", fs.LIT)


# ---------------------------------------------------------------------------------------------------------------------
# Texture edges

def test_64_textures_every_one_used(renderer, oracle):
    """T = RT_MAX_TEXTURES: an 8 x 8 wall of spheres, each with a texture of its own (random dimensions, skewed axes)."""
    rng = np.random.default_rng(64)
    yy, zz = np.meshgrid(np.arange(8) - 3.5, np.arange(8) - 3.5)
    sp = np.zeros((7, 64), np.float32)
    sp[0], sp[1], sp[2], sp[3] = 9.0, yy.reshape(-1) * 1.1, zz.reshape(-1) * 0.65 + 3.0, 0.3
    sp[4:7] = rng.integers(0, 256, (3, 64))
    recs, first = [], 0
    for k in range(64):
        dims = tuple(int(v) for v in rng.choice([1, 2, 3, 5], 3))
        recs.append((rng.uniform(-1, 1, 3), rng.normal(size=(3, 3)) * 6.0, dims, first))
        first += dims[0] * dims[1] * dims[2]
    texels = rng.integers(0, 256, (first, 3)).astype(np.float32)
    sc = _base(64, 48, spheres=sp, sid=(np.arange(64) % 4).astype(np.int32), depth=2)
    sc["textures"] = (recs, np.arange(64, dtype=np.int32), np.array([-1], np.int32), texels)
    assert sorted(sc["textures"][1].tolist()) == list(range(64))
    r8, _ = _check(renderer, oracle, sc, "T = 64", ("textures",))
    flat = {**sc, "sid": np.full(64, 4, np.int32), "depth": 0}   # amb 1, no light: a hit pixel is its texel.  Every sphere shows one
    f8 = fs.oracle_frame(oracle, flat)[0]
    own = [set(map(tuple, texels[r[3]: r[3] + r[2][0] * r[2][1] * r[2][2]][:, [0, 2, 1]].astype(np.uint8).tolist())) for r in recs]
    seen = set(map(tuple, f8.reshape(3, -1).T.tolist()))
    assert sum(bool(o & seen) for o in own) >= 60


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_texture_dimension_4096(renderer, oracle, axis):
    """RT_MAX_TEXTURE_DIM cells along each grid axis in turn, some 800 cells per world unit: the wrap passes 4095 -> 0."""
    dims = [1, 1, 1]
    dims[axis] = 4096
    axes = np.zeros((3, 3))
    axes[axis] = (37.0, 800.0, -113.0)
    sc = _one_texture(_base(), (0.3, -7.0, 0.2), axes, dims, seed=axis)
    _check(renderer, oracle, sc, f"dim 4096 on axis {axis}", ("textures",))
    from python_ray_tracer_amd.scene import texel_index
    pts = np.stack([np.full(200, 4.0), np.linspace(-3, 3, 200), np.full(200, -0.5)], axis=1)      # points of the floor in view
    idx = texel_index(pts, (0.3, -7.0, 0.2), axes, dims)
    assert idx.min() < 400 and idx.max() > 3700                    # (the texture's whole range lies in the frame)


def test_texture_of_all_2_22_texels(renderer, oracle):
    """One 4096 x 1024 x 1 texture over RT_MAX_TEXELS texels on a wall facing the camera, material 'flat' (amb 1, nothing else),
    so that a pixel is its texel: texel i holds the colour (i & 255, (i >> 8) & 255, i >> 16), and the oracle's uint8 frame names
    the texels it read.  Some lie in the first and some in the last hundredth of the array."""
    n = 1 << 22
    i = np.arange(n)
    texels = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=1).astype(np.float32)
    w, h = 256, 64
    pl = np.array([[6.0, 0, 0, -1, 0, 0, 9, 9, 9]], np.float32).T.copy()
    sc = _base(w, h, spheres=np.zeros((7, 0), np.float32), sid=np.zeros(0, np.int32), planes=pl, pid=np.array([4], np.int32), depth=1)
    axes = np.array([[0.0, 0.0, 700.0], [0.0, 80.0, 0.0], [0.0, 0.0, 0.0]])      # some 4800 columns and 2200 rows across the frame
    sc = _one_texture(sc, (6.0, -3.0, -2.96), axes, (4096, 1024, 1), texels=texels)
    r8, _ = _check(renderer, oracle, sc, "2^22 texels", ("textures",))
    px = r8.reshape(3, -1).T.astype(np.int64)                      # stored order (R, B, G)
    got = px[:, 0] | (px[:, 2] << 8) | (px[:, 1] << 16)
    assert (got < n // 100).sum() >= 5 and (got >= n - n // 100).sum() >= 5, (int(got.min()), int(got.max()))
    assert len(np.unique(got)) > w * h // 2


def test_overlapping_texel_ranges(renderer, oracle):
    """Two textures that share texels 8..15 (first 0 and first 8, 16 texels each), one on the spheres and one on the floor."""
    texels = np.random.default_rng(8).integers(0, 256, (24, 3)).astype(np.float32)
    recs = [((0.0, 0.0, 0.0), np.eye(3) * 1.7, (4, 4, 1), 0), ((0.1, 0.2, 0.3), np.eye(3) * 2.3 + 0.4, (2, 2, 4), 8)]
    sc = _base(textures=(recs, np.array([0, 1, 0, 1], np.int32), np.array([1], np.int32), texels))
    _check(renderer, oracle, sc, "overlapping ranges", ("textures",))


def _flat_counts(oracle, sc, texels):
    """How many pixels of the oracle's depth-0 frame show each texel when every object is 'flat' (amb 1: the pixel is the texel)."""
    S, P = sc["spheres"].shape[1], sc["planes"].shape[1]
    f8 = fs.oracle_frame(oracle, {**sc, "sid": np.full(S, 4, np.int32), "pid": np.full(P, 4, np.int32), "depth": 0, "sky": None})[0]
    px = f8.reshape(3, -1).T
    return [int((px == t[[0, 2, 1]].astype(np.uint8)).all(axis=1).sum()) for t in texels]


def test_texture_axes_hit_both_clamps(renderer, oracle):
    """Axes of 1e12 cells per world unit through the middle of the view: f leaves [-2^30, 2^30 - 1] on both sides, and the
    clamped indices take the texels -2^30 mod 3 = 2 and (2^30 - 1) mod 3 = 0 (mod 2: 0 and 1)."""
    texels = np.array([[250, 10, 10], [10, 250, 10], [10, 10, 250], [240, 240, 10], [10, 240, 240], [240, 10, 240]], np.float32)
    axes = np.array([[0.0, 1e12, 0.0], [0.0, 0.0, -1e12], [0.0, 0.0, 0.0]])
    sc = _one_texture(_base(), (4.0, 0.1, 0.4), axes, (3, 2, 1), texels=texels)
    counts = _flat_counts(oracle, sc, texels)
    assert counts[1] == counts[4] == 0 and min(counts[0], counts[2], counts[3], counts[5]) >= 20, counts   # only the clamped cells
    _check(renderer, oracle, sc, "both clamps", ("textures",))


def test_texture_nan_coordinate(renderer, oracle):
    """An origin and an axis near 1e308 with mixed signs: the products overflow to -inf and +inf, g is NaN and takes the index
    -2^30 mod n, here 2 of 3 and 6 of 7."""
    texels = np.random.default_rng(5).integers(0, 256, (21, 3)).astype(np.float32)
    axes = np.array([[1e308, 1e308, 0.0], [-1.5e308, 0.0, 1.5e308], [0.0, 0.0, 0.0]])
    sc = _one_texture(_base(), (1e308, -1e308, 1.2e308), axes, (3, 7, 1), texels=texels)
    counts = _flat_counts(oracle, sc, texels)
    at = 6 * 3 + 2
    assert counts[at] >= 200 and sum(counts) == counts[at], counts   # every hit reads texel (2, 6)
    _check(renderer, oracle, sc, "NaN coordinate", ("textures",))


def test_texture_on_exact_cell_boundaries(renderer, oracle):
    """The floor z = -0.5 under a texture whose third axis has its cell boundary at z = -0.5: the hit point's z is -0.5 to
    rounding (the camera's z = 0.3 is not a binary fraction), so g is -ulp, 0 or +ulp, and floor(g) decides between two texels
    pixel by pixel; and a grid of power-of-two cells with the spheres' centres on its boundaries."""
    texels = np.array([[250, 20, 20], [20, 20, 250]], np.float32)
    sc = _one_texture(_base(64, 48, cam_origin=np.array([0.0, 0.0, 0.3])), (0.0, 0.0, -0.5), np.array([[0, 0, 0], [0, 0, 0], [0.0, 0.0, 1.0]]), (1, 1, 2), texels=texels,
                      spheres=False)
    counts = _flat_counts(oracle, sc, texels)
    assert min(counts) >= 5, counts                                # both sides of the boundary occur
    _check(renderer, oracle, sc, "floor on a cell boundary", ("textures",))
    sc = _one_texture(_base(64, 48), (4.0, -1.25, 0.5), np.eye(3) * 4.0, (2, 2, 2), seed=3)
    _check(renderer, oracle, sc, "power-of-two cells", ("textures",))


def test_texels_at_reflected_refracted_and_scattered_hits(renderer, oracle):
    """A textured glass sphere, a textured rough floor and a textured window plane at depth 4, beside an untextured mirror: texels
    are read at reflected, refracted and scattered hits.  At least 5 pixels whose primary hit has no texture change with the
    textures (they do not at depth 0)."""
    sc = _base(64, 48, depth=4)
    sc["planes"] = np.concatenate([sc["planes"], np.array([[1.5, 0, 0, 1, 0.05, 0.02, 120, 140, 200]], np.float32).T], axis=1)
    sc["pid"] = np.array([2, 3], np.int32)                        # the floor rough, the window glass
    rng = np.random.default_rng(4)
    recs = [((0.0, 0.0, 0.0), rng.normal(size=(3, 3)) * 3.0, (3, 2, 2), 0), ((0.2, 0.1, 0.0), np.eye(3) * 2.5, (2, 2, 1), 12),
            ((0.0, 0.3, 0.1), rng.normal(size=(3, 3)) * 5.0, (5, 1, 3), 16)]
    texels = rng.integers(0, 256, (31, 3)).astype(np.float32)
    sc["textures"] = (recs, np.array([0, -1, -1, -1], np.int32), np.array([1, 2], np.int32), texels)
    r8, _ = _check(renderer, oracle, sc, "texels at depth 4", ("textures", "glass", "rough"))
    off4 = fs.oracle_frame(oracle, fs.strip(sc, "textures"))[0]
    nowin = {**sc, "textures": (recs, sc["textures"][1], np.array([1, -1], np.int32), texels)}      # the window untextured:
    n8 = fs.oracle_frame(oracle, nowin)[0]                                                          # what is seen through it
    assert ((n8 != off4).any(axis=0)).sum() >= 5
    d0 = fs.oracle_frame(oracle, {**nowin, "depth": 0})[0]
    d0off = fs.oracle_frame(oracle, fs.strip({**nowin, "depth": 0}, "textures"))[0]
    assert not (d0 != d0off).any()                                 # (every primary hit is the window, which has no texture there)


def test_textures_with_typed_bias(renderer, oracle):
    """RT_FLAG_TYPED_BIAS on textured planes: the lookup at the unbiased point, the shading at the float64-biased one."""
    sc = fs.draw_lit(49, w=48, h=32, kind="window")
    sc["pid"] = np.array([3, 2], np.int32)
    sc["textures"] = (sc["textures"][0], sc["textures"][1], np.array([0, len(sc["textures"][0]) - 1], np.int32), sc["textures"][3])
    sc.update(depth=4, aa=0, typed=1)
    _, r32 = _check(renderer, oracle, sc, "typed bias", fs.LIT)
    _, u32 = fs.oracle_frame(oracle, {**sc, "typed": 0})
    assert (u32.view(np.uint32) != r32.view(np.uint32)).any(axis=0).sum() >= 5


# ---------------------------------------------------------------------------------------------------------------------
# Lighting edges

def test_every_shininess_in_one_table(renderer, oracle):
    """Eleven glossy spheres, shin = 1, 2, 4, ..., 1024 in one table, each lit by three coloured lights."""
    sp = np.zeros((7, 11), np.float32)
    sp[0], sp[1], sp[2], sp[3] = 6.0, (np.arange(11) % 4 - 1.5) * 1.6, (np.arange(11) // 4) * 1.3 - 0.6, 0.6
    sp[4:7] = np.random.default_rng(11).integers(0, 256, (3, 11))
    table = np.tile(TABLE[0], (11, 1))
    table[:, 6], table[:, 7] = 180.0, SHININESS
    sc = _base(64, 48, spheres=sp, sid=np.arange(11, dtype=np.int32), table=table, pid=np.array([0], np.int32), depth=1)
    r8, _ = _check(renderer, oracle, sc, "every shin", ("lighting",))
    for k in range(11):                                            # each exponent changes pixels of its own
        t = table.copy()
        t[k, 7] = SHININESS[(k + 5) % 11]
        assert (fs.oracle_frame(oracle, {**sc, "table": t})[0] != r8).any(axis=0).sum() >= 5, SHININESS[k]


def test_64_coloured_area_lights_n16(renderer, oracle):
    """L = RT_MAX_LIGHTS coloured lights with mixed zero and nonzero radii, n = RT_MAX_SHADOW_SAMPLES: spec_n = spec / 16."""
    rng = np.random.default_rng(6416)
    li = rng.uniform(-4, 6, (3, 64)).astype(np.float32)
    li[2] = np.abs(li[2]) + 2.0
    rad = (rng.uniform(0.1, 0.8, 64) * (rng.uniform(size=64) < 0.6)).astype(np.float32)
    rad[63] = 0.6
    rgb = (rng.uniform(0, 0.12, (64, 3)) * (rng.uniform(size=(64, 3)) < 0.8)).astype(np.float32)
    sc = _base(24, 16, lights=li, radius=rad, n=16, light_rgb=rgb, depth=1)
    _check(renderer, oracle, sc, "64 area lights, n = 16", ("lighting", "soft"))
    whole = fs.oracle_frame(oracle, sc, wrong=oracle.WRONG["spec_whole"])[0]
    assert (whole != fs.oracle_frame(oracle, sc)[0]).any(axis=0).sum() >= 5      # (spec / n, not spec, is what the frame shows)


@pytest.mark.parametrize("edge", ["spec_underflows", "spec_clips", "lamb_not_positive", "black_light"])
def test_lighting_edge(renderer, oracle, edge):
    sc = _base(radius=np.array([0.4, 0.0, 0.3], np.float32), n=16)
    t = sc["table"]
    if edge == "spec_underflows":
        # spec / 16 underflows to 0: the header argues that deciding on spec_n > 0 (the kernels) or on spec > 0 (the oracle) gives the
        # same bytes; rows of lamb 0 make the highlight the only reason for those surfaces' shadow queries
        t[:, 6] = (5e-324, 1e-323, 5e-324, 2e-323, 0.0)
        t[0, 1] = 0.0
        assert (t[:4, 6] > 0).all() and (t[:4, 6] / 16.0 == 0.0).all()
    elif edge == "spec_clips":
        t[:, 6] = (1e4, 3e3, 1e5, 1e4, 0.0)
        r8 = fs.oracle_frame(oracle, sc)[0]
        assert ((r8 == 255).all(axis=0)).sum() >= 5                # highlights beyond 255 in every channel
    elif edge == "lamb_not_positive":
        t[0, 1], t[2, 1] = 0.0, -0.3                               # lamb <= 0 with spec > 0: wantS alone asks for the query
        dark = fs.oracle_frame(oracle, {**sc, "table": np.where(np.arange(8) == 6, 0.0, t)})[0]
        assert (dark != fs.oracle_frame(oracle, sc)[0]).any(axis=0).sum() >= 20
    else:
        sc["light_rgb"][1] = 0.0                                   # e = (0, 0, 0) among coloured ones
        lit = fs.oracle_frame(oracle, {**sc, "light_rgb": _base()["light_rgb"]})[0]
        assert (lit != fs.oracle_frame(oracle, sc)[0]).any(axis=0).sum() >= 20
    _check(renderer, oracle, sc, edge, ("lighting",))


def test_highlight_in_a_mirror_and_through_glass(renderer, oracle):
    """White lights, and one glossy ball (the only row with spec > 0) between the mirror and the glass sphere: its highlight shows
    at pixels whose primary hit is another object (they do not change at depth 0)."""
    sc = _base(96, 64, light_rgb=np.ones((3, 3), np.float32), depth=3)
    sc["table"][:, 6] = 0.0
    sc["table"] = np.concatenate([sc["table"], [[0.02, 0.3, 0.0, 0.0, 1.0, 0.0, 900.0, 4.0]]])
    sc["spheres"] = np.concatenate([sc["spheres"], np.array([[5.6, -0.3, 0.9, 0.45, 220, 40, 40]], np.float32).T], axis=1)
    sc["sid"] = np.array([3, 1, 2, 0, 5], np.int32)
    r8, _ = _check(renderer, oracle, sc, "highlight in a mirror and through glass", ("lighting", "glass"))
    off = fs.oracle_frame(oracle, fs.strip(sc, "lighting"))[0]
    d0 = (fs.oracle_frame(oracle, {**sc, "depth": 0})[0] != fs.oracle_frame(oracle, fs.strip({**sc, "depth": 0}, "lighting"))[0]).any(axis=0)
    assert ((r8 != off).any(axis=0) & ~d0).sum() >= 5


# ---------------------------------------------------------------------------------------------------------------------
# Sky edges

@pytest.mark.parametrize("sharp, halo_shin", [(1.0, 1.0), (2.0, 1024.0), (4.0, 8.0), (8.0, 64.0), (16.0, 2.0)])
def test_sky_every_sharp(renderer, oracle, sharp, halo_shin):
    """Each sharp with several halo exponents, up and sun_dir off the axes, over the base scene (mirror, glass, rough floor)."""
    k = SKY.copy()
    k[12], k[23] = sharp, halo_shin
    sc = _base(sky=k)
    r8, _ = _check(renderer, oracle, sc, f"sharp {sharp} halo_shin {halo_shin}", ("sky",))
    for at, v in ((12, 16.0 if sharp != 16.0 else 1.0), (23, 1024.0 if halo_shin != 1024.0 else 1.0)):
        k2 = k.copy()
        k2[at] = v
        assert (fs.oracle_frame(oracle, {**sc, "sky": k2})[0] != r8).any(axis=0).sum() >= 5, at


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_sky_camera_along_up(renderer, oracle, sign):
    """The camera looks along +up / -up: a = |h| reaches 1 at the frame's centre (and the clamp a > 1 by rounding)."""
    k = SKY.copy()
    k[0:3] = (sign, 0.0, 0.0)
    sc = _base(31, 21, sky=k, spheres=_base()["spheres"][:, :2], sid=np.array([3, 1], np.int32))
    _check(renderer, oracle, sc, f"camera along {sign:+.0f} up", ("sky",))


def _primary_direction(oracle, sc, x, y):
    px, y0, dy, z0, dz = sc["raygen"]
    return oracle.normalize(np.array([px, x * dy + y0, y * dz + z0]))          # (cam_rot is the identity: v = P exactly)


@pytest.mark.parametrize("which", ["above_one", "below_minus_one", "attained"])
def test_sky_sun_cos(renderer, oracle, which):
    """sun_cos > 1 (no disc), < -1 (the disc everywhere), and equal to dot(d, sun_dir) of one pixel's ray: that pixel has the sun
    (s >= sun_cos), and loses it when sun_cos is one ulp larger."""
    k = SKY.copy()
    sc = _base(40, 30, spheres=np.zeros((7, 0), np.float32), sid=np.zeros(0, np.int32), sky=k, depth=0)
    assert np.array_equal(sc["cam_rot"], np.eye(3))
    x, y = 31, 9
    d = _primary_direction(oracle, sc, x, y)
    s = (d[0] * k[13] + d[1] * k[14]) + d[2] * k[15]
    k[16] = dict(above_one=1.0 + 2.0 ** -52, below_minus_one=-1.5, attained=float(s))[which]
    r8, r32 = _check(renderer, oracle, sc, f"sun_cos {which}", ("sky",))
    nosun = fs.oracle_frame(oracle, {**sc, "sky": np.where(np.arange(24) == 16, 2.0, k)})[0]
    sun = (r8 != nosun).any(axis=0)
    sky_px = int((fs.oracle_frame(oracle, fs.strip(sc, "sky"))[0] != r8).any(axis=0).sum())
    if which == "above_one":
        assert not sun.any()
    elif which == "below_minus_one":
        assert sun.sum() >= sky_px - 5 and sky_px >= 100           # (a pixel whose colour clips already may not change)
    else:
        assert 0.5 < s < 1.0 and sun[x, y] and 5 <= sun.sum() < sky_px
        k2 = k.copy()
        k2[16] = np.nextafter(s, 2.0)
        lost = fs.oracle_frame(oracle, {**sc, "sky": k2})[1]
        assert (lost[:, x, y] != r32[:, x, y]).any() and np.array_equal(lost[:, x, y], fs.oracle_frame(oracle, {**sc, "sky": np.where(np.arange(24) == 16, 2.0, k)})[1][:, x, y])


@pytest.mark.parametrize("depth", [0, 3])
def test_sky_over_an_empty_scene(renderer, oracle, depth):
    """No sphere and no plane: every sample is sky(d) of its primary ray, whatever the depth."""
    sc = _base(33, 17, spheres=np.zeros((7, 0), np.float32), sid=np.zeros(0, np.int32), planes=np.zeros((9, 0), np.float32),
               pid=np.zeros(0, np.int32), sky=SKY.copy(), depth=depth, aa=1)
    r8, _ = _check(renderer, oracle, sc, f"empty scene, depth {depth}", ("sky",))
    assert r8.any(axis=0).all()


@pytest.mark.parametrize("kind, seed", [("mirror16", 26), ("mirror16", 32), ("tir", 16), ("tir", 19), ("grazing", 12), ("grazing", 44)])
def test_sky_in_mirrors_glass_and_grazing_floors(renderer, oracle, kind, seed):
    """The sky in refl = 1 mirrors at depth 16 (bounces 9 to 16 change the frame), behind total internal reflection (a camera
    inside ior 2.4 glass) and over a rough floor at a grazing angle (scattered rays that leave the scene; absorbed ones add
    nothing), all under a lens."""
    sc = fs.draw_lit(seed)
    assert sc["kind"] == kind and sc["lens"][0] > 0
    if kind == "mirror16":
        assert sc["depth"] == 16
        d16, d8 = fs.oracle_frame(oracle, sc)[0], fs.oracle_frame(oracle, {**sc, "depth": 8})[0]
        assert (d16 != d8).any(axis=0).sum() >= 20
    features = {"mirror16": ("sky", "lens"), "tir": ("sky", "glass", "lens"), "grazing": ("sky", "rough", "lens")}[kind]
    r8, _ = _check(renderer, oracle, sc, f"{kind} seed {seed}", features)
    flat = fs.oracle_frame(oracle, sc, wrong=oracle.WRONG["sky_flat"])[0]
    assert (flat != r8).any(axis=0).sum() >= 5                     # the sky arrives weighted with W_b, b >= 1


def test_lit_scene_size_limits_sampled(renderer, oracle):
    """S = 1024, P = 64, L = 64 coloured lights with radii, M = 256 rows of 8 columns with ids over every row, T = 64 textures with
    every one in use, a sky and a lens: sampled pixels (render_pixels)."""
    rng = np.random.default_rng(2048)
    S, P, NL, M, T = 1024, 64, 64, 256, 64
    sp = np.zeros((7, S), np.float32)
    sp[0] = rng.uniform(2, 14, S)
    sp[1:3] = rng.uniform(-6, 6, (2, S))
    sp[3] = rng.uniform(0.05, 0.35, S)
    sp[4:7] = rng.integers(0, 256, (3, S))
    pl = np.zeros((9, P), np.float32)
    pl[0] = rng.uniform(0, 40, P)
    pl[2] = -3.0 - rng.uniform(0, 5, P)
    nrm = rng.normal(size=(3, P)) * 0.03                          # (nearly level floors: the lights above stay visible)
    nrm[2] += 1.0
    pl[3:6] = nrm / np.linalg.norm(nrm, axis=0)
    pl[6:9] = rng.integers(0, 256, (3, P))
    li = rng.uniform(-4, 10, (3, NL)).astype(np.float32)
    li[2] = np.abs(li[2]) + 8
    table = np.zeros((M, 8))
    table[:, 0] = rng.uniform(-0.05, 0.1, M)
    table[:, 1] = rng.uniform(0.003, 0.02, M)                     # (64 lights: small terms, so that the sum does not clip)
    table[:, 2] = rng.uniform(0, 0.8, M)
    table[:, 4] = 1.0
    table[3::5, 2], table[3::5, 3], table[3::5, 4] = 0.0, 0.9, 1.5
    table[4::5, 5] = rng.uniform(0.05, 1.0, len(table[4::5]))
    table[:, 6] = rng.uniform(0, 10, M) * (np.arange(M) % 3 != 0)
    table[:, 7] = [SHININESS[i % 11] for i in range(M)]
    recs, first = [], 0
    for k in range(T):
        dims = tuple(int(v) for v in rng.choice([1, 2, 3, 4], 3))
        recs.append((rng.uniform(-2, 2, 3), rng.normal(size=(3, 3)) * 4.0, dims, first))
        first += dims[0] * dims[1] * dims[2]
    texels = rng.integers(0, 256, (first, 3)).astype(np.float32)
    w, h = 256, 160
    sc = dict(kind="limits", w=w, h=h, spheres=sp, lights=li, planes=pl, table=table, sid=(np.arange(S) * 7 % M).astype(np.int32),
              pid=(np.arange(P) * 5 % M).astype(np.int32), radius=(rng.uniform(0.1, 0.6, NL) * (np.arange(NL) % 3 != 0)).astype(np.float32),
              n=2, lens=(0.05, 6.0), cam_origin=np.zeros(3), cam_rot=np.eye(3), fov=60.0, raygen=raygen_closed_form(w, h, 60.0), depth=3,
              aa=0, flags_aa=0, spp=1, hseed=77, typed=0,
              textures=(recs, (np.arange(S) % (T + 1) - 1).astype(np.int32), (np.arange(P) % T).astype(np.int32), texels),
              light_rgb=(rng.uniform(0, 1.5, (NL, 3)) * (rng.uniform(size=(NL, 3)) < 0.8)).astype(np.float32), sky=SKY.copy())
    assert set(sc["sid"].tolist()) == set(range(M)) and set(sc["textures"][1].tolist()) == set(range(-1, T))
    co = np.stack([rng.integers(0, w, 300), rng.integers(0, h, 300)], axis=1).astype(np.int32)
    _check_sampled(renderer, oracle, sc, "limits", fs.LIT + ("soft", "lens"), co)


# ---------------------------------------------------------------------------------------------------------------------
# Entry points

def test_lit_render_device_and_odd_column_slabs(renderer, oracle):
    """rt_render_device into a full frame, and slabs [x0, x1) at odd offsets in all three AA modes against the oracle on [x0, x1)."""
    sc = fs.draw_lit(25, w=53, h=29)
    sc.update(aa=1, flags_aa=0)
    r8, r32 = fs.oracle_frame(oracle, sc)
    _live(oracle, sc, fs.LIT, r8, least=20)
    w, h = sc["w"], sc["h"]
    try:
        fs.gpu_frame(renderer, sc)
        p = renderer.params(*IGNORED.values(), sc["depth"], sc["aa"], spp=sc["spp"], seed=sc["hseed"])
        d8, d32 = renderer.malloc(3 * w * h), renderer.malloc(12 * w * h)
        try:
            renderer.render_device(p, 0, w, d8, d32, w * h)
            renderer.sync()
            g8, g32 = np.empty((3, w, h), np.uint8), np.empty((3, w, h), np.float32)
            renderer.d2h(g8, d8)
            renderer.d2h(g32, d32)
        finally:
            renderer.free(d8)
            renderer.free(d32)
        _same("rt_render_device", g8, g32, r8, r32)
        for aa, spp in ((1, 1), (2, 3), (0, 1)):
            for x0, x1 in ((1, 52), (7, 20), (33, 53), (17, 18)):
                s8, s32 = fs.oracle_frame(oracle, {**sc, "aa": aa, "spp": spp}, x0=x0, x1=x1)
                u8, f32 = renderer.render(*IGNORED.values(), sc["depth"], aa, x0=x0, x1=x1, u8=True, f32=True, spp=spp, seed=sc["hseed"])
                _same(f"slab [{x0}, {x1}) aa={aa}", u8, f32, s8[:, x0:x1], s32[:, x0:x1])
    finally:
        renderer.set_lens(0.0, 1.0)


def test_lit_chunked_host_path_half_megapixel(renderer, oracle):
    """rt_render on 1024 x 512 (four column chunks on the host path), sampled pixels against the oracle."""
    sc = fs.draw_lit(12, w=1024, h=512)
    sc.update(raygen=raygen_closed_form(1024, 512, sc["fov"]), aa=0, flags_aa=0, depth=3)
    rng = np.random.default_rng(512)
    co = np.stack([rng.integers(0, 1024, 300), rng.integers(0, 512, 300)], axis=1).astype(np.int32)
    co[:4] = [[0, 0], [1023, 511], [255, 100], [256, 100]]       # the frame's corners and a chunk seam
    _check_sampled(renderer, oracle, sc, "rt_render 0.5 MP", fs.LIT, co)


def test_lit_render_sequence_per_frame_cameras(renderer, oracle):
    """rt_render_sequence with a different camera per frame under a sky and a lens: each frame against the oracle with that
    camera, and consecutive frames differ."""
    sc = fs.draw_lit(47, w=40, h=24)
    sc.update(aa=0, flags_aa=0)
    w, h, n = sc["w"], sc["h"], 3
    from python_ray_tracer_amd.scene.rotation import euler_rotation
    cams = []
    for i in range(n):
        o = np.asarray(sc["cam_origin"]) + np.array([0.0, 0.1 * i, 0.05 * i]) * float(sc["spheres"][3].mean())
        R = np.asarray(euler_rotation(2.0 * i, -3.0 * i, 5.0 * i), np.float64) @ np.asarray(sc["cam_rot"])
        cams.append(np.concatenate([o, R.reshape(9)]))
    cams = np.array(cams)
    refs = []
    for i in range(n):
        c = {**sc, "cam_origin": cams[i, :3], "cam_rot": cams[i, 3:].reshape(3, 3)}
        refs.append(fs.oracle_frame(oracle, c))
        _live(oracle, c, ("sky", "lens", "textures", "lighting"), refs[i][0])
        assert i == 0 or (refs[i][0] != refs[i - 1][0]).any(axis=0).sum() >= 20
    try:
        fs.gpu_frame(renderer, sc)
        p = renderer.params(*IGNORED.values(), sc["depth"], 0, seed=sc["hseed"])
        npx = w * h
        d8, d32 = renderer.malloc(n * 3 * npx), renderer.malloc(n * 12 * npx)
        try:
            renderer.render_sequence(p, 0, w, n, d8, d32, npx, 3 * npx, cams, None, 0)
            renderer.sync()
            g8, g32 = np.empty((n, 3, w, h), np.uint8), np.empty((n, 3, w, h), np.float32)
            renderer.d2h(g8, d8)
            renderer.d2h(g32, d32)
        finally:
            renderer.free(d8)
            renderer.free(d32)
    finally:
        renderer.set_lens(0.0, 1.0)
    for i in range(n):
        _same(f"rt_render_sequence frame {i}", g8[i], g32[i], *refs[i])
