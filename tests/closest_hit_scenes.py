"""Scenes and filter inputs built for the paths the stored fixtures do not reach (no tests here: tests/test_closest_hit_scenes.py
holds their conditions on the CPU, tests/test_gpu_closest_hit.py, test_gpu_denoise.py and test_gpu_film.py run them on the GPU).

tie_scene              the equal-distance spheres of tests/golden/tie_break.npz at seeded caller indices among filler spheres, so that
                       the scene is clustered and the packer's spatial sort separates slot order from caller order
coincident_planes_scene  two planes on top of each other under 24 spheres
size_limit_arrays      the generator of test_gpu_features_vs_oracle.test_scene_size_limits_sampled (S = 1024, P = 64, M = 256)
limit_scene            that scene with L lights and textures on every third sphere and every plane
synthetic_guides, synthetic_sums   guides and film sums for the filter that no rendered scene gives
SETTINGS               the closest-hit settings: sphere count, lights, MI355RT_* knobs and the table modes they are there for"""
import os

import numpy as np

from conftest import GOLDEN

from python_ray_tracer_amd.scene import Texture

# ---------------------------------------------------------------------------------------------------------------------
# The tie rule in every table mode.  name: (S, lights, knobs, clustered, the guides kernel's MODE, the render kernel's
# (mode, park, wpw) without AA, the same with an AA mode of its own).  tests/test_closest_hit_scenes.py evaluates rt_plan.h on the
# CPU for every row and holds it to these; the GPU tests hold the library's MI355RT_LOG_KERNELS lines to them.
KNOB_ENV = ("MI355RT_CLUSTER_MINS", "MI355RT_LANES_MINS", "MI355RT_F32_RECORDS", "MI355RT_LANES_PARK", "MI355RT_WPW2_MAX_IMAGE",
            "MI355RT_ORDER_GROUP", "MI355RT_ORDER_TILES", "MI355RT_SEQ_ORDER", "MI355RT_LANES_PRIMARY", "MI355RT_CHUNK_MODE")
BIG = "100000"
SETTINGS = {
    "s36_mode0_clustered":   (36, 3, {}, True, 0, (0, 1, 4), (0, 1, 4)),
    "s64_mode1_clustered":   (64, 3, {}, True, 1, (1, 1, 4), (0, 0, 4)),
    "s64_flat_four_waves":   (64, 3, {"MI355RT_CLUSTER_MINS": BIG}, False, 0, (0, 1, 4), (0, 0, 4)),
    "s256_mode1_flat":       (256, 3, {"MI355RT_CLUSTER_MINS": BIG, "MI355RT_LANES_MINS": BIG}, False, 1, (1, 0, 4), (0, 0, 4)),
    "s256_mode0_clustered":  (256, 3, {"MI355RT_LANES_MINS": BIG, "MI355RT_F32_RECORDS": "0"}, True, 0, (0, 0, 4), (0, 0, 4)),
    "s256_mode2_parked":     (256, 3, {}, True, 2, (2, 1, 4), (3, 1, 4)),
    "s256_mode2_register":   (256, 3, {"MI355RT_LANES_PARK": "0"}, True, 2, (2, 0, 4), (2, 0, 4)),
    "s64_mode2_small":       (64, 3, {"MI355RT_LANES_MINS": "30"}, True, 2, (2, 1, 4), (3, 1, 4)),
    "s1024_no_anchors":      (1024, 3, {}, True, 2, (2, 1, 4), (3, 1, 4)),
    "s1024_anchored":        (1024, 0, {}, True, 2, (2, 0, 4), (2, 0, 4)),
}
TIE_CASES = 6
_TIE = {}


def tie_fixture():
    if not _TIE:
        _TIE.update(np.load(os.path.join(GOLDEN, "tie_break.npz")))
    return _TIE


def tie_scene(case, S, seed, reverse, lights):
    """The 16 equal-distance spheres, grid and camera of case `case` of tests/golden/tie_break.npz (radius 4 around the camera) in a
    scene of S spheres: S - 16 fillers outside that shell (centres 6 to 12 from the origin, radii 0.1 to 0.4, random colours), the
    16 at caller indices drawn from range(S) by the seed and assigned by a seeded permutation, which reverse=True reverses: the
    two spheres of every tie then swap their caller order.  No planes; lights: 0 or 3 point lights far outside (the frames use
    amb 1, lamb 0, refl 0, depth 0, so the lights change no byte, only the anchored cull tables).
    -> dict(spheres (7, S), lights (3, lights), planes (9, 0), cam_origin, cam_rot, pixel_loc (3, 8, 8), tie_at: caller index of
    tie sphere k)"""
    g = tie_fixture()
    tie = g[f"spheres_{case}"]
    K = tie.shape[1]
    assert S >= K and lights in (0, 3)
    rng = np.random.default_rng([seed, S, case])
    sp = np.zeros((7, S), np.float32)
    v = rng.normal(size=(3, S))
    sp[0:3] = v / np.linalg.norm(v, axis=0) * rng.uniform(6.0, 12.0, S)
    sp[3] = rng.uniform(0.1, 0.4, S)
    sp[4:7] = rng.integers(0, 256, (3, S))
    at = np.sort(rng.choice(S, K, replace=False))
    perm = rng.permutation(K)
    if reverse:
        perm = perm[::-1]
    sp[:, at] = tie[:, perm]
    tie_at = np.empty(K, np.int64)
    tie_at[perm] = at
    li = np.array([[-60.0, 40.0, 80.0], [0.0, 90.0, -70.0], [75.0, -50.0, 60.0]], np.float32).T[:, :lights]
    return dict(spheres=sp, lights=np.ascontiguousarray(li), planes=np.zeros((9, 0), np.float32), cam_origin=g[f"cam_origin_{case}"],
                cam_rot=np.eye(3), pixel_loc=g[f"pixel_loc_{case}"], tie_at=tie_at)


UNIFORM_MATERIALS = np.array([[1.0, 0.0, 0.0]])                  # one row (amb, lamb, refl): what the tie frames' scalars say


def uniform_materials(sc):
    return UNIFORM_MATERIALS, np.zeros(sc["spheres"].shape[1], np.int32), np.zeros(sc["planes"].shape[1], np.int32)


def coincident_planes_scene(swap=False):
    """Two planes with the same origin and normal and different colours at indices 0 and 1 (the floor; swap=True swaps the two
    colours), a back wall, 24 spheres above the floor (a clustered scene) and two lights, seen on a 32 x 24 frame.  Of equal
    distances the first wins (trace.py:26): every floor pixel, and every mirror bounce that ends on the floor, shows plane 0."""
    rng = np.random.default_rng(24)
    S = 24
    sp = np.zeros((7, S), np.float32)
    sp[0] = rng.uniform(4.0, 13.0, S)
    sp[1] = rng.uniform(-4.0, 4.0, S)
    sp[3] = rng.uniform(0.3, 0.7, S)
    sp[2] = -3.0 + sp[3] + rng.uniform(0.0, 2.0, S)
    sp[4:7] = rng.integers(30, 256, (3, S))
    colours = ((230.0, 40.0, 60.0), (20.0, 200.0, 120.0))
    a, b = colours[::-1] if swap else colours
    pl = np.array([[0, 0, -3, 0, 0, 1, *a], [0, 0, -3, 0, 0, 1, *b], [18, 0, 0, -1, 0, 0.1, 90, 90, 160]], np.float32).T
    li = np.array([[-2.0, 3.0, 6.0], [6.0, -5.0, 4.0]], np.float32).T
    return dict(spheres=sp, lights=np.ascontiguousarray(li), planes=np.ascontiguousarray(pl), cam_origin=np.zeros(3), cam_rot=np.eye(3),
                w=32, h=24, fov=60.0, shade=(0.1, 0.6, 0.4), depth=2)


# ---------------------------------------------------------------------------------------------------------------------
# The scene-size limits

def size_limit_arrays(rng, S=1024, P=64, NL=64, M=256):
    """The draws of test_scene_size_limits_sampled, in their order: spheres (7, S) in front of the camera, P tilted floors, NL
    lights, a table of M rows of 6 columns with glass and rough rows, ids over every row.  The caller goes on drawing from rng."""
    sp = np.zeros((7, S), np.float32)
    sp[0] = rng.uniform(2, 14, S)
    sp[1:3] = rng.uniform(-6, 6, (2, S))
    sp[3] = rng.uniform(0.05, 0.35, S)
    sp[4:7] = rng.integers(0, 256, (3, S))
    pl = np.zeros((9, P), np.float32)
    pl[0] = rng.uniform(0, 40, P)
    pl[2] = -3.0 - rng.uniform(0, 5, P)
    nrm = rng.normal(size=(3, P)) * 0.2
    nrm[2] += 1.0
    pl[3:6] = nrm / np.linalg.norm(nrm, axis=0)
    pl[6:9] = rng.integers(0, 256, (3, P))
    li = rng.uniform(-4, 10, (3, NL)).astype(np.float32)
    li[2] = np.abs(li[2]) + 3
    table = np.zeros((M, 6))
    table[:, 0] = rng.uniform(-0.05, 0.1, M)
    table[:, 1] = rng.uniform(0.1, 0.9, M)
    table[:, 2] = rng.uniform(0, 0.8, M)
    table[:, 4] = 1.0
    table[3::5, 2], table[3::5, 3], table[3::5, 4] = 0.0, 0.9, 1.5
    table[4::5, 5] = rng.uniform(0.05, 1.0, len(table[4::5]))
    sid = (np.arange(S) * 7 % M).astype(np.int32)
    pid = (np.arange(P) * 5 % M).astype(np.int32)
    return sp, pl, li, table, sid, pid


def three_textures(seed):
    """The three kinds of test_gpu_textures._scene_textures: a checkered floor, a solid checker, a projected image.
    -> (records, texels (N, 3))"""
    rng = np.random.default_rng(seed)
    img = Texture.image(rng.integers(0, 256, (7, 5, 3)), (0.0, -0.3, 0.8), (0.0, 0.9, 0.1), (0.1, 0.0, -0.7))
    tex = [Texture.checker((240, 240, 240), (20, 20, 20), 0.35), Texture.checker((250, 120, 10), (10, 150, 160), 0.12, solid=True), img]
    recs, first = [], 0
    for t in tex:
        recs.append((t.origin, t.axes, t.dims, first))
        first += t.texels.shape[0] * t.texels.shape[1] * t.texels.shape[2]
    return recs, np.concatenate([t.texels.reshape(-1, 3) for t in tex])


def textures_for(S, P, seed):
    """Every third sphere textured, the solid checker and the image in turn; the checkered floor on every plane."""
    recs, texels = three_textures(seed)
    st = np.array([(1 + (i // 3) % 2) if i % 3 == 0 else -1 for i in range(S)], np.int32)
    return recs, st, np.zeros(P, np.int32), texels


LIMIT_W, LIMIT_H = 64, 40
# The 64 tilted floors cut through the cloud of spheres, so from most places some floor fills the view.  This camera stands inside the
# cloud just above every floor and looks nearly level (found by a seeded search over poses): spheres near and far, eight of the
# floors below, and sky in the rows that look up.
LIMIT_CAMERA = (10.8, -3.1, 5.3)
LIMIT_ROTATION = ((0.830822, -0.552599, 0.066107), (0.550858, 0.833447, 0.043831), (-0.079318, 0.0, 0.996849))
LIMIT_RAYGEN = (0.8, 1.3, -2.6 / (LIMIT_W - 1), 1.0, -2.0 / (LIMIT_H - 1))
_LIMIT = {}


def limit_scene(L):
    """S = 1024, P = 64 and L of the 64 lights of size_limit_arrays(default_rng(1024)), its material table, and textures_for it:
    the largest scene the library takes, on a 64 x 40 grid of its own."""
    if L not in _LIMIT:
        sp, pl, li, table, sid, pid = size_limit_arrays(np.random.default_rng(1024))
        for a in (sp, pl, table, sid, pid):
            a.setflags(write=False)
        _LIMIT[L] = dict(spheres=sp, planes=pl, lights=np.ascontiguousarray(li[:, :L]), materials=(table, sid, pid),
                         textures=textures_for(sp.shape[1], pl.shape[1], 1024), cam_origin=np.array(LIMIT_CAMERA), cam_rot=np.array(LIMIT_ROTATION),
                         w=LIMIT_W, h=LIMIT_H, raygen=LIMIT_RAYGEN)
    return _LIMIT[L]


# ---------------------------------------------------------------------------------------------------------------------
# Inputs of the filter

ALBEDOS = np.array([0.0, 0.5, 1.0, 2.0, 255.0, 1e30], np.float32)
BIG_ID = 1087.0                                                  # (1024 spheres + plane 63: the largest id a scene can give)
_GUIDES = {}


def synthetic_guides(ws, h, seed):
    """float32 (8, ws, h) within the contract of rt_film_denoise and unlike any rendered scene's.  Ids in four vertical bands of
    columns: a 1-pixel checkerboard of ids 3 and 7, 3 x 5 blocks of ids 0 to 9, misses (id -1, the other planes +0.0), one id
    >= 1024.  Normals: random unit vectors rounded to float32 per pixel on the upper half of the rows, one constant normal on the
    lower half; on a frame of one row the halves are alternate runs of four columns.  Albedo per pixel and channel from {0, 0.5, 1, 2, 255, 1e30}.  Computed once per argument and read-only."""
    key = (ws, h, seed)
    if key not in _GUIDES:
        rng = np.random.default_rng([seed, ws, h])
        x, y = np.meshgrid(np.arange(ws), np.arange(h), indexing="ij")
        band = np.searchsorted(np.array([ws // 4, ws // 2, 3 * ws // 4]), x, side="right")
        ident = np.select([band == 0, band == 1, band == 2], [np.where((x + y) & 1, 7.0, 3.0), ((x // 3) * 3 + y // 5) % 10, -1.0], BIG_ID)
        g = np.zeros((8, ws, h), np.float32)
        v = rng.normal(size=(3, ws, h))
        v = (v / np.sqrt((v * v).sum(axis=0))).astype(np.float32)
        c = np.array([0.48, -0.6, 0.64], np.float32)
        random_half = y < (h + 1) // 2 if h > 1 else x % 8 < 4       # (one row has no upper half: runs of four columns there)
        g[0:3] = np.where(random_half[None], v, c[:, None, None])
        g[3] = rng.uniform(0.5, 40.0, (ws, h))
        g[4:7] = ALBEDOS[rng.integers(0, len(ALBEDOS), (3, ws, h))]
        g[7] = ident
        g[0:7, ident < 0] = 0.0
        g.setflags(write=False)
        _GUIDES[key] = g
    return _GUIDES[key]


def synthetic_sums(ws, h, n, seed):
    """float64 (3, ws, h) sums of n passes: uniform on 0 to 300 n, a tenth exact zeros, about one in fifty negative down to -4,
    and eight pixels (fewer on a frame of fewer) of 1e200 in every channel: against any other pixel their d2 overflows to inf and the
    colour weight is exactly 0."""
    rng = np.random.default_rng([seed, ws, h, n])
    s = rng.uniform(0.0, 300.0 * n, (3, ws, h))
    s[rng.random((3, ws, h)) < 0.1] = 0.0
    neg = rng.random((3, ws, h)) < 0.02
    s[neg] = -rng.uniform(0.0, 4.0, int(neg.sum()))
    px = rng.choice(ws * h, min(8, ws * h), replace=False)
    s.reshape(3, -1)[:, px] = 1e200
    return s


# (ws, h, levels, normal_shin, sigma, demodulate, n) of every filter launch the GPU tests make on synthetic inputs
DENOISE_SETTINGS = [(0, 32, 0.0, 0, 7), (0, 1, 4.0, 1, 1), (1, 32, 0.0, 0, 1), (1, 4, 0.125, 1, 7), (2, 32, 16.0, 0, 7), (2, 1024, 0.125, 1, 1),
                    (5, 32, 0.125, 1, 7), (5, 2, 0.0, 0, 1), (5, 32, 24.0, 0, 7), (2, 32, 0.0, 1, 7)]       # test_gpu_denoise.SETTINGS
SIX_LEVELS = [(6, 1, 2.0, 0, 3), (6, 1024, 0.125, 1, 3)]
SIX_FRAMES = [(97, 71), (33, 1)]
SYNTHETIC_FRAMES = [(37, 29), (64, 64)]
GRID_CAP_SETTING = (2, 4, 0.125, 1, 3)


def grid_cap_frame(cus):
    """(ws, h) with more pixels than the filter's grid has threads on a device of `cus` compute units: 1031 x 523 for 256."""
    ws, h = 1031, 523
    while ws * h <= 8 * 256 * cus:
        ws += 64
    return ws, h


_FILTERED = {}


def filtered_truth(ws, h, setting, seed=0):
    """(sums, denoise_reference of them) on synthetic_guides(ws, h, seed) for one (levels, shin, sigma, demodulate, n): once."""
    from python_ray_tracer_amd import denoise as D
    key = (ws, h, setting, seed)
    if key not in _FILTERED:
        levels, shin, sigma, dem, n = setting
        s = synthetic_sums(ws, h, n, seed + 1000 * levels + shin)
        out = D.denoise_reference(s, n, synthetic_guides(ws, h, seed), levels, shin, sigma, dem)
        s.setflags(write=False)
        out.setflags(write=False)
        _FILTERED[key] = (s, out)
    return _FILTERED[key]
