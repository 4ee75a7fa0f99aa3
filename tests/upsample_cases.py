"""The frame pairs of the guided-upsampling tests (test_upsample.py on the CPU, test_gpu_upsample.py on the device): the stored
scenes of test_denoise.guide_scene seen through closed-form grids of two sizes (conftest.raygen_closed_form: the same field of view),
their guides from denoise.guides_reference, random finite sums from a seed, and upsample_reference's answer, each computed once and
read-only.  A plain helper module like temporal_cases.py: nothing here is collected.

PAIRS lists (scene, (wl, hl), (w, h)).  With normal_cos 0.9 the pixels of kind 0 / 1 / 2 are COUNTS; every stage is reached, and
pair() asserts that each kind occurs on the pairs of the two large scenes, so a change of fixtures cannot empty a stage unnoticed."""
import numpy as np

from conftest import raygen_closed_form
from test_denoise import guide_scene

from python_ray_tracer_amd import denoise as D, upsample as U

PAIRS = (("c4_s64_d5_sub32", (32, 32), (64, 64)), ("c4_s64_d5_sub32", (32, 32), (97, 71)), ("c5_s256_d8_sub96", (32, 32), (64, 64)),
         ("c5_s256_d8_sub96", (13, 11), (37, 29)), ("odd_37x29", (37, 29), (74, 58)), ("texture_default_64_d4", (40, 24), (80, 48)))
SMALLEST = PAIRS[3]
TEXTURED = PAIRS[5]
# kind 0 / 1 / 2 at normal_cos 0.9 (and 0.5 for the first pair)
COUNTS = {PAIRS[0]: (3977, 109, 10), PAIRS[1]: (6697, 176, 14), PAIRS[2]: (3552, 505, 39), PAIRS[3]: (617, 307, 149), PAIRS[4]: (4288, 3, 1),
          PAIRS[5]: (80 * 48, 0, 0)}
COUNTS_COS_HALF = (4083, 3, 10)
PASSES = (1, 7)

_GUIDES, _PAIRS, _WANT = {}, {}, {}


def guides(name, w, h):
    """(guides_reference of the scene at w x h, its closed-form grid), computed once."""
    if (name, w, h) not in _GUIDES:
        g, _, _, tex = guide_scene(name)
        rg = raygen_closed_form(w, h, float(g["fov"]))
        a = D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h, raygen=rg, textures=tex)
        a.setflags(write=False)
        _GUIDES[(name, w, h)] = (a, rg)
    return _GUIDES[(name, w, h)]


def sums(wl, hl, n, seed, planes=3):
    """A random finite sum of n passes, float64 (planes, wl, hl): colours 0..400 per pass, a few exact zeros."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 400.0 * n, (planes, wl, hl))
    s[:, rng.integers(0, wl, 3), rng.integers(0, hl, 3)] = 0.0
    return s


def kinds(kind):
    return tuple(int((kind == k).sum()) for k in (0.0, 1.0, 2.0))


def pair(p):
    """dict(lo_guides, hi_guides, lo_grid, hi_grid, wl, hl, w, h) of a row of PAIRS."""
    if p not in _PAIRS:
        name, (wl, hl), (w, h) = p
        (lg, lrg), (hg, hrg) = guides(name, wl, hl), guides(name, w, h)
        _PAIRS[p] = dict(name=name, lo_guides=lg, hi_guides=hg, lo_grid=lrg, hi_grid=hrg, wl=wl, hl=hl, w=w, h=h)
        if name.startswith(("c4_", "c5_")):
            got = kinds(want(p, 1, 0)[1])
            assert all(got), (p, got)
    return _PAIRS[p]


def want(p, n, demodulate, normal_cos=0.9, planes=3):
    """(out, kind) of upsample_reference on sums(..., seed by the pair's index) of a row of PAIRS, computed once."""
    key = (p, n, demodulate, normal_cos, planes)
    if key not in _WANT:
        f = pair(p)
        s = sums(f["wl"], f["hl"], n, 31 + PAIRS.index(p), planes)
        out, kind = U.upsample_reference(s, n, f["lo_guides"], f["hi_guides"], f["lo_grid"], f["hi_grid"], normal_cos, demodulate)
        for a in (s, out, kind):
            a.setflags(write=False)
        _WANT[key] = (out, kind, s)
    return _WANT[key]


def synthetic(wl, hl, w, h, seed):
    """Guides that come from no scene, for frames too large to trace in numpy: ids in diagonal bands (-1 among them), unit normals that
    turn slowly, albedos 0..255; the high frame's from the same functions of the position in the field.  Returns (lo_guides, hi_guides,
    lo_grid, hi_grid)."""
    lo_grid = (2.0, 1.0, -2.0 / max(wl - 1, 1), 1.0, -2.0 / max(hl - 1, 1))
    hi_grid = (2.0, 1.0, -2.0 / max(w - 1, 1), 1.0, -2.0 / max(h - 1, 1))

    def make(nx, ny, grid):
        u = (np.arange(nx) * grid[2] + grid[1])[:, None]
        v = (np.arange(ny) * grid[4] + grid[3])[None, :]
        g = np.zeros((8, nx, ny), np.float32)
        ang = 3.0 * u + 2.0 * v
        g[0], g[1], g[2] = np.cos(ang) * 0.6, np.sin(ang) * 0.6, 0.8
        g[3] = 1.0
        for c in range(3):
            g[4 + c] = 128.0 + 120.0 * np.sin((5.0 + c) * u - (3.0 + c) * v + seed)
        g[7] = np.floor((u + 1.0) * 3.7 + (v + 1.0) * 2.9) % 5.0 - 1.0
        return g

    return make(wl, hl, lo_grid), make(w, h, hi_grid), lo_grid, hi_grid
