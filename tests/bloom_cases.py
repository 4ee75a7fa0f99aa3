"""Inputs of the bloom tests (tests/test_bloom.py on the CPU, tests/test_gpu_bloom.py on the device): film sums with highlights that
a wrong tap would show in, and the frames both files walk.  Not test_film's synthetic_sums: its 1e200 pixels would put a glow of
1e198 on every pixel and round every other tap away."""
import numpy as np

# smaller than a tile, smaller than a halo, not a multiple of the 32 x 64 tile, several tiles in both directions
FRAMES = ((1, 1), (33, 1), (1, 33), (5, 300), (37, 29), (64, 64), (97, 71))
THRESHOLD = 255.0

_SUMS = {}


def bloom_sums(ws, h, n, seed=0):
    """float64 (3, ws, h) sums of n passes: uniform on 0..300 n, a tenth exact zeros, one element in fifty slightly negative, and about
    one pixel in 200 a highlight of 1e4 n in all three channels (scaled per channel, so that it has a hue).  Cached: callers do not
    write into the result."""
    key = (ws, h, n, seed)
    if key not in _SUMS:
        rng = np.random.default_rng([ws, h, n, seed])
        s = rng.uniform(0.0, 300.0 * n, (3, ws, h))
        s[rng.random((3, ws, h)) < 0.1] = 0.0
        s[rng.random((3, ws, h)) < 0.02] = -0.5 * n
        hot = rng.random((ws, h)) < 1.0 / 200.0
        if ws * h >= 200 and not hot.any():
            hot[ws // 2, h // 2] = True
        s[:, hot] = np.array([1e4, 0.5e4, 0.25e4])[:, None] * n
        s.setflags(write=False)
        _SUMS[key] = s
    return _SUMS[key]


def glowing_share(s, n, threshold=THRESHOLD):
    """The share of the pixels whose brightest channel's mean is above the threshold."""
    return float(((s[:3] / np.float64(n)).max(axis=0) > threshold).mean())


def nonfinite_sums(ws, h, n):
    """bloom_sums with NaN, +Inf, -Inf and 1e200 sprinkled in: for runs that must not fault; values are not compared."""
    s = np.array(bloom_sums(ws, h, n, seed=9))
    rng = np.random.default_rng(17)
    flat = s.reshape(-1)
    at = rng.choice(flat.size, max(4, flat.size // 12), replace=False)
    flat[at] = rng.choice([np.nan, np.inf, -np.inf, 1e200], at.size)
    flat[at[:4]] = [np.nan, np.inf, -np.inf, 1e200]
    return s
