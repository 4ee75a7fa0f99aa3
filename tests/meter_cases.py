"""Inputs of the meter tests (tests/test_meter.py on the CPU, tests/test_gpu_meter.py on the device): film sums whose luminances
fill every kind of bin, and the frames and settings both files walk."""
import itertools

import numpy as np

from python_ray_tracer_amd import _lib as L
from python_ray_tracer_amd import meter as M

# one pixel, one thin row, a thin tall frame, odd sizes with a tail of 1, 2 and 3 pixels behind the groups of four, several workgroups
FRAMES = ((1, 1), (33, 1), (5, 300), (37, 29), (64, 64), (97, 71))
PASSES = (1, 7)

# the solve's settings: (key, percentile, min_exposure, max_exposure, rate)
SETTINGS = tuple((key, pct, lo, hi, rate) for key, pct, (lo, hi), rate in
                 itertools.product((46.0, 0.18), (0.0, 0.5, 0.9, 1.0), ((2.0 ** -10, 2.0 ** 10), (0.5, 2.0)), (1.0, 0.25)))
CARRIED = (3.0, 1e-3, 777.0, 5.0)                                 # a state with a usable exposure

_SUMS = {}


def meter_sums(ws, h, n, seed=0):
    """float64 (3, ws, h) sums of n passes.  The luminances are log-uniform over 2^-20 .. 2^28 (both out-of-range bins fill), with a
    hue per pixel; about 5 % of the pixels are exact zeros, some are negative, NaN and +Inf; and where the frame has room, grey pixels
    whose mean is exactly a bin edge or its predecessor: edge(b), nextafter(edge(b), 0).  Cached: callers do not write into it."""
    key = (ws, h, n, seed)
    if key not in _SUMS:
        rng = np.random.default_rng([ws, h, n, seed, 355])
        npx = ws * h
        Y = np.exp2(rng.uniform(-20.0, 28.0, npx))
        hue = rng.uniform(0.25, 1.75, (3, npx))
        m = hue * Y[None] / (0.2126 * hue[0] + 0.7152 * hue[1] + 0.0722 * hue[2])[None]
        kind = rng.random(npx)
        m[:, kind < 0.05] = 0.0
        m[:, (kind >= 0.05) & (kind < 0.07)] *= -1.0
        m[0, (kind >= 0.07) & (kind < 0.08)] = np.nan
        m[1, (kind >= 0.08) & (kind < 0.09)] = np.inf
        edges = M.bin_edges()
        exact = np.concatenate([edges, np.nextafter(edges, 0.0)])
        at = rng.permutation(npx)[:min(npx // 4, exact.size)]
        m[:, at] = rng.permutation(exact)[:at.size][None]            # grey: Y is the value but for the rounding of the weights' sum
        s = (m * np.float64(n)).reshape(3, ws, h)
        s.setflags(write=False)
        _SUMS[key] = s
    return _SUMS[key]


def constant_sums(ws, h, n, value=100.0):
    """A frame whose every pixel has the mean (value, value, value): every lane hits one bin."""
    s = np.full((3, ws, h), value * n, np.float64)
    s.setflags(write=False)
    return s


def kinds(hist):
    """(nothing, below, in range, above) of a histogram."""
    hist = np.asarray(hist)
    return int(hist[0]), int(hist[1]), int(hist[2:L.RT_METER_BINS - 1].sum()), int(hist[L.RT_METER_BINS - 1])
