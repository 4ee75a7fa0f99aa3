"""Bloom — the numpy restatement of rt_film_bloom (include/mi355rt.h): bloom_reference is the contract's second statement, as
film.tone_reference and denoise.denoise_reference are.  Film.bloom and resolve(bloom=True) put the kernels behind the film:

    with Film(renderer) as film:
        film.accumulate(params, passes=64)
        film.bloom(threshold=255.0, strength=0.25)     # the mean plus the glow of what is brighter than white
        image, _ = film.resolve(white=400.0, gamma=2, bloom=True)
"""
import numpy as np

from . import _lib as L

THRESHOLD, STRENGTH, LEVELS = 255.0, 0.25, 6      # Film.bloom's defaults: white glows, a quarter of its excess, out to 2^5 * 2 pixels

_K = (0.0625, 0.25, 0.375, 0.25, 0.0625)


def check_bloom(threshold, strength, levels, flags=0):
    """(threshold, strength, levels, flags) as Python numbers, or ValueError: what rt_film_bloom would refuse."""
    threshold, strength, levels, flags = float(threshold), float(strength), int(levels), int(flags)
    if not 0 <= levels <= L.RT_BLOOM_MAX_LEVELS:
        raise ValueError(f"levels must be 0..{L.RT_BLOOM_MAX_LEVELS}, not {levels}")
    if not (np.isfinite(threshold) and threshold >= 0.0):
        raise ValueError(f"threshold must be finite and >= 0, not {threshold!r}")
    if not (np.isfinite(strength) and strength >= 0.0):
        raise ValueError(f"strength must be finite and >= 0, not {strength!r}")
    if flags & ~L.RT_BLOOM_NO_TILES:
        raise ValueError(f"flags may hold RT_BLOOM_NO_TILES only, not {flags:#x}")
    return threshold, strength, levels, flags


def _taps(b, step, axis):
    """T = +0.0; for d = -2..2: the tap at +step*d along `axis`, where it lies inside: T = T + k[d] * b[tap]."""
    T = np.zeros_like(b)
    n = b.shape[axis]
    for d in range(-2, 3):
        o = step * d
        lo, hi = max(0, -o), min(n, n - o)                       # the positions whose tap lies inside
        if lo >= hi:
            continue
        dst = [slice(None)] * b.ndim
        src = [slice(None)] * b.ndim
        dst[axis], src[axis] = slice(lo, hi), slice(lo + o, hi + o)
        T[tuple(dst)] = T[tuple(dst)] + np.float64(_K[d + 2]) * b[tuple(src)]
    return T


def bloom_reference(s, n, threshold=THRESHOLD, strength=STRENGTH, levels=LEVELS):
    """rt_film_bloom in numpy.  s: float64 (3 or more, ws, h), a film sum of n passes (n = 1: a mean); planes 0..2 are read.  Returns
    out, float64 (3, ws, h): the mean plus the glow.  Per pixel p = (x, y) and channel c, float64, no fused multiply-add, in this
    order:
        m_c = s[c][p] / (double)n;      out[c][p] = m_c
        levels == 0:  nothing else is evaluated
        mx = m_0 > m_1 ? m_0 : m_1;   mx = mx > m_2 ? mx : m_2
        mx > threshold:  g = (mx - threshold) / mx;   b_0[c][p] = m_c > 0 ? m_c * g : +0.0        else:  b_0[c][p] = +0.0
        wl = strength / (double)levels   (once)
        for i = 0 .. levels-1:    step = 1 << i;     k = (1/16, 1/4, 3/8, 1/4, 1/16)
            t[c][x,y]       = T after:  T = +0.0;  for d = -2..2:  qx = x + step*d;  0 <= qx < ws:  T = T + k[d] * b_i[c][qx, y]
            b_{i+1}[c][x,y] = B after:  B = +0.0;  for d = -2..2:  qy = y + step*d;  0 <= qy < h:   B = B + k[d] * t[c][x, qy]
            out[c][p] = out[c][p] + wl * b_{i+1}[c][p]"""
    threshold, strength, levels, _ = check_bloom(threshold, strength, levels)
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, not {n}")
    s = np.asarray(s)
    if s.dtype != np.float64 or s.ndim != 3 or s.shape[0] < 3 or s.shape[1] < 1 or s.shape[2] < 1:
        raise ValueError("s must be a float64 array of shape (3 or more, ws, h)")
    with np.errstate(all="ignore"):
        m = s[:3] / np.float64(n)
        out = np.array(m)
        if levels == 0:
            return out
        mx = np.where(m[0] > m[1], m[0], m[1])
        mx = np.where(mx > m[2], mx, m[2])
        bright = mx > np.float64(threshold)
        g = (mx - np.float64(threshold)) / np.where(bright, mx, 1.0)
        b = np.where(bright[None] & (m > 0.0), m * g[None], 0.0)
        wl = np.float64(strength) / np.float64(levels)
        for i in range(levels):
            b = _taps(_taps(b, 1 << i, 1), 1 << i, 2)
            out = out + wl * b
    return out
