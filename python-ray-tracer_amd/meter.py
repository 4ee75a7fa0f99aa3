"""Metering — the numpy restatement of rt_film_meter and rt_film_meter_solve (include/mi355rt.h): bin_reference, bin_edges,
histogram_reference and solve_reference are the contract's second statement, as film.tone_reference and bloom.bloom_reference are.
Film.meter and resolve(auto_exposure=True) put the kernels behind the film:

    with Film(renderer) as film:
        film.accumulate(params, passes=16)
        film.meter(key=46.0)                            # histogram of the luminance, the median mapped to 18 % of 255
        image, _ = film.resolve(white=400.0, gamma=2, auto_exposure=True)
        exposure, luminance, pixels, bin_ = film.exposure()
"""
import struct

import numpy as np

from . import _lib as L

# Film.meter's defaults.  Starting points, not measurements: 46 is 18 % of 255 (middle grey), the median is the metered value, and
# the exposure may move ten stops either way.
KEY, PERCENTILE, MIN_EXPOSURE, MAX_EXPOSURE, RATE = 46.0, 0.5, 2.0 ** -10, 2.0 ** 10, 1.0

_K0 = (1023 + L.RT_METER_LO) * L.RT_METER_SUB                 # 8056
_IN_RANGE = L.RT_METER_OCTAVES * L.RT_METER_SUB                # 320


def check_meter(key, percentile, min_exposure, max_exposure, rate):
    """(key, percentile, min_exposure, max_exposure, rate) as Python floats, or ValueError: what rt_film_meter_solve would refuse."""
    key, percentile, lo, hi, rate = float(key), float(percentile), float(min_exposure), float(max_exposure), float(rate)
    if not (np.isfinite(key) and key > 0.0):
        raise ValueError(f"key must be finite and > 0, not {key!r}")
    if not 0.0 <= percentile <= 1.0:
        raise ValueError(f"percentile must be 0..1, not {percentile!r}")
    if not (np.isfinite(lo) and lo > 0.0):
        raise ValueError(f"min_exposure must be finite and > 0, not {lo!r}")
    if not (np.isfinite(hi) and hi > 0.0):
        raise ValueError(f"max_exposure must be finite and > 0, not {hi!r}")
    if lo > hi:
        raise ValueError(f"min_exposure {lo!r} is above max_exposure {hi!r}")
    if not 0.0 < rate <= 1.0:
        raise ValueError(f"rate must be in (0, 1], not {rate!r}")
    return key, percentile, lo, hi, rate


def bin_reference(Y):
    """The bin of every luminance in Y (float64, any shape): int64, the shape of Y.
        !(Y > 0)  (zero, negative, NaN):  bin 0
        else  u = the 64 bits of Y;   k = (int64)(u >> 49) - 8056        (8056 = (1023 + RT_METER_LO) * 8)
              k < 0: bin 1        k >= 320: bin 322  (+Inf included)        else: bin 2 + k"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    with np.errstate(all="ignore"):
        lit = Y > 0.0
    k = (Y.view(np.uint64) >> np.uint64(49)).astype(np.int64) - _K0
    return np.where(lit, np.where(k < 0, 1, np.where(k >= _IN_RANGE, L.RT_METER_BINS - 1, 2 + k)), 0)


def _edge(b):
    return struct.unpack("<d", struct.pack("<Q", (int(b) - 2 + _K0) << 49))[0]


def bin_edges():
    """float64 (321,): entry i is edge(i + 2), the lower edge of bin i + 2 for bins 2..322 (the last is the upper edge of bin 321).
    Bin b is [edge(b), edge(b+1)), where edge(b) is the float64 whose bits are (uint64)(b - 2 + 8056) << 49: (1 + j/8) * 2^E, exact."""
    return np.array([_edge(b) for b in range(2, L.RT_METER_BINS)], np.float64)


def histogram_reference(s, n):
    """rt_film_meter (with reset) in numpy.  s: float64 (3 or more, ws, h), a film sum of n passes (n = 1: a mean); planes 0..2 are
    read.  Returns RT_METER_BINS uint64 counts.  Per pixel p, in float64 without fused multiply-add:
        m_c = s[c][p] / (double)n
        Y = (0.2126 * m_0 + 0.7152 * m_1) + 0.0722 * m_2
        !(Y > 0)  (zero, negative, NaN):  bin 0
        else  u = the 64 bits of Y;   k = (int64)(u >> 49) - 8056        (8056 = (1023 + RT_METER_LO) * 8)
              k < 0: bin 1        k >= 320: bin 322  (+Inf included)        else: bin 2 + k
        hist[bin] = hist[bin] + 1"""
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, not {n}")
    s = np.asarray(s)
    if s.dtype != np.float64 or s.ndim != 3 or s.shape[0] < 3 or s.shape[1] < 1 or s.shape[2] < 1:
        raise ValueError("s must be a float64 array of shape (3 or more, ws, h)")
    with np.errstate(all="ignore"):
        m = s[:3] / np.float64(n)
        Y = (np.float64(0.2126) * m[0] + np.float64(0.7152) * m[1]) + np.float64(0.0722) * m[2]
    return np.bincount(bin_reference(Y).reshape(-1), minlength=L.RT_METER_BINS).astype(np.uint64)


def solve_reference(hist, state, key=KEY, percentile=PERCENTILE, min_exposure=MIN_EXPOSURE, max_exposure=MAX_EXPOSURE, rate=RATE):
    """rt_film_meter_solve in Python floats (IEEE float64, no fused multiply-add).  hist: RT_METER_BINS counts; state: the
    RT_METER_STATE_DOUBLES float64 before the call (zeros: no history).  Returns the new state, float64 (4,).
        N = hist[1] + ... + hist[322]                    (bin 0 is not metered)
        prev = state[0];   usable = prev is finite and > 0
        N == 0:  e = usable ? prev : clamp(1.0);   state = (e, +0.0, 0.0, 0.0);   done
        r = (uint64)(percentile * (double)N);   r > N-1: r = N-1
        b = the smallest bin in 1..322 with C_b > r,  C_b = hist[1] + ... + hist[b];   below = C_{b-1}
        b == 1: Ym = 2^-16     b == 322: Ym = 2^24
        else  lo = edge(b); hi = edge(b+1);  Ym = lo + (hi - lo) * ((double)(r - below) / (double)hist[b])
        t = clamp(key / Ym)                      clamp(v): v < min_exposure ? min_exposure : (v > max_exposure ? max_exposure : v)
        e = (usable and rate < 1) ? clamp(prev + (t - prev) * rate) : t
        state = (e, Ym, (double)N, (double)b)"""
    key, percentile, lo_e, hi_e, rate = check_meter(key, percentile, min_exposure, max_exposure, rate)
    hist = [int(v) for v in np.asarray(hist).reshape(-1)]
    if len(hist) != L.RT_METER_BINS:
        raise ValueError(f"a histogram has RT_METER_BINS = {L.RT_METER_BINS} counts, not {len(hist)}")
    state = np.asarray(state, dtype=np.float64).reshape(-1)
    if state.size != L.RT_METER_STATE_DOUBLES:
        raise ValueError(f"a state has RT_METER_STATE_DOUBLES = {L.RT_METER_STATE_DOUBLES} doubles, not {state.size}")

    def clamp(v):
        return lo_e if v < lo_e else (hi_e if v > hi_e else v)

    N = sum(hist[1:])
    prev = float(state[0])
    usable = bool(np.isfinite(prev) and prev > 0.0)
    if N == 0:
        return np.array([prev if usable else clamp(1.0), 0.0, 0.0, 0.0], np.float64)
    r = min(int(percentile * float(N)), N - 1)
    C = 0
    for b in range(1, L.RT_METER_BINS):
        below = C
        C += hist[b]
        if C > r:
            break
    if b == 1:
        Ym = _edge(2)
    elif b == L.RT_METER_BINS - 1:
        Ym = _edge(L.RT_METER_BINS - 1)
    else:
        lo, hi = _edge(b), _edge(b + 1)
        Ym = lo + (hi - lo) * (float(r - below) / float(hist[b]))
    t = clamp(key / Ym)
    e = clamp(prev + (t - prev) * rate) if usable and rate < 1.0 else t
    return np.array([e, Ym, float(N), float(b)], np.float64)
