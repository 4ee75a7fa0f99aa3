"""Metering on the device (rt_film_meter, rt_film_meter_solve, rt_film_resolve_metered; python-ray-tracer_amd/csrc/rt_meter.h): the
histogram kernel against meter.histogram_reference exactly on tests/meter_cases.py's sums, with odd strides and sentinels in the pads
and beside the counts; slabs without a reset; a reset over poisoned counts; a constant frame; the grid-stride loop; the solve against
meter.solve_reference bit for bit; the metered resolve against rt_film_resolve and against film.tone_reference; every refusal with its
text and an untouched output; through Film on a rendered scene with a sun."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, raygen_closed_form
import meter_cases as mc
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_film import same_bits

from python_ray_tracer_amd import Film, bloom as B, film as F, meter as M
from python_ray_tracer_amd import _lib as L

pytestmark = pytest.mark.gpu

BINS = L.RT_METER_BINS
WORD = np.uint64(0xfeedfacecafebeef)                               # the words beside the counts
POISON = np.full(BINS, np.float64(np.nan)).view(np.uint64)         # counts that hold NaN patterns before a reset

_WANT = {}


def want_of(ws, h, n):
    if (ws, h, n) not in _WANT:
        _WANT[(ws, h, n)] = M.histogram_reference(mc.meter_sums(ws, h, n), n)
    return _WANT[(ws, h, n)]


def _read(r, d, shape, dtype=np.float64):
    a = np.empty(shape, dtype)
    r.d2h(a, d)
    return a


def _padded(planes, stride, fill=1e300):
    """(3, stride) float64: the planes' elements, then `fill`: a pad that was read would land in bin 322."""
    p = np.full((3, stride), fill)
    p[:, :planes[0].size] = np.asarray(planes[:3]).reshape(3, -1)
    return p


class _Meter:
    """A sum with stride npx + pad, and counts between two sentinel words."""

    def __init__(self, r, ws, h, pad):
        self.r, self.ws, self.h, self.npx, self.stride = r, ws, h, ws * h, ws * h + pad
        self.d_sum, self.d_words = r.malloc(24 * self.stride), r.malloc(8 * (BINS + 2))
        self.d_hist = self.d_words + 8

    def close(self):
        self.r.free(self.d_sum)
        self.r.free(self.d_words)

    def put(self, s, counts=POISON):
        self.r.h2d(self.d_sum, _padded(s, self.stride))
        self.r.h2d(self.d_words, np.concatenate([[WORD], counts, [WORD]]).astype(np.uint64))

    def counts(self):
        self.r.sync()
        words = _read(self.r, self.d_words, (BINS + 2,), np.uint64)
        assert words[0] == WORD and words[-1] == WORD, "a word beside the counts was written"
        return words[1:-1]


# ---------------------------------------------------------------------------------------------------------------------
# The histogram kernel against the restatement

@pytest.mark.parametrize("ws,h", mc.FRAMES)
def test_counts_equal_the_reference_at_odd_strides_and_over_slabs(rend, ws, h):
    for n in mc.PASSES:
        want = want_of(ws, h, n)
        s = mc.meter_sums(ws, h, n)
        for pad in (1, 0, 3):                                     # pad 1 and 3: planes 1 and 2 are misaligned for the 16-byte path
            m = _Meter(rend, ws, h, pad)
            try:
                m.put(s)                                          # reset = 1 over NaN-poisoned counts
                rend.film_meter(m.d_sum, ws, h, n, m.d_hist, sum_stride=m.stride)
                got = m.counts()
                assert np.array_equal(got, want), (ws, h, n, pad, np.flatnonzero(got != want)[:6], mc.kinds(got), mc.kinds(want))
                assert int(got.sum()) == ws * h
                if ws >= 2:                                       # reset = 0 over two slabs equals one call over the frame
                    cut = ws // 2
                    m.put(s, np.zeros(BINS, np.uint64))
                    rend.film_meter(m.d_sum, cut, h, n, m.d_hist, reset=False, sum_stride=m.stride)
                    rend.film_meter(m.d_sum + 8 * cut * h, ws - cut, h, n, m.d_hist, reset=False, sum_stride=m.stride)
                    assert np.array_equal(m.counts(), want), (ws, h, n, pad, "slabs")
                    rend.film_meter(m.d_sum, ws, h, n, m.d_hist, reset=False, sum_stride=m.stride)       # and frames add up
                    assert np.array_equal(m.counts(), 2 * want)
            finally:
                m.close()


def test_a_constant_frame_counts_every_pixel_in_one_bin(rend):
    ws, h, n = 97, 71, 7
    m = _Meter(rend, ws, h, 1)
    try:
        m.put(mc.constant_sums(ws, h, n))
        rend.film_meter(m.d_sum, ws, h, n, m.d_hist, sum_stride=m.stride)
        got = m.counts()
        b = int(M.bin_reference(np.array([(0.2126 * 100.0 + 0.7152 * 100.0) + 0.0722 * 100.0]))[0])
        assert got[b] == 6887 and int(got.sum()) == 6887 and 2 <= b <= 321
        four = np.concatenate([np.array(mc.meter_sums(ws, h, n)), np.full((1, ws, h), 1e300)])          # a four-plane buffer
        d4 = rend.malloc(32 * ws * h)
        try:
            rend.h2d(d4, np.ascontiguousarray(four))
            rend.film_meter(d4, ws, h, n, m.d_hist)
            assert np.array_equal(m.counts(), want_of(ws, h, n))
        finally:
            rend.free(d4)
    finally:
        m.close()


def test_the_histogram_loops_past_the_grid_cap(rend):
    """The smallest frame of height 523 with more groups of four pixels than film_grid's cap has threads (8 blocks of 256 per CU;
    the histogram's grid takes a share of that cap): the grid-stride loop takes a second turn, and more."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == rend.kernel_info()["cu_count"]
    h = 523
    ws = (4 * 8 * 256 * cus) // h + 1
    assert (ws * h + 3) // 4 > 8 * 256 * cus >= ((ws - 1) * h + 3) // 4
    s = mc.meter_sums(ws, h, 1)
    want = want_of(ws, h, 1)
    m = _Meter(rend, ws, h, 1)
    try:
        m.put(s)
        rend.film_meter(m.d_sum, ws, h, 1, m.d_hist, sum_stride=m.stride)
        got = m.counts()
        assert int(got.sum()) == ws * h
        assert np.array_equal(got, want), (np.flatnonzero(got != want)[:6], mc.kinds(got), mc.kinds(want))
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------
# The solve

def test_the_solve_matches_the_reference_bit_for_bit(rend):
    from test_meter import solve_cases
    d_hist, d_state = rend.malloc(8 * BINS), rend.malloc(8 * 6)
    try:
        last = None
        ran = 0
        for hist, state, cfg in solve_cases():
            if hist is not last:
                rend.h2d(d_hist, np.ascontiguousarray(hist, np.uint64))
                last = hist
            rend.h2d(d_state, np.concatenate([[-5.5], state, [-6.5]]))          # the state between two sentinels
            key, pct, lo, hi, rate = cfg
            rend.film_meter_solve(d_hist, d_state + 8, key=key, percentile=pct, min_exposure=lo, max_exposure=hi, rate=rate)
            rend.sync()
            got = _read(rend, d_state, (6,))
            want = M.solve_reference(hist, state, key, pct, lo, hi, rate)
            assert got[0] == -5.5 and got[5] == -6.5
            assert same_bits(got[1:5], want), (cfg, state.tolist(), got.tolist(), want.tolist())
            ran += 1
        assert ran == 256
        # a state carried through three solves: the adaptation along an orbit
        hist = want_of(97, 71, 1)
        rend.h2d(d_hist, hist)
        rend.h2d(d_state, np.zeros(6))
        st = np.zeros(4)
        for pct in (0.5, 0.9, 0.1):
            rend.film_meter_solve(d_hist, d_state, percentile=pct, rate=0.25)
            st = M.solve_reference(hist, st, percentile=pct, rate=0.25)
        rend.sync()
        assert same_bits(_read(rend, d_state, (4,)), st) and st[0] > 0
    finally:
        rend.free(d_hist)
        rend.free(d_state)


# ---------------------------------------------------------------------------------------------------------------------
# The metered resolve

def _resolve(rend, metered, d_sum, ws, h, n, d_state, stride, flags, **tone):
    """(uint8, float32) of one resolve from sentinel-filled outputs; the uint8 frame alone with RT_FLAG_U8_HWC."""
    npx = ws * h
    hwc = bool(flags & L.RT_FLAG_U8_HWC)
    d8, d32 = rend.malloc(3 * npx + 8), rend.malloc(12 * npx + 8)
    try:
        rend.h2d(d8, np.full(3 * npx + 8, 0xA5, np.uint8))
        rend.h2d(d32, np.full(3 * npx + 2, -777.0, np.float32))
        kw = dict(flags=flags, sum_stride=stride, **tone)
        if metered:
            rend.film_resolve_metered(d_sum, ws, h, n, d_state, d8, None if hwc else d32, **kw)
        else:
            rend.film_resolve(d_sum, ws, h, n, d8, None if hwc else d32, **kw)
        rend.sync()
        u8, f32 = _read(rend, d8, (3 * npx + 8,), np.uint8), _read(rend, d32, (3 * npx + 2,), np.float32)
        assert (u8[3 * npx:] == 0xA5).all() and (f32[3 * npx:] == -777.0).all()
        return u8[:3 * npx], f32[:3 * npx]
    finally:
        rend.free(d8)
        rend.free(d32)


@pytest.mark.parametrize("ws,h", [(1, 1), (37, 29), (97, 71)])
def test_the_metered_resolve(rend, ws, h):
    n, npx = 7, ws * h
    stride = npx + 1
    s = np.array(mc.meter_sums(ws, h, n))
    s[~np.isfinite(s)] = 0.0
    s = np.clip(s, -1e6, 1e6)
    d_sum, d_state = rend.malloc(24 * stride), rend.malloc(32)
    try:
        rend.h2d(d_sum, _padded(s, stride))
        tone = dict(exposure=1.5, white=400.0, gamma=2)
        for flags in (0, L.RT_FLAG_U8_RGB, L.RT_FLAG_U8_HWC | L.RT_FLAG_U8_RGB):
            plain = _resolve(rend, False, d_sum, ws, h, n, None, stride, flags, **tone)
            # a state of 1.0, and every state that is not (finite and > 0): rt_film_resolve's outputs bit for bit
            for x in (1.0, 0.0, -2.0, np.nan, np.inf):
                rend.h2d(d_state, np.array([x, 1e300, 1e300, 1e300]))
                got = _resolve(rend, True, d_sum, ws, h, n, d_state, stride, flags, **tone)
                assert np.array_equal(got[0], plain[0]) and same_bits(got[1], plain[1]), (flags, x)
            # a solved state: the exposure is one product, tone->exposure * state[0]
            st = M.solve_reference(M.histogram_reference(s, n), np.zeros(4), 46.0, 0.5, 2.0 ** -10, 2.0 ** 10, 1.0)
            assert st[0] != 1.0 or npx == 1
            rend.h2d(d_state, st)
            u8, f32 = _resolve(rend, True, d_sum, ws, h, n, d_state, stride, flags, **tone)
            v = F.tone_reference(s, n, exposure=np.float64(1.5) * st[0], white=400.0, gamma=2)
            if flags & L.RT_FLAG_U8_HWC:
                assert np.array_equal(u8.reshape(h, ws, 3), F.clip_reference(v).transpose(2, 1, 0))
            else:
                assert same_bits(f32.reshape(3, ws, h), v.astype(np.float32))
                order = (0, 1, 2) if flags & L.RT_FLAG_U8_RGB else (0, 2, 1)
                assert np.array_equal(u8.reshape(3, ws, h), F.clip_reference(v)[list(order)])
            if npx > 1:
                assert not np.array_equal(u8, plain[0])
    finally:
        rend.free(d_sum)
        rend.free(d_state)


# ---------------------------------------------------------------------------------------------------------------------
# Refusals

def test_refusals_carry_their_text_and_leave_the_outputs_untouched(rend):
    import python_ray_tracer_amd as pkg
    ws, h = 37, 29
    npx = ws * h
    d_sum, d_hist, d_state, d_out = rend.malloc(24 * npx), rend.malloc(8 * BINS + 8), rend.malloc(32), rend.malloc(12 * npx)
    nan, inf = float("nan"), float("inf")
    counts = np.arange(BINS + 1, dtype=np.uint64) + 5
    state = np.array([3.0, -1.0, -2.0, -3.0])
    try:
        rend.h2d(d_sum, np.ascontiguousarray(np.nan_to_num(mc.meter_sums(ws, h, 1), posinf=0.0)))
        rend.h2d(d_hist, counts)
        rend.h2d(d_state, state)
        rend.h2d(d_out, np.full(3 * npx, -777.0, np.float32))
        area = "ws*h outside 1..RT_FILM_MAX_PIXELS"
        meter = lambda *a, **kw: rend.film_meter(*a, **kw)
        bad = [("d_sum is NULL", lambda: meter(None, ws, h, 1, d_hist)),
               ("d_hist is NULL", lambda: meter(d_sum, ws, h, 1, None)),
               (area, lambda: meter(d_sum, 0, h, 1, d_hist)),
               (area, lambda: meter(d_sum, ws, -1, 1, d_hist)),
               (area, lambda: meter(d_sum, 1 << 14, (1 << 13) + 1, 1, d_hist)),
               ("n < 1", lambda: meter(d_sum, ws, h, 0, d_hist)),
               ("sum_stride smaller than the frame", lambda: meter(d_sum, ws, h, 1, d_hist, sum_stride=npx - 1)),
               ("d_hist is not 8-byte aligned", lambda: meter(d_sum, ws, h, 1, d_hist + 4)),
               ("d_hist and d_sum must be buffers of their own", lambda: meter(d_sum, ws, h, 1, d_sum)),
               # the order: the first broken rule speaks
               ("d_sum is NULL", lambda: meter(None, 0, h, 0, None)),
               ("d_hist is NULL", lambda: meter(d_sum, 0, h, 0, None)),
               (area, lambda: meter(d_sum, 0, h, 0, d_hist + 4, sum_stride=1)),
               ("n < 1", lambda: meter(d_sum, ws, h, 0, d_hist + 4, sum_stride=1)),
               ("sum_stride smaller than the frame", lambda: meter(d_sum, ws, h, 1, d_hist + 4, sum_stride=1))]
        for text, fn in bad:
            with pytest.raises(pkg.RenderError) as e:
                fn()
            assert e.value.status == L.RT_ERR_BAD_ARG and str(e.value).endswith("rt_film_meter: " + text), (text, str(e.value))
        ok = dict(key=46.0, percentile=0.5, min_exposure=0.5, max_exposure=2.0, rate=1.0)
        solve = lambda hist=d_hist, st=d_state, **kw: rend.film_meter_solve(hist, st, **{**ok, **kw})
        bad = [("d_hist is NULL", lambda: solve(hist=None)),
               ("d_state is NULL", lambda: solve(st=None)),
               ("key must be finite and > 0", lambda: solve(key=0.0)),
               ("key must be finite and > 0", lambda: solve(key=nan)),
               ("key must be finite and > 0", lambda: solve(key=inf)),
               ("percentile outside 0..1", lambda: solve(percentile=-0.01)),
               ("percentile outside 0..1", lambda: solve(percentile=1.01)),
               ("percentile outside 0..1", lambda: solve(percentile=nan)),
               ("min_exposure must be finite and > 0", lambda: solve(min_exposure=0.0)),
               ("min_exposure must be finite and > 0", lambda: solve(min_exposure=nan)),
               ("max_exposure must be finite and > 0", lambda: solve(max_exposure=inf)),
               ("max_exposure must be finite and > 0", lambda: solve(max_exposure=-1.0)),
               ("min_exposure above max_exposure", lambda: solve(min_exposure=4.0)),
               ("rate outside (0, 1]", lambda: solve(rate=0.0)),
               ("rate outside (0, 1]", lambda: solve(rate=1.5)),
               ("rate outside (0, 1]", lambda: solve(rate=nan)),
               ("flags must be 0", lambda: solve(flags=1)),
               ("reserved must be 0", lambda: solve(reserved=-1)),
               ("d_state and d_hist must be buffers of their own", lambda: solve(st=d_hist)),
               ("d_hist is NULL", lambda: solve(hist=None, st=None, key=nan)),
               ("d_state is NULL", lambda: solve(st=None, key=nan)),
               ("key must be finite and > 0", lambda: solve(key=nan, percentile=2.0)),
               ("percentile outside 0..1", lambda: solve(percentile=2.0, min_exposure=0.0)),
               ("min_exposure must be finite and > 0", lambda: solve(min_exposure=0.0, max_exposure=0.0)),
               ("max_exposure must be finite and > 0", lambda: solve(max_exposure=nan, rate=0.0)),
               ("min_exposure above max_exposure", lambda: solve(min_exposure=4.0, rate=0.0)),
               ("rate outside (0, 1]", lambda: solve(rate=0.0, flags=1)),
               ("flags must be 0", lambda: solve(flags=1, reserved=1)),
               ("reserved must be 0", lambda: solve(reserved=1, st=d_hist))]
        for text, fn in bad:
            with pytest.raises(pkg.RenderError) as e:
                fn()
            assert e.value.status == L.RT_ERR_BAD_ARG and str(e.value).endswith("rt_film_meter_solve: " + text), (text, str(e.value))
        lib = L.load()                                            # mt == NULL: below the wrapper, which always passes one
        assert lib.rt_film_meter_solve(rend._ctx, d_hist, None, d_state, None) == L.RT_ERR_BAD_ARG
        assert lib.rt_last_error(rend._ctx).decode() == "rt_film_meter_solve: mt is NULL"
        tone = dict(exposure=1.0, white=400.0, gamma=2)
        res = lambda *a, **kw: rend.film_resolve_metered(*a, **{**tone, **kw})
        named = "rt_film_resolve_metered: "
        bad = [(named + "d_sum is NULL", lambda: res(None, ws, h, 1, d_state, None, d_out)),
               (named + "d_state is NULL", lambda: res(d_sum, ws, h, 1, None, None, d_out)),
               (named + area, lambda: res(d_sum, 0, h, 1, d_state, None, d_out)),
               (named + "n < 1", lambda: res(d_sum, ws, h, 0, d_state, None, d_out)),
               (named + "exposure must be finite and > 0", lambda: res(d_sum, ws, h, 1, d_state, None, d_out, exposure=0.0)),
               (named + "white must be 0, or finite and > 0", lambda: res(d_sum, ws, h, 1, d_state, None, d_out, white=-1.0)),
               (named + "gamma must be 1 or 2", lambda: res(d_sum, ws, h, 1, d_state, None, d_out, gamma=3)),
               (named + "unknown flag bit", lambda: res(d_sum, ws, h, 1, d_state, None, d_out, flags=1 << 20)),
               ("both output pointers are NULL", lambda: res(d_sum, ws, h, 1, d_state, None, None)),
               (named + "sum_stride smaller than the frame", lambda: res(d_sum, ws, h, 1, d_state, None, d_out, sum_stride=npx - 1)),
               ("out_stride smaller than the frame", lambda: res(d_sum, ws, h, 1, d_state, None, d_out, out_stride=npx - 1)),
               ("row pitch smaller than the frame width", lambda: res(d_sum, ws, h, 1, d_state, d_out, None, flags=L.RT_FLAG_U8_HWC, out_stride=ws - 1)),
               (named + "d_state is NULL", lambda: res(d_sum, 0, h, 0, None, None, None))]
        for text, fn in bad:
            with pytest.raises(pkg.RenderError) as e:
                fn()
            assert e.value.status == L.RT_ERR_BAD_ARG and str(e.value).endswith(text), (text, str(e.value))
        rc = lib.rt_film_resolve_metered(rend._ctx, d_sum, npx, ws, h, 1, None, d_state, None, d_out, npx, None)
        assert rc == L.RT_ERR_BAD_ARG and lib.rt_last_error(rend._ctx).decode() == named + "tone is NULL"
        rend.sync()
        assert np.array_equal(_read(rend, d_hist, (BINS + 1,), np.uint64), counts), "a refused call touched the counts"
        assert same_bits(_read(rend, d_state, (4,)), state), "a refused call touched the state"
        assert (_read(rend, d_out, (3 * npx,), np.float32) == -777.0).all(), "a refused call touched the output"
        solve(percentile=0.0, min_exposure=2.0, rate=5e-324)                                  # the edges are accepted
        solve(percentile=1.0)
        rend.sync()
    finally:
        for d in (d_sum, d_hist, d_state, d_out):
            rend.free(d)


# ---------------------------------------------------------------------------------------------------------------------
# Through Film on a rendered scene with a sun

class _Counting:
    """The renderer with its meter calls and allocations counted."""

    def __init__(self, r):
        self._r, self.meters, self.mallocs = r, 0, 0

    def __getattr__(self, name):
        return getattr(self._r, name)

    def malloc(self, n):
        self.mallocs += 1
        return self._r.malloc(n)

    def film_meter(self, *a, **kw):
        self.meters += 1
        return self._r.film_meter(*a, **kw)


def test_film_meter_on_a_scene_with_a_sun(rend):
    g = np.load(os.path.join(GOLDEN, "sky_default_64_d4.npz"))
    w, h = int(g["w"]), int(g["h"])
    rend.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]),
                   light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]), light_rgb=g["light_rgb"], sky=g["sky"])
    rend.set_camera(g["cam_origin"], g["cam_rot"])
    rend.set_lens(0.0, 1.0)
    rend.set_raygen(w, h, *raygen_closed_form(w, h, float(g["fov"])))
    params = rend.params(7.0, -3.0, 2.0, depth=int(g["depth"]), aa=2, spp=1, seed=int(g["seed"]))
    tone = dict(white=400.0, gamma=2)
    r = _Counting(rend)
    with Film(r) as film:
        film.accumulate(params, 2)
        before = r.mallocs
        plain = film.resolve(u8=False, f32=True, **tone)[1]
        assert r.meters == 0 and film.d_meter_hist is None and film.d_meter_state is None and r.mallocs == before + 1     # a film that never meters
        with pytest.raises(ValueError, match="meter\\(\\)"):
            film.resolve(auto_exposure=True, **tone)
        rend.sync()
        s = _read(rend, film.d_sum, (3, w, h))
        # meter, solve, resolve: a host-side restatement of the same three steps
        film.meter()
        got = film.resolve(u8=False, f32=True, auto_exposure=True, exposure=1.25, **tone)[1]
        hist = M.histogram_reference(s, 2)
        st = M.solve_reference(hist, np.zeros(4))
        assert np.array_equal(film.histogram(), hist) and same_bits(film.exposure(), st) and int(hist.sum()) == w * h
        print(f"sky_default_64_d4, 2 passes: exposure {st[0]:.4f} for a median luminance of {st[1]:.2f} over {int(st[2])} pixels")
        assert same_bits(got, F.tone_reference(s, 2, exposure=np.float64(1.25) * st[0], **tone).astype(np.float32))
        assert not same_bits(got, plain) and st[0] != 1.0
        # the exposure survives clear() and adapts: a quarter of the way from the first frame's to the second's
        film.clear()
        params.seed += 2
        film.accumulate(params, 3)
        with pytest.raises(ValueError, match="meter\\(\\)"):
            film.resolve(auto_exposure=True, **tone)
        film.meter(key=100.0, percentile=0.9, rate=0.25)
        rend.sync()
        s3 = _read(rend, film.d_sum, (3, w, h))
        st2 = M.solve_reference(M.histogram_reference(s3, 3), st, key=100.0, percentile=0.9, rate=0.25)
        assert same_bits(film.exposure(), st2) and st2[0] != st[0]
        got = film.resolve(u8=False, f32=True, auto_exposure=True, **tone)[1]
        assert same_bits(got, F.tone_reference(s3, 3, exposure=st2[0], **tone).astype(np.float32))
        # the bloomed source: what resolve(bloom=True) shows is what is metered
        film.bloom(threshold=255.0, strength=0.5, levels=3)
        with pytest.raises(ValueError, match="meter\\(\\)"):
            film.resolve(auto_exposure=True, bloom=True, **tone)
        film.reset_meter()
        assert film.exposure().tolist() == [0.0] * 4
        film.meter(bloom=True, rate=0.25)                         # no history: it jumps
        bl = B.bloom_reference(s3, 3, 255.0, 0.5, 3)
        st3 = M.solve_reference(M.histogram_reference(bl, 1), np.zeros(4), rate=0.25)
        assert same_bits(film.exposure(), st3)
        got = film.resolve(u8=False, f32=True, auto_exposure=True, bloom=True, **tone)[1]
        assert same_bits(got, F.tone_reference(bl, 1, exposure=st3[0], **tone).astype(np.float32))
        assert r.meters == 3 and film.d_meter_hist and film.d_meter_state
