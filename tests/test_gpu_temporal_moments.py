"""The second moment under a history on the GPU (rt_film_temporal_moments, rt_film_denoise_variance_temporal; temporal_moments_kernel of
rt_temporal.h and denoise_var_prepare_len_kernel of rt_denoise_var.h).  Truth is the numpy restatements of python-ray-tracer_amd/temporal.py
and variance.py, which tests/test_temporal_moments.py holds against the kernels' own text on the CPU; every comparison here is bit for
bit.  Four stored scenes under a moved and a still previous camera with random sums, squares, history and lengths, odd strides and NaN
between the planes; the filter on what the call wrote, at three levels and three values of spatial_below; the all-fresh identity with
rt_film_denoise_variance; a frame with more pixels than a launch has threads; through Film: the orbit against the numpy chain, two
streams, the error paths, the example; and the quality figures on the orbit of tests/temporal_cases.py."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import REPO
import closest_hit_scenes as chs
import temporal_cases as tc
from test_denoise import _flat_guides
from test_film import same_bits
from feature_gpu import rend   # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_gpu_denoise import _read
from test_gpu_temporal import _orbit_renderer, _pass_sum, _run, _same, _set_view
from test_temporal_moments import moments_inputs, moments_reference
from test_variance import noisy_passes

from python_ray_tracer_amd import Film, denoise as D, film as F, temporal as T, variance as V
from python_ray_tracer_amd import _lib as L

pytestmark = pytest.mark.gpu


def _upload(r, arrays):
    """{name: (array, planes, stride, dtype)} -> ({name: device address}, {name: the padded host copy}), NaN in every gap."""
    dev, up = {}, {}
    for k, (a, planes, stride, dt) in arrays.items():
        p = np.full((planes, stride), np.nan, dt)
        p[:, :np.asarray(a).size // planes] = np.asarray(a).reshape(planes, -1)
        dev[k] = r.malloc(p.nbytes)
        r.h2d(dev[k], p)
        up[k] = p
    return dev, up


def _run_moments(r, f, s, sq, n, hist, hsq, hl, settings, pads=(3, 1, 5, 7, 9, 11, 13, 15, 17, 19), stream=None):
    """rt_film_temporal_moments on uploaded buffers whose planes are pads[i] elements longer than the frame (odd strides), NaN in every
    gap: (out, out_sq, out_len) after checking that gaps and inputs are what they were."""
    w, h = f["w"], f["h"]
    npx = w * h
    st = [(npx + p) | 1 if p else npx for p in pads]
    host = {"sum": (s, 3, st[0], np.float64), "sq": (sq, 3, st[1], np.float64), "guides": (f["guides"], 8, st[2], np.float32),
            "hist": (hist, 3, st[3], np.float64), "hist_sq": (hsq, 3, st[4], np.float64), "hist_len": (hl, 1, st[5], np.float32),
            "hist_guides": (f["hist_guides"], 8, st[6], np.float32), "out": (np.full((3, w, h), -777.0), 3, st[7], np.float64),
            "out_sq": (np.full((3, w, h), -999.0), 3, st[8], np.float64), "out_len": (np.full((w, h), -888.0, np.float32), 1, st[9], np.float32)}
    dev = {}
    try:
        dev, up = _upload(r, host)
        depth_tol, normal_cos, max_history = settings
        r.film_temporal_moments(dev["sum"], dev["sq"], n, dev["guides"], dev["hist"], dev["hist_sq"], dev["hist_len"], dev["hist_guides"],
                                f["prev_cam"][0], f["prev_cam"][1], dev["out"], dev["out_sq"], dev["out_len"], depth_tol=depth_tol,
                                normal_cos=normal_cos, max_history=max_history, sum_stride=st[0], sq_stride=st[1], guide_stride=st[2], hist_stride=st[3],
                                hist_sq_stride=st[4], hist_guide_stride=st[6], out_stride=st[7], out_sq_stride=st[8], stream=stream)
        r.sync(stream)
        got = {k: _read(r, dev[k], up[k].shape, up[k].dtype) for k in host}
    finally:
        for d in dev.values():
            r.free(d)
    for k in ("sum", "sq", "guides", "hist", "hist_sq", "hist_len", "hist_guides"):
        assert same_bits(got[k], up[k]), f"{k} is read only"
    for k in ("out", "out_sq", "out_len"):
        assert np.isnan(got[k][:, npx:]).all(), f"a gap between the planes of {k} was written"
    return got["out"][:, :npx].reshape(3, w, h), got["out_sq"][:, :npx].reshape(3, w, h), got["out_len"][0, :npx].reshape(w, h)


def _run_filter(r, mean, msq, ln, gd, cases, pads=(3, 9, 1, 5, 7, 11), check=None):
    """rt_film_denoise_variance_temporal for every (levels, shin, kappa, var_floor, demodulate, prefilter, spatial_below) of `cases` on
    uploaded buffers with odd strides and NaN or sentinels in every gap, each against the reference; check(case, pooled) sees which
    pixels pooled."""
    ws, h = ln.shape
    npx = ws * h
    st = [(npx + p) | 1 for p in pads]
    host = {"mean": (mean, 3, st[0], np.float64), "msq": (msq, 3, st[1], np.float64), "len": (ln, 1, st[5], np.float32), "guides": (gd, 8, st[2], np.float32)}
    dev = {}
    d_out, d_work = r.malloc(32 * st[3]), r.malloc(32 * st[4])
    try:
        dev, up = _upload(r, host)
        for case in cases:
            levels, shin, kappa, floor, dem, pre, sb = case
            r.h2d(d_out, np.full(4 * st[3], -777.0))
            r.h2d(d_work, np.full(4 * st[4], -888.0))
            r.film_denoise_variance_temporal(dev["mean"], dev["msq"], dev["len"], ws, h, dev["guides"], d_out, d_work if levels >= 1 else None, levels=levels,
                                             normal_shin=shin, kappa=kappa, var_floor=floor, demodulate=dem, prefilter=pre, spatial_below=sb,
                                             mean_stride=st[0], msq_stride=st[1], guide_stride=st[2], out_stride=st[3], work_stride=st[4])
            r.sync()
            got, work = _read(r, d_out, (4, st[3])), _read(r, d_work, (4, st[4]))
            want, pooled = V.denoise_variance_temporal_reference(mean, msq, ln, gd, levels, shin, kappa, floor, dem, pre, sb, pooled=True)
            what = f"{ws}x{h} levels={levels} shin={shin} kappa={kappa} var_floor={floor} demodulate={dem} prefilter={pre} spatial_below={sb}"
            assert np.isfinite(want).all(), what
            _same(what, got[:, :npx].reshape(4, ws, h), want)
            assert (got[:, npx:] == -777.0).all() and (work[:, npx:] == -888.0).all(), what
            if levels < 1:
                assert (work == -888.0).all(), what
            if check:
                check(case, pooled)
        for k in host:
            assert same_bits(_read(r, dev[k], up[k].shape, up[k].dtype), up[k]), f"{k} is read only"
    finally:
        for d in list(dev.values()) + [d_out, d_work]:
            r.free(d)


def test_symbols_present():
    lib = L.load()
    assert hasattr(lib, "rt_film_temporal_moments") and hasattr(lib, "rt_film_denoise_variance_temporal") and lib.rt_abi_version() == 7


# ---------------------------------------------------------------------------------------------------------------------
# Uploaded frames against the references

# (levels, normal_shin, kappa, var_floor, demodulate, prefilter): levels 0, 1 and 4
FILTERS = ((0, 1, 1.0, 0.0, 1, 1), (1, 32, 1.5, 0.0, 1, 1), (4, 32, 1.5, 0.0, 0, 0))
ABOVE = 1000.0                                                    # a spatial_below above every length: every pixel pools


@pytest.mark.parametrize("prev", ["moved", "still"])
@pytest.mark.parametrize("name", ["odd_37x29", "planes_only_32", "spheres_only_32", "inside_sphere_32"])
def test_moments_and_filter_match_the_references(rend, name, prev):
    """Random finite sums, squares, history and lengths (about a sixth of the lengths 0) on the real guides of both cameras, at the three
    settings of test_gpu_temporal: out and out_len are also rt_film_temporal's device output.  Then the filter on what the n = 1 call
    wrote (lengths 1 to 4.5), at levels 0, 1 and 4 and spatial_below 0, 4 and above every length."""
    f = tc.frame(name, prev)
    _set_view(rend, f)
    w, h = f["w"], f["h"]
    kept = None
    for k, (settings, n) in enumerate(((tc.SETTINGS, 4), ((0.02, 0.95, 3.5), 1), ((0.25, 0.5, 0.0), 7))):
        s, sq, hist, hsq, hl = moments_inputs(w, h, n, 300 + k)
        want, want_sq, want_len = moments_reference(f, s, sq, n, hist, hsq, hl, settings)
        out, out_sq, out_len = _run_moments(rend, f, s, sq, n, hist, hsq, hl, settings)
        what = f"{name} {prev} {settings} n={n}"
        _same(what, out, want)
        _same(what + " squares", out_sq, want_sq)
        _same(what + " length", out_len, want_len)
        plain, plain_len = _run(rend, f, s, n, hist, hl, settings)
        _same(what + " against rt_film_temporal", out, plain)
        _same(what + " length against rt_film_temporal", out_len, plain_len)
        fresh = int((want_len == np.float32(n)).sum())
        assert (hl == 0).sum() > w * h // 10
        if settings[2] == 0.0:
            assert fresh == w * h and same_bits(out_sq, sq / np.float64(n))
        elif k == 0:
            assert 0 < fresh < 3 * w * h // 4, (what, fresh)
        if k == 1:
            kept = (out, out_sq, out_len)
    mean, msq, ln = kept
    assert (ln < 4.0).any() and (ln >= 4.0).any()

    def check(case, pooled):
        sb = case[6]
        if sb == 0.0:
            assert not pooled.any()
        elif sb == ABOVE:
            assert pooled.all()
        else:
            assert np.array_equal(pooled, ln < np.float32(sb)) and pooled.any() and not pooled.all()

    _run_filter(rend, mean, msq, ln, np.array(f["guides"]), [flt + (sb,) for flt in FILTERS for sb in (0.0, 4.0, ABOVE)], check=check)


def test_backward_facing_history_is_all_fresh(rend):
    f = tc.frame("odd_37x29", "backward")
    _set_view(rend, f)
    s, sq, hist, hsq, hl = moments_inputs(f["w"], f["h"], 2, 310)
    out, out_sq, out_len = _run_moments(rend, f, s, sq, 2, hist, hsq, hl, tc.SETTINGS, pads=(0,) * 10)
    _same("backward", out, s / np.float64(2))
    _same("backward squares", out_sq, sq / np.float64(2))
    assert (out_len == 2.0).all()


def test_both_kernels_loop_past_the_grid_cap(rend):
    """The synthetic wall of tests/temporal_cases.py with more pixels than a launch has threads (8 blocks of 256 per CU): the grid-stride
    loops of temporal_moments_kernel and of denoise_var_prepare_len_kernel take a second turn."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == rend.kernel_info()["cu_count"]
    w, h = chs.grid_cap_frame(cus)
    assert w * h > 8 * 256 * cus
    t0 = time.perf_counter()
    f, s, hist, hl = tc.synthetic_frame(w, h)
    rng = np.random.default_rng(9)
    sq = s * s / 3 * rng.uniform(0.95, 1.6, s.shape)
    hsq = hist * hist * rng.uniform(0.95, 1.6, hist.shape)
    settings = (0.05, 0.9, 6.0)
    want, want_sq, want_len = moments_reference(f, s, sq, 3, hist, hsq, hl, settings)
    _set_view(rend, f)
    out, out_sq, out_len = _run_moments(rend, f, s, sq, 3, hist, hsq, hl, settings, pads=(1, 0, 0, 3, 1, 1, 0, 5, 3, 0))
    _same("grid cap", out, want)
    _same("grid cap squares", out_sq, want_sq)
    _same("grid cap length", out_len, want_len)
    fresh = int((want_len == 3.0).sum())
    assert w * h // 20 < fresh < w * h // 2
    seen = []
    _run_filter(rend, out, out_sq, out_len, np.array(f["guides"]), [(0, 1, 1.0, 0.0, 0, 0, 4.0)], check=lambda case, pooled: seen.append(int(pooled.sum())))
    assert seen[0] == fresh                                       # the fresh pixels (length 3) pool, the others (above 4) do not
    print(f"grid cap: {w} x {h} on {cus} CUs, {fresh} fresh; references, device and read-back {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("levels", [0, 1, 4])
def test_all_fresh_is_rt_film_denoise_variance_on_the_device(rend, levels):
    """Sums of n passes through rt_film_temporal_moments with max_history 0 (mean = s/n, msq = sq/n, len = n), then the filter with
    spatial_below 0: the bits rt_film_denoise_variance gives on the sums, on the device."""
    f = tc.frame("odd_37x29", "still")
    _set_view(rend, f)
    w, h, n = f["w"], f["h"], 3
    npx = w * h
    gd = np.array(f["guides"])
    s, q = V.accumulate_moments_reference(None, None, noisy_passes(np.random.default_rng(41), w, h, n))
    mean, msq, ln = _run_moments(rend, f, s, q, n, s, q, np.ones((w, h), np.float32), (0.25, 0.5, 0.0))
    assert same_bits(mean, s / np.float64(n)) and same_bits(msq, q / np.float64(n)) and (ln == 3.0).all()
    bufs = [rend.malloc(k * npx) for k in (24, 24, 24, 24, 4, 32, 32, 32, 32, 32)]
    d_s, d_q, d_m, d_mq, d_l, d_g, d_a, d_b, d_wa, d_wb = bufs
    try:
        for d, a in ((d_s, s), (d_q, q), (d_m, mean), (d_mq, msq), (d_l, ln), (d_g, gd)):
            rend.h2d(d, np.ascontiguousarray(a))
        kw = dict(levels=levels, normal_shin=32, kappa=1.5, var_floor=0.0, demodulate=1, prefilter=1)
        rend.film_denoise_variance(d_s, d_q, w, h, n, d_g, d_a, d_wa, **kw)
        rend.film_denoise_variance_temporal(d_m, d_mq, d_l, w, h, d_g, d_b, d_wb, spatial_below=0.0, **kw)
        rend.sync()
        a, b = _read(rend, d_a, (4, w, h)), _read(rend, d_b, (4, w, h))
        _same(f"levels {levels}", b, a)
        _same(f"levels {levels} reference", b, V.denoise_variance_reference(s, q, n, gd, levels, 32, 1.5, 0.0, 1, 1))
        assert (a[3] > 0).any()
    finally:
        for d in bufs:
            rend.free(d)


def test_one_pixel_and_one_object(rend):
    """A 1 x 1 frame (nothing to pool: SL = Lp), and a frame of one object id, where every window is full."""
    rng = np.random.default_rng(43)
    for ws, h in ((1, 1), (19, 23)):
        gd = _flat_guides(ws, h)
        s, q = V.accumulate_moments_reference(None, None, noisy_passes(rng, ws, h, 4))
        ln = rng.choice([1.0, 2.0, 3.0, 5.5, 8.0], (ws, h)).astype(np.float32)
        _run_filter(rend, s / 4.0, q / 4.0, ln, gd, [(lv, 32, 1.5, 0.0, 1, 1, sb) for lv in (0, 2) for sb in (0.0, 4.0, ABOVE)])


# ---------------------------------------------------------------------------------------------------------------------
# Through Film

def _pass_moments(r, params_of, seed, n, w, h):
    """accumulate_moments_reference of n pass frames rendered one by one with the current camera."""
    d32 = r.malloc(12 * w * h)
    frames = []
    try:
        for i in range(n):
            r.render_device(params_of(seed + i), 0, w, None, d32)
            r.sync()
            frames.append(_read(r, d32, (3, w, h), np.float32))
    finally:
        r.free(d32)
    return V.accumulate_moments_reference(None, None, frames)


def test_film_orbit_against_the_numpy_chain(rend):
    """test_gpu_temporal's three-step orbit on a film with moments: the first frame ends without temporal() (its plain moments become
    the history through next_frame), the second with it (a swap).  Then the variance-guided filter on the temporal mean, its resolve, and
    variance(temporal=True)."""
    sc = tc.orbit_scene()
    w, h, rg = sc["w"], sc["h"], sc["raygen"]
    params_of = _orbit_renderer(rend, sc, 4)
    cams, n = sc["cameras"][:3], 2
    settings = (T.DEPTH_TOL, T.NORMAL_COS, 3.0)
    hist = hist_sq = hist_len = hist_guides = None
    with Film(rend, moments=True) as film:
        for k, cam in enumerate(cams):
            rend.set_camera(*cam)
            total, total_sq = _pass_moments(rend, params_of, 40 + 10 * k, n, w, h)
            gd = D.guides_reference(sc["spheres"], sc["planes"], cam[0], cam[1], w, h, raygen=rg)
            film.next_frame()
            film.accumulate(params_of(40 + 10 * k), n)
            if k == 0:
                assert same_bits(film.guides(), gd)
                want, want_sq, want_len = total / np.float64(n), total_sq / np.float64(n), np.full((w, h), n, np.float32)
            else:
                film.temporal(max_history=settings[2])
                want, want_sq, want_len = T.temporal_moments_reference(total, total_sq, n, gd, hist, hist_sq, hist_len, hist_guides, cam, cams[k - 1], rg,
                                                                       w, h, *settings)
                rend.sync()
                _same(f"frame {k}", _read(rend, film.d_temporal, (3, w, h)), want)
                _same(f"frame {k} squares", _read(rend, film.d_temporal_sq, (3, w, h)), want_sq)
                _same(f"frame {k} length", _read(rend, film.d_temporal_len, (w, h), np.float32), want_len)
                if k == 1:                                        # the history next_frame() made of the first frame's plain moments
                    _same("history squares", _read(rend, film.d_hist_sq, (3, w, h)), hist_sq)
                    _same("history", _read(rend, film.d_hist, (3, w, h)), hist)
            hist, hist_sq, hist_len, hist_guides = want, want_sq, want_len, gd
        assert hist_len.max() == 5.0 and (hist_len == 2.0).any()
        film.denoise(variance=True, temporal=True)                # SPATIAL_BELOW
        den, pooled = V.denoise_variance_temporal_reference(hist, hist_sq, hist_len, hist_guides, 4, 32, V.KAPPA, 0.0, 1, 1, V.SPATIAL_BELOW, pooled=True)
        rend.sync()
        _same("filtered temporal mean", _read(rend, film.d_denoised_var, (4, w, h)), den)
        u8, f32 = film.resolve(white=400.0, gamma=2, f32=True, denoised=True, temporal=True)
        v = F.tone_reference(den[:3], 1, 1.0, 400.0, 2)
        assert same_bits(f32, v.astype(np.float32)) and np.array_equal(u8, F.clip_reference(v)[[0, 2, 1]])
        film.denoise(variance=True, temporal=True, spatial_below=4.0, levels=2, kappa=1.0)
        den4, pooled4 = V.denoise_variance_temporal_reference(hist, hist_sq, hist_len, hist_guides, 2, 32, 1.0, 0.0, 1, 1, 4.0, pooled=True)
        rend.sync()
        _same("spatial_below 4", _read(rend, film.d_denoised_var, (4, w, h)), den4)
        assert pooled4.any() and not pooled4.all()                # the fresh pixels (length 2) pool, the history's do not
        var = film.variance(temporal=True, spatial_below=4.0)
        assert same_bits(var, V.denoise_variance_temporal_reference(hist, hist_sq, hist_len, hist_guides, 0, 1, 0.0, 0.0, 0, 0, 4.0)[3]) and (var > 0).any()
        _, f32 = film.resolve(white=400.0, u8=False, f32=True, temporal=True)
        assert same_bits(f32, F.tone_reference(hist, 1, 1.0, 400.0, 1).astype(np.float32))
        film.denoise(variance=True)                               # the plain variance filter on this frame's two passes, beside it
        rend.sync()
        _same("plain variance filter", _read(rend, film.d_denoised_var, (4, w, h)), V.denoise_variance_reference(total, total_sq, n, hist_guides, 4, 32, V.KAPPA, 0.0, 1, 1))


def test_two_films_on_two_streams(rend):
    """Two films with moments carried through a move each, every call of one film on its own stream, queued together: the serial
    results."""
    sc = tc.orbit_scene()
    w, h, rg = sc["w"], sc["h"], sc["raygen"]
    _orbit_renderer(rend, sc, 4)
    streams = [rend.stream_create(), rend.stream_create()]
    films, wants = [Film(rend, moments=True), Film(rend, moments=True)], []
    try:
        for i, (film, st) in enumerate(zip(films, streams)):
            params_of = _orbit_renderer(rend, sc, 4 if i == 0 else 2)
            cams = (sc["cameras"][i], sc["cameras"][i + 3])
            for cam in cams:
                rend.set_camera(*cam)
                film.next_frame(stream=st)
                film.accumulate(params_of(70 + i), 1, stream=st)
                film.temporal(stream=st)
            film.denoise(variance=True, temporal=True, levels=2, spatial_below=2.0, stream=st)
            wants.append((i, cams))
        for st in streams:
            rend.sync(st)
        for film, (i, cams) in zip(films, wants):
            params_of = _orbit_renderer(rend, sc, 4 if i == 0 else 2)
            for k, cam in enumerate(cams):
                rend.set_camera(*cam)
                total, total_sq = _pass_moments(rend, params_of, 70 + i, 1, w, h)
                gd = D.guides_reference(sc["spheres"], sc["planes"], cam[0], cam[1], w, h, raygen=rg)
                if k == 0:
                    outs = [total, total_sq, np.full((w, h), 1, np.float32), gd]
                else:
                    want, want_sq, want_len = T.temporal_moments_reference(total, total_sq, 1, gd, outs[0], outs[1], outs[2], outs[3], cam, cams[0], rg, w, h,
                                                                           T.DEPTH_TOL, T.NORMAL_COS, T.MAX_HISTORY)
            _same(f"film {i}", _read(rend, film.d_temporal, (3, w, h)), want)
            _same(f"film {i} squares", _read(rend, film.d_temporal_sq, (3, w, h)), want_sq)
            _same(f"film {i} length", _read(rend, film.d_temporal_len, (w, h), np.float32), want_len)
            den, pooled = V.denoise_variance_temporal_reference(want, want_sq, want_len, gd, 2, 32, V.KAPPA, 0.0, 1, 1, 2.0, pooled=True)
            _same(f"film {i} filtered", _read(rend, film.d_denoised_var, (4, w, h)), den)
            assert (want_len == 2.0).sum() > w * h // 2 and pooled.any() and not pooled.all()
    finally:
        for film in films:
            film.close()
        for st in streams:
            rend.stream_destroy(st)


# ---------------------------------------------------------------------------------------------------------------------
# Error paths

def test_errors_leave_the_outputs_untouched(rend):
    import python_ray_tracer_amd as pkg
    f = tc.frame("odd_37x29", "moved")
    _set_view(rend, f)
    w, h = f["w"], f["h"]
    npx = w * h
    names = ("sum", "sq", "guides", "hist", "hsq", "len", "hguides", "out", "osq", "olen")
    size = dict(sum=24, sq=24, guides=32, hist=24, hsq=24, len=4, hguides=32, out=24, osq=24, olen=4)
    d = {k: rend.malloc(size[k] * npx) for k in names}
    d_f, d_w = rend.malloc(32 * npx), rend.malloc(32 * npx)
    nan, inf = float("nan"), float("inf")
    try:
        rend.h2d(d["sum"], np.full(3 * npx, 100.0))
        rend.h2d(d["sq"], np.full(3 * npx, 5050.0))               # two passes of 50 +- 5
        rend.h2d(d["hist"], np.full(3 * npx, 50.0))
        rend.h2d(d["hsq"], np.full(3 * npx, 2525.0))
        rend.h2d(d["guides"], np.ascontiguousarray(f["guides"]))
        rend.h2d(d["hguides"], np.ascontiguousarray(f["hist_guides"]))
        rend.h2d(d["len"], np.full(npx, 4.0, np.float32))
        rend.h2d(d["out"], np.full(3 * npx, -777.0))
        rend.h2d(d["osq"], np.full(3 * npx, -999.0))
        rend.h2d(d["olen"], np.full(npx, -888.0, np.float32))
        ok = dict(depth_tol=0.25, normal_cos=0.5, max_history=16.0)

        def call(r=rend, n=2, prev=f["prev_cam"], **kw):
            b = {k: kw.pop(k, d[k]) for k in names}
            r.film_temporal_moments(b["sum"], b["sq"], n, b["guides"], b["hist"], b["hsq"], b["len"], b["hguides"], prev[0], prev[1], b["out"], b["osq"],
                                    b["olen"], **{**ok, **kw})

        bad = {f"NULL {k}": (lambda k=k: call(**{k: None})) for k in names}
        bad.update({"n 0": lambda: call(n=0), "n above 2^24": lambda: call(n=(1 << 24) + 1), "depth_tol < 0": lambda: call(depth_tol=-0.1),
                    "depth_tol NaN": lambda: call(depth_tol=nan), "normal_cos > 1": lambda: call(normal_cos=1.5), "normal_cos NaN": lambda: call(normal_cos=nan),
                    "max_history < 0": lambda: call(max_history=-1.0), "max_history inf": lambda: call(max_history=inf), "reserved": lambda: call(reserved=(0, 1)),
                    "prev origin NaN": lambda: call(prev=(np.array([0.0, nan, 0.0]), np.eye(3))),
                    "prev rotation inf": lambda: call(prev=(np.zeros(3), np.full((3, 3), inf)))})
        for k in ("sum", "sq", "guide", "hist", "hist_sq", "hist_guide", "out", "out_sq"):
            bad[f"short {k}_stride"] = lambda k=k: call(**{k + "_stride": npx - 1})
        for k in names:
            if k != "osq":
                bad[f"out_sq is {k}"] = lambda k=k: call(osq=d[k])
        for k in ("sum", "sq", "guides", "hist", "hsq", "len", "hguides"):
            bad[f"out is {k}"] = lambda k=k: call(out=d[k])
            bad[f"out_len is {k}"] = lambda k=k: call(olen=d[k])
        bad["out_len is out"] = lambda: call(olen=d["out"])
        for what, fn in bad.items():
            with pytest.raises(pkg.RenderError) as e:
                fn()
            assert e.value.status == L.RT_ERR_BAD_ARG, what
        lib = L.load()                                            # a NULL settings pointer
        vp = lambda k: ctypes.c_void_p(d[k])
        assert lib.rt_film_temporal_moments(rend._ctx, vp("sum"), npx, vp("sq"), npx, 2, vp("guides"), npx, vp("hist"), npx, vp("hsq"), npx, vp("len"),
                                            vp("hguides"), npx, None, vp("out"), npx, vp("osq"), npx, vp("olen"), None) == L.RT_ERR_BAD_ARG
        with pkg.Renderer(0) as fresh:                            # no camera; an explicit grid: the statuses of rt_film_temporal
            with pytest.raises(pkg.RenderError) as e:
                call(r=fresh)
            assert e.value.status == L.RT_ERR_STATE
            fresh.set_camera(*f["cam"])
            px, y0, dy, z0, dz = f["raygen"]
            xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="ij")
            fresh.set_pixel_loc(np.stack([np.full((w, h), px), xs * dy + y0, ys * dz + z0]))
            with pytest.raises(pkg.RenderError) as e:
                call(r=fresh)
            assert e.value.status == L.RT_ERR_STATE
            fresh.set_raygen(w, h, px, y0, 0.0, z0, dz)
            with pytest.raises(pkg.RenderError) as e:
                call(r=fresh)
            assert e.value.status == L.RT_ERR_STATE
        rend.sync()
        assert (_read(rend, d["out"], (3 * npx,)) == -777.0).all() and (_read(rend, d["osq"], (3 * npx,)) == -999.0).all()
        assert (_read(rend, d["olen"], (npx,), np.float32) == -888.0).all()
        call()                                                    # the context is still usable; constants stay constants
        rend.sync()
        out, osq, olen = _read(rend, d["out"], (3, npx)), _read(rend, d["osq"], (3, npx)), _read(rend, d["olen"], (npx,), np.float32)
        assert set(np.unique(olen)) <= {2.0, 6.0} and (olen == 6.0).any() and (olen == 2.0).any()
        assert np.allclose(out, 50.0, rtol=1e-14) and np.allclose(osq, 2525.0, rtol=1e-14)
        # the filter
        rend.h2d(d_f, np.full(4 * npx, -777.0))
        rend.h2d(d_w, np.full(4 * npx, -888.0))
        fok = dict(levels=2, normal_shin=32, kappa=1.0, var_floor=0.0, demodulate=1, prefilter=1, spatial_below=4.0)
        den = lambda *a, **kw: rend.film_denoise_variance_temporal(*a, **{**fok, **kw})
        good = (d["out"], d["osq"], d["olen"], w, h, d["guides"], d_f, d_w)
        swap = lambda i, v: good[:i] + (v,) + good[i + 1:]
        bad = {"NULL mean": lambda: den(*swap(0, None)), "NULL msq": lambda: den(*swap(1, None)), "NULL len": lambda: den(*swap(2, None)),
               "NULL guides": lambda: den(*swap(5, None)), "NULL out": lambda: den(*swap(6, None)), "levels -1": lambda: den(*good, levels=-1),
               "levels 7": lambda: den(*good, levels=7), "shin 3": lambda: den(*good, normal_shin=3), "kappa < 0": lambda: den(*good, kappa=-1.0),
               "kappa NaN": lambda: den(*good, kappa=nan), "var_floor inf": lambda: den(*good, var_floor=inf), "demodulate 2": lambda: den(*good, demodulate=2),
               "prefilter -1": lambda: den(*good, prefilter=-1), "spatial_below < 0": lambda: den(*good, spatial_below=-1.0),
               "spatial_below NaN": lambda: den(*good, spatial_below=nan), "spatial_below inf": lambda: den(*good, spatial_below=inf),
               "ws 0": lambda: den(*swap(3, 0)), "h 0": lambda: den(*swap(4, 0)),
               "short mean_stride": lambda: den(*good, mean_stride=npx - 1), "short msq_stride": lambda: den(*good, msq_stride=npx - 1),
               "short guide_stride": lambda: den(*good, guide_stride=npx - 1), "short out_stride": lambda: den(*good, out_stride=npx - 1),
               "short work_stride": lambda: den(*good, work_stride=npx - 1), "NULL work with one level": lambda: den(*swap(7, None), levels=1),
               "work is out": lambda: den(*swap(7, d_f))}
        for i, k in ((0, "mean"), (1, "msq"), (2, "len"), (5, "guides")):
            bad[f"out is {k}"] = lambda i=i: den(*swap(6, good[i]))
            bad[f"work is {k}"] = lambda i=i: den(*swap(7, good[i]))
        for what, fn in bad.items():
            with pytest.raises(pkg.RenderError) as e:
                fn()
            assert e.value.status == L.RT_ERR_BAD_ARG, what
        assert lib.rt_film_denoise_variance_temporal(rend._ctx, vp("out"), npx, vp("osq"), npx, vp("olen"), w, h, vp("guides"), npx, None, 4.0,
                                                     ctypes.c_void_p(d_f), npx, ctypes.c_void_p(d_w), npx, None) == L.RT_ERR_BAD_ARG
        rend.sync()
        assert (_read(rend, d_f, (4 * npx,)) == -777.0).all() and (_read(rend, d_w, (4 * npx,)) == -888.0).all()
        den(*good, demodulate=0)
        den(d["out"], d["osq"], d["olen"], w, h, d["guides"], d_w, None, levels=0)
        rend.sync()
        got, work = _read(rend, d_f, (4, npx)), _read(rend, d_w, (4, npx))
        assert np.allclose(got[:3], 50.0, rtol=1e-14) and (got[3] >= 0).all() and (work[:3] == out).all()
        assert np.allclose(work[3][olen == 6.0], 3 * 25.0 / 5.0, rtol=1e-10)       # own: (2525 - 2500) / (6 - 1) per channel
    finally:
        for p in list(d.values()) + [d_f, d_w]:
            rend.free(p)


# ---------------------------------------------------------------------------------------------------------------------
# The example

def test_example_with_temporal_and_denoise_variance_writes_a_png(tmp_path):
    """examples/render_png.py --orbit 3 --passes 2 --temporal --denoise-variance, in a fresh child process."""
    from PIL import Image
    out = str(tmp_path / "orbit_var.png")
    log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--sky", "--soft", "--shadow-samples", "1", "--passes", "2",
                                   "--white", "400", "--size", "64x64", "--orbit", "3", "--temporal", "--denoise-variance", "--spatial-below", "4",
                                   "--denoise-levels", "2", "--out", out], text=True)
    assert "wrote" in log and "temporal=True" in log and "denoise_variance=True" in log and "orbit=3" in log
    img = np.asarray(Image.open(out))
    assert img.shape == (64, 64, 3) and img.any() and len(np.unique(img)) > 32


# ---------------------------------------------------------------------------------------------------------------------
# Quality

def test_quality_the_variance_filter_helps_the_temporal_mean_on_matte_pixels(rend):
    """The orbit of tests/temporal_cases.py: 8 camera steps of 2 degrees, 4 passes per frame, ONE shadow sample, truth the mean of 1024
    passes at the last camera; RMSE in linear colour over the whole frame, matte pixels and the rest, for the raw mean, the temporal mean,
    temporal then fixed sigma, temporal then variance-guided (Film's defaults) and variance-guided alone.  Asserted: over matte pixels,
    which must be at least half the frame, the variance-guided filter of the temporal mean is closer to the truth than the unfiltered
    temporal mean.  The figures are results, printed (Variance under a history, has them with the sweep)."""
    sc = tc.orbit_scene()
    w, h = sc["w"], sc["h"]
    params_of = _orbit_renderer(rend, sc, 1)
    last = sc["cameras"][-1]
    matte = tc.matte_mask(sc, D.guides_reference(sc["spheres"], sc["planes"], last[0], last[1], w, h, raygen=sc["raygen"]))
    assert matte.sum() >= w * h // 2
    with Film(rend) as truth_film, Film(rend, moments=True) as film:
        for k, cam in enumerate(sc["cameras"]):
            rend.set_camera(*cam)
            film.next_frame()
            film.accumulate(params_of(1 + tc.ORBIT_PASSES * k), tc.ORBIT_PASSES)
            film.temporal()
        truth_film.accumulate(params_of(5000), 1024)
        film.denoise(temporal=True)
        film.denoise(variance=True, temporal=True)
        rend.sync()
        truth = _read(rend, truth_film.d_sum, (3, w, h)) / 1024.0
        res = {"raw": _read(rend, film.d_sum, (3, w, h)) / float(tc.ORBIT_PASSES), "temporal": _read(rend, film.d_temporal, (3, w, h)),
               "temporal + fixed sigma": _read(rend, film.d_denoised, (3, w, h)),
               "temporal + variance-guided": _read(rend, film.d_denoised_var, (4, w, h))[:3]}
        film.denoise(variance=True)
        rend.sync()
        res["variance-guided alone"] = _read(rend, film.d_denoised_var, (4, w, h))[:3]
        length = _read(rend, film.d_temporal_len, (w, h), np.float32)
    rmse = lambda a, m: float(np.sqrt(np.mean((a - truth)[:, m] ** 2)))
    every = np.ones((w, h), bool)
    for what, m in (("whole frame", every), ("matte", matte), ("not matte", ~matte)):
        print(f"quality, {what} ({int(m.sum())} pixels): rmse " + ", ".join(f"{k} {rmse(v, m):.4f}" for k, v in res.items()))
    print(f"quality: history length mean {float(length.mean()):.2f}, {int((length < V.SPATIAL_BELOW).sum())} pixels below spatial_below {V.SPATIAL_BELOW:g}")
    ours, yard = rmse(res["temporal + variance-guided"], matte), rmse(res["temporal"], matte)
    assert ours < yard, (ours, yard)
