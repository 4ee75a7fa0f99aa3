"""The second moment under a history on the CPU (rt_film_temporal_moments, rt_film_denoise_variance_temporal): the header, the binding
and the exported symbols; the arithmetic of python-ray-tracer_amd/csrc/rt_temporal.h (temporal_moments_pixel) and rt_denoise_var.h
(denoise_var_prepare_len_pixel and the levels), the text the kernels compile, run by tests/algo/temporal_moments_check.cpp under
AddressSanitizer and UBSan and compared bit for bit with the numpy restatements temporal_moments_reference and
denoise_variance_temporal_reference; properties of those restatements on constructed inputs; Film's call sequences and ValueErrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from film_stub import NoDevice
from test_denoise import _flat_guides
from test_film import same_bits
from test_temporal import CONTRACT as TEMPORAL_CONTRACT
from test_variance import frame_guides, noisy_passes
import temporal_cases as tc

from python_ray_tracer_amd import Film, denoise as D, temporal as T, variance as V
from python_ray_tracer_amd import _lib as L

ALGO = os.path.join(REPO, "tests", "algo")

MOMENTS_CONTRACT = ("fresh:                         out_sq[k][e] = sq[k][e] / (double)n",
                    "in the tap loop, after H_k:    Q_k = Q_k + bw * hist_sq[k][q]",
                    "after hm_k:                    hq_k = Q_k / W",
                    "out_sq[k][e] = (L * hq_k + sq[k][e]) / (L + (double)n)")

FILTER_CONTRACT = ("Lp = (double)len[p];   m_c = mean[c][p]",
                   "Lp >= spatial_below  (own):",
                   "r_c = msq[c][p] - m_c*m_c;  r_c > 0 ? r_c : 0 (NaN: 0)",
                   "Lp > 1:  var_c = r_c / (Lp - 1.0)        else:  var_c = 0",
                   "else  (pooled; a NaN length lands here):",
                   "SL = M_c = Q_c = +0.0",
                   "for dx = -2..2 (outer), dy = -2..2 (inner), step 1:   q = (p.x+dx, p.y+dy)",
                   "q outside the frame, or id[q] != id[p]:  skip",
                   "lq = (double)len[q];   !(lq > 0):  skip",
                   "SL = SL + lq;   M_c = M_c + lq * mean[c][q];   Q_c = Q_c + lq * msq[c][q]",
                   "!(SL > 1) or !(Lp > 0):  var_c = 0",
                   "else:  pm = M_c / SL;   r_c = Q_c / SL - pm*pm  (clamped as above);   var_c = (r_c / (SL - 1.0)) * (SL / Lp)",
                   "demodulate, v_0, levels == 0 (out = mean, out[3] = v_0 without demodulation), the levels and the output:",
                   "exactly rt_film_denoise_variance's lines")


# ---------------------------------------------------------------------------------------------------------------------
# Header, binding, exported symbols, contract lines

def test_header_binding_exported_symbols_and_contract():
    hdr = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    assert "int rt_film_temporal_moments(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, const void *d_sq, int64_t sq_stride, int64_t n," in hdr
    assert "int rt_film_denoise_variance_temporal(rt_ctx *ctx, const void *d_mean, int64_t mean_stride, const void *d_msq, int64_t msq_stride," in hdr
    assert "const rt_denoise_variance *dv, double spatial_below," in hdr
    assert "#define RT_ABI_VERSION 7" in hdr and L.RT_ABI_VERSION == 7
    tm, dv = L.PROTOTYPES["rt_film_temporal_moments"], L.PROTOTYPES["rt_film_denoise_variance_temporal"]
    assert tm[0] is C.c_int and len(tm[1]) == 22 and all(tm[1][i] is C.c_int64 for i in (2, 4, 5, 7, 9, 11, 14, 17, 19))
    assert sum(t is C.c_int64 for t in tm[1]) == 9 and tm[1][15] == C.POINTER(L.rt_temporal)
    assert dv[0] is C.c_int and len(dv[1]) == 17 and all(dv[1][i] is C.c_int64 for i in (2, 4, 9, 13, 15))
    assert dv[1][6] is C.c_int and dv[1][7] is C.c_int and dv[1][11] is C.c_double and dv[1][10] == C.POINTER(L.rt_denoise_variance)
    assert "rt_film_temporal_moments" in L.LATER_ENTRIES and "rt_film_denoise_variance_temporal" in L.LATER_ENTRIES
    lib = L.load()                                               # the cross-compiled library
    assert lib.rt_abi_version() == 7 and hasattr(lib, "rt_film_temporal_moments") and hasattr(lib, "rt_film_denoise_variance_temporal")
    # header and numpy restatements state the same arithmetic, line for line
    tdoc, fdoc = T.temporal_moments_reference.__doc__, V.denoise_variance_temporal_reference.__doc__
    at = hdr.index("rt_film_temporal_moments: rt_film_temporal with three more buffers")
    for line in MOMENTS_CONTRACT:
        assert line in hdr[at:], line
        assert line in tdoc, line
    for line in FILTER_CONTRACT:
        assert line in hdr[at:], line
        assert line in fdoc, line
    for line in TEMPORAL_CONTRACT:                                # rt_film_temporal's lines still stand, for both calls
        assert line in hdr[:at], line
    assert V.SPATIAL_BELOW >= 0.0 and V.KAPPA == 1.5
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(REPO, name)).read()
        assert "rt_film_temporal_moments" in text and "rt_film_denoise_variance_temporal" in text, name
    assert "out of scope" not in hdr[hdr.index("rt_film_denoise_variance: rt_film_denoise's"):at]


# ---------------------------------------------------------------------------------------------------------------------
# The kernels' text under the sanitizers against the numpy restatements

FRAMES = ((1, 1), (1, 7), (5, 1), (37, 29), (64, 64))
_FRAME_CACHE = {}


def moments_frame(ws, h, prev="moved"):
    """A temporal_cases-style frame dict of ws x h pixels with real guides of both cameras: odd_37x29 (or a window of it, with the
    grid's origin moved to the window's corner) and, at 64 x 64, the first two cameras of the orbit."""
    key = (ws, h, prev)
    if key in _FRAME_CACHE:
        return _FRAME_CACHE[key]
    if (ws, h) == (64, 64):
        sc = tc.orbit_scene()
        cam, pc = sc["cameras"][1], sc["cameras"][0 if prev == "moved" else 1]
        gd = D.guides_reference(sc["spheres"], sc["planes"], cam[0], cam[1], 64, 64, raygen=sc["raygen"])
        hg = gd if prev == "still" else D.guides_reference(sc["spheres"], sc["planes"], pc[0], pc[1], 64, 64, raygen=sc["raygen"])
        f = dict(w=64, h=64, raygen=sc["raygen"], cam=cam, prev_cam=pc, guides=gd, hist_guides=hg)
    else:
        full = tc.frame("odd_37x29", prev)
        if (ws, h) == (37, 29):
            f = {k: full[k] for k in ("w", "h", "raygen", "cam", "prev_cam", "guides", "hist_guides")}
        else:
            x0, y0 = 10, 12
            px, gy0, dy, gz0, dz = full["raygen"]
            f = dict(w=ws, h=h, raygen=(px, gy0 + x0 * dy, dy, gz0 + y0 * dz, dz), cam=full["cam"], prev_cam=full["prev_cam"],
                     guides=np.ascontiguousarray(full["guides"][:, x0:x0 + ws, y0:y0 + h]),
                     hist_guides=np.ascontiguousarray(full["hist_guides"][:, x0:x0 + ws, y0:y0 + h]))
    _FRAME_CACHE[key] = f
    return f


def moments_inputs(ws, h, n, seed, fractions=False):
    """(sum, sum of squares, history mean, history mean of squares, history lengths): finite, sq >= sum^2 / n and hist_sq >= hist^2 in
    most pixels and below in a few; the lengths whole numbers 0..40 with zeros, or with fractions."""
    rng = np.random.default_rng(seed)
    s, hist, hl = tc.random_inputs(ws, h, n, seed)
    sq = s * s / n * rng.uniform(0.95, 1.6, s.shape)
    hsq = hist * hist * rng.uniform(0.95, 1.6, hist.shape)
    if fractions:
        hl = (hl * rng.choice([1.0, 0.5, 0.37, 1.25], hl.shape)).astype(np.float32)
    return s, sq, hist, hsq, hl


def moments_reference(f, s, sq, n, hist, hsq, hl, settings):
    return T.temporal_moments_reference(s, sq, n, f["guides"], hist, hsq, hl, f["hist_guides"], f["cam"], f["prev_cam"], f["raygen"], f["w"], f["h"],
                                        *settings)


def _sprinkle(rng, arrays, share=12):
    for a in arrays:
        flat = a.reshape(-1)
        at = rng.choice(flat.size, max(1, flat.size // share), replace=False)
        flat[at] = rng.choice([np.nan, np.inf, -np.inf, 1e300 if a.dtype == np.float64 else 3e38, -1.0], at.size)


def temporal_moments_cases():
    """[dict(f, s, sq, n, hist, hsq, hl, settings, pad, sprinkled)]: the five frames under a moved and a still previous camera, the cap
    binding and not, max_history 0, fractional lengths; then NaN and Inf in every input."""
    cases = []
    k = 0
    for ws, h in FRAMES:
        for prev, settings, n, pad, frac in (("moved", tc.SETTINGS, 4, 3, False), ("still", (1e-9, 0.999, 1000.0), 1, 0, True),
                                              ("moved", (0.25, 0.5, 3.5), 2, 1, True), ("moved", (0.25, 0.5, 0.0), 7, 2, False)):
            f = moments_frame(ws, h, prev)
            s, sq, hist, hsq, hl = moments_inputs(ws, h, n, 400 + k, frac)
            cases.append(dict(f=f, s=s, sq=sq, n=n, hist=hist, hsq=hsq, hl=hl, settings=settings, pad=pad, sprinkled=False))
            k += 1
    rng = np.random.default_rng(78)
    for ws, h, prev in ((37, 29, "moved"), (64, 64, "moved"), (37, 29, "still"), (5, 1, "still")):
        f = dict(moments_frame(ws, h, prev))
        s, sq, hist, hsq, hl = moments_inputs(ws, h, 4, 500 + k, True)
        gd, hg = np.array(f["guides"]), np.array(f["hist_guides"])
        _sprinkle(rng, (s, sq, hist, hsq, hl, gd, hg))
        f["guides"], f["hist_guides"] = gd, hg
        cases.append(dict(f=f, s=s, sq=sq, n=4, hist=hist, hsq=hsq, hl=hl, settings=tc.SETTINGS, pad=2, sprinkled=True))
        k += 1
    return cases


def filter_inputs(ws, h, seed, n=4, zeros=True):
    """(mean, msq, length) as a temporal call would leave them: a noisy image's moments, lengths 0..12 with zeros and fractions."""
    rng = np.random.default_rng(seed)
    frames = noisy_passes(rng, ws, h, n)
    s, q = V.accumulate_moments_reference(None, None, frames)
    ln = rng.choice([0.0, 1.0, 1.0, 2.0, 2.5, 3.0, 4.0, 4.0, 6.75, 8.0, 12.0] if zeros else [1.0, 2.0, 3.0, 4.0, 8.0, 12.0], (ws, h)).astype(np.float32)
    return s / n, q / n, ln


def filter_cases():
    """[dict(mean, msq, ln, guides, levels, shin, kappa, floor, dem, pre, sb, pad, compare)]: the five frames at levels 0, 1 and 4 and
    spatial_below 0, 4 and above every length; both demodulate and prefilter values; NaN and Inf in every input."""
    cases = []
    k = 0
    for ws, h in FRAMES:
        gd = frame_guides(ws, h)
        for levels, shin, kappa, floor, dem, pre, sb, pad in ((0, 1, 1.0, 0.0, 1, 1, 4.0, 2), (1, 32, 1.5, 0.0, 1, 1, 4.0, 1), (4, 32, 1.5, 0.0, 1, 1, 100.0, 0),
                                                              (1, 4, 1.0, 0.5, 0, 0, 0.0, 3), (2, 32, 0.75, 0.0, 0, 1, 2.5, 0), (0, 1, 0.0, 0.0, 0, 0, 100.0, 0)):
            mean, msq, ln = filter_inputs(ws, h, 600 + k)
            cases.append(dict(mean=mean, msq=msq, ln=ln, guides=gd, levels=levels, shin=shin, kappa=kappa, floor=floor, dem=dem, pre=pre, sb=sb, pad=pad,
                              compare=True))
            k += 1
    rng = np.random.default_rng(79)
    for levels, dem, pre, sb in ((3, 1, 1, 4.0), (0, 0, 0, 100.0), (2, 0, 1, 0.0)):
        ws, h = 13, 9
        mean, msq, ln = filter_inputs(ws, h, 700 + k)
        gd = np.array(frame_guides(37, 29)[:, 5:5 + ws, 8:8 + h])
        _sprinkle(rng, (mean, msq, ln, gd), share=10)
        cases.append(dict(mean=mean, msq=msq, ln=ln, guides=gd, levels=levels, shin=32, kappa=1.5, floor=0.0, dem=dem, pre=pre, sb=sb, pad=1, compare=False))
        k += 1
    return cases


def _padded(a, planes, pad, dtype, fill):
    p = np.full((planes, a.size // planes + pad), fill, dtype)
    p[:, :a.size // planes] = np.asarray(a).reshape(planes, -1)
    return p.astype("<f8" if dtype == np.float64 else "<f4").tobytes()


def test_arithmetic_under_sanitizers_matches_numpy(tmp_path):
    exe, table, got = str(tmp_path / "temporal_moments_check"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ALGO, "temporal_moments_check.cpp")])
    tcases, fcases = temporal_moments_cases(), filter_cases()
    with open(table, "wb") as fh:
        fh.write(np.array([len(tcases) + len(fcases)], "<i8").tobytes())
        for c in tcases:
            f, pad = c["f"], c["pad"]
            fh.write(np.array([0, f["w"], f["h"], c["n"], pad], "<i8").tobytes())
            fh.write(np.concatenate([c["settings"], f["raygen"], np.reshape(f["cam"][0], 3), np.reshape(f["cam"][1], 9),
                                     np.reshape(f["prev_cam"][0], 3), np.reshape(f["prev_cam"][1], 9)]).astype("<f8").tobytes())
            fh.write(_padded(c["s"], 3, pad, np.float64, 1e300) + _padded(c["sq"], 3, pad, np.float64, 1e300) +
                     _padded(f["guides"], 8, pad, np.float32, np.nan) + _padded(c["hist"], 3, pad, np.float64, 1e300) +
                     _padded(c["hsq"], 3, pad, np.float64, 1e300) + _padded(c["hl"], 1, pad, np.float32, np.nan) +
                     _padded(f["hist_guides"], 8, pad, np.float32, np.nan))
        for c in fcases:
            ws, h = c["guides"].shape[1:]
            pad = c["pad"]
            fh.write(np.array([1, ws, h, c["levels"], c["shin"], c["dem"], c["pre"], pad], "<i8").tobytes() +
                     np.array([c["kappa"], c["floor"], c["sb"]], "<f8").tobytes())
            fh.write(_padded(c["mean"], 3, pad, np.float64, 1e300) + _padded(c["msq"], 3, pad, np.float64, 1e300) +
                     _padded(c["ln"], 1, pad, np.float32, np.nan) + _padded(c["guides"], 8, pad, np.float32, np.nan))
    res = subprocess.run([exe, table, got], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stdout + res.stderr
    assert res.stdout.strip() == f"cases={len(tcases) + len(fcases)} ok", res.stdout
    raw = open(got, "rb").read()
    at = 0
    blended = 0
    for i, c in enumerate(tcases):
        f = c["f"]
        want, want_sq, want_len = moments_reference(f, c["s"], c["sq"], c["n"], c["hist"], c["hsq"], c["hl"], c["settings"])
        plain, plain_len = T.temporal_reference(c["s"], c["n"], f["guides"], c["hist"], c["hl"], f["hist_guides"], f["cam"], f["prev_cam"], f["raygen"],
                                                f["w"], f["h"], *c["settings"])
        assert same_bits(want, plain) and same_bits(want_len, plain_len), i
        npx = f["w"] * f["h"]
        out = np.frombuffer(raw, "<f8", 3 * npx, at).reshape(want.shape)
        out_sq = np.frombuffer(raw, "<f8", 3 * npx, at + 24 * npx).reshape(want.shape)
        out_len = np.frombuffer(raw, "<f4", npx, at + 48 * npx).reshape(want_len.shape)
        at += 52 * npx
        if c["sprinkled"]:                                        # no fault; every finite pixel still equal
            fin = np.isfinite(want).all(axis=0) & np.isfinite(want_sq).all(axis=0)
            assert fin.sum() > npx // 3, (i, int(fin.sum()))
            assert same_bits(out[:, fin], want[:, fin]) and same_bits(out_sq[:, fin], want_sq[:, fin]) and same_bits(out_len[fin], want_len[fin]), i
            continue
        for name, o, w_ in (("out", out, want), ("out_sq", out_sq, want_sq)):
            bad = np.argwhere(o.view(np.uint64) != w_.view(np.uint64))
            assert bad.size == 0, (i, name, c["settings"], len(bad), bad[:4], o[tuple(bad[0])], w_[tuple(bad[0])])
        assert same_bits(out_len, want_len), i
        assert np.isfinite(want_sq).all()
        fresh = want_len == np.float32(c["n"])
        assert same_bits(want_sq[:, fresh], (c["sq"] / np.float64(c["n"]))[:, fresh])
        if c["settings"][2] == 0.0:
            assert fresh.all(), i
        blended += int((~fresh).sum())
    assert blended > 3000 and len(tcases) >= 24
    pooled_seen = own_seen = 0
    for i, c in enumerate(fcases):
        want, pooled = V.denoise_variance_temporal_reference(c["mean"], c["msq"], c["ln"], c["guides"], c["levels"], c["shin"], c["kappa"], c["floor"],
                                                             c["dem"], c["pre"], c["sb"], pooled=True)
        out = np.frombuffer(raw, "<f8", want.size, at).reshape(want.shape)
        at += 8 * want.size
        what = (i, want.shape, c["levels"], c["shin"], c["kappa"], c["floor"], c["dem"], c["pre"], c["sb"])
        if not c["compare"]:
            assert not np.isfinite(want).all(), what
            continue
        bad = np.argwhere(out.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, (what, len(bad), bad[:4], out[tuple(bad[0])], want[tuple(bad[0])])
        assert np.isfinite(want).all(), what
        if c["sb"] == 0.0:
            assert not pooled.any(), what
        elif c["sb"] == 100.0:
            assert pooled.all(), what
        pooled_seen += int(pooled.sum())
        own_seen += int((~pooled).sum())
    assert at == len(raw) and pooled_seen > 3000 and own_seen > 3000 and len(fcases) >= 33


# ---------------------------------------------------------------------------------------------------------------------
# Properties of the restatements

@pytest.mark.parametrize("name", ["odd_37x29", "planes_only_32"])
def test_still_camera_out_sq_is_the_running_mean_of_squares(name):
    """A still camera reads one history pixel with weight 1: with whole-number lengths out_sq is (L * hist_sq + sq) / (L + n), and the
    mean and the lengths are temporal_reference's bits."""
    f = tc.frame(name, "still")
    w, h, n = f["w"], f["h"], 4
    s, sq, hist, hsq, hl = moments_inputs(w, h, n, 21)
    hl = np.maximum(hl, 1.0).astype(np.float32)
    settings = (1e-9, 0.999, 1000.0)
    out, out_sq, out_len = moments_reference(f, s, sq, n, hist, hsq, hl, settings)
    plain, plain_len = tc.reference(f, s, n, hist, hl, settings)
    assert same_bits(out, plain) and same_bits(out_len, plain_len)
    surface = f["guides"][7] >= 0
    Ld = hl.astype(np.float64)
    assert same_bits(out_sq, np.where(surface, (Ld * hsq + sq) / (Ld + np.float64(n)), sq / np.float64(n)))
    # a chain of frames under a still camera: the moments of all the passes so far
    rng = np.random.default_rng(5)
    frames = [[rng.integers(0, 64, (3, w, h)).astype(np.float32) for _ in range(2)] for _ in range(3)]
    mean = msq = ln = None
    for k, fr in enumerate(frames):
        ts, tq = V.accumulate_moments_reference(None, None, fr)
        if k == 0:
            mean, msq, ln = ts / 2.0, tq / 2.0, np.full((w, h), 2, np.float32)
        else:
            mean, msq, ln = moments_reference(f, ts, tq, 2, mean, msq, ln, settings)
    allf = np.stack([x for fr in frames for x in fr]).astype(np.float64)
    assert (ln[surface] == 6.0).all() and np.allclose(msq[:, surface], (allf * allf).mean(axis=0)[:, surface], rtol=1e-13)
    assert np.allclose(mean[:, surface], allf.mean(axis=0)[:, surface], rtol=1e-13)


@pytest.mark.parametrize("dem,pre", [(0, 0), (1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("levels", [0, 1, 4])
def test_all_fresh_input_is_the_parent_filter_bit_for_bit(levels, dem, pre):
    """len == (float)n, mean == s/n and msq == sq/n with spatial_below 0: denoise_variance_reference's bits."""
    rng = np.random.default_rng(31)
    ws, h = 37, 29
    gd = frame_guides(ws, h)
    for n in (2, 5):
        s, q = V.accumulate_moments_reference(None, None, noisy_passes(rng, ws, h, n))
        want = V.denoise_variance_reference(s, q, n, gd, levels, 32, 1.5, 0.0, dem, pre)
        got = V.denoise_variance_temporal_reference(s / np.float64(n), q / np.float64(n), np.full((ws, h), n, np.float32), gd, levels, 32, 1.5, 0.0,
                                                    dem, pre, 0.0)
        assert same_bits(got, want), (levels, dem, pre, n)
        got = V.denoise_variance_temporal_reference(s / np.float64(n), q / np.float64(n), np.full((ws, h), n, np.float32), gd, levels, 32, 1.5, 0.0,
                                                    dem, pre, float(n))       # a length that reaches spatial_below is its own
        assert same_bits(got, want)


def test_a_fresh_pixel_among_long_histories_takes_the_pooled_variance():
    """A pixel of length 1 inside a flat region of identical long-history neighbours: the pooled variance by the contract's formula,
    and 0 with spatial_below 0 (one pass has no variance of its own)."""
    ws, h = 9, 9
    g = _flat_guides(ws, h)
    mean = np.full((3, ws, h), 100.0)
    msq = np.full((3, ws, h), 100.0 * 100.0 + 50.0)              # every neighbour: per-sample variance 50 (a population one)
    ln = np.full((ws, h), 8.0, np.float32)
    ln[4, 4] = 1.0
    mean[:, 4, 4], msq[:, 4, 4] = 130.0, 130.0 * 130.0
    out, pooled = V.denoise_variance_temporal_reference(mean, msq, ln, g, 0, 1, 0.0, 0.0, 0, 0, 4.0, pooled=True)
    assert pooled.sum() == 1 and pooled[4, 4]
    SL = 24 * 8.0 + 1.0
    pm = (24 * 8.0 * 100.0 + 130.0) / SL
    r = (24 * 8.0 * (100.0 * 100.0 + 50.0) + 130.0 * 130.0) / SL - pm * pm
    want = 3 * (r / (SL - 1.0)) * (SL / 1.0)
    assert np.isclose(out[3][4, 4], want, rtol=1e-12) and want > 3 * 50.0
    own = 3 * 50.0 / 7.0
    assert np.allclose(out[3][ln == 8.0], own, rtol=1e-12)
    assert same_bits(out[:3], mean)
    zero = V.denoise_variance_temporal_reference(mean, msq, ln, g, 0, 1, 0.0, 0.0, 0, 0, 0.0)
    assert zero[3][4, 4] == 0.0 and np.allclose(zero[3][ln == 8.0], own, rtol=1e-12)
    ln0 = ln.copy()
    ln0[4, 4] = 0.0                                               # a pixel that stands for no pass: no variance either way
    assert V.denoise_variance_temporal_reference(mean, msq, ln0, g, 0, 1, 0.0, 0.0, 0, 0, 4.0)[3][4, 4] == 0.0
    g2 = g.copy()
    g2[7][4, 4] = 7.0                                             # alone in its object: SL = 1, nothing to pool
    assert V.denoise_variance_temporal_reference(mean, msq, ln, g2, 0, 1, 0.0, 0.0, 0, 0, 4.0)[3][4, 4] == 0.0


def test_a_constant_history_has_variance_zero():
    ws, h = 11, 8
    g = _flat_guides(ws, h)
    rng = np.random.default_rng(3)
    mean = np.full((3, ws, h), 64.0)
    msq = mean * mean
    ln = rng.choice([1.0, 2.0, 3.0, 9.0], (ws, h)).astype(np.float32)
    for sb in (0.0, 4.0, 100.0):
        for levels in (0, 3):
            out = V.denoise_variance_temporal_reference(mean, msq, ln, g, levels, 32, 1.5, 0.0, 0, 1, sb)
            assert (out[3] == 0.0).all() and same_bits(out[:3], mean), (sb, levels)


def test_reference_value_errors():
    assert V.check_spatial_below(4) == 4.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="spatial_below"):
            V.check_spatial_below(bad)
    m, g, ln = np.zeros((3, 4, 4)), np.zeros((8, 4, 4), np.float32), np.ones((4, 4), np.float32)
    for args in ((m[:2], m[:2], ln, g), (m, m[:, :3], ln, g), (m, m, ln.astype(np.float64), g), (m, m, ln[:3], g), (m, m, ln, g[:, :3])):
        with pytest.raises(ValueError):
            V.denoise_variance_temporal_reference(*args, 1, 1, 1.0, 0.0, 0, 0, 4.0)
    with pytest.raises(ValueError, match="spatial_below"):
        V.denoise_variance_temporal_reference(m, m, ln, g, 1, 1, 1.0, 0.0, 0, 0, -1.0)
    f = tc.frame("odd_37x29", "moved")
    s, sq, hist, hsq, hl = moments_inputs(f["w"], f["h"], 2, 1)
    for change in (dict(sq=sq[:2]), dict(hsq=hsq[:, :3]), dict(hsq=None)):
        a = dict(s=s, sq=sq, hist=hist, hsq=hsq, hl=hl)
        a.update(change)
        with pytest.raises(ValueError):
            moments_reference(f, a["s"], a["sq"], 2, a["hist"], a["hsq"], a["hl"], tc.SETTINGS)


# ---------------------------------------------------------------------------------------------------------------------
# Film's call sequences, before the library sees anything

def test_film_moments_call_sequences_and_value_errors():
    r = NoDevice()
    p = L.rt_params()
    with Film(r, moments=True) as film:
        film.accumulate(p, 1)
        n = len(r.calls)
        with pytest.raises(ValueError, match="second moment"):     # no temporal mean yet
            film.denoise(variance=True, temporal=True)
        with pytest.raises(ValueError, match="second moment"):
            film.variance(temporal=True)
        with pytest.raises(ValueError, match="spatial_below"):
            film.denoise(variance=True, temporal=True, spatial_below=-1.0)
        with pytest.raises(ValueError, match="at least 2 passes"):  # the plain variance filter keeps its rule
            film.denoise(variance=True)
        assert len(r.calls) == n
        film.temporal()                                           # no history: guides, three buffers, a call whose max_history is 0
        assert [c[0] for c in r.calls[n:]] == ["malloc", "guides", "malloc", "malloc", "malloc", "temporal_moments"]
        assert r.calls[n + 2:n + 5] == [("malloc", 24 * 32), ("malloc", 4 * 32), ("malloc", 24 * 32)]
        call = r.calls[-1]
        assert call[1:5] == (film.d_sum, film.d_sq, 1, film.d_guides) and call[11:14] == (film.d_temporal, film.d_temporal_sq, film.d_temporal_len)
        assert call[-1]["max_history"] == 0.0 and len({film.d_temporal, film.d_temporal_sq, film.d_temporal_len, film.d_sum, film.d_sq}) == 5
        n = len(r.calls)
        film.denoise(variance=True, temporal=True)                # one pass is enough under temporal=True
        assert [c[0] for c in r.calls[n:]] == ["malloc", "malloc", "denoise_variance_temporal"]
        call = r.calls[-1]
        assert call[1:9] == (film.d_temporal, film.d_temporal_sq, film.d_temporal_len, 8, 4, film.d_guides, film.d_denoised_var, film.d_work_var)
        assert call[9] == dict(levels=4, normal_shin=32, kappa=V.KAPPA, var_floor=0.0, demodulate=1, prefilter=1, spatial_below=V.SPATIAL_BELOW, stream=None)
        film.resolve(denoised=True, temporal=True)
        assert [c for c in r.calls if c[0] == "resolve"][-1][1:5] == (film.d_denoised_var, 8, 4, 1)
        film.resolve(temporal=True)
        assert [c for c in r.calls if c[0] == "resolve"][-1][1:5] == (film.d_temporal, 8, 4, 1)
        v = film.variance(temporal=True, spatial_below=2.0)       # the levels = 0 call into the work buffer: the filtered mean stays
        assert v.shape == (8, 4) and v.dtype == np.float64
        call = r.calls[-2]
        assert call[0] == "denoise_variance_temporal" and call[7:9] == (film.d_work_var, None) and call[9]["levels"] == 0 and call[9]["spatial_below"] == 2.0
        film.denoise(variance=True, temporal=True, levels=0, spatial_below=0)
        assert r.calls[-1][8] is None and r.calls[-1][9]["spatial_below"] == 0.0
        # the camera moves: the temporal buffers become the history, second moment included, without a call
        first = (film.d_temporal, film.d_temporal_sq, film.d_temporal_len, film.d_guides)
        cam0 = r.camera
        r.camera = (np.array([0.1, 0.0, 0.0]), np.eye(3).reshape(9))
        n = len(r.calls)
        film.next_frame()
        assert len(r.calls) == n and (film.d_hist, film.d_hist_sq, film.d_hist_len, film.d_hist_guides) == first
        assert film.d_temporal_sq is None and film.passes == 0
        film.accumulate(p, 2)
        with pytest.raises(ValueError, match="second moment"):     # the filtered temporal mean was the last frame's
            film.denoise(variance=True, temporal=True)
        film.temporal(max_history=8, depth_tol=0.5, normal_cos=0.25)
        assert [c[0] for c in r.calls[n + 1:]] == ["malloc", "guides", "malloc", "malloc", "malloc", "temporal_moments"]
        call = r.calls[-1]
        assert call[1:9] == (film.d_sum, film.d_sq, 2, film.d_guides, first[0], first[1], first[2], first[3]) and call[9] is cam0[0] and call[10] is cam0[1]
        assert call[11:14] == (film.d_temporal, film.d_temporal_sq, film.d_temporal_len) and film.d_temporal_sq not in first
        assert call[-1] == dict(depth_tol=0.5, normal_cos=0.25, max_history=8.0, stream=None)
        film.denoise(variance=True, temporal=True, levels=1)
        assert r.calls[-1][0] == "denoise_variance_temporal" and r.calls[-1][1] == film.d_temporal
        film.denoise(variance=True)                               # two passes: the plain variance filter works beside it
        assert r.calls[-1][0] == "denoise_variance"
        with pytest.raises(ValueError, match="temporal=True"):
            film.resolve(denoised=True, temporal=True)
        # a frame that ends without temporal(): the plain moments become the history through a call that uses no history
        r.camera = (np.array([0.2, 0.0, 0.0]), np.eye(3).reshape(9))
        film.next_frame()
        film.accumulate(p, 3)
        film.guides()
        r.camera = (np.array([0.3, 0.0, 0.0]), np.eye(3).reshape(9))
        n = len(r.calls)
        film.next_frame()
        assert [c[0] for c in r.calls[n:]] == ["temporal_moments"] and r.calls[-1][-1]["max_history"] == 0.0
        assert r.calls[-1][1:4] == (film.d_sum, film.d_sq, 3) and r.calls[-1][11:14] == (film.d_hist, film.d_hist_sq, film.d_hist_len)
        film.accumulate(p, 1)
        film.temporal()
        held = {film.d_temporal, film.d_temporal_sq, film.d_temporal_len, film.d_hist, film.d_hist_sq, film.d_hist_len, film.d_hist_guides, film.d_guides,
                film.d_denoised_var, film.d_work_var, film.d_sq, film.d_sum}
        assert None not in held and len(held) == 12
    assert held <= {c[1] for c in r.calls if c[0] == "free"}


def test_a_plain_film_makes_the_calls_it_made():
    """Without moments: no second-moment buffer, the plain temporal calls, and the variance paths refuse before any call."""
    r = NoDevice()
    p = L.rt_params()
    with Film(r) as film:
        film.accumulate(p, 2)
        film.temporal()
        assert [c[0] for c in r.calls] == ["malloc", "accumulate", "malloc", "guides", "malloc", "malloc", "temporal"]
        n = len(r.calls)
        with pytest.raises(ValueError, match="moments=True"):
            film.denoise(variance=True, temporal=True)
        with pytest.raises(ValueError, match="moments=True"):
            film.variance(temporal=True)
        assert len(r.calls) == n
        r.camera = (np.array([0.1, 0.0, 0.0]), np.eye(3).reshape(9))
        film.next_frame()
        film.accumulate(p, 2)
        film.guides()
        r.camera = (np.array([0.2, 0.0, 0.0]), np.eye(3).reshape(9))
        film.next_frame()
        film.accumulate(p, 1)
        film.temporal()
        kinds = {c[0] for c in r.calls}
        assert "temporal" in kinds and "temporal_moments" not in kinds and "accumulate_moments" not in kinds
        assert film.d_temporal_sq is None and film.d_hist_sq is None
