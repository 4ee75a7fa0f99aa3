"""The variance-guided denoiser on the GPU (rt_film_accumulate_moments, rt_film_denoise_variance; film_add2_kernel of rt_film.h and the
kernels of rt_denoise_var.h).  Truth is the numpy restatement of python-ray-tracer_amd/variance.py, which tests/test_variance.py
holds against the kernels' own text on the CPU; every comparison here is bit for bit.  The moments on slabs of a 37 x 29 frame of the
soft_default_64_d4 scene with (x1-x0)*h mod 4 of 1, 2, 3 and 0, for 1, 3, 4, 5 and 9 passes, into NaN-filled buffers whose planes are
16-byte aligned in one buffer and not in the other, then a second call without reset, and slab by slab in place; the filter on
random passes over real guides for five frame sizes with odd strides and sentinels, at six levels on synthetic guides, on a frame with
more pixels than its grid has threads, with planes more than 2^32 bytes apart; through Film; the quality figures; the error paths;
two streams; the example."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import REPO, raygen_closed_form
import closest_hit_scenes as chs
from feature_gpu import IGNORED
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_film import same_bits
from test_variance import FRAMES, frame_guides, noisy_passes
import variance_cases as vc

from python_ray_tracer_amd import Film, denoise as D, film as F, variance as V
from python_ray_tracer_amd import _lib as L

pytestmark = pytest.mark.gpu


def _read(r, d, shape, dtype=np.float64):
    a = np.empty(shape, dtype)
    r.d2h(a, d)
    return a


def _nan_buffer(r, n_doubles):
    d = r.malloc(8 * n_doubles)
    r.h2d(d, np.full(n_doubles, np.nan))
    return d


def _soft_scene(r, w=None, h=None, shadow_samples=None):
    """soft_default_64_d4 under RT_AA_NONE (area lights: the seed drives the light hashes), on its own grid or on a w x h one."""
    g = vc.fixture()
    w, h = (int(g["w"]) if w is None else w), (int(g["h"]) if h is None else h)
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]),
                light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]) if shadow_samples is None else shadow_samples)
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(0.0, 1.0)
    r.set_raygen(w, h, *raygen_closed_form(w, h, float(g["fov"])))
    return w, h, lambda seed: r.params(**IGNORED, depth=int(g["depth"]), aa=0, seed=seed), int(g["seed"])


_PASSES = {}


def _pass_frames(r, params_of, seed, n, w, h, tag):
    """float32 (3, w, h) frames of seeds seed .. seed+n-1 through rt_render_device: each rendered once per (tag, seed), read-only."""
    d32 = r.malloc(12 * w * h)
    out = []
    try:
        for i in range(n):
            key = (tag, seed + i)
            if key not in _PASSES:
                r.render_device(params_of(seed + i), 0, w, None, d32)
                r.sync()
                a = _read(r, d32, (3, w, h), np.float32)
                a.setflags(write=False)
                _PASSES[key] = a
            out.append(_PASSES[key])
    finally:
        r.free(d32)
    return out


def test_symbols_present():
    lib = L.load()
    assert hasattr(lib, "rt_film_accumulate_moments") and hasattr(lib, "rt_film_denoise_variance") and lib.rt_abi_version() == 7


# ---------------------------------------------------------------------------------------------------------------------
# The moments

SLAB_W, SLAB_H = 37, 29


@pytest.mark.parametrize("passes", [1, 3, 4, 5, 9])
def test_moments_on_slabs_of_every_tail_and_alignment(rend, passes):
    """Slabs of 1, 2, 3 and 4 columns of height 29: 29, 58, 87 and 116 elements, npx mod 4 = 1, 2, 3, 0.  One buffer has an even
    plane stride (every plane 16-byte aligned), the other an odd one (plane 1 only 8-byte aligned), both ways round.  `passes` passes
    with reset into NaNs, then two more without; the sum's bits are rt_film_accumulate's."""
    w, h, params_of, seed = _soft_scene(rend, SLAB_W, SLAB_H)
    frames = _pass_frames(rend, params_of, seed, passes + 2, w, h, "slab")
    for width, x0 in ((1, 0), (2, 7), (3, 20), (4, 33)):
        x1, npx = x0 + width, width * h
        cut = [np.ascontiguousarray(f[:, x0:x1]) for f in frames]
        want1 = V.accumulate_moments_reference(None, None, cut[:passes])
        want2 = V.accumulate_moments_reference(*want1, cut[passes:])
        assert same_bits(want2[0], F.accumulate_reference(None, cut))
        even, odd = (npx + 4) & ~1, (npx + 3) | 1
        for ss, qs in ((even, odd), (odd, even)):
            what = f"passes={passes} columns [{x0}, {x1}) sum_stride={ss} sq_stride={qs}"
            d_sum, d_sq, d_plain = _nan_buffer(rend, 3 * ss), _nan_buffer(rend, 3 * qs), _nan_buffer(rend, 3 * ss)
            try:
                rend.film_accumulate_moments(params_of(seed), x0, x1, passes, True, d_sum, d_sq, ss, qs)
                rend.film_accumulate(params_of(seed), x0, x1, passes, True, d_plain, ss)
                rend.sync()
                s, q, plain = _read(rend, d_sum, (3, ss)), _read(rend, d_sq, (3, qs)), _read(rend, d_plain, (3, ss))
                assert same_bits(s[:, :npx].reshape(3, width, h), want1[0]), what
                assert same_bits(q[:, :npx].reshape(3, width, h), want1[1]), what
                assert same_bits(s, plain), what
                assert np.isnan(s[:, npx:]).all() and np.isnan(q[:, npx:]).all(), what
                rend.film_accumulate_moments(params_of(seed + passes), x0, x1, 2, False, d_sum, d_sq, ss, qs)
                rend.sync()
                s, q = _read(rend, d_sum, (3, ss)), _read(rend, d_sq, (3, qs))
                assert same_bits(s[:, :npx].reshape(3, width, h), want2[0]), what + " + 2"
                assert same_bits(q[:, :npx].reshape(3, width, h), want2[1]), what + " + 2"
                assert np.isnan(s[:, npx:]).all() and np.isnan(q[:, npx:]).all(), what
            finally:
                for p in (d_sum, d_sq, d_plain):
                    rend.free(p)
    assert (want2[1] > 0).any() and not np.array_equal(cut[0], cut[1])


def test_moments_slab_by_slab_in_place(rend):
    """A full-frame pair of buffers filled by two column slabs in place (13 * 29 is odd: the second slab's planes are 8-byte aligned)."""
    w, h, params_of, seed = _soft_scene(rend, SLAB_W, SLAB_H)
    frames = _pass_frames(rend, params_of, seed, 5, w, h, "slab")
    want = V.accumulate_moments_reference(None, None, frames)
    d_sum, d_sq = _nan_buffer(rend, 3 * w * h), _nan_buffer(rend, 3 * w * h)
    try:
        for x0, x1 in ((0, 13), (13, w)):
            rend.film_accumulate_moments(params_of(seed), x0, x1, 5, True, d_sum + 8 * x0 * h, d_sq + 8 * x0 * h, w * h, w * h)
        rend.sync()
        assert same_bits(_read(rend, d_sum, (3, w, h)), want[0]) and same_bits(_read(rend, d_sq, (3, w, h)), want[1])
    finally:
        rend.free(d_sum)
        rend.free(d_sq)


# ---------------------------------------------------------------------------------------------------------------------
# The filter on uploaded sums

# (levels, normal_shin, kappa, var_floor, demodulate, prefilter, n): levels 0, 1, 2, 5 (both parities of the ping-pong), both prefilter
# and demodulate values, kappa 0 with var_floor 0, a var_floor alone
SETTINGS = [(0, 32, 1.5, 0.0, 0, 0, 2), (0, 1, 1.0, 0.0, 1, 1, 7), (1, 32, 1.5, 0.0, 1, 1, 2), (1, 4, 1.0, 0.0, 0, 0, 7), (2, 32, 0.75, 0.0, 1, 0, 3),
            (2, 1024, 2.0, 4.0, 0, 1, 4), (5, 32, 1.5, 0.0, 1, 1, 4), (5, 2, 0.0, 0.0, 0, 1, 3), (5, 32, 0.0, 9.0, 1, 0, 2), (4, 32, 1.5, 0.0, 1, 1, 4)]
SIX_SETTINGS = [(6, 1, 1.5, 0.0, 0, 1, 3), (6, 1024, 1.0, 0.0, 1, 0, 3)]
GRID_CAP_SETTING = (2, 4, 1.5, 0.0, 1, 1, 3)


def _filter(rend, ws, h, gd, settings, seed):
    """rt_film_denoise_variance for every setting on sums of noisy_passes over the guides gd, with strides larger than ws*h and odd
    (planes only 8-byte aligned, guide planes 4-byte) and a sentinel in the padding of every buffer."""
    rng = np.random.default_rng(seed)
    npx = ws * h
    ss, qs, gs, os_, wk = ((npx + k) | 1 for k in (3, 9, 1, 5, 7))
    hg = np.full((8, gs), np.float32(-5.0))
    hg[:, :npx] = gd.reshape(8, -1)
    d_sum, d_sq, d_g, d_out, d_work = rend.malloc(24 * ss), rend.malloc(24 * qs), rend.malloc(32 * gs), rend.malloc(32 * os_), rend.malloc(32 * wk)
    try:
        rend.h2d(d_g, hg)
        for levels, shin, kappa, floor, dem, pre, n in settings:
            s, q = V.accumulate_moments_reference(None, None, noisy_passes(rng, ws, h, n))
            hs, hq = np.full((3, ss), -12345.0), np.full((3, qs), -54321.0)
            hs[:, :npx], hq[:, :npx] = s.reshape(3, -1), q.reshape(3, -1)
            rend.h2d(d_sum, hs)
            rend.h2d(d_sq, hq)
            rend.h2d(d_out, np.full(4 * os_, -777.0))
            rend.h2d(d_work, np.full(4 * wk, -888.0))
            rend.film_denoise_variance(d_sum, d_sq, ws, h, n, d_g, d_out, d_work if levels >= 1 else None, levels=levels, normal_shin=shin,
                                       kappa=kappa, var_floor=floor, demodulate=dem, prefilter=pre, sum_stride=ss, sq_stride=qs, guide_stride=gs,
                                       out_stride=os_, work_stride=wk)
            rend.sync()
            got, work = _read(rend, d_out, (4, os_)), _read(rend, d_work, (4, wk))
            want = V.denoise_variance_reference(s, q, n, gd, levels, shin, kappa, floor, dem, pre)
            what = f"{ws}x{h} levels={levels} shin={shin} kappa={kappa} var_floor={floor} demodulate={dem} prefilter={pre} n={n}"
            assert np.isfinite(want).all(), what
            bad = np.argwhere(got[:, :npx].reshape(4, ws, h).view(np.uint64) != want.view(np.uint64))
            assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[:, :npx].reshape(4, ws, h)[tuple(bad[0])], want[tuple(bad[0])])
            assert (got[:, npx:] == -777.0).all() and (work[:, npx:] == -888.0).all(), what
            if levels < 1:
                assert (work == -888.0).all(), what
            assert same_bits(_read(rend, d_sum, (3, ss)), hs) and same_bits(_read(rend, d_sq, (3, qs)), hq), what     # the inputs are read only
        assert same_bits(_read(rend, d_g, (8, gs), np.float32), hg)
    finally:
        for p in (d_sum, d_sq, d_g, d_out, d_work):
            rend.free(p)


@pytest.mark.parametrize("ws, h", FRAMES)
def test_filter_matches_the_reference(rend, ws, h):
    _filter(rend, ws, h, frame_guides(ws, h), SETTINGS, ws * 100 + h)


@pytest.mark.parametrize("ws, h", chs.SIX_FRAMES)
def test_filter_six_levels(rend, ws, h):
    """levels = 6, taps 32 pixels apart, on guides no rendered scene gives (tests/closest_hit_scenes.py: a 1-pixel checkerboard of ids,
    small blocks, misses, an id above 1024, per-pixel random normals, albedos from 0 to 1e30)."""
    _filter(rend, ws, h, np.array(chs.synthetic_guides(ws, h, 0)), SIX_SETTINGS, ws + h)


def test_filter_loops_past_the_grid_cap(rend):
    """A frame with more pixels than the launch has threads (8 blocks of 256 per CU): the grid-stride loops of the prepare kernel and of
    the level kernel take a second turn.  Sized as tests/test_gpu_denoise.py sizes its frame: 1031 x 523 on 256 CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == rend.kernel_info()["cu_count"]                  # the number the library sizes the grid by
    ws, h = chs.grid_cap_frame(cus)
    assert ws * h > 8 * 256 * cus
    t0 = time.perf_counter()
    _filter(rend, ws, h, np.array(chs.synthetic_guides(ws, h, 0)), [GRID_CAP_SETTING], 77)
    print(f"grid cap: {ws} x {h} on {cus} CUs; reference, device and read-back {time.perf_counter() - t0:.2f} s")


def test_planes_far_apart(rend):
    """Every plane offset is 64-bit: the 37 x 29 filter at two levels four times, one of sum_stride, sq_stride, out_stride and
    work_stride 2^28 + 1 each time, so that plane 2 starts past byte 2^32.  One big buffer at a time, of which only the plane heads
    are written and read, a sentinel behind each.  Without demodulation, so that the work buffer holds the first level's result as
    the reference states it for levels = 1."""
    ws, h = 37, 29
    npx = ws * h
    gd = frame_guides(ws, h)
    s, q = V.accumulate_moments_reference(None, None, noisy_passes(np.random.default_rng(3), ws, h, 3))
    out2, out1 = (V.denoise_variance_reference(s, q, 3, gd, lv, 32, 1.5, 0.0, 0, 1) for lv in (2, 1))
    assert np.isfinite(out2).all() and np.isfinite(out1).all() and not np.array_equal(out2, out1)
    big = 2 ** 28 + 1
    assert 8 * 2 * big > 2 ** 32
    planes = dict(sum=3, sq=3, out=4, work=4)
    fill = dict(out=-777.0, work=-888.0)
    t0 = time.perf_counter()
    d_g = rend.malloc(32 * npx)
    try:
        rend.h2d(d_g, gd)
        for which in planes:
            strides = {k: (big if k == which else npx + 3) for k in planes}
            bufs = {k: rend.malloc(8 * ((planes[k] - 1) * strides[k] + npx + 1)) for k in planes}
            try:
                for k, host in (("sum", s), ("sq", q)):
                    for c in range(3):
                        rend.h2d(bufs[k] + 8 * c * strides[k], np.concatenate([host[c].reshape(-1), [-12345.0]]))
                for k in ("out", "work"):
                    for c in range(4):
                        rend.h2d(bufs[k] + 8 * c * strides[k], np.full(npx + 1, fill[k]))
                rend.film_denoise_variance(bufs["sum"], bufs["sq"], ws, h, 3, d_g, bufs["out"], bufs["work"], levels=2, normal_shin=32, kappa=1.5,
                                           var_floor=0.0, demodulate=0, prefilter=1, sum_stride=strides["sum"], sq_stride=strides["sq"],
                                           out_stride=strides["out"], work_stride=strides["work"])
                rend.sync()
                for c in range(4):
                    go = _read(rend, bufs["out"] + 8 * c * strides["out"], (npx + 1,))
                    gw = _read(rend, bufs["work"] + 8 * c * strides["work"], (npx + 1,))
                    assert go[-1] == -777.0 and gw[-1] == -888.0, (which, c)
                    assert same_bits(np.ascontiguousarray(go[:-1]), np.ascontiguousarray(out2[c].reshape(-1))), f"{which}_stride 2^28 + 1: out plane {c}"
                    assert same_bits(np.ascontiguousarray(gw[:-1]), np.ascontiguousarray(out1[c].reshape(-1))), f"{which}_stride 2^28 + 1: work plane {c}"
                for k, host in (("sum", s), ("sq", q)):
                    for c in range(3):
                        back = _read(rend, bufs[k] + 8 * c * strides[k], (npx + 1,))
                        assert back[-1] == -12345.0 and same_bits(np.ascontiguousarray(back[:-1]), np.ascontiguousarray(host[c].reshape(-1))), (which, k, c)
            finally:
                for b in bufs.values():
                    rend.free(b)
    finally:
        rend.free(d_g)
    print(f"planes far apart: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------
# Through Film, and the quality figures

def test_film_moments_denoise_resolve_variance(rend):
    w, h, params_of, seed = _soft_scene(rend)
    frames = _pass_frames(rend, params_of, seed, 4, w, h, "soft")
    s, q = V.accumulate_moments_reference(None, None, frames)
    with Film(rend, moments=True) as film:
        film.accumulate(params_of(seed), 4)
        plain8, plain32 = film.resolve(white=400.0, f32=True)
        film.denoise(variance=True)
        gd = _read(rend, film.d_guides, (8, w, h), np.float32)
        assert same_bits(gd, np.array(vc.guides()))
        u8, f32 = film.resolve(white=400.0, gamma=2, f32=True, denoised=True)
        den = V.denoise_variance_reference(s, q, 4, gd, 4, 32, V.KAPPA, 0.0, 1, 1)
        v = F.tone_reference(den[:3], 1, 1.0, 400.0, 2)
        assert same_bits(f32, v.astype(np.float32)) and np.array_equal(u8, F.clip_reference(v)[[0, 2, 1]])
        assert same_bits(_read(rend, film.d_denoised_var, (4, w, h)), den)
        again8, again32 = film.resolve(white=400.0, f32=True)     # the plain resolve is what it was
        assert same_bits(again32, plain32) and np.array_equal(again8, plain8)
        assert same_bits(plain32, F.tone_reference(s, 4, 1.0, 400.0, 1).astype(np.float32))
        var = film.variance()
        assert same_bits(var, V.denoise_variance_reference(s, q, 4, gd, 0, 1, 0.0, 0.0, 0, 0)[3]) and (var > 0).any()
        _, f32b = film.resolve(white=400.0, gamma=2, u8=False, f32=True, denoised=True)          # variance() left the filtered mean alone
        assert same_bits(f32b, f32)
        film.denoise(variance=True, levels=1, normal_shininess=4, kappa=0.75, var_floor=2.0, demodulate=False, prefilter=False)
        _, f32 = film.resolve(u8=False, f32=True, denoised=True)
        assert same_bits(f32, V.denoise_variance_reference(s, q, 4, gd, 1, 4, 0.75, 2.0, 0, 0)[:3].astype(np.float32))
        film.denoise()                                            # the fixed-sigma filter on the same film: the parent's result
        _, f32 = film.resolve(u8=False, f32=True, denoised=True)
        assert same_bits(f32, D.denoise_reference(s, 4, gd, 4, 32, F.DENOISE_SIGMA, 1).astype(np.float32))
        film.clear()
        film.accumulate(params_of(seed), 1)
        with pytest.raises(ValueError, match="at least 2 passes"):
            film.denoise(variance=True)


def test_quality_beats_the_raw_mean_and_the_fixed_sigma(rend):
    """tests/test_variance.py's quality test through the device: soft_default_64_d4 with ONE shadow sample, truth the mean of 1024 film
    passes at seeds 1000 and up.  Film.denoise(variance=True) at its defaults is below the raw mean at n = 2, 4, 8, 16 and below
    Film.denoise() at its defaults at n = 4, 8, 16.  The ratios are printed.  (Measured on an MI355X: see DESIGN.md.)"""
    w, h, params_of, seed = _soft_scene(rend, shadow_samples=1)
    with Film(rend) as truth_film, Film(rend, moments=True) as film:
        truth_film.accumulate(params_of(vc.TRUTH_SEED), vc.TRUTH_PASSES)
        rend.sync()
        truth = _read(rend, truth_film.d_sum, (3, w, h)) / float(vc.TRUTH_PASSES)
        for n in vc.QUALITY_N:
            film.accumulate(params_of(seed + film.passes), n - film.passes)
            rend.sync()
            raw = vc.rmse(_read(rend, film.d_sum, (3, w, h)) / float(n), truth)
            film.denoise()
            rend.sync()
            parent = vc.rmse(_read(rend, film.d_denoised, (3, w, h)), truth)
            film.denoise(variance=True)
            rend.sync()
            ours = vc.rmse(_read(rend, film.d_denoised_var, (4, w, h)), truth)
            print(f"quality n={n}: rmse raw {raw:.4f} fixed sigma {parent:.4f} ({parent / raw:.4f}) variance-guided {ours:.4f} ({ours / raw:.4f})")
            assert ours < raw, (n, ours, raw)
            if n >= 4:
                assert ours < parent, (n, ours, parent)


# ---------------------------------------------------------------------------------------------------------------------
# Error paths

def test_errors_leave_the_outputs_untouched(rend):
    import python_ray_tracer_amd as pkg
    w, h, params_of, seed = _soft_scene(rend, SLAB_W, SLAB_H)
    npx = w * h
    nan, inf = float("nan"), float("inf")
    d_g, d_sum, d_sq = rend.malloc(32 * npx), rend.malloc(24 * npx), rend.malloc(24 * npx)
    d_out, d_work = rend.malloc(32 * npx), rend.malloc(32 * npx)
    try:
        rend.h2d(d_sum, np.full(3 * npx, -777.0))
        rend.h2d(d_sq, np.full(3 * npx, -888.0))
        p = params_of(seed)
        acc = lambda *a: rend.film_accumulate_moments(*a)
        bad = {"passes 0": lambda: acc(p, 0, w, 0, True, d_sum, d_sq),
               "NULL sum": lambda: acc(p, 0, w, 1, True, None, d_sq),
               "NULL sq": lambda: acc(p, 0, w, 1, True, d_sum, None),
               "sq is the sum": lambda: acc(p, 0, w, 1, True, d_sum, d_sum),
               "short sum_stride": lambda: acc(p, 0, w, 1, True, d_sum, d_sq, npx - 1, npx),
               "short sq_stride": lambda: acc(p, 0, w, 1, True, d_sum, d_sq, npx, npx - 1),
               "x1 > w": lambda: acc(p, 0, w + 1, 1, True, d_sum, d_sq, 2 * npx, 2 * npx),
               "x0 >= x1": lambda: acc(p, 5, 5, 1, True, d_sum, d_sq)}
        for what, call in bad.items():
            with pytest.raises(pkg.RenderError) as e:
                call()
            assert e.value.status == L.RT_ERR_BAD_ARG, what
        rend.sync()
        assert (_read(rend, d_sum, (3 * npx,)) == -777.0).all() and (_read(rend, d_sq, (3 * npx,)) == -888.0).all(), "a refused call touched the sums"
        rend.h2d(d_g, frame_guides(w, h))
        rend.h2d(d_sum, np.full(3 * npx, 100.0))
        rend.h2d(d_sq, np.full(3 * npx, 5050.0))                   # two passes of 50 +- 5: mean 50, variance of the mean 25 per channel
        rend.h2d(d_out, np.full(4 * npx, -777.0))
        rend.h2d(d_work, np.full(4 * npx, -888.0))
        ok = dict(levels=2, normal_shin=32, kappa=1.0, var_floor=0.0, demodulate=1, prefilter=1)
        den = lambda *a, **kw: rend.film_denoise_variance(*a, **{**ok, **kw})
        good = (d_sum, d_sq, w, h, 2, d_g, d_out, d_work)
        swap = lambda i, v: good[:i] + (v,) + good[i + 1:]
        bad = {"NULL sum": lambda: den(*swap(0, None)), "NULL sq": lambda: den(*swap(1, None)), "NULL guides": lambda: den(*swap(5, None)),
               "NULL out": lambda: den(*swap(6, None)), "n 1": lambda: den(*swap(4, 1)), "n 0": lambda: den(*swap(4, 0)),
               "levels -1": lambda: den(*good, levels=-1), "levels 7": lambda: den(*good, levels=7),
               "shin 0": lambda: den(*good, normal_shin=0), "shin 3": lambda: den(*good, normal_shin=3), "shin 2048": lambda: den(*good, normal_shin=2048),
               "kappa < 0": lambda: den(*good, kappa=-1.0), "kappa NaN": lambda: den(*good, kappa=nan), "kappa inf": lambda: den(*good, kappa=inf),
               "var_floor < 0": lambda: den(*good, var_floor=-1.0), "var_floor NaN": lambda: den(*good, var_floor=nan),
               "var_floor inf": lambda: den(*good, var_floor=inf), "demodulate 2": lambda: den(*good, demodulate=2),
               "prefilter 2": lambda: den(*good, prefilter=2), "prefilter -1": lambda: den(*good, prefilter=-1),
               "ws 0": lambda: den(*swap(2, 0)), "h 0": lambda: den(*swap(3, 0)),
               "ws*h above RT_FILM_MAX_PIXELS": lambda: den(d_sum, d_sq, 2 ** 14, 2 ** 13 + 1, 2, d_g, d_out, d_work, sum_stride=2 ** 28, sq_stride=2 ** 28,
                                                            guide_stride=2 ** 28, out_stride=2 ** 28, work_stride=2 ** 28),
               "short sum_stride": lambda: den(*good, sum_stride=npx - 1), "short sq_stride": lambda: den(*good, sq_stride=npx - 1),
               "short guide_stride": lambda: den(*good, guide_stride=npx - 1), "short out_stride": lambda: den(*good, out_stride=npx - 1),
               "short work_stride": lambda: den(*good, work_stride=npx - 1),
               "NULL work with one level": lambda: den(*swap(7, None), levels=1),
               "out is the sum": lambda: den(*swap(6, d_sum)), "out is sq": lambda: den(*swap(6, d_sq)), "out is the guides": lambda: den(*swap(6, d_g)),
               "work is the sum": lambda: den(*swap(7, d_sum)), "work is sq": lambda: den(*swap(7, d_sq)), "work is the guides": lambda: den(*swap(7, d_g)),
               "work is out": lambda: den(*swap(7, d_out))}
        for what, call in bad.items():
            with pytest.raises(pkg.RenderError) as e:
                call()
            assert e.value.status == L.RT_ERR_BAD_ARG, what
        lib = L.load()                                            # a NULL settings pointer
        assert lib.rt_film_denoise_variance(rend._ctx, d_sum, npx, d_sq, npx, w, h, 2, d_g, npx, None, d_out, npx, d_work, npx, None) == L.RT_ERR_BAD_ARG
        rend.sync()
        assert (_read(rend, d_out, (4 * npx,)) == -777.0).all() and (_read(rend, d_work, (4 * npx,)) == -888.0).all()
        den(*good, demodulate=0)                                  # the context is still usable; a constant stays the constant
        den(d_sum, d_sq, w, h, 2, d_g, d_work, None, levels=0)     # (no level needs no work buffer)
        rend.sync()
        out, work = _read(rend, d_out, (4, npx)), _read(rend, d_work, (4, npx))
        assert np.allclose(out[:3], 50.0, rtol=1e-14) and (out[3] > 0).all() and (out[3] <= 75.0).all()     # (a pixel alone in its object keeps v_0 = 75)
        assert (work[:3] == 50.0).all() and (work[3] == 75.0).all()
    finally:
        for p_ in (d_g, d_sum, d_sq, d_out, d_work):
            rend.free(p_)


# ---------------------------------------------------------------------------------------------------------------------
# Streams

def test_two_streams_their_own_buffers(rend):
    """Moments and filters of two slabs on two streams, queued together: the serial results (the pass scratch is per stream)."""
    w, h, params_of, seed = _soft_scene(rend, SLAB_W, SLAB_H)
    frames = _pass_frames(rend, params_of, seed, 5, w, h, "slab")
    gd_full = D.guides_reference(*(vc.fixture()[k] for k in ("spheres", "planes", "cam_origin", "cam_rot")), w, h,
                                 raygen=raygen_closed_form(w, h, float(vc.fixture()["fov"])))
    slabs = ((0, 13), (13, w))
    streams = [rend.stream_create(), rend.stream_create()]
    bufs = []
    try:
        for (x0, x1), st in zip(slabs, streams):
            npx = (x1 - x0) * h
            b = dict(g=rend.malloc(32 * npx), s=_nan_buffer(rend, 3 * npx), q=_nan_buffer(rend, 3 * npx), out=rend.malloc(32 * npx), work=rend.malloc(32 * npx))
            bufs.append(b)
            rend.render_guides(x0, x1, b["g"], npx, st)
            rend.film_accumulate_moments(params_of(seed), x0, x1, 5, True, b["s"], b["q"], stream=st)
            rend.film_denoise_variance(b["s"], b["q"], x1 - x0, h, 5, b["g"], b["out"], b["work"], levels=3, normal_shin=32, kappa=1.5, stream=st)
        for st in streams:
            rend.sync(st)
        for (x0, x1), b in zip(slabs, bufs):
            ws = x1 - x0
            s, q = V.accumulate_moments_reference(None, None, [np.ascontiguousarray(f[:, x0:x1]) for f in frames])
            gd = np.ascontiguousarray(gd_full[:, x0:x1])
            assert same_bits(_read(rend, b["g"], (8, ws, h), np.float32), gd), (x0, x1)
            assert same_bits(_read(rend, b["s"], (3, ws, h)), s) and same_bits(_read(rend, b["q"], (3, ws, h)), q), (x0, x1)
            assert same_bits(_read(rend, b["out"], (4, ws, h)), V.denoise_variance_reference(s, q, 5, gd, 3, 32, 1.5, 0.0, 1, 1)), (x0, x1)
    finally:
        for st in streams:
            rend.stream_destroy(st)
        for b in bufs:
            for p in b.values():
                rend.free(p)


# ---------------------------------------------------------------------------------------------------------------------
# The example

def test_example_with_denoise_variance_writes_png(tmp_path):
    """examples/render_png.py --denoise-variance: eight passes of the sky scene with soft shadows, filtered, in a process of its own."""
    from PIL import Image
    out = str(tmp_path / "var.png")
    log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--sky", "--soft", "--shadow-samples", "1", "--passes", "8",
                                   "--white", "400", "--size", "64x64", "--frames", "2", "--denoise-variance", "--kappa", "1", "--denoise-levels", "3",
                                   "--out", out], text=True)
    assert "wrote" in log and "denoise_variance=True" in log
    img = np.asarray(Image.open(out))
    assert img.shape == (64, 64, 3) and img.any() and len(np.unique(img)) > 32
