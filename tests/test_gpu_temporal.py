"""Temporal accumulation on the GPU (rt_film_temporal; the kernel of rt_temporal.h).  Truth is the numpy restatement of
python-ray-tracer_amd/temporal.py, which tests/test_temporal.py holds against the kernel's own text on the CPU; every comparison
here is bit for bit.  Four stored scenes under a translated-and-rotated previous camera and under a still one, with random finite
history and lengths (zeros among them), odd strides and NaN sentinels between the planes; a synthetic frame with more pixels than
the launch has threads; through Film: an orbit of three frames against the numpy chain, the error paths, two films on two streams,
the example; and the quality figure on the orbit of tests/temporal_cases.py."""
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
from test_film import same_bits
from feature_gpu import IGNORED, rend   # noqa: F401  (rend: the session's renderer with the pinhole camera restored)
from test_gpu_denoise import _read

from python_ray_tracer_amd import Film, denoise as D, film as F, temporal as T
from python_ray_tracer_amd import _lib as L

pytestmark = pytest.mark.gpu


def _set_view(r, f):
    r.set_camera(f["cam"][0], f["cam"][1])
    r.set_raygen(f["w"], f["h"], *f["raygen"])


def _run(r, f, s, n, hist, hl, settings, pads=(3, 1, 5, 7, 9, 11, 13), stream=None):
    """rt_film_temporal on uploaded buffers whose planes are pads[i] elements longer than the frame (odd strides: planes only 8- and
    4-byte aligned), NaN in every gap: (out (3, w, h), out_len (w, h)) after checking that gaps and inputs are what they were."""
    w, h = f["w"], f["h"]
    npx = w * h
    strides = [(npx + p) | 1 if p else npx for p in pads]
    ss, gs, hs, ls, hgs, os_, ols = strides
    host = {"sum": (s, 3, ss, np.float64), "guides": (f["guides"], 8, gs, np.float32), "hist": (hist, 3, hs, np.float64),
            "hist_len": (hl, 1, ls, np.float32), "hist_guides": (f["hist_guides"], 8, hgs, np.float32),
            "out": (np.full((3, w, h), -777.0), 3, os_, np.float64), "out_len": (np.full((w, h), -888.0, np.float32), 1, ols, np.float32)}
    dev, up = {}, {}
    try:
        for k, (a, planes, stride, dt) in host.items():
            p = np.full((planes, stride), np.nan, dt)
            p[:, :npx] = np.asarray(a).reshape(planes, -1)
            dev[k] = r.malloc(p.nbytes)
            r.h2d(dev[k], p)
            up[k] = p
        depth_tol, normal_cos, max_history = settings
        r.film_temporal(dev["sum"], n, dev["guides"], dev["hist"], dev["hist_len"], dev["hist_guides"], f["prev_cam"][0], f["prev_cam"][1],
                        dev["out"], dev["out_len"], depth_tol=depth_tol, normal_cos=normal_cos, max_history=max_history, sum_stride=ss,
                        guide_stride=gs, hist_stride=hs, hist_guide_stride=hgs, out_stride=os_, stream=stream)
        r.sync(stream)
        got = {k: _read(r, dev[k], up[k].shape, up[k].dtype) for k in host}
    finally:
        for d in dev.values():
            r.free(d)
    for k in ("sum", "guides", "hist", "hist_len", "hist_guides"):
        assert same_bits(got[k], up[k]), f"{k} is read only"
    assert np.isnan(got["out"][:, npx:]).all() and np.isnan(got["out_len"][:, npx:]).all(), "a gap between planes was written"
    return got["out"][:, :npx].reshape(3, w, h), got["out_len"][0, :npx].reshape(w, h)


def _same(what, got, want):
    ut = np.uint64 if want.dtype == np.float64 else np.uint32
    bad = np.argwhere(np.ascontiguousarray(got).view(ut) != np.ascontiguousarray(want).view(ut))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_symbol_present():
    lib = L.load()
    assert hasattr(lib, "rt_film_temporal") and lib.rt_abi_version() == 7


# ---------------------------------------------------------------------------------------------------------------------
# Uploaded frames against temporal_reference

@pytest.mark.parametrize("prev", ["moved", "still"])
@pytest.mark.parametrize("name", ["odd_37x29", "planes_only_32", "spheres_only_32", "inside_sphere_32"])
def test_temporal_matches_the_reference(rend, name, prev):
    """Random finite sums, history and lengths (about a sixth of the lengths 0) on the real guides of both cameras; three settings:
    the loose one of the cases, a tight one with a low cap, and max_history 0."""
    f = tc.frame(name, prev)
    _set_view(rend, f)
    w, h = f["w"], f["h"]
    for k, (settings, n) in enumerate(((tc.SETTINGS, 4), ((0.02, 0.95, 3.5), 1), ((0.25, 0.5, 0.0), 7))):
        s, hist, hl = tc.random_inputs(w, h, n, 300 + k)
        want, want_len = tc.reference(f, s, n, hist, hl, settings)
        out, out_len = _run(rend, f, s, n, hist, hl, settings)
        what = f"{name} {prev} {settings} n={n}"
        _same(what, out, want)
        _same(what + " length", out_len, want_len)
        fresh = int((want_len == np.float32(n)).sum())
        assert (hl == 0).sum() > w * h // 10
        if settings[2] == 0.0:
            assert fresh == w * h
        elif k == 0:
            assert 0 < fresh < 3 * w * h // 4, (what, fresh)       # both kinds of pixel are there
    if name == "spheres_only_32":
        assert (f["guides"][7] < 0).any()                         # misses


def test_backward_facing_history_is_all_fresh(rend):
    f = tc.frame("odd_37x29", "backward")
    _set_view(rend, f)
    s, hist, hl = tc.random_inputs(f["w"], f["h"], 2, 310)
    out, out_len = _run(rend, f, s, 2, hist, hl, tc.SETTINGS, pads=(0,) * 7)
    _same("backward", out, s / np.float64(2))
    assert (out_len == 2.0).all()


def test_temporal_loops_past_the_grid_cap(rend):
    """A synthetic frame (a wall with ids in blocks, no render) with more pixels than the launch has threads (8 blocks of 256 per
    CU): the grid-stride loop takes a second turn.  (torch is imported with the module, before the library loads.)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == rend.kernel_info()["cu_count"]                  # the number the library sizes the grid by
    w, h = chs.grid_cap_frame(cus)
    assert w * h > 8 * 256 * cus
    t0 = time.perf_counter()
    f, s, hist, hl = tc.synthetic_frame(w, h)
    want, want_len = tc.reference(f, s, 3, hist, hl, (0.05, 0.9, 6.0))
    t1 = time.perf_counter()
    _set_view(rend, f)
    out, out_len = _run(rend, f, s, 3, hist, hl, (0.05, 0.9, 6.0), pads=(1, 0, 3, 1, 5, 0, 3))
    _same("grid cap", out, want)
    _same("grid cap length", out_len, want_len)
    fresh = int((want_len == 3.0).sum())
    assert w * h // 20 < fresh < w * h // 2                       # refused taps and kept ones, in numbers
    print(f"grid cap: {w} x {h} on {cus} CUs, {fresh} fresh; reference {t1 - t0:.2f} s, device and read-back {time.perf_counter() - t1:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------
# Through Film

def _orbit_renderer(r, sc, shadow_samples):
    r.set_scene(sc["spheres"], sc["lights"], sc["planes"], materials=sc["materials"], light_radius=sc["light_radius"], shadow_samples=shadow_samples)
    r.set_lens(0.0, 1.0)
    r.set_raygen(sc["w"], sc["h"], *sc["raygen"])
    return lambda seed: r.params(**IGNORED, depth=sc["depth"], aa=0, seed=seed)


def _pass_sum(r, params_of, seed, n, w, h):
    """accumulate_reference of n pass frames rendered one by one with the current camera."""
    d32 = r.malloc(12 * w * h)
    frames = []
    try:
        for i in range(n):
            r.render_device(params_of(seed + i), 0, w, None, d32)
            r.sync()
            frames.append(_read(r, d32, (3, w, h), np.float32))
    finally:
        r.free(d32)
    return F.accumulate_reference(None, frames)


def test_film_orbit_against_the_numpy_chain(rend):
    """Three camera steps, two passes each.  The first frame ends without temporal() (its plain mean, with length 2 and the guides
    of guides(), becomes the history through next_frame), the second with it (a swap).  Then the filter and the resolve on the
    temporal mean."""
    sc = tc.orbit_scene()
    w, h, rg = sc["w"], sc["h"], sc["raygen"]
    params_of = _orbit_renderer(rend, sc, 4)
    cams, n = sc["cameras"][:3], 2
    settings = (T.DEPTH_TOL, T.NORMAL_COS, 3.0)                   # (a cap that binds at the third frame)
    hist = hist_len = hist_guides = None
    with Film(rend) as film:
        for k, cam in enumerate(cams):
            rend.set_camera(*cam)
            total = _pass_sum(rend, params_of, 40 + 10 * k, n, w, h)
            gd = D.guides_reference(sc["spheres"], sc["planes"], cam[0], cam[1], w, h, raygen=rg)
            film.next_frame()
            film.accumulate(params_of(40 + 10 * k), n)
            if k == 0:
                assert same_bits(film.guides(), gd)
                want, want_len = total / np.float64(n), np.full((w, h), n, np.float32)
            else:
                film.temporal(max_history=settings[2])
                want, want_len = T.temporal_reference(total, n, gd, hist, hist_len, hist_guides, cam, cams[k - 1], rg, w, h, *settings)
                rend.sync()
                _same(f"frame {k}", _read(rend, film.d_temporal, (3, w, h)), want)
                _same(f"frame {k} length", _read(rend, film.d_temporal_len, (w, h), np.float32), want_len)
                assert (want_len > n).sum() > w * h // 2 and (want_len == n).any()
            hist, hist_len, hist_guides = want, want_len, gd
        assert hist_len.max() == 5.0                              # 2 + 2 capped at 3, + 2
        _, f32 = film.resolve(white=400.0, u8=False, f32=True, temporal=True)
        assert same_bits(f32, F.tone_reference(hist, 1, 1.0, 400.0, 1).astype(np.float32))
        film.denoise(temporal=True)
        u8, f32 = film.resolve(white=400.0, gamma=2, f32=True, denoised=True, temporal=True)
        v = F.tone_reference(D.denoise_reference(hist, 1, hist_guides, 4, 32, F.DENOISE_SIGMA, 1), 1, 1.0, 400.0, 2)
        assert same_bits(f32, v.astype(np.float32)) and np.array_equal(u8, F.clip_reference(v)[[0, 2, 1]])
        _, plain = film.resolve(white=400.0, u8=False, f32=True)   # the plain resolve is the mean of this frame's passes
        assert same_bits(plain, F.tone_reference(total, n, 1.0, 400.0, 1).astype(np.float32))


def test_quality_the_history_helps_matte_pixels(rend):
    """The orbit of tests/temporal_cases.py: 8 camera steps of 2 degrees, 4 passes per frame, ONE shadow sample, the scene of
    soft_default_64_d4 with a matte floor.  Truth is the mean of 1024 passes at the last camera; RMSE in linear colour.  Asserted:
    over matte pixels (no reflection; the table has no transparency and no specular), which must be at least half the frame, the
    temporal mean at Film.temporal's defaults is closer to the truth than the raw 4-pass mean.  The figures are results, printed
    (Temporal accumulation, has them with the sweep)."""
    sc = tc.orbit_scene()
    w, h = sc["w"], sc["h"]
    params_of = _orbit_renderer(rend, sc, 1)
    last = sc["cameras"][-1]
    matte = tc.matte_mask(sc, D.guides_reference(sc["spheres"], sc["planes"], last[0], last[1], w, h, raygen=sc["raygen"]))
    assert matte.sum() >= w * h // 2
    with Film(rend) as truth_film, Film(rend) as film:
        for k, cam in enumerate(sc["cameras"]):
            rend.set_camera(*cam)
            film.next_frame()
            film.accumulate(params_of(1 + tc.ORBIT_PASSES * k), tc.ORBIT_PASSES)
            film.temporal()
        truth_film.accumulate(params_of(5000), 1024)
        film.denoise(temporal=True)
        rend.sync()
        truth = _read(rend, truth_film.d_sum, (3, w, h)) / 1024.0
        raw = _read(rend, film.d_sum, (3, w, h)) / float(tc.ORBIT_PASSES)
        tmp = _read(rend, film.d_temporal, (3, w, h))
        den = _read(rend, film.d_denoised, (3, w, h))
        length = _read(rend, film.d_temporal_len, (w, h), np.float32)
    rmse = lambda a, m: float(np.sqrt(np.mean((a - truth)[:, m] ** 2)))
    every = np.ones((w, h), bool)
    for what, m in (("whole frame", every), ("matte", matte), ("not matte", ~matte)):
        print(f"quality, {what} ({int(m.sum())} pixels): rmse raw {rmse(raw, m):.4f} temporal {rmse(tmp, m):.4f} temporal+denoise {rmse(den, m):.4f}")
    print(f"quality: history length mean {float(length.mean()):.2f}, {int((length == tc.ORBIT_PASSES).sum())} fresh pixels")
    assert rmse(tmp, matte) < rmse(raw, matte), (rmse(tmp, matte), rmse(raw, matte))


# ---------------------------------------------------------------------------------------------------------------------
# Error paths

def test_errors_leave_the_outputs_untouched(rend):
    import python_ray_tracer_amd as pkg
    f = tc.frame("odd_37x29", "moved")
    _set_view(rend, f)
    w, h = f["w"], f["h"]
    npx = w * h
    names = ("sum", "guides", "hist", "len", "hguides", "out", "olen")
    size = dict(sum=24, guides=32, hist=24, len=4, hguides=32, out=24, olen=4)
    d = {k: rend.malloc(size[k] * npx) for k in names}
    nan, inf = float("nan"), float("inf")
    try:
        rend.h2d(d["sum"], np.full(3 * npx, 50.0))
        rend.h2d(d["hist"], np.full(3 * npx, 50.0))
        rend.h2d(d["guides"], np.ascontiguousarray(f["guides"]))
        rend.h2d(d["hguides"], np.ascontiguousarray(f["hist_guides"]))
        rend.h2d(d["len"], np.full(npx, 4.0, np.float32))
        rend.h2d(d["out"], np.full(3 * npx, -777.0))
        rend.h2d(d["olen"], np.full(npx, -888.0, np.float32))
        ok = dict(depth_tol=0.25, normal_cos=0.5, max_history=16.0)

        def call(r=rend, n=2, prev=f["prev_cam"], **kw):
            bufs = {k: kw.pop(k, d[k]) for k in names}
            r.film_temporal(bufs["sum"], n, bufs["guides"], bufs["hist"], bufs["len"], bufs["hguides"], prev[0], prev[1], bufs["out"], bufs["olen"],
                            **{**ok, **kw})

        bad = {f"NULL {k}": (lambda k=k: call(**{k: None})) for k in names}
        bad.update({"n 0": lambda: call(n=0), "n above 2^24": lambda: call(n=(1 << 24) + 1),
                    "depth_tol < 0": lambda: call(depth_tol=-0.1), "depth_tol NaN": lambda: call(depth_tol=nan), "depth_tol inf": lambda: call(depth_tol=inf),
                    "normal_cos > 1": lambda: call(normal_cos=1.5), "normal_cos < -1": lambda: call(normal_cos=-1.5), "normal_cos NaN": lambda: call(normal_cos=nan),
                    "max_history < 0": lambda: call(max_history=-1.0), "max_history inf": lambda: call(max_history=inf), "max_history NaN": lambda: call(max_history=nan),
                    "reserved": lambda: call(reserved=(0, 1)), "reserved 0": lambda: call(reserved=(2, 0)),
                    "prev origin NaN": lambda: call(prev=(np.array([0.0, nan, 0.0]), np.eye(3))),
                    "prev rotation inf": lambda: call(prev=(np.zeros(3), np.full((3, 3), inf))),
                    "short sum_stride": lambda: call(sum_stride=npx - 1), "short guide_stride": lambda: call(guide_stride=npx - 1),
                    "short hist_stride": lambda: call(hist_stride=npx - 1), "short hist_guide_stride": lambda: call(hist_guide_stride=npx - 1),
                    "short out_stride": lambda: call(out_stride=npx - 1)})
        for k in ("sum", "guides", "hist", "len", "hguides"):
            bad[f"out is {k}"] = lambda k=k: call(out=d[k])
            bad[f"out_len is {k}"] = lambda k=k: call(olen=d[k])
        for what, fn in bad.items():
            with pytest.raises(pkg.RenderError) as e:
                fn()
            assert e.value.status == L.RT_ERR_BAD_ARG, what
        lib = L.load()                                            # a NULL settings pointer
        vp = lambda k: ctypes.c_void_p(d[k])
        assert lib.rt_film_temporal(rend._ctx, vp("sum"), npx, 2, vp("guides"), npx, vp("hist"), npx, vp("len"), vp("hguides"), npx, None,
                                    vp("out"), npx, vp("olen"), None) == L.RT_ERR_BAD_ARG
        rend.set_camera(np.array([0.0, nan, 0.0]), np.eye(3))     # a current camera that is not finite
        with pytest.raises(pkg.RenderError) as e:
            call()
        assert e.value.status == L.RT_ERR_BAD_ARG
        with pkg.Renderer(0) as fresh:                            # no camera; no grid; an explicit grid; a grid without extent
            with pytest.raises(pkg.RenderError) as e:
                call(r=fresh)
            assert e.value.status == L.RT_ERR_STATE
            fresh.set_camera(*f["cam"])
            with pytest.raises(pkg.RenderError) as e:             # no grid (the wrapper's default strides are 0 then: give them)
                call(r=fresh, sum_stride=npx, guide_stride=npx, hist_stride=npx, hist_guide_stride=npx, out_stride=npx)
            assert e.value.status == L.RT_ERR_STATE
            px, y0, dy, z0, dz = f["raygen"]
            xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="ij")
            fresh.set_pixel_loc(np.stack([np.full((w, h), px), xs * dy + y0, ys * dz + z0]))
            with pytest.raises(pkg.RenderError) as e:
                call(r=fresh)
            assert e.value.status == L.RT_ERR_STATE
            for grid in ((px, y0, 0.0, z0, dz), (px, y0, dy, z0, 0.0)):
                fresh.set_raygen(w, h, *grid)
                with pytest.raises(pkg.RenderError) as e:
                    call(r=fresh)
                assert e.value.status == L.RT_ERR_STATE, grid
            fresh.set_raygen(2 ** 14, 2 ** 13 + 1, px, y0, dy, z0, dz)          # w*h above RT_FILM_MAX_PIXELS
            with pytest.raises(pkg.RenderError) as e:
                call(r=fresh)
            assert e.value.status == L.RT_ERR_BAD_ARG
        rend.sync()
        assert (_read(rend, d["out"], (3 * npx,)) == -777.0).all() and (_read(rend, d["olen"], (npx,), np.float32) == -888.0).all()
        _set_view(rend, f)                                        # the context is still usable; a constant stays the constant
        call()
        rend.sync()
        out, olen = _read(rend, d["out"], (3 * npx,)), _read(rend, d["olen"], (npx,), np.float32)
        assert set(np.unique(olen)) <= {2.0, 6.0} and (olen == 6.0).any() and (olen == 2.0).any()
        assert np.allclose(out.reshape(3, -1)[:, olen == 6.0], (4.0 * 50.0 + 50.0) / 6.0, rtol=1e-14) and np.allclose(out.reshape(3, -1)[:, olen == 2.0], 25.0)
    finally:
        for p in d.values():
            rend.free(p)


# ---------------------------------------------------------------------------------------------------------------------
# Streams

def test_two_films_on_two_streams(rend):
    """Two films of two scenes carried through a move each, every call of one film on its own stream, queued together: the serial
    results (cameras and grid travel with the launches)."""
    sc = tc.orbit_scene()
    w, h, rg = sc["w"], sc["h"], sc["raygen"]
    _orbit_renderer(rend, sc, 4)                                  # (the frame size, before the films are made)
    streams = [rend.stream_create(), rend.stream_create()]
    films, wants = [Film(rend), Film(rend)], []
    try:
        for i, (film, st) in enumerate(zip(films, streams)):
            params_of = _orbit_renderer(rend, sc, 4 if i == 0 else 2)
            cams = (sc["cameras"][i], sc["cameras"][i + 3])
            for cam in cams:
                rend.set_camera(*cam)
                film.next_frame(stream=st)
                film.accumulate(params_of(70 + i), 2, stream=st)
                film.temporal(stream=st)
            wants.append((i, cams))
        for st in streams:
            rend.sync(st)
        for film, (i, cams) in zip(films, wants):
            params_of = _orbit_renderer(rend, sc, 4 if i == 0 else 2)
            outs = []
            for k, cam in enumerate(cams):
                rend.set_camera(*cam)
                total = _pass_sum(rend, params_of, 70 + i, 2, w, h)
                gd = D.guides_reference(sc["spheres"], sc["planes"], cam[0], cam[1], w, h, raygen=rg)
                if k == 0:
                    outs = [total / np.float64(2), np.full((w, h), 2, np.float32), gd]
                else:
                    want, want_len = T.temporal_reference(total, 2, gd, outs[0], outs[1], outs[2], cam, cams[0], rg, w, h, T.DEPTH_TOL, T.NORMAL_COS, T.MAX_HISTORY)
            _same(f"film {i}", _read(rend, film.d_temporal, (3, w, h)), want)
            _same(f"film {i} length", _read(rend, film.d_temporal_len, (w, h), np.float32), want_len)
            assert (want_len == 4.0).sum() > w * h // 2
    finally:
        for film in films:
            film.close()
        for st in streams:
            rend.stream_destroy(st)


# ---------------------------------------------------------------------------------------------------------------------
# The example

def test_example_with_temporal_writes_a_png(tmp_path):
    """examples/render_png.py --orbit 3 --passes 2 --temporal --denoise, in a fresh child process."""
    from PIL import Image
    out = str(tmp_path / "orbit.png")
    log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--sky", "--soft", "--shadow-samples", "1", "--passes", "2",
                                   "--white", "400", "--size", "64x64", "--orbit", "3", "--temporal", "--denoise", "--denoise-levels", "2", "--out", out],
                                  text=True)
    assert "wrote" in log and "temporal=True" in log and "orbit=3" in log
    img = np.asarray(Image.open(out))
    assert img.shape == (64, 64, 3) and img.any() and len(np.unique(img)) > 32
