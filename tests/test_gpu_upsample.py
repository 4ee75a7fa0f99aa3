"""Guided upsampling on the device (rt_render_guides_grid, rt_film_upsample; python-ray-tracer_amd/csrc/rt_upsample.h).  The guides on
a grid passed by value against rt_set_raygen plus rt_render_guides, bit for bit, in slabs, on a context without a grid, and with the
renderer's own frame untouched; the lift against upsample.upsample_reference bit for bit on the pairs of tests/upsample_cases.py, with
odd strides, sentinels behind every plane and in every pad, with and without the kind plane, from a four-plane mean; the identity of
equal grids; the grid-stride loop; every refusal with its text and untouched outputs; through Film and Upsampler on a rendered scene."""
import numpy as np
import pytest
import torch

from conftest import raygen_closed_form
from feature_gpu import IGNORED
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_denoise import guide_scene
from test_film import same_bits
import upsample_cases as uc
import variance_cases as vc

from python_ray_tracer_amd import Film, Upsampler, denoise as D, film as F, meter as M, upsample as U, variance as V
from python_ray_tracer_amd import _lib as L

pytestmark = pytest.mark.gpu

SENTINEL, KIND_SENTINEL = -777.0, np.float32(-3.0)


def _read(r, d, shape, dtype=np.float64):
    a = np.empty(shape, dtype)
    r.d2h(a, d)
    return a


def _padded(a, stride, fill, dtype):
    p = np.full((a.shape[0], stride), fill, dtype)
    p[:, :a[0].size] = a.reshape(a.shape[0], -1)
    return p


def _set_scene(r, name):
    g, _, _, tex = guide_scene(name)
    if tex is not None:
        r.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]), textures=tex)
    else:
        r.set_scene(g["spheres"], g["lights"], g["planes"])
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(0.0, 1.0)
    return g


# ---------------------------------------------------------------------------------------------------------------------
# rt_render_guides_grid

def _guides_by(r, call, w, h):
    """(8, w, h) float32 that `call(d, stride)` wrote into a NaN-filled buffer with one element of pad per plane."""
    stride = w * h + 1
    d = r.malloc(4 * 8 * stride)
    try:
        r.h2d(d, np.full(8 * stride, np.nan, np.float32))
        call(d, stride)
        r.sync()
        got = _read(r, d, (8, stride), np.float32)
    finally:
        r.free(d)
    assert np.isnan(got[:, w * h:]).all(), "a pad was written"
    return got[:, :w * h].reshape(8, w, h)


@pytest.mark.parametrize("name,w,h", [("odd_37x29", 37, 29), ("odd_37x29", 97, 71), ("c5_s256_d8_sub96", 32, 32)])
def test_guides_grid_is_set_raygen_plus_render_guides(rend, name, w, h):
    g = _set_scene(rend, name)
    rg = raygen_closed_form(w, h, float(g["fov"]))
    rend.set_raygen(w, h, *rg)
    want = _guides_by(rend, lambda d, stride: rend.render_guides(0, w, d, stride), w, h)
    assert same_bits(want, uc.guides(name, w, h)[0])
    # from another grid of the renderer's own, which stays: a low-resolution frame before and after has the same bytes
    lw, lh = 16, 12
    lrg = raygen_closed_form(lw, lh, float(g["fov"]))
    rend.set_raygen(lw, lh, *lrg)
    before = rend.render(0.1, 0.6, 0.4, 2, False, u8=True, f32=True)
    state = (rend.w, rend.h, rend.raygen, dict(rend.generation))
    got = _guides_by(rend, lambda d, stride: rend.render_guides_grid(w, h, rg, 0, w, d, stride), w, h)
    assert same_bits(got, want)
    assert (rend.w, rend.h, rend.raygen, rend.generation) == state
    after = rend.render(0.1, 0.6, 0.4, 2, False, u8=True, f32=True)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    low = _guides_by(rend, lambda d, stride: rend.render_guides(0, lw, d, stride), lw, lh)       # the context's grid is still the low one
    assert same_bits(low, D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], lw, lh, raygen=lrg))
    # two column slabs into one buffer, in place
    cut = w // 3 + 1

    def slabs(d, stride):
        rend.render_guides_grid(w, h, rg, cut, w, d + 4 * cut * h, stride)
        rend.render_guides_grid(w, h, rg, 0, cut, d, stride)
    assert same_bits(_guides_by(rend, slabs, w, h), want)


def test_guides_grid_needs_no_grid_of_the_context():
    import python_ray_tracer_amd as pkg
    name, w, h = "odd_37x29", 37, 29
    want, rg = uc.guides(name, w, h)
    with pkg.Renderer(0) as fresh:
        d = fresh.malloc(4 * 8 * w * h)
        try:
            for text, setup in (("rt_set_scene has not been called", lambda: None),
                                ("rt_set_camera has not been called", lambda: fresh.set_scene(*[guide_scene(name)[0][k] for k in ("spheres", "lights", "planes")]))):
                setup()
                with pytest.raises(pkg.RenderError) as e:
                    fresh.render_guides_grid(w, h, rg, 0, w, d)
                assert e.value.status == L.RT_ERR_STATE and str(e.value).endswith("rt_render_guides_grid: " + text)
            _set_scene(fresh, name)
            assert fresh.w is None and fresh.raygen is None
            fresh.render_guides_grid(w, h, rg, 0, w, d)
            fresh.sync()
            assert same_bits(_read(fresh, d, (8, w, h), np.float32), want)
            with pytest.raises(pkg.RenderError) as e:               # and the context still has none
                fresh.render_guides(0, 1, d, h)
            assert e.value.status == L.RT_ERR_STATE
        finally:
            fresh.free(d)


# ---------------------------------------------------------------------------------------------------------------------
# rt_film_upsample against the restatement

class _Lift:
    """Device buffers of one lift: inputs with `pad` elements behind every plane (1e300 behind the mean's, NaN behind the guides'),
    outputs filled with sentinels, one more element behind the last plane of each."""

    def __init__(self, r, s, lg, hg, pad):
        self.r, self.w, self.h = r, hg.shape[1], hg.shape[2]
        self.wl, self.hl, self.npx = s.shape[1], s.shape[2], self.w * self.h
        self.slo, self.shi = self.wl * self.hl + pad, self.npx + pad
        self.d = [r.malloc(8 * s.shape[0] * self.slo), r.malloc(32 * self.slo), r.malloc(32 * self.shi), r.malloc(24 * self.shi + 8),
                  r.malloc(4 * self.npx + 8)]
        self.d_lo, self.d_lg, self.d_hg, self.d_out, self.d_kind = self.d
        r.h2d(self.d_lo, _padded(s, self.slo, 1e300, np.float64))
        r.h2d(self.d_lg, _padded(lg, self.slo, np.nan, np.float32))
        r.h2d(self.d_hg, _padded(hg, self.shi, np.nan, np.float32))

    def close(self):
        for d in self.d:
            self.r.free(d)

    def run(self, n, lo_grid, hi_grid, cos, dem, with_kind, **kw):
        r = self.r
        r.h2d(self.d_out, np.full(3 * self.shi + 1, SENTINEL))
        r.h2d(self.d_kind, np.full(self.npx + 2, KIND_SENTINEL, np.float32))
        r.film_upsample(self.d_lo, self.wl, self.hl, n, self.d_lg, self.d_hg, self.w, self.h, lo_grid, hi_grid, self.d_out,
                        self.d_kind if with_kind else None, normal_cos=cos, demodulate=dem, lo_stride=self.slo, lo_guide_stride=self.slo,
                        hi_guide_stride=self.shi, out_stride=self.shi, **kw)
        r.sync()
        return self.outputs(with_kind)

    def outputs(self, with_kind):
        out = _read(self.r, self.d_out, (3 * self.shi + 1,))
        kind = _read(self.r, self.d_kind, (self.npx + 2,), np.float32)
        planes = out[:3 * self.shi].reshape(3, self.shi)
        assert (planes[:, self.npx:] == SENTINEL).all() and out[-1] == SENTINEL, "a pad of the output was written"
        assert (kind[self.npx:] == KIND_SENTINEL).all() and (with_kind or (kind == KIND_SENTINEL).all()), "the kind plane's sentinels"
        return planes[:, :self.npx].reshape(3, self.w, self.h), kind[:self.npx].reshape(self.w, self.h)

    def untouched(self):
        out = _read(self.r, self.d_out, (3 * self.shi + 1,))
        kind = _read(self.r, self.d_kind, (self.npx + 2,), np.float32)
        return (out == SENTINEL).all() and (kind == KIND_SENTINEL).all()


@pytest.mark.parametrize("p", uc.PAIRS, ids=[f"{p[0]}-{p[1][0]}x{p[1][1]}-{p[2][0]}x{p[2][1]}" for p in uc.PAIRS])
def test_upsample_equals_the_reference(rend, p):
    f = uc.pair(p)
    pads = iter((1, 3, 0, 1))
    for n in uc.PASSES:
        for dem in (0, 1):
            want, want_kind, s = uc.want(p, n, dem)
            lift = _Lift(rend, s, f["lo_guides"], f["hi_guides"], next(pads))
            try:
                for with_kind in (True, False):
                    out, kind = lift.run(n, f["lo_grid"], f["hi_grid"], 0.9, dem, with_kind)
                    assert same_bits(out, want), (p, n, dem, with_kind, int((out != want).sum()))
                    assert not with_kind or same_bits(kind, want_kind), (p, n, dem, uc.kinds(kind), uc.kinds(want_kind))
            finally:
                lift.close()
    assert uc.kinds(uc.want(p, 1, 0)[1]) == uc.COUNTS[p]


def test_a_four_plane_mean_another_cosine_and_the_identity(rend):
    p = uc.PAIRS[0]
    f = uc.pair(p)
    want, want_kind, s = uc.want(p, 1, 1, 0.5, planes=4)
    lift = _Lift(rend, s, f["lo_guides"], f["hi_guides"], 3)
    try:
        out, kind = lift.run(1, f["lo_grid"], f["hi_grid"], 0.5, 1, True)
        assert same_bits(out, want) and same_bits(kind, want_kind) and uc.kinds(kind) == uc.COUNTS_COS_HALF
    finally:
        lift.close()
    for q in (uc.PAIRS[4], uc.TEXTURED):                           # equal grids, no demodulation: lo / n bit for bit, every kind 0
        f = uc.pair(q)
        for n in uc.PASSES:
            s = uc.sums(f["wl"], f["hl"], n, 9)
            lift = _Lift(rend, s, f["lo_guides"], f["lo_guides"], 1)
            try:
                out, kind = lift.run(n, f["lo_grid"], f["lo_grid"], 0.999, 0, True)
                assert same_bits(out, s / np.float64(n)) and not kind.any(), (q, n)
            finally:
                lift.close()


def test_the_lift_loops_past_the_grid_cap(rend):
    """The smallest output frame of height 523 with more pixels than the grid's cap has threads (8 blocks of 256 per CU): the
    grid-stride loop takes a second turn.  The low frame has a few columns; the guides come from no scene."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == rend.kernel_info()["cu_count"]
    h = 523
    w = (8 * 256 * cus) // h + 1
    assert w * h > 8 * 256 * cus >= (w - 1) * h
    wl, hl = 5, 131
    lg, hg, lo_grid, hi_grid = uc.synthetic(wl, hl, w, h, 3)
    s = uc.sums(wl, hl, 2, 41)
    want, want_kind = U.upsample_reference(s, 2, lg, hg, lo_grid, hi_grid, 0.9, 1)
    assert all(uc.kinds(want_kind)), uc.kinds(want_kind)
    lift = _Lift(rend, s, lg, hg, 1)
    try:
        out, kind = lift.run(2, lo_grid, hi_grid, 0.9, 1, True)
        assert same_bits(kind, want_kind), (uc.kinds(kind), uc.kinds(want_kind))
        assert same_bits(out, want), int((out != want).sum())
    finally:
        lift.close()


# ---------------------------------------------------------------------------------------------------------------------
# Refusals

def test_refusals_carry_their_text_and_leave_the_outputs_untouched(rend):
    import python_ray_tracer_amd as pkg
    p = uc.SMALLEST
    f = uc.pair(p)
    s = uc.sums(f["wl"], f["hl"], 1, 1)
    wl, hl, w, h = f["wl"], f["hl"], f["w"], f["h"]
    nlo, npx = wl * hl, w * h
    lo_grid, hi_grid = f["lo_grid"], f["hi_grid"]
    nan, inf = float("nan"), float("inf")
    lift = _Lift(rend, s, f["lo_guides"], f["hi_guides"], 0)
    try:
        rend.h2d(lift.d_out, np.full(3 * npx + 1, SENTINEL))
        rend.h2d(lift.d_kind, np.full(npx + 2, KIND_SENTINEL, np.float32))
        A = dict(d_lo=lift.d_lo, wl=wl, hl=hl, n=1, d_lg=lift.d_lg, d_hg=lift.d_hg, w=w, h=h, lo_grid=lo_grid, hi_grid=hi_grid, d_out=lift.d_out,
                 d_kind=lift.d_kind)

        def up(**kw):
            a = {**A, **{k: v for k, v in kw.items() if k in A}}
            rest = {k: v for k, v in kw.items() if k not in A}
            rend.film_upsample(a["d_lo"], a["wl"], a["hl"], a["n"], a["d_lg"], a["d_hg"], a["w"], a["h"], a["lo_grid"], a["hi_grid"], a["d_out"],
                               a["d_kind"], **rest)

        def grid(g, i, v):
            g = list(g)
            g[i] = v
            return tuple(g)
        null, lo_area, hi_area = "a buffer or up is NULL", "wl*hl outside 1..RT_FILM_MAX_PIXELS", "w*h outside 1..RT_FILM_MAX_PIXELS"
        stride, grids, own = "a plane stride is smaller than its frame", "a grid entry is not finite, or a px, dy or dz is 0", \
            "d_out and d_out_kind must be buffers of their own"
        bad = [(null, dict(d_lo=None)), (null, dict(d_lg=None)), (null, dict(d_hg=None)), (null, dict(d_out=None)),
               (lo_area, dict(wl=0)), (lo_area, dict(hl=-1)), (lo_area, dict(wl=1 << 14, hl=(1 << 13) + 1)),
               (hi_area, dict(w=0)), (hi_area, dict(h=-2)), (hi_area, dict(w=1 << 14, h=(1 << 13) + 1)),
               ("n < 1", dict(n=0)), ("n < 1", dict(n=-4)),
               (stride, dict(lo_stride=nlo - 1)), (stride, dict(lo_guide_stride=nlo - 1)), (stride, dict(hi_guide_stride=npx - 1)),
               (stride, dict(out_stride=npx - 1)),
               (grids, dict(lo_grid=grid(lo_grid, 1, nan))), (grids, dict(hi_grid=grid(hi_grid, 3, inf))), (grids, dict(lo_grid=grid(lo_grid, 0, 0.0))),
               (grids, dict(lo_grid=grid(lo_grid, 2, 0.0))), (grids, dict(hi_grid=grid(hi_grid, 4, 0.0))), (grids, dict(hi_grid=grid(hi_grid, 0, -inf))),
               ("normal_cos outside [-1, 1]", dict(normal_cos=1.5)), ("normal_cos outside [-1, 1]", dict(normal_cos=nan)),
               ("normal_cos outside [-1, 1]", dict(normal_cos=-1.01)),
               ("demodulate must be 0 or 1", dict(demodulate=2)), ("demodulate must be 0 or 1", dict(demodulate=-1)),
               ("reserved must be 0", dict(reserved=1)),
               (own, dict(d_out=lift.d_lo)), (own, dict(d_out=lift.d_hg)), (own, dict(d_kind=lift.d_lg)), (own, dict(d_kind=lift.d_out)),
               # the order: the first broken rule speaks
               (null, dict(d_lo=None, wl=0, n=0)),
               (lo_area, dict(wl=0, w=0, n=0)),
               (hi_area, dict(w=0, n=0, lo_stride=1)),
               ("n < 1", dict(n=0, lo_stride=1, normal_cos=2.0)),
               (stride, dict(out_stride=1, lo_grid=grid(lo_grid, 2, 0.0))),
               (grids, dict(hi_grid=grid(hi_grid, 2, nan), normal_cos=2.0)),
               ("normal_cos outside [-1, 1]", dict(normal_cos=2.0, demodulate=3)),
               ("demodulate must be 0 or 1", dict(demodulate=3, reserved=2)),
               ("reserved must be 0", dict(reserved=2, d_kind=lift.d_out))]
        for text, kw in bad:
            with pytest.raises(pkg.RenderError) as e:
                up(**kw)
            assert e.value.status == L.RT_ERR_BAD_ARG and str(e.value).endswith("rt_film_upsample: " + text), (text, kw, str(e.value))
        lib = L.load()                                            # up == NULL: below the wrapper, which always passes one
        rc = lib.rt_film_upsample(rend._ctx, lift.d_lo, nlo, wl, hl, 1, lift.d_lg, nlo, lift.d_hg, npx, w, h, None, lift.d_out, npx, None, None)
        assert rc == L.RT_ERR_BAD_ARG and lib.rt_last_error(rend._ctx).decode() == "rt_film_upsample: " + null
        # rt_render_guides_grid, on the session's renderer (it has a scene and a camera)
        _set_scene(rend, p[0])
        d_g = lift.d_hg
        rend.h2d(d_g, np.full(8 * npx, SENTINEL, np.float32))
        frame = "frame size out of range (1 <= w <= 2^31 - 8, 1 <= h <= 2^29 - 32, w*h <= 2^31)"
        cols = "column range must satisfy 0 <= x0 < x1 <= w"
        gg = lambda w_=w, h_=h, x0=0, x1=w, d=d_g, stride=None: rend._check(rend._lib.rt_render_guides_grid(
            rend._ctx, w_, h_, *hi_grid, x0, x1, d, (x1 - x0) * h_ if stride is None else stride, None))
        bad = [("d_guides is NULL", lambda: gg(d=None)), (frame, lambda: gg(w_=0)), (frame, lambda: gg(h_=0)),
               (frame, lambda: gg(w_=1 << 16, h_=(1 << 15) + 1, x1=1)), (frame, lambda: gg(h_=1 << 29, w_=1, x1=1)),
               (cols, lambda: gg(x0=-1)), (cols, lambda: gg(x1=w + 1)), (cols, lambda: gg(x0=5, x1=5)),
               ("plane_stride smaller than the slab", lambda: gg(stride=npx - 1)),
               ("d_guides is NULL", lambda: gg(d=None, w_=0, x0=-1)), (frame, lambda: gg(w_=0, x0=-1, stride=0)),
               (cols, lambda: gg(x0=-1, stride=0))]
        for text, fn in bad:
            with pytest.raises(pkg.RenderError) as e:
                fn()
            assert e.value.status == L.RT_ERR_BAD_ARG and str(e.value).endswith("rt_render_guides_grid: " + text), (text, str(e.value))
        with pytest.raises(ValueError, match="out of range"):      # the wrapper's own check of the frame
            rend.render_guides_grid(0, h, hi_grid, 0, 1, d_g)
        rend.sync()
        assert lift.untouched(), "a refused call touched an output"
        assert (_read(rend, d_g, (8 * npx,), np.float32) == SENTINEL).all(), "a refused call touched the guides"
        up(normal_cos=-1.0, demodulate=0)                          # the edges are accepted
        up(normal_cos=1.0, d_kind=None)
        rend.sync()
    finally:
        lift.close()


# ---------------------------------------------------------------------------------------------------------------------
# Through Film and Upsampler on a rendered scene

def test_film_and_upsampler_on_the_soft_scene(rend):
    g = vc.fixture()
    wl, hl, w, h = 32, 32, 64, 64
    rend.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]),
                   light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]))
    rend.set_camera(g["cam_origin"], g["cam_rot"])
    rend.set_lens(0.0, 1.0)
    lo_grid = raygen_closed_form(wl, hl, float(g["fov"]))
    rend.set_raygen(wl, hl, *lo_grid)
    params = rend.params(**IGNORED, depth=int(g["depth"]), aa=0, seed=int(g["seed"]))
    tone = dict(white=400.0, gamma=2)
    with Film(rend, moments=True) as film, Upsampler(film, w, h) as up:
        assert up.hi_grid == U.hi_raygen(lo_grid, wl, hl, w, h)
        film.accumulate(params, 4)
        film.denoise(variance=True)
        up.upsample(denoised=True, kinds=True)
        u8, f32 = up.resolve(f32=True, denoised=True, **tone)
        assert (rend.w, rend.h, rend.raygen) == (wl, hl, tuple(float(v) for v in lo_grid))
        s, q = _read(rend, film.d_sum, (3, wl, hl)), _read(rend, film.d_sq, (3, wl, hl))
        lg, hg = _read(rend, film.d_guides, (8, wl, hl), np.float32), _read(rend, up.d_guides, (8, w, h), np.float32)
        assert same_bits(lg, D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], wl, hl, raygen=lo_grid))
        assert same_bits(hg, D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h, raygen=up.hi_grid))
        den = V.denoise_variance_reference(s, q, 4, lg, 4, 32, V.KAPPA, 0.0, 1, 1)
        lifted, kind = U.upsample_reference(den, 1, lg, hg, up.lo_grid, up.hi_grid, U.NORMAL_COS, 1)
        assert same_bits(_read(rend, up.buffer, (3, w, h)), lifted) and same_bits(up.kinds(), kind)
        print(f"soft_default_64_d4 32x32 -> 64x64: kinds {uc.kinds(kind)}")
        v = F.tone_reference(lifted, 1, 1.0, 400.0, 2)
        assert u8.shape == (3, w, h) and same_bits(f32, v.astype(np.float32)) and np.array_equal(u8, F.clip_reference(v)[[0, 2, 1]])
        # the plain passes, without demodulation
        up.upsample(demodulate=False)
        plain, _ = U.upsample_reference(s, 4, lg, hg, up.lo_grid, up.hi_grid, U.NORMAL_COS, 0)
        assert same_bits(up.resolve(u8=False, f32=True)[1], plain.astype(np.float32))
        with pytest.raises(ValueError, match="call upsample\\(\\)"):
            up.resolve(denoised=True, **tone)
        # the film's meter at low resolution drives the full-resolution resolve
        film.meter()
        st = M.solve_reference(M.histogram_reference(s, 4), np.zeros(4))
        got = up.resolve(u8=False, f32=True, auto_exposure=True, **tone)[1]
        assert same_bits(got, F.tone_reference(plain, 1, exposure=st[0], **tone).astype(np.float32)) and st[0] != 1.0
        # one more pass: the lift is stale
        params.seed += 4
        film.accumulate(params, 1)
        with pytest.raises(ValueError):
            up.resolve(**tone)
        up.upsample()
        up.resolve(**tone)
