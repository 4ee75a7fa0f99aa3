"""What the launching entry points of the C ABI refuse, and with which code and rt_last_error text: rt_render, rt_render_device,
rt_render_sequence (one frame and two), rt_render_begin, rt_film_accumulate and rt_render_guides, each with every bad argument its
checks name, and with two at once where the order of the checks decides which one the caller sees.  A refused call leaves the
context as it was: the 16 x 8 frame rendered after it is the frame rendered before.  The texts are literals here, so a change of
the library that rewords, reorders or drops a check fails this test."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 16, 8
BAD_ARG, STATE = -1, -4
COLUMNS = "column range must satisfy 0 <= x0 < x1 <= w"
BOTH_NULL = "both output pointers are NULL"
HWC_DEVICE = "RT_FLAG_U8_HWC re-uses plane_stride as the image row pitch: render the float32 buffer in a separate call"
HWC_HOST = "RT_FLAG_U8_HWC: request the uint8 image and the float32 buffer in separate calls"
NO_SCENE, NO_CAMERA = "rt_set_scene has not been called", "rt_set_camera has not been called"
NO_GRID = "rt_set_raygen / rt_set_pixel_loc has not been called"

SPHERES = np.array([[4.0], [0.0], [0.0], [1.0], [255.0], [64.0], [32.0]], np.float32)
LIGHTS = np.array([[0.0], [3.0], [4.0]], np.float32)
PLANES = np.zeros((9, 0), np.float32)
CAM_O, CAM_R = np.zeros(3), np.eye(3)
RAYGEN = (1.0, 2.0, -4.0 / (W - 1), 1.0, -2.0 / (H - 1))


def _entries(r, L, bufs):
    """name -> a call of the entry with the test's good arguments, each replaceable by keyword."""
    lib, ctx = r._lib, r._ctx
    host8, host32 = np.empty((3, W, H), np.uint8), np.empty((3, W, H), np.float32)
    vp = lambda a: C.c_void_p(a) if a else None          # noqa: E731
    hp = lambda a: a.ctypes.data if a is not None else None   # noqa: E731

    def params(depth=2, aa=L.RT_AA_NONE, flags=0, spp=4):
        return r.params(0.1, 0.7, 0.5, depth, aa, flags, spp=spp)

    def pref(p):
        return C.byref(p) if p is not None else None

    def render(p=params(), x0=0, x1=W, u8=host8, f32=host32):
        return lib.rt_render(ctx, pref(p), x0, x1, hp(u8), hp(f32))

    def begin(p=params(), x0=0, x1=W, u8=host8, f32=host32, slot=1):
        st = lib.rt_render_begin(ctx, pref(p), x0, x1, hp(u8), hp(f32), slot)
        if st == L.RT_OK:
            assert lib.rt_render_end(ctx, slot) == L.RT_OK
        return st

    def device(p=params(), x0=0, x1=W, u8=bufs["u8"], f32=bufs["f32"], stride=W * H):
        return lib.rt_render_device(ctx, pref(p), x0, x1, vp(u8), vp(f32), stride, None)

    def sequence(n, p=params(), x0=0, x1=W, u8=bufs["u8"], f32=bufs["f32"], stride=W * H, frame_stride=3 * W * H, n_streams=0):
        return lib.rt_render_sequence(ctx, pref(p), x0, x1, n, vp(u8), vp(f32), stride, frame_stride, None, None, n_streams, 0)

    def film(p=params(), x0=0, x1=W, passes=1, d_sum=bufs["sum"], stride=W * H):
        return lib.rt_film_accumulate(ctx, pref(p), x0, x1, passes, 1, vp(d_sum), stride, None)

    def guides(x0=0, x1=W, d_guides=bufs["guides"], stride=W * H):
        return lib.rt_render_guides(ctx, x0, x1, vp(d_guides), stride, None)

    return params, dict(render=render, begin=begin, device=device, sequence=sequence, film=film, guides=guides)


def _refusals(L, params, e):
    """(name, call, code, text) of every refusal on a context whose scene, camera and grid are set."""
    hwc = params(flags=L.RT_FLAG_U8_HWC)
    out = []
    # what every entry with rt_params shares (check_params), through each of them
    launching = [("rt_render", e["render"]), ("rt_render_device", e["device"]), ("rt_render_sequence[1]", lambda **k: e["sequence"](1, **k)),
                 ("rt_render_sequence[2]", lambda **k: e["sequence"](2, **k)), ("rt_render_begin", e["begin"]), ("rt_film_accumulate", e["film"])]
    for name, call in launching:
        out += [
            (f"{name}: params NULL", lambda c=call: c(p=None), BAD_ARG, "params is NULL"),
            (f"{name}: depth -1", lambda c=call: c(p=params(depth=-1)), BAD_ARG, "depth outside 0..RT_MAX_DEPTH"),
            (f"{name}: depth 17", lambda c=call: c(p=params(depth=L.RT_MAX_DEPTH + 1)), BAD_ARG, "depth outside 0..RT_MAX_DEPTH"),
            (f"{name}: aa_mode 3", lambda c=call: c(p=params(aa=3)), BAD_ARG, "unknown aa_mode"),
            (f"{name}: spp 0", lambda c=call: c(p=params(aa=L.RT_AA_STOCHASTIC, spp=0)), BAD_ARG, "spp outside 1..RT_MAX_SPP"),
            (f"{name}: spp 65", lambda c=call: c(p=params(aa=L.RT_AA_STOCHASTIC, spp=L.RT_MAX_SPP + 1)), BAD_ARG, "spp outside 1..RT_MAX_SPP"),
            (f"{name}: x0 -1", lambda c=call: c(x0=-1), BAD_ARG, COLUMNS),
            (f"{name}: x1 w+1", lambda c=call: c(x1=W + 1), BAD_ARG, COLUMNS),
            (f"{name}: x0 == x1", lambda c=call: c(x0=8, x1=8), BAD_ARG, COLUMNS),
            # two at once: the depth is looked at before the column range
            (f"{name}: depth 17 and x1 w+1", lambda c=call: c(p=params(depth=17), x1=W + 1), BAD_ARG, "depth outside 0..RT_MAX_DEPTH"),
        ]
    # the outputs
    for name, call in launching[:5]:
        out.append((f"{name}: both outputs NULL", lambda c=call: c(u8=None, f32=None), BAD_ARG, BOTH_NULL))
        # two at once: a bad column range with both outputs NULL
        out.append((f"{name}: x1 w+1 and both outputs NULL", lambda c=call: c(x1=W + 1, u8=None, f32=None), BAD_ARG, COLUMNS))
    for name, call in launching[1:4]:
        out += [
            (f"{name}: HWC with float32", lambda c=call: c(p=hwc, stride=W), BAD_ARG, HWC_DEVICE),
            # two at once: HWC with a float32 pointer and a short pitch
            (f"{name}: HWC with float32 and a short pitch", lambda c=call: c(p=hwc, stride=W - 1), BAD_ARG, HWC_DEVICE),
            (f"{name}: HWC short pitch", lambda c=call: c(p=hwc, f32=None, stride=W - 1), BAD_ARG, "row pitch smaller than the slab width"),
            (f"{name}: short plane_stride", lambda c=call: c(stride=W * H - 1), BAD_ARG, "plane_stride smaller than the slab"),
            (f"{name}: short plane_stride of a slab", lambda c=call: c(x0=8, stride=8 * H - 1), BAD_ARG, "plane_stride smaller than the slab"),
        ]
    for name, call in (launching[0], launching[4]):
        out.append((f"{name}: HWC with float32", lambda c=call: c(p=hwc), BAD_ARG, HWC_HOST))
    seq = e["sequence"]
    out += [
        ("rt_render_sequence: n -1", lambda: seq(-1), BAD_ARG, "rt_render_sequence: negative frame count"),
        ("rt_render_sequence[2]: short frame_stride", lambda: seq(2, frame_stride=3 * W * H - 1), BAD_ARG, "frame_stride smaller than three planes"),
        ("rt_render_sequence[2]: HWC short frame_stride", lambda: seq(2, p=hwc, f32=None, stride=W, frame_stride=3 * W * H - 1), BAD_ARG,
         "frame_stride smaller than one image"),
        ("rt_render_sequence[1]: n_streams -1", lambda: seq(1, n_streams=-1), BAD_ARG, "rt_render_sequence: n_streams without a stream array"),
        ("rt_render_sequence[2]: n_streams 2, no array", lambda: seq(2, n_streams=2), BAD_ARG, "rt_render_sequence: n_streams without a stream array"),
        ("rt_render_begin: slot -1", lambda: e["begin"](slot=-1), BAD_ARG, "rt_render_begin: slot outside 0..RT_RENDER_SLOTS-1"),
        ("rt_render_begin: slot 4", lambda: e["begin"](slot=L.RT_RENDER_SLOTS), BAD_ARG, "rt_render_begin: slot outside 0..RT_RENDER_SLOTS-1"),
        # two at once: the slot is looked at before the outputs
        ("rt_render_begin: slot 4 and both outputs NULL", lambda: e["begin"](slot=4, u8=None, f32=None), BAD_ARG,
         "rt_render_begin: slot outside 0..RT_RENDER_SLOTS-1"),
        ("rt_film_accumulate: passes 0", lambda: e["film"](passes=0), BAD_ARG, "rt_film_accumulate: passes < 1"),
        ("rt_film_accumulate: d_sum NULL", lambda: e["film"](d_sum=None), BAD_ARG, "rt_film_accumulate: d_sum is NULL"),
        ("rt_film_accumulate: short sum_stride", lambda: e["film"](stride=W * H - 1), BAD_ARG, "rt_film_accumulate: sum_stride smaller than the slab"),
        ("rt_film_accumulate: passes 0 and d_sum NULL", lambda: e["film"](passes=0, d_sum=None), BAD_ARG, "rt_film_accumulate: passes < 1"),
        ("rt_render_guides: d_guides NULL", lambda: e["guides"](d_guides=None), BAD_ARG, "rt_render_guides: d_guides is NULL"),
        ("rt_render_guides: x0 -1", lambda: e["guides"](x0=-1), BAD_ARG, COLUMNS),
        ("rt_render_guides: x1 w+1", lambda: e["guides"](x1=W + 1), BAD_ARG, COLUMNS),
        ("rt_render_guides: x0 == x1", lambda: e["guides"](x0=8, x1=8), BAD_ARG, COLUMNS),
        ("rt_render_guides: short plane_stride", lambda: e["guides"](stride=W * H - 1), BAD_ARG, "rt_render_guides: plane_stride smaller than the slab"),
        ("rt_render_guides: x1 w+1 and a short plane_stride", lambda: e["guides"](x1=W + 1, stride=1), BAD_ARG, COLUMNS),
    ]
    return out


def _open(pkg, L):
    r = pkg.Renderer(0)
    bufs = {"u8": r.malloc(2 * 3 * W * H), "f32": r.malloc(2 * 3 * W * H * 4), "sum": r.malloc(3 * W * H * 8),
            "guides": r.malloc(L.RT_GUIDE_PLANES * W * H * 4)}
    return r, bufs


def _last_error(r):
    return r._lib.rt_last_error(r._ctx).decode()


def test_refusals_and_their_texts():
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    r, bufs = _open(pkg, L)
    try:
        r.set_scene(SPHERES, LIGHTS, PLANES)
        r.set_camera(CAM_O, CAM_R)
        r.set_raygen(W, H, *RAYGEN)
        params, e = _entries(r, L, bufs)

        def frame():
            return r.render(0.1, 0.7, 0.5, 2, u8=True, f32=True)
        u8, f32 = frame()
        assert u8.any()
        # every entry accepts the good arguments
        for name in ("render", "begin", "device", "film", "guides"):
            assert e[name]() == L.RT_OK, (name, _last_error(r))
        assert e["sequence"](1) == L.RT_OK and e["sequence"](2) == L.RT_OK, _last_error(r)
        r.sync()
        cases = _refusals(L, params, e)
        wrong = []
        for name, call, code, text in cases:
            st = call()
            if (st, _last_error(r)) != (code, text):
                wrong.append((name, st, _last_error(r), code, text))
            a, b = frame()
            if not (np.array_equal(a, u8) and np.array_equal(b.view(np.uint32), f32.view(np.uint32))):
                wrong.append((name, "the frame after the refused call differs"))
        assert not wrong, wrong[:6]
        assert len(cases) > 100
        # a lens on a scene without a material table (RT_ERR_STATE from every launching entry, guides aside: they ignore the lens)
        r.set_lens(0.25, 4.0)
        lens = "a lens with aperture > 0 needs a scene with a material table (M >= 1)"
        for name in ("render", "begin", "device", "film"):
            assert (e[name](), _last_error(r)) == (STATE, lens), name
        assert (e["sequence"](2), _last_error(r)) == (STATE, lens)
        assert (e["device"](u8=None, f32=None), _last_error(r)) == (STATE, lens)      # (before the outputs are looked at)
        assert e["guides"]() == L.RT_OK
        r.set_lens(0.0, 4.0)
        a, b = frame()
        assert np.array_equal(a, u8) and np.array_equal(b.view(np.uint32), f32.view(np.uint32))
    finally:
        for b in bufs.values():
            r.free(b)
        r.close()


def test_refusals_of_an_unfinished_context():
    """The state checks, in the order scene, camera, grid; a NULL d_guides is reported before the missing scene; RT_AA_STOCHASTIC on
    an explicit grid; RT_FLAG_COUNT_RAYS on a scene with a material table."""
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    r, bufs = _open(pkg, L)
    try:
        params, e = _entries(r, L, bufs)
        calls = [("render", e["render"]), ("device", e["device"]), ("sequence[1]", lambda **k: e["sequence"](1, **k)),
                 ("sequence[2]", lambda **k: e["sequence"](2, **k)), ("begin", e["begin"]), ("film", e["film"]), ("guides", e["guides"])]

        def all_say(code, text, **kw):
            for name, call in calls:
                k = {a: v for a, v in kw.items() if not (name == "guides" and a == "p")}
                assert (call(**k), _last_error(r)) == (code, text), name
        all_say(STATE, NO_SCENE)
        assert (e["guides"](d_guides=None), _last_error(r)) == (BAD_ARG, "rt_render_guides: d_guides is NULL")
        assert (e["render"](p=None), _last_error(r)) == (BAD_ARG, "params is NULL")
        all_say(STATE, NO_SCENE, x1=W + 1)
        all_say(STATE, NO_SCENE, p=params(depth=17))
        r.set_scene(SPHERES, LIGHTS, PLANES)
        all_say(STATE, NO_CAMERA)
        r.set_camera(CAM_O, CAM_R)
        all_say(STATE, NO_GRID)
        y, z = np.meshgrid(RAYGEN[1] + RAYGEN[2] * np.arange(W), RAYGEN[3] + RAYGEN[4] * np.arange(H), indexing="ij")
        r.set_pixel_loc(np.stack([np.full((W, H), RAYGEN[0]), y, z]))
        stoch = params(aa=L.RT_AA_STOCHASTIC)
        for name, call in calls[:6]:
            assert (call(p=stoch), _last_error(r)) == (STATE, "RT_AA_STOCHASTIC needs the closed-form ray grid (rt_set_raygen)"), name
            assert (call(p=stoch, x1=W + 1), _last_error(r)) == (STATE, "RT_AA_STOCHASTIC needs the closed-form ray grid (rt_set_raygen)"), name
            assert (call(p=params(aa=L.RT_AA_STOCHASTIC, spp=0)), _last_error(r)) == (BAD_ARG, "spp outside 1..RT_MAX_SPP"), name
        assert e["guides"]() == L.RT_OK and e["render"]() == L.RT_OK, _last_error(r)
        r.set_scene(SPHERES, LIGHTS, PLANES, materials=(np.array([[0.1, 0.7, 0.5]]), np.zeros(1, np.int32), np.zeros(0, np.int32)))
        count = params(flags=L.RT_FLAG_COUNT_RAYS)
        for name, call in calls[:6]:
            assert (call(p=count), _last_error(r)) == (BAD_ARG, "RT_FLAG_COUNT_RAYS is not available for a scene with materials"), name
            assert (call(p=count, x1=W + 1), _last_error(r)) == (BAD_ARG, COLUMNS), name
        assert e["render"]() == L.RT_OK, _last_error(r)
    finally:
        for b in bufs.values():
            r.free(b)
        r.close()


# ---- the film entries: rt_film_accumulate_moments, rt_film_resolve, rt_film_denoise, rt_film_denoise_variance, rt_film_temporal,
# rt_film_temporal_moments, rt_film_denoise_variance_temporal ----
NPX = W * H
FILM_INPUTS = ("sum", "sq", "guides", "hist", "hist_sq", "hist_len", "hist_guides")
FILM_OUTPUTS = ("out", "work", "out_sq", "out_len", "o8", "o32", "acc_sum", "acc_sq")
SENTINEL = 0xA5
BIG_SIDE = 1 << 14                     # BIG_SIDE^2 = 2^28 pixels: above RT_FILM_MAX_PIXELS, inside rt_set_raygen's limits
HWC_RESOLVE = "RT_FLAG_U8_HWC re-uses out_stride as the image row pitch: resolve the float32 buffer in a separate call"
NAN, INF = float("nan"), float("inf")


def _film_open(pkg, L):
    r = pkg.Renderer(0)
    # every buffer four float64 planes large: the largest any entry writes (rt_film_denoise_variance's d_out) or reads (the guides)
    bufs = {n: r.malloc(4 * NPX * 8) for n in FILM_INPUTS + FILM_OUTPUTS}
    for n in FILM_INPUTS:
        r.h2d(bufs[n], np.zeros(4 * NPX * 8, np.uint8))
    return r, bufs


def _fill_outputs(r, bufs):
    for n in FILM_OUTPUTS:
        r.h2d(bufs[n], np.full(4 * NPX * 8, SENTINEL, np.uint8))


def _outputs_untouched(r, bufs):
    got = np.empty(4 * NPX * 8, np.uint8)
    for n in FILM_OUTPUTS:
        r.d2h(got, bufs[n])
        if not (got == SENTINEL).all():
            return n
    return None


def _film_entries(r, L, b):
    """name -> a call of the entry with the test's good arguments, each replaceable by keyword (a buffer by its address or None)."""
    lib, ctx = r._lib, r._ctx
    vp = lambda a: C.c_void_p(a) if a else None          # noqa: E731
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    good = r.params(0.1, 0.7, 0.5, 2)

    def tone(exposure=1.0, white=0.0, gamma=1, flags=0):
        return L.rt_film_tone(exposure, white, gamma, flags)

    def dn(levels=2, normal_shin=32, sigma=0.0, demodulate=1, reserved=0):
        return L.rt_denoise(levels, normal_shin, sigma, demodulate, reserved)

    def dv(levels=2, normal_shin=32, kappa=1.0, var_floor=0.0, demodulate=1, prefilter=1):
        return L.rt_denoise_variance(levels, normal_shin, kappa, var_floor, demodulate, prefilter)

    def tp(prev_origin=(0.25, 0.0, 0.0), prev_rotation=tuple(np.eye(3).ravel()), depth_tol=0.01, normal_cos=0.9, max_history=32.0, reserved=(0, 0)):
        t = L.rt_temporal()
        t.prev_origin[:] = prev_origin
        t.prev_rotation[:] = prev_rotation
        t.depth_tol, t.normal_cos, t.max_history = depth_tol, normal_cos, max_history
        t.reserved[:] = reserved
        return t

    def moments(p=good, x0=0, x1=W, passes=1, d_sum=b["acc_sum"], sum_stride=NPX, d_sq=b["acc_sq"], sq_stride=NPX):
        return lib.rt_film_accumulate_moments(ctx, ref(p), x0, x1, passes, 1, vp(d_sum), sum_stride, vp(d_sq), sq_stride, None)

    def resolve(d_sum=b["sum"], sum_stride=NPX, ws=W, h=H, n=4, t=tone(), d_u8=b["o8"], d_f32=b["o32"], out_stride=NPX):
        return lib.rt_film_resolve(ctx, vp(d_sum), sum_stride, ws, h, n, ref(t), vp(d_u8), vp(d_f32), out_stride, None)

    def denoise(d_sum=b["sum"], sum_stride=NPX, ws=W, h=H, n=4, d_guides=b["guides"], guide_stride=NPX, s=dn(), d_out=b["out"], out_stride=NPX,
                d_work=b["work"], work_stride=NPX):
        return lib.rt_film_denoise(ctx, vp(d_sum), sum_stride, ws, h, n, vp(d_guides), guide_stride, ref(s), vp(d_out), out_stride, vp(d_work),
                                   work_stride, None)

    def variance(d_sum=b["sum"], sum_stride=NPX, d_sq=b["sq"], sq_stride=NPX, ws=W, h=H, n=4, d_guides=b["guides"], guide_stride=NPX, s=dv(),
                 d_out=b["out"], out_stride=NPX, d_work=b["work"], work_stride=NPX):
        return lib.rt_film_denoise_variance(ctx, vp(d_sum), sum_stride, vp(d_sq), sq_stride, ws, h, n, vp(d_guides), guide_stride, ref(s),
                                            vp(d_out), out_stride, vp(d_work), work_stride, None)

    def temporal(d_sum=b["sum"], sum_stride=NPX, n=4, d_guides=b["guides"], guide_stride=NPX, d_hist=b["hist"], hist_stride=NPX,
                 d_hist_len=b["hist_len"], d_hist_guides=b["hist_guides"], hist_guide_stride=NPX, t=tp(), d_out=b["out"], out_stride=NPX,
                 d_out_len=b["out_len"]):
        return lib.rt_film_temporal(ctx, vp(d_sum), sum_stride, n, vp(d_guides), guide_stride, vp(d_hist), hist_stride, vp(d_hist_len),
                                    vp(d_hist_guides), hist_guide_stride, ref(t), vp(d_out), out_stride, vp(d_out_len), None)

    def temporal_moments(d_sum=b["sum"], sum_stride=NPX, d_sq=b["sq"], sq_stride=NPX, n=4, d_guides=b["guides"], guide_stride=NPX,
                         d_hist=b["hist"], hist_stride=NPX, d_hist_sq=b["hist_sq"], hist_sq_stride=NPX, d_hist_len=b["hist_len"],
                         d_hist_guides=b["hist_guides"], hist_guide_stride=NPX, t=tp(), d_out=b["out"], out_stride=NPX, d_out_sq=b["out_sq"],
                         out_sq_stride=NPX, d_out_len=b["out_len"]):
        return lib.rt_film_temporal_moments(ctx, vp(d_sum), sum_stride, vp(d_sq), sq_stride, n, vp(d_guides), guide_stride, vp(d_hist),
                                            hist_stride, vp(d_hist_sq), hist_sq_stride, vp(d_hist_len), vp(d_hist_guides), hist_guide_stride,
                                            ref(t), vp(d_out), out_stride, vp(d_out_sq), out_sq_stride, vp(d_out_len), None)

    def variance_temporal(d_mean=b["hist"], mean_stride=NPX, d_msq=b["hist_sq"], msq_stride=NPX, d_len=b["hist_len"], ws=W, h=H,
                          d_guides=b["guides"], guide_stride=NPX, s=dv(), spatial_below=4.0, d_out=b["out"], out_stride=NPX, d_work=b["work"],
                          work_stride=NPX):
        return lib.rt_film_denoise_variance_temporal(ctx, vp(d_mean), mean_stride, vp(d_msq), msq_stride, vp(d_len), ws, h, vp(d_guides),
                                                     guide_stride, ref(s), spatial_below, vp(d_out), out_stride, vp(d_work), work_stride, None)

    make = dict(params=lambda **k: r.params(0.1, 0.7, 0.5, **{"depth": 2, **k}), tone=tone, dn=dn, dv=dv, tp=tp)
    return make, dict(moments=moments, resolve=resolve, denoise=denoise, variance=variance, temporal=temporal,
                      temporal_moments=temporal_moments, variance_temporal=variance_temporal)


def _film_refusals(L, mk, e, b):
    """(name, call, code, text) of every refusal of the seven entries on a context whose scene, camera and closed-form 16 x 8 grid are set."""
    out = []

    def add(entry, what, text, code=BAD_ARG, prefix=True, **kw):
        name = {"moments": "rt_film_accumulate_moments", "resolve": "rt_film_resolve", "denoise": "rt_film_denoise",
                "variance": "rt_film_denoise_variance", "temporal": "rt_film_temporal", "temporal_moments": "rt_film_temporal_moments",
                "variance_temporal": "rt_film_denoise_variance_temporal"}[entry]
        out.append((f"{name}: {what}", lambda c=e[entry], k=kw: c(**k), code, f"{name}: {text}" if prefix else text))

    params, tone, dn, dv, tp = mk["params"], mk["tone"], mk["dn"], mk["dv"], mk["tp"]
    # rt_film_accumulate_moments: what every entry with rt_params shares, then its own
    for what, kw, text in [("params NULL", dict(p=None), "params is NULL"), ("depth -1", dict(p=params(depth=-1)), "depth outside 0..RT_MAX_DEPTH"),
                           ("depth 17", dict(p=params(depth=L.RT_MAX_DEPTH + 1)), "depth outside 0..RT_MAX_DEPTH"),
                           ("aa_mode 3", dict(p=params(aa=3)), "unknown aa_mode"),
                           ("spp 0", dict(p=params(aa=L.RT_AA_STOCHASTIC, spp=0)), "spp outside 1..RT_MAX_SPP"),
                           ("spp 65", dict(p=params(aa=L.RT_AA_STOCHASTIC, spp=L.RT_MAX_SPP + 1)), "spp outside 1..RT_MAX_SPP"),
                           ("x0 -1", dict(x0=-1), COLUMNS), ("x1 w+1", dict(x1=W + 1), COLUMNS), ("x0 == x1", dict(x0=8, x1=8), COLUMNS),
                           ("depth 17 and x1 w+1", dict(p=params(depth=17), x1=W + 1), "depth outside 0..RT_MAX_DEPTH"),
                           ("x1 w+1 and passes 0", dict(x1=W + 1, passes=0), COLUMNS)]:
        add("moments", what, text, prefix=False, **kw)
    add("moments", "passes 0", "passes < 1", passes=0)
    add("moments", "d_sum NULL", "d_sum is NULL", d_sum=None)
    add("moments", "d_sq NULL", "d_sq is NULL", d_sq=None)
    add("moments", "d_sq == d_sum", "d_sq and d_sum must be buffers of their own", d_sq=b["acc_sum"])
    add("moments", "short sum_stride", "sum_stride smaller than the slab", sum_stride=NPX - 1)
    add("moments", "short sum_stride of a slab", "sum_stride smaller than the slab", x0=8, sum_stride=8 * H - 1)
    add("moments", "short sq_stride", "sq_stride smaller than the slab", sq_stride=NPX - 1)
    add("moments", "passes 0 and d_sum NULL", "passes < 1", passes=0, d_sum=None)
    add("moments", "d_sum NULL and d_sq NULL", "d_sum is NULL", d_sum=None, d_sq=None)
    add("moments", "d_sq == d_sum and a short sum_stride", "d_sq and d_sum must be buffers of their own", d_sq=b["acc_sum"], sum_stride=NPX - 1)
    add("moments", "short sum_stride and sq_stride", "sum_stride smaller than the slab", sum_stride=1, sq_stride=1)
    # rt_film_resolve
    area = "ws*h outside 1..RT_FILM_MAX_PIXELS"
    add("resolve", "d_sum NULL", "d_sum is NULL", d_sum=None)
    add("resolve", "tone NULL", "tone is NULL", t=None)
    add("resolve", "d_sum NULL and tone NULL", "d_sum is NULL", d_sum=None, t=None)
    add("resolve", "ws 0", area, ws=0)
    add("resolve", "h 0", area, h=0)
    add("resolve", "ws*h 2^28", area, ws=BIG_SIDE, h=BIG_SIDE)
    add("resolve", "n 0", "n < 1", n=0)
    add("resolve", "ws 0 and n 0", area, ws=0, n=0)
    for x in (0.0, -1.0, INF, NAN):
        add("resolve", f"exposure {x}", "exposure must be finite and > 0", t=tone(exposure=x))
    for x in (-1.0, INF, NAN):
        add("resolve", f"white {x}", "white must be 0, or finite and > 0", t=tone(white=x))
    for x in (0, 3):
        add("resolve", f"gamma {x}", "gamma must be 1 or 2", t=tone(gamma=x))
    add("resolve", "n 0 and exposure 0", "n < 1", n=0, t=tone(exposure=0.0))
    add("resolve", "exposure 0 and gamma 3", "exposure must be finite and > 0", t=tone(exposure=0.0, gamma=3))
    for x in (L.RT_FLAG_TYPED_BIAS, L.RT_FLAG_COUNT_RAYS, 1 << 30):
        add("resolve", f"flags {x}", "unknown flag bit", t=tone(flags=x))
    add("resolve", "gamma 3 and an unknown flag", "gamma must be 1 or 2", t=tone(gamma=3, flags=1))
    add("resolve", "both outputs NULL", BOTH_NULL, prefix=False, d_u8=None, d_f32=None)
    add("resolve", "an unknown flag and both outputs NULL", "unknown flag bit", t=tone(flags=1), d_u8=None, d_f32=None)
    add("resolve", "short sum_stride", "sum_stride smaller than the frame", sum_stride=NPX - 1)
    add("resolve", "both outputs NULL and a short sum_stride", BOTH_NULL, prefix=False, d_u8=None, d_f32=None, sum_stride=1)
    hwc = tone(flags=L.RT_FLAG_U8_HWC)
    add("resolve", "HWC with float32", HWC_RESOLVE, prefix=False, t=hwc, out_stride=W)
    add("resolve", "HWC with float32 and a short pitch", HWC_RESOLVE, prefix=False, t=hwc, out_stride=W - 1)
    add("resolve", "HWC short pitch", "row pitch smaller than the frame width", prefix=False, t=hwc, d_f32=None, out_stride=W - 1)
    add("resolve", "short out_stride", "out_stride smaller than the frame", prefix=False, out_stride=NPX - 1)
    add("resolve", "short sum_stride and out_stride", "sum_stride smaller than the frame", sum_stride=1, out_stride=1)
    # the two filters and the filter on a temporal mean: their settings, the frame, the strides, d_work, the aliasing rules
    own = "d_out and d_work must be buffers of their own"
    stride = "a plane stride is smaller than the frame"
    shin = "normal_shin must be 1, 2, 4, ..., 1024"
    for ent, nulls, inputs, strides, need_work in [
            ("denoise", ("d_sum", "d_guides", "s", "d_out"), dict(d_sum="sum", d_guides="guides"),
             ("sum_stride", "guide_stride", "out_stride", "work_stride"), 2),
            ("variance", ("d_sum", "d_sq", "d_guides", "s", "d_out"), dict(d_sum="sum", d_sq="sq", d_guides="guides"),
             ("sum_stride", "sq_stride", "guide_stride", "out_stride", "work_stride"), 1),
            ("variance_temporal", ("d_mean", "d_msq", "d_len", "d_guides", "s", "d_out"),
             dict(d_mean="hist", d_msq="hist_sq", d_len="hist_len", d_guides="guides"),
             ("mean_stride", "msq_stride", "guide_stride", "out_stride", "work_stride"), 1)]:
        st = dn if ent == "denoise" else dv
        sname = "dn" if ent == "denoise" else "dv"
        for i, a in enumerate(nulls):
            add(ent, f"{a} NULL", f"{sname if a == 's' else a} is NULL", **{a: None})
            if i + 1 < len(nulls):                               # two at once: the NULL pointers are reported in argument order
                add(ent, f"{a} NULL and {nulls[i + 1]} NULL", f"{sname if a == 's' else a} is NULL", **{a: None, nulls[i + 1]: None})
        for x in (-1, 7):
            add(ent, f"levels {x}", "levels outside 0..6", s=st(levels=x))
        for x in (0, 3, 2048, -2):
            add(ent, f"normal_shin {x}", shin, s=st(normal_shin=x))
        add(ent, "levels 7 and normal_shin 3", "levels outside 0..6", s=st(levels=7, normal_shin=3))
        add(ent, "demodulate 2", "demodulate must be 0 or 1", s=st(demodulate=2))
        add(ent, "demodulate -1", "demodulate must be 0 or 1", s=st(demodulate=-1))
        for what, kw in (("ws 0", dict(ws=0)), ("h 0", dict(h=0)), ("ws*h 2^28", dict(ws=BIG_SIDE, h=BIG_SIDE))):
            add(ent, what, area, **kw)
        add(ent, "demodulate 2 and ws 0", "demodulate must be 0 or 1", s=st(demodulate=2), ws=0)
        add(ent, "ws 0 and short strides", area, ws=0, out_stride=-1)
        for a in strides:
            add(ent, f"short {a}", stride, **{a: NPX - 1})
        add(ent, f"d_work NULL with levels {need_work}", f"d_work is NULL with levels >= {need_work}", d_work=None, s=st(levels=need_work))
        add(ent, "a short out_stride and d_work NULL", stride, out_stride=NPX - 1, d_work=None)
        add(ent, "d_work NULL and d_out == d_guides", f"d_work is NULL with levels >= {need_work}", d_work=None, d_out=b["guides"])
        for a, src in inputs.items():
            add(ent, f"d_out == {a}", own, d_out=b[src])
            add(ent, f"d_work == {a}", own, d_work=b[src])
        add(ent, "d_work == d_out", own, d_work=b["out"])
    add("denoise", "n 0", "n < 1", n=0)
    add("denoise", "d_out NULL and n 0", "d_out is NULL", d_out=None, n=0)
    add("denoise", "n 0 and levels 7", "n < 1", n=0, s=dn(levels=7))
    for x in (-1.0, INF, NAN):
        add("denoise", f"sigma {x}", "sigma must be 0, or finite and > 0", s=dn(sigma=x))
    add("denoise", "normal_shin 3 and sigma -1", shin, s=dn(normal_shin=3, sigma=-1.0))
    add("denoise", "sigma -1 and demodulate 2", "sigma must be 0, or finite and > 0", s=dn(sigma=-1.0, demodulate=2))
    add("denoise", "reserved 1", "reserved must be 0", s=dn(reserved=1))
    add("denoise", "demodulate 2 and reserved 1", "demodulate must be 0 or 1", s=dn(demodulate=2, reserved=1))
    add("denoise", "reserved 1 and ws 0", "reserved must be 0", s=dn(reserved=1), ws=0)
    add("denoise", "d_work NULL with levels 2 and d_out == d_sum", "d_work is NULL with levels >= 2", d_work=None, d_out=b["sum"])
    add("variance", "n 1", "n < 2", n=1)
    add("variance", "n 0", "n < 2", n=0)
    add("variance", "d_out NULL and n 1", "d_out is NULL", d_out=None, n=1)
    add("variance", "n 1 and levels -1", "n < 2", n=1, s=dv(levels=-1))
    for ent in ("variance", "variance_temporal"):
        for x in (-1.0, INF, NAN):
            add(ent, f"kappa {x}", "kappa must be finite and >= 0", s=dv(kappa=x))
            add(ent, f"var_floor {x}", "var_floor must be finite and >= 0", s=dv(var_floor=x))
        add(ent, "normal_shin 3 and kappa -1", shin, s=dv(normal_shin=3, kappa=-1.0))
        add(ent, "kappa -1 and var_floor -1", "kappa must be finite and >= 0", s=dv(kappa=-1.0, var_floor=-1.0))
        add(ent, "var_floor -1 and demodulate 2", "var_floor must be finite and >= 0", s=dv(var_floor=-1.0, demodulate=2))
        add(ent, "prefilter 2", "prefilter must be 0 or 1", s=dv(prefilter=2))
        add(ent, "demodulate 2 and prefilter 2", "demodulate must be 0 or 1", s=dv(demodulate=2, prefilter=2))
    add("variance", "prefilter 2 and ws 0", "prefilter must be 0 or 1", s=dv(prefilter=2), ws=0)
    for x in (-1.0, INF, NAN):
        add("variance_temporal", f"spatial_below {x}", "spatial_below must be finite and >= 0", spatial_below=x)
    add("variance_temporal", "prefilter 2 and spatial_below -1", "prefilter must be 0 or 1", s=dv(prefilter=2), spatial_below=-1.0)
    add("variance_temporal", "spatial_below -1 and ws 0", "spatial_below must be finite and >= 0", spatial_below=-1.0, ws=0)
    # rt_film_temporal and rt_film_temporal_moments: the second repeats the first's checks in the first's order, then adds its own
    own = "d_out and d_out_len must be buffers of their own"
    t_bufs = ("d_sum", "d_guides", "d_hist", "d_hist_len", "d_hist_guides", "d_out", "d_out_len")
    t_ins = dict(d_sum=b["sum"], d_guides=b["guides"], d_hist=b["hist"], d_hist_len=b["hist_len"], d_hist_guides=b["hist_guides"])
    for ent in ("temporal", "temporal_moments"):
        for a in t_bufs:
            add(ent, f"{a} NULL", "a buffer is NULL", **{a: None})
        add(ent, "tp NULL", "tp is NULL", t=None)
        add(ent, "d_hist NULL and tp NULL", "a buffer is NULL", d_hist=None, t=None)
        for x in (0, -1, (1 << 24) + 1):
            add(ent, f"n {x}", "n outside 1..2^24", n=x)
        add(ent, "tp NULL and n 0", "tp is NULL", t=None, n=0)
        for x in (-1.0, INF, NAN):
            add(ent, f"depth_tol {x}", "depth_tol must be finite and >= 0", t=tp(depth_tol=x))
            add(ent, f"max_history {x}", "max_history must be finite and >= 0", t=tp(max_history=x))
        for x in (-1.5, 1.5, NAN):
            add(ent, f"normal_cos {x}", "normal_cos outside [-1, 1]", t=tp(normal_cos=x))
        add(ent, "n 0 and depth_tol -1", "n outside 1..2^24", n=0, t=tp(depth_tol=-1.0))
        add(ent, "depth_tol -1 and normal_cos 2", "depth_tol must be finite and >= 0", t=tp(depth_tol=-1.0, normal_cos=2.0))
        add(ent, "normal_cos 2 and max_history -1", "normal_cos outside [-1, 1]", t=tp(normal_cos=2.0, max_history=-1.0))
        add(ent, "reserved[0] 1", "reserved must be 0", t=tp(reserved=(1, 0)))
        add(ent, "reserved[1] 1", "reserved must be 0", t=tp(reserved=(0, 1)))
        add(ent, "max_history -1 and reserved", "max_history must be finite and >= 0", t=tp(max_history=-1.0, reserved=(1, 1)))
        add(ent, "prev_origin NaN", "a camera entry is not finite", t=tp(prev_origin=(0.0, NAN, 0.0)))
        add(ent, "prev_rotation Inf", "a camera entry is not finite", t=tp(prev_rotation=(1.0, 0, 0, 0, 1, 0, 0, 0, INF)))
        add(ent, "reserved and prev_origin NaN", "reserved must be 0", t=tp(reserved=(0, 1), prev_origin=(NAN, 0.0, 0.0)))
        for a in ("sum_stride", "guide_stride", "hist_stride", "hist_guide_stride", "out_stride"):
            add(ent, f"short {a}", "a plane stride is smaller than the frame", **{a: NPX - 1})
        add(ent, "prev_origin NaN and a short stride", "a camera entry is not finite", t=tp(prev_origin=(NAN, 0.0, 0.0)), sum_stride=1)
        for a, src in t_ins.items():
            add(ent, f"d_out == {a}", own, d_out=src)
            add(ent, f"d_out_len == {a}", own, d_out_len=src)
        add(ent, "d_out == d_out_len", own, d_out_len=b["out"])
        add(ent, "a short stride and d_out == d_sum", "a plane stride is smaller than the frame", out_stride=NPX - 1, d_out=b["sum"])
    sq_null, sq_stride = "d_sq, d_hist_sq or d_out_sq is NULL", "a plane stride of the second moment is smaller than the frame"
    sq_own = "d_out_sq must be a buffer of its own"
    for a in ("d_sq", "d_hist_sq", "d_out_sq"):
        add("temporal_moments", f"{a} NULL", sq_null, **{a: None})
    for a in ("sq_stride", "hist_sq_stride", "out_sq_stride"):
        add("temporal_moments", f"short {a}", sq_stride, **{a: NPX - 1})
    for a, src in dict(t_ins, d_sq=b["sq"], d_hist_sq=b["hist_sq"], d_out=b["out"], d_out_len=b["out_len"]).items():
        add("temporal_moments", f"d_out_sq == {a}", sq_own, d_out_sq=src)
    for a, src in (("d_sq", b["sq"]), ("d_hist_sq", b["hist_sq"])):
        add("temporal_moments", f"d_out == {a}", own, d_out=src)
        add("temporal_moments", f"d_out_len == {a}", own, d_out_len=src)
    # the order a caller can see: a NULL d_sq only after every check shared with rt_film_temporal
    add("temporal_moments", "d_sq NULL and n 0", "n outside 1..2^24", d_sq=None, n=0)
    add("temporal_moments", "d_sq NULL and tp NULL", "tp is NULL", d_sq=None, t=None)
    add("temporal_moments", "d_sq NULL and a short sum_stride", "a plane stride is smaller than the frame", d_sq=None, sum_stride=NPX - 1)
    add("temporal_moments", "d_sq NULL and d_out == d_hist", own, d_sq=None, d_out=b["hist"])
    add("temporal_moments", "d_out_sq NULL and a short sq_stride", sq_null, d_out_sq=None, sq_stride=1)
    add("temporal_moments", "short sq_stride and d_out_sq == d_sum", sq_stride, sq_stride=NPX - 1, d_out_sq=b["sum"])
    add("temporal_moments", "d_out_sq == d_sum and d_out == d_sq", sq_own, d_out_sq=b["sum"], d_out=b["sq"])
    return out


def test_film_refusals_and_their_texts():
    """Every refusal of the seven film entries after rt_film_accumulate, through the library, with its code and rt_last_error text as
    literals, and with two bad arguments at once wherever the order of the checks decides which one the caller sees.  A refused call
    writes nothing: every output buffer still holds the bytes it was filled with.  At the end every entry accepts the good arguments."""
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    r, bufs = _film_open(pkg, L)
    try:
        r.set_scene(SPHERES, LIGHTS, PLANES)
        r.set_camera(CAM_O, CAM_R)
        r.set_raygen(W, H, *RAYGEN)
        r.render_guides(0, W, bufs["guides"])
        r.render_guides(0, W, bufs["hist_guides"])
        _fill_outputs(r, bufs)
        r.sync()
        mk, e = _film_entries(r, L, bufs)
        cases = _film_refusals(L, mk, e, bufs)
        wrong = []
        for name, call, code, text in cases:
            st = call()
            if (st, _last_error(r)) != (code, text):
                wrong.append((name, st, _last_error(r), code, text))
            r.sync()
            touched = _outputs_untouched(r, bufs)
            if touched:
                wrong.append((name, f"the refused call wrote {touched}"))
                _fill_outputs(r, bufs)
        assert not wrong, wrong[:6]
        assert len(cases) > 300 and len({c[0] for c in cases}) == len(cases)
        # a camera entry that is not finite, on the current camera's side; two at once: with a frame above RT_FILM_MAX_PIXELS
        for ent, name in (("temporal", "rt_film_temporal"), ("temporal_moments", "rt_film_temporal_moments")):
            for o, R in ((np.array([0.0, NAN, 0.0]), CAM_R), (CAM_O, np.diag([1.0, INF, 1.0]))):
                r.set_camera(o, R)
                assert (e[ent](), _last_error(r)) == (BAD_ARG, f"{name}: a camera entry is not finite"), (ent, o)
                r.set_raygen(BIG_SIDE, BIG_SIDE, *RAYGEN)
                assert (e[ent](), _last_error(r)) == (BAD_ARG, f"{name}: a camera entry is not finite"), (ent, o)
                r.set_raygen(W, H, *RAYGEN)
            r.set_camera(CAM_O, CAM_R)
        # a frame above RT_FILM_MAX_PIXELS; two at once: with strides far below it, and with an output that is an input
        r.set_raygen(BIG_SIDE, BIG_SIDE, *RAYGEN)
        for ent, name in (("temporal", "rt_film_temporal"), ("temporal_moments", "rt_film_temporal_moments")):
            assert (e[ent](), _last_error(r)) == (BAD_ARG, f"{name}: w*h above RT_FILM_MAX_PIXELS"), ent
            assert (e[ent](d_out=bufs["sum"]), _last_error(r)) == (BAD_ARG, f"{name}: w*h above RT_FILM_MAX_PIXELS"), ent
            assert (e[ent](t=mk["tp"](prev_origin=(NAN, 0.0, 0.0))), _last_error(r)) == (BAD_ARG, f"{name}: a camera entry is not finite"), ent
        above = "(x1-x0)*h above RT_FILM_MAX_PIXELS"
        assert (e["moments"](x1=BIG_SIDE), _last_error(r)) == (BAD_ARG, f"rt_film_accumulate_moments: {above}")
        assert (e["moments"](x1=BIG_SIDE, d_sq=bufs["acc_sum"]), _last_error(r)) == (
            BAD_ARG, "rt_film_accumulate_moments: d_sq and d_sum must be buffers of their own")
        lib, good = r._lib, r.params(0.1, 0.7, 0.5, 2)
        assert (lib.rt_film_accumulate(r._ctx, C.byref(good), 0, BIG_SIDE, 1, 1, C.c_void_p(bufs["acc_sum"]), NPX, None), _last_error(r)) == (
            BAD_ARG, f"rt_film_accumulate: {above}")
        r.set_raygen(W, H, *RAYGEN)
        # the grid: dy or dz 0
        for rg in ((1.0, 2.0, 0.0, 1.0, -0.25), (1.0, 2.0, -0.25, 1.0, 0.0)):
            r.set_raygen(W, H, *rg)
            for ent, name in (("temporal", "rt_film_temporal"), ("temporal_moments", "rt_film_temporal_moments")):
                assert (e[ent](), _last_error(r)) == (STATE, f"{name}: the grid's dy or dz is 0"), (ent, rg)
                # two at once: before the cameras are looked at
                assert (e[ent](t=mk["tp"](prev_origin=(NAN, 0.0, 0.0))), _last_error(r)) == (STATE, f"{name}: the grid's dy or dz is 0"), (ent, rg)
        r.set_raygen(W, H, *RAYGEN)
        r.sync()
        assert _outputs_untouched(r, bufs) is None
        # every entry accepts the good arguments; the filters also without d_work where they need none, whatever work_stride is
        for name, call in e.items():
            assert call() == L.RT_OK, (name, _last_error(r))
        assert e["denoise"](d_work=None, work_stride=0, s=mk["dn"](levels=1)) == L.RT_OK, _last_error(r)
        assert e["denoise"](d_work=None, work_stride=0, s=mk["dn"](levels=0)) == L.RT_OK, _last_error(r)
        assert e["variance"](d_work=None, work_stride=0, s=mk["dv"](levels=0)) == L.RT_OK, _last_error(r)
        assert e["variance_temporal"](d_work=None, work_stride=0, s=mk["dv"](levels=0)) == L.RT_OK, _last_error(r)
        assert e["resolve"](t=mk["tone"](flags=L.RT_FLAG_U8_HWC | L.RT_FLAG_U8_RGB), d_f32=None, out_stride=W) == L.RT_OK, _last_error(r)
        assert e["resolve"](d_u8=None) == L.RT_OK and e["resolve"](d_f32=None) == L.RT_OK, _last_error(r)
        r.sync()
    finally:
        for b in bufs.values():
            r.free(b)
        r.close()


def test_film_temporal_refusals_of_an_unfinished_context():
    """rt_film_temporal and rt_film_temporal_moments ask for a camera and a closed-form grid, in that order, after their settings and
    before the cameras' entries; they do not ask for a scene."""
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    r, bufs = _film_open(pkg, L)
    try:
        _fill_outputs(r, bufs)
        mk, e = _film_entries(r, L, bufs)
        both = (("temporal", "rt_film_temporal"), ("temporal_moments", "rt_film_temporal_moments"))

        def all_say(code, text, **kw):
            for ent, name in both:
                assert (e[ent](**kw), _last_error(r)) == (code, f"{name}: {text}"), (ent, kw)
        bad_cam = mk["tp"](prev_origin=(NAN, 0.0, 0.0))
        all_say(STATE, "rt_set_camera has not been called")
        all_say(STATE, "rt_set_camera has not been called", t=bad_cam)
        all_say(BAD_ARG, "reserved must be 0", t=mk["tp"](reserved=(1, 0)))
        all_say(BAD_ARG, "a buffer is NULL", d_sum=None)
        r.set_camera(CAM_O, CAM_R)
        all_say(STATE, "rt_set_raygen has not been called")
        all_say(STATE, "rt_set_raygen has not been called", t=bad_cam, sum_stride=1)
        y, z = np.meshgrid(RAYGEN[1] + RAYGEN[2] * np.arange(W), RAYGEN[3] + RAYGEN[4] * np.arange(H), indexing="ij")
        r.set_pixel_loc(np.stack([np.full((W, H), RAYGEN[0]), y, z]))
        # two at once: an explicit grid on a context whose closed-form grid was never set (dy == dz == 0)
        all_say(STATE, "an explicit rt_set_pixel_loc grid cannot be reprojected")
        all_say(STATE, "an explicit rt_set_pixel_loc grid cannot be reprojected", t=bad_cam)
        assert (e["temporal_moments"](d_sq=None), _last_error(r)) == (STATE, "rt_film_temporal_moments: an explicit rt_set_pixel_loc grid cannot be reprojected")
        r.set_raygen(W, H, *RAYGEN)
        r.set_pixel_loc(np.stack([np.full((W, H), RAYGEN[0]), y, z]))
        all_say(STATE, "an explicit rt_set_pixel_loc grid cannot be reprojected")
        r.sync()
        assert _outputs_untouched(r, bufs) is None
        r.set_raygen(W, H, *RAYGEN)
        for ent, _ in both:
            assert e[ent]() == L.RT_OK, (ent, _last_error(r))
        r.sync()
    finally:
        for b in bufs.values():
            r.free(b)
        r.close()
