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
