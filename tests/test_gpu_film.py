"""The film on the GPU (rt_film_accumulate, rt_film_resolve; the two kernels of rt_film.h).  Truth for a pass is the unchanged
render path, render_device with a float32 output and seed s + i, fed to the numpy restatements of python-ray-tracer_amd/film.py;
every comparison is bit for bit.  Accumulate on three scenes and five pass counts over a NaN-filled sum, in two steps, in column
slabs in place; one case against the CPU oracle's frames; tiny frames, a 1080p frame and one whose passes go one by one; resolve on synthetic sums of every awkward
size, stride, layout, output and tone; the identity at n = 1; two streams; the error paths; the example."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_frame, raygen_closed_form
from feature_gpu import IGNORED
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_film import EDGE_SUMS, random_sums, same_bits
from test_oracle_features import _records

from python_ray_tracer_amd import Film, film as F
from python_ray_tracer_amd import _lib as L

pytestmark = pytest.mark.gpu
PASS_COUNTS = (1, 2, 4, 5, 9)                  # below a batch of four, one batch, one batch plus one, two batches plus one


# ---------------------------------------------------------------------------------------------------------------------
# The three scenes, from inputs stored in fixtures

def _lens_scene(r):
    """lens_soft_glass_rough_48_d4 under RT_AA_NONE: the seed drives the lens, light and scatter hashes."""
    g = np.load(os.path.join(GOLDEN, "lens_soft_glass_rough_48_d4.npz"))
    w, h = int(g["w"]), int(g["h"])
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]),
                light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]))
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(float(g["aperture"]), float(g["focus_distance"]))
    r.set_raygen(w, h, *raygen_closed_form(w, h, float(g["fov"])))
    return w, h, lambda seed: r.params(**IGNORED, depth=int(g["depth"]), aa=0, seed=seed), int(g["seed"])


def _sky_scene(r):
    """sky_stoch_40x24_spp3_seed7 under RT_AA_STOCHASTIC."""
    g = np.load(os.path.join(GOLDEN, "sky_stoch_40x24_spp3_seed7.npz"))
    w, h = int(g["w"]), int(g["h"])
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=(g["materials"], g["sphere_material"], g["plane_material"]),
                light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]), light_rgb=g["light_rgb"], sky=g["sky"])
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(0.0, 1.0)
    r.set_raygen(w, h, *raygen_closed_form(w, h, float(g["fov"])))
    return w, h, lambda seed: r.params(**IGNORED, depth=int(g["depth"]), aa=2, spp=int(g["spp"]), seed=seed), int(g["seed"])


def _odd_scene(r):
    """frame_odd_37x29 under RT_AA_STOCHASTIC with spp 1 and no material table: 1073 elements per plane, odd plane bases."""
    g = load_frame("odd_37x29")
    w, h = int(g["w"]), int(g["h"])
    r.set_scene(g["spheres"], g["lights"], g["planes"])
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_lens(0.0, 1.0)
    r.set_raygen(w, h, *raygen_closed_form(w, h, float(g["fov"])))
    return w, h, lambda seed: r.params(float(g["amb"]), float(g["lamb"]), float(g["refl"]), int(g["depth"]), 2, spp=1, seed=seed), 21


SCENES = {"lens": _lens_scene, "sky": _sky_scene, "odd": _odd_scene}
_TRUTH = {}


def _pass_frames(r, name, params_of, seed, n, w, h, x0=0, x1=None):
    """float32 (3, x1-x0, h) frames of seeds seed .. seed+n-1 through rt_render_device: computed once per (scene, seed, slab)."""
    x1 = w if x1 is None else x1
    out = []
    d32 = None
    for i in range(n):
        key = (name, (seed + i) & 0xFFFFFFFF, x0, x1)
        if key not in _TRUTH:
            if d32 is None:
                d32 = r.malloc(12 * (x1 - x0) * h)
            r.render_device(params_of(seed + i), x0, x1, None, d32)
            r.sync()
            a = np.empty((3, x1 - x0, h), np.float32)
            r.d2h(a, d32)
            a.setflags(write=False)
            _TRUTH[key] = a
        out.append(_TRUTH[key])
    if d32 is not None:
        r.free(d32)
    return out


def _nan_sum(r, n_doubles):
    d = r.malloc(8 * n_doubles)
    r.h2d(d, np.full(n_doubles, np.nan))
    return d


def _read(r, d, shape, dtype=np.float64):
    a = np.empty(shape, dtype)
    r.d2h(a, d)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# Accumulate

@pytest.mark.parametrize("passes", PASS_COUNTS)
@pytest.mark.parametrize("scene", list(SCENES))
def test_accumulate_is_the_sum_of_the_render_paths_frames(rend, scene, passes):
    w, h, params_of, seed = SCENES[scene](rend)
    frames = _pass_frames(rend, scene, params_of, seed, passes, w, h)
    stride = w * h + 3                                           # (planes apart by more than the frame: the gap stays NaN)
    d = _nan_sum(rend, 3 * stride)
    try:
        rend.film_accumulate(params_of(seed), 0, w, passes, True, d, stride)
        rend.sync()
        got = _read(rend, d, (3, stride))
    finally:
        rend.free(d)
    want = F.accumulate_reference(None, frames)
    assert same_bits(got[:, :w * h].reshape(3, w, h), want), f"{scene} x {passes} passes"
    assert np.isnan(got[:, w * h:]).all()
    if scene == "lens" and passes == 2:                           # the seeds really advance
        assert not np.array_equal(want, F.accumulate_reference(None, [frames[0], frames[0]]))


@pytest.mark.parametrize("scene", list(SCENES))
def test_accumulate_in_two_steps_and_in_slabs(rend, scene):
    w, h, params_of, seed = SCENES[scene](rend)
    frames = _pass_frames(rend, scene, params_of, seed, 5, w, h)
    want = F.accumulate_reference(None, frames)
    d = _nan_sum(rend, 3 * w * h)
    try:
        rend.film_accumulate(params_of(seed), 0, w, 3, True, d)                      # 3 passes, then 2 more with the seed advanced
        rend.film_accumulate(params_of(seed + 3), 0, w, 2, False, d)
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), want), "3 + 2 passes"
        rend.h2d(d, np.full(3 * w * h, np.nan))
        xm = 13                                                   # two column slabs in place into the full-frame sum (13 h is odd
        for x0, x1 in ((0, xm), (xm, w)):                         # for the odd frame: the second slab's planes are 8-byte aligned)
            rend.film_accumulate(params_of(seed), x0, x1, 5, True, d + 8 * x0 * h, w * h)
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), want), "two slabs in place"
    finally:
        rend.free(d)


def test_film_object_counts_passes_and_resolves(rend):
    w, h, params_of, seed = _lens_scene(rend)
    frames = _pass_frames(rend, "lens", params_of, seed, 6, w, h)
    with Film(rend) as film:
        film.accumulate(params_of(seed), 4)
        film.accumulate(params_of(seed + 4), 2)
        assert film.passes == 6
        total = F.accumulate_reference(None, frames)
        u8, f32 = film.resolve(exposure=0.8, white=400.0, gamma=2, f32=True)
        v = F.tone_reference(total, 6, 0.8, 400.0, 2)
        assert same_bits(f32, v.astype(np.float32)) and np.array_equal(u8, F.clip_reference(v)[[0, 2, 1]])
        img, none = film.resolve(white=400.0, flags=L.RT_FLAG_U8_HWC | L.RT_FLAG_U8_RGB)
        assert none is None and np.array_equal(img, F.clip_reference(F.tone_reference(total, 6, 1.0, 400.0, 1)).transpose(2, 1, 0))
        film.clear()
        film.accumulate(params_of(seed), 1)                       # after clear(): the sum starts again
        _, f32 = film.resolve(u8=False, f32=True)
        assert film.passes == 1 and same_bits(f32, frames[0] + np.float32(0.0))


def test_accumulate_vs_cpu_oracle(rend, oracle):
    g = np.load(os.path.join(GOLDEN, "sky_stoch_40x24_spp3_seed7.npz"))
    w, h, params_of, seed = _sky_scene(rend)
    assert seed == 7
    frames = []
    for i in range(3):
        ref = oracle.render(w, h, g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], 7.0, -3.0, 2.0, int(g["depth"]),
                            2, raygen=raygen_closed_form(w, h, float(g["fov"])), spp=int(g["spp"]), seed=7 + i, want=("f32",),
                            materials=(g["materials"], g["sphere_material"], g["plane_material"]), light_radius=g["light_radius"],
                            shadow_samples=int(g["shadow_samples"]), lens=(0.0, 1.0), light_rgb=g["light_rgb"], sky=g["sky"])
        frames.append(ref["f32"])
    assert not np.array_equal(frames[0], frames[1])
    want = F.accumulate_reference(None, frames)
    d, d8 = _nan_sum(rend, 3 * w * h), rend.malloc(3 * w * h)
    try:
        rend.film_accumulate(params_of(7), 0, w, 3, True, d)
        rend.film_resolve(d, w, h, 3, d8)
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), want)
        assert np.array_equal(_read(rend, d8, (3, w, h), np.uint8), F.clip_reference(F.tone_reference(want, 3))[[0, 2, 1]])
    finally:
        rend.free(d)
        rend.free(d8)


@pytest.mark.parametrize("w, h", [(1, 1), (1, 3), (5, 1), (8, 8)])
def test_tiny_frames(rend, w, h):
    """The tail-only and below-one-wave paths of both kernels."""
    g = load_frame("odd_37x29")
    rend.set_scene(g["spheres"], g["lights"], g["planes"])
    rend.set_camera(g["cam_origin"], g["cam_rot"])
    rend.set_raygen(w, h, 2.4, 1.0, -2.0 / max(w - 1, 1), 1.0, -2.0 / max(h - 1, 1))
    params_of = lambda seed: rend.params(0.0, 0.6, 0.3, 2, 2, spp=1, seed=seed)
    frames = _pass_frames(rend, f"tiny{w}x{h}", params_of, 3, 5, w, h)
    want = F.accumulate_reference(None, frames)
    d, d8, d32 = _nan_sum(rend, 3 * w * h), rend.malloc(3 * w * h), rend.malloc(12 * w * h)
    try:
        rend.film_accumulate(params_of(3), 0, w, 5, True, d)
        rend.film_resolve(d, w, h, 5, d8, d32, white=300.0)
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), want)
        v = F.tone_reference(want, 5, 1.0, 300.0, 1)
        assert same_bits(_read(rend, d32, (3, w, h), np.float32), v.astype(np.float32))
        assert np.array_equal(_read(rend, d8, (3, w, h), np.uint8), F.clip_reference(v)[[0, 2, 1]])
    finally:
        for p in (d, d8, d32):
            rend.free(p)
    assert want.any()


def test_large_frame_loops_past_the_grid_cap(rend):
    """The headline scene at 1920 x 1080, RT_AA_STOCHASTIC spp 1, 3 passes: 518 400 groups of four per plane against a grid of
    at most 8 blocks per CU, so every thread takes several groups."""
    from python_ray_tracer_amd import workloads
    wl = workloads.build(workloads.HEADLINE)
    cam, w, h = wl["camera"], wl["w"], wl["h"]
    assert (w, h) == (1920, 1080)
    rend.set_scene(wl["spheres"], wl["lights"], wl["planes"])
    rend.set_camera(cam.position, cam.rotation)
    rend.set_raygen(w, h, *cam.raygen())
    params_of = lambda seed: rend.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], 2, spp=1, seed=seed)
    frames = _pass_frames(rend, "headline", params_of, 11, 3, w, h)
    want = F.accumulate_reference(None, frames)
    d, d8 = _nan_sum(rend, 3 * w * h), rend.malloc(3 * w * h)
    try:
        rend.film_accumulate(params_of(11), 0, w, 3, True, d)
        rend.film_resolve(d, w, h, 3, d8, flags=L.RT_FLAG_U8_HWC | L.RT_FLAG_U8_RGB)
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), want)
        assert np.array_equal(_read(rend, d8, (h, w, 3), np.uint8), F.clip_reference(F.tone_reference(want, 3)).transpose(2, 1, 0))
    finally:
        rend.free(d)
        rend.free(d8)
    for k in [k for k in _TRUTH if k[0] == "headline"]:
        del _TRUTH[k]                                             # (75 MB of frames nobody else needs)


def test_passes_one_by_one_above_the_scratch_cap(rend):
    """Four float32 pass frames above FILM_SCRATCH_MAX = 256 MiB: rt_film_accumulate then renders and adds its passes one by one
    (batch = 1 with passes > 1), which is what a 4K or 8K film runs.  The headline scene at depth 1, RT_AA_STOCHASTIC spp 1, on
    2368 x 2362 = 5 593 216 pixels (from 5 592 406 on), 5 passes into a NaN-filled sum; then 2 + 3 passes, the same bits."""
    from python_ray_tracer_amd import workloads
    from python_ray_tracer_amd.scene import Camera
    w, h, passes = 2368, 2362, 5
    film_batch, scratch_max = 4, 256 << 20                        # rt_film.h: FILM_BATCH, FILM_SCRATCH_MAX
    fplane = (w * h + 3) & ~3                                     # mi355rt.hip: pass planes padded to four floats
    assert film_batch * fplane * 3 * 4 > scratch_max and passes > 1 and w * h == 5593216
    assert film_batch * 5592405 * 3 * 4 <= scratch_max < film_batch * 5592406 * 3 * 4    # (four unpadded frames of 12 B per pixel)
    t0 = time.perf_counter()
    wl = workloads.build(workloads.HEADLINE)
    cam = Camera(resolution=(w, h), **workloads.CAMERA)
    rend.set_scene(wl["spheres"], wl["lights"], wl["planes"])
    rend.set_camera(cam.position, cam.rotation)
    rend.set_raygen(w, h, *cam.raygen())
    params_of = lambda seed: rend.params(wl["amb"], wl["lamb"], wl["refl"], 1, 2, spp=1, seed=seed)
    try:
        want = F.accumulate_reference(None, _pass_frames(rend, "onebyone", params_of, 31, passes, w, h))
        assert not np.array_equal(_TRUTH[("onebyone", 31, 0, w)], _TRUTH[("onebyone", 35, 0, w)])
    finally:
        for k in [k for k in _TRUTH if k[0] == "onebyone"]:
            del _TRUTH[k]                                         # (335 MB of frames nobody else needs)
    t1 = time.perf_counter()
    d = _nan_sum(rend, 3 * w * h)
    try:
        rend.film_accumulate(params_of(31), 0, w, passes, True, d)
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), want), "5 passes one by one"
        rend.h2d(d, np.full(3 * w * h, np.nan))
        rend.film_accumulate(params_of(31), 0, w, 2, True, d)
        rend.film_accumulate(params_of(33), 0, w, 3, False, d)
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), want), "2 + 3 passes"
    finally:
        rend.free(d)
    assert want.any() and np.isfinite(want).all()
    print(f"one-by-one passes: truth {t1 - t0:.2f} s, two accumulates and read-backs {time.perf_counter() - t1:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------
# Resolve on synthetic sums (uploaded: no render)

SHAPES = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (5, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 1073: (37, 29), 2 ** 21 + 3: (419431, 5)}
TONES = [(e, wh, g) for e in (1.0, 0.37) for wh in (0.0, 255.0, 1000.0) for g in (1, 2)]
LAYOUTS = [(0, "u8"), (0, "f32"), (0, "both"), (L.RT_FLAG_U8_RGB, "u8"), (L.RT_FLAG_U8_RGB, "f32"), (L.RT_FLAG_U8_RGB, "both"),
           (L.RT_FLAG_U8_HWC, "u8"), (L.RT_FLAG_U8_HWC | L.RT_FLAG_U8_RGB, "u8")]
N_SYNTH = 3


def _synthetic(npx):
    rng = np.random.default_rng(npx)
    s = random_sums(rng, 3 * npx) * N_SYNTH
    rng.shuffle(s)
    k = min(3 * npx, 2 * EDGE_SUMS.size)
    s[:k] = np.concatenate([EDGE_SUMS, EDGE_SUMS * N_SYNTH])[:k]
    if npx > 64:
        rng.shuffle(s)
    return s.reshape(3, npx)


@pytest.mark.parametrize("npx", list(SHAPES))
def test_resolve_on_synthetic_sums(rend, npx):
    """Every (layout, outputs) x tone for the small sizes; for 2^21 + 3 pixels every layout and every tone at least once (twelve
    resolves, the layouts in rotation).  sum_stride and out_stride are larger than the plane (and odd or even with npx, so planes are
    16-, 8-, 4- and 1-byte aligned in turn), the image layout has a padded row pitch, and every byte outside the addressed elements
    must be untouched."""
    ws, h = SHAPES[npx]
    sums = _synthetic(npx)
    sstride, ostride, pitch = npx + 3, npx + 5, ws + 3
    host = np.full((3, sstride), -12345.0)
    host[:, :npx] = sums
    d = rend.malloc(host.nbytes)
    d8, d32 = rend.malloc(max(3 * ostride, 3 * h * pitch)), rend.malloc(12 * ostride)
    fill8, fill32 = np.full(max(3 * ostride, 3 * h * pitch), 0xA5, np.uint8), np.full(3 * ostride, -777.0, np.float32)
    combos = [(lay, t) for lay in LAYOUTS for t in TONES] if npx <= 1073 else [(LAYOUTS[i % len(LAYOUTS)], t) for i, t in enumerate(TONES)]
    vs = {}
    try:
        rend.h2d(d, host)
        for (flags, outs), (e, wh, g) in combos:
            if (e, wh, g) not in vs:
                v = F.tone_reference(sums, N_SYNTH, e, wh, g)
                with np.errstate(all="ignore"):
                    vs[(e, wh, g)] = (v.astype(np.float32), F.clip_reference(v))
            v32, v8 = vs[(e, wh, g)]
            what = f"npx={npx} flags={flags} outputs={outs} exposure={e} white={wh} gamma={g}"
            hwc = bool(flags & L.RT_FLAG_U8_HWC)
            rend.h2d(d8, fill8)
            rend.h2d(d32, fill32)
            rend.film_resolve(d, ws, h, N_SYNTH, d8 if outs != "f32" else None, d32 if outs != "u8" else None, exposure=e, white=wh,
                              gamma=g, flags=flags, sum_stride=sstride, out_stride=pitch if hwc else ostride)
            rend.sync()
            got8, got32 = _read(rend, d8, fill8.shape, np.uint8), _read(rend, d32, fill32.shape, np.float32)
            if outs == "u8":
                assert np.array_equal(got32, fill32), what
            else:
                got32 = got32.reshape(3, ostride)
                assert same_bits(got32[:, :npx], v32) and (got32[:, npx:] == -777.0).all(), what
            order = [0, 1, 2] if flags & L.RT_FLAG_U8_RGB else [0, 2, 1]
            if outs == "f32":
                assert np.array_equal(got8, fill8), what
            elif hwc:
                img = got8[:3 * h * pitch].reshape(h, pitch, 3)
                assert np.array_equal(img[:, :ws], v8[order].reshape(3, ws, h).transpose(2, 1, 0)), what
                assert (img[:, ws:] == 0xA5).all() and (got8[3 * h * pitch:] == 0xA5).all(), what
            else:
                planes = got8[:3 * ostride].reshape(3, ostride)
                assert np.array_equal(planes[:, :npx], v8[order]) and (planes[:, npx:] == 0xA5).all(), what
                assert (got8[3 * ostride:] == 0xA5).all(), what
        assert same_bits(_read(rend, d, host.shape), host)          # the sum is read only
    finally:
        for p in (d, d8, d32):
            rend.free(p)


def test_identity_at_n_1(rend):
    w, h, params_of, seed = _lens_scene(rend)
    frame = _pass_frames(rend, "lens", params_of, seed, 1, w, h)[0]
    d, d8, d32 = _nan_sum(rend, 3 * w * h), rend.malloc(3 * w * h), rend.malloc(12 * w * h)
    try:
        rend.film_accumulate(params_of(seed), 0, w, 1, True, d)
        rend.film_resolve(d, w, h, 1, d8, d32)
        rend.sync()
        assert same_bits(_read(rend, d32, (3, w, h), np.float32), frame + np.float32(0.0))   # (a -0.0 colour becomes +0.0 + -0.0 = +0.0)
        assert np.array_equal(_read(rend, d8, (3, w, h), np.uint8), F.clip_reference(frame.astype(np.float64))[[0, 2, 1]])
    finally:
        for p in (d, d8, d32):
            rend.free(p)


# ---------------------------------------------------------------------------------------------------------------------
# Streams

def test_two_streams_two_sums(rend):
    """Two accumulates of different scenes on two streams into two sums, queued together: the serial results (the scratch of pass
    frames is per stream, scene, lens and grid travel with the launches)."""
    wa, ha, pa, sa = _lens_scene(rend)
    want_a = F.accumulate_reference(None, _pass_frames(rend, "lens", pa, sa, 5, wa, ha))
    wb, hb, pb, sb = _sky_scene(rend)
    want_b = F.accumulate_reference(None, _pass_frames(rend, "sky", pb, sb, 5, wb, hb))
    s1, s2 = rend.stream_create(), rend.stream_create()
    da, db = _nan_sum(rend, 3 * wa * ha), _nan_sum(rend, 3 * wb * hb)
    try:
        _lens_scene(rend)
        rend.film_accumulate(pa(sa), 0, wa, 5, True, da, None, s1)
        _sky_scene(rend)
        rend.film_accumulate(pb(sb), 0, wb, 5, True, db, None, s2)
        rend.sync(s1)
        rend.sync(s2)
        assert same_bits(_read(rend, da, (3, wa, ha)), want_a), "stream 1"
        assert same_bits(_read(rend, db, (3, wb, hb)), want_b), "stream 2"
    finally:
        rend.stream_destroy(s1)
        rend.stream_destroy(s2)
        rend.free(da)
        rend.free(db)


# ---------------------------------------------------------------------------------------------------------------------
# Error paths

def test_errors_leave_the_sum_and_the_context(rend):
    import python_ray_tracer_amd as pkg
    w, h, params_of, seed = _sky_scene(rend)
    p = params_of(seed)
    want = F.accumulate_reference(None, _pass_frames(rend, "sky", params_of, seed, 2, w, h))
    npx = w * h
    d, d8 = _nan_sum(rend, 3 * npx), rend.malloc(3 * npx)
    nan = float("nan")
    try:
        rend.film_accumulate(p, 0, w, 1, True, d)
        rend.sync()
        before = _read(rend, d, (3, w, h))
        bad = {"passes 0": lambda: rend.film_accumulate(p, 0, w, 0, False, d),
               "passes -1": lambda: rend.film_accumulate(p, 0, w, -1, False, d),
               "NULL sum": lambda: rend.film_accumulate(p, 0, w, 1, False, None),
               "short sum_stride": lambda: rend.film_accumulate(p, 0, w, 1, False, d, npx - 1),
               "x range": lambda: rend.film_accumulate(p, 0, w + 1, 1, False, d, 2 * npx),
               "spp 0": lambda: rend.film_accumulate(rend.params(**IGNORED, depth=2, aa=2, spp=0), 0, w, 1, False, d),
               "n 0": lambda: rend.film_resolve(d, w, h, 0, d8),
               "exposure 0": lambda: rend.film_resolve(d, w, h, 1, d8, exposure=0.0),
               "exposure NaN": lambda: rend.film_resolve(d, w, h, 1, d8, exposure=nan),
               "white < 0": lambda: rend.film_resolve(d, w, h, 1, d8, white=-1.0),
               "white NaN": lambda: rend.film_resolve(d, w, h, 1, d8, white=nan),
               "gamma 3": lambda: rend.film_resolve(d, w, h, 1, d8, gamma=3),
               "unknown flag": lambda: rend.film_resolve(d, w, h, 1, d8, flags=L.RT_FLAG_U8_RGB | L.RT_FLAG_NO_FEEDBACK),
               "both outputs NULL": lambda: rend.film_resolve(d, w, h, 1, None, None),
               "resolve NULL sum": lambda: rend.film_resolve(None, w, h, 1, d8),
               "short resolve sum_stride": lambda: rend.film_resolve(d, w, h, 1, d8, sum_stride=npx - 1),
               "short out_stride": lambda: rend.film_resolve(d, w, h, 1, d8, out_stride=npx - 1),
               "short row pitch": lambda: rend.film_resolve(d, w, h, 1, d8, flags=L.RT_FLAG_U8_HWC, out_stride=w - 1),
               "float32 with the image layout": lambda: rend.film_resolve(d, w, h, 1, d8, d, flags=L.RT_FLAG_U8_HWC),
               "ws 0": lambda: rend.film_resolve(d, 0, h, 1, d8),
               "ws*h above RT_FILM_MAX_PIXELS": lambda: rend.film_resolve(d, 2 ** 14, 2 ** 13 + 1, 1, d8, sum_stride=2 ** 28, out_stride=2 ** 28)}
        for what, call in bad.items():
            with pytest.raises(pkg.RenderError) as e:
                call()
            assert e.value.status == L.RT_ERR_BAD_ARG, what
        # (x1-x0)*h above RT_FILM_MAX_PIXELS on a thin tall grid: refused before anything is launched
        launches = rend.stats()["launches"]
        rend.set_raygen(1, 2 ** 27 + 1, 2.4, 0.0, 0.0, 1.0, -2.0 / 2 ** 27)
        with pytest.raises(pkg.RenderError) as e:
            rend.film_accumulate(p, 0, 1, 1, False, d, 2 ** 27 + 1)
        assert e.value.status == L.RT_ERR_BAD_ARG and rend.stats()["launches"] == launches
        with pytest.raises(ValueError, match="RT_FILM_MAX_PIXELS"):
            Film(rend)
        rend.set_raygen(w, h, *raygen_closed_form(w, h, 45.0))
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), before), "a refused call touched the sum"
        rend.film_accumulate(params_of(seed + 1), 0, w, 1, False, d)   # the context is still usable
        rend.film_resolve(d, w, h, 2, d8)
        rend.sync()
        assert same_bits(_read(rend, d, (3, w, h)), want)
        assert np.array_equal(_read(rend, d8, (3, w, h), np.uint8), F.clip_reference(F.tone_reference(want, 2))[[0, 2, 1]])
    finally:
        rend.free(d)
        rend.free(d8)


# ---------------------------------------------------------------------------------------------------------------------
# The example

def test_example_with_passes_writes_png(tmp_path):
    """examples/render_png.py --passes: a film of 8 passes of the sky scene through a lens, highlights compressed towards 400."""
    from PIL import Image
    out = str(tmp_path / "film.png")
    log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--sky", "--dof", "0.1", "--passes", "8",
                                   "--white", "400", "--size", "64x64", "--frames", "2", "--out", out], text=True)
    assert "wrote" in log and "passes=8" in log
    img = np.asarray(Image.open(out))
    assert img.shape == (64, 64, 3) and img.any() and len(np.unique(img)) > 32
