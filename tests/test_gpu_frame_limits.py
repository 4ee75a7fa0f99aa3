"""The frame-size limits of include/mi355rt.h on the GPU: a frame of exactly 2^31 pixels, frames one or two pixels thin up to the
longest side accepted and their transposes, both sides of RT_AA_REFERENCE's lattice switch, long sequences, rt_render's chunked
copies at pitches of 2^31 bytes and more, and a slab at x near 2^31 with every feature.

Every large frame is rendered into device buffers prefilled with a sentinel (uint8 0xA5, float32 a signalling NaN, which no
float64 -> float32 conversion produces) with guard elements behind the end, then again as column slabs of at most 2^24 pixels
(which the rest of the suite pins to the oracle) into buffers with another sentinel: the two must be equal bit for bit (so no
sentinel is left in either) and the guards untouched.  About 2000 pixels (corners, the last column, tile / slab / chunk seams,
the pixels at linear offsets 2^24, 2^30 and 2^31 - 1, random ones) are compared with the oracle, uint8 and float32 bit for bit.
Each case prints its time and the device memory in use at its peak."""
import os
import sys
import time

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import feature_scenes as fs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096                      # elements behind every buffer's end
SNAN_A, SNAN_B = 0x7FA00001, 0x7F800F0F   # signalling NaNs (quiet bit clear): never the result of a float64 -> float32 conversion
U8_A, U8_B = 0xA5, 0x5A
SLAB_PX = 1 << 24
GIB = 1 << 30
MAX_W, MAX_H = 2 ** 31 - 8, 2 ** 29 - 32
DEV = "cuda:0"

# A Lambert-shaded floor under most of the frame, three spheres, two lights: every pixel's float32 value depends on where it is.
SPHERES = np.array([[6.0, 8.0, 5.0], [-1.5, 1.0, 2.5], [-0.2, 0.3, 0.6], [0.8, 1.2, 0.5],
                    [220, 40, 60], [30, 200, 90], [70, 90, 230]], np.float32)
LIGHTS = np.array([[2.0, 5.0], [-3.0, 4.0], [5.0, 3.0]], np.float32)
PLANES = np.array([[0.0], [0.0], [-1.0], [0.0], [0.0], [1.0], [200.0], [180.0], [150.0]], np.float32)
CAM_O, CAM_R = np.zeros(3), np.eye(3)
SHADE = dict(amb=0.1, lamb=0.6, refl=0.35, depth=2)


def _raygen(w, h):
    """px, y0, dy, z0, dz: y from 2 to -2 across the columns, z from 0.2 to -1 down the rows (dz = 0 for h = 1: one row at -0.6)."""
    dy = -4.0 / (w - 1) if w > 1 else 0.0
    if h == 1:
        return (1.0, 2.0 if w > 1 else 0.3, dy, -0.6, 0.0)
    return (1.0, 2.0 if w > 1 else 0.3, dy, 0.2, -1.2 / (h - 1))


class _Case:
    """Timing and peak device memory of one case (printed at the end)."""

    def __init__(self, name):
        self.name, self.t0, self.peak = name, time.perf_counter(), 0

    def mark(self):
        free, total = torch.cuda.mem_get_info()
        self.peak = max(self.peak, total - free)

    def done(self):
        self.mark()
        print(f"\nCASE {self.name}: {time.perf_counter() - self.t0:.1f} s, peak device memory in use {self.peak / GIB:.1f} GiB",
              flush=True)


def _need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"needs {gib} GiB of free device memory, {free / GIB:.1f} GiB free on this shared device")


def _renderer(w, h, features=None):
    import python_ray_tracer_amd as pkg
    r = pkg.Renderer(0)
    if features is None:
        r.set_scene(SPHERES, LIGHTS, PLANES)
        r.set_camera(CAM_O, CAM_R)
    else:
        sc = features
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"], flags=int(sc["typed"]), materials=(sc["table"], sc["sid"], sc["pid"]),
                    light_radius=sc["radius"], shadow_samples=sc["n"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        r.set_lens(*sc["lens"])
    r.set_raygen(w, h, *(_raygen(w, h) if features is None else features["raygen"]))
    return r


def _params(r, aa=0, flags=0, features=None):
    if features is None:
        return r.params(SHADE["amb"], SHADE["lamb"], SHADE["refl"], SHADE["depth"], aa, flags)
    return r.params(7.0, -3.0, 2.0, features["depth"], aa, flags, seed=features["hseed"])


def _buffers(n, u8=True, f32=True, which="A"):
    b8 = torch.full((3 * n + GUARD,), U8_A if which == "A" else U8_B, dtype=torch.uint8, device=DEV) if u8 else None
    b32 = torch.full((3 * n + GUARD,), SNAN_A if which == "A" else SNAN_B, dtype=torch.int32, device=DEV) if f32 else None
    torch.cuda.synchronize()
    return b8, b32


def _guards_intact(n, b8, b32, which="A"):
    if b8 is not None:
        assert bool((b8[3 * n:] == (U8_A if which == "A" else U8_B)).all()), "uint8 guard overwritten"
    if b32 is not None:
        assert bool((b32[3 * n:] == (SNAN_A if which == "A" else SNAN_B)).all()), "float32 guard overwritten"


def _render_full(r, p, x0, x1, h, u8=True, f32=True):
    n = (x1 - x0) * h
    a8, a32 = _buffers(n, u8, f32, "A")
    r.render_device(p, x0, x1, a8.data_ptr() if u8 else None, a32.data_ptr() if f32 else None, plane_stride=n)
    r.sync()
    _guards_intact(n, a8, a32, "A")
    return a8, a32


def _same_as_slabs(r, p, x0, x1, h, a8, a32, case):
    """Columns [x0, x1) rendered again as column slabs of at most 2^24 pixels into buffers with the other sentinel: every slab
    equal to the full frame's columns, bit for bit (so neither holds a sentinel), the slab buffers' guards untouched."""
    n = (x1 - x0) * h
    cols = max(1, SLAB_PX // h)
    m_max = min(cols, x1 - x0) * h
    b8, b32 = _buffers(m_max, a8 is not None, a32 is not None, "B")
    case.mark()
    for sx0 in range(x0, x1, cols):
        sx1 = min(x1, sx0 + cols)
        m = (sx1 - sx0) * h
        if b8 is not None:
            b8.fill_(U8_B)
        if b32 is not None:
            b32.fill_(SNAN_B)
        torch.cuda.synchronize()
        r.render_device(p, sx0, sx1, b8.data_ptr() if b8 is not None else None, b32.data_ptr() if b32 is not None else None,
                        plane_stride=m)
        r.sync()
        o = (sx0 - x0) * h
        for c in range(3):
            if a8 is not None:
                assert torch.equal(a8[c * n + o:c * n + o + m], b8[c * m:(c + 1) * m]), f"uint8 plane {c}, slab [{sx0}, {sx1})"
            if a32 is not None:
                assert torch.equal(a32[c * n + o:c * n + o + m], b32[c * m:(c + 1) * m]), f"float32 plane {c}, slab [{sx0}, {sx1})"
        if b8 is not None:
            assert bool((b8[3 * m:] == U8_B).all()), f"slab [{sx0}, {sx1}): uint8 written past its end"
        if b32 is not None:
            assert bool((b32[3 * m:] == SNAN_B).all()), f"slab [{sx0}, {sx1}): float32 written past its end"
    if a32 is not None:   # (equal to slabs with another sentinel: none left; and a float32 value is never a signalling NaN)
        assert not bool((a32[:3 * n] == SNAN_A).any())


def _coords(w, h, x0, x1, seed, n_random=1500):
    """(k, 2) pixels of [x0, x1) x [0, h): corners, the last column, tile / slab / dispatch-slab / chunk seams, linear offsets
    2^24, 2^30 and 2^31 - 1 where the range has them, random pixels."""
    rng = np.random.default_rng(seed)
    n = (x1 - x0) * h
    xs, ys = [x0, x0, x1 - 1, x1 - 1], [0, h - 1, 0, h - 1]
    for y in np.linspace(0, h - 1, min(h, 64)).astype(np.int64):          # the last column
        xs.append(x1 - 1); ys.append(int(y))
    seams = set()
    for k in rng.integers(0, max(1, (x1 - x0) // 8), 64):                  # tile seams in x
        seams.update((x0 + 8 * int(k) - 1, x0 + 8 * int(k)))
    cols = max(1, SLAB_PX // h)                                           # the slabs of _same_as_slabs
    seams.update(s for sx in range(x0 + cols, x1, cols) for s in (sx - 1, sx))
    tiles_y = (h + 7) // 8
    for wpw in (2, 4):                                                    # dispatch() column slabs (rt_geometry.h)
        max_cols = ((2 ** 32 - 1) // (64 * wpw)) * wpw // tiles_y
        tx = ((x1 - x0) + 7) // 8
        if tx * tiles_y > ((2 ** 32 - 1) // (64 * wpw)) * wpw:
            ns = -(-tx // max_cols)
            st = -(-tx // ns)
            seams.update(s for k in range(1, ns) for s in (x0 + 8 * st * k - 1, x0 + 8 * st * k))
    tiles = ((x1 - x0) + 7) // 8                                          # rt_render's chunk edges (four chunks)
    for c in range(1, 4):
        cx = x0 + (tiles * (2 * c - 1) // 6) * 8
        seams.update((cx - 1, cx))
    for x in sorted(s for s in seams if x0 <= s < x1)[:400]:
        for y in {0, h - 1, int(rng.integers(0, h)), min(h - 1, 8 * int(rng.integers(0, tiles_y)))}:
            xs.append(x); ys.append(y)
    for y in rng.integers(0, tiles_y, 64):                                # tile seams in y
        for yy in (8 * int(y) - 1, 8 * int(y)):
            if 0 <= yy < h:
                xs.append(int(rng.integers(x0, x1))); ys.append(yy)
    for off in (2 ** 24, 2 ** 30, 2 ** 31 - 1, n - 1):
        if off < n:
            xs.append(x0 + off // h); ys.append(off % h)
    xs += list(rng.integers(x0, x1, n_random)); ys += list(rng.integers(0, h, n_random))
    co = np.stack([np.asarray(xs, np.int64), np.asarray(ys, np.int64)], axis=1)
    return np.unique(co, axis=0)


def _same_as_oracle(oracle, what, w, h, x0, x1, co, a8, a32, aa=0, features=None):
    """The sampled pixels of the device frame (gathered on the device) against orc.render_pixels, bit for bit."""
    n = (x1 - x0) * h
    off = torch.as_tensor((co[:, 0] - x0) * h + co[:, 1], dtype=torch.int64, device=DEV)
    idx = torch.stack([off + c * n for c in range(3)], dim=1)
    if features is None:
        r8, r64 = oracle.render_pixels(w, h, co, CAM_O, CAM_R, SPHERES, LIGHTS, PLANES, SHADE["amb"], SHADE["lamb"], SHADE["refl"],
                                       SHADE["depth"], aa, raygen=_raygen(w, h))
    else:
        r8, r64 = oracle.render_pixels(w, h, co, features["cam_origin"], features["cam_rot"], features["spheres"], features["lights"],
                                       features["planes"], 0.0, 0.0, 0.0, features["depth"], aa, **fs.oracle_kwargs(features))
    bad = np.zeros(len(co), bool)
    if a8 is not None:
        bad |= (a8[idx].cpu().numpy() != r8).any(axis=1)
    if a32 is not None:
        bad |= (a32[idx].cpu().numpy().view(np.uint32) != r64.astype(np.float32).view(np.uint32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(co)} pixels differ from the oracle, e.g. {co[bad][:4].tolist()}"
    assert len(np.unique(r8, axis=0)) > 8, f"{what}: the sampled pixels are nearly uniform"


def _full_frame_case(oracle, name, w, h, aa=0, u8=True, f32=True, gib=40, seed=1):
    _need(gib)
    case = _Case(name)
    with _renderer(w, h) as r:
        p = _params(r, aa)
        a8, a32 = _render_full(r, p, 0, w, h, u8, f32)
        case.mark()
        _same_as_slabs(r, p, 0, w, h, a8, a32, case)
        _same_as_oracle(oracle, name, w, h, 0, w, _coords(w, h, 0, w, seed), a8, a32, aa)
    del a8, a32
    torch.cuda.empty_cache()
    case.done()


# ---------------------------------------------------------------------------------------------------------------------
def test_frame_of_2_31_pixels(oracle):
    """65536 x 32768 = 2^31 pixels, aa 0: the parked offset reaches 2^31 - 1, 2^25 tiles, no scheduler feedback."""
    _full_frame_case(oracle, "65536 x 32768 (2^31 px), aa 0, u8 + f32", 65536, 32768, gib=40)


@pytest.mark.parametrize("side", [23170, 23171])
def test_lattice_switch(oracle, side):
    """RT_AA_REFERENCE at 23170^2 ((2w-1)(2h-1) just below 2^31: the half-pixel lattice, 51 GB of float64 samples) and 23171^2
    (just above: nine taps per pixel), full frame and slabs."""
    lattice = (2 * side - 1) ** 2 < 2 ** 31
    _full_frame_case(oracle, f"{side}^2 RT_AA_REFERENCE ({'lattice' if lattice else 'nine taps'})", side, side, aa=1,
                     gib=64 if lattice else 12, seed=side)


@pytest.mark.parametrize("w,h", [(2 ** 29 + 8, 2), (2 ** 30, 2), (2 ** 29 + 8, 1), (MAX_W, 1),
                                 (2, 2 ** 28 + 8), (2, MAX_H), (1, MAX_H)])
def test_thin_frames(oracle, w, h):
    """Frames one or two pixels thin: 8x padding makes a single frame more work-items than one dispatch holds (the library
    sends it as column slabs), tiles_x near 2^28; the transposes, up to the tallest frame accepted (one tile column of
    2^26 - 4 tiles); h = 1 with dz = 0."""
    _full_frame_case(oracle, f"{w} x {h} (thin), aa 0, u8 + f32", w, h, gib=40, seed=w + h)


def test_frame_limits_are_refused():
    """Sides beyond rt_geometry.h's limits and more than 2^31 pixels: RT_ERR_BAD_ARG from the library (called directly) and
    ValueError from Renderer; the previous grid stays."""
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib
    with _renderer(64, 32) as r:
        for w, h in [(MAX_W + 1, 1), (2 ** 31 - 1, 1), (1, MAX_H + 1), (2, 2 ** 29 + 8), (65536, 32769), (2 ** 30 + 1, 2)]:
            assert r._lib.rt_set_raygen(r._ctx, w, h, *_raygen(64, 32)) == _lib.RT_ERR_BAD_ARG, (w, h)
            with pytest.raises(ValueError):
                r.set_raygen(w, h, *_raygen(64, 32))
        u8, _ = r.render(SHADE["amb"], SHADE["lamb"], SHADE["refl"], SHADE["depth"])
        assert u8.shape == (3, 64, 32)
    assert pkg.Renderer is not None


def test_sequence_8_frames_of_2_29_pixels():
    """rt_render_sequence, 8 frames of 32768 x 16384 (u8) at the default frames_per_launch: 2^32 work-items in one launch
    (the library dispatches 7 + 1); frame 0 equals one rt_render_device, every later frame frame 0."""
    _sequence_case("8 x 2^29 px sequence, default frames_per_launch", 32768, 16384, 8, 0, gib=24)


def test_sequence_131_frames_8k():
    """131 frames of 7680 x 4320 at frames_per_launch = 131: 4.35e9 work-items in one launch (the library dispatches 129 + 2)."""
    _sequence_case("131 x 7680 x 4320 sequence, frames_per_launch 131", 7680, 4320, 131, 131, gib=24)


def _sequence_case(name, w, h, n, fpl, gib):
    _need(gib)
    case = _Case(name)
    with _renderer(w, h) as r:
        p = _params(r)
        npx = w * h
        seq = torch.full((3 * npx * n + GUARD,), U8_A, dtype=torch.uint8, device=DEV)
        one, _ = _buffers(npx, True, False, "B")
        r.render_sequence(p, 0, w, n, d_u8=seq.data_ptr(), frames_per_launch=fpl)
        r.render_device(p, 0, w, one.data_ptr(), None)
        r.sync()
        case.mark()
        assert bool((seq[3 * npx * n:] == U8_A).all()), "sequence guard overwritten"
        _guards_intact(npx, one, None, "B")
        f0 = seq[:3 * npx]
        assert torch.equal(f0, one[:3 * npx]), "frame 0 of the sequence differs from rt_render_device"
        for i in range(1, n):
            assert torch.equal(seq[3 * npx * i:3 * npx * (i + 1)], f0), f"frame {i} differs from frame 0"
    del seq, one
    torch.cuda.empty_cache()
    case.done()


def _host_compare(host, a, x0, x1, h, hwc=False):
    """Host frame (3, w, h) planar, or (h, w, 3) with hwc, against the device frame a (planar, flat) in column blocks."""
    n = (x1 - x0) * h
    cols = max(1, SLAB_PX // h)
    for sx0 in range(0, x1 - x0, cols):
        sx1 = min(x1 - x0, sx0 + cols)
        for c in range(3):
            d = a[c * n + sx0 * h:c * n + sx1 * h]
            if hwc:
                assert np.array_equal(host[:, sx0:sx1, c], d.view(sx1 - sx0, h).t().cpu().numpy()), f"channel {c}, columns [{sx0}, {sx1})"
            else:
                assert np.array_equal(host[c, sx0:sx1].reshape(-1), d.cpu().numpy()), f"plane {c}, columns [{sx0}, {sx1})"


@pytest.mark.parametrize("pinned", [False, True])
def test_rt_render_f32_over_2_29_pixels(oracle, pinned):
    """rt_render (chunks, copies to the host) of float32 at 16392 x 32768 = 2^29 + 2^18 pixels: plane pitch 2^31 + 2^20 bytes
    (plane-by-plane copies), into pageable and page-locked memory; equal to the device frame, no sentinel left."""
    w, h = 16392, 32768
    _need(16)
    case = _Case(f"rt_render f32 {w} x {h} to {'rt_host_alloc' if pinned else 'pageable'} memory")
    with _renderer(w, h) as r:
        out = r.host_array((3, w, h), np.float32) if pinned else np.empty((3, w, h), np.float32)
        try:
            out.view(np.uint32).fill(SNAN_A)
            r.render_into(SHADE["amb"], SHADE["lamb"], SHADE["refl"], SHADE["depth"], 0, None, out)
            case.mark()
            _, a32 = _render_full(r, _params(r), 0, w, h, u8=False, f32=True)
            _host_compare(out.view(np.int32), a32, 0, w, h)
            co = _coords(w, h, 0, w, 7, n_random=500)
            _same_as_oracle(oracle, "rt_render f32", w, h, 0, w, co, None, a32)
        finally:
            if pinned:
                r.release_host_array(out)
            del out
    torch.cuda.empty_cache()
    case.done()


@pytest.mark.parametrize("hwc", [False, True])
def test_rt_render_u8_2_31_pixels(oracle, hwc):
    """rt_render of uint8 at 65536 x 32768 = 2^31 pixels: planar into pageable memory (plane pitch 2^31 bytes: plane-by-plane
    copies), RT_FLAG_U8_HWC into page-locked memory (one launch, one 6 GiB copy); equal to the device frame."""
    from python_ray_tracer_amd import _lib
    w, h = 65536, 32768
    _need(16)
    case = _Case(f"rt_render u8 {'HWC to rt_host_alloc' if hwc else 'planar to pageable'} {w} x {h}")
    with _renderer(w, h) as r:
        shape = (h, w, 3) if hwc else (3, w, h)
        out = r.host_array(shape, np.uint8) if hwc else np.empty(shape, np.uint8)
        try:
            out.fill(U8_B)
            r.render_into(SHADE["amb"], SHADE["lamb"], SHADE["refl"], SHADE["depth"], 0, out,
                          flags=_lib.RT_FLAG_U8_HWC if hwc else 0)
            case.mark()
            a8, _ = _render_full(r, _params(r), 0, w, h, u8=True, f32=False)
            _host_compare(out, a8, 0, w, h, hwc=hwc)
        finally:
            if hwc:
                r.release_host_array(out)
            del out
    torch.cuda.empty_cache()
    case.done()


@pytest.mark.parametrize("w,h", [(MAX_W, 1), (2 ** 30, 2), (65536, 32768)])
def test_feature_slab_at_the_right_edge(oracle, w, h):
    """Columns [w - 13, w) with every feature (a lens, area lights, rough and glass rows), every pixel against the oracle: the
    slab offsets and the hash keys X = 2x at x near 2^31 (X near 2^32).  (Scene 2 of tools/feature_scenes.py: on these slabs
    every pixel changes with the lens, the rough rows and the area lights.)"""
    sc = fs.draw(2, w=48, h=32)
    sc.update(w=w, h=h, raygen=_raygen(w, h), depth=2)
    case = _Case(f"feature slab [w - 13, w) of {w} x {h}")
    x0, x1 = w - 13, w
    with _renderer(w, h, features=sc) as r:
        for aa in (0, 1):
            p = _params(r, aa, features=sc)
            a8, a32 = _render_full(r, p, x0, x1, h)
            xs, ys = np.meshgrid(np.arange(x0, x1), np.arange(h), indexing="ij")
            co = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)
            if len(co) > 3000:
                co = co[np.random.default_rng(aa).choice(len(co), 3000, replace=False)]
            r8, r64 = oracle.render_pixels(w, h, co, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"],
                                           0.0, 0.0, 0.0, sc["depth"], aa, **fs.oracle_kwargs(sc))
            n = (x1 - x0) * h
            off = torch.as_tensor((co[:, 0] - x0) * h + co[:, 1], dtype=torch.int64, device=DEV)
            idx = torch.stack([off + c * n for c in range(3)], dim=1)
            g8, g32 = a8[idx].cpu().numpy(), a32[idx].cpu().numpy().view(np.uint32)
            bad = (g8 != r8).any(axis=1) | (g32 != r64.astype(np.float32).view(np.uint32)).any(axis=1)
            assert not bad.any(), f"aa {aa}: {int(bad.sum())} of {len(co)} pixels differ, e.g. {co[bad][:4].tolist()}"
            if aa == 0:                                                       # the lens keys are live here
                s2 = fs.strip(dict(sc), "lens")
                n8, _ = oracle.render_pixels(w, h, co, s2["cam_origin"], s2["cam_rot"], s2["spheres"], s2["lights"], s2["planes"],
                                             0.0, 0.0, 0.0, s2["depth"], aa, **fs.oracle_kwargs(s2))
                assert (n8 != r8).any(axis=1).sum() >= len(co) // 2
    case.done()
