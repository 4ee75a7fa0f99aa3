"""tests/output_layouts.py held to itself, without a GPU: what tests/test_gpu_output_layouts.py compares the render kernels' stores
with must see a store that is wrong.
  * classify against a map of the allocation painted forwards, element by element, for every layout, slab and frame count;
  * teeth: a second statement of the addressing with one term wrong at a time (planes 1 and 2 swapped, every pixel one element
    later, a stride or the frame stride off by one, the slab one column to the left, h and x1-x0 exchanged in the HWC index) and
    single bytes in every kind of pad and in both guard bands: the whole-buffer comparison fails and names the place;
  * a frame that equals the sentinels inside the slab passes: the comparison is with `expected`, not with "changed";
  * the HWC rule against viewer.frame_to_hwc, which states it independently;
  * the oracle's frames of every variant are informative: at least 100 distinct colours and at least 40 pixels whose planes 1 and
    2 differ, or a G/B swap or a shifted pixel could go unseen."""
import numpy as np
import pytest

import output_layouts as ol
from output_layouts import H, LAYOUTS, SLABS, W

CASES = [(layout, x0, x1, n) for layout in LAYOUTS for x0, x1 in SLABS for n in (1, ol.N_SEQ)]


def _frame(seed=0):
    """A random frame: every byte value, and float32 words with both zeros among them."""
    rng = np.random.default_rng(seed)
    ref8 = rng.integers(0, 256, (3, W, H)).astype(np.uint8)
    ref32 = rng.uniform(-40.0, 300.0, (3, W, H)).astype(np.float32)
    ref32[0, 4, 5], ref32[1, 17, 0] = 0.0, -0.0
    return ref8, ref32


def _paint(layout, x0, x1, n):
    """The place of every element of the allocation, painted forwards: the bands by their slices, between the frames by what no
    frame owns, the frame's own columns element by element by the addressing rule, and what is left inside a frame is the pad its
    layout has (in-place layouts have none: their strides are the full frame's)."""
    g, ly = ol.geometry(layout, W, H, x0, x1, n), LAYOUTS[layout]
    label = np.full(g.total, "pad between frames", dtype=object)
    label[:g.guard] = "front guard band"
    label[g.total - g.guard:] = "rear guard band"
    start = g.guard                                           # of frame 0: the base less the in-place offset of column x0
    for i in range(n):
        f0 = start + i * g.frame_stride
        label[f0:f0 + g.extent] = "pad between rows" if g.hwc else "pad between planes"
        lo, hi = (0, W) if ly.strides == "inplace" else (x0, x1)
        for x in range(lo, hi):
            for y in range(H):
                for c in range(3):
                    if ly.strides == "inplace":
                        at = (y * g.stride + x) * 3 + c if g.hwc else c * g.stride + x * H + y
                    else:
                        at = (y * g.stride + (x - x0)) * 3 + c if g.hwc else c * g.stride + (x - x0) * H + y
                    label[f0 + at] = "pixel" if x0 <= x < x1 else "column outside the slab"
    return g, label


_PAINTED = {}


def _painted(layout, x0, x1, n):
    if (layout, x0, x1, n) not in _PAINTED:
        _PAINTED[layout, x0, x1, n] = _paint(layout, x0, x1, n)
    return _PAINTED[layout, x0, x1, n]


def test_the_flags_are_the_headers():
    from python_ray_tracer_amd import _lib as L
    assert (ol.U8_RGB, ol.U8_HWC, ol.COUNT_RAYS, ol.AA_PER_PIXEL) == (L.RT_FLAG_U8_RGB, L.RT_FLAG_U8_HWC, L.RT_FLAG_COUNT_RAYS, L.RT_FLAG_AA_PER_PIXEL)


def test_the_sentinels_depend_on_the_position():
    a, b = ol.sentinel_u8(4000), ol.sentinel_f32(4000)
    assert a.dtype == np.uint8 and a[0] == 89 and a[1] == 220 and a[2] == (2 * 131 + 89) & 0xff and len(set(a[:256].tolist())) == 256
    assert b.dtype == np.uint32 and b[0] == 0x7fc00000 and b[3999] == 0x7fc00000 + 3999 and np.isnan(b.view(np.float32)).all()
    for k in (1, 13, 21, 273):                                 # a block moved by a row, a column or a plane is not the same block
        assert (a[k:] != a[:-k]).all() and (b[k:] != b[:-k]).all()


@pytest.mark.parametrize("layout,x0,x1,n", CASES)
def test_classify_is_the_painted_map(layout, x0, x1, n):
    g, label = _painted(layout, x0, x1, n)
    got = np.array([ol.classify(i, layout, W, H, x0, x1, n) for i in range(g.total)], dtype=object)
    bad = np.flatnonzero(got != label)
    assert not bad.size, (layout, x0, x1, n, [(int(i), got[i], label[i]) for i in bad[:4]])
    assert set(label) <= set(ol.PLACES) and (label == "pixel").sum() == 3 * (x1 - x0) * H * n
    # every pad the layout's strides make is there to be written to
    ly = LAYOUTS[layout]
    want = {"pixel", "front guard band", "rear guard band"} | ({"pad between frames"} if n > 1 else set())
    if ly.strides == "pad":
        want.add("pad between rows" if g.hwc else "pad between planes")
    if ly.strides == "inplace" and x1 - x0 < W:
        want.add("column outside the slab")
    assert set(label) == want, (layout, x0, x1, n, set(label))


@pytest.mark.parametrize("layout,x0,x1,n", CASES)
def test_the_strides_and_the_bands(layout, x0, x1, n):
    """The strides are the table's, a sequence's frame stride the smallest the entry accepts plus 7, and the bands hold a store one
    stride or one frame too far, in front and behind, and a planar one displaced by all it may add."""
    g, ly = ol.geometry(layout, W, H, x0, x1, n), LAYOUTS[layout]
    ws = x1 - x0
    compact = ws if g.hwc else ws * H
    assert g.stride == {"compact": compact, "pad": compact + (3 if g.hwc else 5), "inplace": W if g.hwc else W * H}[ly.strides]
    assert g.base - g.guard == {"compact": 0, "pad": 0, "inplace": 3 * x0 if g.hwc else x0 * H}[ly.strides]
    least = 3 * g.stride * H if g.hwc else 3 * g.stride        # rt_launch.h: check_device_outputs
    assert g.frame_stride == (least + 7 if n > 1 else 0) and g.guard >= 3 * W * H
    _, label = _painted(layout, x0, x1, n)
    px = np.flatnonzero(label == "pixel")
    far = max(g.frame_stride, 3 * g.stride if g.hwc else g.stride, 0 if g.hwc else 2 * g.stride + ws * H)
    assert px[0] - far >= 0 and px[-1] + far < g.total, (layout, x0, x1, n, g)


def _mutant(layout, ref8, ref32, x0, x1, n, *, swap=False, later=0, dstride=0, dframe=0, left=0, exchange=False):
    """`expected` said again with one term wrong: the teeth tests' stand-in for a kernel that stores to the wrong place."""
    g, ly = ol.geometry(layout, W, H, x0, x1, n), LAYOUTS[layout]
    ws, stride, fs = x1 - x0, g.stride + dstride, g.frame_stride + dframe
    out = []
    for which, src, fill in (("u8", ref8[[0, 2, 1]] if ly.flags & ol.U8_RGB else ref8, ol.sentinel_u8),
                             ("f32", ref32.view(np.uint32), ol.sentinel_f32)):
        if which not in ly.outputs:
            out.append(None)
            continue
        if swap:
            src = src[[0, 2, 1]]
        buf = fill(g.total)
        for i in range(n):
            for c in range(3):
                for x in range(ws):
                    for y in range(H):
                        off = (x - left) * H + y
                        if g.hwc:
                            xr, yy = (off // ws, off - (off // ws) * ws) if exchange else (x - left, y)
                            at = (yy * stride + xr) * 3 + c
                        else:
                            at = c * stride + off
                        buf[g.base + i * fs + at + later] = src[c, x0 + x, y]
        out.append(buf)
    return out


def _bites(layout, x0, x1, n, what, **mutation):
    """The mutant's buffers differ from `expected`, the message names the layout and the places, and the places are the painted
    map's at the elements that differ.  -> the places of the uint8 or, where the layout has none, the float32 buffer."""
    ref8, ref32 = _frame()
    _, label = _painted(layout, x0, x1, n)
    first = None
    for want, got in zip(ol.expected(layout, ref8, ref32, W, H, x0, x1, n), _mutant(layout, ref8, ref32, x0, x1, n, **mutation)):
        if want is None:
            continue
        msg = ol.mismatch(got, want, what, layout, W, H, x0, x1, n)
        assert msg is not None, (what, layout, x0, x1, n)
        where = ol.places(got, want, layout, W, H, x0, x1, n)
        truth = {p: int((label[np.flatnonzero(got != want)] == p).sum()) for p in where}
        assert dict(where) == truth and what in msg and f"layout {layout}," in msg and all(p in msg for p in where), msg
        bad = np.flatnonzero(got != want)[:4]
        assert all(f"{int(i)} (base{int(i) - ol.geometry(layout, W, H, x0, x1, n).base:+d}: {label[i]}" in msg for i in bad), msg
        first = where if first is None else first
    return first


@pytest.mark.parametrize("layout,x0,x1,n", CASES)
def test_teeth_planes_swapped(layout, x0, x1, n):
    assert set(_bites(layout, x0, x1, n, "planes 1 and 2 swapped", swap=True)) == {"pixel"}


@pytest.mark.parametrize("layout,x0,x1,n", CASES)
def test_teeth_every_pixel_one_element_later(layout, x0, x1, n):
    where = _bites(layout, x0, x1, n, "one element later", later=1)
    _, label = _painted(layout, x0, x1, n)
    behind = label[np.flatnonzero(label == "pixel")[-1] + 1]     # the element behind the last pixel is no pixel, and is written
    assert "pixel" in where and behind != "pixel" and behind in where, (where, behind)


@pytest.mark.parametrize("layout,x0,x1,n", CASES)
def test_teeth_stride_off_by_one(layout, x0, x1, n):
    where = _bites(layout, x0, x1, n, "stride + 1", dstride=1)
    assert "pixel" in where and set(where) - {"pixel"}, where    # plane 2 (the last row) ends two (three) elements behind its place


@pytest.mark.parametrize("layout,x0,x1", [c[:3] for c in CASES if c[3] > 1])
def test_teeth_frame_stride_off_by_one(layout, x0, x1):
    where = _bites(layout, x0, x1, ol.N_SEQ, "frame_stride + 1", dframe=1)
    assert "pixel" in where and set(where) - {"pixel"}, where


@pytest.mark.parametrize("layout,x0,x1,n", CASES)
def test_teeth_slab_one_column_to_the_left(layout, x0, x1, n):
    where = _bites(layout, x0, x1, n, "one column to the left", left=1)
    inplace = LAYOUTS[layout].strides == "inplace"
    assert ("column outside the slab" if inplace and x0 > 0 else "front guard band") in where, where


@pytest.mark.parametrize("layout,x0,x1,n", [c for c in CASES if LAYOUTS[c[0]].flags & ol.U8_HWC])
def test_teeth_h_and_width_exchanged_in_the_hwc_index(layout, x0, x1, n):
    """off / ws for off / h.  One case is no mutation: in a compact image one pixel wide (pitch 1) the row is `off` either way, and
    the case says so; the same slab at the pitches of hwc_pitch and hwc_inplace, and every wider slab, catch it."""
    if x1 - x0 == 1 and LAYOUTS[layout].strides == "compact":
        ref8, ref32 = _frame()
        assert np.array_equal(_mutant(layout, ref8, ref32, x0, x1, n, exchange=True)[0], ol.expected(layout, ref8, ref32, W, H, x0, x1, n)[0])
        return
    assert "pixel" in _bites(layout, x0, x1, n, "h and x1-x0 exchanged", exchange=True)


@pytest.mark.parametrize("layout,x0,x1,n", CASES)
def test_teeth_one_byte_in_every_pad_and_band(layout, x0, x1, n):
    ref8, ref32 = _frame()
    g, label = _painted(layout, x0, x1, n)
    for want in ol.expected(layout, ref8, ref32, W, H, x0, x1, n):
        if want is None:
            continue
        for place in sorted(set(label) - {"pixel"}):
            at = np.flatnonzero(label == place)
            for i in (at[0], at[-1], at[len(at) // 2]):            # the first, the last and one between
                got = want.copy()
                got[i] ^= 1
                msg = ol.mismatch(got, want, "one element", layout, W, H, x0, x1, n)
                assert msg is not None and ol.places(got, want, layout, W, H, x0, x1, n) == {place: 1}, (place, int(i), msg)
                assert f"{{'{place}': 1}}" in msg and f"{int(i)} (base{int(i) - g.base:+d}: {place}" in msg, msg


@pytest.mark.parametrize("layout,x0,x1,n", CASES)
def test_unmutated_buffers_pass_whatever_the_frame_holds(layout, x0, x1, n):
    """`expected` against itself, and a frame that equals the sentinels inside the slab: nothing in the allocation changes, and the
    comparison passes.  (Where each element of the frame lands is read from two placements of its own index, low byte and high.)"""
    ref8, ref32 = _frame()
    for a, b in zip(ol.expected(layout, ref8, ref32, W, H, x0, x1, n), ol.expected(layout, ref8.copy(), ref32.copy(), W, H, x0, x1, n)):
        assert a is None or ol.mismatch(a, b, "unmutated", layout, W, H, x0, x1, n) is None
    if n > 1 or "u8" not in LAYOUTS[layout].outputs:             # (frames of a sequence are one frame n times: they cannot all be the sentinels)
        return
    g, label = _painted(layout, x0, x1, n)
    ident = np.arange(3 * W * H).reshape(3, W, H)
    lo = ol.expected(layout, (ident & 0xff).astype(np.uint8), ref32, W, H, x0, x1)[0]
    hi = ol.expected(layout, (ident >> 8).astype(np.uint8), ref32, W, H, x0, x1)[0]
    at = np.flatnonzero(label == "pixel")
    k = lo[at].astype(np.int64) | (hi[at].astype(np.int64) << 8)
    assert len(set(k.tolist())) == at.size == 3 * (x1 - x0) * H
    same = ref8.copy()
    same.reshape(-1)[k] = ol.sentinel_u8(g.total)[at]
    want = ol.expected(layout, same, ref32, W, H, x0, x1)[0]
    assert np.array_equal(want, ol.sentinel_u8(g.total))         # the rendered buffer would be the untouched one
    assert ol.mismatch(ol.sentinel_u8(g.total), want, "sentinel frame", layout, W, H, x0, x1) is None
    other = ol.expected(layout, ref8, ref32, W, H, x0, x1)[0]
    assert ol.mismatch(ol.sentinel_u8(g.total), other, "untouched", layout, W, H, x0, x1) is not None   # and an unrendered one fails


def test_hwc_is_the_viewers_image():
    from python_ray_tracer_amd.viewer import frame_to_hwc
    planar, _ = _frame(3)
    for layout, undo in (("hwc", False), ("hwc_rgb_inplace", True)):
        g = ol.geometry(layout, W, H, 0, W)
        assert g.stride == W and g.base == g.guard                # pitch x1-x0 over the full frame
        img = ol.expected(layout, planar, None, W, H, 0, W)[0][g.base:g.base + 3 * W * H].reshape(H, W, 3)
        assert np.array_equal(img, frame_to_hwc(planar, undo_swap=undo)), layout
    part = ol.expected("hwc", planar, None, W, H, 3, 18)[0]
    g = ol.geometry("hwc", W, H, 3, 18)
    assert np.array_equal(part[g.base:g.base + 3 * 15 * H].reshape(H, 15, 3), frame_to_hwc(planar)[:, 3:18])


def _informative(u8):
    return len(np.unique(u8.reshape(3, -1).T, axis=0)), int((u8[1] != u8[2]).sum())


@pytest.mark.parametrize("name", list(ol.VARIANTS))
def test_reference_frames_are_informative(oracle, name):
    u8, f32 = ol.reference(oracle, name)
    colours, differ = _informative(u8)
    print(f"{name}: {colours} distinct colours, {differ} pixels with plane 1 != plane 2")
    assert u8.shape == f32.shape == (3, W, H) and colours >= 100 and differ >= 40, (name, colours, differ)
    if ol.keyed(name):                                            # a slab through the oracle's x0, x1 is the frame's columns
        for x0, x1 in SLABS[1:]:
            s8, s32 = ol.reference(oracle, name, x0, x1)
            assert np.array_equal(s8[:, x0:x1], u8[:, x0:x1]) and s32[:, x0:x1].tobytes() == f32[:, x0:x1].tobytes(), (name, x0, x1)
            assert not s8[:, :x0].any() and not s8[:, x1:].any()


def test_the_sky_seed_is_the_first_that_serves(oracle):
    """SKY_SEED: the first seed of draw_lit whose scene is of family SKY_LENS_SOFT (rt_plan.h: family_of: a sky with a colour that
    is not zero, a lens aperture > 0, a light radius > 0) and whose frame meets the bounds."""
    from feature_gpu import fs
    for seed in range(ol.SKY_SEED + 1):
        sc = fs.draw_lit(seed, w=W, h=H)
        family = sc["sky"] is not None and np.asarray(sc["sky"])[3:12].any() and sc["lens"][0] > 0.0 and float(np.max(sc["radius"])) > 0.0
        u8 = fs.oracle_frame(oracle, {**sc, "depth": ol.DEPTH, "aa": 0, "flags_aa": 0})[0]
        colours, differ = _informative(u8)
        serves = bool(family) and colours >= 100 and differ >= 40
        assert serves == (seed == ol.SKY_SEED), (seed, family, colours, differ)
    assert np.array_equal(u8, ol.reference(oracle, "sky_lens_soft")[0])
