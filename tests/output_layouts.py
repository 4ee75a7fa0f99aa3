"""Where the render kernels put their pixels (no tests here: tests/test_output_layouts.py holds this module to itself on the CPU,
tests/test_gpu_output_layouts.py renders into what it describes).  rt_device.h's store_pixel and the offsets around it (`off`, `fo`,
rt_launch.h's frame_params and slab_params, aa_resolve_kernel's `idx`) against the addressing rule of include/mi355rt.h, restated
here in numpy index arithmetic:
    planar   element [c, x, y] at base + c*plane_stride + (x-x0)*h + y
    HWC      byte c of pixel (x, y) at base + (y*pitch + (x-x0))*3 + c
    frame i of a sequence at + i*frame_stride

sentinel_u8, sentinel_f32   what every output buffer holds before a launch: values that depend on the position
LAYOUTS, geometry           the ways a caller lays a slab out, and the strides, offsets and sizes of one of them
expected                    the sentinel-filled allocation with the oracle's pixels where the rule puts them: nothing else
classify, mismatch          where a differing element lies, and the failure message that says so
VARIANTS, scene_of, reference   the scenes, knobs and modes whose kernels between them hold every form of the store, what
                            MI355RT_LOG_KERNELS must name for each, and the oracle's frames of them

Every buffer carries a guard band in front of the first frame and one behind the last: a store that lands a stride or a frame too
far lands in a band, inside the allocation, where the comparison (over the whole allocation) sees it.  A band is one whole frame,
3*w*h elements, and wider where a layout's strides ask for it (geometry)."""
import collections

import numpy as np

from conftest import load_frame, raygen_closed_form

W, H = 21, 13                                  # 3 x 2 tiles of 8 x 8, part tiles in both directions, w != h, h odd
SLABS = ((0, 21), (3, 18), (17, 18))           # the frame, an interior slab that starts and ends inside tiles, one column
U8_RGB, U8_HWC, COUNT_RAYS, AA_PER_PIXEL = 2, 8, 16, 32    # RT_FLAG_* of include/mi355rt.h (test_output_layouts.py compares them)
N_SEQ, FRAMES_PER_LAUNCH = 3, 2                # a sequence: one launch of two frames and one of a single frame
DEPTH = 2


def sentinel_u8(n):
    return ((131 * np.arange(n, dtype=np.int64) + 89) & 0xff).astype(np.uint8)


def sentinel_f32(n):
    """uint32 words: quiet NaNs whose payload is the position.  float32 buffers are compared as these words, never as floats."""
    return (0x7fc00000 | (np.arange(n, dtype=np.int64) & 0x3fffff)).astype(np.uint32)


# name: (outputs, flags, how the strides are formed)
Layout = collections.namedtuple("Layout", "outputs flags strides")
LAYOUTS = {
    "planar_both":     Layout(("u8", "f32"), 0, "compact"),
    "planar_u8":       Layout(("u8",), 0, "compact"),
    "planar_f32":      Layout(("f32",), 0, "compact"),
    "planar_pad":      Layout(("u8", "f32"), 0, "pad"),            # plane_stride = (x1-x0)*h + 5
    "planar_inplace":  Layout(("u8", "f32"), 0, "inplace"),        # plane_stride = w*h, base at column x0
    "rgb_both":        Layout(("u8", "f32"), U8_RGB, "compact"),   # (float32 unchanged by the flag)
    "hwc":             Layout(("u8",), U8_HWC, "compact"),         # pitch x1-x0
    "hwc_pitch":       Layout(("u8",), U8_HWC, "pad"),             # pitch x1-x0+3
    "hwc_inplace":     Layout(("u8",), U8_HWC, "inplace"),         # pitch w, base + 3*x0
    "hwc_rgb_inplace": Layout(("u8",), U8_HWC | U8_RGB, "inplace"),
}
SEQUENCE_LAYOUTS = ("planar_inplace", "planar_u8", "hwc_inplace", "hwc_pitch")
HOST_LAYOUTS = ("planar_both", "planar_u8", "planar_f32", "rgb_both", "hwc")     # compact: host buffers have no strides

# stride: plane_stride, or the row pitch in pixels under HWC.  base: index of the launch's base pointer in the allocation.
# extent: elements from the first frame's start to the end of what one frame owns.  frame_stride: 0 for a single frame.
Geometry = collections.namedtuple("Geometry", "hwc stride base extent frame_stride n guard total w h x0 x1")


def geometry(layout, w, h, x0, x1, n_frames=1):
    """The strides a caller passes for `layout` and the allocation around them.  A sequence's frame_stride is the smallest the entry
    accepts (3*plane_stride; 3*pitch*h under HWC) plus 7.
    The guard bands: 3*w*h elements, which hold a store one plane_stride (at most w*h + 5) or one row pitch too far.  Two cases need
    more, and get it: a store a whole frame too far needs frame_stride elements behind the last frame (frame_stride is the least
    plus 7: hwc_pitch's is 943 against 819), and a planar store displaced by all it may add, 2*plane_stride + (x1-x0)*h, needs that
    (planar_pad's full slab: 829 against 819).  What a kernel does with a term of store_pixel dropped stays inside too: without
    `+ fo` every frame lands on frame 0, with the two plane steps exchanged the same addresses take each other's values, and
    without the `* 3` of the HWC address a pixel's three bytes start at base + y*pitch + (x-x0), below where they belong."""
    ly = LAYOUTS[layout]
    hwc, ws = bool(ly.flags & U8_HWC), x1 - x0
    if ly.strides == "inplace":
        stride, off, extent = (w, 3 * x0, 3 * w * h) if hwc else (w * h, x0 * h, 3 * w * h)
    else:
        pad = 0 if ly.strides == "compact" else (3 if hwc else 5)
        stride = (ws if hwc else ws * h) + pad
        off, extent = 0, (3 * stride * h if hwc else 3 * stride)
    fs = (3 * stride * h if hwc else 3 * stride) + 7 if n_frames > 1 else 0
    guard = max(3 * w * h, fs, 0 if hwc else 2 * stride + ws * h)
    return Geometry(hwc, stride, guard + off, extent, fs, n_frames, guard, 2 * guard + (n_frames - 1) * fs + extent, w, h, x0, x1)


def expected(layout, ref8, ref32, w, h, x0, x1, n_frames=1):
    """(uint8 allocation or None, float32 allocation as uint32 words or None): sentinels, with columns [x0, x1) of the oracle's
    frame placed by the addressing rule.  ref8: uint8 (3, w, h) in the stored (R,B,G) order; ref32: float32 (3, w, h) in the true
    (R,G,B) order.  Calls no library code."""
    g = geometry(layout, w, h, x0, x1, n_frames)
    ly = LAYOUTS[layout]
    xr, y = np.arange(x1 - x0)[:, None], np.arange(h)[None, :]
    out = []
    for which, src, fill in (("u8", np.asarray(ref8)[[0, 2, 1]] if ly.flags & U8_RGB else np.asarray(ref8), sentinel_u8),
                             ("f32", np.ascontiguousarray(ref32, np.float32).view(np.uint32), sentinel_f32)):
        if which not in ly.outputs:
            out.append(None)
            continue
        buf = fill(g.total)
        for i in range(n_frames):
            for c in range(3):
                at = (y * g.stride + xr) * 3 + c if g.hwc else c * g.stride + xr * h + y
                buf[g.base + i * g.frame_stride + at] = src[c, x0:x1, :]
        out.append(buf)
    return tuple(out)


PLACES = ("pixel", "pad between planes", "pad between rows", "pad between frames", "column outside the slab", "front guard band",
          "rear guard band")


def classify(index, layout, w, h, x0, x1, n_frames=1):
    """Where element `index` of the allocation lies: one of PLACES."""
    g = geometry(layout, w, h, x0, x1, n_frames)
    if index < g.guard:
        return "front guard band"
    if index >= g.total - g.guard:
        return "rear guard band"
    r = index - g.guard
    if n_frames > 1:
        r -= min(r // g.frame_stride, n_frames - 1) * g.frame_stride
        if r >= g.extent:
            return "pad between frames"
    inplace = LAYOUTS[layout].strides == "inplace"
    if g.hwc:
        col = (r % (3 * g.stride)) // 3                   # the pixel of its row
        if inplace:
            return "pixel" if x0 <= col < x1 else "column outside the slab"
        return "pixel" if col < x1 - x0 else "pad between rows"
    q = r % g.stride                                      # the element of its plane
    if inplace:
        return "pixel" if x0 <= q // h < x1 else "column outside the slab"
    return "pixel" if q < (x1 - x0) * h else "pad between planes"


def places(got, want, layout, w, h, x0, x1, n_frames=1):
    """{place: elements that differ there} of two allocations, compared over their whole length."""
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return collections.Counter(classify(int(i), layout, w, h, x0, x1, n_frames) for i in bad)


def mismatch(got, want, what, layout, w, h, x0, x1, n_frames=1):
    """None where the two allocations are the same elements (uint8 bytes, or the uint32 words of float32 buffers: bit for bit, the
    sign of zero included), else the failure message: what was rendered, the layout, every place that differs with its count, and
    the first four offsets with the place of each."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.dtype in (np.uint8, np.uint32) and got.size == want.size, (what, layout, got.dtype, got.size, want.size)
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return None
    g = geometry(layout, w, h, x0, x1, n_frames)
    assert got.size == g.total, (what, layout, got.size, g.total)
    where = places(got, want, layout, w, h, x0, x1, n_frames)
    first = [f"{int(i)} (base{int(i) - g.base:+d}: {classify(int(i), layout, w, h, x0, x1, n_frames)}, got {int(got[i]):#x}, want {int(want[i]):#x})"
             for i in bad[:4]]
    return (f"{what}: layout {layout}, columns [{x0}, {x1}), {n_frames} frame(s), {'uint8' if got.dtype == np.uint8 else 'float32'}: "
            f"{bad.size} elements differ: {dict(where)}; first offsets {'; '.join(first)}")


# ---------------------------------------------------------------------------------------------------------------------
# The kernels.  name: (scene, MI355RT_* knobs, aa mode, launch flags, spp, seed, explicit grid, the seven fields every logged
# render_kernel<...> line must name, the line's tail, the cull groups line behind it (0: none)).  Between them: the compile-time
# TRIM store with the scalar frame offset (small_twin), the plain store behind an offset parked in LDS (ground_twin, generic_two_wave,
# four_wave_mode1, lanes_parked), rematerialised (lanes_mode3) and formed in registers (counting, lanes_register), and `idx` of
# aa_resolve_kernel (lattice_resolve); an AA mode of the kernel's own from an explicit grid, the closed form and the stochastic
# samples; a family with a material table and the last family of the table.
Variant = collections.namedtuple("Variant", "scene knobs aa flags spp seed explicit line tail groups")
SKY_SEED = 0                                   # the first seed of tools/feature_scenes.draw_lit(seed, w=21, h=13) whose scene is of
                                               # family SKY_LENS_SOFT and whose frame meets test_output_layouts.py's bounds
VARIANTS = {
    "small_twin":       Variant("odd", {}, 0, 0, 0, 1, False, (0, 1, 2, 0, 0, 0, 0), "ground", 2),
    "ground_twin":      Variant("odd", {"MI355RT_SMALL_SCENE": "0"}, 0, 0, 0, 1, False, (0, 1, 2, 0, 0, 0, 0), "ground", 0),
    "generic_two_wave": Variant("odd", {"MI355RT_GROUND_PLANE": "0"}, 0, 0, 0, 1, False, (0, 1, 2, 0, 0, 0, 0), "", 0),
    "counting":         Variant("odd", {}, 0, COUNT_RAYS, 0, 1, False, (0, 0, 4, 1, 0, 0, 0), "", 0),
    "four_wave_mode1":  Variant("c4", {}, 0, 0, 0, 1, False, (0, 1, 4, 0, 0, 1, 0), "ground", 0),
    "lanes_parked":     Variant("c5", {}, 0, 0, 0, 1, False, (0, 1, 4, 0, 0, 2, 0), "ground", 0),
    "lanes_mode3":      Variant("c5", {}, 1, AA_PER_PIXEL, 0, 1, False, (1, 1, 4, 0, 0, 3, 0), "ground", 0),
    "lanes_register":   Variant("c5", {"MI355RT_LANES_PARK": "0"}, 0, 0, 0, 1, False, (0, 0, 4, 0, 0, 2, 0), "", 0),
    "lattice_resolve":  Variant("odd", {}, 1, 0, 0, 1, False, (0, 1, 2, 0, 1, 0, 0), "ground", 2),
    "per_pixel_aa":     Variant("odd", {}, 1, 0, 0, 1, True, (1, 1, 2, 0, 0, 0, 0), "ground", 2),
    "stochastic":       Variant("odd", {}, 2, 0, 2, 5, False, (1, 1, 2, 0, 0, 0, 0), "ground", 2),
    "mat_family":       Variant("mat", {}, 0, 0, 0, 1, False, (0, 1, 2, 0, 0, 0, 1), "", 0),
    "sky_lens_soft":    Variant("sky", {}, 0, 0, 0, 1, False, (0, 0, 2, 0, 0, 0, 18), "", 0),
}
REDUCED = ("small_twin", "ground_twin", "four_wave_mode1", "lanes_mode3", "lattice_resolve", "sky_lens_soft")
_SCENES, _REF = {}, {}


def scene_of(name):
    """The scene of a variant: spheres, lights, planes, camera, fov and shading scalars; with "materials" and the rest of a
    tools/feature_scenes scene where the variant has them."""
    which = VARIANTS[name].scene
    if which not in _SCENES:
        import ground_plane_scenes as gps
        if which in ("odd", "mat"):
            sc = gps.fixture_scene("odd_37x29")
            if which == "mat":
                # closest_hit_scenes.uniform_materials: one table row for every object.  Its own row (1, 0, 0) renders flat object
                # colours, too few for test_output_layouts.py's bounds; the row here is the fixture's scalars (amb, lamb, refl),
                # so the frame keeps the shading of small_twin's
                import closest_hit_scenes as chs
                _, sid, pid = chs.uniform_materials(sc)
                sc = dict(sc, materials=(np.array([sc["shade"]]), sid, pid))
        elif which in ("c4", "c5"):
            g = load_frame({"c4": "c4_s64_d5_sub32", "c5": "c5_s256_d8_sub96"}[which])
            sc = dict(spheres=g["spheres"], lights=g["lights"], planes=g["planes"], cam_origin=g["cam_origin"], cam_rot=g["cam_rot"],
                      fov=float(g["fov"]), shade=(float(g["amb"]), float(g["lamb"]), float(g["refl"])))
        else:
            from feature_gpu import fs
            sc = fs.draw_lit(SKY_SEED, w=W, h=H)
        _SCENES[which] = sc
    return _SCENES[which]


def raygen_of(name):
    sc = scene_of(name)
    return sc["raygen"] if VARIANTS[name].scene == "sky" else raygen_closed_form(W, H, sc["fov"])


def reference(oracle, name, x0=0, x1=W):
    """The oracle's (uint8, float32) frames (3, W, H) of a variant, columns [x0, x1) rendered and the rest zero; once per range,
    read-only."""
    key = (name, x0, x1)
    if key not in _REF:
        from feature_gpu import grid
        v, sc = VARIANTS[name], scene_of(name)
        view = dict(pixel_loc=grid(W, H, raygen_of(name))) if v.explicit else dict(raygen=raygen_of(name))
        if v.scene == "sky":
            from feature_gpu import fs
            kw = {**fs.oracle_kwargs(sc), **view, "spp": v.spp, "seed": sc["hseed"]}
            shade = (0.0, 0.0, 0.0)
        else:
            kw = dict(view, spp=v.spp, seed=v.seed, materials=sc.get("materials"))
            shade = sc["shade"]
        ref = oracle.render(W, H, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], *shade, DEPTH, v.aa,
                            x0=x0, x1=x1, want=("u8", "f32"), **kw)
        _REF[key] = (ref["u8"], ref["f32"])
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def keyed(name):
    """The variant's samples are keyed by the absolute column (the stochastic jitter; the scatter, light and lens hashes): its
    reference is rendered slab by slab through the oracle's own x0, x1."""
    return VARIANTS[name].aa == 2 or VARIANTS[name].scene == "sky"
