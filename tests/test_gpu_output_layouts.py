"""Where the render kernels put their pixels, in every form of the store (rt_device.h: store_pixel, the offsets `off` and `fo` of
render_kernel, `idx` of aa_resolve_kernel; rt_launch.h: frame_params, slab_params), against tests/output_layouts.py's restatement of
include/mi355rt.h's addressing rule.  The other render tests ask whether the pixels are the oracle's and read them from a compact
planar buffer; these ask where they land once the caller picks the layout, and what else is written.

Every output buffer is filled with sentinels that depend on the position, with a guard band of a frame or more in front of the first
frame and behind the last; after the launch the whole allocation is compared with `expected`: the oracle's pixels where the rule
puts them and the sentinels everywhere else, byte for byte (uint8) and bit for bit (float32).  A failure names the place: a pixel of
the slab, a pad between planes, rows or frames, a column outside the slab, a guard band.

Frames of 21 x 13 (3 x 2 tiles, part tiles both ways), column ranges [0, 21), [3, 18) and [17, 18); every variant of
output_layouts.VARIANTS in a context of its own that logs its kernels, every logged line held to the variant's:
  * rt_render_device: the ten LAYOUTS (both outputs, one, padded strides, in place in a full frame, RT_FLAG_U8_RGB, RT_FLAG_U8_HWC
    at three pitches) for every variant;
  * rt_render_sequence: three frames in launches of two, frame_stride the least plus 7, three calls (the third in the settled
    order) and one call with a camera per frame, for six of the variants;
  * rt_render and rt_render_begin / rt_render_end on slots 0 and 3 into views of a larger sentinel-filled host array, for the same six.
Nothing here passes an argument the library refuses (tests/test_gpu_entry_errors.py) or renders a frame beyond one dispatch
(tests/test_gpu_frame_limits.py)."""
import contextlib
import re

import numpy as np
import pytest

import output_layouts as ol
from feature_gpu import IGNORED, grid
from output_layouts import H, LAYOUTS, SLABS, VARIANTS, W
from test_gpu_fixed_path import KNOBS

pytestmark = pytest.mark.gpu
LOG_LINE = re.compile(r"mi355rt: (?:render_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), \(rt::Family\)(\d+)>([^\n]*)|cull groups (\d+))")
ROOM = max(ol.geometry(layout, W, H, x0, x1, n).total for layout in LAYOUTS for x0, x1 in SLABS for n in (1, ol.N_SEQ)) + 64
_SEEN = {}            # variant -> {(the seven fields, the line's tail, cull groups)} that its rt_render_device launches logged


def _lines(capfd):
    """[(the seven fields, the tail, the cull groups logged behind the line or 0)] of the launches since the last call."""
    lines = []
    for m in LOG_LINE.findall(capfd.readouterr().err):
        if m[8]:
            assert lines and lines[-1][2] == 0, "a cull groups line that follows no kernel line"
            lines[-1] = (lines[-1][0], lines[-1][1], int(m[8]))
        else:
            lines.append((tuple(int(v) for v in m[:7]), m[7].strip(), 0))
    return lines


def _lines_are_the_variants(capfd, name, what):
    v, lines = VARIANTS[name], _lines(capfd)
    assert lines and all(ln == (v.line, v.tail, v.groups) for ln in lines), (name, what, (v.line, v.tail, v.groups), sorted(set(lines)))
    return set(lines)


@contextlib.contextmanager
def _context(monkeypatch, capfd, name):
    """A context of the variant's own: its knobs in the environment and the others cleared, its scene, camera and grid set."""
    import python_ray_tracer_amd as pkg
    v, sc = VARIANTS[name], ol.scene_of(name)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, value in v.knobs.items():
        monkeypatch.setenv(k, value)
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    capfd.readouterr()
    r = pkg.Renderer(0)
    try:
        if v.scene == "sky":
            r.set_scene(sc["spheres"], sc["lights"], sc["planes"], flags=int(sc["typed"]), materials=(sc["table"], sc["sid"], sc["pid"]),
                        light_radius=sc["radius"], shadow_samples=sc["n"], textures=sc["textures"], light_rgb=sc["light_rgb"], sky=sc["sky"])
            r.set_lens(*sc["lens"])
        else:
            r.set_scene(sc["spheres"], sc["lights"], sc["planes"], materials=sc.get("materials"))
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        if v.explicit:
            r.set_pixel_loc(grid(W, H, ol.raygen_of(name)))
        else:
            r.set_raygen(W, H, *ol.raygen_of(name))
        yield r
    finally:
        try:
            if v.scene == "sky":
                r.set_lens(0.0, 1.0)
        finally:
            r.close()


def _shading(name):
    """(amb, lamb, refl, depth, aa) and the flags, spp and seed of the variant's launches; a scene with a table must not read the scalars."""
    v, sc = VARIANTS[name], ol.scene_of(name)
    shade = tuple(IGNORED.values()) if v.scene in ("mat", "sky") else sc["shade"]
    return (*shade, ol.DEPTH, v.aa), dict(spp=v.spp, seed=sc["hseed"] if v.scene == "sky" else v.seed)


def _ref(oracle, name, x0, x1):
    return ol.reference(oracle, name, x0, x1) if ol.keyed(name) else ol.reference(oracle, name)


def _same(what, name, layout, x0, x1, n, got8, got32, ref):
    """The allocations read back against `expected`, and what lies behind them in the buffer against the sentinels."""
    g = ol.geometry(layout, W, H, x0, x1, n)
    for got, want, fill in zip((got8, got32), ol.expected(layout, ref[0], ref[1], W, H, x0, x1, n), (ol.sentinel_u8, ol.sentinel_f32)):
        assert (got is None) == (want is None)
        if got is None:
            continue
        msg = ol.mismatch(got[:g.total], want, f"{name}: {what}", layout, W, H, x0, x1, n)
        assert msg is None, msg
        beyond = np.flatnonzero(got[g.total:] != fill(got.size)[g.total:])
        assert not beyond.size, f"{name}: {what}: layout {layout}: written beyond the rear guard band, at {(beyond[:4] + g.total).tolist()} of {g.total}"


class _Buffers:
    """Two device buffers of ROOM elements; a launch's allocation (output_layouts.geometry) is their front."""

    def __init__(self, r):
        self.r, self.d8, self.d32 = r, r.malloc(ROOM), r.malloc(4 * ROOM)

    def free(self):
        self.r.free(self.d8)
        self.r.free(self.d32)

    def launch(self, name, layout, x0, x1, ref, what, n=1, cameras=None):
        r, ly, g = self.r, LAYOUTS[layout], ol.geometry(layout, W, H, x0, x1, n)
        args, kw = _shading(name)
        p = r.params(*args, VARIANTS[name].flags | ly.flags, **kw)
        r.h2d(self.d8, ol.sentinel_u8(ROOM))
        r.h2d(self.d32, ol.sentinel_f32(ROOM))
        d8 = self.d8 + g.base if "u8" in ly.outputs else None           # a pointer that is NULL has no buffer behind it
        d32 = self.d32 + 4 * g.base if "f32" in ly.outputs else None
        if n == 1:
            r.render_device(p, x0, x1, d8, d32, g.stride)
        else:
            r.render_sequence(p, x0, x1, n, d8, d32, g.stride, g.frame_stride, cameras, None, ol.FRAMES_PER_LAUNCH)
        r.sync()
        got8, got32 = np.empty(ROOM, np.uint8), np.empty(ROOM, np.uint32)
        r.d2h(got8, self.d8)
        r.d2h(got32, self.d32)
        # the buffer of an output that was not asked for holds its sentinels still
        if d8 is None:
            assert np.array_equal(got8, ol.sentinel_u8(ROOM)), f"{name}: {what}: layout {layout}: the uint8 buffer was written to"
        if d32 is None:
            assert np.array_equal(got32, ol.sentinel_f32(ROOM)), f"{name}: {what}: layout {layout}: the float32 buffer was written to"
        _same(what, name, layout, x0, x1, n, got8 if d8 else None, got32 if d32 else None, ref)


def _run_device(name, monkeypatch, capfd, oracle):
    """Every layout over the three column ranges through rt_render_device, in a context of the variant's own; once per variant."""
    if name in _SEEN:
        return _SEEN[name]
    seen = set()
    with _context(monkeypatch, capfd, name) as r:
        b = _Buffers(r)
        try:
            for x0, x1 in SLABS:
                ref = _ref(oracle, name, x0, x1)
                for layout in LAYOUTS:
                    b.launch(name, layout, x0, x1, ref, "rt_render_device")
                    if len(LAYOUTS[layout].outputs) == 1 and not LAYOUTS[layout].flags:   # behind a NULL pointer: the context is unharmed
                        b.launch(name, "planar_both", x0, x1, ref, f"rt_render_device behind {layout}")
                seen |= _lines_are_the_variants(capfd, name, f"rt_render_device [{x0}, {x1})")
        finally:
            b.free()
    _SEEN[name] = seen
    return seen


@pytest.mark.parametrize("name", list(VARIANTS))
def test_render_device_every_layout(monkeypatch, capfd, oracle, name):
    seen = _run_device(name, monkeypatch, capfd, oracle)
    print(f"{name}: {sorted(seen)}")


@pytest.mark.parametrize("name", ol.REDUCED)
def test_render_sequence_layouts(monkeypatch, capfd, oracle, name):
    """Three frames in launches of two (one launch of two frames and one of one), three calls, so that the third call's launches go
    out in the settled order, where a launch holds several frames; then one call with three equal cameras, a launch per frame."""
    sc = ol.scene_of(name)
    cameras = np.tile(np.concatenate([np.asarray(sc["cam_origin"], np.float64).reshape(3), np.asarray(sc["cam_rot"], np.float64).reshape(9)]),
                      (ol.N_SEQ, 1))
    with _context(monkeypatch, capfd, name) as r:
        b = _Buffers(r)
        try:
            for x0, x1 in SLABS:
                ref = _ref(oracle, name, x0, x1)
                for layout in ol.SEQUENCE_LAYOUTS:
                    for call in range(3):
                        b.launch(name, layout, x0, x1, ref, f"rt_render_sequence call {call}", n=ol.N_SEQ)
                    b.launch(name, layout, x0, x1, ref, "rt_render_sequence with cameras", n=ol.N_SEQ, cameras=cameras)
                _lines_are_the_variants(capfd, name, f"rt_render_sequence [{x0}, {x1})")
            st = r.stats()
        finally:
            b.free()
    print(f"{name}: launches {st['launches']}, frames {st['frames']}, settled {st['launches_settled']}, measuring {st['launches_measuring']}")
    if not VARIANTS[name].line[4]:                                # (the lattice goes out frame by frame, before each frame's resolve)
        assert st["frames"] > st["launches"], (name, st)          # some launch held more than one frame: `fo` of a frame > 0 in one grid


@pytest.mark.parametrize("name", ol.REDUCED)
def test_host_entries_layouts(monkeypatch, capfd, oracle, name):
    """rt_render, and rt_render_begin / rt_render_end on the first and the last slot, into views of a larger sentinel-filled host
    array: the guard bands exist on the host too."""
    args, kw = _shading(name)
    with _context(monkeypatch, capfd, name) as r:
        for x0, x1 in SLABS:
            ref = _ref(oracle, name, x0, x1)
            for layout in ol.HOST_LAYOUTS:
                ly, g = LAYOUTS[layout], ol.geometry(layout, W, H, x0, x1)
                for entry in ("rt_render", 0, 3):
                    big8, big32 = ol.sentinel_u8(g.total), ol.sentinel_f32(g.total)
                    n = 3 * (x1 - x0) * H
                    out8 = big8[g.base:g.base + n] if "u8" in ly.outputs else None
                    out32 = big32.view(np.float32)[g.base:g.base + n] if "f32" in ly.outputs else None
                    flags = VARIANTS[name].flags | ly.flags
                    if entry == "rt_render":
                        r.render_into(*args, out8, out32, x0=x0, x1=x1, flags=flags, **kw)
                    else:
                        r.render_begin(entry, *args, out8, out32, x0=x0, x1=x1, flags=flags, **kw)
                        r.render_end(entry)
                    what = entry if entry == "rt_render" else f"rt_render_begin/end slot {entry}"
                    _same(what, name, layout, x0, x1, 1, big8 if out8 is not None else None, big32 if out32 is not None else None, ref)
            _lines_are_the_variants(capfd, name, f"host entries [{x0}, {x1})")


def test_the_variants_reach_every_store_form(monkeypatch, capfd, oracle):
    """Over the module (the variants run here if they have not yet): every form of the store and of the offsets was launched."""
    seen = set().union(*(_run_device(name, monkeypatch, capfd, oracle) for name in VARIANTS))
    print(f"render_kernel lines seen ((aa, park, wpw, count, lat, mode, family), tail, cull groups): {sorted(seen)}")
    fields = ("aa", "park", "wpw", "count", "lat", "mode", "family")
    rows = [dict(zip(fields, ln), tail=tail, groups=groups) for ln, tail, groups in seen]
    forms = {
        "the TRIM store (a cull groups line)": lambda k: k["groups"] > 0 and k["park"] and k["wpw"] == 2 and not k["aa"] and not k["lat"],
        "a parked two-wave ground twin without it": lambda k: k["groups"] == 0 and k["tail"] == "ground" and k["park"] and k["wpw"] == 2,
        "the generic kernel (an empty tail)": lambda k: k["tail"] == "" and k["park"] and k["wpw"] == 2 and k["family"] == 0,
        "count = 1": lambda k: k["count"] == 1,
        "mode 1": lambda k: k["mode"] == 1,
        "mode 2 parked": lambda k: k["mode"] == 2 and k["park"],
        "mode 2 register": lambda k: k["mode"] == 2 and not k["park"],
        "mode 3": lambda k: k["mode"] == 3,
        "lat = 1": lambda k: k["lat"] == 1,
        "family 1": lambda k: k["family"] == 1,
        "family 18": lambda k: k["family"] == 18,
    }
    missing = [form for form, has in forms.items() if not any(has(k) for k in rows)]
    assert not missing, (missing, sorted(seen))
