"""The ground-plane twins of the PLAIN render kernels (rt_device.h: GROUND, rt_plan.h: ground_plane) against the generic
kernels: the same scene rendered by two contexts, MI355RT_GROUND_PLANE unset and 0.  The uint8 and the float32 frames must be the
same bytes, and the MI355RT_LOG_KERNELS lines must name the twin ("... > ground") in the first and the generic kernel in the second.
Scenes whose plane is not the one z-up ground (tilted, on another axis, facing down, two planes) must run generic kernels either way,
and so must a shape that has no twin.
The other parity tests render the twins by default (every BASELINE workload has the ground plane); this file keeps the generic
kernels covered on the same kind of scene.  Frames of 32 x 24 to 48 x 48."""
import re

import numpy as np
import pytest

from conftest import raygen_closed_form
import ground_plane_scenes as gps

pytestmark = pytest.mark.gpu
KERNEL_LINE = re.compile(r"mi355rt: render_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), \(rt::Family\)(\d+)>([^\n]*)")
FIELDS = ("aa", "park", "wpw", "count", "lat", "mode", "family")
KNOBS = ("MI355RT_CLUSTER_MINS", "MI355RT_LANES_MINS", "MI355RT_F32_RECORDS", "MI355RT_LANES_PARK", "MI355RT_WPW2_MAX_IMAGE",
         "MI355RT_ORDER_GROUP", "MI355RT_ORDER_TILES", "MI355RT_SEQ_ORDER", "MI355RT_CHUNKS", "MI355RT_GROUND_PLANE")


def _render(monkeypatch, capfd, sc, w, h, depth, ground, *, aa=0, flags=(), knobs=None, raygen=None, sequence=0):
    """One context with the knobs in its environment: (uint8 frames, float32 frames, [(shape fields, tail of the log line)]).
    sequence = n > 0: rt_render_sequence of n frames per call, three calls (the first ones measure frame by frame, a settled one
    launches the n frames at once): the frames of all three calls."""
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (knobs or {}).items():
        monkeypatch.setenv(k, v)
    if not ground:
        monkeypatch.setenv("MI355RT_GROUND_PLANE", "0")
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    fl = 0
    for name in flags:
        fl |= getattr(L, name)
    amb, lamb, refl = sc["shade"]
    capfd.readouterr()
    with pkg.Renderer(0) as r:
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        r.set_raygen(w, h, *(raygen or raygen_closed_form(w, h, sc["fov"])))
        if sequence:
            n, npx = sequence, w * h
            p = r.params(amb, lamb, refl, depth, aa, fl)
            d8, d32 = r.malloc(n * 3 * npx), r.malloc(n * 12 * npx)
            try:
                u8, f32 = np.empty((3, n, 3, w, h), np.uint8), np.empty((3, n, 3, w, h), np.float32)
                for call in range(3):
                    r.h2d(d8, np.zeros(n * 3 * npx, np.uint8))
                    r.render_sequence(p, 0, w, n, d8, d32, npx, 3 * npx, None, None, n)
                    r.sync()
                    r.d2h(u8[call], d8)
                    r.d2h(f32[call], d32)
            finally:
                r.free(d8); r.free(d32)
        else:
            u8, f32 = r.render(amb, lamb, refl, depth, aa, u8=True, f32=True, flags=fl)
    lines = [(dict(zip(FIELDS, (int(v) for v in m[:7]))), m[7].strip()) for m in KERNEL_LINE.findall(capfd.readouterr().err)]
    return u8, f32, lines


def _compare(monkeypatch, capfd, name, sc, w, h, depth, *, twin=True, expect=None, **kw):
    """Renders with the knob unset and 0.  twin: the first run must log twins; else both log generic kernels."""
    a8, a32, la = _render(monkeypatch, capfd, sc, w, h, depth, True, **kw)
    b8, b32, lb = _render(monkeypatch, capfd, sc, w, h, depth, False, **kw)
    print(f"{name}: knob unset {[(tuple(s.values()), t) for s, t in la]}, knob 0 {[(tuple(s.values()), t) for s, t in lb]}")
    assert la and lb and [s for s, _ in la] == [s for s, _ in lb], name          # the plan is the same: only the twin differs
    assert all(t == ("ground" if twin else "") for _, t in la), (name, la)
    assert all(t == "" for _, t in lb), (name, lb)
    for s, _ in la:
        assert s["family"] == 0 and s["count"] == 0 and all(s[k] == v for k, v in (expect or {}).items()), (name, s, expect)
    assert a8.any() and len(np.unique(a8)) > 8, name
    assert a8.tobytes() == b8.tobytes(), (name, int((a8 != b8).sum()))
    assert a32.tobytes() == b32.tobytes(), (name, int((a32.view(np.uint32) != b32.view(np.uint32)).sum()))
    return a8


def test_default_scene_depth_3(monkeypatch, capfd):
    _compare(monkeypatch, capfd, "default 48x48 d3", gps.fixture_scene("default_128_d3"), 48, 48, 3, expect=dict(wpw=2, park=1, mode=0))


def test_odd_frame(monkeypatch, capfd):
    _compare(monkeypatch, capfd, "odd 37x29", gps.fixture_scene("odd_37x29"), 37, 29, 3)


def test_horizon(monkeypatch, capfd):
    """The horizon scene's camera looks along the ground.  On a frame with an odd number of rows the middle row's rays are parallel to
    the plane (den = 0 exactly).  The second frame is a band of rows 0.0004 apart around z = 0, seen from half a unit above the
    ground among the spheres: |den| crosses 0.001 inside the frame (intersections.py:55), the rows below that meet the ground
    between t = 60 and beyond t = 999, and every row shows spheres (the CPU oracle's frame has 37 distinct byte values)."""
    sc = gps.fixture_scene("horizon_64")
    _compare(monkeypatch, capfd, "horizon 47x47", sc, 47, 47, 2)
    px = float(1 / np.tan(np.radians(sc["fov"]) / 2))
    low = dict(sc, cam_origin=np.array([0.0, 0.0, 0.5]))
    _compare(monkeypatch, capfd, "horizon band 40x41", low, 40, 41, 2, raygen=(px, 1.0, -2.0 / 39, 0.008, -0.0004))


def test_camera_inside_a_sphere(monkeypatch, capfd):
    _compare(monkeypatch, capfd, "inside 32x32", gps.fixture_scene("inside_sphere_32"), 32, 32, 2)


def test_render_sequence_of_three_frames(monkeypatch, capfd):
    _compare(monkeypatch, capfd, "sequence 3 x 40x24", gps.fixture_scene("default_128_d3"), 40, 24, 3, sequence=3)


@pytest.mark.parametrize("name", list(gps.SHAPES))
def test_twin_of_every_kind_of_shape(monkeypatch, capfd, name):
    which, knobs, aa, flags, expect, twin = gps.SHAPES[name]
    sc = gps.crowd_scene() if which == "crowd" else dict(gps.fixture_scene("default_128_d3"), shade=(0.05, 0.6, 0.3))
    _compare(monkeypatch, capfd, name, sc, 32, 24, 2, aa=aa, flags=flags, knobs=knobs, expect=expect, twin=twin)


NOT_THE_GROUND = {
    "tilted": [(5.0, 0.0, 0.0, 0.0, 0.6, 0.8, 125.0, 125.0, 125.0)],
    "x_axis": [(9.0, 0.0, 0.0, -1.0, 0.0, 0.0, 90.0, 90.0, 160.0)],
    "two_planes": [gps.GROUND, (9.0, 0.0, 0.0, -1.0, 0.0, 0.0, 90.0, 90.0, 160.0)],
    "facing_down": [(5.0, 0.0, 0.0, 0.0, 0.0, -1.0, 125.0, 125.0, 125.0)],
}


@pytest.mark.parametrize("name", list(NOT_THE_GROUND))
def test_other_planes_run_generic_kernels(monkeypatch, capfd, name):
    sc = dict(gps.fixture_scene("default_128_d3"), planes=gps.planes_of(*NOT_THE_GROUND[name]))
    _compare(monkeypatch, capfd, name, sc, 32, 24, 2, twin=False)
