"""The small-scene twins of the two-wave ground-plane kernels (rt_device.h: NG, rt_plan.h: cull_groups) against the ground-plane
kernels compiled for any sphere count: the same scene rendered by two contexts, MI355RT_SMALL_SCENE unset and 0.  The uint8 and the
float32 frames must be the same bytes; the first context must log "mi355rt: cull groups N" behind every kernel line, the second no
such line, and both the same "... > ground" kernel lines.  Scenes that are not small (nine spheres), have no ground-plane twin
(a tilted plane) or plan a four-wave shape (64 lights) must log no cull groups either way.
The other parity tests render the small-scene twins by default (every golden scene but the crowds has at most eight spheres);
this file keeps the ground-plane kernels covered on the same scenes.  Frames of 32 x 24 to 48 x 48."""
import re

import numpy as np
import pytest

from conftest import raygen_closed_form
import ground_plane_scenes as gps

pytestmark = pytest.mark.gpu
LOG_LINE = re.compile(r"mi355rt: (?:render_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), \(rt::Family\)(\d+)>([^\n]*)|cull groups (\d+))")
FIELDS = ("aa", "park", "wpw", "count", "lat", "mode", "family")
KNOBS = ("MI355RT_CLUSTER_MINS", "MI355RT_LANES_MINS", "MI355RT_F32_RECORDS", "MI355RT_LANES_PARK", "MI355RT_WPW2_MAX_IMAGE",
         "MI355RT_ORDER_GROUP", "MI355RT_ORDER_TILES", "MI355RT_SEQ_ORDER", "MI355RT_CHUNKS", "MI355RT_GROUND_PLANE", "MI355RT_SMALL_SCENE")

# Spheres resting on the ground around the shadow pair (x, y, radius), in front of the default camera
FILLERS = ((1.0, -1.3, 0.35), (1.0, 1.3, 0.35), (3.4, -1.4, 0.4), (3.4, 1.4, 0.4), (0.2, 0.9, 0.25), (4.2, 0.1, 0.45), (0.4, -0.8, 0.2))
CATCHER = (2.0, 0.0, 0.5, 0.5)          # x, y, z, radius: rests on the ground


def small_scene(S):
    """S spheres over the ground, the default scene's camera and lights.  The last slot is a sphere on the ground (the catcher),
    the one before it hovers between the catcher and light 0 and shadows it (the caster): shadow rays that leave the catcher run the
    SELF cull on the last slot, and the caster certifies nothing for them.  With S >= 6 both are in the second group of four, with
    S = 5 the catcher is.  The slots before them are spheres on the ground around the pair."""
    g = gps.fixture_scene("default_128_d3")
    rows = [(x, y, r, r) for x, y, r in FILLERS[:max(S - 2, 0)]]
    c = np.array(CATCHER[:3])
    if S >= 2:
        to_light = g["lights"][:, 0].astype(np.float64) - c
        u = to_light / np.linalg.norm(to_light)
        k = c + 1.25 * u
        rows.append((k[0], k[1], k[2], 0.3))
        # the straight line from the catcher's point nearest the light to the light passes through the caster
        assert np.linalg.norm(np.cross(k - (c + 0.5 * u), u)) < 0.3
    rows.append(CATCHER)
    sp = np.zeros((7, S), np.float32)
    sp[:4] = np.array(rows, np.float32).T
    sp[4:7] = np.random.default_rng(S).integers(60, 256, (3, S))
    return dict(g, spheres=sp)


def _render(monkeypatch, capfd, sc, w, h, depth, small, *, aa=0, flags=(), knobs=None, pixel_loc=None, sequence=0):
    """One context with the knobs in its environment: (uint8 frames, float32 frames, [(shape fields, tail of the kernel line, cull
    groups logged behind it or 0)]).  sequence = n > 0: rt_render_sequence of n frames per call, three calls: the frames of all three."""
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (knobs or {}).items():
        monkeypatch.setenv(k, v)
    if not small:
        monkeypatch.setenv("MI355RT_SMALL_SCENE", "0")
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    fl = 0
    for name in flags:
        fl |= getattr(L, name)
    amb, lamb, refl = sc["shade"]
    capfd.readouterr()
    with pkg.Renderer(0) as r:
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        if pixel_loc is not None:
            r.set_pixel_loc(pixel_loc)
        else:
            r.set_raygen(w, h, *raygen_closed_form(w, h, sc["fov"]))
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
    lines = []
    for m in LOG_LINE.findall(capfd.readouterr().err):
        if m[8]:
            assert lines and lines[-1][2] == 0, "a cull groups line that follows no kernel line"
            lines[-1] = (lines[-1][0], lines[-1][1], int(m[8]))
        else:
            lines.append((dict(zip(FIELDS, (int(v) for v in m[:7]))), m[7].strip(), 0))
    return u8, f32, lines


def _compare(monkeypatch, capfd, name, sc, w, h, depth, groups, *, tail="ground", expect=None, **kw):
    """Renders with the knob unset and 0.  groups: what the first run must log behind every kernel line (0: no such line)."""
    a8, a32, la = _render(monkeypatch, capfd, sc, w, h, depth, True, **kw)
    b8, b32, lb = _render(monkeypatch, capfd, sc, w, h, depth, False, **kw)
    print(f"{name}: knob unset {[(tuple(s.values()), t, g) for s, t, g in la]}, knob 0 {[(tuple(s.values()), t, g) for s, t, g in lb]}")
    assert la and lb and [(s, t) for s, t, _ in la] == [(s, t) for s, t, _ in lb], name      # the same kernel lines
    assert all(t == tail for _, t, _ in la), (name, la)
    assert all(g == groups for _, _, g in la), (name, la)
    assert all(g == 0 for _, _, g in lb), (name, lb)
    for s, _, _ in la:
        assert s["family"] == 0 and s["count"] == 0 and all(s[k] == v for k, v in (expect or {}).items()), (name, s, expect)
    assert a8.any() and len(np.unique(a8)) > 8, name
    assert a8.tobytes() == b8.tobytes(), (name, int((a8 != b8).sum()))
    assert a32.tobytes() == b32.tobytes(), (name, int((a32.view(np.uint32) != b32.view(np.uint32)).sum()))
    return a8, a32


@pytest.mark.parametrize("S", [1, 3, 4, 5, 6, 7, 8])
def test_group_boundaries(monkeypatch, capfd, S):
    _compare(monkeypatch, capfd, f"S={S} 40x32 d3", small_scene(S), 40, 32, 3, (S + 3) // 4, expect=dict(aa=0, park=1, wpw=2, lat=0, mode=0))


@pytest.mark.parametrize("S", [5, 7])
def test_nan_rays_with_live_padding_slots(monkeypatch, capfd, S):
    """A block of zero vectors in the pixel table, among ordinary pixels: their rays have NaN directions, which no certificate
    holds for, the padding slots' included; the mask's trim keeps those from the float64 test."""
    w, h = 40, 32
    px, y0, dy, z0, dz = raygen_closed_form(w, h, 45.0)
    grid = np.empty((3, w, h))
    grid[0] = px
    grid[1] = (np.arange(w) * dy + y0)[:, None]
    grid[2] = (np.arange(h) * dz + z0)[None, :]
    grid[:, 11:21, 9:19] = 0.0                    # (crosses tiles, and leaves waves with both kinds of lanes)
    _compare(monkeypatch, capfd, f"S={S} NaN rays", small_scene(S), w, h, 3, 2, pixel_loc=grid)


def test_camera_inside_a_sphere(monkeypatch, capfd):
    sc = gps.fixture_scene("inside_sphere_32")
    _compare(monkeypatch, capfd, "inside 32x32", sc, 32, 32, 2, (sc["spheres"].shape[1] + 3) // 4)


def test_odd_frame(monkeypatch, capfd):
    sc = gps.fixture_scene("odd_37x29")
    _compare(monkeypatch, capfd, "odd 37x29", sc, 37, 29, 3, (sc["spheres"].shape[1] + 3) // 4)


def test_render_sequence_of_three_frames(monkeypatch, capfd):
    _compare(monkeypatch, capfd, "sequence 3 x 40x24", gps.fixture_scene("default_128_d3"), 40, 24, 3, 2, sequence=3)


# the two-wave shapes besides the headline's whose small-scene twins are compiled (rt_plan.h: SMALL_TWIN), by their names in
# tests/ground_plane_scenes.py
KEPT_SHAPES = ("two_waves_aa", "two_waves_lattice")


@pytest.mark.parametrize("name", KEPT_SHAPES)
def test_kept_shapes(monkeypatch, capfd, name):
    _, knobs, aa, flags, expect, _ = gps.SHAPES[name]
    _compare(monkeypatch, capfd, name, small_scene(6), 32, 24, 2, 2, aa=aa, flags=flags, knobs=knobs, expect=dict(expect, park=1))


def _tilted():
    return dict(small_scene(6), planes=gps.planes_of((5.0, 0.0, 0.0, 0.0, 0.6, 0.8, 125.0, 125.0, 125.0)))


def _nine():
    sc = small_scene(8)
    extra = np.array([[2.6], [-1.9], [0.3], [0.3], [200.0], [90.0], [40.0]], np.float32)
    return dict(sc, spheres=np.ascontiguousarray(np.concatenate([sc["spheres"], extra], axis=1)))


def _most_lights():
    """RT_MAX_LIGHTS = 64 lights.  anchors_of returns 0 only where the anchored table is over its 40 KiB budget, which a scene of at
    most eight spheres never is (65 rows of 128 bytes; tests/test_small_scene.py has the predicate with a smaller budget).  What 64
    lights do is grow the LDS image past the two-wave bound: the launch is a four-wave one, which has no small-scene twin."""
    rng = np.random.default_rng(64)
    li = np.stack([rng.uniform(-3.0, 6.0, 64), rng.uniform(-5.0, 5.0, 64), rng.uniform(2.0, 7.0, 64)]).astype(np.float32)
    sc = small_scene(8)
    return dict(sc, lights=li, shade=(0.0, 0.02, 0.3))


@pytest.mark.parametrize("name,scene,tail", [("nine_spheres", _nine, "ground"), ("tilted_plane", _tilted, ""), ("most_lights", _most_lights, "ground")])
def test_scenes_that_take_no_small_scene_twin(monkeypatch, capfd, name, scene, tail):
    _compare(monkeypatch, capfd, name, scene(), 32, 24, 2, 0, tail=tail)


@pytest.mark.parametrize("name,scene,tail,groups", [("default_scene", lambda: gps.fixture_scene("default_128_d3"), "ground", 2),
                                                    ("nine_spheres", _nine, "ground", 0), ("tilted_plane", _tilted, "", 0)])
def test_kernel_info_reads_the_twin_the_scene_runs(monkeypatch, capfd, name, scene, tail, groups):
    """rt_get_kernel_info reports the headline shape's kernel in the twin that the current scene's plain launches run: the
    small-scene twin for the default scene's eight spheres, the ground-plane twin with a ninth sphere, the generic kernel over a
    tilted plane.  One 32 x 24 frame each, default parameters; the launch must log that twin, and the call must succeed behind it.
    The three instantiations have the same register count (71 VGPRs, 94 SGPRs in the compiler's resource remarks for
    render_kernel<0, 1, 2, 0, 0, 0, PLAIN>, <..., true> and <..., true, 2>), so `vgprs` cannot tell them apart and is not compared:
    that the call reads the entry of the launch's own table is what rt_plan.h's twin_of and the checks under tests/algo pin."""
    import python_ray_tracer_amd as pkg
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    sc, w, h = scene(), 32, 24
    amb, lamb, refl = sc["shade"]
    capfd.readouterr()
    with pkg.Renderer(0) as r:
        before = r.kernel_info()                                  # no scene yet: the generic kernel
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"])
        r.set_camera(sc["cam_origin"], sc["cam_rot"])
        r.set_raygen(w, h, *raygen_closed_form(w, h, sc["fov"]))
        u8, _ = r.render(amb, lamb, refl, 3, 0, u8=True)
        info = r.kernel_info()
    got = LOG_LINE.findall(capfd.readouterr().err)
    kernels = [m for m in got if not m[8]]
    print(f"{name}: {got}, kernel_info {info}")
    assert kernels and all(tuple(int(v) for v in m[:7]) == (0, 1, 2, 0, 0, 0, 0) and m[7].strip() == tail for m in kernels), (name, got)
    assert [int(m[8]) for m in got if m[8]] == ([groups] * len(kernels) if groups else []), (name, got)
    assert np.asarray(u8).any(), name
    for i in (before, info):
        assert i["vgprs"] > 0 and i["wave_size"] == 64 and i["cu_count"] > 0, (name, i)


def test_against_the_oracle(monkeypatch, capfd, oracle):
    sc, w, h = small_scene(6), 48, 48
    u8, f32 = _compare(monkeypatch, capfd, "S=6 48x48 d3", sc, w, h, 3, 2)
    amb, lamb, refl = sc["shade"]
    ref = oracle.render(w, h, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], amb, lamb, refl, 3, False,
                        raygen=raygen_closed_form(w, h, sc["fov"]), want=("u8", "f32"))
    assert np.array_equal(u8, ref["u8"]), int((u8 != ref["u8"]).any(axis=0).sum())
    assert f32.tobytes() == ref["f32"].tobytes()
