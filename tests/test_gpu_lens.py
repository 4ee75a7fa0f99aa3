"""Depth of field on the GPU (rt_set_lens, the lens kernels): every lens_* fixture through every entry point, the large fixtures
on every traversal, all 44 lens kernels through the dispatcher's environment overrides, aperture 0 against the pinhole camera,
a lens closed again and a frame in flight keeping its lens, column slabs, the seed, the error paths and the example."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from feature_gpu import (BIG, IGNORED, VARIANTS, aim, check as _check, column_slabs_are_the_full_frame, fixture_lens as _lens,
                         kw as _kw, large_fixtures_on_a_traversal, lens_materials, render_host as _render_host, render_modes,
                         run_example, same_as_first, set_view, variant_renderers, variant_source, walk_entry_points)
from feature_gpu import rend  # noqa: F401  (the session's renderer with the pinhole camera restored)
from test_lens import lens_cases

pytestmark = pytest.mark.gpu


def _load(case):
    return np.load(os.path.join(GOLDEN, f"lens_{case}.npz"))


def _mats(g):
    return g["materials"], g["sphere_material"], g["plane_material"]


def _scene(r, g):
    r.set_scene(g["spheres"], g["lights"], g["planes"], materials=_mats(g), light_radius=g["light_radius"],
                shadow_samples=int(g["shadow_samples"]))


def _setup(r, g, explicit=False, lens=True):
    return set_view(r, g, _scene, lens=_lens(g) if lens else (0.0, 1.0), explicit=explicit)


@pytest.mark.parametrize("case", lens_cases())
def test_fixture_every_entry_point(rend, case):
    g = _load(case)
    walk_entry_points(rend, g, _setup, case in BIG, cameras=True, begin_end=True, explicit=case != BIG[1])
    _setup(rend, g, lens=False)                                 # the pinhole camera: the fixture's u8_pinhole
    u8, _ = _render_host(rend, g)
    _check(g, u8, None, "aperture 0", key="u8_pinhole")


@pytest.mark.parametrize("lanes_mins, records", [("30", "1"), ("30", "0"), ("100000", "1"), ("100000", "0")])
def test_large_fixtures_on_every_traversal(monkeypatch, lanes_mins, records):
    large_fixtures_on_a_traversal(monkeypatch, lanes_mins, records, _load, _setup)


@pytest.mark.parametrize("soft", [False, True], ids=["scatter", "area_lights"])
@pytest.mark.parametrize("case", list(VARIANTS))
def test_every_lens_kernel_same_bytes(monkeypatch, case, soft):
    """feature_gpu.VARIANTS launches every one of the 22 lens kernels of each family (rt_device.h LENS: the scatter twins without
    a light radius, the area-light twins with one).  The frames of one scene must be the same bytes in every variant."""
    src = variant_source(case, _load)
    S, P, NL = src["spheres"].shape[1], src["planes"].shape[1], src["lights"].shape[1]
    radius = np.array([0.5, 0.0, 0.3][:NL], np.float32) if soft else np.zeros(NL, np.float32)
    first = None
    for env, r in variant_renderers(monkeypatch, case):
        aim(r, src, 160, 96)
        r.set_scene(src["spheres"], src["lights"], src["planes"], materials=lens_materials(S, P), light_radius=radius, shadow_samples=2)
        if first is None:
            pin = r.render(*IGNORED.values(), 3, 0, u8=True, seed=3)[0]
        r.set_lens(0.08, 3.0)
        outs = render_modes(r)
        assert first is not None or not np.array_equal(outs[0][0], pin)     # (the lens kernels ran)
        first = same_as_first(first, outs, env)


@pytest.mark.parametrize("kind", ["mat", "refr", "scat", "soft"])
def test_aperture_zero_is_the_pinhole(rend, kind):
    """Aperture 0: the bytes of the same scene without a lens, whatever the focus distance (a MAT, REFR, SCAT and SOFT table)."""
    g = _load("soft_glass_rough_48_d4")
    w, h = _setup(rend, g, lens=False)
    table, sid, pid = _mats(g)
    table = np.array(table)
    if kind == "mat":
        table = table[:, :3]
    elif kind == "refr":
        table = table[:, :5]
    elif kind == "scat":
        assert (table[:, 5] > 0).any()
    rad = g["light_radius"] if kind == "soft" else np.zeros_like(g["light_radius"])
    rend.set_scene(g["spheres"], g["lights"], g["planes"], materials=(table, sid, pid), light_radius=rad, shadow_samples=2)
    for aa, spp in ((0, 0), (1, 0), (2, 3)):
        rend.set_lens(0.0, 1.0)
        ref8, ref32 = rend.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, spp=spp, seed=5)
        for f in (0.5, 2.0, 1e6):
            rend.set_lens(0.0, f)
            u8, f32 = rend.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, spp=spp, seed=5)
            assert u8.tobytes() == ref8.tobytes() and f32.tobytes() == ref32.tobytes(), (aa, f)
        rend.set_lens(0.1, 2.0)                                   # and a lens does differ from it
        u8, _ = rend.render(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], 3, aa, u8=True, f32=True, spp=spp, seed=5)
        assert not np.array_equal(u8, ref8), aa


def test_lens_closed_again_and_a_frame_in_flight_keeps_its_lens(rend):
    g = _load("default_64_d4")
    w, h = _setup(rend, g)
    a, f = _lens(g)
    lens8, _ = _render_host(rend, g)
    _check(g, lens8, None, "lens")
    rend.set_lens(0.0, f)                                         # closed again: the pinhole frame
    u8, _ = _render_host(rend, g)
    _check(g, u8, None, "closed again", key="u8_pinhole")
    rend.set_lens(2 * a, 0.5 * f)
    other8, _ = _render_host(rend, g)
    assert not np.array_equal(other8, lens8)
    # launches queued on two streams, the lens changed between them: each frame keeps the lens it was launched with
    p = rend.params(IGNORED["amb"], IGNORED["lamb"], IGNORED["refl"], int(g["depth"]), int(g["aa"]), **_kw(g))
    npx = w * h
    s1, s2 = rend.stream_create(), rend.stream_create()
    bufs = [rend.malloc(3 * npx) for _ in range(3)]
    try:
        rend.set_lens(a, f)
        rend.render_device(p, 0, w, bufs[0], None, npx, stream=s1)
        rend.set_lens(2 * a, 0.5 * f)
        rend.render_device(p, 0, w, bufs[1], None, npx, stream=s2)
        rend.set_lens(0.0, f)
        rend.render_device(p, 0, w, bufs[2], None, npx, stream=s1)
        rend.sync(s1)
        rend.sync(s2)
        got = [np.empty((3, w, h), np.uint8) for _ in range(3)]
        for o, b in zip(got, bufs):
            rend.d2h(o, b)
        _check(g, got[0], None, "in flight, lens")
        assert np.array_equal(got[1], other8), "in flight, the second lens"
        _check(g, got[2], None, "in flight, closed", key="u8_pinhole")
    finally:
        for b in bufs:
            rend.free(b)
        rend.stream_destroy(s1)
        rend.stream_destroy(s2)


@pytest.mark.parametrize("aa, spp", [(0, 0), (1, 0), (2, 2)])
def test_column_slab_is_the_full_frame(rend, aa, spp):
    column_slabs_are_the_full_frame(rend, _load("soft_glass_rough_48_d4"), _setup, aa, spp, ((9, 41), (33, 48)))


def test_seed_moves_the_lens_samples(rend):
    """A matte table (no rough row, no area light): only the lens samples depend on the seed.  The same seed gives the same
    bytes, different seeds different ones; without a lens the seed changes nothing."""
    g = _load("default_64_d4")
    _setup(rend, g)
    frames = {s: _render_host(rend, g, seed=s) for s in (1, 2, 0xFFFFFFFF)}
    again = _render_host(rend, g, seed=2)
    assert again[0].tobytes() == frames[2][0].tobytes() and again[1].tobytes() == frames[2][1].tobytes()
    assert not np.array_equal(frames[1][0], frames[2][0]) and not np.array_equal(frames[2][0], frames[0xFFFFFFFF][0])
    rend.set_lens(0.0, 1.0)
    pts = [_render_host(rend, g, seed=s)[1] for s in (1, 2, 0xFFFFFFFF)]
    assert all(p.tobytes() == pts[0].tobytes() for p in pts)


def test_errors(rend):
    import python_ray_tracer_amd as pkg
    from python_ray_tracer_amd import _lib as L
    g = _load("default_64_d4")
    _setup(rend, g)
    a, f = _lens(g)
    lib = rend._lib
    for bad in ((-0.1, f), (float("nan"), f), (float("inf"), f), (-float("inf"), f), (a, 0.0), (a, -1.0), (a, float("nan")),
                (a, float("inf"))):
        assert lib.rt_set_lens(rend._ctx, *bad) == L.RT_ERR_BAD_ARG, bad
        u8, f32 = _render_host(rend, g)                           # the previous lens stays
        _check(g, u8, f32, f"after a refused lens {bad}")
    assert lib.rt_set_lens(None, a, f) == L.RT_ERR_BAD_ARG
    with pytest.raises(pkg.RenderError) as e:                     # no counting kernels with a lens (nor for a material scene)
        _render_host(rend, g, flags=L.RT_FLAG_COUNT_RAYS)
    assert e.value.status == L.RT_ERR_BAD_ARG
    # a lens on a scalar-only scene: refused at launch, with the lens still set; fine again without it
    rend.set_scene(g["spheres"], g["lights"], g["planes"])
    with pytest.raises(pkg.RenderError) as e:
        rend.render(0.0, 0.6, 0.3, 2, 0, u8=True)
    assert e.value.status == L.RT_ERR_STATE and "material table" in str(e.value)
    rend.set_lens(0.0, f)
    assert rend.render(0.0, 0.6, 0.3, 2, 0, u8=True)[0].any()
    _setup(rend, g)
    u8, f32 = _render_host(rend, g)
    _check(g, u8, f32, "after the refused launches")


def test_example_with_depth_of_field_writes_png(tmp_path):
    """examples/render_png.py --dof A --spp N: the default scene with materials through a thin lens focused on sphere 0."""
    outs = {}
    for flag in (["--materials", "--spp", "4"], ["--dof", "0.1", "--spp", "4"], ["--dof", "0.1", "--spp", "4", "--focus-on-sphere", "3"]):
        log, outs[" ".join(flag)] = run_example(str(tmp_path / f"{'_'.join(x.strip('-') for x in flag)}.png"), "160x96", 3, 2, *flag)
    assert "dof=0.1" in log
    a, b, c = outs.values()
    assert b.shape == (96, 160, 3) and b.any()
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
