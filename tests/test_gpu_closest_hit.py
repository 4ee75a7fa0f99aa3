"""closest_hit's tie rule in every table mode (rt_device.h: `tq == tb && sphere_orig(k) < sphere_orig(bidx)`).  Of equal distances
the sphere with the lowest index in the CALLER's order wins; a clustered scene is stored in the packer's spatial order, so a kernel
that kept the lowest slot would differ wherever two spheres tie.  tests/golden/tie_break.npz ties in 57 to 63 of its 64 pixels but
has 16 spheres: a flat scene, slot order equal to caller order.  Here its 16 spheres stand at seeded caller indices among fillers
(tests/closest_hit_scenes.py: tie_scene; tests/test_closest_hit_scenes.py shows on the CPU that the caller's order decides 64 of 64
pixels), in scenes and under knobs that reach every table mode (SETTINGS), each in a fresh context that logs its kernels:
MODE 0 from LDS records, MODE 1, 2 and 3 from global memory, the lane-owned ones through the merge across lanes; the PLAIN and the
MAT kernels; with and without AA.  Truth is the CPU oracle, bit for bit, uint8 and float32.  Then two planes on top of each other,
through mirror bounces."""
import pytest

from conftest import raygen_closed_form
import closest_hit_scenes as chs
from feature_gpu import KERNEL_LINE, same as _same

from python_ray_tracer_amd import _lib as L

pytestmark = pytest.mark.gpu
SEED = 7
ORDERS = [(case, reverse) for case in range(chs.TIE_CASES) for reverse in (False, True)]
STOCH_GRID = raygen_closed_form(8, 8, 45.0)       # RT_AA_STOCHASTIC needs the closed-form grid: the one the fixture's targets come from
_SEEN = {}                                        # setting -> {(family, clustered, aa, (mode, park, wpw))} of its launches


def _launched(capfd):
    names = [tuple(int(v) for v in n) for n in KERNEL_LINE.findall(capfd.readouterr().err)]
    assert names, "no render_kernel line was logged"
    return names


def _oracle(oracle, sc, aa, spp=0, materials=None):
    grid = dict(raygen=STOCH_GRID) if aa == 2 else dict(pixel_loc=sc["pixel_loc"])
    shade = (7.0, -3.0, 2.0) if materials is not None else (1.0, 0.0, 0.0)           # (a material scene must not read them)
    ref = oracle.render(8, 8, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], *shade, 0, aa, spp=spp, seed=SEED,
                        want=("u8", "f32"), materials=materials, **grid)
    return ref["u8"], ref["f32"]


def _run_setting(name, monkeypatch, capfd, oracle):
    """Every tie case in both caller orders under one setting, in a context of its own; the launches' shapes into _SEEN[name]."""
    if name in _SEEN:
        return _SEEN[name]
    import python_ray_tracer_amd as pkg
    S, lights, knobs, clustered, _, plain, with_aa = chs.SETTINGS[name]
    for k in chs.KNOB_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MI355RT_LOG_KERNELS", "1")
    monkeypatch.setenv("MI355RT_CHUNKS", "1")
    seen = set()
    with pkg.Renderer(0) as r:
        for case, reverse in ORDERS:
            sc = chs.tie_scene(case, S, SEED, reverse, lights)
            r.set_camera(sc["cam_origin"], sc["cam_rot"])
            for materials in (None, chs.uniform_materials(sc)):
                r.set_scene(sc["spheres"], sc["lights"], sc["planes"], materials=materials)
                shade = (1.0, 0.0, 0.0) if materials is None else (7.0, -3.0, 2.0)
                for aa, flags, spp in ((0, 0, 0), (1, L.RT_FLAG_AA_PER_PIXEL, 0), (2, 0, 2)):
                    if aa == 2 and materials is not None:
                        continue
                    if aa == 2:
                        r.set_raygen(8, 8, *STOCH_GRID)
                    else:
                        r.set_pixel_loc(sc["pixel_loc"])
                    capfd.readouterr()
                    u8, f32 = r.render(*shade, 0, aa, u8=True, f32=True, flags=flags, spp=spp, seed=SEED)
                    what = f"{name} case {case} reverse={reverse} aa={aa} {'MAT' if materials is not None else 'PLAIN'}"
                    for n in _launched(capfd):
                        shape = (n[5], n[1], n[2])                               # (mode, park, wpw)
                        assert n[0] == (aa != 0) and n[6] == (materials is not None), (what, n)
                        if materials is None:                                    # the shape the setting is there for (rt_plan.h on the CPU)
                            assert shape == (with_aa if aa else plain), (what, n)
                        seen.add((n[6], clustered, aa != 0, shape))
                    _same(what, u8, f32, *_oracle(oracle, sc, aa, spp, materials))
    _SEEN[name] = seen
    return seen


@pytest.mark.parametrize("name", list(chs.SETTINGS))
def test_tie_rule_in_every_table_mode(monkeypatch, capfd, oracle, name):
    seen = _run_setting(name, monkeypatch, capfd, oracle)
    print(f"{name}: render_kernel (family, clustered, aa, (mode, park, wpw)) launched: {sorted(seen)}")


def test_the_settings_reach_every_table_mode(monkeypatch, capfd, oracle):
    """Over the module (the settings run here if they have not yet): MODE 0 in four-wave workgroups on a clustered scene, MODE 1,
    MODE 2 parked and register, MODE 3; and the MAT kernels in MODE 0, 1 and 2."""
    seen = set().union(*(_run_setting(name, monkeypatch, capfd, oracle) for name in chs.SETTINGS))
    shapes = {(clustered, shape) for fam, clustered, aa, shape in seen if fam == 0}
    print(f"render_kernel shapes seen, PLAIN (clustered, (mode, park, wpw)): {sorted(shapes)}")
    print(f"render_kernel shapes seen, MAT: {sorted({(c, s) for fam, c, aa, s in seen if fam == 1})}")
    modes = {(mode, park) for _, (mode, park, wpw) in shapes}
    assert any(c and s[0] == 0 and s[2] == 4 for c, s in shapes), "MODE 0, four waves, clustered"
    assert any(not c and s[0] == 0 and s[2] == 4 for c, s in shapes), "MODE 0, four waves, flat"
    assert {m for m, _ in modes} == {0, 1, 2, 3} and {(2, 1), (2, 0), (3, 1)} <= modes, modes
    assert any(c and s[0] == 1 for c, s in shapes) and any(not c and s[0] == 1 for c, s in shapes), "MODE 1 clustered and flat"
    assert {0, 1, 2} <= {s[0] for fam, c, aa, s in seen if fam == 1}, "the MAT kernels"


@pytest.mark.parametrize("aa", [0, 1])
def test_coincident_planes_through_mirror_bounces(renderer, oracle, aa):
    """Two planes with the same origin and normal at indices 0 and 1 under 24 spheres (clustered), depth 2: the floor pixels and
    the mirror bounces that end on the floor show plane 0 (tests/test_closest_hit_scenes.py: swapping the two colours changes 246
    and 301 of the 768 pixels of the oracle's frames)."""
    sc = chs.coincident_planes_scene()
    w, h = sc["w"], sc["h"]
    rg = raygen_closed_form(w, h, sc["fov"])
    ref = oracle.render(w, h, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], *sc["shade"], sc["depth"], aa,
                        raygen=rg, want=("u8", "f32"))
    renderer.set_scene(sc["spheres"], sc["lights"], sc["planes"])
    renderer.set_camera(sc["cam_origin"], sc["cam_rot"])
    renderer.set_raygen(w, h, *rg)
    for flags in (0, L.RT_FLAG_AA_PER_PIXEL) if aa else (0,):
        u8, f32 = renderer.render(*sc["shade"], sc["depth"], aa, u8=True, f32=True, flags=flags)
        _same(f"coincident planes aa={aa} flags={flags}", u8, f32, ref["u8"], ref["f32"])
