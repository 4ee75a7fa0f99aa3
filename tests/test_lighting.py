"""Lighting on the CPU (rt_set_scene_lighting): the numpy statement of the contract on hand-computed cases, Material and Light
validation, the 8-column table, the binding, and the lighting_* fixtures' consistency (the white-light, spec = 0 frame of an
untextured fixture is the CPU oracle's; sampled pixels of fixtures, the textured ones among them, recomputed with
tools/gen_lighting_golden.py where the reference checkout is)."""
import glob
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, raygen_closed_form

from python_ray_tracer_amd.scene import Light, Material, Plane, Scene, Sphere
from python_ray_tracer_amd.scene.lighting import SHININESS, light_terms, light_wants, squarings

CASES = ("default_64_d4", "aa_48_d2", "stoch_40x24_spp3_seed7", "c4_s64_d5_sub32", "c5_s256_d8_sub96", "inside_32_d3",
         "everything_48_d4", "grazing_48_d2", "shin_extremes_32_d1")
TEXTURED = ("default_64_d4", "everything_48_d4")            # the fixtures with a textured object
EVENTS = ("highlight_without_lambert", "facing_light_no_highlight", "occluded_specular_only", "highlight_on_glass")


def lighting_cases():
    return sorted(os.path.basename(p)[len("lighting_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "lighting_*.npz")))


def load_lighting(case):
    return np.load(os.path.join(GOLDEN, f"lighting_{case}.npz"))


def fixture_textures(g, textured=True):
    """The `textures=` argument of Renderer.set_scene for a fixture, or None for a fixture without textures."""
    if len(g["tex_first"]) == 0:
        return None
    recs = [(g["tex_origin"][k], g["tex_axes"][k], tuple(int(v) for v in g["tex_dims"][k]), int(g["tex_first"][k]))
            for k in range(len(g["tex_first"]))]
    st, pt = np.array(g["sphere_texture"]), np.array(g["plane_texture"])
    if not textured:
        st, pt = np.full_like(st, -1), np.full_like(pt, -1)
    return recs, st, pt, g["texels"]


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def by_hand(rgb, d, N, Ld, col, e, lamb_n, spec, spec_n, shin, occluded):
    """The header's per-light arithmetic for one trace in Python floats."""
    rgb = [float(v) for v in rgb]
    cN = float(Ld[0]) * float(N[0]) + float(Ld[1]) * float(N[1]) + float(Ld[2]) * float(N[2])
    k = lamb_n * cN
    wantL, wantS = k > 0, spec > 0 and cN > 0
    if not (wantL or wantS) or occluded:
        return rgb
    if wantL:
        rgb = [rgb[c] + ((k * float(e[c])) * float(col[c])) for c in range(3)]
    if wantS:
        Hs = [float(Ld[c]) + (-float(d[c])) for c in range(3)]
        nrm = math.sqrt(Hs[0] * Hs[0] + Hs[1] * Hs[1] + Hs[2] * Hs[2])
        if nrm == 0.0:
            return rgb                                             # s is NaN: no highlight
        H = [Hs[c] / nrm for c in range(3)]
        s = float(N[0]) * H[0] + float(N[1]) * H[1] + float(N[2]) * H[2]
        if s > 0:
            q = s
            for _ in range(int(math.log2(shin))):
                q = q * q
            a = spec_n * q
            rgb = [rgb[c] + (a * float(e[c])) for c in range(3)]
    return rgb


N_UP = np.array([0.0, 0.0, 1.0])
D_IN = unit([1.0, 0.0, -1.0])
L_UP = unit([0.3, 0.2, 1.0])
COL = np.array([200.0, 100.0, 50.0])
RGB0 = np.array([10.0, 20.0, 30.0])


@pytest.mark.parametrize("shin", SHININESS)
def test_every_shininess_by_hand(shin):
    e = np.array([0.5, 1.0, 2.0], np.float32)
    got = light_terms(RGB0, D_IN, N_UP, L_UP, COL, e, 0.6, 120.0, 120.0, shin, False)
    want = by_hand(RGB0, D_IN, N_UP, L_UP, COL, e, 0.6, 120.0, 120.0, shin, False)
    assert got.tolist() == want
    # the power is log2(shin) squarings of s = dot(N, H)
    H = unit(L_UP - D_IN)
    s = float(N_UP[0] * H[0] + N_UP[1] * H[1] + N_UP[2] * H[2])
    q = s
    for _ in range(squarings(shin)):
        q = q * q
    lam = 0.6 * float(L_UP[2])
    assert got[1] == (20.0 + (lam * 1.0) * 100.0) + (120.0 * q) * 1.0
    assert 2 ** squarings(shin) == shin


def test_cases_without_a_highlight():
    e = (1.0, 1.0, 1.0)
    lam = [RGB0[c] + (0.6 * float(L_UP[2])) * COL[c] for c in range(3)]
    # s <= 0: the surface is met from behind (d.N > 0) and the light grazes it
    graze, d_back = unit([1.0, 0.0, 0.05]), unit([0.0, 0.3, 1.0])
    got = light_terms(RGB0, d_back, N_UP, graze, COL, e, 0.0, 50.0, 50.0, 4, False)
    assert got.tolist() == RGB0.tolist()
    cN, k, wantL, wantS = light_wants(graze, N_UP, 0.0, 50.0)
    assert cN > 0 and not wantL and wantS
    # a zero half vector (the light straight behind the ray): s is NaN, the Lambert term stays
    got = light_terms(RGB0, L_UP, N_UP, L_UP, COL, e, 0.6, 50.0, 50.0, 4, False)
    assert got.tolist() == lam
    # occluded, spec = 0, and a light below the horizon
    assert light_terms(RGB0, D_IN, N_UP, L_UP, COL, e, 0.6, 50.0, 50.0, 4, True).tolist() == RGB0.tolist()
    assert light_terms(RGB0, D_IN, N_UP, L_UP, COL, e, 0.6, 0.0, 0.0, 1024, False).tolist() == lam
    assert light_terms(RGB0, D_IN, N_UP, -L_UP, COL, e, 0.6, 50.0, 50.0, 4, False).tolist() == RGB0.tolist()
    # a negative lamb: k <= 0 with cN > 0 leaves the highlight alone
    got = light_terms(RGB0, D_IN, N_UP, L_UP, COL, e, -0.4, 50.0, 25.0, 2, False)
    assert got.tolist() == by_hand(RGB0, D_IN, N_UP, L_UP, COL, e, -0.4, 50.0, 25.0, 2, False) and got[0] > RGB0[0]
    # NaN compares false everywhere
    assert light_terms(RGB0, D_IN, N_UP, np.full(3, np.nan), COL, e, 0.6, 50.0, 50.0, 4, False).tolist() == RGB0.tolist()


def test_light_colour_scales_both_terms():
    white = light_terms(np.zeros(3), D_IN, N_UP, L_UP, COL, (1.0, 1.0, 1.0), 0.5, 64.0, 64.0, 8, False)
    plain = [(0.5 * float(L_UP[2])) * COL[c] for c in range(3)]
    # e = (2, 2, 2) with lamb halved is the white light's Lambert term (a power of two: exact), and twice its highlight
    twice = light_terms(np.zeros(3), D_IN, N_UP, L_UP, COL, (2.0, 2.0, 2.0), 0.25, 64.0, 64.0, 8, False)
    hl = [white[c] - plain[c] for c in range(3)]
    assert np.allclose(twice, [plain[c] + 2 * hl[c] for c in range(3)], rtol=1e-15)
    red = light_terms(np.zeros(3), D_IN, N_UP, L_UP, COL, (1.0, 0.0, 0.0), 0.5, 64.0, 64.0, 8, False)
    assert red[0] == white[0] and red[1] == 0.0 and red[2] == 0.0
    black = light_terms(RGB0, D_IN, N_UP, L_UP, COL, (0.0, 0.0, 0.0), 0.5, 64.0, 64.0, 8, False)
    assert black.tolist() == RGB0.tolist()
    # vectorised over traces, with per-trace coefficients
    many = light_terms(np.tile(RGB0, (4, 1)), np.tile(D_IN, (4, 1)), np.tile(N_UP, (4, 1)), np.tile(L_UP, (4, 1)), np.tile(COL, (4, 1)),
                       (0.3, 1.0, 4.0), np.array([0.6, 0.0, -0.2, 0.6]), np.array([10.0, 20.0, 0.0, 30.0]),
                       np.array([5.0, 10.0, 0.0, 15.0]), np.array([1, 1024, 16, 2]), np.array([False, False, False, True]))
    for i, (lamb, sp, sn, sh, oc) in enumerate([(0.6, 10.0, 5.0, 1, False), (0.0, 20.0, 10.0, 1024, False), (-0.2, 0.0, 0.0, 16, False),
                                               (0.6, 30.0, 15.0, 2, True)]):
        assert many[i].tolist() == by_hand(RGB0, D_IN, N_UP, L_UP, COL, (0.3, 1.0, 4.0), lamb, sp, sn, sh, oc)


def test_material_and_light_validation():
    assert Material(0.1, 0.5, 0.2).specular == 0.0 and Material(0.1, 0.5, 0.2).shininess == 1
    for shin in SHININESS:
        assert Material(0.1, 0.5, 0.2, specular=3.0, shininess=shin).glossy
    assert Material(0.0, 0.1, 0.0, transparency=0.9, ior=1.5, specular=10.0, shininess=64).key8()[6:] == (10.0, 64.0)
    assert Material(0.0, 0.1, 0.3, roughness=0.4, specular=10.0, shininess=2).glossy
    for bad in (dict(specular=-1.0), dict(specular=float("nan")), dict(specular=float("inf")), dict(specular=1.0, shininess=3),
                dict(shininess=0), dict(shininess=2048), dict(shininess=1.5), dict(shininess=-2)):
        with pytest.raises(ValueError):
            Material(0.1, 0.5, 0.2, **bad)
    li = Light([0, 0, 1])
    assert li.rgb().dtype == np.float32 and li.rgb().tolist() == [1.0, 1.0, 1.0] and li.radius == 0.0
    assert Light([0, 0, 1], 0.5, (1.0, 0.5, 0.25), 2.0).rgb().tolist() == [2.0, 1.0, 0.5]
    assert Light([0, 0, 1], color=(0.1, 0.2, 0.3), intensity=3.0).rgb().tolist() == \
        (3.0 * np.array([0.1, 0.2, 0.3])).astype(np.float32).tolist()
    for bad in (dict(color=(1.0, -0.1, 0.0)), dict(color=(1.0, float("nan"), 0.0)), dict(intensity=float("inf")),
                dict(intensity=-1.0), dict(color=(1.0, 1.0)), dict(color=(1e30, 1.0, 1.0), intensity=1e30)):
        with pytest.raises(ValueError):
            Light([0, 0, 1], **bad)


def test_generate_materials_has_eight_columns_only_when_needed():
    sc = Scene.default_scene()
    table, sid, pid = sc.generate_materials(Material(0.05, 0.8, 0.0))
    assert table.shape == (1, 3)
    sc.spheres[1].material = Material(0.0, 0.3, 0.5, roughness=0.2)
    assert sc.generate_materials(Material(0.05, 0.8, 0.0))[0].shape == (2, 6)
    sc.spheres[2].material = Material(0.0, 0.3, 0.5, roughness=0.2, specular=0.0, shininess=64)     # spec 0: not glossy
    assert sc.generate_materials(Material(0.05, 0.8, 0.0))[0].shape[1] == 6
    sc.spheres[0].material = Material(0.02, 0.1, 0.0, transparency=0.9, ior=1.5, specular=150.0, shininess=128)
    sc.spheres[3].material = Material(0.02, 0.1, 0.0, transparency=0.9, ior=1.5, specular=150.0, shininess=128)
    table, sid, pid = sc.generate_materials(Material(0.05, 0.8, 0.0))
    assert table.shape == (4, 8) and table.dtype == np.float64
    assert table[sid[0]].tolist() == [0.02, 0.1, 0.0, 0.9, 1.5, 0.0, 150.0, 128.0] and sid[0] == sid[3]
    assert table[sid[1]].tolist() == [0.0, 0.3, 0.5, 0.0, 1.0, 0.2, 0.0, 1.0]
    assert table[sid[2]].tolist() == [0.0, 0.3, 0.5, 0.0, 1.0, 0.2, 0.0, 64.0]
    assert table[pid[0]].tolist() == [0.05, 0.8, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0]


def test_get_light_colors():
    sc = Scene.default_scene()
    assert sc.get_light_colors().dtype == np.float32 and sc.get_light_colors().tolist() == [[1.0, 1.0, 1.0]] * 3
    sc.lights[0] = Light(sc.lights[0].origin, color=(1.0, 0.8, 0.6), intensity=1.5)
    sc.lights[2] = Light(sc.lights[2].origin, 0.4, (0.0, 0.0, 1.0), 0.25)
    want = np.array([1.5 * np.array([1.0, 0.8, 0.6]), [1.0, 1.0, 1.0], [0.0, 0.0, 0.25]]).astype(np.float32)
    assert np.array_equal(sc.get_light_colors(), want) and sc.get_light_colors().shape == (3, 3)
    assert sc.get_light_radii().tolist() == [0.0, 0.0, np.float32(0.4)]
    assert sc.get_lights().shape == (3, 3)                                    # the positions are as before
    assert Scene([], [], [Plane([0, 0, 0], [0, 0, 1], (1, 2, 3))]).get_light_colors().shape == (0, 3)
    assert Sphere([0, 0, 0], 1.0, (1, 2, 3)).texture is None


def test_binding_declares_the_entry_point():
    from python_ray_tracer_amd import _lib as L
    assert "rt_set_scene_lighting" in L.PROTOTYPES
    tex, lit = L.PROTOTYPES["rt_set_scene_textures"], L.PROTOTYPES["rt_set_scene_lighting"]
    assert lit[0] is tex[0] and lit[1][:-1] == tex[1] and len(lit[1]) == len(tex[1]) + 1
    assert L.RT_ABI_VERSION == 7
    hdr = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    assert "int rt_set_scene_lighting(" in hdr
    for line in ("cN = dot(Ld, N)", "= lamb_n * cN", "wantL = k > 0;  wantS = spec > 0 and cN > 0",
                 "rgb_c = rgb_c + ((k * e_c) * col_c)", "rgb_c = rgb_c + (a * e_c)"):
        assert line in hdr and line in light_terms.__doc__, line


def test_all_fixtures_exist():
    assert set(lighting_cases()) == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_fixture_is_self_consistent(case, oracle):
    g = load_lighting(case)
    S, P, NL = g["spheres"].shape[1], g["planes"].shape[1], g["lights"].shape[1]
    n = len(g["coords"])
    assert g["rgb64"].shape == (n, 3) and g["u8"].shape == (n, 3) and g["u8_plain"].shape == (n, 3)
    assert g["u8"].dtype == np.uint8 and g["rgb64"].dtype == np.float64
    e, t = g["light_rgb"], g["materials"]
    assert e.dtype == np.float32 and e.shape == (NL, 3) and np.isfinite(e).all() and (e >= 0).all()
    assert t.shape[1] == 8 and t.shape[0] > g["sphere_material"].max() and t.shape[0] > g["plane_material"].max()
    assert (t[:, 6] >= 0).all() and all(float(v) in [float(s) for s in SHININESS] for v in t[:, 7])
    assert (e != 1.0).any() or (t[:, 6] > 0).any()                # the scene runs the lighting kernels
    assert g["sphere_texture"].shape == (S,) and g["plane_texture"].shape == (P,) and g["light_radius"].shape == (NL,)
    want = np.clip(np.rint(g["rgb64"]), 0, 255).astype(np.uint8)[:, [0, 2, 1]]
    assert np.array_equal(g["u8"], want)
    differ = int((g["u8"] != g["u8_plain"]).any(axis=1).sum())
    assert 4 * differ >= n, f"only {differ} of {n} pixels differ from the white-light, spec = 0 scene"
    ev = dict(zip(EVENTS, g["events"].tolist()))
    if case == "grazing_48_d2":
        assert min(ev.values()) >= 8, ev
        assert ((t[:, 1] == 0) & (t[:, 6] > 0)).any() and (t[:, 1] < 0).any()
    if case == "shin_extremes_32_d1":
        assert {1.0, 1024.0} <= set(t[t[:, 6] > 0, 7].tolist()) and (t[:, 6] == 0).any()
        assert {0.0, np.float32(0.3), 4.0} <= set(e.reshape(-1).tolist())
    if case == "everything_48_d4":
        assert (g["light_radius"] > 0).any() and float(g["aperture"]) > 0 and (t[:, 3] > 0).any() and (t[:, 5] > 0).any()
        assert len(g["tex_first"]) > 0
    size = os.path.getsize(os.path.join(GOLDEN, f"lighting_{case}.npz"))
    assert size <= os.path.getsize(os.path.join(GOLDEN, "lens_c4_s64_d5_sub32.npz")) and size < 1 << 20
    # white lights and spec = 0: the CPU oracle's frame of the scene, every sampled pixel, the two textured fixtures included
    # (test_regenerate_sampled_pixels below recomputes them with the reference as well).
    assert (len(g["tex_first"]) > 0) == (case in TEXTURED)
    tex = None
    if case in TEXTURED:
        tex = ([(g["tex_origin"][k], g["tex_axes"][k], g["tex_dims"][k], int(g["tex_first"][k])) for k in range(len(g["tex_first"]))],
               g["sphere_texture"], g["plane_texture"], g["texels"])
    w, h = int(g["w"]), int(g["h"])
    u8, _ = oracle.render_pixels(w, h, g["coords"], g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"],
                                 0.0, 0.0, 0.0, int(g["depth"]), int(g["aa"]), raygen=raygen_closed_form(w, h, float(g["fov"])),
                                 spp=int(g["spp"]) if "spp" in g else 0, seed=int(g["seed"]),
                                 materials=(np.ascontiguousarray(t[:, :6]), g["sphere_material"], g["plane_material"]),
                                 light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]),
                                 lens=(float(g["aperture"]), float(g["focus_distance"])), textures=tex)
    assert np.array_equal(u8, g["u8_plain"])


from test_textures import REFERENCE  # noqa: E402  (where the reference checkout lies, as the texture test has it)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not present")
@pytest.mark.parametrize("case", ["default_64_d4", "everything_48_d4", "grazing_48_d2", "shin_extremes_32_d1"])
def test_regenerate_sampled_pixels(case):
    """The fixture's lit colours (rgb64 and u8, bit for bit) and its u8_plain on 64 sampled pixels; the white-light pass also
    compares every trace of the restatement with the reference's own trace()."""
    import multiprocessing as mp
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gen_lighting_golden as gl
    from oracle import gen_golden as gg
    from python_ray_tracer_amd import workloads
    g = load_lighting(case)
    args, tex, light_rgb, kw = gl.scenes(gg, workloads)[case]
    assert (tex is not None) == (case in TEXTURED)
    pick = np.random.default_rng(7).choice(len(g["coords"]), 64, replace=False)
    kw = {**kw, "coords": g["coords"][pick]}
    mods = gg._import_reference()
    with mp.Pool(2, initializer=gl._init) as pool:
        d, render = gl.render_pixels(pool, 2, mods, *args, tex, light_rgb, **kw)
        rgb64, u8, _ = render(True)
        _, u8p, _ = render(False)
    assert np.array_equal(d["light_rgb"], g["light_rgb"]) and np.array_equal(d["materials"], g["materials"])
    assert np.array_equal(rgb64.view(np.uint64), g["rgb64"][pick].view(np.uint64))
    assert np.array_equal(u8, g["u8"][pick]) and np.array_equal(u8p, g["u8_plain"][pick])
