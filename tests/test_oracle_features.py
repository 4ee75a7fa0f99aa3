"""The CPU oracle's feature path (oracle/rt_oracle.c orc_render_ex: per-object materials, refraction, scatter, area lights, the
thin lens, textures, lighting and the sky, restated from include/mi355rt.h) pinned to EVERY pixel of every feature fixture
(tests/golden/{materials,refraction,scatter,soft,lens,texture,lighting,sky}_*.npz, made around the reference's own trace() by
tools/gen_*_golden.py): uint8 and float64, bit for bit, the fixtures' second outputs (u8_plain, u8_pinhole, u8_point and the
second sky's u8_b / rgb64_b) included.  Each deliberately wrong restatement (oracle.WRONG) fails at least one fixture, the
oracle refuses what the header refuses, and its leaf arithmetic (orc_texel_index, orc_light_terms, orc_sky_color) equals the
numpy restatements of the package (scene.texel_index, scene.lighting.light_terms, scene.sky.sky_color) bit for bit."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame, raygen_closed_form

FAMILIES = ("materials", "refraction", "scatter", "soft", "lens", "texture", "lighting", "sky")


def feature_cases():
    return sorted(os.path.basename(p)[:-len(".npz")] for f in FAMILIES for p in glob.glob(os.path.join(GOLDEN, f"{f}_*.npz")))


def _records(g):
    return [(g["tex_origin"][k], g["tex_axes"][k], g["tex_dims"][k], int(g["tex_first"][k])) for k in range(len(g["tex_first"]))]


def _render(oracle, g, wrong=0, **over):
    w, h = int(g["w"]), int(g["h"])
    kw = dict(materials=(g["materials"], g["sphere_material"], g["plane_material"]), spp=int(g["spp"]) if "spp" in g else 0,
              seed=int(g["seed"]) if "seed" in g else 1)
    if "light_radius" in g:
        kw.update(light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]))
    if "aperture" in g:
        kw.update(lens=(float(g["aperture"]), float(g["focus_distance"])))
    if "tex_first" in g and len(g["tex_first"]):
        kw.update(textures=(_records(g), g["sphere_texture"], g["plane_texture"], g["texels"]))
    if "light_rgb" in g:
        kw.update(light_rgb=g["light_rgb"])
    if "sky" in g:
        kw.update(sky=g["sky"])
    kw.update(over)
    # amb, lamb and refl of the call are not read for a scene with a table
    return oracle.render_pixels(w, h, g["coords"], g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"],
                                7.0, -3.0, 2.0, int(g["depth"]), int(g["aa"]), raygen=raygen_closed_form(w, h, float(g["fov"])),
                                wrong=wrong, **kw)


def test_every_family_has_fixtures():
    cases = feature_cases()
    assert len(cases) >= 68
    for f in FAMILIES:
        assert any(c.startswith(f + "_") for c in cases), f


@pytest.mark.parametrize("case", feature_cases())
def test_fixture_every_pixel(oracle, case):
    g = np.load(os.path.join(GOLDEN, f"{case}.npz"))
    u8, f64 = _render(oracle, g)
    bad = (u8 != g["u8"]).any(axis=1)
    assert not bad.any(), f"uint8: {int(bad.sum())} of {len(bad)} pixels differ, e.g. {g['coords'][bad][:4].tolist()}"
    bad = (f64.view(np.uint64) != g["rgb64"].view(np.uint64)).any(axis=1)
    assert not bad.any(), (f"float64: {int(bad.sum())} of {len(bad)} pixels differ, e.g. {g['coords'][bad][:4].tolist()}: "
                           f"{f64[bad][:2].tolist()} != {g['rgb64'][bad][:2].tolist()}")
    if "u8_pinhole" in g:                                      # the same pixels with aperture 0
        u8p, _ = _render(oracle, g, lens=(0.0, float(g["focus_distance"])))
        assert np.array_equal(u8p, g["u8_pinhole"])
        assert not np.array_equal(u8p, u8)
    if "u8_point" in g:                                        # the same pixels with every radius 0
        u8p, _ = _render(oracle, g, light_radius=np.zeros_like(g["light_radius"]))
        assert np.array_equal(u8p, g["u8_point"])
        assert not np.array_equal(u8p, u8)
    if "u8_plain" in g:                                        # the same pixels with the family's feature off
        family = case.split("_")[0]
        if family == "texture":                                # every texture id -1
            off = dict(textures=None)
        elif family == "lighting":                             # white lights and spec = 0 (the textures stay)
            off = dict(light_rgb=None, materials=(np.ascontiguousarray(g["materials"][:, :6]), g["sphere_material"], g["plane_material"]))
        else:                                                  # no sky (the same lights and materials)
            off = dict(sky=None)
        u8p, _ = _render(oracle, g, **off)
        assert np.array_equal(u8p, g["u8_plain"])
        assert not np.array_equal(u8p, u8)
    if "sky_b" in g:                                           # the same scene under the fixture's second sky
        u8b, f64b = _render(oracle, g, sky=g["sky_b"])
        assert np.array_equal(u8b, g["u8_b"]) and np.array_equal(f64b.view(np.uint64), g["rgb64_b"].view(np.uint64))
        assert not np.array_equal(u8b, u8)


# Each wrong restatement, and fixtures it must fail (float64 bits or uint8).
TEETH = {
    "key_pixel": ("scatter_default_64_d4", "soft_aa_48_d2", "lens_aa_48_d2"),
    "pow_weight": ("materials_default_64_d3", "refraction_default_64_d4"),
    "soft_i_major": ("soft_default_64_d4", "soft_mixed_32_n16_d2"),
    "lamb_whole": ("soft_default_64_d4",),
    "tir_far": ("refraction_overlap_48_d5",),
    "no_bounce": ("scatter_default_64_d4",),
    "focus_f": ("lens_default_64_d4",),
    "no_absorb": ("scatter_grazing_48_d3",),
    "tex_biased": ("texture_aa_48_d2", "texture_default_64_d4", "lighting_default_64_d4"),
    "tex_trunc": ("texture_wrap_33_d2", "texture_inside_32_d3", "texture_c5_s256_d8_sub96", "sky_everything_48_d4"),
    "spec_texel": ("lighting_default_64_d4", "lighting_shin_extremes_32_d1", "sky_events_48_d4"),
    "spec_whole": ("lighting_everything_48_d4", "sky_everything_48_d4"),
    "sun_first": ("sky_default_64_d4", "sky_events_48_d4", "sky_spheres_only_32_d3"),
    "sky_flat": ("sky_default_64_d4", "sky_sharp_extremes_32_d1", "sky_spheres_only_32_d3"),
    "lamb_order": ("lighting_default_64_d4", "lighting_grazing_48_d2", "sky_aa_48_d2"),
}


@pytest.mark.parametrize("wrong", sorted(TEETH))
def test_wrong_restatements_fail_the_fixtures(oracle, wrong):
    assert set(TEETH) == set(oracle.WRONG)
    for case in TEETH[wrong]:
        g = np.load(os.path.join(GOLDEN, f"{case}.npz"))
        u8, f64 = _render(oracle, g, wrong=oracle.WRONG[wrong])
        n = int((f64.view(np.uint64) != g["rgb64"].view(np.uint64)).any(axis=1).sum())
        assert n > 0, f"{wrong} passes {case}"


def test_no_features_is_the_plain_path(oracle):
    """orc_render_ex without a table, a radius or a lens is orc_render (same bytes); a uniform power-of-two table is the
    scalars' frame (mi355rt.h rt_set_scene_materials).  T == 0 or every id -1, white lights with spec = 0 and a NULL or
    all-black sky are the same bytes again (rt_set_scene_textures, _lighting, _sky), shadow-query counters included."""
    g = load_frame("default_128_d3")
    w, h = int(g["w"]), int(g["h"])
    args = (w, h, g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], 0.05, 0.6, 0.5, 3)
    kw = dict(raygen=raygen_closed_form(w, h, float(g["fov"])), want=("u8", "f64"))
    S, P = g["spheres"].shape[1], g["planes"].shape[1]
    for aa, spp in ((0, 0), (1, 0), (2, 3)):
        ref = oracle.render(*args, aa, spp=spp, **kw)
        a = oracle.render(*args, aa, spp=spp, light_radius=np.zeros(g["lights"].shape[1]), lens=(0.0, 2.0), **kw)
        b = oracle.render(*args, aa, spp=spp, materials=(np.array([[0.05, 0.6, 0.5]]), np.zeros(S), np.zeros(P)), **kw)
        for o in (a, b):
            assert o["u8"].tobytes() == ref["u8"].tobytes() and o["f64"].tobytes() == ref["f64"].tobytes(), aa
    # a feature scene: no texture in use, white lights, spec = 0, a black sky
    g = np.load(os.path.join(GOLDEN, "texture_everything_48_d4.npz"))
    NL, M = g["lights"].shape[1], len(g["materials"])
    plain = _render(oracle, g, textures=None)
    assert np.array_equal(plain[0], g["u8_plain"])
    t8 = np.concatenate([g["materials"], np.zeros((M, 1)), np.full((M, 1), 1024.0)], axis=1)   # spec 0, any shin
    black = np.zeros(24)
    black[[2, 13]], black[12], black[16], black[23] = 1.0, 16.0, -1.0, 512.0
    none = (np.full(g["spheres"].shape[1], -1), np.full(g["planes"].shape[1], -1))
    for kw in (dict(textures=([], *none, np.zeros((0, 3)))),
               dict(textures=(_records(g), *none, g["texels"])),
               dict(textures=None, light_rgb=np.ones((NL, 3))),
               dict(textures=None, materials=(t8, g["sphere_material"], g["plane_material"])),
               dict(textures=None, sky=black),
               dict(textures=(_records(g), *none, g["texels"]), light_rgb=np.ones((NL, 3)), sky=black,
                    materials=(t8, g["sphere_material"], g["plane_material"]))):
        o = _render(oracle, g, **kw)
        assert o[0].tobytes() == plain[0].tobytes() and o[1].tobytes() == plain[1].tobytes(), sorted(kw)
    w, h = int(g["w"]), int(g["h"])                            # (whole frames: the counters of the queries asked)
    args = (w, h, g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], 0.0, 0.0, 0.0, int(g["depth"]), 0)
    base = dict(raygen=raygen_closed_form(w, h, float(g["fov"])), seed=int(g["seed"]), light_radius=g["light_radius"],
                shadow_samples=int(g["shadow_samples"]), materials=(g["materials"], g["sphere_material"], g["plane_material"]))
    ref = oracle.render(*args, **base)
    o = oracle.render(*args, **{**base, "materials": (t8, g["sphere_material"], g["plane_material"])}, sky=black,
                      light_rgb=np.ones((NL, 3)), textures=(_records(g), *none, g["texels"]))
    assert o["u8"].tobytes() == ref["u8"].tobytes() and o["f64"].tobytes() == ref["f64"].tobytes() and o["counters"] == ref["counters"]


def test_refuses_what_the_header_refuses(oracle):
    g = np.load(os.path.join(GOLDEN, "soft_glass_rough_48_d4.npz"))
    table = np.array(g["materials"])
    bad = []
    t = table.copy(); t[4, 5] = 0.5; t[4, 3] = 0.9; bad.append(dict(materials=(t, g["sphere_material"], g["plane_material"])))  # rough glass
    t = table.copy(); t[0, 3] = 0.5; t[0, 2] = 0.3; bad.append(dict(materials=(t, g["sphere_material"], g["plane_material"])))  # refl + trans
    t = table.copy(); t[0, 5] = 1.5; bad.append(dict(materials=(t, g["sphere_material"], g["plane_material"])))                # rough > 1
    t = table.copy(); t[0, 4] = 0.0; bad.append(dict(materials=(t, g["sphere_material"], g["plane_material"])))                # ior 0
    t = table.copy(); t[0, 0] = np.nan; bad.append(dict(materials=(t, g["sphere_material"], g["plane_material"])))             # NaN
    bad.append(dict(materials=(table[:, :4], g["sphere_material"], g["plane_material"])))                                       # 4 columns
    sid = np.array(g["sphere_material"]); sid[0] = len(table); bad.append(dict(materials=(table, sid, g["plane_material"])))  # bad id
    bad.append(dict(materials=(np.zeros((257, 3)), np.zeros(6), np.zeros(1))))                                                 # M > 256
    bad.append(dict(shadow_samples=17)); bad.append(dict(shadow_samples=0))
    bad.append(dict(light_radius=np.array([0.5, -0.1, 0.0]))); bad.append(dict(light_radius=np.array([0.5, np.inf, 0.0])))
    bad.append(dict(lens=(-0.1, 1.0))); bad.append(dict(lens=(0.1, 0.0))); bad.append(dict(lens=(np.nan, 1.0)))
    for b in bad:
        with pytest.raises(ValueError):
            _render(oracle, g, **b)
    w, h = int(g["w"]), int(g["h"])                            # area lights or a lens without a table
    args = (w, h, g["coords"][:4], g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], 0.0, 0.6, 0.3, 2, 0)
    for kw in (dict(light_radius=g["light_radius"]), dict(lens=(0.1, 2.0))):
        with pytest.raises(ValueError):
            oracle.render_pixels(*args, raygen=raygen_closed_form(w, h, 45.0), **kw)
    # textures, lighting and the sky (mi355rt.h rt_set_scene_textures, _lighting, _sky)
    g = np.load(os.path.join(GOLDEN, "sky_everything_48_d4.npz"))
    g = {k: g[k] for k in g.files}
    g["coords"] = g["coords"][:8]
    S, P, NL, T, NT = g["spheres"].shape[1], g["planes"].shape[1], g["lights"].shape[1], len(g["tex_first"]), len(g["texels"])
    assert T >= 1 and g["materials"].shape[1] == 8
    _render(oracle, g)                                          # (the scene itself is accepted)
    recs, tsid, tpid, texels = _records(g), g["sphere_texture"], g["plane_texture"], g["texels"]
    mats = lambda t: dict(materials=(t, g["sphere_material"], g["plane_material"]))

    def rec(k, **ch):
        r = [list(x) for x in recs]
        for key, v in ch.items():
            r[k][dict(origin=0, axes=1, dims=2, first=3)[key]] = v
        return dict(textures=([tuple(x) for x in r], tsid, tpid, texels))
    cells = int(np.prod(recs[0][2]))
    bad = []
    i = np.array(tsid); i[0] = T; bad.append(dict(textures=(recs, i, tpid, texels)))                   # id == T
    i = np.array(tpid); i[0] = -2; bad.append(dict(textures=(recs, tsid, i, texels)))                  # id < -1
    bad.append(dict(textures=([], tsid if (tsid >= 0).any() else np.zeros(S), tpid, texels)))           # T == 0 with an id in use
    bad.append(rec(0, dims=(0, 1, 1))); bad.append(rec(0, dims=(4097, 1, 1))); bad.append(rec(0, dims=(1, 1, -1)))
    bad.append(rec(0, first=-1)); bad.append(rec(0, first=NT - cells + 1))                             # one texel past the end
    bad.append(rec(0, first=NT + 1))
    bad.append(rec(0, origin=(0.0, np.nan, 0.0))); bad.append(rec(0, axes=np.array([[1, 0, 0], [0, np.inf, 0], [0, 0, 1.0]])))
    x = np.array(texels); x[-1, 2] = np.nan; bad.append(dict(textures=(recs, tsid, tpid, x)))           # a texel not finite
    bad.append(dict(textures=(recs * 65, tsid, tpid, texels)))                                          # T > 64
    e = np.array(g["light_rgb"]); e[0, 1] = -0.5; bad.append(dict(light_rgb=e))
    e = np.array(g["light_rgb"]); e[NL - 1, 2] = np.inf; bad.append(dict(light_rgb=e))
    e = np.array(g["light_rgb"]); e[0, 0] = np.nan; bad.append(dict(light_rgb=e))
    t = np.array(g["materials"])
    for col, v in ((6, -1.0), (6, np.nan), (6, np.inf), (7, 3.0), (7, 0.0), (7, 2048.0), (7, 0.5), (7, -2.0)):
        b = t.copy(); b[1, col] = v; bad.append(mats(b))
    bad.append(mats(t[:, :7]))                                                                          # 7 columns
    k = np.array(g["sky"])
    for at, v in ((0, np.nan), (16, np.inf), (3, -1.0), (8, -0.5), (19, -1e-9), (21, -1.0), (12, 3.0), (12, 32.0), (12, 0.0),
                  (23, 2048.0), (23, 0.0), (23, 12.0)):
        b = k.copy(); b[at] = v; bad.append(dict(sky=b))
    b = k.copy(); b[0:3] *= 1.0 + 1e-5; bad.append(dict(sky=b))                                         # |up|^2 = 1 + 2e-5
    b = k.copy(); b[13:16] *= 1.0 - 1e-5; bad.append(dict(sky=b))
    b = k.copy(); b[0:3] = 0.0; bad.append(dict(sky=b))
    bad.append(dict(sky=k[:23]))
    for b in bad:
        with pytest.raises(ValueError):
            _render(oracle, g, **b)
    b = k.copy(); b[0:3] *= 1.0 + 4e-7; _render(oracle, g, sky=b)                                       # inside 1 +- 1e-6
    # a texture, a coloured light, spec > 0 or a sky without a table
    w, h = int(g["w"]), int(g["h"])
    args = (w, h, g["coords"][:4], g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], 0.0, 0.6, 0.3, 2, 0)
    rg = raygen_closed_form(w, h, 45.0)
    for kw in (dict(textures=(recs, tsid, tpid, texels)), dict(light_rgb=g["light_rgb"]), dict(sky=g["sky"])):
        with pytest.raises(ValueError):
            oracle.render_pixels(*args, raygen=rg, **kw)
    white = oracle.render_pixels(*args, raygen=rg, light_rgb=np.ones((NL, 3)), sky=np.where(np.isin(np.arange(24), (2, 12, 13, 23)), 1.0, 0.0))
    assert white[1].tobytes() == oracle.render_pixels(*args, raygen=rg)[1].tobytes()     # white lights and a black sky: the scalars' frame


def test_leaf_texel_index_equals_numpy(oracle):
    """orc_texel_index against scene.texel_index: seeded random records and points, exact multiples and cell boundaries, both
    clamps, NaN, skewed axes and axes with dim == 1 (not evaluated: a NaN-producing axis there changes nothing)."""
    from python_ray_tracer_amd.scene.texture import texel_index
    rng = np.random.default_rng(11)
    n = 0
    for trial in range(60):
        dims = [int(rng.choice([1, 2, 3, 7, 64, 4095, 4096])) for _ in range(3)]
        first = int(rng.integers(0, 1000))
        origin = rng.uniform(-3, 3, 3) * float(rng.choice([1e-3, 1.0, 1e3]))
        axes = rng.normal(size=(3, 3)) * float(rng.choice([1e-2, 1.0, 37.0, 1e4]))
        if trial % 4 == 0:
            axes = np.diag(rng.choice([0.5, 1.0, 2.0, 4.0], 3))          # exact arithmetic: the boundaries below are hit exactly
            origin = rng.integers(-4, 5, 3).astype(np.float64)
        pts = rng.uniform(-50, 50, (40, 3))
        cells = rng.integers(-9000, 9000, (40, 3)).astype(np.float64)
        edge = origin + cells / np.where(np.diag(axes) != 0, np.diag(axes), 1.0)     # exact multiples on the diagonal records
        pts = np.concatenate([pts, edge, np.nextafter(edge, -np.inf), np.nextafter(edge, np.inf), origin[None, :], -pts[:3] * 0.0])
        got = oracle.texel_index(pts, origin, axes, dims, first)
        want = texel_index(pts, origin, axes, dims, first)
        assert np.array_equal(got, want), (trial, dims)
        assert (got >= first).all() and (got < first + dims[0] * dims[1] * dims[2]).all()
        n += len(pts)
    # the clamps and NaN: g = +-2^30 - 1, +-2^30, +-2^30 + 1, beyond int64, infinite and NaN, on each axis in turn
    for a in range(3):
        for dim in (2, 3, 7, 4096):
            dims = [1, 1, 1]; dims[a] = dim
            axes = np.zeros((3, 3)); axes[a, 0] = 1.0
            xs = np.array([-2.0 ** 30 - 2, -2.0 ** 30 - 1, -2.0 ** 30 - 0.5, -2.0 ** 30, -2.0 ** 30 + 1, 2.0 ** 30 - 2, 2.0 ** 30 - 1,
                           2.0 ** 30 - 0.5, 2.0 ** 30, 2.0 ** 30 + 1, 1e19, -1e19, 1e300, -1e300, -0.0, 0.0, -1e-300, 1 - 2.0 ** -53])
            pts = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], axis=1)
            got, want = oracle.texel_index(pts, (0, 0, 0), axes, dims, 5), texel_index(pts, (0, 0, 0), axes, dims, 5)
            assert np.array_equal(got, want), (a, dim)
            stride = [1, 1, 1][a]
            assert got[1] == 5 + stride * ((-2 ** 30) % dim) and got[0] == got[1] and got[8] == 5 + stride * ((2 ** 30 - 1) % dim) == got[10]
            big = np.array([[1e308, 1e308, 0.0]])                       # g = inf - inf = NaN takes -2^30
            ax = np.zeros((3, 3)); ax[a] = (1e308, -1e308, 0.0)
            got, want = oracle.texel_index(big, (0, 0, 0), ax, dims, 0), texel_index(big, (0, 0, 0), ax, dims, 0)
            assert got[0] == want[0] == (-2 ** 30) % dim
            dims1 = [dim, dim, dim]; dims1[a] = 1                       # dim == 1: that axis is not evaluated
            ax = np.eye(3); ax[a] = (1e308, -1e308, 0.0)
            p = np.array([[1e300, 1e300, 3.5], [2.5, 1.5, 0.5]])
            assert np.array_equal(oracle.texel_index(p, (0, 0, 0), ax, dims1, 0), texel_index(p, (0, 0, 0), ax, dims1, 0))
    # the wrong restatement differs exactly on negative non-integral g
    pts = np.array([[-0.5, 0, 0], [-1.0, 0, 0], [0.5, 0, 0], [-2.25, 0, 0]])
    ok, tr = oracle.texel_index(pts, (0, 0, 0), np.eye(3), (4, 1, 1)), oracle.texel_index(pts, (0, 0, 0), np.eye(3), (4, 1, 1), wrong=oracle.WRONG["tex_trunc"])
    assert ok.tolist() == [3, 3, 0, 1] and tr.tolist() == [0, 3, 0, 2]
    assert n > 5000


def _units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def test_leaf_light_terms_equals_numpy(oracle):
    """orc_light_terms against scene.lighting.light_terms: every shin, spec 0 and > 0, lamb <= 0 with spec > 0, lights facing away,
    occluded queries, e with zeros and values above 1, spec / n for every n, Hs == 0 (Ld == d: NaN, no highlight) and s <= 0."""
    from python_ray_tracer_amd.scene.lighting import SHININESS, light_terms
    rng = np.random.default_rng(23)
    n = 2000
    rgb = rng.uniform(-5, 300, (n, 3))
    d, N, Ld = _units(rng, n), _units(rng, n), _units(rng, n)
    col = rng.integers(0, 256, (n, 3)).astype(np.float64)
    shin = rng.choice(SHININESS, n).astype(np.float64)
    shin[:11] = SHININESS
    ns = rng.integers(1, 17, n).astype(np.float64)
    lamb = rng.uniform(-0.3, 0.9, n) * (rng.uniform(size=n) < 0.85)
    spec = rng.uniform(0, 400, n) * (rng.uniform(size=n) < 0.7)
    spec[11:15] = (5e-324, 1e-320, 0.0, 1e6)                            # spec / n underflows to 0; no spec; a clipping one
    occ = rng.uniform(size=n) < 0.3
    Ld[20:30] = d[20:30]                                                # Hs == (0, 0, 0)
    Ld[30:40] = -N[30:40]                                               # cN < 0 exactly -1 to rounding
    N[40:50] = Ld[40:50]                                                # cN == 1 to rounding, d random
    d[50:60] = Ld[50:60] * 0.999999 + N[50:60] * 1e-9                   # a tiny Hs
    for e in ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (2.5, 0.0, np.float32(0.3)), (4.0, 1.0, 0.125)):
        want = light_terms(rgb, d, N, Ld, col, e, lamb / ns, spec, spec / ns, shin, occ)
        got = oracle.light_terms(rgb, d, N, Ld, col, e, lamb / ns, spec, spec / ns, shin, occ)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), e
    assert np.array_equal(got[20:30].view(np.uint64), light_terms(rgb[20:30], d[20:30], N[20:30], Ld[20:30], col[20:30], e,
                                                                  (lamb / ns)[20:30], 0.0, 0.0, 1.0, occ[20:30]).view(np.uint64))
    changed = (got != rgb).any(axis=1)
    assert changed.sum() > n // 5 and (~changed).sum() > n // 5
    # each exponent on one geometry: s, s^2, ..., s^1024 by squarings
    dd, NN, LL = np.array([[0.0, 0.0, -1.0]]), np.array([[0.0, 0.0, 1.0]]), np.array([[0.6, 0.0, 0.8]])
    for i, sh in enumerate(SHININESS):
        got = oracle.light_terms(np.zeros((1, 3)), dd, NN, LL, np.zeros((1, 3)), (1.0, 2.0, 0.0), 0.0, 10.0, 10.0, float(sh), False)
        H = np.array([0.6, 0.0, 1.8]) / np.sqrt(0.6 * 0.6 + 0.0 * 0.0 + 1.8 * 1.8)
        q = 0.0 * H[0] + 0.0 * H[1] + 1.0 * H[2]
        for _ in range(i):
            q = q * q
        assert got[0].tolist() == [10.0 * q, 10.0 * q * 2.0, 0.0], sh


def test_leaf_sky_color_equals_numpy(oracle):
    """orc_sky_color against scene.sky.sky_color: every sharp and halo_shin, directions along +-up, on the horizon (h = +-0.0),
    |h| > 1 by rounding and by length, s == sun_cos exactly, sun_cos above 1 and below -1."""
    from python_ray_tracer_amd.scene.sky import HALO_SHININESS, SHARPNESS, sky_color
    rng = np.random.default_rng(31)
    n = 600
    for trial, (sharp, shin) in enumerate([(s, h) for s in SHARPNESS for h in HALO_SHININESS]):
        up, sun = _units(rng, 1)[0], _units(rng, 1)[0]
        if trial % 5 == 0:
            up = np.array([0.0, 0.0, 1.0])
        k = np.zeros(24)
        k[0:3], k[13:16] = up, sun
        k[3:12] = rng.uniform(0, 255, 9)
        k[12], k[23] = sharp, shin
        k[17:23] = rng.uniform(0, 300, 6) * (rng.uniform(size=6) < 0.8)
        d = _units(rng, n)
        d[0], d[1], d[2], d[3] = up, -up, sun, -sun
        d[4], d[5] = up * 1.5, -up * (1 + 2.0 ** -52)                   # a > 1: t clamps to 1
        perp = np.cross(up, [0.3, -0.2, 0.9]); perp /= np.sqrt((perp * perp).sum())
        d[6], d[7] = perp, -perp                                        # the horizon
        d[8], d[9] = np.array([1.0, 0.0, -0.0]), np.array([-1.0, 0.0, 0.0])
        for cos in (float(rng.uniform(-1, 1)), 1.5, -1.5, 1.0, float((d[10] * sun).sum())):
            s10 = d[10, 0] * sun[0] + d[10, 1] * sun[1] + d[10, 2] * sun[2]
            k[16] = s10 if cos == float((d[10] * sun).sum()) else cos  # equal to the value direction 10 attains
            want, got = sky_color(d, k), oracle.sky_color(d, k)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (sharp, shin, cos)
        k[16] = s10
        on = oracle.sky_color(d[10:11], k)[0]
        k[16] = np.nextafter(s10, 2.0)
        off = oracle.sky_color(d[10:11], k)[0]
        assert (on == off + k[17:20]).all() or (k[17:20] == 0).all()   # s >= sun_cos holds at equality, and only the sun is added
    k = np.zeros(24)                                                    # h = -0.0 takes zenith with t = 0: exactly the horizon
    k[0:3], k[13:16], k[3:12], k[12], k[16], k[23] = (0, 0, 1), (0, 0, 1), (1, 2, 3, 40, 50, 60, 7, 8, 9), 4, 2.0, 1
    assert oracle.sky_color(np.array([1.0, 0.0, -0.0]), k).tolist() == [40.0, 50.0, 60.0]
    assert oracle.sky_color(np.array([0.0, 0.0, -1.0]), k).tolist() == [7.0, 8.0, 9.0]
    assert oracle.sky_color(np.array([0.0, 0.0, 3.0]), k).tolist() == [1.0, 2.0, 3.0]


def test_fixtures_reach_the_gaps(oracle):
    """Feature fixtures pin the oracle where the first ones did not reach (tools/gen_soft_shadow_golden.py): more than 8 lights
    with zero and nonzero radii and n = 16; a 256-row table with every row used and more than 256 spheres; depth 16 whose
    bounces 9 to 16 change the frame; 64 stochastic samples."""
    def load(case):
        return np.load(os.path.join(GOLDEN, f"{case}.npz"))
    g = load("soft_many_lights_24_n16_d2")
    r = g["light_radius"]
    assert g["lights"].shape[1] >= 9 and int(g["shadow_samples"]) == 16 and (r == 0).any() and (r > 0).sum() >= 6
    g = load("soft_table256_s324_32x24_d3")
    table = g["materials"]
    assert table.shape[0] == 256 and set(g["sphere_material"].tolist()) == set(range(256)) and g["spheres"].shape[1] >= 300
    assert (table[:, 3] > 0).any() and (table[:, 5] > 0).any()
    g = load("soft_deep16_32_d16")
    table = g["materials"]
    used = table[np.concatenate([g["sphere_material"], g["plane_material"]])]
    assert int(g["depth"]) == 16 and (used[:, 3] > 0).any() and (used[:, 5] > 0).any() and (used[:, 2] == 1.0).any()
    shallow, _ = _render(oracle, {**{k: g[k] for k in g.files}, "depth": 8})
    assert (shallow != g["u8"]).any(axis=1).sum() >= 100
    g = load("soft_spp64_16x12_d2")
    assert int(g["aa"]) == 2 and int(g["spp"]) == 64


def test_draw_lit_scenes(oracle):
    """tools/feature_scenes.draw_lit: draw(seed) underneath, unchanged; textures with shared texel ranges and ids of -1, coloured
    lights with zeros and values above 1, spec / shin columns with every exponent, a sky with every sharp; the oracle accepts each
    scene, and strip() / live() know the three features."""
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import feature_scenes as fs
    shins, sharps, kinds = set(), set(), set()
    above_one = black = no_tex = lamb0 = overlap = 0
    for seed in range(40):
        sc, plain = fs.draw_lit(seed), fs.draw(seed)
        for k, v in plain.items():
            if k != "table":
                assert np.array_equal(sc[k], v) if isinstance(v, np.ndarray) else sc[k] == v, (seed, k)
        assert np.array_equal(sc["table"][:, :6], plain["table"]) or (sc["table"][0, 1] <= 0 and np.array_equal(sc["table"][1:, :6], plain["table"][1:]))
        recs, st, pt, texels = sc["textures"]
        assert 1 <= len(recs) <= 4 and st.min() >= -1 and st.max() < len(recs) and (st >= 0).any()
        spans = sorted((r[3], r[3] + r[2][0] * r[2][1] * r[2][2]) for r in recs)
        assert all(0 <= a and b <= len(texels) for a, b in spans) and len(np.unique(texels, axis=0)) > 1
        overlap += any(spans[i + 1][0] < spans[i][1] for i in range(len(spans) - 1))
        no_tex += bool((st == -1).any())
        e = sc["light_rgb"]
        assert e.dtype == np.float32 and e.shape == (sc["lights"].shape[1], 3) and (e >= 0).all()
        above_one += bool((e > 1).any())
        black += bool((e == 0).any())
        t = sc["table"]
        assert t.shape[1] == 8 and (t[:, 6] >= 0).all() and (t[:, 6] > 0).any()
        lamb0 += bool(((t[:, 1] <= 0) & (t[:, 6] > 0)).any())
        shins |= set(t[:, 7].tolist())
        k = sc["sky"]
        assert abs(k[0:3] @ k[0:3] - 1) < 1e-12 and abs(k[13:16] @ k[13:16] - 1) < 1e-12 and k[16] < 1
        sharps.add(float(k[12]))
        kinds.add(sc["kind"])
        for what in fs.LIT:
            assert fs.strip(sc, what)[dict(textures="textures", lighting="light_rgb", sky="sky")[what]] is None
        assert (fs.strip(sc, "lighting")["table"][:, 6] == 0).all() and (sc["table"][:, 6] > 0).any()
    assert shins == set(fs.SHININESS) and sharps == set(fs.SHARPNESS) and kinds == set(fs.KINDS)
    assert min(above_one, black, no_tex, lamb0, overlap) >= 3, (above_one, black, no_tex, lamb0, overlap)
    for seed in (6, 14, 62):                                       # small scenes: the oracle's frame, and each feature live in it
        sc = fs.draw_lit(seed)
        lv = fs.live(oracle, sc)
        assert set(lv) == {"materials", "glass", "rough", "soft", "lens", "textures", "lighting", "sky"}
        assert min(lv[k] for k in fs.LIT) >= 5, (seed, lv)
        assert set(fs.live(oracle, fs.draw(seed))) == {"materials", "glass", "rough", "soft", "lens"}
