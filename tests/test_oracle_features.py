"""The CPU oracle's feature path (oracle/rt_oracle.c orc_render_ex: per-object materials, refraction, scatter, area lights and
the thin lens, restated from include/mi355rt.h) pinned to EVERY pixel of every feature fixture (tests/golden/{materials,
refraction,scatter,soft,lens}_*.npz, made around the reference's own trace() by tools/gen_*_golden.py): uint8 and float64,
bit for bit.  Each deliberately wrong restatement (oracle.WRONG) fails at least one fixture, and the oracle refuses what the
header refuses."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_frame, raygen_closed_form

FAMILIES = ("materials", "refraction", "scatter", "soft", "lens")


def feature_cases():
    return sorted(os.path.basename(p)[:-len(".npz")] for f in FAMILIES for p in glob.glob(os.path.join(GOLDEN, f"{f}_*.npz")))


def _render(oracle, g, wrong=0, **over):
    w, h = int(g["w"]), int(g["h"])
    kw = dict(materials=(g["materials"], g["sphere_material"], g["plane_material"]), spp=int(g["spp"]) if "spp" in g else 0,
              seed=int(g["seed"]) if "seed" in g else 1)
    if "light_radius" in g:
        kw.update(light_radius=g["light_radius"], shadow_samples=int(g["shadow_samples"]))
    if "aperture" in g:
        kw.update(lens=(float(g["aperture"]), float(g["focus_distance"])))
    kw.update(over)
    # amb, lamb and refl of the call are not read for a scene with a table
    return oracle.render_pixels(w, h, g["coords"], g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"],
                                7.0, -3.0, 2.0, int(g["depth"]), int(g["aa"]), raygen=raygen_closed_form(w, h, float(g["fov"])),
                                wrong=wrong, **kw)


def test_every_family_has_fixtures():
    cases = feature_cases()
    assert len(cases) >= 42
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
    scalars' frame (mi355rt.h rt_set_scene_materials)."""
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
