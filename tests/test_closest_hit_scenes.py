"""The conditions of tests/closest_hit_scenes.py, on the CPU: a scene or a filter input that does not discriminate would let the GPU
tests that use it pass whatever the kernels do.  The CPU oracle and the numpy restatements say what each construction shows: the
tie scenes' frames depend on the caller's order of the spheres in (nearly) every pixel and never show a filler; the coincident
planes' frame depends on which of the two wins; the limit scene shows textured spheres, planes and sky; the synthetic filter inputs
give finite results that are not the plain mean, and a sixth level changes them.  rt_plan.h, run by tests/algo/guides_plan_check.cpp
under AddressSanitizer and UBSan, says which table mode every setting of the GPU tests reaches."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, raygen_closed_form
import closest_hit_scenes as chs
from test_denoise import guide_scene

from python_ray_tracer_amd import denoise as D

ALGO = os.path.join(REPO, "tests", "algo")
NO_LIGHTS = np.zeros((3, 0), np.float32)
SIZES = sorted({v[0] for v in chs.SETTINGS.values()})


# ---------------------------------------------------------------------------------------------------------------------
# The plan of every setting

def _plan_rows(tmp_path, rows):
    """rt_plan.h on rows of (S, P, L, M, T, cluster_min, lanes_min_spheres, f32_records, lanes_park): per row a dict of what
    tests/algo/guides_plan_check.cpp prints."""
    exe = str(tmp_path / "guides_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ALGO, "guides_plan_check.cpp")])
    res = subprocess.run([exe] + [str(v) for r in rows for v in r], capture_output=True, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stdout + res.stderr
    names = ("S", "NC", "anchors", "guides_mode", "guides_lds", "m0", "park0", "wpw0", "m1", "park1", "wpw1")
    out = [dict(zip(names, (int(v) for v in line.split()))) for line in res.stdout.splitlines()]
    assert len(out) == len(rows)
    return out


def _knob_row(S, P, L, M, T, knobs):
    return (S, P, L, M, T, max(8, int(knobs.get("MI355RT_CLUSTER_MINS", 20))), int(knobs.get("MI355RT_LANES_MINS", 161)),
            int(knobs.get("MI355RT_F32_RECORDS", 1)), int(knobs.get("MI355RT_LANES_PARK", 1)))


def test_every_setting_plans_the_mode_it_is_there_for(tmp_path):
    names = list(chs.SETTINGS)
    # after the settings, the guides tests' other scenes: the limit scenes (1024 spheres, 64 planes, textured), the textured clustered
    # ones, the empty one
    others = [_knob_row(1024, 64, 3, 256, 3, {}), _knob_row(1024, 64, 1, 256, 3, {}), _knob_row(64, 1, 3, 4, 3, {}), _knob_row(256, 1, 3, 4, 3, {}),
              _knob_row(64, 1, 3, 4, 3, {"MI355RT_F32_RECORDS": "0"}), _knob_row(0, 0, 1, 0, 0, {})]
    rows = _plan_rows(tmp_path, [_knob_row(chs.SETTINGS[n][0], 0, chs.SETTINGS[n][1], 0, 0, chs.SETTINGS[n][2]) for n in names] + others)
    plans, (lim3, lim1, c4, c5, c4_rec, empty) = rows[:len(names)], rows[len(names):]
    for n, p in zip(names, plans):
        S, lights, knobs, clustered, gmode, plain, aa = chs.SETTINGS[n]
        assert (p["NC"] > 0) == clustered and p["guides_mode"] == gmode, (n, p)
        assert (p["m0"], p["park0"], p["wpw0"]) == plain and (p["m1"], p["park1"], p["wpw1"]) == aa, (n, p)
    by = dict(zip(names, plans))
    assert by["s1024_no_anchors"]["anchors"] == 0 and by["s1024_anchored"]["anchors"] == 1
    seen = {chs.SETTINGS[n][5] for n in names} | {chs.SETTINGS[n][6] for n in names}
    assert {(0, 1, 4), (1, 1, 4), (1, 0, 4), (2, 1, 4), (2, 0, 4), (3, 1, 4)} <= seen
    guides = {(chs.SETTINGS[n][4], chs.SETTINGS[n][3]) for n in names}             # (mode, clustered)
    assert {(0, True), (0, False), (1, True), (1, False), (2, True)} <= guides
    assert lim3["guides_mode"] == 2 and lim3["anchors"] == 0 and lim3["guides_lds"] <= 65536
    assert lim1["guides_mode"] == 2 and lim1["anchors"] == 2 and lim1["guides_lds"] == 66608 > 65536     # raise_lds has to act
    assert (c4["guides_mode"], c5["guides_mode"], c4_rec["guides_mode"], empty["guides_mode"]) == (1, 2, 0, 0)
    for name, S in (("c4_s64_d5_sub32", 64), ("c5_s256_d8_sub96", 256)):                # (the rows above are those scenes' sizes)
        g = guide_scene(name)[0]
        assert (g["spheres"].shape[1], g["planes"].shape[1], g["lights"].shape[1]) == (S, 1, 3)


# ---------------------------------------------------------------------------------------------------------------------
# The tie scenes

def _tie_frames(oracle, sc, aa):
    return oracle.render(8, 8, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], 1.0, 0.0, 0.0, 0, aa,
                         pixel_loc=sc["pixel_loc"], want=("u8", "f32"))


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("case", range(chs.TIE_CASES))
def test_tie_scene_frames_depend_on_the_callers_order(oracle, case, S):
    fx = chs.tie_fixture()
    pair = [chs.tie_scene(case, S, 7, rev, 3) for rev in (False, True)]
    ids = []
    for sc in pair:
        g = D.guides_reference(sc["spheres"], sc["planes"], sc["cam_origin"], sc["cam_rot"], 8, 8, pixel_loc=sc["pixel_loc"])
        assert np.isin(g[7], sc["tie_at"].astype(np.float32)).all(), "a filler or a miss wins a pixel"
        assert (g[3] == np.float32(4.0)).all()                   # every tie is at distance 4.0, as the fixture has it
        ids.append(np.argsort(sc["tie_at"])[np.searchsorted(np.sort(sc["tie_at"]), g[7].astype(np.int64))])   # tie sphere per pixel
    n_ids = int((ids[0] != ids[1]).sum())
    assert n_ids >= 60, n_ids
    counts = []
    for aa in (0, 1):
        a, b = (_tie_frames(oracle, sc, aa) for sc in pair)
        counts.append(int((a["u8"] != b["u8"]).any(axis=0).sum()))
        # the oracle's frame shows the winner's colour: amb 1 (aa 0; aa 1 averages nine winners)
        if aa == 0:
            assert np.array_equal(a["f32"], fx[f"spheres_{case}"][4:7][:, ids[0]].astype(np.float32))
    # RT_AA_STOCHASTIC needs the closed-form grid: the 8 x 8 one over the field the fixture's targets were picked from, jittered.
    # Those rays were not chosen for their ties, so the condition is half the frame (57 to 63 of 64 as measured)
    st = [oracle.render(8, 8, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], 1.0, 0.0, 0.0, 0, 2, spp=2, seed=7,
                        raygen=raygen_closed_form(8, 8, 45.0), want=("u8",))["u8"] for sc in pair]
    n_stoch = int((st[0] != st[1]).any(axis=0).sum())
    print(f"tie case {case} S={S}: caller order changes {counts[0]} (aa 0), {counts[1]} (aa 1) and {n_stoch} (aa 2 spp 2) of 64 pixels, "
          f"the id of {n_ids}")
    assert min(counts) >= 60 and n_stoch >= 32, (counts, n_stoch)
    if S == 16 + 20:                                              # lights change no byte, and neither does the uniform table
        sc = pair[0]
        dark = oracle.render(8, 8, sc["cam_origin"], sc["cam_rot"], sc["spheres"], NO_LIGHTS, sc["planes"], 1.0, 0.0, 0.0, 0, 0,
                             pixel_loc=sc["pixel_loc"], want=("u8", "f32"))
        mat = oracle.render(8, 8, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], 7.0, -3.0, 2.0, 0, 0,
                            pixel_loc=sc["pixel_loc"], want=("u8", "f32"), materials=chs.uniform_materials(sc))
        lit = _tie_frames(oracle, sc, 0)
        assert np.array_equal(dark["f32"], lit["f32"]) and np.array_equal(mat["f32"], lit["f32"]) and np.array_equal(mat["u8"], lit["u8"])


def test_tie_scene_puts_the_sixteen_where_the_seed_says():
    a, b = chs.tie_scene(2, 256, 7, False, 3), chs.tie_scene(2, 256, 7, True, 0)
    tie = chs.tie_fixture()["spheres_2"]
    assert np.array_equal(a["spheres"][:, a["tie_at"]], tie) and np.array_equal(b["spheres"][:, b["tie_at"]], tie)
    assert np.array_equal(np.sort(a["tie_at"]), np.sort(b["tie_at"])) and np.array_equal(a["tie_at"], np.sort(a["tie_at"])[::-1][np.argsort(np.argsort(b["tie_at"]))])
    fill = np.setdiff1d(np.arange(256), a["tie_at"])
    assert np.array_equal(a["spheres"][:, fill], b["spheres"][:, fill])
    d = np.linalg.norm(a["spheres"][0:3, fill].astype(np.float64), axis=0)
    assert (d - a["spheres"][3, fill] > 5.5).all() and d.max() <= 12.001 and a["lights"].shape == (3, 3) and b["lights"].shape == (3, 0)
    assert not np.array_equal(chs.tie_scene(2, 256, 8, False, 3)["tie_at"], a["tie_at"])


# ---------------------------------------------------------------------------------------------------------------------
# Coincident planes

def coincident_frame(oracle, sc, aa):
    w, h = sc["w"], sc["h"]
    return oracle.render(w, h, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], *sc["shade"], sc["depth"], aa,
                         raygen=raygen_closed_form(w, h, sc["fov"]), want=("u8", "f32"))


def test_coincident_planes_the_first_wins(oracle):
    sc, swapped = chs.coincident_planes_scene(), chs.coincident_planes_scene(swap=True)
    w, h, S = sc["w"], sc["h"], sc["spheres"].shape[1]
    assert S > 20 and np.array_equal(sc["planes"][0:6, 0], sc["planes"][0:6, 1]) and not np.array_equal(sc["planes"][6:9, 0], sc["planes"][6:9, 1])
    g = D.guides_reference(sc["spheres"], sc["planes"], sc["cam_origin"], sc["cam_rot"], w, h, raygen=raygen_closed_form(w, h, sc["fov"]))
    assert (g[7] != S + 1).all() and (g[7] == S).sum() >= 100 and (g[7] < S).sum() >= 50
    for aa in (0, 1):
        n = int((coincident_frame(oracle, sc, aa)["u8"] != coincident_frame(oracle, swapped, aa)["u8"]).any(axis=0).sum())
        print(f"coincident planes aa={aa}: swapping the two colours changes {n} of {w * h} pixels")
        assert n >= 100, n
    # the mirror bounces see the planes again: pixels of spheres change with the swap too
    on_sphere = (g[7] >= 0) & (g[7] < S)
    assert ((coincident_frame(oracle, sc, 0)["u8"] != coincident_frame(oracle, swapped, 0)["u8"]).any(axis=0) & on_sphere).sum() >= 10


# ---------------------------------------------------------------------------------------------------------------------
# The limit scene

_LIMIT_GUIDES = {}


def limit_guides(L, textured=True):
    """guides_reference of limit_scene(L) on its 64 x 40 grid: once, read-only."""
    key = (L, textured)
    if key not in _LIMIT_GUIDES:
        sc = chs.limit_scene(L)
        a = D.guides_reference(sc["spheres"], sc["planes"], sc["cam_origin"], sc["cam_rot"], sc["w"], sc["h"], raygen=sc["raygen"],
                               textures=sc["textures"] if textured else None)
        a.setflags(write=False)
        _LIMIT_GUIDES[key] = a
    return _LIMIT_GUIDES[key]


def test_limit_scene_shows_textured_spheres_planes_and_sky():
    sc1, sc3 = chs.limit_scene(1), chs.limit_scene(3)
    sp, pl, li, table, sid, pid = chs.size_limit_arrays(np.random.default_rng(1024))
    assert np.array_equal(sc3["spheres"], sp) and np.array_equal(sc3["planes"], pl) and np.array_equal(sc3["lights"], li[:, :3])
    assert np.array_equal(sc1["lights"], li[:, :1]) and sp.shape == (7, 1024) and pl.shape == (9, 64)
    recs, st, pt, texels = sc3["textures"]
    assert len(recs) == 3 and (st[0::3] >= 1).all() and (st[1::3] == -1).all() and (st[2::3] == -1).all() and {1, 2} == set(st[0::3].tolist())
    assert (pt == 0).all()
    g, plain = limit_guides(3), limit_guides(3, textured=False)
    ids = g[7].astype(np.int64)
    on_sphere = (ids >= 0) & (ids < 1024)
    textured = on_sphere & (st[np.clip(ids, 0, 1023)] >= 0)
    n_tex, n_plane, n_miss = int(textured.sum()), int((ids >= 1024).sum()), int((ids < 0).sum())
    n_albedo = int(((g[4:7] != plain[4:7]).any(axis=0)).sum())
    print(f"limit scene 64x40: {n_tex} pixels of textured spheres, {n_plane} of planes, {n_miss} misses; textures change {n_albedo} albedos")
    assert n_tex >= 200 and n_plane >= 200 and n_miss >= 50 and n_albedo >= 300
    assert len(np.unique(ids[ids >= 1024])) >= 5 and len(np.unique(ids[textured])) >= 5 and len(np.unique(ids[on_sphere])) >= 12
    slab = ids[19:45]                                            # the column slab of the in-place test shows all three too
    assert (slab < 0).sum() >= 20 and (slab >= 1024).sum() >= 100 and ((slab >= 0) & (slab < 1024)).sum() >= 100


# ---------------------------------------------------------------------------------------------------------------------
# The filter's synthetic inputs

def test_synthetic_guides_are_what_they_say():
    g = chs.synthetic_guides(97, 71, 0)
    assert g.dtype == np.float32 and g.shape == (8, 97, 71)
    ids = g[7]
    assert set(np.unique(ids[:24]).tolist()) == {3.0, 7.0} and (ids[:24][1:, :] != ids[:24][:-1, :]).all()
    assert set(np.unique(ids[24:48]).tolist()) == set(float(i) for i in range(10))
    miss = ids < 0
    assert miss[48:72].all() and not miss[:48].any() and not miss[72:].any() and (g[0:7][:, miss].view(np.uint32) == 0).all()
    assert (ids[72:] == chs.BIG_ID).all() and chs.BIG_ID >= 1024
    n2 = (g[0:3].astype(np.float64) ** 2).sum(axis=0)
    assert np.allclose(n2[~miss], 1.0, atol=1e-6)
    low = g[0:3, :24, 36:]
    assert (low == low[:, :1, :1]).all() and len(np.unique(g[0, :24, :36])) > 800
    assert set(np.unique(g[4:7][:, ~miss]).tolist()) == set(chs.ALBEDOS.tolist())
    s = chs.synthetic_sums(97, 71, 3, 1)
    assert 0.07 < (s == 0.0).mean() < 0.13 and (s < 0).sum() >= 100 and s.min() >= -4.0 and ((s == 1e200).all(axis=0)).sum() == 8
    assert ((chs.synthetic_sums(2, 2, 1, 0) == 1e200).all(axis=0)).sum() == 4


def _filter_launches():
    out = [(ws, h, st) for ws, h in chs.SIX_FRAMES for st in chs.SIX_LEVELS]
    out += [(ws, h, st) for ws, h in chs.SYNTHETIC_FRAMES for st in chs.DENOISE_SETTINGS]
    return out + [chs.grid_cap_frame(256) + (chs.GRID_CAP_SETTING,)]


def _certain_to_mix(ws, h, guides, sums):
    """Pixels of a one-row frame that some tap reaches with a weight that cannot vanish, at any normal shininess: the pixel and the
    tap show the same id, both have the constant normal or are misses (cn = 1), and neither holds 1e200 (a finite colour weight)."""
    assert h == 1
    ids, steady = guides[7, :, 0], (guides[0:3, :, 0] == guides[0:3, 4:5, 0]).all(axis=0) | (guides[7, :, 0] < 0)
    ok = steady & ~(sums[:, :, 0] == 1e200).any(axis=0)
    out = np.zeros(ws, bool)
    for step in (1, 2, 4, 8, 16, 32):
        for d in (-2, -1, 1, 2):
            q = np.arange(ws) + step * d
            inside = (q >= 0) & (q < ws)
            qc = np.clip(q, 0, ws - 1)
            out |= inside & ok & ok[qc] & (ids[qc] == ids)
    return out


@pytest.mark.parametrize("ws, h, setting", _filter_launches(), ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_filter_of_the_synthetic_inputs_is_finite_and_not_the_mean(ws, h, setting):
    """Every filter launch the GPU tests make on the synthetic inputs: finite everywhere (so a comparison of bits is one of
    values), and unlike the plain mean in at least half the pixels (levels 0 is the mean itself).  One launch cannot reach half:
    33 x 1 at normal shininess 1024.  Half of its 33 pixels have random normals, whose cosine to the 1024th power leaves the centre
    tap alone, and eight hold 1e200, which no colour weight lets mix: about twelve pixels remain.  Its condition is the one that
    reasoning gives: every pixel that a tap reaches with a weight that cannot vanish (_certain_to_mix) differs from the mean, and
    there are at least eight of them (20 pixels have cn = 1: four in each band of ids and the eight misses; at most eight of those
    hold 1e200, and a few of the other twelve have no partner of their id)."""
    levels, shin, sigma, dem, n = setting
    s, out = chs.filtered_truth(ws, h, setting)
    assert np.isfinite(out).all() and out.shape == (3, ws, h)
    differs = (out != s / np.float64(n)).any(axis=0)
    changed = int(differs.sum())
    if levels == 0:
        assert changed == 0
        return
    print(f"{ws} x {h} {setting}: the filter changes {changed} of {ws * h} pixels")
    if h == 1:
        must = _certain_to_mix(ws, h, chs.synthetic_guides(ws, h, 0), s)
        print(f"{ws} x {h} {setting}: {int(must.sum())} pixels are certain to mix")
        assert must.sum() >= 8 and differs[:, 0][must].all(), (int(must.sum()), np.flatnonzero(must & ~differs[:, 0]).tolist())
    if (ws, h, shin) != (33, 1, 1024):
        assert 2 * changed >= ws * h, (changed, ws * h)


def test_a_sixth_level_changes_the_result():
    for st in chs.SIX_LEVELS:
        s, six = chs.filtered_truth(97, 71, st)
        five = D.denoise_reference(s, st[4], chs.synthetic_guides(97, 71, 0), 5, *st[1:4])
        n = int((six != five).any(axis=0).sum())
        print(f"levels 6 against 5 on 97 x 71, shin {st[1]} sigma {st[2]} demodulate {st[3]}: {n} of {97 * 71} pixels differ")
        assert n >= 1000, n
