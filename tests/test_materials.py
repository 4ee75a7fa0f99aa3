"""Per-object materials without a GPU: the Material / Scene.generate_materials API, the C-ABI constants, and the
material fixtures (tests/golden/materials_*.npz, tools/gen_material_golden.py) pinned against the C oracle where the
table is uniform."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO, raygen_closed_form


def material_cases():
    return sorted(os.path.basename(p)[len("materials_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "materials_*.npz")))


def test_generate_materials_dedups_and_fills_the_default():
    from python_ray_tracer_amd.scene import Scene, Sphere, Plane, Light, Material
    mirror, matte = Material(0.0, 0.2, 0.9), Material(0.1, 0.7, 0.0)
    s = Scene([Light([1, 2, 3])],
              [Sphere([0, 0, 1], 1.0, [255, 0, 0], material=matte), Sphere([2, 0, 1], 0.5, [0, 255, 0]),
               Sphere([4, 0, 1], 0.5, [0, 0, 255], material=Material(0.1, 0.7, 0.0))],
              [Plane([0, 0, 0], [0, 0, 1], [125, 125, 125], material=mirror), Plane([9, 0, 0], [-1, 0, 0], [10, 20, 30])])
    table, sid, pid = s.generate_materials(Material(0.0, 0.6, 0.3))
    assert table.dtype == np.float64 and table.shape == (3, 3)
    assert sid.dtype == np.int32 and sid.shape == (3,) and pid.dtype == np.int32 and pid.shape == (2,)
    assert table.tolist() == [[0.1, 0.7, 0.0], [0.0, 0.6, 0.3], [0.0, 0.2, 0.9]]
    assert sid.tolist() == [0, 1, 0] and pid.tolist() == [2, 1]
    sp, li, pl = s.generate_scene()                           # the reference's layouts, untouched by materials
    assert sp.shape == (7, 3) and pl.shape == (9, 2) and li.shape == (3, 1)


def test_generate_materials_of_an_empty_scene():
    from python_ray_tracer_amd.scene import Scene, Material
    table, sid, pid = Scene([], [], []).generate_materials(Material(0.0, 0.6, 0.3))
    assert table.shape == (0, 3) and sid.shape == (0,) and pid.shape == (0,)


def test_abi_constants():
    from python_ray_tracer_amd import _lib
    src = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    assert int(re.search(r"#define\s+RT_MAX_MATERIALS\s+(\d+)", src).group(1)) == _lib.RT_MAX_MATERIALS == 256
    assert _lib.RT_ABI_VERSION == 7 and "rt_set_scene_materials" in _lib.PROTOTYPES


def test_material_fixtures_are_complete():
    cases = material_cases()
    assert {"default_64_d3", "uniform_48_d4", "aa_48_d2", "stoch_40x24_spp3_seed7", "c4_s64_d5_sub32", "c5_s256_d8_sub96"} <= set(cases)
    for c in cases:
        path = os.path.join(GOLDEN, f"materials_{c}.npz")
        assert os.path.getsize(path) < 1 << 20, c
        g = np.load(path)
        M = g["materials"].shape[0]
        assert g["materials"].shape == (M, 3) and g["materials"].dtype == np.float64 and np.isfinite(g["materials"]).all()
        assert g["sphere_material"].shape == (g["spheres"].shape[1],) and g["plane_material"].shape == (g["planes"].shape[1],)
        for ids in (g["sphere_material"], g["plane_material"]):
            assert ids.dtype == np.int32 and ((ids >= 0) & (ids < M)).all()
        assert g["rgb64"].shape == g["u8"].shape == (len(g["coords"]), 3)


def test_uniform_fixture_is_the_global_shading_bit_for_bit(oracle):
    """A uniform power-of-two table: the generator's restated sample() must be the C oracle's global-shading frame, every
    float64 bit — pins the generator's composition to the already pinned oracle."""
    g = np.load(os.path.join(GOLDEN, "materials_uniform_48_d4.npz"))
    table = g["materials"]
    assert table.shape == (1, 3) and tuple(table[0]) == (float(g["amb"]), float(g["lamb"]), float(g["refl"]))
    w, h = int(g["w"]), int(g["h"])
    ref = oracle.render(w, h, g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], float(g["amb"]),
                        float(g["lamb"]), float(g["refl"]), int(g["depth"]), False, raygen=raygen_closed_form(w, h, float(g["fov"])),
                        want=("u8", "f64"))
    co = g["coords"]
    assert np.array_equal(ref["f64"][:, co[:, 0], co[:, 1]].T.view(np.uint64), g["rgb64"].view(np.uint64))
    assert np.array_equal(ref["u8"][:, co[:, 0], co[:, 1]].T, g["u8"])


def test_per_object_fixture_differs_from_any_global_shading(oracle):
    """The per-object fixture is not the global path with its first material (the materials do something)."""
    g = np.load(os.path.join(GOLDEN, "materials_default_64_d3.npz"))
    w, h = int(g["w"]), int(g["h"])
    a, l, r = g["materials"][0]
    ref = oracle.render(w, h, g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], a, l, r, int(g["depth"]), False,
                        raygen=raygen_closed_form(w, h, float(g["fov"])), want=("u8",))
    co = g["coords"]
    assert (ref["u8"][:, co[:, 0], co[:, 1]].T != g["u8"]).any(axis=1).sum() > len(co) // 10
