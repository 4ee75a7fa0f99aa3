"""Scenes and settings of the ground-plane twins' tests (no tests here: tests/test_ground_plane.py holds the settings to the shapes
they are there for on the CPU, tests/test_gpu_ground_plane.py renders them with MI355RT_GROUND_PLANE on and off).

GROUND, the reference's ground: the plane through (5, 0, 0) with normal (0, 0, 1) that every golden scene has.
fixture_scene   the scene and camera of a golden frame (its plane is GROUND)
crowd_scene     64 spheres over GROUND: the scene the four-wave, MODE 1 and MODE 2 twins are reached with
SHAPES          name: (scene, MI355RT_* knobs, AA mode, launch flags by name, what the logged kernel must show, whether it is a twin)"""
import numpy as np

from conftest import load_frame

BIG = "100000"
GROUND = (5.0, 0.0, 0.0, 0.0, 0.0, 1.0, 125.0, 125.0, 125.0)


def planes_of(*rows):
    return np.ascontiguousarray(np.array(rows, np.float32).reshape(len(rows), 9).T)


def fixture_scene(name):
    g = load_frame(name)
    assert g["planes"].shape == (9, 1) and tuple(g["planes"][:, 0].tolist()) == GROUND
    return dict(spheres=g["spheres"], lights=g["lights"], planes=g["planes"], cam_origin=g["cam_origin"], cam_rot=g["cam_rot"],
                fov=float(g["fov"]), shade=(float(g["amb"]), float(g["lamb"]), float(g["refl"])))


def crowd_scene(S=64):
    """S spheres resting on or hovering over GROUND in front of the default camera (so that they are clustered by the packer's
    default rule and shadow one another and the ground), the default scene's lights."""
    g = load_frame("default_128_d3")
    rng = np.random.default_rng(64)
    sp = np.zeros((7, S), np.float32)
    sp[0] = rng.uniform(0.0, 9.0, S)
    sp[1] = rng.uniform(-3.5, 3.5, S)
    sp[3] = rng.uniform(0.15, 0.45, S)
    sp[2] = sp[3] + rng.uniform(0.0, 1.5, S)
    sp[4:7] = rng.integers(40, 256, (3, S))
    return dict(spheres=sp, lights=g["lights"], planes=planes_of(GROUND), cam_origin=g["cam_origin"], cam_rot=g["cam_rot"],
                fov=float(g["fov"]), shade=(0.05, 0.6, 0.3))


# name: (scene: "default" (the six spheres of the golden default scene) or "crowd", knobs, aa, flags, the logged kernel's fields,
# the knob-unset run logs a twin)
# The crowd rows are tests/closest_hit_scenes.py's s64 settings with one plane; tests/test_ground_plane.py evaluates rt_plan.h for them.
SHAPES = {
    "two_waves":        ("default", {}, 0, (), dict(aa=0, park=1, wpw=2, lat=0, mode=0), True),
    "two_waves_aa":     ("default", {}, 1, ("RT_FLAG_AA_PER_PIXEL",), dict(aa=1, wpw=2, lat=0, mode=0), True),
    "two_waves_lattice": ("default", {}, 1, (), dict(aa=0, wpw=2, lat=1, mode=0), True),
    "four_waves":       ("crowd", {"MI355RT_CLUSTER_MINS": BIG}, 0, (), dict(aa=0, park=1, wpw=4, lat=0, mode=0), True),
    "four_waves_small": ("default", {"MI355RT_WPW2_MAX_IMAGE": "0"}, 0, (), dict(aa=0, wpw=4, lat=0, mode=0), True),
    "mode1":            ("crowd", {}, 0, (), dict(aa=0, park=1, wpw=4, lat=0, mode=1), True),
    "mode2":            ("crowd", {"MI355RT_LANES_MINS": "30"}, 0, (), dict(aa=0, park=1, wpw=4, lat=0, mode=2), True),
    "mode3_aa":         ("crowd", {"MI355RT_LANES_MINS": "30"}, 1, ("RT_FLAG_AA_PER_PIXEL",), dict(aa=1, park=1, wpw=4, lat=0, mode=3), True),
    # a shape without a twin (rt_plan.h: NO_GROUND_TWIN): the generic kernel, knob or not
    "mode2_register_no_twin": ("crowd", {"MI355RT_LANES_MINS": "30", "MI355RT_LANES_PARK": "0"}, 0, (), dict(aa=0, park=0, wpw=4, lat=0, mode=2), False),
    "four_waves_aa":    ("crowd", {}, 1, ("RT_FLAG_AA_PER_PIXEL",), dict(aa=1, park=0, wpw=4, lat=0, mode=0), True),
}
