"""rt::ground_plane (python-ray-tracer_amd/csrc/rt_plan.h): which launches run the ground-plane twins of the PLAIN render kernels
(rt_device.h: GROUND).  True exactly for a scene whose only plane has the stored normal (0, 0, 1), without a material table,
in a launch that does not count rays, with MI355RT_GROUND_PLANE not 0.  tests/algo/ground_plane_check.cpp asks it about scenes
packed by the library's own packer (so the axis codes are the ones rt_set_scene derives from the normals), under AddressSanitizer
and UndefinedBehaviorSanitizer, and checks that the choice is a dimension of its own: the plan of a launch (family, shape, index,
LDS bytes: what tests/golden/launch_plan.npz pins) is the same whatever the knob says.  No GPU."""
import os
import subprocess

from conftest import REPO

ALGO = os.path.join(REPO, "tests", "algo")

EXPECTED = {
    "one_z_up": 1, "one_z_up_s64": 1, "one_z_up_s256": 1, "one_z_up_no_bundles": 1,
    "no_plane": 0,                      # P == 0
    "two_planes": 0, "two_z_up": 0,     # P == 2, whatever their normals
    "tilted": 0,                        # code 0
    "z_down": 0,                        # code -3
    "x_up": 0, "x_down": 0,             # codes +1, -1
    "y_up": 0, "y_down": 0,             # codes +2, -2
    "z_up_length_2": 0,                 # (0, 0, 2) is not e_z as stored: code 0
    "materials": 0,                     # a material table: family MAT
    "count_rays": 0,                    # RT_FLAG_COUNT_RAYS
    "knob_off": 0,                      # MI355RT_GROUND_PLANE=0
}


def test_ground_plane_predicate(tmp_path):
    exe = str(tmp_path / "ground_plane_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ALGO, "ground_plane_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stdout + res.stderr
    lines = [ln.split() for ln in res.stdout.strip().splitlines()]
    assert {ln[0]: int(ln[1]) for ln in lines if ln[0] != "twin"} == EXPECTED
    # PLAIN's 25 shapes less the three that count rays, less the six register variants whose twins showed no gain (rt_plan.h:
    # NO_GROUND_TWIN): digits aa, park, wpw, lat, mode
    twins = {ln[1] for ln in lines if ln[0] == "twin"}
    every = {"01200", "11200", "00400", "01400", "10400", "11400", "01401", "01210", "00210", "00410", "01410", "01411",
             "01402", "10402", "11403", "01412", "00200", "10200", "00401", "00411", "00402", "00412"}
    assert len(every) == 22 and twins == every - {"00200", "10200", "00401", "00411", "00402", "00412"}, sorted(twins)


def test_gpu_settings_plan_the_shapes_they_are_there_for(tmp_path):
    """tests/ground_plane_scenes.py: SHAPES names, per setting of tests/test_gpu_ground_plane.py, the kernel the library must log.
    rt_plan.h (through tests/algo/guides_plan_check.cpp, under AddressSanitizer and UBSan) says here, without a GPU, that the
    settings reach those shapes: two-wave and four-wave workgroups, MODE 0, 1, 2 and 3, with an AA mode of their own and without.
    (MI355RT_WPW2_MAX_IMAGE is not an argument of that program: its row is left to the GPU test.)"""
    import ground_plane_scenes as gps
    exe = str(tmp_path / "guides_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ALGO, "guides_plan_check.cpp")])
    names = [n for n, s in gps.SHAPES.items() if "MI355RT_WPW2_MAX_IMAGE" not in s[1] and not (s[2] and not s[3])]   # (no lattice rows either)
    args = []
    for n in names:
        which, knobs = gps.SHAPES[n][:2]
        S = gps.crowd_scene()["spheres"].shape[1] if which == "crowd" else gps.fixture_scene("default_128_d3")["spheres"].shape[1]
        args += [S, 1, 3, 0, 0, max(8, int(knobs.get("MI355RT_CLUSTER_MINS", 20))), int(knobs.get("MI355RT_LANES_MINS", 161)), 1,
                 int(knobs.get("MI355RT_LANES_PARK", 1))]
    res = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stdout + res.stderr
    seen = set()
    for n, line in zip(names, res.stdout.splitlines()):
        v = [int(x) for x in line.split()]
        aa, expect = gps.SHAPES[n][2], gps.SHAPES[n][4]
        mode, park, wpw = v[8:11] if aa else v[5:8]
        got = dict(mode=mode, park=park, wpw=wpw)
        assert all(got[k] == expect[k] for k in got if k in expect), (n, got, expect)
        seen.add((wpw, mode, aa))
    assert seen == {(2, 0, 0), (2, 0, 1), (4, 0, 0), (4, 1, 0), (4, 2, 0), (4, 3, 1), (4, 0, 1)}, seen
    assert not gps.SHAPES["mode2_register_no_twin"][5] and all(s[5] for n, s in gps.SHAPES.items() if n != "mode2_register_no_twin")
