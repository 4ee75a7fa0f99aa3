"""What the render kernels' once-per-tile path takes for granted (python-ray-tracer_amd/csrc/rt_device.h: render_kernel's prologue,
store_pixel), on the CPU: tests/algo/fixed_path_check.cpp compiles rt_math.h, rt_layout.h and rt_plan.h as the kernel does, under
AddressSanitizer and UndefinedBehaviorSanitizer, and checks
  * rt::clip_color, the straight-line clip, against the rule written out in the program (NaN -> 0, c <= -0.5 -> 0, c >= 255.5 -> 255,
    else rint(c) clamped to 0..255) on the special values, every tie k + 0.5 with both neighbours and 10^7 seeded bit patterns;
  * rt::flat_layout, the two fields of the table layout a two-wave kernel reads, against rt::table_layout for every scene the
    small-scene twins are sent (S = 1..8, L = 0..RT_MAX_LIGHTS) and every flat scene, and rt::lds_bytes against the image formed from it;
  * over the launch plan's case grid (tests/algo/launch_plan_check.cpp), that no clustered scene is planned a two-wave shape.
No GPU."""
import os
import subprocess

import pytest

from conftest import REPO

ALGO = os.path.join(REPO, "tests", "algo")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fixed_path") / "fixed_path_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(ALGO, "fixed_path_check.cpp")])
    return out


def _run(exe, what):
    res = subprocess.run([exe, what], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stdout + res.stderr
    return res.stdout.split()


def test_clip_color_is_the_rule(exe):
    out = _run(exe, "clip")
    assert out[0] == "clip" and out[-1] == "ok"
    assert int(out[1]) == 20 + 4 * 260 + 10_000_000


def test_flat_layout_is_table_layout(exe):
    out = _run(exe, "layout")
    assert out[0] == "layout" and out[-1] == "ok"
    assert int(out[1]) == 20 * 65          # S = 1..CLUSTER_MIN, L = 0..RT_MAX_LIGHTS


def test_no_clustered_scene_in_a_two_wave_shape(exe):
    out = _run(exe, "plan")
    assert out[0] == "plan" and out[-1] == "ok"
    assert int(out[1]) > 0 and 0 < int(out[2]) < int(out[1])
