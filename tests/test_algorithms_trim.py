"""CPU replays of the restatements behind the instruction trims of the two-wave kernels (rt_device.h, Lds::trim), checked
against the straightforward forms.  No GPU needed; the GPU parity tests then confirm the device code."""
import os
import subprocess

from conftest import REPO

ALGO = os.path.join(REPO, "tests", "algo")


def _build(name, tmp_path):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ALGO, name + ".cpp")])
    return exe


def test_plane_tests_do_not_depend_on_the_joint_sign_of_den_and_num(tmp_path):
    """plane_den_num(no_negate) and any_hit_masks' sign-bit form of "the signs agree": the same decisions, and the same
    quotient bit for bit, as the straightforward forms — on every pair of a list of special values (zeros, denormals, the
    0.001 / 998 / 999 / 1000 boundaries and their neighbours, infinities, NaN) and on 5 million random pairs."""
    out = subprocess.check_output([_build("plane_sign_check", tmp_path), "5000000"], text=True)
    assert "mismatches=0" in out, out
    assert int(out.split("checked=")[1].split()[0]) > 5000000, out
