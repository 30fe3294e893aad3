"""The perturbed rotations R exp(eps e_k) of the intra-camera pose solve, built from the factor's structure (coslam_amd/csrc/pose_math.h),
against the full product they replace: tests/cxx/pose_math_test.cpp on the host, byte for byte, no HIP and no device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structured_perturbed_rotations_equal_the_full_product(tmp_path):
    exe = str(tmp_path / "pose_math_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cxx", "pose_math_test.cpp"),
                           "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0 and got.stdout.startswith("pose_math ok"), got.stdout + got.stderr
