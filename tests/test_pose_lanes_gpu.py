"""The lane exchanges of the intra-camera pose solve's LM step, bit for bit against the forms they replaced (kept in the test program's
own source): the transposed butterfly cs_reduce_many<N> on lane swaps and DPP against the select-and-shuffle form, per owner lane, for
every N the library instantiates (9, 27, 28, 33, 42, 45) and the tree's small ends (1, 2, 3, 7); and the column-per-lane 6 x 6 solve against the entry-per-lane one on a few hundred systems
(J^T J + lambda I over lambda = 1e-3 ... 1e18, pivots off the diagonal at every step, ties, zero pivots, not-a-number entries).
tests/cxx/pose_lanes_dev_test.hip is one short program, compiled once per module."""
import os
import subprocess

import pytest

from coslam_amd import build as cbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lanes_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pose_lanes") / "pose_lanes_dev_test")
    subprocess.check_call([cbuild._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cxx", "pose_lanes_dev_test.hip"), "-o", exe])
    return exe


def _run(exe, what):
    got = subprocess.run([exe, what], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0 and "pose_lanes ok" in got.stdout, got.stdout + got.stderr
    return got.stdout


@pytest.mark.gpu
def test_reduce_many_equals_the_shuffle_butterfly_bit_for_bit(hip, lanes_exe):
    out = _run(lanes_exe, "reduce")
    # 42 cases of each N: N owner lanes each
    assert f"reduce {42 * (1 + 2 + 3 + 7 + 9 + 27 + 28 + 33 + 42 + 45)} " in out, out


@pytest.mark.gpu
def test_column_per_lane_solve_equals_the_entry_per_lane_solve_bit_for_bit(hip, lanes_exe):
    out = _run(lanes_exe, "solve")
    assert "solve: 474 systems" in out, out

