"""CPU checks of the merge front: the C-ABI's symbols and struct sizes, the refusals that need no device, the loud failure
without one, the sample generator against hand-computed values, and the numpy restatement (tests/mergefront_ref.py) on the planted scenes
with their cover conditions (tests/mergefront_scenes.py asserts them while it builds a scene)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coslam_amd
from coslam_amd import merge as M
from tests import mergefront_ref as R
from tests import mergefront_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["create", "destroy", "run_dev", "match_dev", "from_matches_dev", "results", "buffers_get", "download"]


def test_symbols_and_constants_equal_the_header(tmp_path):
    lib = coslam_amd.lib()
    assert all(hasattr(lib, "cs_merge_front_" + n) for n in NAMES)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coslam_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bcs_merge_front_([a-z_]+)\s*\(", hdr))) == sorted(NAMES)
    src = tmp_path / "constants.c"   # (the mirrors' sizes and offsets: tests/test_abi.py's table)
    src.write_text('#include <stdio.h>\n#include "coslam_hip.h"\nint main(void) { printf("%d\\n", CS_MERGE_FRONT_MAX_JOBS); return 0; }\n')
    exe = tmp_path / "constants"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [M.MERGE_FRONT_MAX_JOBS]
    assert (M.MERGE_FRONT_TOO_FEW, M.MERGE_FRONT_NO_MODEL) == (R.TOO_FEW, R.NO_MODEL) == (1, 2)


def test_refusals_that_need_no_device():
    lib = coslam_amd.lib()
    for args in [(0, 0, 10, 64, 1, 10), (0, 17, 10, 64, 1, 10), (0, 2, 0, 64, 1, 10), (0, 2, 32769, 64, 1, 10), (0, 2, 10, 0, 1, 10),
                 (0, 2, 10, 129, 1, 10), (0, 2, 10, 64, 0, 10), (0, 2, 10, 64, 257, 10), (0, 2, 10, 64, 1, 0)]:
        assert not lib.cs_merge_front_create(*args)
        assert b"cs_merge_front_create: bad argument" in lib.cs_last_error()
    cam, job, res, buf = (M.MergeFrontCam * 2)(), (M.MergeFrontJob * 1)(), (M.MergeFrontResult * 1)(), M.MergeFrontBuffers()
    z = C.c_void_p(None)
    assert lib.cs_merge_front_run_dev(z, z, cam, 1, job, C.c_double(0.8), C.c_double(0.6), 200, C.c_double(2.0), 15, C.c_ulonglong(0)) != 0
    assert b"null handle" in lib.cs_last_error()
    assert lib.cs_merge_front_match_dev(z, z, cam, 1, job, C.c_double(0.8), C.c_double(0.6)) != 0
    assert lib.cs_merge_front_from_matches_dev(z, z, cam, 1, job, z, z, 200, C.c_double(2.0), 15, C.c_ulonglong(0)) != 0
    assert lib.cs_merge_front_results(z, z, 1, res) != 0
    assert lib.cs_merge_front_buffers_get(z, C.byref(buf)) != 0
    assert lib.cs_merge_front_download(z, z, z, z, C.c_size_t(0)) != 0
    lib.cs_merge_front_destroy(z)


def test_device_arena_and_range_test_on_the_host(tmp_path):
    """tests/cxx/dev_arena_test.cpp: the merge handles' layout arena (two passes, 256-byte alignment, declared order, empty arrays) and the
    range test behind every cs_merge_*_download (both ends, a pointer below the base, byte counts that would wrap) -- no HIP, no device"""
    exe = str(tmp_path / "dev_arena_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cxx", "dev_arena_test.cpp"), "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True)
    assert got.returncode == 0 and got.stdout.strip() == "dev_arena ok", got.stdout + got.stderr


def test_no_device_means_loud_failure():
    if coslam_amd.lib().cs_device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(coslam_amd.CoslamHipError):
        coslam_amd.MergeFront(2, 100, 64, 2, 200)
    assert hasattr(coslam_amd.MergeCamGroups, "run_from_descriptors")


def test_generator_against_hand_computed_values():
    """rand_hi by its definition written out once more, and three sample rows computed by hand from it"""
    m64 = (1 << 64) - 1

    def mix(seed, k, h, d):
        z = (seed + (((k << 40) | (h << 8) | d) + 1) * 0x9E3779B97F4A7C15) & m64
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & m64
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & m64
        return (z ^ (z >> 31)) >> 32

    for args, want in [((0, 0, 0, 0), 3793791033), ((77, 2, 5, 3), 3063993440), (((1 << 63) + 5, 255, 1999, 63), 4151429213)]:
        assert R.rand_hi(*args) == mix(*args) == want
    assert R.sample8(77, 0, 0, 25) == [9, 12, 13, 4, 19, 10, 22, 11]
    assert R.sample8(77, 2, 199, 127) == [52, 23, 49, 53, 104, 24, 99, 97]
    assert R.sample8(1, 0, 3, 8) == [6, 5, 2, 1, 3, 0, 7, 4]
    assert R.sample8(1, 0, 0, 7) is None
    for n in (8, 9, 127):
        for h in range(50):
            s = R.sample8(3, 1, h, n)
            assert s is None or (len(set(s)) == 8 and 0 <= min(s) and max(s) < n)


def test_restatement_meets_the_cover_conditions_of_every_scene():
    for dim in (64, 128):
        for n1, n2 in [(1, 1), (2, 1), (63, 65), (65, 63), (700, 650)]:
            S.descriptor_scene(n1, n2, dim)
    cases = [S.ransac_case(*c[:4], c[4], c[5]) for c in S.CLEAN + S.NOISY]
    frac, worst = S.gap_study(cases)
    assert frac >= 0.9 and 100.0 * worst <= S.E_TOL       # test 4's two numbers as the GPU test states them
    for sc, exp in cases:
        assert exp["emat_ok"] == int(exp["inlier_num"] >= 15) and exp["inlier_num"] == int(sc["truth"].sum()) and exp["flags"] == 0
        m = R.match_surf(sc["cam1"]["pts"], sc["cam1"]["desc"], sc["cam2"]["pts"], sc["cam2"]["desc"])
        assert np.array_equal(m["matches"], sc["matches"])      # the descriptor stage hands the RANSAC exactly the planted list
        S.assert_descriptor_cover(m, 0.8, 0.6, sc["cam1"]["desc"])


def test_restatement_solves_and_projects():
    """the Jacobi of the restatement against numpy on random symmetric matrices; the projection onto the essential manifold"""
    rng = np.random.default_rng(0)
    A = rng.normal(0, 1, (20, 9, 9))
    A = A + A.transpose(0, 2, 1)
    L, V = R.jacobi_eig(A)
    for h in range(20):
        lam = np.diagonal(L[h])
        assert np.abs(np.sort(lam) - np.linalg.eigvalsh(A[h])).max() < 1e-12
        assert np.abs(V[h] @ np.diag(lam) @ V[h].T - A[h]).max() < 1e-12
    E, ok = R.project_essential(rng.normal(0, 1, (20, 3, 3)))
    assert ok.all()
    for h in range(20):
        assert np.abs(np.linalg.svd(E[h], compute_uv=False) - np.array([1, 1, 0]) / np.sqrt(2)).max() < 1e-14
    few = R.estimate_emat(S.K, S.K, np.zeros((7, 2)), np.zeros((7, 2)), np.stack([np.arange(7)] * 2, axis=1))
    assert few["emat_ok"] == 0 and few["flags"] == R.TOO_FEW and few["surf_num"] == 7
