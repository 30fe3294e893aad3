"""The line-cited restatement of MergeCameraGroup::checkPossibleMergable (tests/merge_ref.py; reference
src/app/SL_MergeCameraGroup.cpp:56-177) on its own, before any kernel is looked at: the hand-counted lattice scene, the planted scenes'
conditions and margins, the ctypes mirror's sizes and the C++ shim.

Why 1e-6 px is the margin asked of the planted scenes: two correct f64 evaluations of a projection through about 30 operations on pixel-size
numbers differ by less than 1e-11 px, and an orientation test over coordinates below 640 rounds below 1e-10 -- 1e-6 leaves four decades, so
no decision of the device's f64 path can differ from the restatement's exact one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import merge_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def planted():
    scenes = M.scene_set()
    return scenes, M.scene_results(scenes)


def test_the_restatement_reproduces_the_hand_counted_lattice_scene():
    s = M.lattice_scene()
    # every projection into camera 1 is the lattice point itself, exactly
    for (u, v), m in zip(M.LATTICE_HULL + M.LATTICE_INNER, range(0, 100, 2)):
        assert M.project(s["K"][1], s["R"][1], s["t"][1], s["mapPts"][m]) == (float(u), float(v))
    assert sum(inside for _, inside in M.LATTICE_PIXELS) == M.LATTICE_IN_NUM == 14
    hull = M.exact_hull([(float(u), float(v)) for u, v in M.LATTICE_HULL + M.LATTICE_INNER])
    assert sorted(hull) == sorted((u, v) for u, v in M.LATTICE_HULL)          # the inner points, those on edges included, are no vertices
    for (x, y), inside in M.LATTICE_PIXELS:
        assert M.pixel_in_hull(hull, int(x), int(y))[0] == bool(inside), (x, y)
    r = M.check_possible_mergable(s, *M.LATTICE_PARAMS)
    assert r["nInCam"][0, 1] == len(M.LATTICE_HULL) + len(M.LATTICE_INNER) and r["inNum"][0, 1] == M.LATTICE_IN_NUM
    assert r["nFeat"] == [13, len(M.LATTICE_PIXELS)] and r["fromTo"][0, 1] == 1    # 14 >= 0.5 * 21
    assert r["nInCam"][1, 0] == 0 and r["inNum"][1, 0] == -1 and r["fromTo"][1, 0] == 0 and r["info"] == []


def test_degenerate_hulls_set_no_pixel():
    assert M.exact_hull([(1.0, 1.0), (2.0, 2.0)]) == []
    assert M.exact_hull([(3.0, 1.0), (3.0, 2.0), (3.0, 7.5)]) == []            # all x equal
    assert M.exact_hull([(0.0, 0.0), (1.0, 0.5), (2.0, 1.0), (4.0, 2.0)]) == []   # collinear
    assert M.pixel_in_hull([], 1, 1) == (False, float("inf"))


def test_the_planted_scenes_hold_every_case_with_safe_margins(planted):
    scenes, res = planted
    assert [s["nCams"] for _, s, _ in scenes] == [2, 3, 5, 8, 16]
    for _, s, _ in scenes:
        assert (s["W"], s["H"]) == (640, 480) and 200 <= s["N"] <= 600 and 1000 <= s["nMap"] <= 2000
    seen = M.assert_scene_conditions(scenes, res)     # margins >= 1e-6 and every case of the list, on the restatement's own tables
    print(seen)
    r5 = res["edge5", False]
    assert [g for _, s, _ in scenes for g in s["groups"] if g == [0, 2, 1]]
    assert r5["beyond"] == [(1, 4)] and r5["fromTo"][0, 3] == 1 and r5["fromTo"][3, 0] == 0
    r16 = res["singletons16", False]
    assert len(r16["info"]) > 16 and [x[1:3] for x in r16["info"]] == sorted(x[1:3] for x in r16["info"])   # singletons: the loop order is ascending
    # same-group pairs are not evaluated without all_pairs
    assert r5["nInCam"][0, 2] == -1 and res["edge5", True]["nInCam"][0, 2] >= 0
    r8 = res["onegroup8", False]
    assert r8["info"] == [] and (r8["nInCam"] == -1).all() and not r8["fromTo"].any() and r8["nFeat"] == [-1] * 8


def test_the_info_list_follows_the_group_order_not_the_camera_order():
    s = M.lattice_scene()
    s["groups"] = [[1], [0]]
    r = M.check_possible_mergable(s, 0, 0.0, 6.0)  # minInNum 0, ratio 0: every evaluated direction holds
    assert r["info"] == [(3, 1, 0, 3, 0, 1)]


def test_ctypes_structs_have_the_headers_sizes():
    """(sizes and offsets against the compiler: tests/test_abi.py's table of mirrors)"""
    from coslam_amd.merge import MergeCandidates

    m = MergeCandidates.from_bytes(np.full(C.sizeof(MergeCandidates), 255, dtype=np.uint8).tobytes())
    assert m.nMergeInfo == -1 and m.inNum[15][15] == -1 and m.fromTo[3][4] == 255
    hdr = open(os.path.join(ROOT, "include", "coslam_hip.h")).read()
    for sym in ("cs_merge_check_dev", "cs_merge_check_scratch_bytes", "cs_merge_check", "cs_merge_cam", "cs_merge_info", "cs_merge_candidates"):
        assert sym in hdr


def test_merge_shim_compiles_and_links():
    """include/shim/app/CoSLAMMergeCheck.h: checkPossibleMergable's shape over the C-ABI; the driver also pins the record's size"""
    src = os.path.join(ROOT, "tests", "cxx", "merge_shim_link_test.cpp")
    exe = os.path.join(ROOT, "tests", "cxx", "merge_shim_link_test.bin")
    libdir = os.path.join(ROOT, "coslam_amd", "lib")
    cmd = ["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "shim"), src,
           "-L", libdir, "-lcoslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "merge shim ok" in out.stdout and "refused" in out.stdout
