"""Camera grouping without a GPU: known answers of the restatement of CoSLAM::getViewOverlapCosts / cameraGrouping (tests/grouping_ref.py,
reference src/app/SL_CoSLAM.cpp:1543-1697), the conditions the GPU tests' scene set must meet, the C-ABI's new symbols and the loud failure
of the wrappers where there is no device."""
import numpy as np
import pytest

from tests import grouping_ref as G

W, H = 640, 480


def tables(nCams, points, false=(), N=64):
    """points: one tuple of cameras per map point; pixels spread over the image"""
    rng = np.random.RandomState(7)
    pf = np.full((len(points), nCams), -1, dtype=np.int32)
    nxt = [0] * nCams
    for p, cams in enumerate(points):
        for c in cams:
            pf[p, c] = nxt[c]
            nxt[c] += 1
    flags = np.zeros(len(points), dtype=np.uint8)
    for p in false:
        flags[p] = G.MAP_FALSE
    xy = np.stack([np.stack([rng.uniform(0, W, N), rng.uniform(0, H, N)], axis=1) for _ in range(nCams)])
    return pf, flags, xy


def circle(nCams, far=()):
    Rs = [np.eye(3) for _ in range(nCams)]
    Cs = [np.array([np.cos(2 * np.pi * c / nCams), 0.0, np.sin(2 * np.pi * c / nCams)]) for c in range(nCams)]
    ts = [-C for C in Cs]
    init = G.init_cam_translation(Rs, ts)
    for c in far:
        ts[c] = -40.0 * Cs[c]
    return Rs, ts, init


def group(nCams, points, false=(), far=(), num=0, ratio=0.0):
    pf, flags, xy = tables(nCams, points, false)
    Rs, ts, init = circle(nCams, far)
    return G.camera_grouping(pf, flags, xy, W, H, Rs, ts, init, 6.0, num, ratio)


def test_the_order_inside_a_group_is_the_order_of_discovery():
    r = group(3, [(0, 2)] * 5 + [(2, 1)] * 5)
    assert r["groups"] == [[0, 2, 1]] and r["groupId"] == [0, 0, 0]


def test_an_isolated_camera_is_its_own_group_and_groups_are_numbered_by_their_lowest_camera():
    r = group(5, [(1, 3)] * 4 + [(0, 4)] * 4)
    assert r["groups"] == [[0, 4], [1, 3], [2]] and r["groupId"] == [0, 1, 2, 1, 0]


def test_one_camera_is_one_group():
    r = group(1, [(0,)] * 3)
    assert r["groups"] == [[0]] and r["groupId"] == [0]


def test_a_pair_that_shares_only_false_points_is_not_connected():
    r = group(2, [(0, 1)] * 6, false=range(6))
    assert r["groups"] == [[0], [1]] and int(r["nShare"][0, 1]) == 0 and r["vcosts"][0, 1] == 0   # (a cost of 0 is no edge: `> 0`, :1680)


def test_a_point_held_by_exactly_one_camera_adds_nothing():
    r = group(3, [(0,), (1,), (2,), (0,)])
    assert not r["nShare"].any() and r["groups"] == [[0], [1], [2]]


def test_exactly_min_overlap_num_passes_and_one_fewer_fails():
    assert group(2, [(0, 1)] * 10, num=10)["groups"] == [[0, 1]]
    r = group(2, [(0, 1)] * 9, num=10)
    assert r["groups"] == [[0], [1]] and r["vcosts"][0, 1] == -1 and int(r["nShare"][0, 1]) == 9


@pytest.mark.parametrize("pts", [[], [(3.0, 4.0)], [(3.0, 4.0), (100.0, 50.0)], [(0.0, 0.0), (10.0, 10.0), (20.0, 20.0), (5.0, 5.0)]])
def test_fewer_than_three_or_collinear_shared_points_have_area_zero_and_fail_any_positive_ratio(pts):
    assert G.exact_hull_area(pts) == 0.0
    pf = np.array([[k, k] for k in range(len(pts))], dtype=np.int32).reshape(len(pts), 2)
    xy = np.zeros((2, 8, 2))
    for k, p in enumerate(pts):
        xy[0, k] = xy[1, k] = p
    v, n, a = G.view_overlap_costs(pf, None, xy, W, H, 0, 1e-12)
    assert v[0, 1] == -1 and v[1, 0] == -1 and int(n[0, 1]) == len(pts) and a[0, 1] == 0.0


def test_the_exact_area_of_known_hulls():
    sq = [(0.0, 0.0), (4.0, 0.0), (4.0, 3.0), (0.0, 3.0), (2.0, 1.0), (1.0, 2.0), (4.0, 3.0)]
    assert G.exact_hull_area(sq) == 12.0
    assert G.exact_hull_area([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]) == 0.5


def test_the_distance_cut_removes_an_edge_with_a_positive_count_and_leaves_the_count():
    r = group(3, [(0, 1)] * 7 + [(1, 2)] * 5, far=(2,))
    assert r["cut"] == [(1, 2)] and r["vcosts"][1, 2] == -1 and r["vcosts"][2, 1] == -1 and int(r["nShare"][1, 2]) == 5
    assert r["groups"] == [[0, 1], [2]]


def test_the_planted_scenes_exercise_what_the_gpu_tests_rely_on():
    scenes = G.scene_set()
    G.assert_scene_conditions(scenes, G.scene_results(scenes))


def test_the_library_exports_the_grouping_entries_and_the_module_imports():
    import coslam_amd
    import coslam_amd.grouping as grouping

    lib = coslam_amd.lib()
    for s in ("cs_view_overlap_costs_dev", "cs_camera_grouping_dev", "cs_camera_grouping_scratch_bytes"):
        assert hasattr(lib, s), s
    assert coslam_amd.camera_grouping_dev is grouping.camera_grouping_dev
    assert grouping.camera_grouping_scratch_bytes(8, 2000) >= 4 * 257 + 8 * 256


def test_no_device_means_the_grouping_wrappers_fail_loudly():
    import coslam_amd
    from coslam_amd.grouping import camera_grouping_dev, view_overlap_costs_dev

    if coslam_amd.lib().cs_device_count() > 0:
        pytest.skip("a GPU is visible here")
    cams = [dict(xy=8, R=8, t=8), dict(xy=8, R=8, t=8)]   # (never dereferenced: the call fails before any launch)
    with pytest.raises(coslam_amd.CoslamHipError):
        view_overlap_costs_dev(0, cams, 16, 32, 0, 8, 0, W, H, 8, 8, 8)
    with pytest.raises(coslam_amd.CoslamHipError):
        camera_grouping_dev(0, cams, 16, 32, 0, 8, 0, W, H, 8, 8, 8, 1.0, 8)
