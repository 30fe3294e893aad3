"""The live view without a GPU: known answers, worked by hand, of the restatement of the curMapPts rule, CoSLAM::getNumDynamicStaticPoints,
CoSLAM::storeDynamicPoints and getDynTracks (tests/liveview_ref.py; reference src/app/SL_CoSLAM.cpp:1182-1197, :1447-1471, :1900-1911,
src/gui/GLScenePane.cpp:19-52), the C-ABI's new symbols and the loud failure of the wrappers where there is no device."""
import os

import numpy as np
import pytest

from tests import liveview_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(nCams, rows, mapCount=None):
    """rows: one (cameras, flags) per map point; point r lies at (r, 10 r, 100 r)"""
    pf = np.full((len(rows), nCams), -1, dtype=np.int32)
    flags = np.zeros(len(rows), dtype=np.uint8)
    for r, (cams, fl) in enumerate(rows):
        for c in cams:
            pf[r, c] = 7 + r
        flags[r] = fl
    pts = np.array([[r, 10.0 * r, 100.0 * r] for r in range(len(rows))], dtype=np.float64).reshape(len(rows), 3)
    return pf, flags, pts, len(rows) if mapCount is None else mapCount


def test_of_the_eight_flag_combinations_only_0_is_static_and_only_dynamic_alone_is_dynamic():
    pf, flags, pts, n = tables(2, [((0, 1), fl) for fl in range(8)])
    c = L.num_dynamic_static_points(pf, flags, n)
    assert c == dict(nStatic=1, nDynamic=1, nStaticFeat=[1, 1], nDynamicFeat=[1, 1])
    assert L.store_dynamic_points(pf, flags, pts, n) == [(1, 1.0, 10.0, 100.0)]          # flags == 1 is row 1
    cur = L.current_points(pf, flags, pts, n)
    assert [p[0] for p in cur] == list(range(8)) and [p[3] for p in cur] == list(range(8))   # false and uncertain points are listed, flagged


def test_the_counts_per_camera_follow_the_features():
    pf, flags, pts, n = tables(3, [((0,), 0), ((0, 2), 0), ((1, 2), 1), ((2,), 1), ((0, 1, 2), 4), ((1,), 2)])
    c = L.num_dynamic_static_points(pf, flags, n)
    assert c == dict(nStatic=2, nDynamic=2, nStaticFeat=[2, 0, 1], nDynamicFeat=[0, 1, 2])
    cur = L.current_points(pf, flags, pts, n)
    assert [(p[2], p[4]) for p in cur] == [(1, 1), (5, 2), (6, 2), (4, 1), (7, 3), (2, 1)]   # camMask, numVisCam


def test_a_row_beyond_the_map_count_and_a_row_with_no_feature_do_not_take_part():
    pf, flags, pts, n = tables(2, [((0,), 1), ((), 1), ((1,), 1), ((0, 1), 1)], mapCount=3)
    assert L.participating(pf, n) == [0, 2]
    assert L.num_dynamic_static_points(pf, flags, n)["nDynamic"] == 2
    assert [d[0] for d in L.store_dynamic_points(pf, flags, pts, n)] == [0, 2]
    assert L.participating(pf, 0) == [] and L.participating(pf, 99) == [0, 2, 3]


def test_one_camera_gives_an_empty_dynamic_list_but_a_filled_current_list_and_counts():
    pf, flags, pts, n = tables(1, [((0,), 1), ((0,), 0), ((0,), 1)])
    assert L.store_dynamic_points(pf, flags, pts, n) == []
    assert [p[0] for p in L.current_points(pf, flags, pts, n)] == [0, 1, 2]
    assert L.num_dynamic_static_points(pf, flags, n) == dict(nStatic=1, nDynamic=2, nStaticFeat=[1], nDynamicFeat=[2])


def P(pid, f):
    return (pid, float(f), float(pid), 0.5)


def test_trails_a_gap_is_skipped_an_absent_id_gets_none_ids_ascend_and_the_newest_comes_first():
    frames = [[P(9, 0), P(3, 0)],           # oldest
              [P(3, 1), P(9, 1), P(5, 1)],
              [P(9, 2), P(5, 2)],           # 3 is missing here
              [P(9, 3), P(3, 3)]]           # newest: 5 is absent
    t = L.get_dyn_tracks(frames, 150)        # longer than the frames held
    assert [pid for pid, _ in t] == [3, 9]                                   # ascending ids; 5 is not in the newest frame: no trail
    assert dict(t)[3] == [(3.0, 3.0, 0.5), (1.0, 3.0, 0.5), (0.0, 3.0, 0.5)]   # the gap at frame 2 is skipped, it does not end the trail
    assert dict(t)[9] == [(3.0, 9.0, 0.5), (2.0, 9.0, 0.5), (1.0, 9.0, 0.5), (0.0, 9.0, 0.5)]   # newest first
    t2 = L.get_dyn_tracks(frames, 2)
    assert dict(t2)[3] == [(3.0, 3.0, 0.5)] and dict(t2)[9] == [(3.0, 9.0, 0.5), (2.0, 9.0, 0.5)]
    assert L.get_dyn_tracks(frames, 0) == [] and L.get_dyn_tracks([], 5) == []
    assert L.get_dyn_tracks(frames[:3] + [[]], 4) == []                      # an empty newest frame: no trails at all


def test_the_caps_keep_the_first_entries_in_map_order():
    pf, flags, pts, n = tables(2, [((0, 1), 1)] * 9 + [((1,), 0)] * 11)
    h = L.header_of(pf, flags, pts, n, 8, 4)
    assert (h["nCur"], h["curOverflow"], h["nDyn"], h["dynOverflow"]) == (8, 12, 4, 5)
    assert [p[0] for p in h["cur"]] == list(range(8)) and [d[0] for d in h["dyn"]] == [0, 1, 2, 3]
    assert h["nStatic"] == 11 and h["nDynamic"] == 9                         # the counts are not cut


def test_the_library_exports_the_live_view_entries_the_header_declares_them_and_the_module_imports():
    import coslam_amd
    import coslam_amd.liveview as liveview

    lib = coslam_amd.lib()
    names = ("cs_liveview_create", "cs_liveview_destroy", "cs_liveview_frame_dev", "cs_liveview_newest", "cs_liveview_fetch", "cs_liveview_rings",
             "cs_liveview_trails", "cs_liveview_trails_dev", "cs_map_counts_dev", "cs_map_counts_scratch_bytes")
    header = open(os.path.join(ROOT, "include", "coslam_hip.h")).read()
    for s in names:
        assert hasattr(lib, s), s
        assert s + "(" in header, s
    assert coslam_amd.LiveView is liveview.LiveView
    assert liveview.map_counts_scratch_bytes() >= 4 * 35


def test_the_shim_and_its_driver_are_in_the_tree():
    assert os.path.exists(os.path.join(ROOT, "include", "shim", "app", "CoSLAMLiveView.h"))
    assert os.path.exists(os.path.join(ROOT, "tests", "cxx", "liveview_shim_test.cpp"))


def test_bad_arguments_are_refused_before_any_device_is_touched():
    import coslam_amd
    from coslam_amd.liveview import LiveView, map_counts_dev

    for kw in (dict(nCams=0), dict(nCams=17), dict(cur_cap=0), dict(dyn_cap=0), dict(depth=1), dict(trail_depth=0), dict(every=0)):
        a = dict(nCams=2, cur_cap=8, dyn_cap=8, depth=2, trail_depth=4, every=1)
        a.update(kw)
        with pytest.raises(coslam_amd.CoslamHipError, match="bad arguments"):
            LiveView(**a)
    with pytest.raises(coslam_amd.CoslamHipError, match="cameras"):
        map_counts_dev(0, 17, 32, 0, 8, 0, 8, 8)
    with pytest.raises(coslam_amd.CoslamHipError, match="null"):
        map_counts_dev(0, 2, 32, 0, 0, 0, 8, 8)


def test_no_device_means_the_live_view_wrappers_fail_loudly():
    import coslam_amd
    from coslam_amd.liveview import LiveView, map_counts_dev

    if coslam_amd.lib().cs_device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(coslam_amd.CoslamHipError):
        LiveView(2, 64, 16)
    with pytest.raises(coslam_amd.CoslamHipError):
        map_counts_dev(0, 2, 32, 0, 8, 0, 8, 8)   # (never dereferenced: the call fails before any launch)
