"""cs_merge_constraints_apply_map_dev on the device against the restatement tests/mergemap_ref.py, which the CPU tests pin to the
post-state of the reference's own objects (tests/golden/mergeconstraints_golden.npz).  Every comparison is exact: integers and copied
doubles."""
import numpy as np
import pytest

import coslam_amd
from tests import mergeconstraints_ref as ref
from tests import mergemap_planted as planted
from tests import mergemap_ref as mref
from tests.mergeconstraints_dev import DeviceScene, assemble_dev
from tests.mergeconstraints_golden_util import expand, load
from tests.mergeconstraints_scenes import make_scene
from tests.mergemap_dev import TABLES, MapTables, handle_bytes, poke, same_tables, with_tables

pytestmark = pytest.mark.gpu

SCENES = load()
COUNTS0 = (5, 4, 3, 2, 1, 9)          # d_counts is accumulated, never cleared


def _dev():
    import torch

    return torch.device("cuda:0")


def _run(S, f1, solve=False, apply_points=True, matches=None):
    """scene -> assembly (-> solves) -> map update; the device's tables against the restatement's, and everything the call must leave
    alone against its state before.  Returns (tables, want, views, problem, solution or None)."""
    S = with_tables(S)
    D = DeviceScene(S, _dev())
    mc, P, views = assemble_dev(D, f1, matches=matches)
    A = ref.assemble(S if matches is None else dict(S, matches=np.asarray(matches, np.int32).reshape(-1, 2)), f1)
    assert views.tolist() == [[int(x) for x in v] for v in A["views"]]
    sol = None
    if solve:
        mc.solve()
        sol = mc.solution(1)
    T = MapTables(D, COUNTS0)
    scene_before, handle_before = D.snapshot(), handle_bytes(mc)
    T.apply(mc, apply_points)
    got = T.download()
    with_pts = solve and apply_points and P["header"].verdict == 1
    want = mref.apply_map(S, views.tolist(), P["pointMap"] if with_pts else None, sol["pts"] if with_pts else None, f1)
    want["counts"] = [a + b for a, b in zip(COUNTS0, want["counts"])]
    same_tables(got, want)
    scene_after = D.snapshot()
    for k in ("K", "xy", "state", "groups", "histR", "histT", "segs"):
        if k in scene_before:
            assert scene_before[k].tobytes() == scene_after[k].tobytes(), k
    assert handle_bytes(mc) == handle_before
    # rows and slots the list does not name: as before
    start = mref.tables(S)
    rows, slots = np.zeros((S["nMap"], S["nC"]), bool), np.zeros((S["nC"], S["N"]), bool)
    for v in views.tolist():
        rows[v[3], v[1]], slots[v[1], v[2]] = True, True
    for k in ("featRef", "refStatic", "pointFeat"):
        assert np.array_equal(got[k][~rows], start[k][~rows]), k
    assert np.array_equal(got["slot2map"][~slots], start["slot2map"][~slots])
    if not with_pts:
        assert got["M"].tobytes() == start["M"].tobytes() and got["counts"][4] == COUNTS0[4]
    mc.close()
    D.th.close()
    return got, want, views.tolist(), P, sol


@pytest.mark.parametrize("sc", range(len(SCENES)))
def test_golden_scenes(hip, sc):
    """all four tables bit for bit as the restatement gives them; slot2map on the feature slots is the reference's cur_mpt; the history's
    poses and segments, the handle's buffers and every row the list does not name are byte-identical; a rejected verdict changes nothing"""
    S, G = SCENES[sc]
    got, want, views, P, _ = _run(S, int(G["first_frame"]))
    assert np.array_equal(np.where(np.isin(S["state"], (0, 1)), got["slot2map"], -1), G["cur_mpt"])
    assert np.array_equal(np.where(got["featRef"][:, :, :1] >= 0, got["featRef"][:, :, :2], -1), G["pfeat"])
    if int(G["verdict"]) != 1:
        start = mref.tables(with_tables(S))
        for k in TABLES:
            assert got[k].tobytes() == start[k].tobytes(), k
        assert got["counts"] == list(COUNTS0)
    else:
        assert got["counts"][0] == COUNTS0[0] + len(views) > COUNTS0[0] and got["counts"][1] > COUNTS0[1]


def test_repeated_call_and_null_optionals(hip):
    """the winner tables are restored by the kernel itself: a second handle-sharing call on fresh tables gives the same result; pointFeat,
    refStatic and counts may be NULL"""
    S, G = SCENES[5]
    S, f1 = with_tables(S), int(G["first_frame"])
    D = DeviceScene(S, _dev())
    mc, P, views = assemble_dev(D, f1)
    want = mref.apply_map(S, views.tolist(), f1=f1)
    first = MapTables(D)
    first.apply(mc)
    same_tables(first.download(), want)
    D2 = DeviceScene(S, _dev())                      # fresh tables, the SAME handle
    T = MapTables(D2)
    T.apply(mc)
    same_tables(T.download(), want)
    D3 = DeviceScene(S, _dev())
    T3 = MapTables(D3)
    T3.apply(mc, with_optional=False)
    g3 = T3.download()
    assert g3["slot2map"].tobytes() == want["slot2map"].tobytes() and g3["featRef"].tobytes() == want["featRef"].astype(np.int32).tobytes()
    assert g3["pointFeat"].tobytes() == np.asarray(S["pointFeat"], np.int32).tobytes() and g3["counts"] == [0] * 6
    mc.close()
    for d in (D, D2, D3):
        d.th.close()


@pytest.mark.parametrize("case", ("shared_row", "slot_in_two_tracks", "from_is_an_m1", "detached_then_named_again"))
@pytest.mark.parametrize("sc", (1, 5))
def test_planted_lists(hip, sc, case):
    """two tracks that share (m1, c); one slot in two tracks; a `from` that is another track's m1 (gather before scatter); a DETACHED view
    that is not the last one of its slot -- each built by editing the scene so that the ASSEMBLED list holds it (tests/mergemap_planted.py)"""
    S, G = SCENES[sc]
    f1 = int(G["first_frame"])
    made = getattr(planted, case)(S, f1)
    P, extra = made if isinstance(made, tuple) else (made, None)
    got, want, views, _, _ = _run(P, f1)
    if case == "from_is_an_m1":
        A, B, C, c = extra
        assert np.array_equal(got["featRef"][C][c], S["featRef"][A][c]) and np.array_equal(got["featRef"][A][c], S["featRef"][B][c])
    if case == "detached_then_named_again":
        c, s = extra
        assert got["slot2map"][c][s] == -1
    assert got["counts"][5] > COUNTS0[5]


def test_moved_reference_with_a_linked_segment(hip):
    """a reference that moves from m2 to m1 with a segment behind it: the row arrives whole, seg field included"""
    S, G = SCENES[5]
    got, _, views, _, _ = _run(S, int(G["first_frame"]))
    win = {(v[3], v[1]): v for v in views}
    moved = [(m1, c, v[4]) for (m1, c), v in win.items() if v[4] != m1 and S["featRef"][v[4]][c][3] >= 0]
    assert moved
    for m1, c, fr in moved:
        assert np.array_equal(got["featRef"][m1][c], S["featRef"][fr][c])
        assert mref.walk_chain(S, c, got["featRef"][m1][c]) == mref.walk_chain(S, c, S["featRef"][fr][c])


def test_hand_made_list_with_entries_outside_the_tables(hip):
    """cameras, slots and rows outside the tables in the views and in pointMap: skipped and counted as lost, nothing else moves"""
    S, G = SCENES[0]
    S, f1 = with_tables(S), int(G["first_frame"])
    D = DeviceScene(S, _dev())
    mc, P, views = assemble_dev(D, f1)
    mc.solve()
    nC, N, nMap = S["nC"], S["N"], S["nMap"]
    good = views.tolist()[:4]
    made = good + [[9, nC, 0, 0, 1, 0, -1], [9, -1, 0, 0, 1, 2, -1], [9, 0, N, 0, 1, 2, -1], [9, 0, -5, 0, 1, 0, -1], [9, 0, 1, nMap, 1, 0, -1],
                   [9, 0, 1, 0, -1, 2, -1], [9, 0, 2 ** 30, 2 ** 30, 2 ** 30, 2, -1]] + views.tolist()[4:6]
    poke(mc.buf.views, np.array([v + [0] for v in made], np.int32))
    poke(mc.buf.header + 32, np.array([len(made)], np.int32))                       # nMergeViews
    pm = P["pointMap"].copy()
    pm[1], pm[2], pm[3] = nMap, -1, 2 ** 30
    poke(mc.buf.pointMap, pm)
    T = MapTables(D, COUNTS0)
    T.apply(mc)
    want = mref.apply_map(S, made, pm, mc.solution(1)["pts"], f1)
    assert want["counts"][5] >= 7 + 3 and want["counts"][0] == 6
    want["counts"] = [a + b for a, b in zip(COUNTS0, want["counts"])]
    same_tables(T.download(), want)
    mc.close()
    D.th.close()


def _made(spec, seed):
    S = expand(make_scene(0, spec, np.random.default_rng(seed)))
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    return S, int(S["key_frames"][ref.first_constrain(S["key_frames"], S["self_motion"], ids)[0]])


def test_sixteen_cameras(hip):
    """two groups of 8 cameras"""
    spec = dict(groups=[[0, 3, 1, 2, 4, 7, 6, 5], [8, 9, 15, 14, 13, 12, 11, 10]], g=(1, 0), ij=(12, 3), nF=12, gaps=(2, 3, 4),
                moved=[{1, 9}, set(), set(range(16))], nA=60, nB=60, nMatch=14, plant="shared")
    S, f1 = _made(spec, 300)
    got, _, views, _, _ = _run(S, f1, solve=True)
    assert S["nC"] == 16 and max(v[1] for v in views) >= 12 and got["counts"][4] > COUNTS0[4]


def test_more_views_and_points_than_one_pass(hip):
    """more than 1024 tracks: the merge list and pointMap both cross a pass of the workgroup"""
    spec = dict(groups=[[0, 1], [3, 2]], g=(0, 1), ij=(1, 3), nF=10, gaps=(3, 2, 2), moved=[{0, 1, 2, 3}, {1}, set()], nA=500, nB=500, nMatch=420,
                plant="mixed")
    S, f1 = _made(spec, 301)
    got, _, views, P, _ = _run(S, f1, solve=True)
    assert len(views) > 1024 and P["header"].P > 1024 and got["counts"][4] > COUNTS0[4]


def test_solved_points_highest_index_wins(hip):
    """with solve(): M at the rows of pointMap is solution(1) by the highest-index rule, every other row byte-identical.  The scene has two
    tracks of one m1, so pointMap names that row twice with DIFFERENT solved values (other measurements); an unmerged point seen by k
    cameras is listed k times too."""
    S, G = SCENES[1]
    f1 = int(G["first_frame"])
    Pl = planted.shared_row(S, f1)
    got, want, views, P, sol = _run(Pl, f1, solve=True)
    pm, pts = P["pointMap"], sol["pts"]
    dup = [m for m in set(pm.tolist()) if (pm == m).sum() > 1]
    differ = [m for m in dup if len(set(pts[i].tobytes() for i in np.nonzero(pm == m)[0])) > 1]
    assert dup and differ, (len(dup), len(differ))
    for m in range(Pl["nMap"]):
        ix = np.nonzero(pm == m)[0]
        if len(ix):
            assert got["M"][m].tobytes() == pts[ix[-1]].tobytes()
        else:
            assert got["M"][m].tobytes() == np.asarray(Pl["M"], np.float64)[m].tobytes()
    for m in differ:
        assert got["M"][m].tobytes() != pts[np.nonzero(pm == m)[0][0]].tobytes()
    assert got["counts"][4] - COUNTS0[4] == len(set(pm.tolist())) and got["counts"][4] - COUNTS0[4] < len(pm)


def test_without_a_solve_the_map_points_stay(hip):
    """no solve: the list is applied, M is byte-identical and counts[4] stays; the same with applyPoints = 0 behind a solve, and again
    after a new assembly (the earlier solve is not this assembly's)"""
    S, G = SCENES[4]
    f1 = int(G["first_frame"])
    _run(S, f1, solve=False)
    _run(S, f1, solve=True, apply_points=False)
    S = with_tables(S)
    D = DeviceScene(S, _dev())
    mc, P, views = assemble_dev(D, f1)
    mc.solve()
    mc.assemble(D.th, D.cams, D.featRef.data_ptr(), S["nMap"], D.M.data_ptr(), D.groups.data_ptr(), S["gId1"], S["gId2"], S["maxiCam"], S["maxjCam"],
                f1, S["frame0"] + S["nF"] - 1, S["matches"])
    T = MapTables(D)
    T.apply(mc)
    got = T.download()
    same_tables(got, mref.apply_map(S, views.tolist(), f1=f1))
    assert got["counts"][4] == 0
    mc.close()
    D.th.close()


def test_refusals_before_any_launch(hip):
    """a null handle or table, nMap beyond the handle's maxMap, a null slot2map of one camera: CS_ERR_INVALID with its text, nothing written"""
    import ctypes as C

    S, G = SCENES[0]
    S = with_tables(S)
    D = DeviceScene(S, _dev())
    mc, P, views = assemble_dev(D, int(G["first_frame"]))
    T = MapTables(D)
    ptrs = [D.slot2map[c].data_ptr() for c in range(S["nC"])]
    args = (T.pointFeat.data_ptr(), D.featRef.data_ptr(), T.refStatic.data_ptr())
    with pytest.raises(coslam_amd.CoslamHipError, match="created for"):
        mc.apply_map(ptrs, *args, S["nMap"] + 1)
    with pytest.raises(coslam_amd.CoslamHipError, match="camera 1"):
        mc.apply_map([ptrs[0], 0] + ptrs[2:], *args, S["nMap"])
    with pytest.raises(coslam_amd.CoslamHipError, match="null"):
        mc.apply_map(ptrs, T.pointFeat.data_ptr(), None, T.refStatic.data_ptr(), S["nMap"])
    L = coslam_amd.lib()
    arr = (C.c_void_p * S["nC"])(*ptrs)
    assert L.cs_merge_constraints_apply_map_dev(None, None, arr, None, C.c_void_p(D.featRef.data_ptr()), None, S["nMap"], None, 1, None) == -1
    assert L.cs_merge_constraints_apply_map_dev(C.c_void_p(mc._m), None, None, None, C.c_void_p(D.featRef.data_ptr()), None, S["nMap"], None, 1, None) == -1
    got, start = T.download(), mref.tables(S)
    for k in TABLES:
        assert got[k].tobytes() == start[k].tobytes(), k
    mc.close()
    D.th.close()
