"""The merge pose correction without a device: the numpy restatement (tests/mergegraph_ref.py) of computeNewCameraRotations +
computeNewCameraTranslations4 against the reference's own outputs (tests/golden/mergegraph_golden.npz, written by
tests/cxx/ref_mergegraph_test.cpp), the rank condition on the fixture, and cs_merge_keygraph_plan (host code of libcoslam_hip)
against the restatement of searchFirstKeyFrameForMerge + _constructGraphForKeyFrms, exactly.

Tolerance: TOL_R / TOL_T of tests/test_posegraph_gpu.py, by the same argument -- two factorisations (the stand-in's QR there,
lstsq's SVD here) of one full-rank least-squares problem; the scales are unknowns of the translation system: TOL_T."""
import os

import numpy as np
import pytest

import coslam_amd
from coslam_amd.synth import make_merge_pose_graph
from tests import mergegraph_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mergegraph_golden.npz")
TOL_R, TOL_T = 1e-10, 1e-9
# (cameras, key frames, first-constrained key frame, split) of the golden merge graphs, as tests/cxx/ref_mergegraph_test.cpp builds them
MERGE_SHAPES = {"merge_2x3": (2, 3, 1, 1), "merge_3x4": (3, 4, 2, 1), "merge_8x6": (8, 6, 3, 4), "merge_16x4": (16, 4, 2, 8),
                "merge_8x24": (8, 24, 15, 4)}


def golden_graphs():
    g = np.load(GOLD)
    out = []
    for k, name in enumerate(g["names"]):
        ns, es = slice(g["node_ptr"][k], g["node_ptr"][k + 1]), slice(g["edge_ptr"][k], g["edge_ptr"][k + 1])
        d = {key: g[key][ns] for key in ("fixed", "nodeR", "nodeT", "newR", "newT", "frame", "cam", "node_constraint")}
        d.update({key: g[key][es] for key in ("id1", "id2", "scale_id", "edgeR", "edgeT", "edgeS", "edge_constraint")})
        d["name"], d["n_constraint"], d["n_fixed"] = str(name), int(g["n_constraint"][k]), int(g["n_fixed"][k])
        out.append(d)
    return out


@pytest.fixture(scope="module")
def restated():
    return [(d, ref.relax_scaled(d["fixed"], d["nodeR"], d["nodeT"], d["id1"], d["id2"], d["edgeR"], d["edgeT"], d["scale_id"]))
            for d in golden_graphs()]


def test_fixture_holds_the_graphs_the_pin_needs():
    gs = {d["name"]: d for d in golden_graphs()}
    assert list(gs) == list(MERGE_SHAPES) + ["two_scales", "shared_scale", "fixed_id2", "fixed_id1"]
    for name, (nc, nk, _f, _s) in MERGE_SHAPES.items():
        d = gs[name]
        assert len(d["fixed"]) == nc * nk and d["n_fixed"] == nc and d["n_constraint"] == (d["scale_id"] >= 0).sum() > 0
        assert np.array_equal(d["edge_constraint"] != 0, d["scale_id"] >= 0)
        ends = np.unique(np.concatenate([d["id1"][d["scale_id"] >= 0], d["id2"][d["scale_id"] >= 0]]))
        assert np.array_equal(np.nonzero(d["node_constraint"])[0], ends)
    assert sorted(set(gs["two_scales"]["scale_id"][gs["two_scales"]["scale_id"] >= 0])) == [0, 3]
    d = gs["fixed_id2"]
    sc = d["scale_id"] >= 0
    assert (d["fixed"][d["id2"][sc]] != 0).any() and (d["fixed"][d["id1"][sc]] & d["fixed"][d["id2"][sc]]).any()
    d = gs["fixed_id1"]
    sc = d["scale_id"] >= 0
    assert ((d["fixed"][d["id1"][sc]] != 0) & (d["fixed"][d["id2"][sc]] == 0)).any()


def test_every_golden_system_has_full_column_rank(restated):
    for d, (_r, _t, _s, A) in restated:
        assert np.linalg.matrix_rank(A) == A.shape[1], d["name"]


def test_restatement_matches_the_reference_golden(restated):
    for d, (newR, newT, edgeS, _A) in restated:
        dR, dT, dS = np.abs(newR - d["newR"]).max(), np.abs(newT - d["newT"]).max(), np.abs(edgeS - d["edgeS"]).max()
        print(f"{d['name']}: |dR| {dR:.2e} |dt| {dT:.2e} |ds| {dS:.2e}")
        assert dR < TOL_R and dT < TOL_T and dS < TOL_T, d["name"]
        sc = d["scale_id"] >= 0
        assert np.all(d["edgeS"][~sc] == 0) and np.all(d["edgeS"][sc] != 0)
        for s in set(d["scale_id"][sc]):
            assert len(set(d["edgeS"][d["scale_id"] == s])) == 1             # one unknown per id


def _same(plan, want):
    assert want is not None
    assert plan["fixed_kf"] == want["fixed_kf"] and plan["n_constraint"] == want["n_constraint"]
    for k in ("node_kf", "node_cam", "fixed", "id1", "id2", "scale_id"):
        assert np.array_equal(plan[k], want[k]), k


@pytest.mark.parametrize("name", list(MERGE_SHAPES))
def test_keygraph_plan_on_the_golden_topologies(name):
    nc, nk, f, split = MERGE_SHAPES[name]
    m = make_merge_pose_graph(nc, nk, f, split, seed=1)
    args = (m["frames"], m["groups"], m["cam_ids"], m["first_constrain"], m["camid1"], m["camid2"], m["infos"])
    plan = coslam_amd.merge_keygraph_plan(*args)
    _same(plan, ref.keygraph_plan(*args))
    d = {g["name"]: g for g in golden_graphs()}[name]                        # ... and it IS the graph the reference's classes were given
    assert plan["fixed_kf"] == 0
    for k, key in (("fixed", "fixed"), ("id1", "id1"), ("id2", "id2"), ("scale_id", "scale_id"), ("node_cam", "cam")):
        assert np.array_equal(plan[k], d[key]), k
    assert np.array_equal(np.asarray(m["frames"])[plan["node_kf"]], d["frame"])
    for k in ("fixed", "id1", "id2", "scale_id"):
        assert np.array_equal(m[k], plan[k]), k                              # the generator's own topology


def _case(n_key, groups, cam_ids, first, c1, c2, infos, n_max=100):
    frames = [7 * k + 3 for k in range(n_key)]
    infos = [(frames[a], ca, frames[b], cb) for (a, ca, b, cb) in infos]
    return (frames, groups, cam_ids, first, c1, c2, infos, n_max)


def test_keygraph_plan_refuses_a_first_constrained_frame_with_no_older_key_frame():
    args = _case(3, [[[0], [1]]] * 3, [0, 1], 0, 0, 1, [(0, 0, 2, 1)])
    assert ref.keygraph_plan(*args) is None
    with pytest.raises(coslam_amd.CoslamHipError, match="older"):
        coslam_amd.merge_keygraph_plan(*args)


def test_keygraph_plan_search_quirks():
    sep, tog = [[0], [1]], [[0, 1]]
    # nMaxKeyFrame reached before a shared group is found: n <= nMax lets nMax + 1 older frames be visited, the last becomes fixed
    args = _case(8, [tog] + [sep] * 7, [0, 1], 6, 0, 1, [(6, 0, 7, 1)], n_max=2)
    want = ref.keygraph_plan(*args)
    assert want["fixed_kf"] == 3
    _same(coslam_amd.merge_keygraph_plan(*args), want)
    # the cameras share a group in the first older frame: that frame is the fixed one
    args = _case(5, [sep, sep, tog, sep, sep], [0, 1], 3, 0, 1, [(3, 0, 4, 1), (4, 0, 4, 1)])
    want = ref.keygraph_plan(*args)
    assert want["fixed_kf"] == 2 and want["n_constraint"] == 2
    _same(coslam_amd.merge_keygraph_plan(*args), want)
    # no shared group anywhere: the oldest key frame
    args = _case(4, [sep] * 4, [0, 1], 2, 0, 1, [(2, 0, 3, 1)])
    assert ref.keygraph_plan(*args)["fixed_kf"] == 0
    _same(coslam_amd.merge_keygraph_plan(*args), ref.keygraph_plan(*args))


def test_keygraph_plan_groups_and_cam_id_sets():
    # a group with only one camera in camIds gives no intra-frame edge; group order (not ascending) orders the chain; cameras outside
    # camIds are passed over; the closing edge needs more than two
    groups = [[[4, 0, 2, 5]], [[2, 0, 3], [5, 1]], [[0, 3], [2, 5, 4]], [[0], [2], [5]]]
    args = _case(4, groups, [0, 2, 5], 2, 0, 2, [(2, 0, 3, 2), (3, 0, 3, 5)])
    want = ref.keygraph_plan(*args)
    plain = want["scale_id"] < 0
    assert want["id1"][0] == 1 and want["id2"][0] == 0                      # kf 1, group [2, 0, 3]: the edge 2 -> 0
    assert want["fixed_kf"] == 1 and len(want["id1"]) == 1 + (1 + 3) + 3 + 2 and plain.sum() == 8
    _same(coslam_amd.merge_keygraph_plan(*args), want)
    # 1-element camIds: only successive-frame edges
    args = _case(3, [[[0, 1]], [[0], [1]], [[0], [1]]], [1], 1, 0, 1, [])
    want = ref.keygraph_plan(*args)
    assert len(want["id1"]) == 2 and want["n_constraint"] == 0
    _same(coslam_amd.merge_keygraph_plan(*args), want)
    # 16-element camIds, one group of 16 in the fixed frame (chain of 15 + the closing edge)
    ids = list(range(16))
    args = _case(3, [[ids[::-1]], [ids[:9], ids[9:]], [ids[:9], ids[9:]]], ids, 1, 0, 9, [(1, 0, 2, 9), (2, 8, 2, 15)])
    want = ref.keygraph_plan(*args)
    assert len(want["fixed"]) == 48 and want["fixed"].sum() == 16
    _same(coslam_amd.merge_keygraph_plan(*args), want)


def test_create_scaled_refuses_bad_scale_ids_before_it_asks_for_a_device():
    """the refusals of cs_posegraph_create_scaled are decided on the host: CS_ERR_INVALID (-1) with text, device or not"""
    fixed = np.array([1, 0, 0, 0, 0, 1], np.uint8)
    id1, id2 = np.arange(5, dtype=np.int32), np.arange(1, 6, dtype=np.int32)
    for sid, text in (([-1, 5, -1, -1, -1], "scale id 5"),):
        with pytest.raises(coslam_amd.CoslamHipError, match=text) as ei:
            coslam_amd.PoseGraphs([(fixed, id1, id2)], scale_ids=[sid])
        assert "code -1" in str(ei.value)
    with pytest.raises(coslam_amd.CoslamHipError, match="fixed nodes only") as ei:
        coslam_amd.PoseGraphs([(fixed, np.append(id1, 0).astype(np.int32), np.append(id2, 5).astype(np.int32))], scale_ids=[[-1, 0, -1, -1, -1, 2]])
    assert "code -1" in str(ei.value)
    f12 = np.zeros(12, np.uint8)
    f12[0] = 1
    with pytest.raises(coslam_amd.CoslamHipError, match="at most 4") as ei:
        coslam_amd.PoseGraphs([(f12, np.arange(11, dtype=np.int32), np.arange(1, 12, dtype=np.int32))], scale_ids=[[0, 1, 2, 3, 4] + [-1] * 6])
    assert "code -1" in str(ei.value)
