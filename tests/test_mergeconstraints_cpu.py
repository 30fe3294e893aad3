"""The merge constraints on the host: the plain restatement tests/mergeconstraints_ref.py reproduces the reference's own
MergeCameraGroup::genMergeInfoVer2 (tests/golden/mergeconstraints_golden.npz, recorded with a solver stand-in that changes nothing) bit for
bit; cs_merge_first_constrain equals the reference's m_pFirstConstrainFrm and pose order; the library exports what the header declares."""
import os
import re

import numpy as np
import pytest

import coslam_amd
from tests import mergeconstraints_ref as ref
from tests.mergeconstraints_golden_util import GOLDEN, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = load()
IDS = range(len(SCENES))


def _f1(G):
    return int(G["first_frame"])


def test_golden_covers_the_cases():
    """six scenes; the generator asserts every case of the list, this only keeps the file's shape in view"""
    assert len(SCENES) >= 5 and os.path.getsize(GOLDEN) < 1137966
    sizes = [sorted(len(S["groups"][g]) for g in (S["gId1"], S["gId2"])) for S, _ in SCENES]
    assert [1, 2] in sizes and any(sum(s) >= 9 for s in sizes)
    assert any(int(G["verdict"]) == 0 for _, G in SCENES) and any(len(S["matches"]) == 3 for S, _ in SCENES)


@pytest.mark.parametrize("sc", IDS)
def test_restatement_reproduces_the_reference(sc):
    """header, camera order, pointMap, obs_ptr / obs_cam / obs_xy, avgErr, the poses, and the MergeInfo ints and R / t"""
    S, G = SCENES[sc]
    A = ref.assemble(S, _f1(G))
    assert A["verdict"] == int(G["verdict"]) and A["avgErr"] == float(G["avgErr"])
    assert A["order"] == [tuple(int(v) for v in r) for r in G["order"]]
    if A["verdict"] != ref.VERDICT_MERGE:
        assert A["avgErr"] > 500 and len(G["pts"]) == 0 and len(G["info_ints"]) == 0 and A["views"] == [] and A["pointMap"] == []
        return
    assert A["avgErr"] <= 500
    for k in ("Ks", "Rs", "Ts", "pts", "obs_xy"):
        assert np.array_equal(np.array(A[k]).reshape(G[k].shape), G[k]), k
    for k in ("pointMap", "obs_ptr", "obs_cam"):
        assert np.array_equal(np.array(A[k]), G[k]), k
    assert G["ba_args"].tolist() == [[1, 1, 1, 100, 800], [1, 1, 5, 30, 30]]          # :646-647
    ints, R, t = ref.merge_infos(S, A["Rs"], A["Ts"], A["order"])
    assert np.array_equal(np.array(ints), G["info_ints"][:, :6]) and (G["info_ints"][:, 6] == 1).all()
    assert np.array_equal(np.array(R), G["info_R"]) and np.array_equal(np.array(t), G["info_t"])


@pytest.mark.parametrize("sc", IDS)
def test_merge_list_gives_the_recorded_post_state(sc):
    """the emitted merge list, applied, is what mergeMapPoints and the duplicate marks left in the reference's objects: every current
    feature's map point, every point's references, the detached nodes"""
    S, G = SCENES[sc]
    A = ref.assemble(S, _f1(G))
    cur, pfeat, det = ref.apply_views(S, A["views"], _f1(G))
    assert np.array_equal(np.array(cur), G["cur_mpt"]) and np.array_equal(np.array(pfeat), G["pfeat"])
    assert [list(d) for d in det] == sorted(G["detached"].tolist())
    if A["verdict"] != ref.VERDICT_MERGE:
        assert np.array_equal(G["cur_mpt"], np.where(np.isin(S["state"], (0, 1)), S["slot2map"], -1))     # a rejected merge touches nothing


@pytest.mark.parametrize("sc", IDS)
def test_first_constrain_equals_the_reference(sc):
    S, G = SCENES[sc]
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    k, order = coslam_amd.merge_first_constrain(S["key_frames"], S["self_motion"], ids)
    assert int(S["key_frames"][k]) == _f1(G) and order == [tuple(int(v) for v in r) for r in G["order"]]
    assert (k, order) == ref.first_constrain(S["key_frames"], S["self_motion"], ids)


def test_first_constrain_rule_and_refusals():
    frames = [10, 20, 30, 40, 50]
    sm = np.zeros((5, 3), np.uint8)
    sm[3, 0] = sm[2, 0] = sm[0, 0] = 1        # camera 0: the newest two are frames 40 and 30; frame 10 is a third and is not visited
    sm[1, 2] = 1                              # camera 2: only frame 20
    assert coslam_amd.merge_first_constrain(frames, sm, [0, 1])[0] == 2
    k, order = coslam_amd.merge_first_constrain(frames, sm, [0, 2])
    assert k == 1 and order == [(50, 0), (50, 2), (20, 0), (20, 2)]
    assert coslam_amd.merge_first_constrain(frames, sm, [2])[0] == 1
    sm[4, 1] = 1                              # the current key frame's own flag is not read
    with pytest.raises(coslam_amd.CoslamHipError, match="self-motion"):
        coslam_amd.merge_first_constrain(frames, sm, [1])
    assert ref.first_constrain(frames, sm, [1]) is None
    for bad in (dict(frames=[10, 10, 30, 40, 50]), dict(ids=[2, 0]), dict(ids=[0, 3])):
        with pytest.raises(coslam_amd.CoslamHipError):
            coslam_amd.merge_first_constrain(bad.get("frames", frames), sm, bad.get("ids", [0, 1]))


def test_symbols_and_structs():
    """every cs_merge_* name the header declares is exported (the mirrors' layouts: tests/test_abi.py's table)"""
    hdr = open(os.path.join(ROOT, "include", "coslam_hip.h")).read()
    names = sorted(set(re.findall(r"\b(cs_merge_[a-z_]+)\(", hdr)))
    for need in ("cs_merge_first_constrain", "cs_merge_constraints_create", "cs_merge_constraints_assemble_dev", "cs_merge_info_dev",
                 "cs_merge_constraints_solve", "cs_merge_constraints_solution", "cs_merge_constraints_info_dev", "cs_merge_constraints_buffers_get", "cs_merge_constraints_header_get", "cs_merge_constraints_download", "cs_merge_constraints_destroy"):
        assert need in names, need
    L = coslam_amd.lib()
    for name in names:
        assert hasattr(L, name), name
    assert all(hasattr(coslam_amd, n) for n in ("MergeConstraints", "merge_first_constrain"))
