"""MergeCamGroups.run_from_descriptors: from the gate's list and the key frames' key points + descriptors to the merged state --
against run_from_seeds fed the restatement front's E, seeds, surf_num and emat_ok (tests/mergefront_ref.py), byte for byte.  The scene
(tests/mergefront_e2e.py) asserts what makes that a fair demand: exact flags of the front, no matcher candidate within 1e-6 px of epiMax."""
import numpy as np
import pytest

import coslam_amd
from tests import mergefront_dev as FD
from tests import mergefront_e2e as FE
from tests import mergefront_scenes as FS
from tests import mergematch_dev as D
from tests import mergematch_e2e as E2
from tests.mergemap_dev import SIGMA, Live

pytestmark = pytest.mark.gpu


def test_run_from_descriptors_ends_where_the_restatement_front_ends(hip):
    S, cams, infos, front_cams, want = FE.build()
    dc, keep = D.upload_cams(cams)
    fc, keep2 = FD.upload_cams(front_cams)
    A = Live(S)
    mg = coslam_amd.MergeCamGroups(S["nC"], S["N"], S["N"], S["nMap"])
    mm = coslam_amd.MergeMatcher(S["nC"], S["N"], 4, S["N"], 1 << 14, S["N"])
    mf = coslam_amd.MergeFront(S["nC"], S["N"], FE.DIM, 2, FE.N_RANSAC)          # 3 entries through 2 batch slots
    rep = mg.run_from_descriptors(mf, fc, mm, dc, E2.WS, E2.HS, infos, A.D.th, A.tables, S["groups"], S["key_frames"], S["self_motion"],
                                  A.key_groups, SIGMA, n_ransac=FE.N_RANSAC, seed=FE.GEN_SEED)
    got = rep["front"]
    for g, w in zip(got, want):
        assert (g["surf_num"], g["emat_ok"], g["inlier_num"], g["rounds"]) == (w["surf_num"], w["emat_ok"], w["inlier_num"], w["rounds"])
        assert g["seeds"].tobytes() == np.ascontiguousarray(w["seeds"]).tobytes()
    assert got[2]["best_hyp"] == want[2]["best_hyp"] and np.abs(got[2]["E"] * np.sign(got[2]["E"] @ want[2]["E"]) - want[2]["E"]).max() <= FS.E_TOL
    assert rep["status"] == "merged" and rep["merged"] and rep["choice"]["entry"] == 2 and rep["job_of_entry"] == [-1, -1, 0]
    a = A.state()
    # ---- run_from_seeds fed the restatement front's answers, on a scene of its own
    B = Live(S)
    mg2 = coslam_amd.MergeCamGroups(S["nC"], S["N"], S["N"], S["nMap"])
    mm2 = coslam_amd.MergeMatcher(S["nC"], S["N"], 4, S["N"], 1 << 14, S["N"])
    rep2 = mg2.run_from_seeds(mm2, dc, E2.WS, E2.HS, infos, [w["surf_num"] for w in want], [w["emat_ok"] for w in want],
                              [dict(E=w["E"], seeds=w["seeds"]) for w in want], B.D.th, B.tables, S["groups"], S["key_frames"],
                              S["self_motion"], B.key_groups, SIGMA)
    b = B.state()
    assert rep2["status"] == "merged" and rep2["header"] == rep["header"] and rep2["choice"] == rep["choice"]
    assert np.array_equal(rep2["match_counts"], rep["match_counts"]) and rep["match_counts"][0][0] > 20
    n = int(rep["match_counts"][0][0])
    assert np.array_equal(mm.matches(0, n)[0], mm2.matches(0, n)[0])
    assert rep2["apply_counts"] == rep["apply_counts"] and rep2["recompute_counts"] == rep["recompute_counts"] and rep2["groups"] == rep["groups"]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["histR"].tobytes() != np.asarray(S["histR"], np.float64).tobytes()                          # a real correction
    for x in (mg, mg2, mm, mm2, mf):
        x.close()
    A.close(), B.close()
