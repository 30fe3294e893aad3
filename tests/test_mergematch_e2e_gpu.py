"""MergeCamGroups.run_from_seeds: from the gate's list with the host front's E and seeds to the merged state, the chosen job's
matches handed to the constraints as a DEVICE table -- against MergeCamGroups.run given the restatement's matches from the host."""
import numpy as np
import pytest

import coslam_amd
from tests import mergematch_dev as D
from tests import mergematch_e2e as E2
from tests import mergematch_ref as R
from tests.mergemap_dev import SIGMA, Live

pytestmark = pytest.mark.gpu


def _front(S, entry, job):
    """the gate's list: the true pair last, behind an entry with too few SURF matches and one whose computeEMat failed"""
    f2, g1, g2 = entry[0], S["gId1"], S["gId2"]
    infos = [(f2, 1, g1, f2, 3, g2), (f2, 1, g1, f2, 2, g2), entry]
    return infos, [10, 40, 60], [1, 0, 1], [dict(E=job["E"], seeds=job["seeds"]), None, dict(E=job["E"], seeds=job["seeds"])]


def test_run_from_seeds_merges_with_the_matchers_device_table(hip):
    S, cams, entry, job = E2.build()
    ref = R.match_job(cams, E2.WS, E2.HS, job)
    want_m, want_s = D.as_arrays(ref["matches"])
    infos, surf, ok, jobs = _front(S, entry, job)
    A = Live(S)
    mg = coslam_amd.MergeCamGroups(S["nC"], S["N"], S["N"], S["nMap"])
    mm = coslam_amd.MergeMatcher(S["nC"], S["N"], 4, 16, 1 << 14, S["N"])
    dc, keep = D.upload_cams(cams)
    rep = mg.run_from_seeds(mm, dc, E2.WS, E2.HS, infos, surf, ok, jobs, A.D.th, A.tables, S["groups"], S["key_frames"], S["self_motion"],
                            A.key_groups, SIGMA)
    assert rep["status"] == "merged" and rep["merged"] and rep["verdict"] == 1
    assert rep["choice"]["entry"] == 2 and rep["job_of_entry"] == [-1, -1, 0]
    assert (rep["choice"]["maxgId1"], rep["choice"]["maxgId2"], rep["choice"]["maxiCam"], rep["choice"]["maxjCam"]) == A.pair
    cnt = rep["match_counts"][0]
    assert cnt[0] == len(want_m) > 20 and cnt[1] == 0
    m, s = mm.matches(0, cnt[0])
    assert np.array_equal(m, want_m) and np.array_equal(s.view(np.int64), want_s.view(np.int64))
    assert rep["matches_ptr"] == mm.matches_ptr(0) and mg.mc._keep.data_ptr() == mm.matches_ptr(0)      # handed over, not copied
    assert rep["header"]["nMergedTracks"] + rep["header"]["skippedMatches"] == len(want_m)
    a = A.state()
    # ---- run() handed those same matches from the host, on a scene of its own
    B = Live(dict(S, matches=want_m))
    mg2 = coslam_amd.MergeCamGroups(S["nC"], S["N"], S["N"], S["nMap"])
    rep2 = B.run(mg2)
    b = B.state()
    assert rep2["status"] == "merged" and rep2["header"] == rep["header"]
    assert rep2["apply_counts"] == rep["apply_counts"] and rep2["recompute_counts"] == rep["recompute_counts"] and rep2["groups"] == rep["groups"]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["histR"].tobytes() != np.asarray(S["histR"], np.float64).tobytes()                          # a real correction
    for x in (mg, mg2, mm):
        x.close()
    A.close(), B.close()


def test_withheld_matcher_output_merges_nothing(hip):
    """zero jobs (the host front found nothing): no pair, nothing enqueued behind the matcher, every table byte-identical"""
    S, cams, entry, job = E2.build()
    infos, surf, ok, jobs = _front(S, entry, job)
    A = Live(S)
    before = A.state()
    mg = coslam_amd.MergeCamGroups(S["nC"], S["N"], S["N"], S["nMap"], last_merge_frame=-1000)
    mm = coslam_amd.MergeMatcher(S["nC"], S["N"], 4, 16, 1 << 14, S["N"])
    dc, keep = D.upload_cams(cams)
    rep = mg.run_from_seeds(mm, dc, E2.WS, E2.HS, infos, surf, ok, [None] * 3, A.D.th, A.tables, S["groups"], S["key_frames"], S["self_motion"],
                            A.key_groups, SIGMA)
    after = A.state()
    assert rep["status"] == "no_pair" and not rep["merged"] and rep["choice"]["status"] == 0 and mg.last_merge_frame == -1000
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    mg.close(), mm.close()
    A.close()
