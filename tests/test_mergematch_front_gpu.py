"""MergeMatcher.run_front and MergeCamGroups.run_from_descriptors(device_jobs=True): the matcher's jobs filled on the
device from the front's buffers -- against the host-fed matcher given what the SAME device front returned (E, seeds), byte for byte, on
the scene of tests/mergefront_e2e.py (too few SURF matches / no E / the true pair) and, images in, on surf_scenes.banded_pair()."""
import numpy as np
import pytest

import coslam_amd
from coslam_amd.merge import MERGE_MATCH_SEEDS_OVERFLOW, MERGE_MATCH_SKIPPED, merge_match_fmat, ncc_small_image_dev
from tests import mergefront_dev as FD
from tests import mergefront_e2e as FE
from tests import mergematch_dev as D
from tests import mergematch_e2e as E2
from tests.mergemap_dev import SIGMA, Live

pytestmark = pytest.mark.gpu


def handles(S, max_seeds=None):
    mm = coslam_amd.MergeMatcher(S["nC"], S["N"], 4, S["N"] if max_seeds is None else max_seeds, 1 << 14, S["N"])
    mf = coslam_amd.MergeFront(S["nC"], S["N"], FE.DIM, 2, FE.N_RANSAC)          # 3 entries through 2 batch slots
    return mm, mf


def test_front_jobs_and_matches_equal_the_host_fed_matcher(hip):
    S, cams, infos, front_cams, want = FE.build()
    dc, keep = D.upload_cams(cams)
    fc, keep2 = FD.upload_cams(front_cams)
    mm, mf = handles(S)
    pairs = [(int(inf[1]), int(inf[4])) for inf in infos]
    mf.enqueue(fc, pairs, n_ransac=FE.N_RANSAC, seed=FE.GEN_SEED)
    mm.run_front(dc, E2.WS, E2.HS, pairs, mf)
    cnt = mm.counts(3)                                                             # the one wait
    fj = mm.front_jobs(3)
    res = mf.results(3)
    assert fj["flags"].tolist() == [MERGE_MATCH_SKIPPED, MERGE_MATCH_SKIPPED, 0] and (MERGE_MATCH_SKIPPED, MERGE_MATCH_SEEDS_OVERFLOW) == (4, 8)
    assert fj["n_seeds"].tolist() == [0, 0, res[2]["inlier_num"]] and res[2]["inlier_num"] == want[2]["inlier_num"] >= 18
    i, j = pairs[2]
    assert fj["F"][2].tobytes() == merge_match_fmat(cams[i]["K"], cams[j]["K"], res[2]["E"]).tobytes()
    assert np.isnan(fj["F"][:2]).all()
    assert cnt[0].tolist() == [0, 4, 0, 0] and cnt[1].tolist() == [0, 4, 0, 0]
    n = int(cnt[2][0])
    assert n > 20 and cnt[2][1] == 0
    got_m, got_s = mm.matches(2, n)
    # ---- the host-fed matcher, given the downloaded E and seeds of that same front
    mm2 = coslam_amd.MergeMatcher(S["nC"], S["N"], 4, S["N"], 1 << 14, S["N"])
    mm2.run(dc, E2.WS, E2.HS, [dict(iCam=i, jCam=j, E=res[2]["E"], seeds=mf.seeds(2, res[2]["inlier_num"]))])
    c2 = mm2.counts(1)
    assert c2[0].tolist() == cnt[2].tolist()
    ref_m, ref_s = mm2.matches(0, n)
    assert got_m.tobytes() == ref_m.tobytes() and got_s.tobytes() == ref_s.tobytes()
    for x in (mm, mm2, mf):
        x.close()


def test_run_from_descriptors_device_jobs_ends_where_the_host_fed_path_ends(hip):
    S, cams, infos, front_cams, want = FE.build()
    dc, keep = D.upload_cams(cams)
    fc, keep2 = FD.upload_cams(front_cams)
    reps, states, hs = [], [], []
    for device_jobs in (True, False):
        A = Live(S)
        mg = coslam_amd.MergeCamGroups(S["nC"], S["N"], S["N"], S["nMap"])
        mm, mf = handles(S)
        rep = mg.run_from_descriptors(mf, fc, mm, dc, E2.WS, E2.HS, infos, A.D.th, A.tables, S["groups"], S["key_frames"], S["self_motion"],
                                      A.key_groups, SIGMA, n_ransac=FE.N_RANSAC, seed=FE.GEN_SEED, device_jobs=device_jobs)
        reps.append(rep), states.append(A.state()), hs.append((A, mg, mm, mf))
    a, b = reps
    assert a["status"] == b["status"] == "merged" and a["choice"] == b["choice"] and a["choice"]["entry"] == 2
    assert a["header"] == b["header"] and a["apply_counts"] == b["apply_counts"] and a["recompute_counts"] == b["recompute_counts"]
    assert a["groups"] == b["groups"] and set(a) == set(b)
    assert a["job_of_entry"] == [-1, -1, 2] and b["job_of_entry"] == [-1, -1, 0]
    assert a["match_counts"].shape == (3, 4) and a["match_counts"][:2].tolist() == [[0, 4, 0, 0]] * 2
    assert a["match_counts"][2].tolist() == b["match_counts"][0].tolist() and a["match_counts"][2][0] > 20
    assert a["matches_ptr"] == hs[0][2].matches_ptr(2) and hs[0][1].mc._keep.data_ptr() == a["matches_ptr"]      # handed over, not copied
    assert all("seeds" not in g for g in a["front"]) and all("seeds" in g for g in b["front"])
    for ga, gb in zip(a["front"], b["front"]):
        assert all(np.array_equal(ga[k], gb[k]) for k in ga)
    for k in states[0]:
        assert states[0][k].tobytes() == states[1][k].tobytes(), k
    assert states[0]["histR"].tobytes() != np.asarray(S["histR"], np.float64).tobytes()                          # a real correction
    for A, mg, mm, mf in hs:
        mg.close(), mm.close(), mf.close(), A.close()


def test_more_inliers_than_seed_rows_flags_the_job_and_merges_nothing(hip):
    S, cams, infos, front_cams, want = FE.build()
    assert want[2]["inlier_num"] >= 18
    dc, keep = D.upload_cams(cams)
    fc, keep2 = FD.upload_cams(front_cams)
    A = Live(S)
    before = A.state()
    mg = coslam_amd.MergeCamGroups(S["nC"], S["N"], S["N"], S["nMap"], last_merge_frame=-1000)
    mm, mf = handles(S, max_seeds=8)
    rep = mg.run_from_descriptors(mf, fc, mm, dc, E2.WS, E2.HS, infos, A.D.th, A.tables, S["groups"], S["key_frames"], S["self_motion"],
                                  A.key_groups, SIGMA, n_ransac=FE.N_RANSAC, seed=FE.GEN_SEED, device_jobs=True)
    assert rep["match_counts"][2].tolist() == [0, 8, 0, 0] and rep["job_of_entry"] == [-1, -1, -1]
    assert rep["status"] == "no_pair" and not rep["merged"] and mg.last_merge_frame == -1000
    assert mm.front_jobs(3)["flags"].tolist() == [4, 4, 8]
    after = A.state()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    mg.close(), mm.close(), mf.close(), A.close()


def test_images_in_one_wait(hip):
    """Surf.enqueue -> MergeFront.enqueue -> MergeMatcher.run_front on one stream, one wait; against the host-fed matcher through the same
    device front.  The planted matcher cameras and the condition (>= 10 matches on the restatements) are tests/mergematch_front_scene.py's."""
    import torch

    from tests import mergematch_front_scene as P
    from tests import surf_scenes as SS
    from tests.test_surf_gpu import upload

    img1, img2, cams, Ws, Hs, job, ref_matches = P.build()
    assert len(ref_matches) >= P.MIN_MATCHES
    W, H, N = SS.E2E_W, SS.E2E_H, P.N
    s = torch.cuda.current_stream().cuda_stream
    t, p = upload([img1, img2])
    small = [torch.zeros(Ws * Hs, dtype=torch.uint8, device="cuda") for _ in range(2)]
    for im, sm in zip(t, small):
        assert ncc_small_image_dev(s, im.data_ptr(), W, H, P.SCALE, sm.data_ptr()) == (Ws, Hs)
    xy = [torch.as_tensor(c["xy"].reshape(-1), device="cuda") for c in cams]
    st = [torch.as_tensor(c["state"], device="cuda") for c in cams]
    dc = [dict(xy=xy[c].data_ptr(), state=st[c].data_ptr(), imgSmall=small[c].data_ptr(), K=cams[c]["K"], imgScale=P.SCALE) for c in range(2)]
    sf = coslam_amd.Surf(2, W, H, N)
    mf = coslam_amd.MergeFront(2, N, 64, 1, SS.N_RANSAC)
    mm = coslam_amd.MergeMatcher(2, N, 1, N, 1 << 14, N)
    sf.enqueue(t, SS.THRESHOLD, pitch=p)
    mf.enqueue(sf.front_cams([c["K"] for c in cams]), [(0, 1)], n_ransac=SS.N_RANSAC)
    mm.run_front(dc, Ws, Hs, [(0, 1)], mf)
    cnt = mm.counts(1)                                                             # the one wait
    res = mf.results(1)[0]
    assert (res["surf_num"], res["emat_ok"], res["inlier_num"]) == (job["surf_num"], 1, job["inlier_num"])
    assert [int(small[c].cpu().numpy().reshape(Hs, Ws).tobytes() == cams[c]["imgSmall"].tobytes()) for c in range(2)] == [1, 1]
    n = int(cnt[0][0])
    got_m, got_s = mm.matches(0, n)
    mm2 = coslam_amd.MergeMatcher(2, N, 1, N, 1 << 14, N)
    mm2.run(dc, Ws, Hs, [dict(iCam=0, jCam=1, E=res["E"], seeds=mf.seeds(0, res["inlier_num"]))])
    c2 = mm2.counts(1)
    print(f"device-fed {cnt[0].tolist()}, host-fed {c2[0].tolist()}, restatement {len(ref_matches)} matches")
    assert int(c2[0][0]) >= P.MIN_MATCHES and cnt[0].tolist() == c2[0].tolist() and cnt[0][1] == 0
    ref_m, ref_s = mm2.matches(0, n)
    assert got_m.tobytes() == ref_m.tobytes() and got_s.tobytes() == ref_s.tobytes()
    for x in (sf, mf, mm, mm2):
        x.close()
