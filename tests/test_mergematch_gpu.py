"""The merge matcher on the device (cs_merge_match) against the plain restatement tests/mergematch_ref.py: blocks, F, the
candidate set, the matches, their scores and their order bit for bit; the matcher alone (cs_merge_match_from_pairs_dev) against the
sequential greedy on lists it cannot sort in LDS, in every order."""
import numpy as np
import pytest

from tests import mergematch_dev as D
from tests import mergematch_ref as R

pytestmark = pytest.mark.gpu
WS, HS = 192, 144


def _check_job(mm, k, slot, ref, check_pairs=True):
    cnt = mm.counts(k + 1)[k]
    m, s = mm.matches(k, cnt[0])
    rm, rs = D.as_arrays(ref["matches"])
    assert cnt[1] == 0 and cnt[0] == len(rm) and cnt[2] == len(ref["cands"])
    assert np.array_equal(m, rm)
    assert np.array_equal(s.view(np.int64), rs.view(np.int64))
    if check_pairs:
        total, rec = mm.pairs(slot)
        assert total == len(ref["cands"])
        got = sorted((int(r["i"]), int(r["j"]), float(r["epi"]).hex(), float(r["ncc"]).hex()) for r in rec)
        assert got == sorted((c[0], c[1], c[2].hex(), c[3].hex()) for c in ref["cands"])


@pytest.mark.parametrize("N,n_cams,pair", [(70, 2, (0, 1)), (70, 16, (14, 15)), (2100, 2, (1, 0))])
def test_run_equals_the_restatement(hip, N, n_cams, pair):
    """N = 70: no multiple of 32; N = 2100: tables are not sized for 2048; cameras 14 / 15 of a 16-camera rig"""
    import coslam_amd

    cams, job, _inv = R.shifted_pair_scene(N=N, n_cams=n_cams, pair=pair, seed=N + n_cams)
    ref = R.match_job(cams, WS, HS, job)
    assert len(ref["matches"]) > 20
    mm = coslam_amd.MergeMatcher(n_cams, N, 1, 64, 1 << 18, N)
    dc, keep = D.upload_cams(cams)
    mm.run(dc, WS, HS, [job])
    assert np.array_equal(coslam_amd.merge_match_fmat(cams[pair[0]]["K"], cams[pair[1]]["K"], job["E"]).view(np.int64), ref["F"].view(np.int64))
    blocks, abc, valid = mm.blocks()
    for side, c in enumerate(pair):
        live = ref["valid"][side] == 1
        assert np.array_equal(valid[c], ref["valid"][side])
        assert np.array_equal(blocks[c][live][:, :121], ref["blocks"][side][live][:, :121])
        assert np.array_equal(abc[c][live].view(np.int64), ref["abc"][side][live].view(np.int64))
    _check_job(mm, 0, 0, ref)
    mm.close()


@pytest.mark.parametrize("max_jobs,n_jobs", [(2, 5), (9, 9)])
def test_batches_and_more_than_one_candidate_launch(hip, max_jobs, n_jobs):
    """maxJobs = 2 with 5 jobs: three batches; 9 jobs: two launches of the candidate kernel (8 + 1)"""
    import coslam_amd

    N = 70
    cams, job, _ = R.shifted_pair_scene(N=N, n_cams=4, seed=5)
    order = [(0, 1), (1, 0), (0, 2), (2, 3), (1, 3), (0, 1), (3, 0), (2, 1), (1, 0)][:n_jobs]
    jobs = []
    for q, (a, b) in enumerate(order):
        E = job["E"] if (a, b) != (1, 0) else np.asarray(job["E"]).reshape(3, 3).T.reshape(9)
        sd = job["seeds"] if (a, b) == (0, 1) else (job["seeds"][:, [2, 3, 0, 1]] if (a, b) == (1, 0) else np.zeros((0, 4)))
        jobs.append(dict(iCam=a, jCam=b, E=E, seeds=sd[:len(sd) - (q % 2)]))
    refs = [R.match_job(cams, WS, HS, j) for j in jobs]
    assert len(refs[0]["matches"]) > 20 and len(refs[1]["matches"]) > 20
    mm = coslam_amd.MergeMatcher(4, N, max_jobs, 16, 4096, N)
    dc, keep = D.upload_cams(cams)
    mm.run(dc, WS, HS, jobs)
    last = (n_jobs - 1) // max_jobs * max_jobs
    for k, ref in enumerate(refs):
        _check_job(mm, k, k - last, ref, check_pairs=k >= last)
    mm.close()


def _random_list(rng, N, n, levels):
    ij = rng.choice(N * N, n, replace=False)
    return [(int(q // N), int(q % N), float(rng.integers(0, levels)) / levels) for q in ij]


def test_order_independence(hip):
    """~5000 candidates (several passes of the 1024-lane workgroup), scores from 40 levels (ties everywhere), in 4 orders: one result"""
    import coslam_amd

    rng = np.random.default_rng(1)
    N = 300
    cands = _random_list(rng, N, 5000, 40)
    want = D.as_arrays(R.greedy(cands))
    xy = np.zeros((2, N))
    mm = coslam_amd.MergeMatcher(1, N, 4, 0, 6000, N)
    lists = [cands, cands[::-1], [cands[q] for q in rng.permutation(len(cands))], sorted(cands, key=lambda c: (c[1], c[0]))]
    for m, s, cnt in D.from_pairs(mm, lists, xy, xy):
        assert cnt[1] == 0 and cnt[2] == 5000
        assert np.array_equal(m, want[0]) and np.array_equal(s, want[1])
    mm.close()


def test_planted_ties_in_rows_and_columns(hip):
    """bit-equal scores competing for a row (the smaller column wins) and for a column (the smaller row wins), and a pair listed twice"""
    import coslam_amd

    N = 70
    cands = [(5, 9, 0.9), (5, 3, 0.9), (5, 69, 0.9),          # row 5: column 3
             (8, 40, 0.8), (2, 40, 0.8), (69, 40, 0.8),       # column 40: row 2
             (2, 41, 0.8),                                    # loses row 2 to (2, 40)
             (11, 12, 0.7), (11, 12, 0.7),                    # listed twice
             (0, 0, -0.25), (1, 0, -0.25), (0, 1, -0.25), (33, 34, 0.0), (34, 33, -0.0)]
    want = D.as_arrays(R.greedy(cands))
    assert [tuple(r) for r in want[0][:3]] == [(5, 3), (2, 40), (11, 12)]
    xy = np.zeros((2, N))
    mm = coslam_amd.MergeMatcher(1, N, 2, 0, 64, N)
    for m, s, cnt in D.from_pairs(mm, [cands, cands[::-1]], xy, xy):
        assert np.array_equal(m, want[0]) and np.array_equal(s, want[1] + 0.0)
    mm.close()


def test_staircase_needs_one_round_per_match(hip):
    """d_k = (k, k) becomes dominant only when d_(k-1) has taken column k - 1 from o_(k-1) = (k, k - 1): 300 matches in 300 rounds, so
    the round bound must not cut a legal run short"""
    import coslam_amd

    n, N = 300, 301
    cands = []
    for k in range(n):
        cands += [(k, k, 1000.0 - 2 * k), (k + 1, k, 1000.0 - 2 * k - 1)]
    want = D.as_arrays(R.greedy(cands))
    assert len(want[0]) == n and all(a == b for a, b in want[0])
    xy = np.zeros((2, N))
    mm = coslam_amd.MergeMatcher(1, N, 1, 0, 1024, N)
    (m, s, cnt), = D.from_pairs(mm, [cands[::-1]], xy, xy)
    assert np.array_equal(m, want[0]) and np.array_equal(s, want[1])
    assert cnt[3] == n
    mm.close()


@pytest.mark.parametrize("n_seeds", [0, 1, 1100])
def test_seed_guide(hip, n_seeds):
    """no seeds (greedyNCCMatch), one seed, more seeds than the workgroup has lanes; equidistant seeds (the first wins); a candidate
    exactly at maxDisp stays, the next binary64 above goes"""
    import coslam_amd

    rng = np.random.default_rng(7 + n_seeds)
    N = 70
    xy1, xy2 = rng.uniform(0, 640, (2, N)), rng.uniform(0, 640, (2, N))
    seeds = np.zeros((n_seeds, 4))
    if n_seeds:
        seeds[:, :2] = rng.uniform(0, 640, (n_seeds, 2))
        seeds[:, 2:] = seeds[:, :2] + rng.uniform(-30, 30, (n_seeds, 2))
    if n_seeds > 1:
        xy1[:, 0] = (100.0, 100.0)
        seeds[3], seeds[9] = (90.0, 100.0, 95.0, 100.0), (110.0, 100.0, 300.0, 300.0)      # equidistant from slot 0: seed 3 wins
        seeds[[k for k in range(n_seeds) if k not in (3, 9)], :2] += 2000.0
        xy2[:, 1] = (100.0 + 5.0 + 150.0, 100.0)                                           # disparity exactly 150 under seed 3
        xy2[:, 2] = (np.nextafter(255.0, 1e9), 100.0)
    cands = _random_list(rng, N, 1500, 25) + [(0, 1, 2.0), (0, 2, 3.0)]
    cands = list({(c[0], c[1]): c for c in cands}.values())
    kept = R.guide(cands, xy1, xy2, seeds, 150.0)
    if n_seeds > 1:
        assert (0, 1, 2.0) in kept and (0, 2, 3.0) not in kept
    if n_seeds:
        assert 0 < len(kept) < len(cands)
    want = D.as_arrays(R.greedy(kept))
    mm = coslam_amd.MergeMatcher(1, N, 1, 1100, 2048, N)
    (m, s, cnt), = D.from_pairs(mm, [cands], xy1, xy2, [seeds], 150.0)
    assert np.array_equal(m, want[0]) and np.array_equal(s, want[1])
    mm.close()


def test_overflows_set_their_flags_and_select_skips_them(hip):
    import coslam_amd

    rng = np.random.default_rng(3)
    N = 70
    cands = _random_list(rng, N, 900, 1000)
    full = D.as_arrays(R.greedy(cands))
    xy = np.zeros((2, N))
    mm = coslam_amd.MergeMatcher(1, N, 2, 0, 900, 25)
    # job 0: more matches than maxMatches -- the kept head is the greedy's head; job 1: the count says more passed than pairCap holds
    (m0, s0, c0), (m1, s1, c1) = D.from_pairs(mm, [cands, cands], xy, xy, counts=[900, 1200])
    assert len(full[0]) > 25
    assert c0[0] == 25 and c0[1] == 2 and np.array_equal(m0, full[0][:25]) and np.array_equal(s0, full[1][:25])
    assert c1[1] == 3 and c1[2] == 1200 and np.array_equal(m1, full[0][:25])
    mm.close()
    infos = [(5, 0, 0, 5, 2, 1), (5, 1, 0, 5, 2, 1)]
    free = coslam_amd.merge_match_select(infos, [30, 30], [1, 1], [60, 40], [2, 1])
    flagged = coslam_amd.merge_match_select(infos, [30, 30], [1, 1], [60, 40], [2, 1], eligible=[0, 1])
    assert (free["entry"], flagged["entry"]) == (0, 1)
    assert flagged == R.select(infos, [30, 30], [1, 1], [60, 40], [2, 1] + [0] * 14, [0, 1])


def test_refusals_come_before_any_launch(hip):
    import coslam_amd
    from coslam_amd._lib import CoslamHipError

    with pytest.raises(CoslamHipError):
        coslam_amd.MergeMatcher(2, 32769, 1, 4, 64, 8)          # N above the cap
    with pytest.raises(CoslamHipError):
        coslam_amd.MergeMatcher(17, 64, 1, 4, 64, 8)
    cams, job, _ = R.shifted_pair_scene(N=70)
    mm = coslam_amd.MergeMatcher(2, 70, 1, 4, 4096, 70)
    dc, keep = D.upload_cams(cams)
    before = mm.counts(1).copy()
    with pytest.raises(CoslamHipError):
        mm.run(dc, WS, HS, [dict(job, jCam=2)])                 # camera outside the rig
    with pytest.raises(CoslamHipError):
        mm.run(dc, WS, HS, [dict(job, seeds=np.zeros((5, 4)))])  # more than maxSeeds
    with pytest.raises(CoslamHipError):
        mm.run([dict(dc[0], xy=0), dc[1]], WS, HS, [job])        # null table
    with pytest.raises(CoslamHipError):
        mm.from_pairs([0], [0], [0], [0])
    assert np.array_equal(mm.counts(1), before)
    mm.close()


def test_small_image_is_the_truncated_size_resize(hip):
    """cs_ncc_small_image_dev = cv::resize(img, Size((int)(W s), (int)(H s))) against the oracle's resize at fx = Ws / W, fy = Hs / H;
    641 x 483 at 0.3: (int)(192.3) x (int)(144.9) = 192 x 144 where the Size(), s, s form rounds to 192 x 145"""
    import torch

    import coslam_amd
    import oracle

    rng = np.random.default_rng(2)
    W, H, s = 641, 483, 0.3
    img = R.textured_image(W, H, rng)
    d_img = torch.as_tensor(img, device="cuda")
    d_small = torch.zeros(144 * 192, dtype=torch.uint8, device="cuda")
    ws, hs = coslam_amd.ncc_small_image_dev(torch.cuda.current_stream().cuda_stream, d_img.data_ptr(), W, H, s, d_small.data_ptr())
    assert (ws, hs) == (192, 144)
    want = oracle.resize_linear_u8(img, ws / W, hs / H)
    assert want.shape == (144, 192)
    assert np.array_equal(d_small.cpu().numpy().reshape(144, 192), want)


def test_golden_scenes_equal_the_reference(hip):
    """cs_merge_match_run_dev on every scene of tests/golden/mergematch_golden.npz: matches, scores and order against the reference's OWN
    matchFeaturePointsNCC bit for bit, F likewise; blocks, abc and the candidate set against the restatement.  The scenes hold a candidate
    exactly at epiMax, at maxDisp and at nccMin, equidistant seeds, bit-equal scores competing for a row and for a column, features at
    the small image's border and dead slots between live ones (the generator asserts each)."""
    import coslam_amd
    from tests import mergematch_scenes as MS
    from tests.mergematch_golden_util import load

    for S, G in load():
        jobs = MS.jobs_of(S)
        mm = coslam_amd.MergeMatcher(S["nC"], S["N"], 8, 64, 1 << 14, S["N"])
        dc, keep = D.upload_cams(S["cams"])
        mm.run(dc, S["Ws"], S["Hs"], [j for _, j in jobs], *S["par"])
        cnt = mm.counts(len(jobs))
        blocks, abc, valid = mm.blocks()
        for k, (e, job) in enumerate(jobs):
            m, s = mm.matches(k, cnt[k][0])
            assert cnt[k][1] == 0 and np.array_equal(m, G["matches"][e]) and s.tobytes() == G["scores"][e].tobytes(), (e, k)
            ref = R.match_job(S["cams"], S["Ws"], S["Hs"], job, *S["par"])
            total, rec = mm.pairs(k)
            assert total == len(ref["cands"])
            assert sorted((int(r["i"]), int(r["j"]), float(r["epi"]).hex(), float(r["ncc"]).hex()) for r in rec) == \
                sorted((c[0], c[1], c[2].hex(), c[3].hex()) for c in ref["cands"])
            for side, c in enumerate((job["iCam"], job["jCam"])):
                live = ref["valid"][side] == 1
                assert np.array_equal(valid[c], ref["valid"][side]) and np.array_equal(blocks[c][live][:, :121], ref["blocks"][side][live][:, :121])
                assert abc[c][live].tobytes() == ref["abc"][side][live].tobytes()
            q = S["entries"][e]
            assert coslam_amd.merge_match_fmat(S["cams"][q["iCam"]]["K"], S["cams"][q["jCam"]]["K"], q["E"]).tobytes() == G["F"][e].tobytes()
        mm.close()


def test_per_camera_img_scale_and_positions_that_are_no_pixel(hip):
    """KeyPose::imgScale is per camera: camera 1's small image is read at 0.25 of positions twice as large (one cutter launch per distinct
    scale).  A LIVE slot whose position is NaN or beyond 1e6 pixels takes no part: the result is that of the same scene with the slot dead."""
    import coslam_amd

    N = 70
    cams, job, _ = R.shifted_pair_scene(N=N, seed=33)
    cams[1]["xy"] = cams[1]["xy"] * (cams[1]["imgScale"] / 0.25)
    cams[1]["imgScale"] = 0.25
    job = dict(job, seeds=np.zeros((0, 4)))
    live = [s for s in range(N) if cams[0]["state"][s] in (0, 1)]
    bad = live[3], live[10]
    dev_cams = [dict(c, xy=c["xy"].copy()) for c in cams]
    dev_cams[0]["xy"][0, bad[0]], dev_cams[0]["xy"][1, bad[1]] = np.nan, 1.0e9
    ref_cams = [dict(c, state=c["state"].copy()) for c in cams]
    ref_cams[0]["state"][list(bad)] = -1
    ref = R.match_job(ref_cams, WS, HS, job, 1.0e9, 0.45, 150.0)
    assert len(ref["matches"]) > 20
    mm = coslam_amd.MergeMatcher(2, N, 1, 4, 1 << 14, N)
    dc, keep = D.upload_cams(dev_cams)
    mm.run(dc, WS, HS, [job], 1.0e9, 0.45, 150.0)
    blocks, abc, valid = mm.blocks()
    assert valid[0][bad[0]] == 0 and valid[0][bad[1]] == 0 and np.array_equal(valid[0], ref["valid"][0])
    lv = ref["valid"][1] == 1
    assert np.array_equal(blocks[1][lv][:, :121], ref["blocks"][1][lv][:, :121])
    _check_job(mm, 0, 0, ref)
    mm.close()
