"""CPU checks of the merge matcher: the host selection cs_merge_match_select and F against the plain restatement
tests/mergematch_ref.py, the exactness argument of the device's matcher executed (rounds of locally dominant candidates in numpy against
the sequential greedy on random lists with planted ties), and that the end-to-end scene cannot pass by matching nothing."""
import numpy as np

import coslam_amd
from tests import mergematch_ref as R


def test_fmat_is_the_restatement_bit_for_bit():
    rng = np.random.default_rng(0)
    for _ in range(20):
        K1 = np.array([500 + 30 * rng.random(), 0.3 * rng.random(), 320 + 5 * rng.normal(), 0, 505 + 30 * rng.random(), 240 + 5 * rng.normal(), 0, 0, 1])
        K2 = np.array([480 + 30 * rng.random(), 0, 300 + 5 * rng.normal(), 0, 470 + 30 * rng.random(), 250 + 5 * rng.normal(), 0, 0, 1])
        E = rng.normal(size=9)
        F = coslam_amd.merge_match_fmat(K1, K2, E)
        assert np.array_equal(F.view(np.int64), R.fmat(K1, K2, E).view(np.int64))
        want = np.linalg.inv(K1.reshape(3, 3)).T @ E.reshape(3, 3).T @ np.linalg.inv(K2.reshape(3, 3))
        assert np.allclose(F.reshape(3, 3), want, rtol=1e-10, atol=1e-14)


INFOS = [(7, 0, 0, 7, 4, 2), (7, 0, 0, 7, 2, 1), (7, 1, 0, 7, 2, 1), (7, 1, 0, 7, 3, 1), (7, 2, 1, 7, 4, 2)]   # group pairs (0,1) x 3, (0,2), (1,2)
SIZES = [2, 2, 1]


def _both(infos, surf, ok, ncc, sizes, eligible=None):
    got = coslam_amd.merge_match_select(infos, surf, ok, ncc, sizes, eligible)
    assert got == R.select(infos, surf, ok, ncc, list(sizes) + [0] * (16 - len(sizes)), eligible)
    return got


def test_select_restates_the_loop_with_its_quirks():
    # (0,1) comes first whatever the list order.  Its first entry fails SURF, so for the second i = 1 but k = 0: the threshold becomes
    # featMatches[1].num, still unfilled (0), and the third entry wins with FEWER matches than the second -- even with fewer than 20.
    got = _both(INFOS, [30, 10, 30, 30, 30], [1, 1, 1, 1, 0], [0, 99, 50, 12, 0], SIZES)
    assert (got["status"], got["entry"], got["maxk"], got["maxiCam"], got["maxjCam"], got["maxgId1"], got["maxgId2"]) == (1, 3, 1, 1, 3, 0, 1)
    # without the skipped entry i == k and the larger count keeps the pair
    got = _both(INFOS, [30, 30, 30, 30, 30], [1, 1, 1, 1, 0], [0, 50, 40, 12, 0], SIZES)
    assert got["entry"] == 1
    # nMinNCCMatchNum is reset per group pair and maxk survives: a later group pair with 21 matches takes over from one with 99
    got = _both(INFOS, [30, 30, 10, 10, 30], [1, 1, 1, 1, 1], [21, 99, 0, 0, 0], SIZES)
    assert (got["entry"], got["maxgId1"], got["maxgId2"], got["maxk"]) == (0, 0, 2, 1)
    # a failed computeEMat does not advance k; fewer than 25 SURF matches skip the entry
    got = _both(INFOS, [30, 24, 25, 30, 30], [1, 1, 0, 1, 1], [5, 77, 66, 30, 5], SIZES)
    assert (got["entry"], got["maxk"]) == (3, 0)
    # both orientations of m_gid1 / m_gid2: the larger group first; equal sizes take the else branch
    a = _both(INFOS[:1], [30], [1], [30], [2, 1, 1])
    b = _both(INFOS[:1], [30], [1], [30], [1, 1, 2])
    c = _both(INFOS[:1], [30], [1], [30], [2, 1, 2])
    assert (a["gid1"], a["gid2"], a["camid1"], a["camid2"]) == (0, 2, 0, 4)
    assert (b["gid1"], b["gid2"], b["camid1"], b["camid2"]) == (2, 0, 4, 0) and (c["gid1"], c["camid1"]) == (2, 4)
    # nothing matched / matched with no pair above the threshold (the reference's undefined run): a status and no pair
    assert _both(INFOS, [10] * 5, [1] * 5, [99] * 5, SIZES)["status"] == 0
    und = _both(INFOS, [30] * 5, [1] * 5, [20] * 5, SIZES)
    assert und["status"] == -1 and und["entry"] == -1 and und["gid1"] == -1
    # a flagged job is not eligible
    assert _both(INFOS[1:3], [30, 30], [1, 1], [60, 40], SIZES, [0, 1])["entry"] == 1
    assert _both([], [], [], [], SIZES)["status"] == 0


def test_select_equals_the_restatement_on_random_lists():
    rng = np.random.default_rng(4)
    for _ in range(300):
        n = int(rng.integers(1, 12))
        infos = []
        for _e in range(n):
            g1 = int(rng.integers(0, 3))
            g2 = int(rng.integers(g1 + 1, 4))
            infos.append((9, int(rng.integers(0, 8)), g1, 9, int(rng.integers(8, 16)), g2))
        _both(infos, rng.integers(20, 30, n), rng.integers(0, 2, n), rng.integers(15, 40, n), rng.integers(1, 5, 4),
              rng.integers(0, 2, n) if rng.random() < 0.5 else None)


def test_rounds_of_locally_dominant_candidates_equal_the_sequential_greedy():
    """the device's form, in numpy, on 200 random lists with planted ties (scores from a handful of levels, duplicates, a pair listed
    twice): the same matches in the same order"""
    rng = np.random.default_rng(9)
    most = 0
    for t in range(200):
        N = int(rng.integers(3, 60))
        n = int(rng.integers(1, min(N * N, 400)))
        ij = rng.choice(N * N, n, replace=False)
        levels = int(rng.integers(1, 12)) if t % 2 else 1000
        cands = [(int(q // N), int(q % N), float(rng.integers(-levels, levels + 1)) / levels) for q in ij]
        if t % 5 == 0:
            cands.append(cands[0])
        want = R.greedy(cands)
        got, rounds = R.rounds_match([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], N)
        assert got == want
        assert rounds <= max(len(want), 1)
        most = max(most, rounds)
    assert most > 1


def test_the_end_to_end_scene_has_more_matches_than_the_selection_threshold():
    """nMinNCCMatchNum = 20: below it no pair is ever chosen, so the end-to-end GPU test cannot pass by matching nothing"""
    from tests import mergematch_e2e as E2

    S, cams, entry, job = E2.build()
    ref = R.match_job(cams, E2.WS, E2.HS, job)
    true = set(map(tuple, np.asarray(S["matches"]).tolist()))
    got = set((a, b) for a, b, _ in ref["matches"])
    assert len(ref["matches"]) > 20 and len(true & got) > 20


# ---- the reference pin: tests/golden/mergematch_golden.npz holds what the reference's OWN functions gave (tests/cxx/ref_mergematch_test.cpp) ----
def test_restatement_equals_the_reference_on_every_golden_scene():
    """matches (pairs AND order), scores and F of every job, bit for bit"""
    from tests import mergematch_scenes as MS
    from tests.mergematch_golden_util import load

    n_jobs = 0
    for S, G in load():
        for e, q in enumerate(S["entries"]):
            F = R.fmat(S["cams"][q["iCam"]]["K"], S["cams"][q["jCam"]]["K"], q["E"])
            assert np.array_equal(F.view(np.int64), G["F"][e].view(np.int64)), e
            assert np.array_equal(coslam_amd.merge_match_fmat(S["cams"][q["iCam"]]["K"], S["cams"][q["jCam"]]["K"], q["E"]).view(np.int64),
                                  G["F"][e].view(np.int64))
        jobs = MS.jobs_of(S)
        assert [e for e, _ in jobs] == [e for e, r in enumerate(G["ran"]) if r]
        for e, job in jobs:
            ref = R.match_job(S["cams"], S["Ws"], S["Hs"], job, *S["par"])
            assert [[a, b] for a, b, _ in ref["matches"]] == G["matches"][e].tolist(), e
            assert np.array([s for _, _, s in ref["matches"]]).tobytes() == G["scores"][e].tobytes(), e
            n_jobs += 1
    assert n_jobs == 5


def test_select_equals_the_reference_on_every_golden_scene():
    """cs_merge_match_select and its restatement against matchMergableCameras' own run: the pair handed to genMergeInfoVer2, its matches,
    m_gid1 / m_gid2 / m_camid1 / m_camid2"""
    from tests.mergematch_golden_util import front, load

    winners = []
    for S, G in load():
        infos, surf, ok, ncc = front(S, G)
        sizes = [len(g) for g in S["groups"]]
        got = coslam_amd.merge_match_select(infos, surf, ok, ncc, sizes)
        assert got == R.select(infos, surf, ok, ncc, sizes + [0] * (16 - len(sizes)))
        num, called, g1, g2, ic, jc, mg1, mg2, mc1, mc2 = (int(v) for v in G["loop"])
        assert (num, called, got["status"]) == (1, 1, 1)
        assert (got["maxgId1"], got["maxgId2"], got["maxiCam"], got["maxjCam"]) == (g1, g2, ic, jc)
        assert (got["gid1"], got["gid2"], got["camid1"], got["camid2"]) == (mg1, mg2, mc1, mc2)
        if S["par"] == (20.0, 0.45, 150.0):      # (scene 2 runs the driver's own calls at another nccMin; the loop's are the reference's)
            assert np.array_equal(G["matches"][got["entry"]], G["rec_matches"])
        winners.append((got["entry"], ncc))
    e, ncc = winners[0]          # the quirk: the chosen entry has FEWER matches than another of its group pair
    assert ncc[e] < max(ncc) and ncc[e] > 20
