"""The merge front on the device against its numpy restatement (tests/mergefront_ref.py), layer by layer, on the planted scenes
of tests/mergefront_scenes.py -- whose cover conditions (asserted there, on the restatement alone) are what makes `equal exactly` a fair
demand: no matchSurf decision within 1e-3 of its threshold, a winner that leads by 3, no match within 0.05 px of maxEpiErr.

Test 4's two numbers, measured on the CPU (mergefront_scenes.gap_study: the restatement's cyclic Jacobi against numpy.linalg.eigh on the
samples of the four RANSAC cases below): at an eigenvalue gap (second-smallest / largest of A^T A) of g = 1e-6 at least 95.5 % of a scene's
hypotheses qualify and the largest difference of the two unit-norm E is 2.5e-11; the tolerance is 100 x that, 2.5e-9."""
import numpy as np
import pytest

import coslam_amd
from tests import mergefront_dev as D
from tests import mergefront_ref as R
from tests import mergefront_scenes as S

pytestmark = pytest.mark.gpu

CLEAN, NOISY = S.CLEAN, S.NOISY
IK = np.linalg.inv(S.K.reshape(3, 3))


# ---- 1. the descriptor stage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128])
def test_descriptor_stage_equals_the_restatement(hip, dim):
    shapes = [(1, 1), (2, 1), (63, 65), (65, 63), (700, 650)]
    mf = coslam_amd.MergeFront(16, 700, dim, 8, 1)
    for n1, n2 in shapes:
        c1, c2, exp = S.descriptor_scene(n1, n2, dim)
        cams = [D.filler(dim, S.K)] * 14 + [c1, c2]              # cameras 14 and 15 of 16
        dc, keep = D.upload_cams(cams)
        mf.match(dc, [(14, 15)])
        n = int(mf.counts(1)[0])
        m, d = mf.matches(0, n)
        assert n == len(exp["matches"]) and np.array_equal(m, exp["matches"]), (n1, n2)
        assert np.all(np.abs(d - exp["dist"]) <= 1e-5 * exp["dist"]), (n1, n2)      # 64 f32 ulps: the order of a 64 .. 128-term sum
    assert len(exp["matches"]) > 200
    mf.close()


# ---- 2. the samples -----------------------------------------------------------------------------------------------------------------
def test_samples_equal_the_generator_bit_for_bit(hip):
    sc = S.two_view_scene(100, 40, 0.3, 3)
    dc, keep = D.upload_cams([sc["cam1"], sc["cam2"]])
    mf = coslam_amd.MergeFront(2, 200, 64, 3, 257)
    for n in (8, 9, 25, 127):
        for nr in (1, 64, 200, 257):
            mf.from_matches(dc, [(0, 1), (1, 0), (0, 1)], [sc["matches"][:n], sc["matches"][:n, ::-1], sc["matches"][:n]], n_ransac=nr, seed=77)
            mf.results(3)
            for k in (0, 2):
                got = mf.hypotheses(k, nr)[0]
                want = np.array([R.sample8(77, k, h, n) or [-1] * 8 for h in range(nr)], np.int32)
                assert np.array_equal(got, want), (n, nr, k)
    mf.close()


# ---- 3 - 6: one device run per RANSAC case, shared -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(hip):
    out = {}
    for case in CLEAN + NOISY:
        nt, no, noise, seed, nr, gs = case
        sc, exp = S.ransac_case(nt, no, noise, seed, nr, gs)
        dc, keep = D.upload_cams([sc["cam1"], sc["cam2"]])
        mf = coslam_amd.MergeFront(2, 200, 64, 1, nr)
        res = mf.run(dc, [(0, 1)], n_ransac=nr, seed=gs)
        out[case] = (sc, exp, D.layers(mf, 0, 0, nr, res[0]))
        mf.close()
    return out


def test_scoring_counts_what_its_own_E_says(runs):
    """hypCount[h] against evaluateEMat on the CPU from the device's OWN hypE[h]"""
    total = left = 0
    for sc, exp, got in runs.values():
        assert np.array_equal(got["pix"], exp["pix"])
        for h in range(len(got["hyp_E"])):
            total += 1
            if not got["hyp_E"][h].any():
                assert got["hyp_count"][h] == 0
                continue
            e = R.epi_err(R.fmat(IK, IK, got["hyp_E"][h]), got["pix"])
            if (np.abs(e - 2.0) < 1e-9).any():
                left += 1
                continue
            assert got["hyp_count"][h] == int((e < 2.0).sum()), h
    assert left <= 0.01 * total


def test_minimal_solve_equals_the_restatement(runs):
    """g = 1e-6, tolerance 2.5e-9 (the module docstring says where both come from); every hypE on the essential manifold"""
    for sc, exp, got in runs.values():
        assert np.array_equal(got["hyp_sample"], exp["hyp_sample"])
        live = np.nonzero((exp["hyp_sample"][:, 0] >= 0) & (exp["hyp_gap"] >= S.EIG_GAP))[0]
        assert len(live) >= 0.9 * len(exp["hyp_E"])
        for h in live:
            a, b = got["hyp_E"][h], exp["hyp_E"][h]
            assert np.abs(a * np.sign(a @ b) - b).max() <= S.E_TOL, h
        for h in range(len(got["hyp_E"])):
            if got["hyp_E"][h].any():
                sv = np.linalg.svd(got["hyp_E"][h].reshape(3, 3), compute_uv=False)
                assert np.abs(sv - np.array([1, 1, 0]) / np.sqrt(2)).max() <= 1e-12, h


@pytest.mark.parametrize("case", CLEAN)
def test_whole_ransac_on_noise_free_scenes(runs, case):
    sc, exp, got = runs[case]
    assert got["best_hyp"] == exp["best_hyp"] and got["surf_num"] == len(sc["matches"]) and np.array_equal(got["matches"], sc["matches"])
    assert np.array_equal(got["inlier"], exp["inlier"]) and np.array_equal(got["inlier"], sc["truth"])
    assert got["inlier_num"] == int(sc["truth"].sum()) and got["flags"] == 0 and got["emat_ok"] == exp["emat_ok"]
    e = R.epi_err(R.fmat(IK, IK, got["E"]), got["pix"])
    assert e[sc["truth"]].max() < 1e-6


@pytest.mark.parametrize("case", NOISY)
def test_whole_ransac_on_noisy_scenes(runs, case):
    sc, exp, got = runs[case]
    assert got["best_hyp"] == exp["best_hyp"] and got["rounds"] == exp["rounds"] and got["inlier_num"] == exp["inlier_num"]
    assert np.array_equal(got["inlier"], exp["inlier"]) and got["emat_ok"] == exp["emat_ok"] == 1 and got["flags"] == 0
    assert got["seeds"].tobytes() == np.ascontiguousarray(exp["seeds"]).tobytes() and np.array_equal(got["new_matches"], exp["new_matches"])
    assert np.abs(got["E"] * np.sign(got["E"] @ exp["E"]) - exp["E"]).max() <= S.E_TOL
    assert abs(got["epi_err"] - exp["epi_err"]) <= 1e-6


# ---- 7. edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges_too_few_matches_the_inlier_threshold_batches_and_repeatability(hip):
    sc, exp = S.ransac_case(*NOISY[0][:4], NOISY[0][4], NOISY[0][5])
    dc, keep = D.upload_cams([sc["cam1"], sc["cam2"]])
    mf = coslam_amd.MergeFront(2, 200, 64, 2, 200)
    # n = 7
    mf.from_matches(dc, [(0, 1)], [sc["matches"][:7]], n_ransac=200, seed=1)
    r = mf.results(1)[0]
    assert (r["surf_num"], r["emat_ok"], r["inlier_num"], r["flags"], r["best_hyp"]) == (7, 0, 0, coslam_amd.merge.MERGE_FRONT_TOO_FEW, -1)
    assert (mf.hypotheses(0, 200)[0] == -1).all() and not r["E"].any()
    # inlierNum at minInlierNum and one below it
    n_in = exp["inlier_num"]
    for mn, ok in ((n_in, 1), (n_in + 1, 0)):
        mf.from_matches(dc, [(0, 1)], [sc["matches"]], n_ransac=200, min_inlier_num=mn, seed=NOISY[0][5])
        r = mf.results(1)[0]
        assert r["inlier_num"] == n_in and r["emat_ok"] == ok
    # 5 jobs through maxJobs = 2: job k's answer does not depend on the batching (k seeds the generator, the outputs are every job's)
    pairs = [(0, 1), (1, 0), (0, 1), (0, 1), (1, 0)]
    res = mf.run(dc, pairs, n_ransac=200, seed=5)
    big = coslam_amd.MergeFront(2, 200, 64, 8, 200)
    res2 = big.run(dc, pairs, n_ransac=200, seed=5)
    for k in range(5):
        assert res[k]["surf_num"] == len(sc["matches"]) and res[k]["inlier_num"] >= 8
        for key in ("E", "seeds"):
            assert res[k][key].tobytes() == res2[k][key].tobytes(), (k, key)
        assert {q: res[k][q] for q in ("surf_num", "emat_ok", "inlier_num", "rounds", "best_hyp", "flags", "epi_err")} == \
            {q: res2[k][q] for q in ("surf_num", "emat_ok", "inlier_num", "rounds", "best_hyp", "flags", "epi_err")}
    # two runs are byte-equal, layer by layer
    a = D.layers(big, 4, 4, 200, big.run(dc, pairs, n_ransac=200, seed=5)[4])
    b = D.layers(big, 4, 4, 200, big.run(dc, pairs, n_ransac=200, seed=5)[4])
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    big.close(), mf.close()


def test_refusals_before_any_launch(hip):
    sc = S.two_view_scene(80, 47, 0.3, 0)
    dc, keep = D.upload_cams([sc["cam1"], sc["cam2"]])
    mf = coslam_amd.MergeFront(2, 200, 64, 2, 50)
    bad = [dict(pairs=[(0, 2)]), dict(pairs=[(-1, 1)]), dict(pairs=[(1, 1)]), dict(pairs=[(0, 1)], n_ransac=51), dict(pairs=[(0, 1)], n_ransac=0),
           dict(pairs=[(0, 1)] * 257)]
    for kw in bad:
        with pytest.raises(coslam_amd.CoslamHipError):
            mf.enqueue(dc, kw["pairs"], n_ransac=kw.get("n_ransac", 50))
    with pytest.raises(coslam_amd.CoslamHipError, match="points"):
        mf.enqueue([dict(dc[0], n=201), dc[1]], [(0, 1)], n_ransac=50)
    with pytest.raises(coslam_amd.CoslamHipError, match="singular"):
        mf.enqueue([dict(dc[0], K=np.zeros(9)), dc[1]], [(0, 1)], n_ransac=50)
    with pytest.raises(coslam_amd.CoslamHipError):
        mf.from_matches(dc, [(0, 1)] * 3, [sc["matches"]] * 3, n_ransac=50)          # more than maxJobs
    mf.close()
