"""Planted scenes of the merge front and the COVER CONDITIONS the GPU tests lean on, asserted on the numpy restatement
(tests/mergefront_ref.py) alone: whoever builds a scene through this module gets the restatement's answer only when the scene is one on
which the device's answer must equal it exactly.  640 x 480 images, f = 500, a non-planar cloud, descriptors = unit vectors + noise, gross
outliers at least 10 px from their true epipolar line."""
import functools

import numpy as np

from tests import mergefront_ref as ref

W, H, FOCAL = 640, 480, 500.0
K = np.array([FOCAL, 0, W / 2.0, 0, FOCAL, H / 2.0, 0, 0, 1.0])
EIG_GAP = 1.0e-6      # test 4: hypotheses whose A^T A has (second-smallest / largest eigenvalue) >= EIG_GAP are compared
E_TOL = 2.5e-9        # ... within this (100 x the largest Jacobi-against-eigh difference measured at that gap: see gap_study)
MARGIN_REL = 1.0e-3   # test 1: no matchSurf decision of the restatement within this (relative) of ratio d2 or maxDist
# the RANSAC cases of tests 3 - 6: (nTrue, nOut, noise, scene seed, nRansac, generator seed), chosen so that the cover conditions hold
CLEAN = [(80, 47, 0.0, 0, 200, 1), (12, 7, 0.0, 0, 200, 1)]
NOISY = [(80, 47, 0.3, 0, 200, 1), (80, 30, 0.3, 1, 200, 3)]
THRESH_BAND = 0.05    # test 6: no match within this many px of maxEpiErr under the winner's or any refit round's E


def unit_rows(rng, n, dim):
    v = rng.normal(0, 1, (n, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ---- the descriptor stage ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def descriptor_scene(n1, n2, dim, seed=0, ratio=0.8, max_dist=0.6):
    """-> (cam1, cam2, expected): cams dict(pts [n][2], desc [n][dim] f32, K); expected = ref.match_surf's dict.  About 60 % of the smaller
    camera's points have a partner (descriptor + noise of a spread of sizes, so that both tests decide both ways); planted where the sizes
    allow: rows with IDENTICAL descriptors (several i onto one j with bit-equal distances), two rows at different distances onto one j, a
    partner pair split by a near twin in camera 2 (the ratio test fails), a NaN descriptor on either side, a dead key point on either side."""
    last = None
    for attempt in range(64):                          # the first sub-seed whose scene meets the cover conditions
        try:
            return _descriptor_scene(n1, n2, dim, 1000 * seed + attempt, ratio, max_dist)
        except AssertionError as e:
            last = e
    raise AssertionError(f"no descriptor scene {n1} x {n2} x {dim} meets the cover conditions: {last}")


def _descriptor_scene(n1, n2, dim, rng_seed, ratio, max_dist):
    rng = np.random.default_rng(100000 * rng_seed + 7 * n1 + 3 * n2 + dim)
    d1, d2 = unit_rows(rng, n1, dim), unit_rows(rng, n2, dim)
    p1 = np.stack([rng.uniform(0, W, n1), rng.uniform(0, H, n1)], axis=1)
    p2 = np.stack([rng.uniform(0, W, n2), rng.uniform(0, H, n2)], axis=1)
    m = min(n1, n2)
    if m >= 1:
        nc = max(1, int(0.6 * m))
        ia, ja = rng.permutation(n1)[:nc], rng.permutation(n2)[:nc]
        sig = rng.choice([0.005, 0.02, 0.05, 0.085], nc) / np.sqrt(dim / 64.0)    # |noise| ~ sig sqrt(dim): 0.04 .. 0.7 around maxDist
        sig[:9] = 0.005 / np.sqrt(dim / 64.0)
        d2[ja] = d1[ia] + (rng.normal(0, 1, (nc, dim)) * sig[:, None]).astype(np.float32)
        if m >= 40:
            d1[ia[1]] = d1[ia[0]]                                 # two rows, one descriptor: bit-equal distances onto ja[0]
            d1[ia[3]] = d1[ia[2]] + np.float32(0.05) * unit_rows(rng, 1, dim)[0]   # two rows onto ja[2] at different distances
            free = [j for j in range(n2) if j not in set(ja)]
            d2[free[0]] = d2[ja[4]] + np.float32(0.002) * unit_rows(rng, 1, dim)[0]   # a near twin: the ratio test fails for ia[4]
            d1[ia[5], 3] = np.nan
            d2[ja[6], dim - 1] = np.inf
            p1[ia[7]] = [np.nan, 10.0]
            p2[ja[8]] = [5.0, 2.0e6]
    cam1, cam2 = dict(pts=p1, desc=d1, K=K.copy()), dict(pts=p2, desc=d2, K=K.copy())
    exp = ref.match_surf(p1, d1, p2, d2, ratio, max_dist)
    assert_descriptor_cover(exp, ratio, max_dist, d1)
    if m >= 40:                                        # the planted cases decide as planted
        acc, j1 = exp["accept"], exp["j1"]
        assert acc[ia[0]] and acc[ia[1]] and j1[ia[0]] == j1[ia[1]] == ja[0] and exp["d1"][ia[0]] == exp["d1"][ia[1]]
        assert acc[ia[2]] and acc[ia[3]] and j1[ia[2]] == j1[ia[3]] == ja[2]
        assert not acc[ia[4]] and not acc[ia[5]] and not acc[ia[7]] and j1[ia[6]] != ja[6] and j1[ia[8]] != ja[8]
    return cam1, cam2, exp


def assert_descriptor_cover(exp, ratio, max_dist, desc1):
    """no decision within MARGIN_REL of its threshold; rows that compete for one column differ by more than that or are the same descriptor"""
    d1, d2, j1 = exp["d1"].astype(np.float64), exp["d2"].astype(np.float64), exp["j1"]
    for i in range(len(d1)):
        if j1[i] < 0:
            continue
        assert abs(d1[i] - max_dist) > MARGIN_REL * max_dist, (i, d1[i])
        if np.isfinite(d2[i]) and d1[i] < max_dist:
            assert abs(d1[i] - ratio * d2[i]) > MARGIN_REL * ratio * d2[i], (i, d1[i], d2[i])
        if np.isfinite(d2[i]) and exp["accept"][i]:
            assert d2[i] - d1[i] > MARGIN_REL * d2[i], (i, d1[i], d2[i])     # (which j is nearest is beyond doubt)
    rows = np.nonzero(exp["accept"])[0]
    for a in rows:
        for b in rows:
            if a < b and j1[a] == j1[b]:
                same = np.array_equal(desc1[a].view(np.uint32), desc1[b].view(np.uint32))
                assert same or abs(d1[a] - d1[b]) > MARGIN_REL * max(d1[a], d1[b]), (a, b)


# ---- two views ------------------------------------------------------------------------------------------------------------------------
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


@functools.lru_cache(maxsize=None)
def two_view_scene(n_true, n_out, noise, seed=0, dim=64, extra=5):
    """-> dict(cam1, cam2 [pts, desc, K], matches [n][2] in ascending i, truth [n] bool, E_true [9], F_true).  x2 = R x1 + t.  The true
    pairs and the gross outliers both carry partner descriptors (the descriptor stage returns exactly `matches`); `extra` points per camera
    have no partner."""
    rng = np.random.default_rng(50000 + 131 * seed + 7 * n_true + n_out)
    R, t = _rot(0.03, -0.17, 0.05), np.array([1.0, 0.12, 0.25])
    Km = K.reshape(3, 3)
    Et = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    iK = np.linalg.inv(Km)
    Ft = iK.T @ Et @ iK
    a, b = [], []
    while len(a) < n_true:
        X = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(4, 10)])
        u1, u2 = Km @ X, Km @ (R @ X + t)
        u1, u2 = u1[:2] / u1[2], u2[:2] / u2[2]
        if 5 < u1[0] < W - 5 and 5 < u1[1] < H - 5 and 5 < u2[0] < W - 5 and 5 < u2[1] < H - 5:
            a.append(u1 + rng.normal(0, noise, 2) if noise else u1), b.append(u2 + rng.normal(0, noise, 2) if noise else u2)
    while len(a) < n_true + n_out:
        u1, u2 = rng.uniform([5, 5], [W - 5, H - 5]), rng.uniform([5, 5], [W - 5, H - 5])
        if ref.epi_err(Ft, np.concatenate([u1, u2])[None])[0] >= 10.0 and ref.epi_err(Ft.T, np.concatenate([u2, u1])[None])[0] >= 10.0:
            a.append(u1), b.append(u2)
    n = n_true + n_out
    truth = np.arange(n) < n_true
    o1, o2 = rng.permutation(n + extra), rng.permutation(n + extra)        # where pair q sits in camera 1 / 2
    p1 = np.stack([rng.uniform(5, W - 5, n + extra), rng.uniform(5, H - 5, n + extra)], axis=1)
    p2 = np.stack([rng.uniform(5, W - 5, n + extra), rng.uniform(5, H - 5, n + extra)], axis=1)
    d1, d2 = unit_rows(rng, n + extra, dim), unit_rows(rng, n + extra, dim)
    for q in range(n):
        p1[o1[q]], p2[o2[q]] = a[q], b[q]
        d2[o2[q]] = d1[o1[q]] + (rng.normal(0, 0.004, dim)).astype(np.float32)
    order = np.argsort(o1[:n])
    matches = np.stack([o1[:n][order], o2[:n][order]], axis=1).astype(np.int32)
    return dict(cam1=dict(pts=p1, desc=d1, K=K.copy()), cam2=dict(pts=p2, desc=d2, K=K.copy()), matches=matches, truth=truth[order],
                E_true=Et.reshape(9) / np.linalg.norm(Et), F_true=Ft)


@functools.lru_cache(maxsize=None)
def ransac_case(n_true, n_out, noise, seed, n_ransac, gen_seed, k=0, max_epi_err=2.0, min_inlier_num=15):
    """a two-view scene with the restatement's estimateEMat of job k and the cover conditions of tests 5 / 6 asserted -> (scene, expected)"""
    sc = two_view_scene(n_true, n_out, noise, seed)
    exp = ref.estimate_emat(K, K, sc["cam1"]["pts"], sc["cam2"]["pts"], sc["matches"], n_ransac, max_epi_err, min_inlier_num, gen_seed, k)
    assert_ransac_cover(sc, exp, noise, max_epi_err)
    return sc, exp


def contaminated(sc, exp):
    """per hypothesis: does its sample hold a gross outlier"""
    return np.array([(s[0] >= 0) and (not sc["truth"][s].all()) for s in exp["hyp_sample"]])


def assert_ransac_cover(sc, exp, noise, max_epi_err):
    cnt = exp["hyp_count"].astype(np.int64)
    best = exp["best_hyp"]
    n_true = int(sc["truth"].sum())
    assert (exp["hyp_gap"][exp["hyp_sample"][:, 0] >= 0] >= EIG_GAP).mean() >= 0.9
    iK = np.linalg.inv(K.reshape(3, 3))
    if noise == 0:
        bad = contaminated(sc, exp)
        assert (~bad & (exp["hyp_sample"][:, 0] >= 0)).any(), "no all-inlier sample"
        assert cnt[bad].max(initial=0) <= n_true - 3
        assert cnt[best] == n_true and np.array_equal(exp["inlier"], sc["truth"])
        assert ref.epi_err(ref.fmat(iK, iK, exp["E"]), exp["pix"])[sc["truth"]].max() < 1e-9
        assert cnt[:best].max(initial=0) <= n_true - 3                     # (an all-inlier sample in front of the winner is degenerate)
    else:
        others = np.delete(cnt, best)
        assert len(others) == 0 or cnt[best] - others.max() >= 3, (cnt[best], others.max())
    for E in exp["round_E"]:
        e = ref.epi_err(ref.fmat(iK, iK, E), exp["pix"])
        assert not (np.abs(e - max_epi_err) < THRESH_BAND).any()


def gap_study(cases):
    """test 4's two numbers, measured on the CPU: the restatement's Jacobi against numpy.linalg.eigh on the same samples -> (fraction of the
    hypotheses with gap >= EIG_GAP, the largest difference of the two unit-norm, sign-aligned E among them)"""
    worst, frac = 0.0, []
    for sc, exp in cases:
        iK = np.linalg.inv(K.reshape(3, 3))
        pix = exp["pix"]
        nrm = np.concatenate([ref.normalise(iK, pix[:, :2]), ref.normalise(iK, pix[:, 2:])], axis=1)
        live = exp["hyp_sample"][:, 0] >= 0
        frac.append(float((exp["hyp_gap"][live] >= EIG_GAP).mean()))
        for h in np.nonzero(live & (exp["hyp_gap"] >= EIG_GAP))[0]:
            A, T1, T2, ok = ref.design_ata(nrm[exp["hyp_sample"][h]])
            w, v = np.linalg.eigh(A)
            E, ok2 = ref.project_essential((T2.T @ v[:, 0].reshape(3, 3) @ T1)[None])
            a, b = E[0].reshape(9), exp["hyp_E"][h]
            if not (ok and ok2[0]) or not b.any():
                continue
            worst = max(worst, float(np.abs(a * np.sign(a @ b) - b).max()))
    return min(frac), worst
