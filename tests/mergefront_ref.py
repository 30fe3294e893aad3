"""Plain numpy restatement of the merge front: matchSurf, estimateEMat and evaluateEMat as DESIGN 5.1 defines them
(un-vendored LibVisualSLAM: the definitions are this project's), behind matchSURFPoints / computeEMat / getMatchedPts of
matchMergableCameras (reference src/app/SL_MergeCameraGroup.cpp:360-378).  Written from the definitions, never calls the library.
TEST INFRASTRUCTURE: the eigen-solves run for all hypotheses of a job at once (numpy batches), everything else one item at a time."""
import numpy as np

from tests.mergematch_ref import inv33

DRAWS = 64          # draws a hypothesis may spend on its 8 distinct indices
SWEEPS9 = 10        # cyclic Jacobi on the 9 x 9: a fixed number of sweeps, rows p < q in order
SWEEPS3 = 10        # the one-sided 3 x 3 Jacobi
REFIT_ROUNDS = 4
TOO_FEW, NO_MODEL = 1, 2
M64 = (1 << 64) - 1


# ---- matchSurf ---------------------------------------------------------------------------------------------------------------------
def valid_points(pts, desc):
    """a point takes part iff its key point is finite and within 1e6 px and every component of its descriptor is finite"""
    pts, desc = np.asarray(pts, dtype=np.float64).reshape(-1, 2), np.asarray(desc, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (np.abs(pts) < 1.0e6).all(axis=1) & np.isfinite(desc).all(axis=1)


def match_surf(pts1, desc1, pts2, desc2, ratio=0.8, max_dist=0.6):
    """-> dict(matches int [count][2] in ascending i, dist f32 [count], d1 / d2 / j1 per row of camera 1 (f32; for the cover assertions),
    accept per row)"""
    d1_, d2_ = np.asarray(desc1, dtype=np.float32), np.asarray(desc2, dtype=np.float32)
    n1, n2 = len(d1_), len(d2_)
    v1, v2 = valid_points(pts1, d1_), valid_points(pts2, d2_)
    ratio, max_dist = np.float32(ratio), np.float32(max_dist)
    D1, D2, J1 = np.full(n1, np.inf, np.float32), np.full(n1, np.inf, np.float32), np.full(n1, -1)
    acc = np.zeros(n1, bool)
    for i in range(n1):
        if n2 == 0:
            break
        with np.errstate(invalid="ignore", over="ignore"):
            diff = d1_[i][None, :] - d2_
            d = np.sqrt(np.sum(diff * diff, axis=1, dtype=np.float32)).astype(np.float32)
        d[~v2] = np.inf
        d[np.isnan(d)] = np.inf
        j = int(np.argmin(d))                      # the lowest j of equals
        if not np.isfinite(d[j]):
            continue
        D1[i], J1[i] = d[j], j
        D2[i] = np.min(np.delete(d, j)) if n2 > 1 else np.inf
        acc[i] = bool(v1[i] and D1[i] < max_dist and D1[i] < np.float32(ratio * D2[i]))
    best = {}                                      # one-to-one: the integer minimum of {f32 bits of d1, i} per column
    for i in np.nonzero(acc)[0]:
        key = (int(np.float32(D1[i]).view(np.uint32)) << 32) | int(i)
        if J1[i] not in best or key < best[J1[i]]:
            best[J1[i]] = key
    keep = [i for i in np.nonzero(acc)[0] if best[J1[i]] & 0xFFFFFFFF == i]
    return dict(matches=np.array([[i, J1[i]] for i in keep], dtype=np.int32).reshape(-1, 2), dist=D1[keep].astype(np.float32),
                d1=D1, d2=D2, j1=J1, accept=acc)


# ---- the sample generator ----------------------------------------------------------------------------------------------------------
def rand_hi(seed, k, h, draw):
    """the upper 32 bits of a 64-bit mix of (seed, job k, hypothesis h, draw)"""
    c = (k << 40) | (h << 8) | draw
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


def sample8(seed, k, h, n):
    """8 distinct match indices, a repeated index redrawn with the next counter; None when the draws run out (or n < 8)"""
    got = []
    if n < 8:
        return None
    for draw in range(DRAWS):
        idx = (rand_hi(seed, k, h, draw) * n) >> 32
        if idx not in got:
            got.append(idx)
            if len(got) == 8:
                return got
    return None


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def normalise(iK, xy):
    """x^ = iK (x, y, 1), divided by its third component"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    iK = np.asarray(iK, dtype=np.float64).reshape(3, 3)
    h = xy @ iK[:, :2].T + iK[:, 2]
    return h[:, :2] / h[:, 2:3]


def fmat(iK1, iK2, E):
    """getFMat(iK1, iK2, E) = iK2^T E iK1"""
    return np.asarray(iK2, dtype=np.float64).reshape(3, 3).T @ np.asarray(E, dtype=np.float64).reshape(3, 3) @ np.asarray(iK1, dtype=np.float64).reshape(3, 3)


def epi_err(F, pix):
    """epipolarError(F, p2, p1) of every row {x1, y1, x2, y2}: the distance of p2 from the line F (p1, 1)"""
    pix = np.asarray(pix, dtype=np.float64).reshape(-1, 4)
    l = np.concatenate([pix[:, :2], np.ones((len(pix), 1))], axis=1) @ np.asarray(F, dtype=np.float64).reshape(3, 3).T
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(l[:, 0] * pix[:, 2] + l[:, 1] * pix[:, 3] + l[:, 2]) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2)


def evaluate_emat(F, pix, max_epi_err):
    """-> (flags, count, mean error of the inliers); a NaN error is no inlier"""
    e = epi_err(F, pix)
    with np.errstate(invalid="ignore"):
        fl = e < max_epi_err
    n = int(fl.sum())
    return fl, n, (float(e[fl].sum()) / n if n else 0.0)


def jacobi_eig(A, sweeps=SWEEPS9):
    """cyclic Jacobi on a batch of symmetric matrices [H][n][n]: rows p < q in order, `sweeps` sweeps, a rotation with a_pq == 0 skipped.
    -> (A rotated: the eigenvalues on its diagonal, V: the eigenvectors in its columns)"""
    A = np.array(A, dtype=np.float64)
    H, n, _ = A.shape
    V = np.tile(np.eye(n), (H, 1, 1))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq, app, aqq = A[:, p, q].copy(), A[:, p, p].copy(), A[:, q, q].copy()
                    skip = apq == 0.0
                    th = (aqq - app) / (2.0 * apq)
                    t = np.where(th >= 0.0, 1.0, -1.0) / (np.abs(th) + np.sqrt(th * th + 1.0))
                    t = np.where(skip, 0.0, t)
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    cp, cq = A[:, :, p].copy(), A[:, :, q].copy()
                    np_, nq = c[:, None] * cp - s[:, None] * cq, s[:, None] * cp + c[:, None] * cq
                    A[:, :, p], A[:, p, :], A[:, :, q], A[:, q, :] = np_, np_, nq, nq
                    A[:, p, p], A[:, q, q] = app - t * apq, aqq + t * apq
                    A[:, p, q], A[:, q, p] = np.where(skip, apq, 0.0), np.where(skip, apq, 0.0)
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p], V[:, :, q] = c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq
    return A, V


def project_essential(E, sweeps=SWEEPS3):
    """U diag(1, 1, 0) V^T of a batch [H][3][3] by a one-sided Jacobi (columns of B = E W made orthogonal; pairs (0,1), (0,2), (1,2)); the
    column of the smallest norm (the first of equals) is dropped; unit Frobenius norm.  -> (E', ok)"""
    B = np.array(E, dtype=np.float64)
    H = len(B)
    W = np.tile(np.eye(3), (H, 1, 1))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                bp, bq = B[:, :, p].copy(), B[:, :, q].copy()
                al, be, ga = (bp * bp).sum(1), (bq * bq).sum(1), (bp * bq).sum(1)
                ze = (be - al) / (2.0 * ga)
                t = np.where(ze >= 0.0, 1.0, -1.0) / (np.abs(ze) + np.sqrt(ze * ze + 1.0))
                t = np.where(ga == 0.0, 0.0, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = (t * c)[:, None]
                c = c[:, None]
                wp, wq = W[:, :, p].copy(), W[:, :, q].copy()
                B[:, :, p], B[:, :, q] = c * bp - s * bq, s * bp + c * bq
                W[:, :, p], W[:, :, q] = c * wp - s * wq, s * wp + c * wq
        nc = np.sqrt((B * B).sum(1))                      # [H][3] column norms
        drop = np.argmin(nc, axis=1)                      # the first of equals
        out, ok = np.zeros((H, 3, 3)), np.zeros(H, bool)
        for h in range(H):
            ca, cb = [c for c in range(3) if c != drop[h]]
            na, nb = nc[h, ca], nc[h, cb]
            ok[h] = bool(na > 0 and nb > 0 and np.isfinite(na) and np.isfinite(nb))
            if ok[h]:
                out[h] = (np.outer(B[h, :, ca] / na, W[h, :, ca]) + np.outer(B[h, :, cb] / nb, W[h, :, cb])) * 0.70710678118654752440
    return out, ok


def hartley(xy):
    """-> (s, cx, cy, ok): centroid, mean distance sqrt(2)"""
    c = xy.mean(axis=0) if len(xy) else np.zeros(2)
    m = np.sqrt(((xy - c) ** 2).sum(axis=1)).mean() if len(xy) else 0.0
    ok = bool(m > 0 and np.isfinite(m))
    return (np.sqrt(2.0) / m if ok else 0.0), c[0], c[1], ok


def design_ata(rows):
    """rows [m][4] normalised image coordinates {x1, y1, x2, y2} -> (A^T A [9][9], T1, T2, ok) of the Hartley-normalised eight-point system"""
    s1, cx1, cy1, ok1 = hartley(rows[:, :2])
    s2, cx2, cy2, ok2 = hartley(rows[:, 2:])
    T1 = np.array([[s1, 0, -s1 * cx1], [0, s1, -s1 * cy1], [0, 0, 1.0]])
    T2 = np.array([[s2, 0, -s2 * cx2], [0, s2, -s2 * cy2], [0, 0, 1.0]])
    x1, y1, x2, y2 = s1 * (rows[:, 0] - cx1), s1 * (rows[:, 1] - cy1), s2 * (rows[:, 2] - cx2), s2 * (rows[:, 3] - cy2)
    D = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=1)
    return D.T @ D, T1, T2, ok1 and ok2


def eight_point(row_sets):
    """the normalised eight-point solve of every row set (a list of [m][4] arrays, m >= 8) -> (E [H][9] -- 0: no model, ok [H],
    gap [H]: the second-smallest over the largest eigenvalue of A^T A as the Jacobi leaves them)"""
    H = len(row_sets)
    A, T1, T2, ok = np.zeros((H, 9, 9)), np.zeros((H, 3, 3)), np.zeros((H, 3, 3)), np.zeros(H, bool)
    for h, rows in enumerate(row_sets):
        a, T1[h], T2[h], ok[h] = design_ata(np.asarray(rows, dtype=np.float64))
        if ok[h] and np.isfinite(a).all():
            A[h] = a
        else:
            ok[h] = False
    L, V = jacobi_eig(A)
    lam = np.diagonal(L, axis1=1, axis2=2)
    m = np.argmin(lam, axis=1)                            # the first of equals
    Fh = np.stack([V[h, :, m[h]].reshape(3, 3) for h in range(H)]) if H else np.zeros((0, 3, 3))
    E0 = np.stack([T2[h].T @ Fh[h] @ T1[h] for h in range(H)]) if H else np.zeros((0, 3, 3))
    E, ok2 = project_essential(E0)
    ok &= ok2
    E[~ok] = 0.0
    ls = np.sort(lam, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(ls[:, -1] > 0, ls[:, 1] / ls[:, -1], 0.0)
    return E.reshape(H, 9), ok, gap


def estimate_emat(K1, K2, pts1, pts2, matches, n_ransac=200, max_epi_err=2.0, min_inlier_num=15, seed=0, k=0):
    """estimateEMat + evaluateEMat + getMatchedPts of job k -> dict(E, emat_ok, inlier_num, rounds, best_hyp, flags, epi_err, inlier (flags per
    match), new_matches, seeds, pix, hyp_sample [H][8], hyp_E [H][9], hyp_count [H], hyp_gap [H], round_E (every E that was scored behind
    the best hypothesis, kept or not), surf_num)"""
    matches = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
    p1, p2 = np.asarray(pts1, dtype=np.float64).reshape(-1, 2), np.asarray(pts2, dtype=np.float64).reshape(-1, 2)
    iK1, iK2 = inv33(np.asarray(K1, dtype=np.float64).reshape(9)).reshape(3, 3), inv33(np.asarray(K2, dtype=np.float64).reshape(9)).reshape(3, 3)
    n = len(matches)
    pix = np.concatenate([p1[matches[:, 0]], p2[matches[:, 1]]], axis=1) if n else np.zeros((0, 4))
    nrm = np.concatenate([normalise(iK1, pix[:, :2]), normalise(iK2, pix[:, 2:])], axis=1) if n else np.zeros((0, 4))
    H = int(n_ransac)
    out = dict(surf_num=n, pix=pix, hyp_sample=np.full((H, 8), -1, np.int32), hyp_E=np.zeros((H, 9)), hyp_count=np.zeros(H, np.int32),
               hyp_gap=np.zeros(H), round_E=[], E=np.zeros(9), emat_ok=0, inlier_num=0, rounds=0, best_hyp=-1, flags=TOO_FEW, epi_err=0.0,
               inlier=np.zeros(n, bool), new_matches=np.zeros((0, 2), np.int32), seeds=np.zeros((0, 4)))
    if n < 8:
        return out
    smp = [sample8(seed, k, h, n) for h in range(H)]
    live = [h for h in range(H) if smp[h] is not None]
    E, ok, gap = eight_point([nrm[smp[h]] for h in live])
    for a, h in enumerate(live):
        out["hyp_sample"][h], out["hyp_E"][h], out["hyp_gap"][h] = smp[h], E[a], gap[a]
        out["hyp_count"][h] = evaluate_emat(fmat(iK1, iK2, E[a]), pix, max_epi_err)[1] if ok[a] else 0
    best = int(np.argmax(out["hyp_count"]))               # the maximum count, then the lowest h
    cur = out["hyp_E"][best].copy()
    fl, cnt, err = evaluate_emat(fmat(iK1, iK2, cur), pix, max_epi_err)
    out["round_E"].append(cur.copy())
    rounds = 0
    for _ in range(REFIT_ROUNDS):
        if cnt < 8:
            break
        E2, ok2, _ = eight_point([nrm[fl]])
        if not ok2[0]:
            break
        out["round_E"].append(E2[0].copy())
        fl2, cnt2, err2 = evaluate_emat(fmat(iK1, iK2, E2[0]), pix, max_epi_err)
        if cnt2 < cnt:
            break
        cur, fl, cnt, err, rounds = E2[0].copy(), fl2, cnt2, err2, rounds + 1
    out.update(E=cur, inlier=fl, inlier_num=cnt, emat_ok=int(cnt >= min_inlier_num), rounds=rounds, best_hyp=best,
               flags=NO_MODEL if out["hyp_count"][best] == 0 else 0, epi_err=err, new_matches=matches[fl].astype(np.int32), seeds=pix[fl])
    return out


def front_job(cam1, cam2, ratio=0.8, max_dist=0.6, n_ransac=200, max_epi_err=2.0, min_inlier_num=15, seed=0, k=0):
    """the whole front of one job: cams are dict(pts [n][2], desc [n][dim], K [9]) -> estimate_emat's dict plus `match` (match_surf's)"""
    m = match_surf(cam1["pts"], cam1["desc"], cam2["pts"], cam2["desc"], ratio, max_dist)
    out = estimate_emat(cam1["K"], cam2["K"], cam1["pts"], cam2["pts"], m["matches"], n_ransac, max_epi_err, min_inlier_num, seed, k)
    out["match"] = m
    return out
