"""Plain restatement of the merge matcher: MergeCameraGroup::storeFeaturePoints, matchFeaturePointsNCC and the loop of
matchMergableCameras (reference src/app/SL_MergeCameraGroup.cpp:179-188, 262-307, 320-421), on slots behind a validity mask.

The OpenCV cutter and getEpiNccMat are oracle/ncc_oracle.c's restatements; getDisparityMat / greedyGuidedNCCMatch / getMatchedPts are
un-vendored LibVisualSLAM, this library's definitions (csrc/newpts.hip:15-21, oracle/ncc_oracle.c:330-353) operation for operation.
TEST INFRASTRUCTURE: sequential, one candidate at a time."""
import numpy as np


def inv33(K):
    """mat33Inv as the reference drivers are linked with it (oracle/ref_shim/shim_impl.cpp matInv): Gauss-Jordan with partial pivoting"""
    M = [[float(K[3 * i + j]) for j in range(3)] + [1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for c in range(3):
        piv = c
        for r in range(c + 1, 3):
            if abs(M[r][c]) > abs(M[piv][c]):
                piv = r
        M[c], M[piv] = M[piv], M[c]
        d = M[c][c]
        M[c] = [v / d for v in M[c]]
        for r in range(3):
            if r == c or M[r][c] == 0.0:
                continue
            f = M[r][c]
            M[r] = [M[r][j] - f * M[c][j] for j in range(6)]
    return np.array([M[i][3 + j] for i in range(3) for j in range(3)])


def fmat(K1, K2, E):
    """mat33Trans(E, Et); getFMat(iK2, iK1, Et, F): T = iK1^T Et accumulated from 0 (matATB), F = T iK2 (mat33AB)"""
    K1, K2 = np.asarray(K1, dtype=np.float64).reshape(9), np.asarray(K2, dtype=np.float64).reshape(9)
    a, b = [float(v) for v in inv33(K1)], [float(v) for v in inv33(K2)]
    E = [float(v) for v in np.asarray(E, dtype=np.float64).reshape(9)]
    T = []
    for i in range(3):
        for j in range(3):
            t = 0.0
            for k in range(3):
                t += a[3 * k + i] * E[3 * j + k]
            T.append(t)
    return np.array([T[3 * i] * b[j] + T[3 * i + 1] * b[3 + j] + T[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)])


def valid_mask(state):
    """storeFeaturePoints: camera c's list = its slots with state 0 / 1 in slot order"""
    s = np.asarray(state)
    return ((s == 0) | (s == 1)).astype(np.int32)


def scaled_blocks(small, xy, scale):
    """getScaledNCCBlocks: cv::getRectSubPix(small, 11 x 11, (x scale, y scale)) of every slot -> (blocks [N][128], abc [N][4])"""
    import oracle

    xy = np.asarray(xy, dtype=np.float64).reshape(2, -1)
    return oracle.get_ncc_blocks(small, xy[0] * scale, xy[1] * scale, 1.0)


def candidates(F, xy1, blk1, abc1, valid1, xy2, blk2, abc2, valid2, epi_max, ncc_min):
    """getEpiNccMat as a list of (i, j, epi, ncc), row-major"""
    import oracle

    xy1, xy2 = np.asarray(xy1, dtype=np.float64).reshape(2, -1), np.asarray(xy2, dtype=np.float64).reshape(2, -1)
    epi, ncc = oracle.ncc_epi_mat(F, xy1[0], xy1[1], blk1, abc1, valid1, xy2[0], xy2[1], blk2, abc2, valid2, epi_max, ncc_min, -1.0)
    ii, jj = np.nonzero(ncc != -1.0)
    return [(int(i), int(j), float(epi[i, j]), float(ncc[i, j])) for i, j in zip(ii, jj)]


def guide(cands, xy1, xy2, seeds, max_disp):
    """getDisparityMat's test of every candidate: the seed nearest to c1_i in image 1 (squared distance, the first of equals);
    (i, j) survives iff sqrt(ex^2 + ey^2) <= maxDisp, e = (c2_j - c1_i) - (s2_k - s1_k).  No seeds: no guide."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 4)
    if len(seeds) == 0:
        return list(cands)
    xy1, xy2 = np.asarray(xy1, dtype=np.float64).reshape(2, -1), np.asarray(xy2, dtype=np.float64).reshape(2, -1)
    out, near = [], {}
    for c in cands:
        i, j = c[0], c[1]
        x1, y1 = xy1[0, i], xy1[1, i]
        if i not in near:
            dx, dy = seeds[:, 0] - x1, seeds[:, 1] - y1
            near[i] = int(np.argmin(dx * dx + dy * dy))     # argmin: the first of equals
        s = seeds[near[i]]
        ex, ey = (xy2[0, j] - x1) - (s[2] - s[0]), (xy2[1, j] - y1) - (s[3] - s[1])
        if np.sqrt(ex * ex + ey * ey) <= max_disp:
            out.append(c)
    return out


def greedy(cands):
    """greedyNCCMatch over a candidate list: score falling, then row rising, then column rising; a candidate is a match when neither its
    row nor its column has one -> [(i, j, score)] in acceptance order"""
    rows, cols, out = set(), set(), []
    for c in sorted(cands, key=lambda c: (-c[-1], c[0], c[1])):
        if c[0] in rows or c[1] in cols:
            continue
        rows.add(c[0]), cols.add(c[1])
        out.append((c[0], c[1], c[-1]))
    return out


def rounds_match(i, j, score, N):
    """The device's form in numpy: rounds of locally dominant candidates.  Every live candidate bids for its row and its column (maximum of
    the score), equal bids are settled by the minimum of the column (row) -- a candidate that holds both is a match; its row's and column's
    candidates die.  -> ([(i, j, score)] ranked by the total order, rounds)"""
    i, j, s = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(score, dtype=np.float64)
    live = np.arange(len(i))
    won, rounds = [], 0
    row_m, col_m = np.full(N, -1), np.full(N, -1)
    while len(live) and rounds < N:
        li, lj, ls = i[live], j[live], s[live]
        rb, cb = np.full(N, -np.inf), np.full(N, -np.inf)
        np.maximum.at(rb, li, ls), np.maximum.at(cb, lj, ls)
        rt, ct = np.full(N, np.iinfo(np.int64).max), np.full(N, np.iinfo(np.int64).max)
        np.minimum.at(rt, li[ls == rb[li]], lj[ls == rb[li]])
        np.minimum.at(ct, lj[ls == cb[lj]], li[ls == cb[lj]])
        win = (ls == rb[li]) & (rt[li] == lj) & (ls == cb[lj]) & (ct[lj] == li)
        for q in live[win]:
            if row_m[i[q]] < 0:                      # (a pair listed twice is one match)
                row_m[i[q]], col_m[j[q]] = j[q], i[q]
                won.append((int(i[q]), int(j[q]), float(s[q])))
        live = live[(row_m[li] < 0) & (col_m[lj] < 0)]
        rounds += 1
    return sorted(won, key=lambda c: (-c[2], c[0], c[1])), rounds


def match_job(cams, Ws, Hs, job, epi_max=20.0, ncc_min=0.45, max_disp=150.0):
    """matchFeaturePointsNCC of one job.  cams: per camera dict(xy [2][N], state [N], K [9], imgSmall [Hs][Ws] uint8, imgScale);
    job: dict(iCam, jCam, E, seeds [n][4]).  -> dict(F, cands (the list in front of the guide), matches [(i, j, score)], blocks / abc /
    valid of both cameras)"""
    a, b = cams[job["iCam"]], cams[job["jCam"]]
    F = fmat(a["K"], b["K"], job["E"])
    b1, c1 = scaled_blocks(a["imgSmall"], a["xy"], a["imgScale"])
    b2, c2 = scaled_blocks(b["imgSmall"], b["xy"], b["imgScale"])
    v1, v2 = valid_mask(a["state"]), valid_mask(b["state"])
    cands = candidates(F, a["xy"], b1, c1, v1, b["xy"], b2, c2, v2, epi_max, ncc_min)
    kept = guide(cands, a["xy"], b["xy"], job.get("seeds", np.zeros((0, 4))), max_disp)
    return dict(F=F, cands=cands, matches=greedy(kept), blocks=(b1, b2), abc=(c1, c2), valid=(v1, v2))


def select(infos, surf_num, emat_ok, ncc_num, group_size, eligible=None):
    """matchMergableCameras' loop (:325-414) as it runs -- see cs_merge_match_select (include/coslam_hip.h)"""
    by_pair = {}
    for e, inf in enumerate(infos):
        by_pair.setdefault((int(inf[2]), int(inf[5])), []).append(e)
    feat = [0] * 512
    out = dict(status=0, entry=-1, maxk=-1, maxiCam=-1, maxjCam=-1, maxgId1=-1, maxgId2=-1, gid1=-1, gid2=-1, camid1=-1, camid2=-1)
    matched, k = False, 0
    for key in sorted(by_pair):
        n_min = 20
        for i, e in enumerate(by_pair[key]):
            if surf_num[e] < 25 or not emat_ok[e]:
                continue
            feat[k] = int(ncc_num[e])
            matched = True
            if feat[k] > n_min and (eligible is None or eligible[e]):
                n_min = feat[i]
                out.update(maxk=k, entry=e, maxiCam=int(infos[e][1]), maxjCam=int(infos[e][4]), maxgId1=key[0], maxgId2=key[1])
            k += 1
    if not matched:
        return out
    if out["maxk"] < 0:
        out["status"] = -1
        return out
    out["status"] = 1
    if group_size[out["maxgId1"]] > group_size[out["maxgId2"]]:
        out.update(gid1=out["maxgId1"], gid2=out["maxgId2"], camid1=out["maxiCam"], camid2=out["maxjCam"])
    else:
        out.update(gid1=out["maxgId2"], gid2=out["maxgId1"], camid1=out["maxjCam"], camid2=out["maxiCam"])
    return out


# ---- scenes: two textured views of one plane of dots, so that true correspondences have matching patches ----------------------------------
def textured_image(W, H, rng, blobs=220):
    """smooth random texture with enough contrast for NCC on 11 x 11 blocks"""
    img = rng.normal(0, 1, (H, W))
    for _ in range(3):                                   # cheap blur: neighbours' mean
        img = (img + np.roll(img, 1, 0) + np.roll(img, -1, 0) + np.roll(img, 1, 1) + np.roll(img, -1, 1)) / 5.0
    img = (img - img.min()) / (img.max() - img.min())
    return np.ascontiguousarray(np.clip(img * 255.0, 0, 255).astype(np.uint8))


def shifted_pair_scene(N=70, W=192, H=144, scale=0.3, shift=(12.0, -7.0), n_cams=2, dead_every=7, seed=0, n_seeds=6, pair=(0, 1)):
    """Cameras pair[0] and pair[1] see the same fronto-parallel texture, camera pair[1] shifted by `shift` SMALL-image pixels (a pure
    translation: E = [t]x with t along the shift, every true correspondence lies on its epipolar line and its patches agree up to the
    cutter's interpolation).  Positions are full-image pixels (small / scale); every dead_every-th slot is dead (state -1: rank != slot);
    some features sit within 5 px of the small image's border.  The other cameras hold an unrelated texture."""
    rng = np.random.default_rng(seed)
    big = textured_image(W + 64, H + 64, rng)
    sx, sy = shift
    K = np.array([300.0, 0, W / scale / 2, 0, 300.0, H / scale / 2, 0, 0, 1.0])
    cams = []
    for c in range(n_cams):
        if c == pair[0]:
            small = big[32:32 + H, 32:32 + W]
        elif c == pair[1]:
            small = big[32 - int(sy):32 - int(sy) + H, 32 - int(sx):32 - int(sx) + W]
        else:
            small = textured_image(W, H, np.random.default_rng(seed + 100 + c))
        cams.append(dict(K=K.copy(), imgSmall=np.ascontiguousarray(small), imgScale=scale))
    # features of camera pair[0] on the small image; camera pair[1] sees them shifted
    px = rng.uniform(3.0, W - 3.0 - abs(sx) - 1, N) + (abs(sx) + 1 if sx < 0 else 0)
    py = rng.uniform(3.0, H - 3.0 - abs(sy) - 1, N) + (abs(sy) + 1 if sy < 0 else 0)
    px[:4], py[:4] = [1.5, W - abs(sx) - 2.5, 40.25, 60.0], [30.0, 50.5, 2.0, H - abs(sy) - 2.25]   # the cutter's border path
    if sx < 0:
        px[:2] = [abs(sx) + 1.5, W - 2.5]
    if sy < 0:
        py[2:4] = [abs(sy) + 2.0, H - 2.25]
    perm = rng.permutation(N)
    for c in range(n_cams):
        state = np.where(np.arange(N) % dead_every == 3, -1, np.arange(N) % 2).astype(np.int32)
        if c == pair[0]:
            xy = np.stack([px, py]) / scale
        elif c == pair[1]:
            xy = np.stack([px[perm] + int(sx), py[perm] + int(sy)]) / scale
        else:
            xy = np.stack([rng.uniform(8, W - 8, N), rng.uniform(8, H - 8, N)]) / scale
        cams[c].update(xy=np.ascontiguousarray(xy), state=state)
    t = np.array([float(int(sx)), float(int(sy)), 0.0])
    t /= np.linalg.norm(t)
    E = np.array([0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0.0])
    inv = np.argsort(perm)                      # slot of camera pair[1] that holds feature i of camera pair[0]
    ids = rng.choice(N, n_seeds, replace=False) if n_seeds else np.zeros(0, int)
    a, b = cams[pair[0]]["xy"], cams[pair[1]]["xy"]
    seeds = np.array([[a[0, i], a[1, i], b[0, inv[i]], b[1, inv[i]]] for i in ids]).reshape(-1, 4)
    return cams, dict(iCam=pair[0], jCam=pair[1], E=E, seeds=seeds), inv
