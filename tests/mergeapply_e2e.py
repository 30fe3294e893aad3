"""The end-to-end scene of the merge tests: 4 cameras in two groups, 6 key frames x 4 frames per interval, 192 points on 64
slots per camera.  Group 2's history and the points only it sees carry make_merge_pose_graph's drift; the merge infos come from the truth.
Also the host restatement of the whole sequence (pose correction -> re-triangulation -> groups) from tests/mergegraph_ref.py, the oracle's
chain relaxation and tests/mergeapply_ref.py."""
import numpy as np

from coslam_amd.synth import make_merge_pose_graph
from tests.mergeapply_golden_util import inv_k, pixel

K0 = np.array([520.0, 0.0, 320.0, 0.0, 515.0, 240.0, 0.0, 0.0, 1.0])
FRAME0 = 900


def build(n_cams=4, n_key=6, step=4, split=2, seed=3, n_slots=64):
    m = make_merge_pose_graph(n_cams, n_key, 1, split, seed=seed, frames_per_interval=step)
    ch = m["chains"]
    nF = (n_key - 1) * step + 1
    key_frames = np.array([FRAME0 + k * step for k in range(n_key)], np.int32)
    # the truth of every frame is not among synth's outputs: the chain of the FIRST group is undrifted (truth), the second group's truth is
    # rebuilt from the truth at the key frames and the drifted odometry in between -- good enough for pixels: what matters is that the
    # second group's views disagree with the first group's until the correction
    curR, curT = ch["nodeR"].reshape(n_cams, nF, 9).copy(), ch["nodeT"].reshape(n_cams, nF, 3).copy()
    truR, truT = curR.copy(), curT.copy()
    for i, (k, c) in enumerate(zip(m["node_kf"], m["node_cam"])):
        truR[c, k * step], truT[c, k * step] = m["truthR"][i], m["truthT"][i]
    for c in range(split, n_cams):          # between key frames: the drift spread linearly over the interval (first order)
        for k in range(n_key - 1):
            a, b = k * step, (k + 1) * step
            dRa, dRb = truR[c, a].reshape(3, 3) @ curR[c, a].reshape(3, 3).T, truR[c, b].reshape(3, 3) @ curR[c, b].reshape(3, 3).T
            for i in range(a + 1, b):
                w = (i - a) / step
                D = (1 - w) * dRa + w * dRb
                U, _s, Vt = np.linalg.svd(D)
                truR[c, i] = ((U @ Vt) @ curR[c, i].reshape(3, 3)).reshape(9)
                truT[c, i] = curT[c, i] + (1 - w) * (truT[c, a] - curT[c, a]) + w * (truT[c, b] - curT[c, b])
    windows = [(0, step), (step + 1, 3 * step), (3 * step + 1, 5 * step)]
    nP = n_slots * len(windows)
    rng = np.random.default_rng(seed + 100)
    X = np.stack([rng.uniform(-1.5, 1.5, nP), rng.uniform(-1.5, 1.5, nP), rng.uniform(14, 20, nP)], axis=1)
    ref = np.full((nP, n_cams, 4), -1, np.int32)
    ref[:, :, 1:3] = 0
    histXY = np.full((n_cams, nF, 2 * n_slots), -1e9)
    Kl = [K0.tolist()] * n_cams
    only2 = np.zeros(nP, bool)
    first, last = np.zeros(nP, np.int32), np.zeros(nP, np.int32)
    for p in range(nP):
        slot, (lo, hi) = p % n_slots, windows[p // n_slots]
        kind = p % 3                                     # 0: both groups see it, 1: group 1 only, 2: group 2 only
        cams = range(n_cams) if kind == 0 else (range(split) if kind == 1 else range(split, n_cams))
        only2[p] = kind == 2
        for c in cams:
            ref[p, c] = (slot, FRAME0 + hi, FRAME0 + lo, -1)
            for i in range(lo, hi + 1):
                histXY[c, i, slot], histXY[c, i, n_slots + slot] = pixel(Kl[c], truR[c, i].tolist(), truT[c, i].tolist(), X[p].tolist(), p, c, i, seed)
        first[p], last[p] = FRAME0 + lo, FRAME0 + hi
    S = dict(K=np.tile(K0, (n_cams, 1)), iK=np.tile(inv_k(K0), (n_cams, 1)), histR=curR, histT=curT, histXY=histXY, N=n_slots, nC=n_cams,
             nF=nF, frame0=FRAME0, featRef=ref, segPool=np.full((n_cams, 0, 4), -1, np.int32), X=X, cov0=np.tile((np.eye(3) * 0.01).reshape(9), (nP, 1)),
             key_frames=key_frames, f_start=FRAME0, f_end=FRAME0 + nF - 1, sigma=3.0, flags=np.zeros(nP, np.uint8), firstFrame=first, lastFrame=last)
    plan = dict(fixed_kf=0, node_kf=m["node_kf"], node_cam=m["node_cam"], fixed=m["fixed"], id1=m["id1"], id2=m["id2"], scale_id=m["scale_id"])
    sc = m["scale_id"] >= 0
    return dict(m=m, S=S, plan=plan, infoR=m["edgeR"][sc], infoT=m["edgeT"][sc], only2=only2, truR=truR, truT=truT, split=split,
                groups=[list(range(split)), list(range(split, n_cams))])


def start_points(E, ref_mod):
    """the map before the merge: every point triangulated from the poses its cameras HAVE (group 2's: drifted) -- the key-frame views"""
    S = E["S"]
    M = S["X"] + 0.02
    cov = S["cov0"].copy()
    ref_mod.recompute_map_points_keyfrms(S["K"], S["iK"], S["histR"], S["histT"], S["histXY"], S["frame0"], S["featRef"], S["segPool"], None,
                                         S["firstFrame"], S["lastFrame"], S["flags"], S["f_start"], S["f_end"], S["key_frames"], M, cov, S["sigma"])
    return M, cov


def corrected_poses_host(E):
    """the pose correction on the host: tests/mergegraph_ref.py's relax_scaled on the key graph, the oracle's relaxation on every chain with
    the corrected key poses held (edges from the poses BEFORE the correction) -> (histR, histT) of the whole span"""
    import oracle
    from tests import mergegraph_ref as mref

    m, ch = E["m"], E["m"]["chains"]
    wR, wT, _wS, _A = mref.relax_scaled(m["fixed"], m["nodeR"], m["nodeT"], m["id1"], m["id2"], m["edgeR"], m["edgeT"], m["scale_id"])
    cR, cT = ch["nodeR"].copy(), ch["nodeT"].copy()
    cR[ch["key_node"]], cT[ch["key_node"]] = wR, wT
    outR, outT = cR.copy(), cT.copy()
    for c, (fixed, id1, id2) in enumerate(ch["graphs"]):
        ns = slice(ch["node_ptr"][c], ch["node_ptr"][c + 1])
        R0, T0 = ch["nodeR"][ns].reshape(-1, 3, 3), ch["nodeT"][ns]
        eR = np.einsum("eij,ekj->eik", R0[id2], R0[id1])
        eT = T0[id2] - np.einsum("eij,ej->ei", eR, T0[id1])
        rc, oR, oT = oracle.posegraph_relax(fixed, cR[ns], cT[ns], id1, id2, eR.reshape(-1, 9), eT)
        assert rc == 0
        outR[ns], outT[ns] = oR, oT
    nC, nF = E["S"]["nC"], E["S"]["nF"]
    return outR.reshape(nC, nF, 9), outT.reshape(nC, nF, 3)


def reproj_median(E, M, histR, histT):
    """median pixel distance of the drifted group's own points from their projections into the OTHER group's cameras at the current key frame,
    against where those cameras would see the true point"""
    S = E["S"]
    errs = []
    for p in np.nonzero(E["only2"])[0]:
        for c in range(E["split"]):
            R, t = histR[c, -1].reshape(3, 3), histT[c, -1]
            K = K0.reshape(3, 3)
            a, b = K @ (R @ M[p] + t), K @ (E["truR"][c, -1].reshape(3, 3) @ S["X"][p] + E["truT"][c, -1])
            errs.append(float(np.hypot(a[0] / a[2] - b[0] / b[2], a[1] / a[2] - b[1] / b[2])))
    return float(np.median(errs))
