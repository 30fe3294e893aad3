"""numpy restatements for the merge pose correction (test infrastructure, no device):
  * relax_scaled: GlobalPoseGraph::computeNewCameraRotations (reference src/slam/SL_GlobalPoseEstimation.cpp:52-219) followed
    by computeNewCameraTranslations4 (:361-525), line by line as dense least squares (lstsq) and an SVD polar factor;
  * keygraph_plan: MergeCameraGroup::searchFirstKeyFrameForMerge (src/app/SL_MergeCameraGroup.cpp:884-906) and
    _constructGraphForKeyFrms (:907-1035) over plain records of the key frames."""
import numpy as np


def rotation_system(fixed, nodeR, id1, id2, edgeR):
    """(A, b, column of every node or -1): :52-197.  9 rows per edge with a free end, 9 unknowns per free node (row-major R)."""
    n = len(fixed)
    indC = -np.ones(n, int)
    indC[~fixed.astype(bool)] = np.arange(int((fixed == 0).sum()))
    rows = [k for k in range(len(id1)) if not (fixed[id1[k]] and fixed[id2[k]])]
    A = np.zeros((9 * len(rows), 9 * int((fixed == 0).sum())))
    b = np.zeros(9 * len(rows))
    for r, k in enumerate(rows):
        i, j, R = id1[k], id2[k], edgeR[k].reshape(3, 3)
        # R_j - R_ij R_i = 0, element (u, v): R_j[u, v] - sum_m R[u, m] R_i[m, v]
        for u in range(3):
            for v in range(3):
                row = 9 * r + 3 * u + v
                if not fixed[j]:
                    A[row, 9 * indC[j] + 3 * u + v] += 1.0
                else:
                    b[row] -= nodeR[j].reshape(3, 3)[u, v]
                for m in range(3):
                    if not fixed[i]:
                        A[row, 9 * indC[i] + 3 * m + v] -= R[u, m]
                    else:
                        b[row] += R[u, m] * nodeR[i].reshape(3, 3)[m, v]
    return A, b, indC


def translation4_system(fixed, nodeT, id1, id2, edgeR, edgeT, scale_id):
    """(A, b, column of every node or -1, {scale id: column}): :361-500.  scale_id[k] >= 0: the edge is `constraint` and
    `uncertainScale` with that CamPoseEdge::scaleId.  (The reference also reads indScale[-1] for a plain edge and never uses
    the value: not behaviour.)"""
    n = len(fixed)
    free = fixed == 0
    nv = int(free.sum())
    indC = -np.ones(n, int)
    indC[free] = np.arange(nv)
    rows = [k for k in range(len(id1)) if not (fixed[id1[k]] and fixed[id2[k]])]
    ids = sorted({int(s) for s in scale_id if s >= 0})      # sIdFlag / indScale (:383-403): ascending by id
    assert all(s < len(id1) for s in ids), "the reference indexes indScale[nEdges]"
    col = {s: 3 * nv + c for c, s in enumerate(ids)}
    A = np.zeros((3 * len(rows), 3 * nv + len(ids)))
    b = np.zeros(3 * len(rows))
    for r, k in enumerate(rows):
        i, j, R, t, s = id1[k], id2[k], edgeR[k].reshape(3, 3), edgeT[k], int(scale_id[k])
        sl = slice(3 * r, 3 * r + 3)
        if not fixed[j]:
            A[sl, 3 * indC[j]:3 * indC[j] + 3] += np.eye(3)
        if not fixed[i]:
            A[sl, 3 * indC[i]:3 * indC[i] + 3] -= R
        if s >= 0:
            A[sl, col[s]] -= t
        else:
            b[sl] += t
        if fixed[j]:
            b[sl] -= nodeT[j]
        if fixed[i]:
            b[sl] += R @ nodeT[i]
    return A, b, indC, col


def polar(M):
    """approxRotationMat: U V^T of the SVD"""
    U, _, Vt = np.linalg.svd(M)
    return U @ Vt


def relax_scaled(fixed, nodeR, nodeT, id1, id2, edgeR, edgeT, scale_id):
    """one graph -> (newR [n,9], newT [n,3], edgeS [e], A_t): fixed nodes copied (:213-214, :507-509), the scale written to
    every uncertain-scale edge (:515-522), A_t the translation matrix (for the rank assertion)"""
    fixed = np.asarray(fixed, np.uint8)
    nodeR, nodeT = np.asarray(nodeR, float).reshape(-1, 9), np.asarray(nodeT, float).reshape(-1, 3)
    edgeR, edgeT = np.asarray(edgeR, float).reshape(-1, 9), np.asarray(edgeT, float).reshape(-1, 3)
    newR, newT, edgeS = nodeR.copy(), nodeT.copy(), np.zeros(len(id1))
    A, b, indC = rotation_system(fixed, nodeR, id1, id2, edgeR)
    if A.shape[1]:
        x = np.linalg.lstsq(A, b, rcond=None)[0]
        for k in np.nonzero(indC >= 0)[0]:
            newR[k] = polar(x[9 * indC[k]:9 * indC[k] + 9].reshape(3, 3)).reshape(9)
    At, bt, indC, col = translation4_system(fixed, nodeT, id1, id2, edgeR, edgeT, scale_id)
    if At.shape[1]:
        x = np.linalg.lstsq(At, bt, rcond=None)[0]
        for k in np.nonzero(indC >= 0)[0]:
            newT[k] = x[3 * indC[k]:3 * indC[k] + 3]
        for k, s in enumerate(scale_id):
            if s >= 0:
                edgeS[k] = x[col[int(s)]]
    return newR, newT, edgeS, At


def keygraph_plan(frames, groups, cam_ids, first_constrain, camid1, camid2, infos, n_max_keyfrm=100):
    """frames[k]: frame number of key frame k, oldest first (the last one is the current key frame); groups[k]: its camera
    groups, a list of camera-id lists; cam_ids ascending; first_constrain: index of m_pFirstConstrainFrm; infos: the valid
    merge infos (frame1, cam1, frame2, cam2) with FRAME NUMBERS.  Returns None where the reference asserts on a null
    m_pFixedKeyFrm, else dict(fixed_kf, node_kf, node_cam, fixed, id1, id2, scale_id, n_constraint)."""
    first_f = frames[first_constrain]
    fixed_kf, n, found = None, 0, False
    k = len(frames) - 1
    while k >= 0 and n <= n_max_keyfrm and not found:      # :888: kf = m_pCurKeyFrm; kf && n <= nMax && !find; kf = kf->prev
        if frames[k] >= first_f:
            k -= 1
            continue
        for g in groups[k]:
            if camid1 in g and camid2 in g:
                found = True
                break
        fixed_kf = k
        n += 1
        k -= 1
    if fixed_kf is None:
        return None
    cam_ids = list(cam_ids)
    node_kf, node_cam, node_of = [], [], {}
    for kf in range(fixed_kf, len(frames)):
        for c in cam_ids:
            node_of[(frames[kf], c)] = len(node_kf)
            node_kf.append(kf), node_cam.append(c)
    fixed = [1 if kf == fixed_kf else 0 for kf in node_kf]
    id1, id2, sid = [], [], []
    for kf in range(fixed_kf, len(frames)):
        f = frames[kf]
        for g in groups[kf]:
            cams = [c for c in g if c in cam_ids]
            if len(cams) > 1 and f <= first_f:
                for i in range(1, len(cams)):
                    id1.append(node_of[(f, cams[i - 1])]), id2.append(node_of[(f, cams[i])]), sid.append(-1)
                if len(cams) > 2:
                    id1.append(node_of[(f, cams[-1])]), id2.append(node_of[(f, cams[0])]), sid.append(-1)
        if kf != fixed_kf:
            for c in cam_ids:
                id1.append(node_of[(frames[kf - 1], c)]), id2.append(node_of[(f, c)]), sid.append(-1)
    nc = 0
    for (f1, c1, f2, c2) in infos:
        id1.append(node_of[(f1, c1)]), id2.append(node_of[(f2, c2)]), sid.append(0)
        nc += 1
    i32 = lambda v: np.array(v, np.int32)  # noqa: E731
    return dict(fixed_kf=fixed_kf, node_kf=i32(node_kf), node_cam=i32(node_cam), fixed=np.array(fixed, np.uint8), id1=i32(id1),
                id2=i32(id2), scale_id=i32(sid), n_constraint=nc)
