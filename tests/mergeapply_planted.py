"""Planted scenes for cs_recompute_map_points_keyfrms_dev (tests/test_mergeapply_gpu.py; the CPU tests check that the restatement takes the
planted views): the 64-lane block edges of a walk, equal maxima across blocks and segments, the store's end, corrupt pools, the selection's
edges, 9-16 cameras with two views each.  Layout: tests/mergeapply_ref.py's (frame-indexed history)."""
import numpy as np

from tests.mergeapply_golden_util import inv_k, pixel

K0 = np.array([520.0, 0.0, 320.0, 0.0, 515.0, 240.0, 0.0, 0.0, 1.0])
FAR = 6.0   # how far an outlier pose stands off the camera's path


def _finish(nC, nF, frame0, pos, chains, X, key_frames, seed=5, flags=None, first=None, last=None):
    """pos [nC][nF][3] camera centres (R = I, t = -pos); chains[p][c] = [(last, first), ...] newest first or None"""
    histR = np.tile(np.eye(3).reshape(9), (nC, nF, 1))
    histT = -np.asarray(pos, dtype=np.float64)
    nP = len(chains)
    ref = np.full((nP, nC, 4), -1, np.int32)
    ref[:, :, 1:3] = 0
    pools, n_slot = [[] for _ in range(nC)], [0] * nC
    for p in range(nP):
        for c in range(nC):
            segs = chains[p][c]
            if not segs:
                continue
            slots = list(range(n_slot[c], n_slot[c] + len(segs)))
            n_slot[c] += len(segs)
            nxt = -1
            for q in range(len(segs) - 1, 0, -1):
                pools[c].append((slots[q], segs[q][0], segs[q][1], nxt))
                nxt = len(pools[c]) - 1
            ref[p, c] = (slots[0], segs[0][0], segs[0][1], nxt)
    cap = max(1, max(len(q) for q in pools))
    pool = np.full((nC, cap, 4), -1, np.int32)
    for c in range(nC):
        if pools[c]:
            pool[c, :len(pools[c])] = np.array(pools[c], np.int32)
    N = max(1, max(n_slot))
    histXY = np.full((nC, nF, 2 * N), -1e9)
    K = np.tile(K0, (nC, 1))
    Kl, Rl, Tl, Xl = K.tolist(), histR.tolist(), histT.tolist(), np.asarray(X, dtype=np.float64).tolist()
    for p in range(nP):
        for c in range(nC):
            for q, (la, fi) in enumerate(chains[p][c] or []):
                slot = ref[p, c, 0] if q == 0 else None
                if q > 0:   # the q-th segment's slot: follow the links
                    sidx = ref[p, c, 3]
                    for _ in range(q - 1):
                        sidx = pool[c, sidx, 3]
                    slot = pool[c, sidx, 0]
                for f in range(la, fi - 1, -1):
                    i = f - frame0
                    if 0 <= i < nF:
                        histXY[c, i, slot], histXY[c, i, N + slot] = pixel(Kl[c], Rl[c][i], Tl[c][i], Xl[p], p, c, f, seed)
    X = np.asarray(X, dtype=np.float64)
    return dict(K=K, iK=np.stack([inv_k(k) for k in K]), histR=histR, histT=histT, histXY=histXY, N=N, nC=nC, nF=nF, frame0=frame0,
                featRef=ref, segPool=pool, X=X, M0=X + np.array([0.03, -0.02, 0.06]), cov0=np.tile((np.eye(3) * 0.01).reshape(9), (nP, 1)),
                key_frames=np.asarray(key_frames, np.int32), f_start=frame0, f_end=frame0 + nF - 1, sigma=3.0,
                flags=np.zeros(nP, np.uint8) if flags is None else np.asarray(flags, np.uint8),
                firstFrame=np.full(nP, frame0, np.int32) if first is None else np.asarray(first, np.int32),
                lastFrame=np.full(nP, frame0 + nF - 1, np.int32) if last is None else np.asarray(last, np.int32))


def _path(nF, c, rng):
    """a camera that creeps along x: the angle at a point grows with the distance walked, nothing stands out"""
    p = np.zeros((nF, 3))
    p[:, 0] = 0.4 * c + 1e-3 * np.arange(nF) + 1e-5 * rng.normal(size=nF)
    p[:, 1] = 1e-5 * rng.normal(size=nF)
    return p


RUNS = (63, 64, 65, 128, 129)
WIN = 131


def block_edges():
    """camera i walks runs of RUNS[i] key-frame nodes (every frame is a key frame); window q of WIN frames plants the widest angle at walk
    position (0, 63 -> run - 1 when shorter, 64 -> run - 1 when shorter, last)[q].  Returns (scene, want[p][c] = the planted frame)."""
    rng = np.random.default_rng(11)
    nC, nF, frame0 = len(RUNS), 4 * WIN, 1000
    pos = np.stack([_path(nF, c, rng) for c in range(nC)])
    chains, want, X = [], [], []
    for q in range(4):
        head = frame0 + q * WIN + WIN - 1
        ch, wt = [None] * nC, [None] * nC
        for c, n in enumerate(RUNS):
            k = (0, min(63, n - 1), min(64, n - 1), n - 1)[q]
            f = head - 1 - k
            pos[c, f - frame0] += (FAR, 0.3, 0.0)
            ch[c], wt[c] = [(head, head - n)], f
        chains.append(ch), want.append(wt), X.append([1.0 + 0.2 * q, 0.3, 9.0 + q])
    return _finish(nC, nF, frame0, pos, chains, X, range(frame0, frame0 + nF)), want


def equal_maxima():
    """camera 0: one run of 150 nodes with the SAME outlier pose at walk positions 10 and 100 (two 64-lane blocks); camera 1: two segments
    with that pose once in each; camera 2: once in the head's run and once in a linked segment.  The newest must win."""
    rng = np.random.default_rng(12)
    nC, nF, frame0 = 3, 200, 2000
    pos = np.stack([_path(nF, c, rng) for c in range(nC)])
    head = frame0 + nF - 1
    planted = ((head - 11, head - 101), (head - 20, head - 90), (head - 5, head - 120))
    for c, (a, b) in enumerate(planted):
        pos[c, a - frame0] += (FAR, 0.2, 0.0)
        pos[c, b - frame0] = pos[c, a - frame0]   # bit-identical
    (a0, _), (a1, _), (a2, _) = planted
    chains = [[[(head, head - 150)], [(head, head - 40), (head - 70, head - 110)], [(head, head - 30), (head - 100, head - 140)]]]
    return _finish(nC, nF, frame0, pos, chains, [[0.8, 0.2, 8.0]], range(frame0, frame0 + nF, 1)), [[a0, a1, a2]]


def many_cameras(nC):
    """nC cameras, every one with a key-frame head and a widest key node behind it: 2 nC views (32 at 16, the reference's array bound)"""
    rng = np.random.default_rng(13 + nC)
    nF, frame0 = 40, 500
    pos = np.stack([_path(nF, c, rng) for c in range(nC)])
    pos[:, :, 0] = pos[:, :, 0] * 0.5 + 0.02 * np.arange(nF)[None, :]
    keys = list(range(frame0 + 1, frame0 + nF, 3))
    head = keys[-1]
    chains, X = [], []
    for p in range(6):
        chains.append([[(head, frame0 + 2 + (p + c) % 5)] for c in range(nC)])
        X.append([2.0 + 0.3 * p, 0.2 * p - 0.5, 8.0 + p])
    S = _finish(nC, nF, frame0, pos, chains, X, keys)
    return S
