"""tests/golden/mergeapply_golden.npz -> the arrays the tests and the restatement take (shared by tests/golden/make_mergeapply_golden.py,
which writes the file, and the tests, which read it).

To keep the file small it holds no pixel and no full-precision pose: poses are stored as float32 (and used as exactly those values in
binary64 -- the reference's function takes R, t as given, a rotation that is orthogonal to 1e-7 is as good a test vector), and the pixel of
node (point p, camera c, frame f) is a FUNCTION of the stored values: the projection of the point's true position X under that pose plus a
hashed offset of up to 0.6 px, evaluated in Python floats with a fixed operation order (IEEE binary64 +, *, / only: the same bits wherever
it runs).  The generator fed the reference's driver the pixels of this same function."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mergeapply_golden.npz")


def inv_k(K):
    """getInvK as the reference driver's stand-in computes it (oracle/ref_shim/ref_triangulate_impl.cpp)"""
    fx, s, cx, fy, cy = (float(K[i]) for i in (0, 1, 2, 4, 5))
    return np.array([1.0 / fx, -s / (fx * fy), (s * cy - cx * fy) / (fx * fy), 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0])


def _hash(p, c, f, seed):
    return ((p * 73856093) ^ (c * 19349663) ^ (f * 83492791) ^ (seed * 2654435761)) & 0xFFFFFFFF


def pixel(K, R, t, X, p, c, f, seed):
    """the pixel of node (p, c, f): Python floats, fixed order"""
    Xc = [((R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2]) + t[r] for r in range(3)]
    h = _hash(p, c, f, seed)
    n0, n1 = ((h & 0xFFFF) - 32768) / 65536.0 * 1.2, (((h >> 16) & 0xFFFF) - 32768) / 65536.0 * 1.2
    return ((K[0] * Xc[0] + K[1] * Xc[1]) + K[2] * Xc[2]) / Xc[2] + n0, (K[4] * Xc[1] + K[5] * Xc[2]) / Xc[2] + n1


def start_point(X, p, seed):
    """the map point's position before the call: the true position off by up to 5 cm / 10 cm"""
    h = _hash(p, 77, 1234, seed)
    d = [(((h >> (8 * q)) & 0xFF) - 128) / 128.0 for q in range(3)]
    return [X[0] + 0.05 * d[0], X[1] + 0.05 * d[1], X[2] + 0.1 * d[2]]


def start_cov(p):
    return (np.eye(3) * (0.01 * (1 + p % 7))).reshape(9)


def chain_nodes(ref, pool_c):
    """[(frame, slot)] of a whole chain, newest first (no store, no key-frame filter); a corrupt pool is not followed"""
    out = []
    slot, frame, first, seg = (int(v) for v in ref)
    if slot < 0:
        return out
    out.append((frame, slot))
    hi, lo = frame - 1, first
    while True:
        out += [(f, slot) for f in range(hi, lo - 1, -1)]
        if seg < 0:
            return out
        slot, hi, lo, seg = (int(v) for v in pool_c[seg])


def expand(S, seed):
    """S: dict(K, R, t (float32 or float64), frame0, X, featRef, segPool, ...) -> adds iK, histR, histT (float64), histXY, N, M0, cov0"""
    K = np.asarray(S["K"], dtype=np.float64).reshape(-1, 9)
    nC = K.shape[0]
    histR = np.asarray(S["R"]).astype(np.float64).reshape(nC, -1, 9)
    histT = np.asarray(S["t"]).astype(np.float64).reshape(nC, -1, 3)
    nF, frame0 = histR.shape[1], int(S["frame0"])
    X = np.asarray(S["X"]).astype(np.float64)
    ref, pool = np.asarray(S["featRef"]).astype(np.int32), np.asarray(S["segPool"]).astype(np.int32)
    N = int(max(1, ref[:, :, 0].max() + 1, pool[:, :, 0].max() + 1 if pool.size else 0))
    histXY = np.full((nC, nF, 2 * N), -1e9)
    Kl, Rl, Tl, Xl = K.tolist(), histR.tolist(), histT.tolist(), X.tolist()
    for p in range(ref.shape[0]):
        for c in range(nC):
            for f, slot in chain_nodes(ref[p, c], pool[c]):
                i = f - frame0
                if 0 <= i < nF:
                    histXY[c, i, slot], histXY[c, i, N + slot] = pixel(Kl[c], Rl[c][i], Tl[c][i], Xl[p], p, c, f, seed)
    out = dict(S)
    out.update(K=K, iK=np.stack([inv_k(k) for k in K]), histR=histR, histT=histT, histXY=histXY, N=N, nC=nC, nF=nF, frame0=frame0,
               featRef=ref, segPool=pool, X=X, M0=np.array([start_point(Xl[p], p, seed) for p in range(len(Xl))]).reshape(-1, 3),
               cov0=np.stack([start_cov(p) for p in range(len(Xl))]).reshape(-1, 9))
    return out


def scene(g, sc):
    """scene sc of the loaded golden file, expanded"""
    keys = ("K", "R", "t", "frame0", "X", "featRef", "segPool", "key_frames", "f_start", "f_end", "sigma", "flags", "firstFrame", "lastFrame",
            "list", "M_ref", "cov_ref", "selected", "filter_points")
    S = expand({k: g[f"s{sc}_{k}"] for k in keys}, int(g["seed"]) + sc)
    for k in ("f_start", "f_end"):
        S[k] = int(S[k])
    S["sigma"] = float(S["sigma"])
    S["key_frames"] = np.asarray(S["key_frames"]).astype(np.int32)
    for k in ("flags", "firstFrame", "lastFrame"):
        S[k] = np.asarray(S[k]).astype(np.uint8 if k == "flags" else np.int32)
    return S
