"""Plain numpy restatement of the SURF stage: integral image -> fast-Hessian layers -> maxima -> ordered list ->
orientation -> descriptors.  The reference's SURF is external (OpenCV nonfree / asrl GPU-SURF behind ::detectSURFPoints,
src/app/SL_MergeCameraGroup.cpp:311): THE DEFINITION IS THIS FILE.  Written from the definition, never calls the library.
TEST INFRASTRUCTURE.

Exact layers: box sums are integers, responses are f64 in one written-out expression order, every sum that is not an integer runs in a
fixed order (np.cumsum is sequential; np.sum is pairwise and is not used on floats).  exp / cos / sin / atan2 are libm's (math.*), the
only places where the device may differ by ulps."""
import math

import numpy as np

MAX_OCTAVES, MAX_LAYERS = 5, 6          # layers per octave: nOctaveLayers + 2 <= 6
ORI_GRID = [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36]   # 109 samples, i (x) outer, j (y) inner
ORI_WEIGHT = [math.exp(-(i * i + j * j) / 8.0) for i, j in ORI_GRID]                    # sigma = 2 s
N_WINDOWS, WINDOW_STEP, WINDOW_WIDTH = 72, math.pi / 36.0, math.pi / 3.0
TWO_PI = 2.0 * math.pi
DESC_SIGMA2 = 2.0 * 3.3 * 3.3
# the 20 x 20 descriptor samples: a (x) and b (y) in 0..19, offsets (a - 9.5, b - 9.5) in units of s, weight index b * 20 + a
DESC_WEIGHT = [math.exp(-((a - 9.5) * (a - 9.5) + (b - 9.5) * (b - 9.5)) / DESC_SIGMA2) for b in range(20) for a in range(20)]


# ---- 1. integral image ----------------------------------------------------------------------------------------------------------------
def integral(img):
    """u32 [(H + 1)][(W + 1)], row 0 and column 0 zero; refuses W H 255 >= 2^32"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    if W * H * 255 >= 1 << 32:
        raise ValueError("W H 255 >= 2^32")
    I = np.zeros((H + 1, W + 1), np.uint64)
    I[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.uint64), axis=0), axis=1)
    return I.astype(np.uint32)


def box(I, r0, c0, r1, c1):
    """the sum over rows [r0, r1) and columns [c0, c1), every corner clamped into [0, H] x [0, W]: a box that leaves the image is the
    sum over its part inside.  int64, scalars or arrays."""
    H, W = I.shape[0] - 1, I.shape[1] - 1
    r0, r1 = np.clip(r0, 0, H), np.clip(r1, 0, H)
    c0, c1 = np.clip(c0, 0, W), np.clip(c1, 0, W)
    J = I.astype(np.int64) if I.dtype != np.int64 else I
    return J[r1, c1] - J[r0, c1] - J[r1, c0] + J[r0, c0]


def haar(I, r, c, h):
    """-> (right half minus left half, lower half minus upper half) of the h x h box whose top-left is (r - h/2, c - h/2), split at (r, c)"""
    r0, c0 = r - h // 2, c - h // 2
    r1, c1 = r0 + h, c0 + h
    return box(I, r0, c, r1, c1) - box(I, r0, c0, r1, c), box(I, r, c0, r1, c1) - box(I, r0, c0, r, c1)


# ---- 2. fast-Hessian layers ------------------------------------------------------------------------------------------------------------
def layer_size(o, l):
    return (9 + 6 * l) << o


def layer_fits(W, H, o, l):
    return layer_size(o, l) < min(W, H)


def map_dims(W, H, o):
    return H >> o, W >> o          # rows, columns of octave o's maps: a sample every 1 << o pixels


def layer_map(I, o, l):
    """-> (det f64 [mh][mw], laplacian u8 [mh][mw]) of layer l of octave o; a layer that does not fit is all zero"""
    J = I.astype(np.int64)
    H, W = I.shape[0] - 1, I.shape[1] - 1
    mh, mw = map_dims(W, H, o)
    if not layer_fits(W, H, o, l):
        return np.zeros((mh, mw)), np.zeros((mh, mw), np.uint8)
    L = layer_size(o, l)
    lb, b = L // 3, L // 2
    r = (np.arange(mh, dtype=np.int64) << o)[:, None]
    c = (np.arange(mw, dtype=np.int64) << o)[None, :]
    # the filter is the L x L window with top-left (r - L/2, c - L/2), cut into 3 x 3 squares of lb: Dxx is the middle row of squares with
    # the middle one counted -2, Dyy the middle column; Dxy the four lb x lb squares about the window's centre (a gap of one pixel when
    # L is odd).  An even window is centred half a pixel up-left of its sample: detect() reports the centre.
    r0, c0, e = r - b, c - b, L - b
    Dxx = box(J, r0 + lb, c0, r0 + 2 * lb, c0 + L) - 3 * box(J, r0 + lb, c0 + lb, r0 + 2 * lb, c0 + 2 * lb)
    Dyy = box(J, r0, c0 + lb, r0 + L, c0 + 2 * lb) - 3 * box(J, r0 + lb, c0 + lb, r0 + 2 * lb, c0 + 2 * lb)
    Dxy = (box(J, r0 + b - lb, c0 + b - lb, r0 + b, c0 + b) + box(J, r0 + e, c0 + e, r0 + e + lb, c0 + e + lb)
           - box(J, r0 + b - lb, c0 + e, r0 + b, c0 + e + lb) - box(J, r0 + e, c0 + b - lb, r0 + e + lb, c0 + b))
    area = float(L * L)
    dx, dy, dxy = Dxx / area, Dyy / area, Dxy / area
    det = (dx * dy) - ((0.81 * dxy) * dxy)
    return det, ((dx + dy) > 0.0).astype(np.uint8)


def layer_maps(I, n_octaves=4, n_layers=2):
    return [[layer_map(I, o, l) for l in range(n_layers + 2)] for o in range(n_octaves)]


# ---- 3. maxima -------------------------------------------------------------------------------------------------------------------------
def newton(N0, N1, N2, i, j):
    """the 3 x 3 Newton step about sample (i, j) of the middle layer N1 as an explicit adjugate solve -> (x0, x1, x2, det) or None when
    the determinant is 0.  Python floats: the same scalar expressions as the kernel."""
    v = float(N1[i, j])
    g0 = (float(N1[i, j + 1]) - float(N1[i, j - 1])) * 0.5
    g1 = (float(N1[i + 1, j]) - float(N1[i - 1, j])) * 0.5
    g2 = (float(N2[i, j]) - float(N0[i, j])) * 0.5
    a = (float(N1[i, j + 1]) + float(N1[i, j - 1])) - 2.0 * v
    d = (float(N1[i + 1, j]) + float(N1[i - 1, j])) - 2.0 * v
    f = (float(N2[i, j]) + float(N0[i, j])) - 2.0 * v
    b = ((float(N1[i + 1, j + 1]) - float(N1[i + 1, j - 1])) - (float(N1[i - 1, j + 1]) - float(N1[i - 1, j - 1]))) * 0.25
    c = ((float(N2[i, j + 1]) - float(N2[i, j - 1])) - (float(N0[i, j + 1]) - float(N0[i, j - 1]))) * 0.25
    e = ((float(N2[i + 1, j]) - float(N2[i - 1, j])) - (float(N0[i + 1, j]) - float(N0[i - 1, j]))) * 0.25
    c00, c01, c02 = (d * f) - (e * e), (c * e) - (b * f), (b * e) - (c * d)
    c11, c12, c22 = (a * f) - (c * c), (b * c) - (a * e), (a * d) - (b * b)
    det = ((a * c00) + (b * c01)) + (c * c02)
    if det == 0.0 or det != det:
        return None
    x0 = -(((c00 * g0) + (c01 * g1)) + (c02 * g2)) / det
    x1 = -(((c01 * g0) + (c11 * g1)) + (c12 * g2)) / det
    x2 = -(((c02 * g0) + (c12 * g1)) + (c22 * g2)) / det
    return x0, x1, x2, det


def detect(I, threshold, n_octaves=4, n_layers=2, maps=None, info=None):
    """-> the key points of one image in ascending (octave, layer, row, column): dict of arrays x, y, size, s, response, laplacian, octave,
    layer, cell [n][2] (row, column of the sample).  info (a dict, optional) collects what the cover conditions look at."""
    H, W = I.shape[0] - 1, I.shape[1] - 1
    maps = layer_maps(I, n_octaves, n_layers) if maps is None else maps
    out = {k: [] for k in ("x", "y", "size", "s", "response", "laplacian", "octave", "layer", "cell")}
    dets, offs = [], []
    for o in range(n_octaves):
        mh, mw = map_dims(W, H, o)
        for m in range(1, n_layers + 1):
            if not layer_fits(W, H, o, m + 1):
                continue
            N0, N1, N2 = maps[o][m - 1][0], maps[o][m][0], maps[o][m + 1][0]
            mg = (layer_size(o, m + 1) // 2 >> o) + 1
            if mh - 2 * mg <= 0 or mw - 2 * mg <= 0:
                continue
            ctr = N1[mg:mh - mg, mg:mw - mg]
            keep = ctr > threshold
            dets.append(ctr.ravel())
            for N in (N0, N1, N2):
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        if N is N1 and di == 0 and dj == 0:
                            continue
                        keep &= ctr > N[mg + di:mh - mg + di, mg + dj:mw - mg + dj]
            for i, j in zip(*np.nonzero(keep)):
                i, j = int(i) + mg, int(j) + mg
                st = newton(N0, N1, N2, i, j)
                if st is None:
                    continue
                x0, x1, x2, _ = st
                offs += [x0, x1, x2]
                if not (abs(x0) <= 1.0 and abs(x1) <= 1.0 and abs(x2) <= 1.0):
                    continue
                size = layer_size(o, m) + x2 * float(6 << o)
                half = 0.5 if o > 0 else 0.0          # the centre of an even window
                out["x"].append((j + x0) * float(1 << o) - half), out["y"].append((i + x1) * float(1 << o) - half)
                out["size"].append(size), out["s"].append((1.2 * size) / 9.0), out["response"].append(float(N1[i, j]))
                out["laplacian"].append(int(maps[o][m][1][i, j])), out["octave"].append(o), out["layer"].append(m), out["cell"].append((i, j))
    if info is not None:
        info["det"] = np.concatenate(dets) if dets else np.zeros(0)
        info["offsets"] = np.array(offs)
    res = {k: np.array(v, dtype=np.float64) for k, v in out.items() if k in ("x", "y", "size", "s", "response")}
    res["laplacian"] = np.array(out["laplacian"], dtype=np.uint8)
    res["octave"], res["layer"] = np.array(out["octave"], dtype=np.int32), np.array(out["layer"], dtype=np.int32)
    res["cell"] = np.array(out["cell"], dtype=np.int32).reshape(-1, 2)
    return res


# ---- 5. orientation --------------------------------------------------------------------------------------------------------------------
def rnd(v):
    """to the nearest pixel: floor(v + 0.5)"""
    return np.floor(np.asarray(v, dtype=np.float64) + 0.5).astype(np.int64)


def serial_sum(v):
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1]) if len(v) else 0.0


def orientation(I, x, y, s, weights=ORI_WEIGHT, info=None):
    """-> the angle of one key point: Haar responses of size 4 s at the 109 grid points, weighted, 72 windows of 60 degrees every 5
    degrees, window w from (w + 0.5) 5 degrees on (integer Haar responses put many sample angles EXACTLY on multiples of 45 degrees: no
    window edge lies there); a window's sums run in sample order over its members; a sample whose two responses are zero takes no part"""
    J = I if I.dtype == np.int64 else I.astype(np.int64)
    gi = np.array([g[0] for g in ORI_GRID], dtype=np.float64)
    gj = np.array([g[1] for g in ORI_GRID], dtype=np.float64)
    fx, fy = x + gi * s, y + gj * s
    px, py = rnd(fx), rnd(fy)
    h = max(2, int(rnd(4.0 * s)))
    hx, hy = haar(J, py, px, h)
    w = np.asarray(weights, dtype=np.float64)
    rx, ry = w * hx, w * hy
    live = (rx != 0.0) | (ry != 0.0)
    ang = np.array([math.atan2(b, a) for a, b in zip(rx, ry)])
    ang = np.where(ang < 0.0, ang + TWO_PI, ang)
    scores, sums, edge = [], [], np.inf
    for wdx in range(N_WINDOWS):
        d = ang - (wdx + 0.5) * WINDOW_STEP
        d = np.where(d < 0.0, d + TWO_PI, d)
        member = live & (d < WINDOW_WIDTH)
        if live.any():
            dl = d[live]
            edge = min(edge, float(np.min(np.minimum(np.minimum(dl, np.abs(dl - WINDOW_WIDTH)), TWO_PI - dl))))
        sx, sy = serial_sum(rx[member]), serial_sum(ry[member])
        scores.append((sx * sx) + (sy * sy)), sums.append((sx, sy))
    best = int(np.argmax(scores))                  # the lowest index of equals
    best_score, (bx, by) = scores[best], sums[best]
    # neighbouring windows often hold the SAME samples and then the same bits: the runner-up is the best window that differs
    second = max([sc for sc in scores if sc < best_score], default=0.0)
    if info is not None:
        info.setdefault("ori_half", []).append(float(np.min(np.abs(np.concatenate([fx, fy]) + 0.5 - np.round(np.concatenate([fx, fy]) + 0.5)))))
        info.setdefault("ori_half", []).append(abs((4.0 * s + 0.5) - round(4.0 * s + 0.5)))
        info.setdefault("ori_edge", []).append(edge)
        info.setdefault("ori_lead", []).append((best_score, second))
    return math.atan2(by, bx)


# ---- 6. descriptor ---------------------------------------------------------------------------------------------------------------------
def descriptor(I, x, y, s, angle, dim=64, upright=False, shape="kernel", weights=DESC_WEIGHT, info=None, as_f64=False):
    """-> (f32 [dim], norm).  shape "kernel": a subregion's 25 samples t = 0..24 (t = 5 (b % 5) + a % 5) go to four partial sums q = t % 4,
    each serial in t, combined as (p0 + p1) + (p2 + p3); "serial": one sum in t order."""
    J = I if I.dtype == np.int64 else I.astype(np.int64)
    co, si = (1.0, 0.0) if upright else (math.cos(angle), math.sin(angle))
    a = np.tile(np.arange(20), 20)
    b = np.repeat(np.arange(20), 20)
    u, v = a - 9.5, b - 9.5
    fx = x + ((u * co) - (v * si)) * s
    fy = y + ((u * si) + (v * co)) * s
    px, py = rnd(fx), rnd(fy)
    h = max(2, int(rnd(2.0 * s)))
    hx, hy = haar(J, py, px, h)
    g = np.asarray(weights, dtype=np.float64)
    rx, ry = g * hx, g * hy
    tdx = (co * rx) + (si * ry)
    tdy = (co * ry) - (si * rx)
    if info is not None:
        f = np.concatenate([fx, fy])
        info.setdefault("desc_half", []).append(float(np.min(np.abs(f + 0.5 - np.round(f + 0.5)))))
        info.setdefault("desc_half", []).append(abs((2.0 * s + 0.5) - round(2.0 * s + 0.5)))
    if dim == 64:
        comps = [tdx, tdy, np.abs(tdx), np.abs(tdy)]
    else:
        z = np.zeros_like(tdx)
        comps = [np.where(tdy < 0.0, tdx, z), np.where(tdy < 0.0, z, tdx), np.where(tdy < 0.0, np.abs(tdx), z), np.where(tdy < 0.0, z, np.abs(tdx)),
                 np.where(tdx < 0.0, tdy, z), np.where(tdx < 0.0, z, tdy), np.where(tdx < 0.0, np.abs(tdy), z), np.where(tdx < 0.0, z, np.abs(tdy))]
    nc = len(comps)
    sub = (b // 5) * 4 + a // 5
    t = 5 * (b % 5) + a % 5
    vec = np.zeros(dim)
    for sr in range(16):
        idx = np.nonzero(sub == sr)[0]
        idx = idx[np.argsort(t[idx])]
        for k, cmp_ in enumerate(comps):
            vals = cmp_[idx]
            if shape == "serial":
                vec[sr * nc + k] = serial_sum(vals)
            else:
                p = [serial_sum(vals[q::4]) for q in range(4)]
                vec[sr * nc + k] = (p[0] + p[1]) + (p[2] + p[3])
    norm = math.sqrt(serial_sum(vec * vec))
    if norm == 0.0 or norm != norm:
        return np.zeros(dim, np.float32), 0.0
    return (vec / norm) if as_f64 else (vec / norm).astype(np.float32), norm


# ---- the whole stage -------------------------------------------------------------------------------------------------------------------
def run(img, threshold, n_octaves=4, n_layers=2, dim=64, upright=False, max_pts=None, shape="kernel", info=None):
    """-> dict: the key-point arrays of detect() (first max_pts of them), pts [n][2], angle, desc f32 [n][dim], count, overflow.  A key
    point whose descriptor has zero norm keeps its row with NaN coordinates."""
    I = integral(img)
    kp = detect(I, threshold, n_octaves, n_layers, info=info)
    total = len(kp["x"])
    n = total if max_pts is None else min(total, max_pts)
    kp = {k: v[:n] for k, v in kp.items()}
    J = I.astype(np.int64)
    ang, desc = np.zeros(n), np.zeros((n, dim), np.float32)
    pts = np.stack([kp["x"], kp["y"]], axis=1).reshape(-1, 2)
    for k in range(n):
        x, y, s = float(kp["x"][k]), float(kp["y"][k]), float(kp["s"][k])
        ang[k] = 0.0 if upright else orientation(J, x, y, s, info=info)
        desc[k], norm = descriptor(J, x, y, s, ang[k], dim, upright, shape, info=info)
        if norm == 0.0:
            pts[k] = np.nan
    kp.update(pts=pts, angle=ang, desc=desc, count=n, overflow=total - n, integral=I)
    return kp
