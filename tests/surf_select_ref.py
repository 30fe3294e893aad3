"""The strongest-first choice of the SURF stage (CS_SURF_KEEP_STRONGEST) restated over tests/surf_ref.py's uncapped detect():
of more than max_pts maxima the max_pts with the largest response stay (f64 values; equals at the cut: the earlier in the list), in
ascending list order.  Orientation and descriptors are surf_ref's, for the kept rows only.  TEST INFRASTRUCTURE; never calls the library."""
import numpy as np

from tests import surf_ref as R


def select(response, max_pts):
    """-> the ascending list indices of the rows kept.  Written as the definition: a row stays when fewer than max_pts rows beat it, and
    row b beats row a when it is stronger, or as strong and earlier."""
    r = np.asarray(response, dtype=np.float64)
    n = len(r)
    if n <= max_pts:
        return np.arange(n)
    idx = np.arange(n)
    beats = (r[None, :] > r[:, None]) | ((r[None, :] == r[:, None]) & (idx[None, :] < idx[:, None]))   # [a][b]: b beats a
    return np.nonzero(beats.sum(axis=1) < max_pts)[0]


def run(img, threshold, max_pts, n_octaves=4, n_layers=2, dim=64, upright=False, info=None):
    """surf_ref.run with the strongest-first choice -> the same dict, plus total (the maxima before the choice) and kept (list indices)"""
    I = R.integral(img)
    kp = R.detect(I, threshold, n_octaves, n_layers, info=info)
    total = len(kp["x"])
    kept = select(kp["response"], max_pts)
    n = len(kept)
    kp = {k: v[kept] for k, v in kp.items()}
    J = I.astype(np.int64)
    ang, desc = np.zeros(n), np.zeros((n, dim), np.float32)
    pts = np.stack([kp["x"], kp["y"]], axis=1).reshape(-1, 2)
    for k in range(n):
        x, y, s = float(kp["x"][k]), float(kp["y"][k]), float(kp["s"][k])
        ang[k] = 0.0 if upright else R.orientation(J, x, y, s, info=info)
        desc[k], norm = R.descriptor(J, x, y, s, ang[k], dim, upright, info=info)
        if norm == 0.0:
            pts[k] = np.nan
    kp.update(pts=pts, angle=ang, desc=desc, count=n, overflow=total - n, total=total, kept=kept, integral=I)
    return kp


def tie_image(W=96, H=64):
    """two identical blobs 32 px apart on a flat background (their windows see the same pixels: one response, bit for bit), and two
    other blobs, one stronger and one weaker, later in the list -> u8 image."""
    from tests import surf_scenes as S

    img = np.full((H, W), 128, np.int32)
    for cx, cy, amp in ((24, 20, 100.0), (56, 20, 100.0), (40, 44, 120.0), (76, 44, 90.0)):
        img += S.blob(W, H, cx, cy, 2.4, amp).astype(np.int32) - 128
    return np.clip(img, 0, 255).astype(np.uint8)
