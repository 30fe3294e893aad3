"""Planted inputs of the SURF tests and their COVER CONDITIONS, asserted on the numpy restatement alone (tests/surf_ref.py):
a scene is only used where the restatement's decisions sit far from every edge at which an ulp of atan2 / cos / sin could flip them.
TEST INFRASTRUCTURE; never calls the library."""
import functools

import numpy as np

from tests import surf_ref as R

SIGMAS = (1.6, 2.4, 3.5, 5.0, 7.0)
THRESHOLD = 100.0
COVER = 1.0e-9
# the committed seeds: the first of 0, 1, 2, ... at which every cover condition holds (scene() asserts them again on every use)
SEEDS = {(320, 240): 0, (160, 120): 0, (161, 123): 0, (96, 64): 0}


def texture(W, H, seed, px_per_blob=250.0):
    """a sum of Gaussian blobs on 128: sigma from SIGMAS, amplitude +-70..120, one blob per px_per_blob px^2, rounded to u8"""
    rng = np.random.default_rng(seed)
    n = int(round(W * H / px_per_blob))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W), 128.0)
    for _ in range(n):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        sg = SIGMAS[int(rng.integers(len(SIGMAS)))]
        amp = rng.uniform(70.0, 120.0) * (1.0 if rng.random() < 0.5 else -1.0)
        img += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sg * sg))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def blob(W, H, cx, cy, sigma, amp=100.0):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.clip(np.rint(128.0 + amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma * sigma))), 0, 255).astype(np.uint8)


def cover_failures(info, threshold, oriented=True):
    """the cover conditions over what a run of the restatement collected -> list of failures (empty: the scene is usable)"""
    bad = []
    det, off = info["det"], info["offsets"]
    if len(det) and np.min(np.abs(det - threshold)) <= COVER * threshold:
        bad.append("a det within 1e-9 relative of the threshold")
    if len(off) and np.min(np.abs(np.abs(off) - 1.0)) <= COVER:
        bad.append("a Newton offset within 1e-9 of +-1")
    for key in ("ori_half", "desc_half") if oriented else ("desc_half",):
        if key in info and min(info[key]) <= COVER:
            bad.append(f"{key}: a sample coordinate within 1e-9 px of a half-integer")
    if oriented:
        if "ori_edge" in info and min(info["ori_edge"]) <= COVER:
            bad.append("a sample angle within 1e-9 rad of a window edge")
        for best, second in info.get("ori_lead", []):
            if not best - second > COVER * best:
                bad.append("the best window does not lead the second by 1e-9 relative")
                break
    return bad


@functools.lru_cache(maxsize=None)
def scene(W=320, H=240, dim=64, upright=False, seed=None, max_pts=None, shift=None):
    """-> (img u8 [H][W], the restatement's run of it).  shift = (dx, dy): the texture is drawn on a larger canvas and this view of it is
    displaced by that many pixels (scene(shift=None) and scene(shift=(dx, dy)) see the same blobs)."""
    seed = SEEDS[(W, H)] if seed is None else seed
    big = texture(W + 64, H + 64, seed)
    dx, dy = shift or (0, 0)
    assert 0 <= dx <= 64 and 0 <= dy <= 64
    img = np.ascontiguousarray(big[dy:dy + H, dx:dx + W])
    info = {}
    ref = R.run(img, THRESHOLD, dim=dim, upright=upright, max_pts=max_pts, info=info)
    bad = cover_failures(info, THRESHOLD, oriented=not upright)
    assert not bad, (W, H, seed, bad)
    ref["info"] = info
    return img, ref


def find_seed(W, H, tries=20):
    """the first seed at which the oriented and the upright scene, 64 and 128, meet their cover conditions"""
    for seed in range(tries):
        try:
            for dim in (64, 128):
                for upright in (False, True):
                    scene.__wrapped__(W, H, dim, upright, seed)
            return seed
        except AssertionError:
            continue
    raise AssertionError("no seed found")


# ---- the two-view scenes of tests/test_surf_e2e_gpu.py ---------------------------------------------------------------------------------
E2E_W, E2E_H, E2E_SHIFT = 320, 240, (24, 8)


def K300(W=E2E_W, H=E2E_H):
    return np.array([[300.0, 0.0, W / 2.0], [0.0, 300.0, H / 2.0], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def shifted_pair():
    """image 2 is image 1 shifted by E2E_SHIFT: a point at (x, y) of image 1 is at (x - 24, y - 8) of image 2.  Asserts, on the
    restatements alone, >= 28 matches (the reference's gate of 25 plus 3) of which >= 90 % lie within 1.5 px of the shift."""
    from tests import mergefront_ref as MF

    (img1, r1), (img2, r2) = scene(E2E_W, E2E_H), scene(E2E_W, E2E_H, shift=E2E_SHIFT)
    m = MF.match_surf(r1["pts"], r1["desc"], r2["pts"], r2["desc"], 0.8, 0.6)
    mt = m["matches"]
    assert len(mt) >= 28, len(mt)
    d = (r1["pts"][mt[:, 0]] - r2["pts"][mt[:, 1]]) - np.array(E2E_SHIFT, dtype=np.float64)
    good = np.hypot(d[:, 0], d[:, 1]) < 1.5
    assert good.mean() >= 0.9, good.mean()
    return (img1, r1), (img2, r2), m


# ---- the descriptor tolerance study --------------------------------------------------------------------------------------
F32_FLOOR = 2.4e-7          # two f32 ulps of 1: the descriptor is stored as f32 and a component rounds once on either side


@functools.lru_cache(maxsize=None)
def descriptor_study(dim=64):
    """Over every key point of the 320 x 240 scene: the largest change of a descriptor component (before the f32 store) when the
    restatement's angle moves by +-1e-12 rad and its weights by 1 ulp -- what an ulp of the device's atan2 / cos / sin / exp may do, with
    four decades of room -- and the largest difference between the serial and the kernel-shaped summation.
    -> dict(d, shape, tol): the GPU tolerance is max(100 d, F32_FLOOR)."""
    _img, ref = scene(E2E_W, E2E_H, dim=dim)
    J = ref["integral"].astype(np.int64)
    w = np.asarray(R.DESC_WEIGHT)
    d = shape = 0.0
    for k in range(ref["count"]):
        x, y, s, a = float(ref["x"][k]), float(ref["y"][k]), float(ref["s"][k]), float(ref["angle"][k])
        base = R.descriptor(J, x, y, s, a, dim)[0].astype(np.float64)
        for da, ww in ((1e-12, w), (-1e-12, w), (0.0, np.nextafter(w, 2.0)), (0.0, np.nextafter(w, 0.0))):
            d = max(d, float(np.max(np.abs(_exact(J, x, y, s, a + da, dim, ww) - _exact(J, x, y, s, a, dim, w)))))
        shape = max(shape, float(np.max(np.abs(R.descriptor(J, x, y, s, a, dim, shape="serial")[0].astype(np.float64) - base))))
    return dict(d=d, shape=shape, tol=max(100.0 * d, F32_FLOOR))


def _exact(J, x, y, s, a, dim, w):
    """the descriptor in f64, before the f32 store: perturbations far below an f32 ulp stay visible"""
    vec, norm = R.descriptor(J, x, y, s, a, dim, weights=w, as_f64=True)
    return vec


# ---- a non-planar two-view pair: depth bands under a sideways translation ------------------------------------------------------------
BAND_DISPARITY = (8, 20, 36, 14)  # px, one per vertical band of image 2 (left to right): fronto-parallel depths.  With the three bands
# 8 / 20 / 36 alone the restatements' E leaves a true correspondence at 2.17 px (the bound is 2): a fourth band was added, as foreseen
N_RANSAC = 1000                   # the front's own study: 1000 hypotheses with the refit


def checked_run(img, dim=64):
    """the restatement's run of an image with its cover conditions asserted"""
    info = {}
    ref = R.run(img, THRESHOLD, dim=dim, info=info)
    bad = cover_failures(info, THRESHOLD)
    assert not bad, bad
    return ref


@functools.lru_cache(maxsize=None)
def banded_pair():
    """image 1 is a view of the texture; column x of image 2 shows column x + disparity(band of x) of image 1: a camera moved sideways in
    front of four depth bands.  -> (img1, ref1, img2, ref2, the restatement front's job).  Asserts ON THE TWO RESTATEMENTS ALONE:
    emat_ok = 1, inlier_num >= 18, and the recovered E maps the true correspondences (a grid of points of every band) to under 2 px of
    epipolar error."""
    from tests import mergefront_ref as MF

    W, H = E2E_W, E2E_H
    big = texture(W + 64, H + 64, SEEDS[(W, H)])
    img1 = np.ascontiguousarray(big[:H, :W])
    img2 = np.zeros_like(img1)
    edges = [k * W // len(BAND_DISPARITY) for k in range(len(BAND_DISPARITY) + 1)]
    for b, d in enumerate(BAND_DISPARITY):
        img2[:, edges[b]:edges[b + 1]] = big[:H, edges[b] + d:edges[b + 1] + d]
    r1, r2 = checked_run(img1), checked_run(img2)
    K = K300().reshape(9)
    job = MF.front_job(dict(pts=r1["pts"], desc=r1["desc"], K=K), dict(pts=r2["pts"], desc=r2["desc"], K=K), n_ransac=N_RANSAC)
    assert job["emat_ok"] == 1 and job["inlier_num"] >= 18, (job["surf_num"], job["emat_ok"], job["inlier_num"])
    iK = np.linalg.inv(K.reshape(3, 3))
    rows = [(x + d, y, x, y) for b, d in enumerate(BAND_DISPARITY) for x in range(edges[b] + 10, edges[b + 1] - 10, 15) if x + d < W
            for y in range(10, H, 20)]
    err = MF.epi_err(MF.fmat(iK, iK, job["E"]), np.array(rows, dtype=np.float64))
    assert err.max() < 2.0, err.max()
    job["true_err"] = float(err.max())
    return img1, r1, img2, r2, job
