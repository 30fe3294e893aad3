"""Problems of the intra-camera pose solve that the CPU precondition (tests/test_pose_cases_cpu.py) and the GPU tests
(tests/test_pose_batch_gpu.py, tests/test_pose_ba_gpu.py, tests/test_handback_gpu.py) share: one builder and ONE committed list of cases.

A case is a dict of the builder's arguments.  The precondition runs over ALL_CASES: the oracle must agree with itself on every case
when the points are handed over in reversed order, which bounds what the order of the sum over points alone can do to it.  A case that
misses that bound gets another seed here; the bound stays."""
import functools

import numpy as np

from coslam_amd.synth import Scene, rodrigues

TAU = 10.0
W, H = 640, 480


@functools.lru_cache(maxsize=8)
def _scene(seed, n_points):
    return Scene(1, W, H, n_points, seed=seed)


def scene_points_for(npts):
    """points in the scene: about 95 % of them are visible from the path's first frames"""
    return 3000 if npts <= 2500 else int(1.2 * npts) + 200


def pose_problem(seed, npts=192, noise=0.5, n_out=10, frame=3, K=None, rot=0.01, trans=0.03, exact=True):
    """-> K, R0, t0, Ms, ms, R, t: npts correspondences of a synthetic camera (pixel noise, n_out gross outliers), started
    rot rad / trans units away from the true pose (R, t).  K: the calibration to project with (None = the scene's).
    exact: the scene must yield the requested count."""
    rng = np.random.default_rng(seed)
    sc = _scene(100 + seed, scene_points_for(npts))
    K = sc.K if K is None else np.asarray(K, dtype=np.float64)
    R, t = sc.pose(0, frame)
    X = sc.points @ R.T + t
    z = X[:, 2]
    uv = (X @ K.T)[:, :2] / z[:, None]
    vis = (z > 0.1) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)
    idx = np.nonzero(vis)[0][:npts]
    Ms = np.ascontiguousarray(sc.points[idx])
    assert len(Ms) == npts or not exact, (seed, npts, len(Ms))
    ms = uv[idx] + noise * rng.standard_normal((len(idx), 2))
    ms[:n_out] += 30 * rng.standard_normal((n_out, 2))
    R0 = R @ rodrigues(rot * rng.standard_normal(3))
    t0 = t + trans * rng.standard_normal(3)
    return K.copy(), R0, t0, Ms, np.ascontiguousarray(ms), R, t


def calib(j):
    """the j-th calibration: focal length, skew-free, principal point -- all different from problem to problem"""
    f = 0.82 * W * (1.0 + 0.04 * ((j * 3) % 7 - 3))
    return np.array([[f, 0, W / 2.0 + 9.0 * ((j * 5) % 9 - 4)], [0, f * (1.0 + 0.01 * (j % 3)), H / 2.0 - 7.0 * ((j * 2) % 7 - 3)], [0, 0, 1.0]])


def case(npts, j=None, seed=None, **kw):
    """npts points, the j-th calibration (None: the scene's own), seed 11 + npts unless given"""
    c = dict(seed=11 + npts if seed is None else seed, npts=npts, n_out=min(10, npts // 4))
    if j is not None:
        c["K"] = calib(j)
    c.update(kw)
    return c


def build(c):
    return pose_problem(**c)


def _batch(counts, seeds=None):
    seeds = seeds or {}
    return [case(n, j, seed=seeds.get(j)) for j, n in enumerate(counts)]


# ---- the batches of cs_pose_intracam_batch_dev: name -> (ptsStride, cases) ------------------------------------------------------
_rng16 = np.random.default_rng(1616)
BATCHES = {
    "loop192": (192, _batch([170, 0, 1, 5, 63, 64, 65, 192])),           # the loops' shape
    "wave64": (64, _batch([64, 7, 33, 0, 1])),                           # the one-wave template with blockIdx > 0
    "stride65": (65, _batch([65, 3])),
    "trips600": (600, _batch([255, 256, 257, 600, 513])),                # second and third trips of the 256-thread pass
    "lds4096": (4096, _batch([4096, 4095])),                             # the largest stride the entry accepts
    "sixteen": (192, _batch([int(n) for n in _rng16.integers(100, 193, 16)], seeds={j: 700 + j for j in range(16)})),
}
# one option record per problem: (field, value) pairs on top of the defaults
OPTION_BATCH = (192, _batch([170, 150, 130, 192, 66], seeds={0: 800, 1: 813, 2: 802, 3: 803, 4: 804}),   # (seed 801 at one round: 3.8e-9 / 3.8e-8 against itself)
                [(), (("maxIterRW", 1),), (("maxIterLM", 1),), (("lambda0", 1.0),), (("maxIterRW", 0),)])
# a far start the solve still converges from: rotation about 0.9 rad, t off by several units
FAR_START = case(180, 3, seed=924, rot=0.52, trans=2.0, n_out=0, noise=0.3)      # 0.90 rad, |t0 - t| = 4.0
# the failing solve: FAIL_AT's measurement is not-a-number (set by failing()), its neighbours are valid
FAIL_CASE, FAIL_AT = case(120, 2, seed=902), 57
FAILURE_BATCH = (192, [case(100, 0, seed=903), FAIL_CASE, FAR_START, case(64, 4, seed=904)])
FAILURE_INDEX, FAR_INDEX = 1, 2
# the host-pointer entry cs_pose_intracam: one problem per call, ptsStride == npts
HOST_CASES = ([case(n) for n in (0, 65, 256, 257, 4096, 4097)] + [case(5000, seed=5), case(6000, seed=6), case(100, seed=7, n_out=10)] +
              [case(192, seed=0), case(192, seed=1), case(64, seed=2), case(7, seed=3), case(1000, seed=4)])

# (the problems of the hand-back chain at the end of this file come out of oracle.handback: chain_by_oracle())
ALL_CASES = [c for _, cs in BATCHES.values() for c in cs] + OPTION_BATCH[1] + FAILURE_BATCH[1] + HOST_CASES


def failing(K, R0, t0, Ms, ms, *rest):
    """the problem with one measurement replaced by not-a-number"""
    ms = ms.copy()
    ms[FAIL_AT, 0] = np.nan
    return (K, R0, t0, Ms, ms) + tuple(rest)


def prev_errors(batch_cases, all_out):
    """previous reprojection errors per problem (a list of float64[npts]): half-normal, scale 6 px, so that some points start with
    weight 0 (>= TAU); problem `all_out` has every error >= TAU: every weight 0 in the first round"""
    rng = np.random.default_rng(4242)
    out = []
    for j, c in enumerate(batch_cases):
        e = np.abs(rng.standard_normal(c["npts"])) * 6
        if j == all_out:
            e = TAU + np.abs(rng.standard_normal(c["npts"])) * 6
            e[::3] = TAU          # exactly tau is out as well (e >= tau)
        out.append(e)
    return out


# ---- the chain hand-back -> batched solve (tests/test_handback_gpu.py): three cameras over four frames -------------------------------
CHAIN = dict(n_cams=3, n_frames=4, N=600, stride=192, nColBlk=16, nRowBlk=12, seed=77)


def chain_scene():
    """Tracker output of CHAIN's cameras looking at one synthetic scene: slot i of every camera follows scene point i (map point i once
    the map is initialised behind frame 0), 0.3 px noise.  -> dict(K [c], points, feats[f][c] (the tracker's records), pose[f][c] = (R, t))"""
    from coslam_amd import KLT_TrackedFeature

    n_cams, n_frames, N = CHAIN["n_cams"], CHAIN["n_frames"], CHAIN["N"]
    sc = Scene(n_cams, W, H, N, seed=CHAIN["seed"])
    rng = np.random.default_rng(CHAIN["seed"])
    Ks = [calib(c) for c in range(n_cams)]
    feats, pose = [], []
    seen = np.zeros((n_cams, N), bool)
    for f in range(n_frames):
        feats.append([])
        pose.append([sc.pose(c, f) for c in range(n_cams)])
        for c in range(n_cams):
            R, t = pose[f][c]
            X = sc.points @ R.T + t
            uv = (X @ Ks[c].T)[:, :2] / X[:, 2:3] + 0.3 * rng.standard_normal((N, 2))
            vis = (uv[:, 0] >= 2) & (uv[:, 0] < W - 2) & (uv[:, 1] >= 2) & (uv[:, 1] < H - 2)
            rec = np.zeros(N, dtype=KLT_TrackedFeature)
            rec["status"] = np.where(vis, np.where(seen[c], 0, 1), -1)
            rec["pos"] = (uv / [W, H]).astype(np.float32)
            rec["gain"], rec["fed"] = 1.0, -1
            seen[c] = vis
            feats[f].append(rec)
    return dict(K=Ks, points=sc.points.copy(), feats=feats, pose=pose)


def chain_by_oracle(scene=None):
    """oracle.handback of every camera and frame, with the map initialised behind frame 0 (slot i -> map point i for every live slot)
    -> (scene, out[f][c] = dict(hb = the hand-back's result, state copies s2m / tl / xy, problem = (K, R0, t0, Ms, ms) with the previous
    frame's true pose as the start; None for frame 0))"""
    import oracle

    S = scene or chain_scene()
    n_cams, N = CHAIN["n_cams"], CHAIN["N"]
    st = [dict(s2m=np.full(N, -1, np.int32), tl=np.full(2 * N, -1, np.int32), xy=np.zeros(2 * N)) for _ in range(n_cams)]
    out = []
    for f, recs in enumerate(S["feats"]):
        out.append([])
        for c, rec in enumerate(recs):
            o = st[c]
            if f == 1:
                live = o["tl"][:N] >= 0
                o["s2m"][live] = np.nonzero(live)[0]
            hb = oracle.handback(rec, W, H, S["K"][c], np.zeros(7), S["points"], o["s2m"], o["tl"], o["xy"], 10 + f,
                                 nColBlk=CHAIN["nColBlk"], nRowBlk=CHAIN["nRowBlk"], ptsStride=CHAIN["stride"])
            prob = None if f == 0 else (S["K"][c], S["pose"][f - 1][c][0], S["pose"][f - 1][c][1], hb["Ms"].copy(), hb["ms"].copy())
            out[f].append(dict(hb=hb, s2m=o["s2m"].copy(), tl=o["tl"].copy(), xy=o["xy"].copy(), problem=prob))
    return S, out
