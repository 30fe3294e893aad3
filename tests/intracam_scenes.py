"""Planted scenes of the intra-camera source of new map points (cs_newpts_intracam_dev) beyond one camera and one commit
pass, and their COVER CONDITIONS, asserted on the C oracle alone (oracle.intracam_new_points, which tests/test_oracle_cpu.py holds bit for
bit to the reference's own SingleSLAM::newMapPoints on tests/golden/intracam_newpts_golden.npz).  Plain numpy; never calls the library.
TEST INFRASTRUCTURE.

A scene: nC cameras with their own K, each on a smooth trajectory of T frames (sideways, slowly turning, and turning back after 0.8 of
the frames kept, so that the widest parallax of a long track lies inside it and of a shorter one at its oldest view) in front of its own static
points, N slots per camera, pixels = projections + 0.3 px of noise.  Slots: long unmapped static tracks (the candidates; some span exactly
minTrackLen frames, some are older than the frames fed), tracks one frame too short and shorter, mapped, dynamic, dead slots, features
new in this frame, candidates 30 px off the epipolar line in the oldest view the call uses or in the newest one (both re-projection gates
reject), candidates of points far away (the covariance test) and behind the camera.

The reference's function is per camera (genNewMapPoints calls it camera after camera, src/app/SL_CoSLAM.cpp:1310-1330): the multi-camera
expectation is the oracle called camera by camera, in camera order, over the cameras d_ready admits and the newest `stored` frames."""
import functools

import numpy as np

SIGMA = 10.0        # Const::PIXEL_ERR_VAR
MAX_EPI_ERR = 2.0   # genNewMapPoints' maxEpiErr
MIN_TRACK_LEN = 20  # Param::nMinFeatTrkLen
BASE = 11           # map points the map already holds (slot2map of a mapped slot points into them)
PASS = 1024         # entries of a commit pass (k_intracam_newpts_commit: one workgroup of 1024 threads)
POISON = 1.0e4      # pixels of frames a track does not reach: never read

# name -> cameras, slots per camera, frames the store keeps, frames fed, depth of the walks' centre table
SPECS = {
    "three": dict(nC=3, N=160, store=48, T=40, walk=48),
    "two_pass": dict(nC=8, N=200, store=48, T=40, walk=48),
    "ragged": dict(nC=9, N=115, store=48, T=40, walk=48),
    "sixteen": dict(nC=16, N=129, store=48, T=40, walk=48),
    "wrapped": dict(nC=2, N=96, store=48, T=75, walk=48),
    "deep": dict(nC=2, N=64, store=100, T=100, walk=64),
    "still": dict(nC=3, N=64, store=100, T=100, walk=64),
}
DEEP_WALKS = (2, 3, 64, 65, 1024)
STILL_FROM = 30     # `still`, camera 0: the poses of depths 30 .. 99 (its oldest 70 frames) are bit-identical
# the committed seeds: the first of 0, 1, 2, ... at which every cover condition holds (scene() asserts them again on every use)
SEEDS = {"three": 0, "two_pass": 0, "ragged": 0, "sixteen": 0, "wrapped": 0, "deep": 0, "still": 0}


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th if th > 0 else np.zeros(3)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def build(name, seed):
    """the arrays of a scene, by walk depth (entry 0 = the current frame): K, iK [nC][9]; histR [nC][T][9], histT [nC][T][3],
    histXY [nC][T][2N]; state, slot2map [nC][N], trackSpan [nC][2N], isStatic [nC][N] as they stand at the call"""
    sp = SPECS[name]
    nC, N, T, store = sp["nC"], sp["N"], sp["T"], sp["store"]
    idx = list(SPECS).index(name)
    rng = np.random.default_rng((seed, idx))
    cur = 700 + 13 * idx
    stored = min(T, store)
    step = min(0.045, 1.8 / T)
    K, iK = np.zeros((nC, 9)), np.zeros((nC, 9))
    hR, hT = np.zeros((nC, T, 9)), np.zeros((nC, T, 3))
    hXY = np.full((nC, T, 2 * N), POISON)
    state, s2m = np.full((nC, N), -1, np.int32), np.full((nC, N), -1, np.int32)
    span, fstat = np.full((nC, 2 * N), -1, np.int32), np.ones((nC, N), np.uint8)
    kind = np.zeros((nC, N), np.int32)
    for c in range(nC):
        Kc = np.array([[500 + 14 * c + 5 * rng.random(), 0, 320 + 3 * c], [0, 505 + 11 * c + 5 * rng.random(), 240 - 2 * c], [0, 0, 1]])
        K[c], iK[c] = Kc.reshape(9), np.linalg.inv(Kc).reshape(9)
        org = np.array([0.3 * c, 0.1 * (c % 3), 0.0])
        yaw, ph = 0.2 * c, 6.283 * rng.random(4)
        along = np.array([np.cos(yaw), np.sin(yaw), 0.0])
        still_all = name == "still" and c == 1
        st = 0.045 if name == "still" and c == 0 else step
        for j in range(T):
            jj = 0 if still_all else (min(j, STILL_FROM) if name == "still" and c == 0 else j)
            w = np.array([0.004 * np.sin(0.21 * jj + ph[0]), 0.03 * c + 0.1 * jj / T + 0.002 * np.sin(0.33 * jj + ph[1]), 0.001 * np.sin(0.17 * jj + ph[2])])
            R = _rodrigues(w)
            pos = org - st * jj * (1 - jj / (1.6 * stored)) * along + np.array([0.0, 0.004, 0.006]) * jj * (st / 0.045) + 0.01 * np.sin(0.3 * jj + ph[3]) * np.array([0, 1.0, 0])
            hR[c, j], hT[c, j] = R.reshape(9), -R @ pos
        for k in range(N):
            u = rng.random()
            # 0 dead, 1 new, 2 short, 3 mapped, 4 dynamic, 5 oldest view off, 6 newest view off, 7 far away, 8 behind, 9 fine
            kd = 0 if u < 0.07 else 1 if u < 0.11 else 2 if u < 0.22 else 3 if u < 0.30 else 4 if u < 0.37 else 5 if u < 0.41 else 6 if u < 0.45 \
                else 7 if u < 0.49 else 8 if u < 0.52 else 9
            kind[c, k] = kd
            if kd == 0:
                continue
            if kd == 1:
                Ld = 0
            elif kd == 2:
                Ld = MIN_TRACK_LEN - 1 if rng.random() < 0.4 else 1 + int(rng.random() * (MIN_TRACK_LEN - 1))
            elif name == "still" and rng.random() < 0.7:
                Ld = 94 + int(rng.random() * 12)
            else:   # (up to 8 frames more than were fed: the older nodes have no pose)
                Ld = MIN_TRACK_LEN if rng.random() < 0.1 else MIN_TRACK_LEN + int(rng.random() * (T + 8 - MIN_TRACK_LEN))
            state[c, k] = 1 if kd == 1 else 0
            span[c, k], span[c, N + k] = cur - Ld, cur
            if kd == 3:
                s2m[c, k] = k % BASE
            if kd == 4:
                fstat[c, k] = 0
            X = org + np.array([-2.5 + 5 * rng.random(), -1.5 + 3 * rng.random(), 4 + 8 * rng.random()])
            if kd == 7:
                X[2] = 400 + 300 * rng.random()
            if kd == 8:
                X[2] = -3 - 3 * rng.random()
            n = min(Ld + 1, T)
            Rs, ts = hR[c, :n].reshape(n, 3, 3), hT[c, :n]
            Xc = Rs @ X + ts
            Kc = K[c].reshape(3, 3)
            m = (Xc @ Kc.T)[:, :2] / Xc[:, 2:3] + 0.3 * rng.normal(size=(n, 2))
            if kd == 5:
                m[min(Ld, stored - 1)] += (12.0, 30.0)
            if kd == 6:
                m[0] += (12.0, 30.0)
            hXY[c, :n, k], hXY[c, :n, N + k] = m[:, 0], m[:, 1]
    return dict(name=name, seed=seed, nC=nC, N=N, T=T, store=store, stored=stored, walk=sp["walk"], cur=cur, K=K, iK=iK, histR=hR, histT=hT,
                histXY=hXY, state=state, slot2map=s2m, trackSpan=span, isStatic=fstat, kind=kind)


def frames(S):
    """the records to feed the ring, oldest frame first: (frame, R [nC][9], t [nC][3], xy [nC][2N], state [nC][N]) -- the real pose of
    every frame goes to the call that pushes it; a slot is dead before its track begins"""
    N, cur = S["N"], S["cur"]
    f1 = S["trackSpan"][:, :N]
    for j in range(S["T"] - 1, -1, -1):
        f = cur - j
        st = np.where((f1 >= 0) & (f1 <= f), np.where(f1 == f, 1, 0), -1).astype(np.int32)
        yield f, S["histR"][:, j], S["histT"][:, j], S["histXY"][:, j], (S["state"] if j == 0 else st)


def admitted(S, ready=None, readyMin=1):
    return [c for c in range(S["nC"]) if ready is None or ready[c] >= readyMin]


def candidates(S, c, stored=None):
    """the slots of camera c that pass the prefilter (getUnMappedAndTrackedFeatPts, src/app/SL_SingleSLAM.cpp:159, and the walk's stop at a
    dynamic feature, :938-944) and have an older view with a pose"""
    N = S["N"]
    stored = S["stored"] if stored is None else stored
    st, f1, f2 = S["state"][c], S["trackSpan"][c, :N], S["trackSpan"][c, N:]
    ok = ((st == 0) | (st == 1)) & (f1 >= 0) & (f2 - f1 >= MIN_TRACK_LEN) & (S["slot2map"][c] < 0) & (S["isStatic"][c] != 0)
    return np.nonzero(ok & (np.minimum(f2 - f1, stored - 1) >= 1))[0]


_expect_cache = {}


def expect(S, maxWalk=None, ready=None, readyMin=1, stored=None):
    """what the call must append, in (camera, slot) order: the oracle camera by camera over the newest `stored` frames.
    -> dict(slot, camera, first, M, cov, candidates, per_camera = successes of every camera (0 where not admitted)); shared: leave unchanged"""
    import oracle

    stored = S["stored"] if stored is None else stored
    cams = admitted(S, ready, readyMin)
    key = (S["name"], S["seed"], maxWalk, tuple(cams), stored)
    if key in _expect_cache:
        return _expect_cache[key]
    slot, cam, first, M, cov, per = [], [], [], [], [], np.zeros(S["nC"], np.int64)
    ncand = 0
    for c in cams:
        s, f, m, cv = oracle.intracam_new_points(S["K"][c], S["iK"][c], S["histR"][c, :stored], S["histT"][c, :stored], S["histXY"][c, :stored],
                                                 S["state"][c], S["slot2map"][c], S["trackSpan"][c], S["isStatic"][c], MIN_TRACK_LEN, MAX_EPI_ERR,
                                                 SIGMA, maxWalk=maxWalk)
        slot.append(s), cam.append(np.full(len(s), c, np.int32)), first.append(f), M.append(m), cov.append(cv)
        per[c] = len(s)
        ncand += len(candidates(S, c, stored))
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)   # noqa: E731
    out = dict(slot=cat(slot, (0,), np.int32), camera=cat(cam, (0,), np.int32), first=cat(first, (0,), np.int32), M=cat(M, (0, 3), np.float64),
               cov=cat(cov, (0, 9), np.float64), candidates=ncand, per_camera=per)
    _expect_cache[key] = out
    return out


def per_pass(S, E):
    """the successes in every commit pass: entries e = camera * N + slot in blocks of 1024"""
    n = (S["nC"] * S["N"] + PASS - 1) // PASS
    return np.bincount((E["camera"].astype(np.int64) * S["N"] + E["slot"]) // PASS, minlength=n)


def jp_of(S, E):
    """the depth of the oldest view of every expected point"""
    return S["cur"] - E["first"]


def walk_cosines(S, c, k, M):
    """the cosines refineTriangulation compares for slot k of camera c around the first triangulation M, at the walk depths 1 .. jp, in
    the oracle's expression order (cam_center, cos_between: + * / sqrt only, so binary64 numpy reproduces every value exactly)"""
    N = S["N"]
    jp = min(int(S["trackSpan"][c, N + k] - S["trackSpan"][c, k]), S["stored"] - 1)

    def centre(j):
        R, t = S["histR"][c, j], S["histT"][c, j]
        return [-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]) for i in range(3)]

    C0 = centre(0)
    a = [C0[i] - M[i] for i in range(3)]
    na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    out = np.zeros(jp + 1)
    out[0] = np.inf   # (the feature itself is not a candidate)
    for j in range(1, jp + 1):
        Cj = centre(j)
        b = [Cj[i] - M[i] for i in range(3)]
        d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
        nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
        out[j] = d / np.sqrt(na * nb)
    return out


def still_ties(S):
    """`still`, camera 0: for every expected point, the depths at which the walk's smallest cosine is attained.  The first triangulation
    (what the walk measures its angles around) is the oracle's result under a walk bound of one node, which keeps it.
    -> list of (slot, depths)"""
    E, E1 = expect(S), expect(S, maxWalk=1)
    first_M = {int(s): E1["M"][i] for i, s in enumerate(E1["slot"]) if E1["camera"][i] == 0}
    out = []
    for i in np.nonzero(E["camera"] == 0)[0]:
        k = int(E["slot"][i])
        if k not in first_M:
            continue
        cv = walk_cosines(S, 0, k, first_M[k])
        out.append((k, np.nonzero(cv == cv.min())[0]))
    return out


def cover(S):
    """the cover conditions of a scene, on the oracle alone -> the counts measured (AssertionError where one fails)"""
    name, nC, N = S["name"], S["nC"], S["N"]
    E = expect(S)
    cand = np.array([len(candidates(S, c)) for c in range(nC)])
    succ = E["per_camera"]
    passes = per_pass(S, E)
    out = dict(candidates=cand.tolist(), successes=succ.tolist(), per_pass=passes.tolist(), A=int(len(E["slot"])), a1=int(passes[0]))
    assert E["candidates"] == cand.sum()
    assert np.isfinite(E["M"]).all() and np.isfinite(E["cov"]).all()
    for c in range(nC):
        if name == "still" and c == 1:   # every earlier centre is the current one: nothing to add
            assert cand[c] >= 10 and succ[c] == 0, (name, c, cand[c], succ[c])
        else:
            assert cand[c] > succ[c] >= 5, (name, c, cand[c], succ[c])
    # the refinement matters: points whose widest-parallax view is not the first triangulation's oldest one (a walk bound of one node
    # keeps the first triangulation), next to points where it is
    E1 = expect(S, maxWalk=1)
    first_M = {(int(c), int(k)): E1["M"][i] for i, (c, k) in enumerate(zip(E1["camera"], E1["slot"]))}
    moved = [not np.array_equal(E["M"][i], first_M[(int(c), int(k))]) for i, (c, k) in enumerate(zip(E["camera"], E["slot"])) if (int(c), int(k)) in first_M]
    out["refined_elsewhere"], out["refined_at_oldest"] = int(np.sum(moved)), int(len(moved) - np.sum(moved))
    assert out["refined_elsewhere"] >= 5 and out["refined_at_oldest"] >= 5, (name, out)
    kinds = S["kind"]
    assert all((kinds == q).sum() >= 2 for q in range(10)), "a kind of slot is missing"
    spanlen = S["trackSpan"][:, N:] - S["trackSpan"][:, :N]
    assert ((kinds == 2) & (spanlen == MIN_TRACK_LEN - 1)).any() and ((kinds >= 5) & (spanlen == MIN_TRACK_LEN)).any(), "the length threshold"
    if name in ("two_pass", "ragged", "sixteen"):
        assert len(passes) == {"two_pass": 2, "ragged": 2, "sixteen": 3}[name] and (passes >= 2).all(), (name, passes)
    if name == "ragged":   # pass 2 = the last 11 slots of camera 8
        assert nC * N - PASS == 11
    if name == "two_pass":
        assert out["a1"] >= 3 and out["A"] - out["a1"] >= 3
    if name == "deep":
        jp = jp_of(S, E)
        out["jp_ge_64"] = int((jp >= 64).sum())
        assert out["jp_ge_64"] >= 10 and jp.max() == 99
        Ew = {w: expect(S, maxWalk=w) for w in DEEP_WALKS}
        same = lambda a, b: all(np.array_equal(a[q], b[q]) for q in ("slot", "camera", "first", "M", "cov"))   # noqa: E731
        assert not same(Ew[2], Ew[3]) and not same(Ew[64], Ew[65])
        # 65 and 1024 agree only if no point's walk reaches past depth 64; here points with jp >= 65 exist and the two differ
        out["jp_ge_65"] = int((jp >= 65).sum())
        assert out["jp_ge_65"] >= 1 and not same(Ew[65], Ew[1024])
        assert same(Ew[1024], E)
    if name == "wrapped":
        for c in range(nC):
            ks = candidates(S, c)
            old = (spanlen[c, ks] > S["stored"] - 1).sum()
            out.setdefault("older_than_store", []).append(int(old))
            out.setdefault("younger", []).append(int(len(ks) - old))
        assert sum(out["older_than_store"]) >= 20 and sum(out["younger"]) >= 20
        jp = jp_of(S, E)
        assert (jp == S["stored"] - 1).sum() >= 5 and (jp < S["stored"] - 1).sum() >= 5
        assert S["T"] - S["store"] == 27
        Eall = expect(S, stored=S["T"])   # over all 75 frames: the clamp to the store is visible
        assert not (len(Eall["M"]) == len(E["M"]) and np.array_equal(Eall["M"], E["M"]) and np.array_equal(Eall["first"], E["first"]))
    if name == "still":
        assert all(np.array_equal(S["histR"][0, j], S["histR"][0, STILL_FROM]) and np.array_equal(S["histT"][0, j], S["histT"][0, STILL_FROM])
                   for j in range(STILL_FROM, S["T"]))
        ties = still_ties(S)
        both = 0
        for _k, depths in ties:
            d = depths[:, None] - depths[None, :]
            if len(depths) >= 2 and (d == 64).any() and ((d > 0) & (d % 64 != 0)).any():
                both += 1
        out["tied"] = both
        assert both >= 10, both
    return out


@functools.lru_cache(maxsize=None)
def scene(name, seed=None):
    """the committed scene with its cover conditions asserted; computed once and shared: callers leave the arrays unchanged"""
    S = build(name, SEEDS[name] if seed is None else seed)
    S["cover"] = cover(S)
    return S


def find_seed(name, tries=50):
    """the first seed at which the scene meets its cover conditions"""
    for seed in range(tries):
        try:
            scene.__wrapped__(name, seed)
            return seed
        except AssertionError:
            continue
    raise AssertionError("no seed found")
