"""Synthetic scenes of the merge constraints in the stored layout of tests/mergeconstraints_golden_util.py: what
tests/golden/make_mergeconstraints_golden.py feeds the reference's driver, and what the GPU tests and tools/mergeconstraints_time.py build
where the golden file does not reach (16 cameras, thousands of slots).  A spec: groups (discovery order, not ascending), g = (gId1, gId2),
ij = (maxiCam, maxjCam), nF frames held, gaps = key-frame distances back from the current frame, moved = per older key frame (newest
first) the cameras with the self-motion flag, nA / nB points per side, nMatch matches, plant in ("mixed", "shared", "reject", "clean");
optional noise = the pixel noise of a node (default 0.5; 0 gives exact projections of the true points)."""
import math
import struct

import numpy as np

from tests import mergeconstraints_ref as ref


def rodrigues(w):
    th = float(np.linalg.norm(w))
    k = w / th if th > 0 else np.zeros(3)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def make_scene(sc, spec, rng):
    groups, nF = spec["groups"], spec["nF"]
    nC = 1 + max(max(g) for g in groups)
    frame0 = 200 + 37 * sc
    f2 = frame0 + nF - 1
    keys = [f2]
    for gap in spec["gaps"]:
        keys.append(keys[-1] - gap)
    keys = keys[::-1]
    assert keys[0] >= frame0
    self_motion = np.zeros((len(keys), nC), np.int8)
    for back, cams in enumerate(spec["moved"]):
        for c in cams:
            self_motion[len(keys) - 2 - back, c] = 1
    self_motion[-1] = rng.integers(0, 2, nC)                     # the current key frame's own flag is never read
    gId1, gId2 = spec["g"]
    cam_ids = ref.cam_ids_in_both_groups(groups, gId1, gId2)
    fc = ref.first_constrain(keys, self_motion, cam_ids)
    assert fc is not None
    f1 = keys[fc[0]]
    K = np.zeros((nC, 9), np.float32)
    R, t = np.zeros((nC, nF, 9), np.float32), np.zeros((nC, nF, 3), np.float32)
    for c in range(nC):
        K[c] = [515 + 15 * rng.random(), 0.3 if c % 2 else 0.0, 320 + 4 * rng.normal(), 0, 512 + 15 * rng.random(), 240 + 4 * rng.normal(), 0, 0, 1]
        base = np.array([0.8 * (c % 5) - 1.5, 0.3 * (c // 5) + 0.04 * c, -0.2 * (c % 3)])
        vel = np.array([0.02 + 0.01 * rng.random(), 0.004 * rng.normal(), 0.006 * rng.normal()])
        for i in range(nF):
            Rm = rodrigues(np.array([0.01 * c + 0.002 * rng.normal(), 0.04 * (c % 5) - 0.08 - 0.001 * i, 0.002 * rng.normal()]))
            R[c, i], t[c, i] = Rm.reshape(9), -(Rm @ (base + vel * i + 0.003 * rng.normal(size=3)))
    Kd, Rd, td = K.astype(np.float64), R.astype(np.float64), t.astype(np.float64)

    n_slot = [0] * nC
    pools = [[] for _ in range(nC)]
    nodes = []           # (cam, frame, slot, X, noise scale)
    cur_slots = []       # (cam, slot, map index or -1, state)
    M, feat_ref = [], []

    def new_slot(c):
        n_slot[c] += 1
        return n_slot[c] - 1

    def chain(c, m, X, head, kind):
        """one reference of point m in camera c with its chain -> feat_ref[m][c]"""
        lo_min = max(frame0, f1 - 3)
        if kind == "run":            # the head's run reaches f1
            runs = [(head, int(rng.integers(lo_min, min(f1, head) + 1)))]
        elif kind == "short":        # ends above f1, nothing behind
            runs = [(head, int(rng.integers(f1 + 1, head + 1)))]
        elif kind == "seg":          # f1 only through a linked segment
            a = int(rng.integers(f1 + 1, head + 1))
            runs = [(head, a), (a - 1 - int(rng.integers(0, min(2, a - 1 - f1) + 1)), int(rng.integers(lo_min, f1 + 1)))]
            if runs[1][0] < f1:
                runs[1] = (f1, runs[1][1])
        elif kind == "seg2":         # two segments, the older one holds f1
            a = int(rng.integers(f1 + 2, head + 1)) if head >= f1 + 2 else head
            runs = [(head, a), (a - 1, f1 + 1), (f1, int(rng.integers(lo_min, f1 + 1)))] if a - 1 >= f1 + 1 else [(head, a), (f1, lo_min)]
        else:                        # "gap": a segment wholly older than f1
            a = int(rng.integers(f1 + 1, head + 1))
            runs = [(head, a), (f1 - 1, int(rng.integers(lo_min, f1)))] if f1 - 1 >= lo_min else [(head, a)]
        runs = [(hi, lo) for hi, lo in runs if frame0 <= lo <= hi]
        slots = [new_slot(c) for _ in runs]
        nxt = -1
        for q in range(len(runs) - 1, 0, -1):
            pools[c].append((slots[q], runs[q][0], runs[q][1], nxt))
            nxt = len(pools[c]) - 1
        for (hi, lo), s in zip(runs, slots):
            for f in range(lo, hi + 1):
                nodes.append((c, f, s, X, spec.get("noise", 0.5)))
        feat_ref[m][c] = (slots[0], runs[0][0], runs[0][1], nxt)
        if head == f2:
            cur_slots.append((c, slots[0], m, int(rng.integers(0, 2))))
        return slots[0]

    def add_point(X, seen, kinds=("run", "run", "short", "seg", "seg2", "gap"), off=0.03, stale=()):
        m = len(M)
        M.append(np.asarray(X) + off * rng.normal(size=3))
        feat_ref.append([(-1, 0, 0, -1)] * nC)
        out = {}
        for c in seen:
            out[c] = chain(c, m, X, f2, kinds[int(rng.integers(0, len(kinds)))])
        for c in stale:              # a reference the camera lost a few frames ago
            chain(c, m, X, f2 - int(rng.integers(1, 4)), "run")
        return m, out

    def rand_X():
        return np.array([-2 + 6 * rng.random(), -1.5 + 3 * rng.random(), 7 + 5 * rng.random()])

    def subset(cams, must=None, pmore=0.5):
        s = [c for c in cams if rng.random() < pmore]
        if must is not None and must not in s:
            s.append(must)
        if not s:
            s = [cams[int(rng.integers(0, len(cams)))]]
        return sorted(s)

    g1, g2 = sorted(groups[gId1]), sorted(groups[gId2])
    iC, jC = spec["ij"]
    others = [c for c in range(nC) if c not in g1 and c not in g2]
    plant = spec["plant"]
    matches = []
    for k in range(spec["nMatch"]):
        X = rand_X()
        dup = plant in ("mixed", "shared") and k % 3 == 1          # m2 holds a view in a camera where m1 holds one
        seenA = subset(g1, iC)
        if plant == "shared" and k % 4 == 2:
            seenA = sorted(set(seenA) | {g2[-1]})                  # m1 is already seen by a camera of the other group
        ma, sa = add_point(X, seenA, stale=others[:1] if k % 2 else ())
        Xb = X + (np.array([14.0, -9.0, 3.0]) if plant == "reject" and k < 3 else 0.0)
        seenB = subset(g2, jC)
        if dup:
            seenB = sorted(set(seenB) | {iC})
        mb, sb = add_point(Xb, seenB, off=0.05)
        matches.append((sa[iC], sb[jC]))
        if plant == "shared" and k % 5 == 4:                       # a second match onto the same point of camera j
            X2 = rand_X()
            m3, s3 = add_point(X2, subset(g1, iC))
            matches.append((s3[iC], sb[jC]))
    for _ in range(spec["nA"]):
        r = rng.random()
        seen = subset(g1, pmore=0.6)
        if r < 0.25:
            seen = [seen[0]]
        if r > 0.9 and len(g2) > 0:
            seen = sorted(set(seen) | {g2[0]})
        if others and 0.6 < r < 0.8:
            seen = sorted(set(seen) | {others[0]})      # numVisCam counts every camera, not only the groups'
        add_point(rand_X(), seen, kinds=("short",) if r < 0.15 else ("run", "run", "short", "seg", "seg2", "gap"), stale=others[:1] if r > 0.8 else ())
    for _ in range(spec["nB"]):
        r = rng.random()
        seen = subset(g2, pmore=0.6)
        if r < 0.25:
            seen = [seen[0]]
        add_point(rand_X(), seen, kinds=("short",) if r < 0.15 else ("run", "run", "short", "seg", "seg2", "gap"))
    for c in others:
        for _ in range(6):
            add_point(rand_X(), [c])
    # tracked slots of no map point (a match may land on one), and slots that hold nothing
    unmapped = {}
    for c in range(nC):
        for _ in range(5):
            s = new_slot(c)
            cur_slots.append((c, s, -1, 0))
            nodes.append((c, f2, s, rand_X(), 2.0))
            unmapped.setdefault(c, []).append(s)
        new_slot(c)
    if plant in ("mixed", "shared"):
        X = rand_X()
        ma, sa = add_point(X, [iC])
        matches.insert(2, (sa[iC], unmapped[jC][0]))
        matches.append((unmapped[iC][1], unmapped[jC][2]))
    N = max(n_slot)
    nMap = len(M)
    xy = np.full((nC, nF, 2 * N), -1.0, np.float32)
    for c, f, s, X, ns in nodes:
        i = f - frame0
        u, v = ref.project(Kd[c].tolist(), Rd[c, i].tolist(), td[c, i].tolist(), [float(x) for x in X])
        xy[c, i, s], xy[c, i, N + s] = u + ns * rng.normal(), v + ns * rng.normal()
    state = np.full((nC, N), -1, np.int8)
    slot2map = np.full((nC, N), -1, np.int16)
    for c, s, m, st in cur_slots:
        state[c, s], slot2map[c, s] = st, m
    cap = max(1, max(len(p) for p in pools))
    seg_pool = np.full((nC, cap, 4), -1, np.int16)
    for c in range(nC):
        if pools[c]:
            seg_pool[c, :len(pools[c])] = np.array(pools[c], np.int16)
    g_arr = np.full((len(groups), 16), -1, np.int8)
    for g, cams in enumerate(groups):
        g_arr[g, :len(cams)] = cams
    Mf = np.array(M, np.float32)
    assert len(set(map(bytes, Mf))) == nMap, "the map points' coordinates must be unique"
    return dict(frame0=np.int32(frame0), key_frames=np.array(keys, np.int16), self_motion=self_motion, groups=g_arr,
                gids=np.array([gId1, gId2, iC, jC], np.int8), K=K, R=R, t=t, M=Mf, state=state, slot2map=slot2map, xy=xy,
                featRef=np.array(feat_ref, np.int16).reshape(nMap, nC, 4), segPool=seg_pool, matches=np.array(matches, np.int16).reshape(-1, 2))


def write_input(f, S):
    """an expanded scene S as the binary record tests/cxx/ref_mergeconstraints_test.cpp and tests/cxx/mergeconstraints_shim_test.cpp read"""
    nC, N, nMap, nF = S["nC"], S["N"], S["nMap"], S["nF"]
    keys, groups = [int(k) for k in S["key_frames"]], S["groups"]
    f.write(struct.pack("12i", nC, N, nMap, nF, S["frame0"], len(keys), len(groups), S["gId1"], S["gId2"], S["maxiCam"], S["maxjCam"], len(S["matches"])))
    f.write(np.asarray(keys, np.int32).tobytes() + np.ascontiguousarray(S["self_motion"], np.int32).tobytes())
    for g in groups:
        f.write(struct.pack(f"{1 + len(g)}i", len(g), *g))
    f.write(np.ascontiguousarray(S["K"], np.float64).tobytes())
    f.write(np.concatenate([S["histR"], S["histT"]], axis=2).astype(np.float64).tobytes())
    f.write(np.ascontiguousarray(S["M"], np.float64).tobytes())
    f.write(np.ascontiguousarray(S["state"], np.int32).tobytes() + np.ascontiguousarray(S["slot2map"], np.int32).tobytes())
    f.write(np.ascontiguousarray(S["histXY"], np.float64).tobytes())
    f.write(np.ascontiguousarray(S["featRef"], np.int32).tobytes())
    for c in range(nC):
        pool = S["segPool"][c]
        n = int((pool[:, 0] >= 0).sum())
        assert (pool[:n, 0] >= 0).all()
        f.write(struct.pack("i", n) + np.ascontiguousarray(pool[:n], np.int32).tobytes())
    f.write(np.ascontiguousarray(S["matches"], np.int32).tobytes())
