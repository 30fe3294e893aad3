"""Writes tests/golden/mergeapply_golden.npz: the reference's OWN CoSLAM::getMapPts + updateStaticPointPositionAtKeyFrms (what
MergeCameraGroup::recomputeMapPoints runs per point) on four scenes of chains built with its classes -- the fixture of
cs_recompute_map_points_keyfrms_dev.  Needs oracle/_ref/ref_mergeapply_test (tests/cxx/ref_mergeapply_test.cpp, built by
oracle/Makefile); where the reference tree exists:

    python tests/golden/make_golden.py mergeapply

Scenes: 3, 4, 6 and 12 cameras, 80-160 frames of poses, a key frame every 3-9 frames at irregular spacing, ~150 points each, per point and
camera a chain of 0-3 segments with gaps and stale heads.  Some cameras stand still for the older half of the run (bit-identical poses:
equal angles, the newest node wins), one camera of the larger scenes only rotates about the origin (bit-identical centres: angle 0, no
second view).  The file holds data only (tests/mergeapply_golden_util.py says how pixels and full arrays are formed from it)."""
import math
import os
import struct
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import mergeapply_ref as ref  # noqa: E402
from tests.golden.fixtures import run_driver  # noqa: E402
from tests.mergeapply_golden_util import chain_nodes, expand  # noqa: E402

SEED = 20
MIN_EACH = 30


def rodrigues(w):
    th = float(np.linalg.norm(w))
    k = w / th if th > 0 else np.zeros(3)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def make_scene(sc, rng):
    nC = (3, 4, 6, 12)[sc]
    nF = (160, 120, 100, 80)[sc]
    nPts = (150, 150, 150, 140)[sc]
    frame0 = 300 + 50 * sc
    cur = frame0 + nF - 1
    keys = [cur]
    while keys[-1] - 3 >= frame0:
        keys.append(keys[-1] - int(rng.integers(3, 10)))
    keys = sorted(k for k in keys if k >= frame0)
    f_start = keys[2]
    f_end = cur if sc < 2 else keys[-3]
    # motion per camera: 0 moving, 1 stands still for the older half, 2 rotates about the origin
    motion = [0] * nC
    if sc >= 1:
        motion[1] = 1
    if sc >= 2:
        motion[2], motion[nC - 1] = 2, 1
    K = np.zeros((nC, 9))
    R, t = np.zeros((nC, nF, 9), np.float32), np.zeros((nC, nF, 3), np.float32)
    for c in range(nC):
        K[c] = [515 + 15 * rng.random(), 0.3 if c % 2 else 0.0, 320 + 4 * rng.normal(), 0, 512 + 15 * rng.random(), 240 + 4 * rng.normal(), 0, 0, 1]
        base = np.array([0.9 * (c % 6) - 1.0, 0.3 * (c // 6) + 0.05 * c, -0.2 * (c % 3)])
        vel = np.array([0.02 + 0.01 * rng.random(), 0.004 * rng.normal(), 0.006 * rng.normal()])
        for i in range(nF):
            w = np.array([0.01 * c + 0.002 * rng.normal(), 0.05 * (c % 6) - 0.1 - 0.0015 * i, 0.002 * rng.normal()])
            Rm = rodrigues(w)
            pos = base + vel * i + 0.004 * rng.normal(size=3)
            if motion[c] == 2:
                pos = np.zeros(3)
            R[c, i], t[c, i] = Rm.reshape(9), -(Rm @ pos)
            if motion[c] == 2:
                t[c, i] = 0.0
        if motion[c] == 1:
            R[c, :nF // 2], t[c, :nF // 2] = R[c, nF // 2], t[c, nF // 2]     # bit-identical poses
    X = np.stack([-2 + 7 * rng.random(nPts), -1.5 + 3 * rng.random(nPts), 7 + 6 * rng.random(nPts)], axis=1).astype(np.float32)
    flags = np.zeros(nPts, np.uint8)
    u = rng.random(nPts)
    flags[u < 0.08], flags[(u >= 0.08) & (u < 0.16)], flags[(u >= 0.16) & (u < 0.24)] = 1, 2, 4
    flags[(u >= 0.24) & (u < 0.26)] = 5
    feat_ref = np.full((nPts, nC, 4), -1, np.int16)
    feat_ref[:, :, 1:3] = 0
    pools = [[] for _ in range(nC)]
    n_slot = [0] * nC
    first_frame, last_frame = np.zeros(nPts, np.int32), np.zeros(nPts, np.int32)
    kin = [k for k in keys]
    for p in range(nPts):
        lo_all, hi_all = cur, frame0
        see = rng.random(nC) < (0.85 if nC <= 6 else 0.45)
        early = rng.random() < 0.09          # a point the run left behind before f_start
        late = sc >= 2 and rng.random() < 0.16 and not early
        lonely = not early and not late and rng.random() < 0.12     # one camera, a track of a few frames: fewer than two views
        if lonely:
            see[:] = False
            see[int(rng.integers(0, nC))] = True
        for c in range(nC):
            if not see[c]:
                continue
            want = 1 if lonely else int(rng.choice([1, 2, 3], p=[0.3, 0.4, 0.3]))
            r = rng.random()
            if early:
                head = int(rng.integers(frame0 + 2, f_start))
            elif late:
                head = cur - int(rng.integers(0, 3)) if rng.random() < 0.5 else int(rng.choice([k for k in kin if k > f_end] or [cur]))
            elif r < 0.45:
                head = cur
            elif r < 0.75:
                head = int(rng.choice(kin[len(kin) // 2:]))                      # a stale head at a key frame
            else:
                head = cur - int(rng.integers(1, 9))                             # a stale head wherever the track ended
            segs, f = [], head
            for q in range(want):
                L = 1 + int(rng.integers(0, 10 if (q == 0 and want > 1) else 40))
                if q == 0 and want > 1 and rng.random() < 0.3:
                    L = 1
                if (late and q == want - 1) or lonely:
                    L = min(L, 3)
                first = max(f - L + 1, frame0 if not late else f_end + 1 if f > f_end else frame0)
                if first > f:
                    break
                segs.append((f, first))
                f = first - 1 - int(rng.integers(1, 13))
                if f < frame0 or (late and f <= f_end):
                    break
            if not segs:
                continue
            slots = []
            for _ in segs:
                slots.append(n_slot[c])
                n_slot[c] += 1
            nxt = -1
            for q in range(len(segs) - 1, 0, -1):
                pools[c].append((slots[q], segs[q][0], segs[q][1], nxt))
                nxt = len(pools[c]) - 1
            feat_ref[p, c] = (slots[0], segs[0][0], segs[0][1], nxt)
            lo_all, hi_all = min(lo_all, segs[-1][1]), max(hi_all, segs[0][0])
        first_frame[p], last_frame[p] = (lo_all, hi_all) if hi_all >= lo_all else (cur, cur)
    cap = max(1, max(len(q) for q in pools))
    seg_pool = np.full((nC, cap, 4), -1, np.int16)
    for c in range(nC):
        if pools[c]:
            seg_pool[c, :len(pools[c])] = np.array(pools[c], np.int16)
    return dict(K=K, R=R, t=t, frame0=np.int32(frame0), X=X, featRef=feat_ref, segPool=seg_pool, key_frames=np.array(keys, np.int16),
                f_start=np.int32(f_start), f_end=np.int32(f_end), sigma=np.float64(3.0), flags=flags, firstFrame=first_frame.astype(np.int16),
                lastFrame=last_frame.astype(np.int16), list=rng.integers(0, 3, nPts).astype(np.uint8), motion=np.array(motion, np.uint8))


def write_input(f, S):
    E = S["_e"]
    nC, nF, nPts = E["nC"], E["nF"], len(E["X"])
    keys = [int(k) for k in S["key_frames"]]
    f.write(struct.pack("7i", nC, nF, E["frame0"], nPts, int(S["f_start"]), int(S["f_end"]), len(keys)))
    f.write(struct.pack(f"{len(keys)}i", *keys))
    f.write(struct.pack("d", float(S["sigma"])))
    f.write(E["K"].tobytes())
    f.write(np.concatenate([E["histR"], E["histT"]], axis=2).tobytes())
    N = E["N"]
    for p in range(nPts):
        f.write(E["M0"][p].tobytes() + E["cov0"][p].tobytes())
        f.write(struct.pack("4i", int(S["flags"][p]), int(S["firstFrame"][p]), int(S["lastFrame"][p]), int(S["list"][p])))
        for c in range(nC):
            nodes = chain_nodes(E["featRef"][p, c], E["segPool"][c])
            runs = []
            for fr, slot in nodes:
                if runs and runs[-1][2] == slot:
                    runs[-1][1] = fr
                else:
                    runs.append([fr, fr, slot])
            f.write(struct.pack("i", len(runs)))
            for last, first, slot in runs:
                f.write(struct.pack("2i", last, first))
                for fr in range(last, first - 1, -1):
                    i = fr - E["frame0"]
                    f.write(struct.pack("2d", E["histXY"][c, i, slot], E["histXY"][c, i, N + slot]))


def categories(S, E, M_ref):
    """what the file has to hold (the issue's list), counted with the restatement"""
    keys = [int(k) for k in S["key_frames"]]
    keyset, cur, frame0 = set(keys), E["frame0"] + E["nF"] - 1, E["frame0"]
    all_frames = list(range(frame0, cur + 1))
    det = {}
    M, cov = E["M0"].copy(), E["cov0"].copy()
    cnt = ref.recompute_map_points_keyfrms(E["K"], E["iK"], E["histR"], E["histT"], E["histXY"], frame0, E["featRef"], E["segPool"], None,
                                           S["firstFrame"], S["lastFrame"], S["flags"], int(S["f_start"]), int(S["f_end"]), keys, M, cov,
                                           float(S["sigma"]), detail=det)
    Ma = E["M0"].copy()
    ref.recompute_map_points_keyfrms(E["K"], E["iK"], E["histR"], E["histT"], E["histXY"], frame0, E["featRef"], E["segPool"], None,
                                     S["firstFrame"], S["lastFrame"], S["flags"], int(S["f_start"]), int(S["f_end"]), keys, Ma, E["cov0"].copy(),
                                     float(S["sigma"]), angles=True)
    assert np.array_equal(M, Ma), "cosine order and angle order disagree"
    c = dict(head_not_key=0, only_head=0, filter_changes=0, behind_gap=0, few_views=cnt[2], before=0, after=0, flag1=0, flag2=0, flag4=0,
             standing=0, rotating=0, filter_points=[])
    fl, ff, lf = S["flags"], S["firstFrame"], S["lastFrame"]
    c["before"], c["after"] = int((lf < int(S["f_start"])).sum()), int((ff > int(S["f_end"])).sum())
    c["flag1"], c["flag2"], c["flag4"] = int((fl == 1).sum()), int((fl == 2).sum()), int((fl == 4).sum())
    Rl, Tl = E["histR"].tolist(), E["histT"].tolist()
    centre = lambda cc, f: ref.cam_center(Rl[cc][f - frame0], Tl[cc][f - frame0])  # noqa: E731
    for m, rec in det.items():
        M0 = [float(v) for v in E["M0"][m]]
        changed = False
        for cc in range(E["nC"]):
            r4 = E["featRef"][m, cc]
            if r4[0] < 0:
                continue
            nodes = chain_nodes(r4, E["segPool"][cc])
            if int(r4[1]) not in keyset:
                c["head_not_key"] += any(f in keyset for f, _ in nodes[1:])
                continue
            w = rec["walks"][cc]
            if not w["nodes"]:
                c["only_head"] += 1
                continue
            # the runner-up: at least 1e-9 rad away, or bit-equal
            cs = sorted(set(v for _, _, v in w["nodes"]))
            if len(cs) > 1 and w["node"] is not None:
                assert abs(math.acos(min(1.0, cs[0])) - math.acos(min(1.0, cs[1]))) >= 1e-9, (m, cc, cs[:2])
            if w["node"] is None:
                assert all(v == 1.0 for _, _, v in w["nodes"])
                c["rotating"] += 1
                continue
            best = min(v for _, _, v in w["nodes"])
            ties = [f for f, _, v in w["nodes"] if v == best]
            if len(ties) > 1:
                assert w["node"][1] == max(ties)
                c["standing"] += 1
            c["behind_gap"] += w["node"][0] != int(r4[0])
            wa = ref.walk_widest_key_node(cc, r4, E["segPool"], E["segPool"].shape[1], E["N"], all_frames, frame0, cur, centre, M0,
                                          centre(cc, int(r4[1])))
            if wa["node"] is not None and wa["node"][1] not in keyset:
                c["filter_changes"] += 1
                changed = True
        if changed and len(rec["views"]) >= 2:
            c["filter_points"].append(m)
    assert np.array_equal(M, M_ref), "the restatement does not reproduce the reference"
    return c, cnt


def mergeapply_case():
    rng = np.random.default_rng(SEED)
    scenes = [make_scene(sc, rng) for sc in range(4)]
    for sc, S in enumerate(scenes):
        S["_e"] = expand(S, SEED + sc)
    with tempfile.TemporaryDirectory() as td:
        pin, pout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(pin, "wb") as f:
            f.write(struct.pack("i", len(scenes)))
            for S in scenes:
                write_input(f, S)
        print(run_driver("ref_mergeapply_test", "golden", pin, pout).strip())
        raw = open(pout, "rb").read()
    off, total = 0, {}
    out = dict(n_scenes=np.int32(len(scenes)), seed=np.int32(SEED))
    for sc, S in enumerate(scenes):
        nPts = len(S["X"])
        n_sel = struct.unpack_from("i", raw, off)[0]
        off += 4
        rec = np.frombuffer(raw, dtype=np.dtype([("sel", "<i4"), ("M", "<f8", 3), ("cov", "<f8", 9)]), count=nPts, offset=off)
        off += nPts * rec.dtype.itemsize
        assert n_sel == int(rec["sel"].sum())
        S["M_ref"], S["cov_ref"], S["selected"] = rec["M"].copy(), rec["cov"].copy(), rec["sel"].astype(np.uint8)
        E = S.pop("_e")
        c, cnt = categories(S, E, S["M_ref"])
        assert cnt[0] == n_sel, (cnt, n_sel)
        assert np.array_equal(np.where((S["M_ref"] != E["M0"]).any(axis=1)[:, None], S["cov_ref"], E["cov0"]), S["cov_ref"])
        S["filter_points"] = np.array(c.pop("filter_points"), np.int16)
        print(f"scene {sc}: {E['nC']} cameras, {E['nF']} frames, {len(S['key_frames'])} key frames, {nPts} points, counts {cnt}: {c}")
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
        for k, v in S.items():
            out[f"s{sc}_{k}"] = v
    print("all scenes:", total)
    for k, v in total.items():
        assert v >= MIN_EACH, f"only {v} of {k}"
    assert sum(len(S["filter_points"]) for S in scenes) >= MIN_EACH
    return out
