"""Scenes of the merge matcher's reference pin: what tests/golden/make_mergematch_golden.py feeds the reference's driver
tests/cxx/ref_mergematch_test.cpp, and the record layout both sides read.

A scene is PLANTED: small images of 192 x 144 at imgScale 0.5 (full positions are even integers, every product below is exact), K with
power-of-two focal length and E a pure translation along x, so that F's entries are powers of two and the epipolar error of (p1, p2) is
exactly |y1 - y2|.  Every camera's small image is its own white noise; a feature carries a 15 x 15 patch pasted at its integer small
position, and a correspondence is the same patch pasted into the other camera: identical blocks, bit-equal scores."""
import struct

import numpy as np

WS, HS, SCALE = 192, 144, 0.5
K = np.array([256.0, 0, 192.0, 0, 256.0, 144.0, 0, 0, 1.0])
E_X = np.array([0.0, 0, 0, 0, 0, -1.0, 0, 1.0, 0])       # [t]x, t = (1, 0, 0)
SITES = [(22 + 17 * cx, 10 + 17 * cy) for cy in range(8) for cx in range(10)]     # 80 patch sites, 17 px apart, clear of the borders


class Cam:
    def __init__(self, rng, N):
        self.img = rng.integers(0, 256, (HS, WS)).astype(np.uint8)
        self.N, self.n = N, 0
        self.xy = np.zeros((2, N))
        self.state = np.full(N, -1, np.int32)

    def paste(self, patch, u, v):
        """the patch centred at small pixel (u, v), clipped to the image"""
        for dy in range(-7, 8):
            for dx in range(-7, 8):
                if 0 <= v + dy < HS and 0 <= u + dx < WS:
                    self.img[v + dy, u + dx] = patch[dy + 7, dx + 7]

    def feature(self, u, v, dead_before=0):
        """a live slot at small pixel (u, v) behind `dead_before` dead slots -> its slot"""
        self.n += dead_before
        s = self.n
        self.xy[:, s] = (u / SCALE, v / SCALE)
        self.state[s] = s % 2
        self.n += 1
        return s

    def record(self):
        return dict(K=K.copy(), xy=self.xy.copy(), state=self.state.copy(), imgSmall=self.img.copy(), imgScale=SCALE)


def _link(rng, a, b, sites, du, dv=0, noise=0.0):
    """the features of camera a at `sites` (made here) copied into camera b at (u + du, v + dv) -> [(slot a, slot b)]"""
    out = []
    for q, (u, v) in enumerate(sites):
        patch = rng.integers(0, 256, (15, 15)).astype(np.uint8)
        a.paste(patch, u, v)
        pb = patch if not noise else np.clip(patch.astype(np.float64) + rng.normal(0, noise * (1 + q), (15, 15)), 0, 255).astype(np.uint8)
        b.paste(pb, u + du, v + dv)
        out.append((a.feature(u, v, dead_before=1 if q % 4 == 1 else 0), b.feature(u + du, v + dv, dead_before=1 if q % 5 == 2 else 0)))
    return out


def _pts(ca, cb, pairs):
    """slot pairs -> [(position in camera a, position in camera b)]"""
    return [(tuple(ca.xy[:, a]), tuple(cb.xy[:, b])) for a, b in pairs]


def scene_quirk(seed=1):
    """5 cameras, groups {0, 1}, {2, 3}, {4}.  Group pair (0, 1): (0, 2) has fewer than 25 SURF matches, (0, 3) gives 30 matches, (1, 2)
    gives 25 -- and wins, because behind the skipped entry the threshold is read from an unfilled slot; group pair (0, 2): (0, 4) fails
    computeEMat, (1, 4) gives 10 matches.  Equal group sizes: m_gid1 is the SECOND group."""
    rng = np.random.default_rng(seed)
    N = 100
    c = [Cam(rng, N) for _ in range(5)]
    p03 = _link(rng, c[0], c[3], SITES[:30], 5)
    p12 = _link(rng, c[1], c[2], SITES[30:55], -4)
    p14 = _link(rng, c[1], c[4], SITES[55:65], 3)
    junk = [((7.0 * k, 5.0 * k), (300.0 - 3 * k, 11.0 * k)) for k in range(1, 25)]
    ent = [(0, 0, 4, 2, junk[:9], 40), (1, 0, 4, 2, _pts(c[1], c[4], p14)[:8] + junk[:8], 30), (0, 0, 2, 1, junk[:24], 24),
           (0, 0, 3, 1, _pts(c[0], c[3], p03)[:16], 40), (1, 0, 2, 1, _pts(c[1], c[2], p12)[:15], 35)]
    return _finish(rng, c, [[0, 1], [2, 3], [4]], ent, (20.0, 0.45, 150.0), 300)


def scene_edges(seed=2, ncc_min=0.45):
    """3 cameras, groups {0, 1}, {2} (m_gid1 is the FIRST group), one entry (0, 2) with, next to 22 plain correspondences:
    a copy 10 small pixels lower (epipolar error exactly 20.0: stays) and one 11 lower (22: goes); a copy 75 small pixels to the right of
    the seeds' disparity (exactly maxDisp 150: stays) and one 76 to the right (goes); two seeds equidistant from a feature, the first with
    the disparity that keeps its candidate; one patch pasted twice into camera 2 (two bit-equal scores for a row) and one pasted twice
    into camera 0 (for a column); features 2 px from the image's border; noisy copies with scores between nccMin and 1."""
    rng = np.random.default_rng(seed)
    N = 110
    c = [Cam(rng, N) for _ in range(3)]
    du = 6
    pairs = _link(rng, c[0], c[2], SITES[10:32], du)
    notes = {}
    # epiMax: feature at site 30, true copy, a copy 10 below and one 11 below
    for name, (site, offs) in dict(epi=(34, [(du, 0), (du + 40, 10), (du + 80, 11)]), disp=(40, [(du, 0), (du + 75, 0)]), disp_out=(50, [(du, 0), (du + 76, 0)]),
                                   row=(60, [(du, 0), (du + 30, 0)])).items():
        u, v = SITES[site]
        patch = rng.integers(0, 256, (15, 15)).astype(np.uint8)
        c[0].paste(patch, u, v)
        a = c[0].feature(u, v, dead_before=1)
        notes[name] = (a, [])
        for (ou, ov) in offs:
            c[2].paste(patch, u + ou, v + ov)
            notes[name][1].append(c[2].feature(u + ou, v + ov))
    u, v = SITES[70]                                   # column tie: one patch twice in camera 0
    patch = rng.integers(0, 256, (15, 15)).astype(np.uint8)
    c[0].paste(patch, u, v), c[0].paste(patch, u + 34, v), c[2].paste(patch, u + du, v)
    notes["col"] = ([c[0].feature(u, v), c[0].feature(u + 34, v)], c[2].feature(u + du, v))
    for (u, v) in ((2, 70), (160, 2), (WS - 3 - du, 100), (150, HS - 3)):     # the cutter's border path
        patch = rng.integers(0, 256, (15, 15)).astype(np.uint8)
        c[0].paste(patch, u, v), c[2].paste(patch, u + du, v)
        pairs.append((c[0].feature(u, v), c[2].feature(u + du, v)))
    noisy = _link(rng, c[0], c[2], SITES[:6], du, noise=14.0)
    c[1].feature(50, 50), c[1].feature(90, 70)
    notes["noisy"] = noisy
    inl = _pts(c[0], c[2], pairs)[:15]
    # two seeds equidistant from the `disp` feature, 10 px left and right of it: the first carries the true disparity, the second one
    # under which the feature's candidates would all fail
    x, y = c[0].xy[:, notes["disp"][0]]
    inl += [((x - 10, y), (x - 10 + 2 * du, y)), ((x + 10, y), (x + 10 + 2 * du + 400, y))]
    x, y = c[0].xy[:, notes["disp_out"][0]]
    inl += [((x, y + 4), (x + 2 * du, y + 4))]
    S = _finish(rng, c, [[0, 1], [2]], [(0, 0, 2, 1, inl, 30)], (20.0, ncc_min, 150.0), 310)
    S["notes"] = notes
    return S


def _finish(rng, cams, groups, ent, par, frame):
    """ent: (iCam, gId1, jCam, gId2, inlier point pairs, total SURF matches).  detectSURFPoints depends on the camera only: every camera gets
    ONE point list, the entries' matches index it; the matches behind the inliers are random points with flag 0."""
    surf = [[] for _ in cams]

    def add(c, p):
        surf[c].append((float(p[0]), float(p[1])))
        return len(surf[c]) - 1

    entries = []
    for (i, g1, j, g2, inl, nm) in ent:
        idx = [(add(i, a), add(j, b)) for a, b in inl]
        idx += [(add(i, rng.uniform(0, 380, 2)), add(j, rng.uniform(0, 280, 2))) for _ in range(nm - len(inl))]
        flags = np.zeros(nm, np.uint8)
        flags[:len(inl)] = 1
        entries.append(dict(iCam=i, gId1=g1, jCam=j, gId2=g2, idx=np.array(idx, np.int32), E=E_X.copy(), flags=flags))
    for q in entries:
        q["surf1"], q["surf2"] = np.array(surf[q["iCam"]]).reshape(-1, 2), np.array(surf[q["jCam"]]).reshape(-1, 2)
    return dict(nC=len(cams), N=cams[0].N, Ws=WS, Hs=HS, frame=frame, scale=SCALE, par=par, groups=groups, cams=[c.record() for c in cams],
                entries=entries)


def jobs_of(S):
    """the entries the loop matches (25 or more SURF matches, 15 or more inliers) as mergematch_ref jobs -> [(entry, job)]"""
    out = []
    for e, q in enumerate(S["entries"]):
        if len(q["idx"]) >= 25 and int(q["flags"].sum()) >= 15:
            k = np.nonzero(q["flags"])[0]
            seeds = np.concatenate([q["surf1"][q["idx"][k, 0]], q["surf2"][q["idx"][k, 1]]], 1)
            out.append((e, dict(iCam=q["iCam"], jCam=q["jCam"], E=q["E"], seeds=seeds)))
    return out


def write_input(f, scenes):
    f.write(struct.pack("i", len(scenes)))
    for S in scenes:
        f.write(struct.pack("=5id3d", S["nC"], S["N"], S["Ws"], S["Hs"], S["frame"], S["scale"], *S["par"]))
        f.write(struct.pack("i", len(S["groups"])))
        for g in S["groups"]:
            f.write(struct.pack("i%di" % len(g), len(g), *g))
        for c in S["cams"]:
            f.write(np.asarray(c["K"], np.float64).tobytes() + np.ascontiguousarray(c["xy"], np.float64).tobytes())
            f.write(np.asarray(c["state"], np.int32).tobytes() + np.ascontiguousarray(c["imgSmall"], np.uint8).tobytes())
        f.write(struct.pack("i", len(S["entries"])))
        for q in S["entries"]:
            f.write(struct.pack("4i", q["iCam"], q["gId1"], q["jCam"], q["gId2"]))
            for s in (q["surf1"], q["surf2"]):
                f.write(struct.pack("i", len(s)) + np.ascontiguousarray(s, np.float64).tobytes())
            f.write(struct.pack("i", len(q["idx"])) + np.ascontiguousarray(q["idx"], np.int32).tobytes())
            f.write(np.asarray(q["E"], np.float64).tobytes() + np.asarray(q["flags"], np.uint8).tobytes())


def read_output(raw, scenes):
    """the driver's record -> per scene dict(ran [nInfo], F [nInfo][9], matches [per entry int32 [n][2] SLOT pairs], scores, loop: numMatched,
    called, maxgId1, maxgId2, maxiCam, maxjCam, m_gid1, m_gid2, m_camid1, m_camid2, rec_matches)"""
    off, out = 0, []
    for S in scenes:
        G = dict(ran=[], F=[], matches=[], scores=[])
        for _ in S["entries"]:
            (ran,) = struct.unpack_from("i", raw, off)
            F = np.frombuffer(raw, np.float64, 9, off + 4)
            (n,) = struct.unpack_from("i", raw, off + 76)
            rec = np.frombuffer(raw, np.dtype([("a", "<i4"), ("b", "<i4"), ("s", "<f8")]), n, off + 80)
            off += 80 + 16 * n
            G["ran"].append(ran), G["F"].append(F.copy()), G["matches"].append(np.stack([rec["a"], rec["b"]], 1).astype(np.int32).reshape(-1, 2))
            G["scores"].append(rec["s"].copy())
        v = struct.unpack_from("11i", raw, off)
        off += 44
        G["loop"] = np.array(v[:10], np.int32)
        G["rec_matches"] = np.frombuffer(raw, np.int32, 2 * v[10], off).reshape(-1, 2).copy()
        off += 8 * v[10]
        out.append(G)
    assert off == len(raw)
    return out
