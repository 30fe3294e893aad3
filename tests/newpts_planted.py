"""Planted scenes for the new-map-point tests (cs_newpts_from_pairs_dev against oracle.new_map_points_from_pairs): every track is
asked for by a specification -- its first camera, its number of views, one view moved off so that the re-projection gate rejects it,
views whose feature is DYNAMIC, a view pinned to a given pixel -- instead of being left to chance, so that a scene holds exactly the
(first camera, length) combinations, the register sets and the decidePointType distances a test is about.  Pure numpy, no GPU.

planted_scene() returns the record tests.test_newpts_gpu._run_both consumes.  The cameras are tests.poseupdate_scene.Scene's, frame 2:
Re / te are the poses the kernels get, Rt / tt project the truth.

A track specification is a dict:
    c0, nv          first camera, number of views (cameras c0 .. c0 + nv - 1)
    bad_view        optional: index of a view moved 40 px in y (the cameras lie side by side along x, a move in x would only change the
                    depth): the whole track fails the 3 px re-projection gate
    dynamic_views   optional: indices of views whose feature is not static
    anchor          optional (view, x, y) or (view, ("rel", track, view, dx, dy)): the scene point is the back-projection of that pixel
                    of camera c0 + view at `depth`, and the view's feature is EXACTLY that pixel (no noise); "rel" names the feature
                    of an earlier track (or, with track < 0, of map point -1 - track's `feats` entry `view`)
    depth           optional: the anchor's depth in its camera (default: drawn from 8..12)
A map-point specification (points the map holds already) is a dict:
    flag            its type (0 certain static, 1 certain dynamic, 4 uncertain, 5 uncertain dynamic, 2 false)
    feats           its features of this frame: (cam, x, y), or (cam, ("rel", track, view, dx, dy)) beside a planted track's feature
    index           optional: its place in the map
    views           instead of feats: (c0, nv), the noisy projections of a scene point of its own
"""
import numpy as np

from tests.poseupdate_scene import Scene

W_IMG, H_IMG = 640, 480
FRAME = 2


def _project(K, R, t, P):
    u = K @ (R @ P + t)
    return u[:2] / u[2]


def planted_scene(nC, N, seed, specs, map_points=(), n_map=None, extra=None, noise=0.2, check=True):
    """the record of _run_both: sc, nC, N, nMap, cap, xy, state, s2m, R, t, mapPts, mapCov, flags, pf, is_static, pairs, frame; plus
    planted (per specification the [(camera, slot)] of its views) and map_slots (per map-point specification its [(camera, slot)]).
    n_map: length of the existing map (default: the map-point specifications, which take its FIRST indices unless they carry `index`);
    the map's other points have no feature in this frame.  check: assert the builder's guarantees through the restatement."""
    rng = np.random.default_rng(seed)
    sc = Scene(nC=nC, N=8, nMap=1, T=FRAME + 1, seed=seed)
    f = FRAME
    R = np.stack([sc.Re[f][c].reshape(9) for c in range(nC)])
    t = np.stack([sc.te[f][c] for c in range(nC)])
    perm = [rng.permutation(N) for _ in range(nC)]       # slots are handed out in this order: slot order is not track order
    used = [0] * nC
    # every slot nobody asks for holds a live, unmapped, static feature somewhere in the image
    xy = [np.concatenate([rng.uniform(5, W_IMG - 5, N), rng.uniform(5, H_IMG - 5, N)]) for _ in range(nC)]
    state = [np.zeros(N, dtype=np.int32) for _ in range(nC)]
    s2m = [np.full(N, -1, dtype=np.int32) for _ in range(nC)]
    is_static = [np.ones(N, dtype=np.uint8) for _ in range(nC)]

    def take(c, x, y):
        assert used[c] < N, f"camera {c} has no free slot left (N = {N})"
        s = int(perm[c][used[c]])
        used[c] += 1
        xy[c][s], xy[c][N + s] = x, y
        return s

    planted, map_slots = [], [None] * len(map_points)

    def resolve(v):
        if isinstance(v, tuple) and v and v[0] == "rel":
            _, tr, view, dx, dy = v
            c, s = planted[tr][view] if tr >= 0 else map_slots[-1 - tr][view]
            return xy[c][s] + dx, xy[c][N + s] + dy
        return v

    def plant_map_feats(only_absolute):
        for q, mp in enumerate(map_points):
            if map_slots[q] is not None:
                continue
            if "views" in mp:
                c0, nv = mp["views"]
                P = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(8, 12)])
                map_slots[q] = []
                for c in range(c0, c0 + nv):
                    m = _project(sc.K, sc.Rt[f][c], sc.tt[f][c], P) + rng.normal(0, noise, 2)
                    map_slots[q].append((c, take(c, m[0], m[1])))
                continue
            if only_absolute and any(len(ft) == 2 for ft in mp["feats"]):   # (relative to a track: behind the tracks)
                continue
            map_slots[q] = []
            for ft in mp["feats"]:
                x, y = resolve(ft[1]) if len(ft) == 2 else (ft[1], ft[2])
                map_slots[q].append((ft[0], take(ft[0], x, y)))

    plant_map_feats(only_absolute=True)
    for sp in specs:
        c0, nv = sp["c0"], sp["nv"]
        assert 0 <= c0 and nv >= 2 and c0 + nv <= nC
        anchor = sp.get("anchor")
        if anchor is None:
            P = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(8, 12)])
        else:
            av = anchor[0]
            ax, ay = resolve(anchor[1]) if len(anchor) == 2 else (anchor[1], anchor[2])
            depth = sp.get("depth", rng.uniform(8, 12))
            Rc, tc = sc.Rt[f][c0 + av], sc.tt[f][c0 + av]
            P = Rc.T @ (sc.iK @ np.array([ax, ay, 1.0]) * depth - tc)
        views = []
        for k in range(nv):
            c = c0 + k
            if anchor is not None and k == anchor[0]:
                m = np.array([ax, ay], dtype=float)
            else:
                m = _project(sc.K, sc.Rt[f][c], sc.tt[f][c], P) + rng.normal(0, noise, 2)
            if sp.get("bad_view") == k:
                m = m + np.array([0.0, 40.0])
            s = take(c, m[0], m[1])
            if k in sp.get("dynamic_views", ()):
                is_static[c][s] = 0
            views.append((c, s))
        planted.append(views)
    plant_map_feats(only_absolute=False)
    # the existing map
    n_spec = len(map_points)
    nMap = n_spec if n_map is None else n_map
    assert nMap >= n_spec
    cap = nMap + (len(specs) + 16 if extra is None else extra)
    mapPts, mapCov = np.zeros((cap, 3)), np.zeros((cap, 9))
    mapPts[:nMap] = rng.uniform(-2, 2, (nMap, 3)) + np.array([0, 0, 10.0])
    mapCov[:nMap] = (0.01 * np.eye(3)).reshape(9)
    flags = np.zeros(cap, dtype=np.uint8)
    flags[:nMap] = 4                                     # (what carries no specification is uncertain: never a seed, never dynamic)
    pf = np.full((cap, nC), -1, dtype=np.int32)
    taken = {mp["index"] for mp in map_points if "index" in mp}
    assert len(taken) == sum("index" in mp for mp in map_points)
    free = (i for i in range(nMap) if i not in taken)
    for q, mp in enumerate(map_points):
        m = mp["index"] if "index" in mp else next(free)
        assert 0 <= m < nMap
        flags[m] = mp["flag"]
        for c, s in map_slots[q]:
            assert pf[m, c] < 0, "one feature per camera and map point"
            pf[m, c], s2m[c][s] = s, m
    # the candidate lists: the true links, scores on a grid of 0.01 (ties occur), shuffled
    pairs = []
    for a in range(nC - 1):
        lst = []
        for views in planted:
            d = dict(views)
            if a in d and a + 1 in d:
                lst.append((d[a], d[a + 1], 0.0, round(float(rng.uniform(0.8, 1.0)), 2)))
        order = rng.permutation(len(lst))
        pairs.append([lst[q] for q in order])
    S = dict(sc=sc, nC=nC, N=N, nMap=nMap, cap=cap, xy=xy, state=state, s2m=s2m, R=R, t=t, mapPts=mapPts, mapCov=mapCov, flags=flags, pf=pf,
             is_static=is_static, pairs=pairs, frame=f, planted=planted, map_slots=map_slots, specs=list(specs))
    if check:
        points_of(S, run_restatement(S, max_disp=1e9)[1], check=True)
    return S


def run_restatement(S, max_disp=1e9, min_len=2, max_seeds=512, c_form=False):
    """oracle.new_map_points_from_pairs (or its C form) on copies of S's arrays: (result, arrays)"""
    import oracle

    sc, nC, N = S["sc"], S["nC"], S["N"]
    cap = S["cap"]
    o = dict(mapPts=S["mapPts"].copy(), mapCov=S["mapCov"].copy(), flags=S["flags"].copy(), newPt=np.zeros(cap, np.uint8),
             first=np.zeros(cap, np.int32), pf=S["pf"].copy(), s2m=[x.copy() for x in S["s2m"]], reproj=[np.zeros(N) for _ in range(nC)])
    args = (N, S["pairs"], [sc.K] * nC, [sc.iK] * nC, S["R"], S["t"], S["xy"], S["state"], o["s2m"], S["is_static"], o["mapPts"], o["mapCov"],
            o["flags"], o["newPt"], o["first"], o["pf"], S["nMap"], S["frame"])
    kw = dict(max_disp=max_disp, min_len=min_len, max_seeds=max_seeds, W=W_IMG, H=H_IMG)
    if c_form:
        res = oracle.new_map_points_from_pairs_c(*args, **kw)
    else:
        res = oracle.new_map_points_from_pairs(*args, reproj=o["reproj"], **kw)
    return res, o


def points_of(S, o, min_len=2, check=False):
    """per track specification the map point the restatement made of it (-1: none).  check: a track without bad_view (and of at least
    min_len views) became a point that holds exactly its views, a track with bad_view became none"""
    out = []
    for sp, views in zip(S["specs"], S["planted"]):
        ms = {int(o["s2m"][c][s]) for c, s in views}
        m = ms.pop() if len(ms) == 1 else -2
        if m >= S["nMap"]:
            row = np.full(S["nC"], -1, dtype=np.int32)
            for c, s in views:
                row[c] = s
            assert np.array_equal(o["pf"][m], row), (sp, o["pf"][m])
        if check:
            want_point = sp.get("bad_view") is None and sp["nv"] >= min_len
            assert (m >= S["nMap"]) == want_point and m != -2, (sp, m)
        out.append(m if m >= S["nMap"] else -1)
    return out


def every_c0_nv(nC, min_nv=2):
    return [dict(c0=c0, nv=nv) for c0 in range(nC) for nv in range(min_nv, nC - c0 + 1)]


def second_register_set_specs(nC=16, two_view=False):
    """every long track (9 .. nC views, every admissible first camera) and the eight-view tracks in four variants: (a) clean; (b) a bad
    view at an index >= 8 only (eight views: view 6 or 7); (c) two DYNAMIC views, both at indices >= 8 (eight views: 6 and 7; nine views
    have ONE index >= 8, so they have no variant c); (d) one DYNAMIC view below 8 and one at or above (eight views: 0 and 7).
    `variant` is carried in the specification."""
    specs = []
    for nv in range(8, nC + 1):
        for c0 in range(0, nC - nv + 1):
            hi = list(range(8, nv)) if nv > 8 else [6, 7]
            # nine views have a single index >= 8: variant (c) needs two, so it starts at ten views (nine: 7 and 8, which is variant d's kind)
            two_hi = hi[-2:] if len(hi) >= 2 else None
            specs.append(dict(c0=c0, nv=nv, variant="a"))
            specs.append(dict(c0=c0, nv=nv, variant="b", bad_view=hi[(c0 + nv) % len(hi)]))
            if two_hi is not None:
                specs.append(dict(c0=c0, nv=nv, variant="c", dynamic_views=two_hi))
            specs.append(dict(c0=c0, nv=nv, variant="d", dynamic_views=[(c0 + nv) % min(nv, 8) if nv > 8 else 0, hi[-1]]))
    if two_view:
        specs += [dict(c0=c0, nv=2, variant="two") for c0 in range(nC - 1)]
        specs += [dict(c0=c0, nv=3, variant="three") for c0 in range(0, nC - 2, 3)]
    return specs


# ---- decidePointType's 20 px edge (SL_NewMapPointsInterCam.cpp:25-91), ten cameras ---------------------------------------------------
# Every track under test carries `expect`, the type the restatement must give its point, and sits on an integer pixel in the camera
# concerned.  The tracks under test are short (two cameras) so that nothing but the planted feature comes near them; this run's own
# dynamic points need ten views (two DYNAMIC ones at indices >= 8) and lie at depth 4, where a feature moves 25 to 35 px from one
# camera to the next, the tracks tested against them at depth 30, where it moves 20 px the other way.
OFFSETS = [((20, 0), 4), ((21, 0), 0), ((0, 20), 4), ((0, 21), 0), ((20, 20), 4), ((21, 21), 0), ((21, 20), 0), ((20, 21), 0),
           ((-20, 0), 4), ((-21, 0), 0), ((0, -20), 4), ((0, -21), 0)]


def decide_edge_scene(seed=41):
    nC, cam = 10, 3
    specs, mps = [], []
    near = dict(c0=cam, nv=2, depth=13.0)
    for q, ((dx, dy), want) in enumerate(OFFSETS):                          # (i) an existing certain dynamic point, same camera
        X, Y = 80 + 90 * (q % 6), 70 + 80 * (q // 6)
        mps.append(dict(flag=1, feats=[(cam, X, Y)]))
        specs.append(dict(near, anchor=(0, X + dx, Y + dy), expect=want, case="i"))
    for q, ((dx, dy), _) in enumerate(OFFSETS[:6]):                         # (ii) the dynamic feature is another camera's
        X, Y = 80 + 180 * (q % 3), (225, 25)[q // 3]
        mps.append(dict(flag=1, feats=[(cam + 4, X, Y)]))
        specs.append(dict(c0=cam, nv=5, depth=20.0, anchor=(0, X + dx, Y + dy), expect=0, case="ii"))
    dyn = dict(c0=0, nv=nC, depth=4.0, dynamic_views=[8, 9], expect=1, case="dyn")
    far = dict(nv=2, depth=30.0)
    # (iii) this run's own dynamic point, its feature in a camera >= 8: the tail of the list, camera in the top byte
    specs.append(dict(dyn, anchor=(9, 120, 300)))
    d9 = len(specs) - 1
    for (dx, dy), want in (((-20, 0), 4), ((-21, 0), 0), ((-20, -20), 4), ((-21, -20), 0), ((-20, -21), 0), ((0, 20), 4)):
        specs.append(dict(far, c0=8, anchor=(1, ("rel", d9, 9, dx, dy)), expect=want, case="iii"))
    specs.append(dict(dyn, anchor=(8, 400, 300)))
    d8 = len(specs) - 1
    for (dx, dy), want in (((20, 0), 4), ((21, 0), 0), ((0, 20), 4), ((0, 21), 0)):
        specs.append(dict(far, c0=8, anchor=(0, ("rel", d8, 8, dx, dy)), expect=want, case="iii"))
    # (iv) the same pixel in the camera beside: only the camera byte tells them apart
    for q, (c_dyn, c0_new, view, depth) in enumerate(((9, 7, 1, 30.0), (8, 8, 1, 4.0), (8, 6, 1, 30.0))):
        specs.append(dict(dyn, anchor=(c_dyn, 120 + 200 * q, 380)))
        specs.append(dict(c0=c0_new, nv=2, depth=depth, anchor=(view, ("rel", len(specs) - 1, c_dyn, 0, 0)), expect=0, case="iv"))
    # (v) a dynamic feature left of the image whose square reaches in (-15.5 rounds to -15: 19 px from x = 4; -17.5 to -17: 21 px)
    mps.append(dict(flag=1, feats=[(cam, -15.5, 70)]))
    specs.append(dict(near, anchor=(0, 4, 70), expect=4, case="v"))
    mps.append(dict(flag=1, feats=[(cam, -17.5, 150)]))
    specs.append(dict(near, anchor=(0, 4, 150), expect=0, case="v"))
    # (vi) a feature that rounds to x = -1 is skipped, whatever lies beside it (-1.6 + 0.5 truncates to -1; 0.4 rounds to 0 and counts)
    mps.append(dict(flag=1, feats=[(cam, 5, 225)]))
    specs.append(dict(near, anchor=(0, -1.6, 225), expect=0, case="vi"))
    mps.append(dict(flag=1, feats=[(cam, 5, 262)]))
    specs.append(dict(near, anchor=(0, 0.4, 262), expect=4, case="vi"))
    return planted_scene(nC, 250, seed, specs, map_points=mps, n_map=len(mps) + 5)


def expected_types_hold(S, o):
    """the restatement's type of every planted point is the specification's `expect`; returns the (case, type) combinations seen"""
    seen = set()
    for sp, m in zip(S["specs"], points_of(S, o)):
        if "expect" in sp:
            assert m >= 0 and int(o["flags"][m]) == sp["expect"], (sp, m, int(o["flags"][m]) if m >= 0 else None)
            seen.add((sp["case"], sp["expect"]))
    return seen


# ---- the seeds' segments (k_np_prep cuts the map into eight, k_np_match strings them together) ------------------------------------------
def seeds_capped_scene(seed=51):
    """a map of 4200 points (segments of 768): the first 700 are certain static and seen by all three cameras, so segment 0 alone holds
    more than 512 seeds; four `poison` seeds in later segments sit exactly on a track's feature in camera 0 with a disparity 300 px
    off -- used, each would reject its track's candidate of pair 0.  Tracks [0, 4) are the poisoned ones."""
    specs = [dict(c0=0, nv=3) for _ in range(40)] + [dict(c0=q % 2, nv=2) for q in range(20)]
    mps = [dict(flag=0, views=(0, 3), index=m) for m in range(700)]
    for q, m in enumerate((800, 1700, 3100, 4199)):
        mps.append(dict(flag=0, index=m, feats=[(0, ("rel", q, 0, 0, 0)), (1, ("rel", q, 1, 300, 0))]))
    return planted_scene(3, 790, seed, specs, map_points=mps, n_map=4200, check=False)


def seeds_spread_scene(seed=52):
    """a map of 1800 points (segments of 256, the last holds eight points): 300 seeds spread over all eight segments, no cap.  Six pairs
    of seeds lie on the SAME pixel of camera 0 (a track's feature) in different segments, one with the track's disparity, one 300 px
    off: the nearest seed is the first of equals in MAP order, so tracks 0, 2, 4 (the good one first) keep their candidate and
    1, 3, 5 lose it -- only if the segments are strung together in order."""
    specs = [dict(c0=0, nv=3) for _ in range(40)] + [dict(c0=q % 2, nv=2) for q in range(20)]
    idx = sorted(set(int(v) for v in np.linspace(0, 1799, 288)) | {1792, 1795})
    first = [100, 300, 600, 860, 1100, 1500]
    second = [400, 700, 1300, 1200, 1793, 1799]
    idx = [m for m in idx if m not in first + second]
    mps = [dict(flag=0, views=(0, 3), index=m) for m in idx]
    for q in range(6):
        good, bad = (first[q], second[q]) if q % 2 == 0 else (second[q], first[q])
        mps.append(dict(flag=0, index=good, feats=[(0, ("rel", q, 0, 0, 0)), (1, ("rel", q, 1, 1, 0))]))
        mps.append(dict(flag=0, index=bad, feats=[(0, ("rel", q, 0, 0, 0)), (1, ("rel", q, 1, 300, 0))]))
    return planted_scene(3, 410, seed, specs, map_points=mps, n_map=1800, check=False)


# ---- the dynamic features' lists (1024 per camera, 4096 in all) and the candidates' list (2048 per pair) --------------------------------
def dyn_list_scene(nC, N, per_cam, n_tracks, seed):
    """per_cam features of certain dynamic map points in EVERY camera (nC = 2: in camera 0 only), on a lattice of 4 px inside the image;
    the tracks run over all cameras, anchored on integer pixels all over the middle camera's image so that some fall inside the
    lattice's reach and some do not"""
    rng = np.random.default_rng(seed)
    cams = [0] if nC == 2 else list(range(nC))
    mps = []
    for c in cams:
        for q in range(per_cam):
            mps.append(dict(flag=1, feats=[(c, 60 + 4 * (q % 40), 100 + 4 * (q // 40))]))
    mid = 0 if nC == 2 else nC // 2
    specs = [dict(c0=0, nv=nC, anchor=(mid, int(rng.integers(30, 610)), int(rng.integers(30, 450)))) for _ in range(n_tracks)]
    return planted_scene(nC, N, seed, specs, map_points=mps)


def candidates_scene(n_pairs, seed=71):
    """two cameras, n_pairs one-to-one true candidates in ONE list, no seeds (every map point is uncertain)"""
    return planted_scene(2, 2304, seed, [dict(c0=0, nv=2) for _ in range(n_pairs)], n_map=50)
