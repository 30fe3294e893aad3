"""cs_newpts_from_pairs_dev where the suite never went: tracks of 9 to 16 views (the SECOND register set of k_np_reconstruct's eight
lanes per track), every (first camera, length), minLen 3, decidePointType's 20 px edge with the tail list of this run's own dynamic
points, k_np_prep's eight map segments and the 512-seed cap, the dynamic features' lists at 1024 per camera and 4096 in all, and a
candidate list beyond 2048 -- on planted scenes (tests/newpts_planted.py), against oracle.new_map_points_from_pairs, bit for bit."""
import numpy as np
import pytest

from tests import newpts_planted as P
from tests.test_newpts_gpu import _run_both, _same_map, _scene

pytestmark = pytest.mark.gpu


def _same_counts(res, g, nC, min_len=2, flags=0):
    """counts[0..3] and the matches of every pair"""
    out = g["out"]
    assert out[0] == len(res["new"]) and out[1] == len(res["tracks"]) and out[2] == sum(len(t) >= min_len for t in res["tracks"]), out
    assert out[3] == flags, out
    assert out[4:4 + nC - 1] == [int((res["matches"][a] >= 0).sum()) for a in range(nC - 1)]
    assert g["count"] == res["map_count"]
    for a in range(nC - 1):
        has = res["matches"][a] >= 0
        assert np.array_equal(g["rows"][a], has) and np.array_equal(g["match"][a][has], res["matches"][a][has]), a


def _equal(S, max_disp=1e9, min_len=2, flags=0):
    res, o, g = _run_both(S, max_disp, min_len=min_len)
    _same_counts(res, g, S["nC"], min_len, flags)
    _same_map(o, g, S["nC"])
    return res, o, g


@pytest.mark.parametrize("nC", [9, 10, 12, 16])
def test_every_first_camera_and_length(hip, nC):
    """one track for every first camera c0 and every length nv >= 2, 250 features a camera (the last mask word is partial).  A track
    with c0 >= 1 and nv >= 9 has a view whose lane holds it in the second register set while the lane's own column of pointFeat
    belongs to the first: nine cameras have none (the control), ten have one."""
    S = P.planted_scene(nC, 250, 100 + nC, P.every_c0_nv(nC))
    res, o, g = _equal(S)
    assert len(res["new"]) == len(S["specs"]) == nC * (nC - 1) // 2
    crossed = sum(1 for t in res["tracks"] if t[0][0] >= 1 and len(t) >= 9)
    assert crossed == (0 if nC == 9 else (nC - 9) * (nC - 8) // 2)


def _variants(S, o):
    by = {}
    for sp, m in zip(S["specs"], P.points_of(S, o)):
        by.setdefault(sp["variant"], []).append((sp, m))
    return by


def test_second_register_set_decides(hip):
    """16 cameras: every long track in four variants -- clean, an outlier view at an index >= 8 only, two DYNAMIC views at indices >= 8,
    one below 8 and one above -- and the eight-view tracks likewise: the gate and the point's type come out of views 8..15"""
    S = P.planted_scene(16, 250, 7, P.second_register_set_specs(16))
    res, o, g = _equal(S)
    by = _variants(S, o)
    assert len(by["a"]) == len(by["b"]) == len(by["d"]) == 45 and len(by["c"]) == 37
    assert all(m >= 0 and o["flags"][m] in (0, 4) for _, m in by["a"]) and all(m < 0 for _, m in by["b"])
    assert all(sp["bad_view"] >= (8 if sp["nv"] > 8 else 6) for sp, _ in by["b"])
    assert all(m >= 0 and o["flags"][m] == 1 for _, m in by["c"] + by["d"])
    assert all(min(sp["dynamic_views"]) >= 8 for sp, _ in by["c"] if sp["nv"] > 8)
    assert all(min(sp["dynamic_views"]) < 8 <= max(sp["dynamic_views"]) for sp, _ in by["d"] if sp["nv"] > 8)


def test_second_register_set_with_min_len_three(hip):
    """the same with minLen = 3 on a scene that also holds two-view tracks: they are counted as tracks, not as long ones, none becomes
    a point"""
    S = P.planted_scene(16, 250, 8, P.second_register_set_specs(16, two_view=True))
    res, o, g = _equal(S, min_len=3)
    by = _variants(S, o)
    assert len(by["two"]) == 15 and all(m < 0 for _, m in by["two"]) and all(m >= 0 for _, m in by["three"] + by["a"])
    assert g["out"][2] == sum(len(t) >= 3 for t in res["tracks"]) == g["out"][1] - 15
    assert all((o["pf"][m] >= 0).sum() >= 3 for m in res["new"])


def test_decide_point_type_edge(hip):
    """20 px keeps a new point uncertain, 21 px (on either axis) makes it certain static; another camera's dynamic feature does not
    count; this run's own dynamic points count through the tail list, in their own camera only; a square that reaches in from outside
    the image counts, a feature that rounds to x = -1 is skipped"""
    S = P.decide_edge_scene()
    seen = P.expected_types_hold(S, P.run_restatement(S)[1])
    assert seen == {("dyn", 1), ("i", 0), ("i", 4), ("ii", 0), ("iii", 0), ("iii", 4), ("iv", 0), ("v", 0), ("v", 4), ("vi", 0), ("vi", 4)}
    _equal(S)


def test_seed_cap_over_all_segments(hip):
    """532 and 534 seeds of a pair, in all eight 256-point segments: the first 512 in map order are the seeds"""
    import oracle

    S = _scene(31, nC=3, N=2048, nMap=1800, extra=600)
    sc, nC = S["sc"], S["nC"]
    for a in range(nC - 1):
        seeds = np.nonzero(((S["flags"][:S["nMap"]] & 6) == 0) & (S["pf"][:S["nMap"], a] >= 0) & (S["pf"][:S["nMap"], a + 1] >= 0))[0]
        assert len(seeds) > 512 and np.all(np.bincount(seeds // 256, minlength=8) > 0)
    m = []
    for max_seeds in (512, 10 ** 9):       # (the C form: it is the Python restatement's equal, tests/test_oracle_cpu.py, and quick)
        s2m = [x.copy() for x in S["s2m"]]
        r = oracle.new_map_points_from_pairs_c(S["N"], S["pairs"], [sc.K] * nC, [sc.iK] * nC, S["R"], S["t"], S["xy"], S["state"], s2m, S["is_static"],
                                               S["mapPts"].copy(), S["mapCov"].copy(), S["flags"].copy(), np.zeros(S["cap"], np.uint8),
                                               np.zeros(S["cap"], np.int32), S["pf"].copy(), S["nMap"], S["frame"], max_disp=25.0, max_seeds=max_seeds)
        m.append(r["matches"])
    assert not np.array_equal(m[0], m[1])                                   # (or the test could not see the cap)
    res, o, g = _run_both(S, 25.0)
    assert np.array_equal(res["matches"], m[0])
    _same_counts(res, g, nC)
    _same_map(o, g, nC)


def test_first_segment_alone_fills_the_seeds(hip):
    """a map of 4200 points whose first segment holds 700 seeds: the scan stops there, the seeds planted in later segments -- each
    would cost a track its candidate -- are not used"""
    S = P.seeds_capped_scene()
    first = [S["planted"][q][0][1] for q in range(4)]
    capped, _ = P.run_restatement(S, max_disp=80.0)
    free, _ = P.run_restatement(S, max_disp=80.0, max_seeds=10 ** 9)
    assert all(capped["matches"][0][s] >= 0 for s in first) and all(free["matches"][0][s] < 0 for s in first)
    res, o, g = _equal(S, max_disp=80.0)
    assert all(g["match"][0][s] == capped["matches"][0][s] and g["rows"][0][s] for s in first)


def test_seeds_strung_together_in_map_order(hip):
    """300 seeds over all eight segments of a map of 1800, no cap: of two seeds on the same pixel in different segments the first in
    MAP order is the nearest"""
    S = P.seeds_spread_scene()
    seeds = np.nonzero(((S["flags"][:1800] & 6) == 0) & (S["pf"][:1800, 0] >= 0) & (S["pf"][:1800, 1] >= 0))[0]
    assert 280 <= len(seeds) <= 320 and np.all(np.bincount(seeds // 256, minlength=8) > 0)
    res, o, g = _equal(S, max_disp=80.0)
    kept = [bool(res["matches"][0][S["planted"][q][0][1]] >= 0) for q in range(6)]
    assert kept == [True, False, True, False, True, False]


@pytest.mark.parametrize("nC,N,per_cam,n_tracks,seed,over", [(2, 1200, 1024, 80, 61, False), (2, 1200, 1100, 80, 62, True), (5, 1024, 1000, 24, 63, True)])
def test_dynamic_lists_at_their_limits(hip, nC, N, per_cam, n_tracks, seed, over):
    """1024 features of certain dynamic points in one camera fit; 1100 do not, nor do 5 x 1000 in all: flag bit 2, the lists are cut in
    arrival order, so a new point may miss its dynamic neighbour (certain static where the restatement says uncertain) but never
    finds one that is not there; everything else is the restatement's"""
    S = P.dyn_list_scene(nC, N, per_cam, n_tracks, seed)
    res, o, g = _run_both(S, 1e9)
    types = o["flags"][res["new"]]
    assert (types == 4).sum() >= 3 and (types == 0).sum() >= 3
    _same_counts(res, g, nC, flags=4 if over else 0)
    if over:
        new = np.asarray(res["new"])
        got, want = g["flags"][new], o["flags"][new]
        assert np.all((got == want) | ((got == 0) & (want == 4)))
        g["flags"][new] = want
    _same_map(o, g, nC)


def test_exactly_2048_candidates_fit(hip):
    S = P.candidates_scene(2048)
    res, o, g = _equal(S)
    assert g["out"][4] == 2048 == len(res["new"])


def test_more_than_2048_candidates_are_cut_and_flagged(hip):
    """2100 one-to-one candidates of one pair: 2048 of them survive, which ones depends on arrival order -- every match made is the
    uncut restatement's match of that row, every new point is one of its points"""
    S = P.candidates_scene(2100)
    N, nMap = S["N"], S["nMap"]
    res, o, g = _run_both(S, 1e9)
    assert len(res["new"]) == 2100
    out = g["out"]
    assert out[3] & 1 and out[3] & ~1 == 0 and out[4] == 2048 and out[0] == out[1] == out[2] == 2048 and g["count"] == nMap + 2048
    rows = g["rows"][0]
    assert rows.sum() == 2048 and np.array_equal(g["match"][0][rows], res["matches"][0][rows])
    theirs = {(int(o["pf"][m, 0]), int(o["pf"][m, 1])): m for m in res["new"]}
    seen = set()
    for m in range(nMap, nMap + 2048):
        row = (int(g["pf"][m, 0]), int(g["pf"][m, 1]))
        assert row in theirs and row not in seen and rows[row[0]] and g["match"][0][row[0]] == row[1]
        seen.add(row)
        q = theirs[row]
        assert np.array_equal(g["mapPts"][m], o["mapPts"][q]) and np.array_equal(g["mapCov"][m], o["mapCov"][q])
        assert g["flags"][m] == o["flags"][q] == 0 and g["newPt"][m] == 1 and g["first"][m] == o["first"][q]
        for c in range(2):
            assert g["s2m"][c][row[c]] == m and g["reproj"][c][row[c]] == o["reproj"][c][row[c]]
    # the points come in track order: by the feature of the first camera
    assert np.all(np.diff(g["pf"][nMap:nMap + 2048, 0]) > 0)
    # nothing else was touched
    assert np.array_equal(g["flags"][:nMap], S["flags"][:nMap]) and not g["newPt"][nMap + 2048:].any() and np.all(g["pf"][nMap + 2048:] == -1)
    for c in range(2):
        untouched = np.ones(N, dtype=bool)
        untouched[[r[c] for r in seen]] = False
        assert np.array_equal(g["s2m"][c][untouched], S["s2m"][c][untouched]) and not g["reproj"][c][untouched].any()
