"""The cover conditions of tests/intracam_scenes.py, on the scenes and the C oracle alone: without them a green
tests/test_intracam_newpts_gpu.py could be vacuous.  (The oracle itself is held to the reference's own SingleSLAM::newMapPoints by
tests/test_oracle_cpu.py::test_intracam_new_map_points_restatement_reproduces_the_reference, with its walk unbounded.)"""
import numpy as np
import pytest

from tests import intracam_scenes as IS


@pytest.mark.parametrize("name", list(IS.SPECS))
def test_scene_meets_its_cover_conditions_at_the_first_seed_that_does(name):
    """Every admitted camera: candidates (the prefilter of src/app/SL_SingleSLAM.cpp:159 / :938-944, counted in numpy) > successes >= 5,
    every kind of slot present, tracks of minTrackLen - 1 and of minTrackLen frames among them; the scene's own conditions (below); and
    the committed seed is the first of 0, 1, 2, ... at which all of it holds."""
    S = IS.scene(name)
    cv = S["cover"]
    print(name, cv)
    assert IS.find_seed(name) == IS.SEEDS[name]
    E = IS.expect(S)
    assert E["candidates"] == sum(cv["candidates"]) > len(E["slot"]) == cv["A"]
    # (camera, slot) order, one point per slot, and only candidates succeed
    e = E["camera"].astype(np.int64) * S["N"] + E["slot"]
    assert (np.diff(e) > 0).all()
    for c in range(S["nC"]):
        assert set(E["slot"][E["camera"] == c]) <= set(IS.candidates(S, c))


def test_several_commit_passes_hold_successes():
    """two_pass: 1024 + 576 entries; ragged: 1024 + 11 (the last 11 slots of camera 8); sixteen: 1024 + 1024 + 16 -- at least 2 successes
    in every pass, and in two_pass room for a capacity cut on either side of the pass boundary."""
    for name, sizes in (("two_pass", (1024, 576)), ("ragged", (1024, 11)), ("sixteen", (1024, 1024, 16))):
        S = IS.scene(name)
        total = S["nC"] * S["N"]
        assert tuple(min(IS.PASS, total - p * IS.PASS) for p in range(len(sizes))) == sizes
        passes = IS.per_pass(S, IS.expect(S))
        assert len(passes) == len(sizes) and (passes >= 2).all(), (name, passes)
    S = IS.scene("ragged")
    E = IS.expect(S)
    last = E["slot"][E["camera"] == 8]
    assert (last >= S["N"] - 11).sum() >= 2
    cv = IS.scene("two_pass")["cover"]
    assert 2 <= cv["a1"] - 1 and cv["a1"] + 1 <= cv["A"] - 1


def test_three_cameras_ready_masks_select_what_they_should():
    """d_ready = [0, 2, 1]: readyMin 1 admits cameras 1 and 2, readyMin 2 camera 1 alone; [0, 0, 0] nobody -- and every one of these
    expectations differs from the others."""
    S = IS.scene("three")
    full = IS.expect(S)
    e1, e2, e0 = IS.expect(S, ready=[0, 2, 1], readyMin=1), IS.expect(S, ready=[0, 2, 1], readyMin=2), IS.expect(S, ready=[0, 0, 0], readyMin=1)
    assert sorted(set(e1["camera"])) == [1, 2] and sorted(set(e2["camera"])) == [1] and len(e0["slot"]) == 0 and e0["candidates"] == 0
    assert len(full["slot"]) > len(e1["slot"]) > len(e2["slot"]) >= 5
    assert full["candidates"] > e1["candidates"] > e2["candidates"] > 0
    assert len({tuple(S["K"][c]) for c in range(3)}) == 3


def test_deep_walk_bounds_are_visible():
    """deep: jp up to 99 over a centre table of 64 depths.  The expectation differs between maxWalk 2 and 3 and between 64 and 65; it
    ALSO differs between 65 and 1024, because points whose oldest view lies at depth >= 65 succeed (they would agree only if none did);
    1024 is the unbounded walk; at least 10 successes have jp >= 64."""
    S = IS.scene("deep")
    assert S["walk"] == 64 and S["stored"] == 100
    E = {w: IS.expect(S, maxWalk=w) for w in IS.DEEP_WALKS}
    diff = lambda a, b: not (np.array_equal(a["slot"], b["slot"]) and np.array_equal(a["M"], b["M"]) and np.array_equal(a["cov"], b["cov"]))   # noqa: E731
    assert diff(E[2], E[3]) and diff(E[64], E[65]) and diff(E[65], E[1024])
    assert not diff(E[1024], IS.expect(S))
    jp = IS.jp_of(S, E[1024])
    assert (jp >= 64).sum() >= 10 and (jp >= 65).sum() >= 1 and (jp < 64).sum() >= 10
    # the bound leaves the first triangulation's oldest view alone: the same first frames wherever the same slot succeeds
    for w in IS.DEEP_WALKS:
        both = np.intersect1d(E[w]["camera"] * S["N"] + E[w]["slot"], E[1024]["camera"] * S["N"] + E[1024]["slot"])
        fw = dict(zip((E[w]["camera"] * S["N"] + E[w]["slot"]).tolist(), E[w]["first"].tolist()))
        f0 = dict(zip((E[1024]["camera"] * S["N"] + E[1024]["slot"]).tolist(), E[1024]["first"].tolist()))
        # (a walk of two or three nodes pairs the current view with its neighbours: hardly any baseline, few points survive)
        assert len(both) >= (10 if w >= 64 else 2) and all(fw[q] == f0[q] for q in both.tolist())


def test_wrapped_ring_clamps_to_the_store():
    """wrapped: 75 frames into a store of 48 -- the head wraps, 27 frames are overwritten.  At least 20 candidates are older than the
    store (their points' first frame is f2 - 47, the oldest frame that still has a pose), at least 20 younger, successes of both kinds;
    over all 75 frames the expectation is another one."""
    S = IS.scene("wrapped")
    cv = S["cover"]
    assert S["T"] == 75 and S["stored"] == 48
    assert sum(cv["older_than_store"]) >= 20 and sum(cv["younger"]) >= 20
    E, Eall = IS.expect(S), IS.expect(S, stored=75)
    assert (E["first"] == S["cur"] - 47).sum() >= 5 and (E["first"] > S["cur"] - 47).sum() >= 5 and E["first"].min() == S["cur"] - 47
    assert Eall["first"].min() < S["cur"] - 47
    assert not (len(E["M"]) == len(Eall["M"]) and np.array_equal(E["M"], Eall["M"]))


def test_still_cameras_tie_and_degenerate():
    """still, camera 0 (stood still for its oldest 70 frames): for at least 10 of its points the walk's smallest cosine -- recomputed in
    numpy binary64 in the oracle's expression order -- is attained at two or more depths, among them a pair 64 apart (one lane of the
    device's walk meets both) and a pair not a multiple of 64 apart (two lanes); the first of them is the still stretch's newest frame.
    Camera 1 (never moved): at least 10 candidates and no point.  Camera 2 is the control."""
    S = IS.scene("still")
    ties = IS.still_ties(S)
    n = 0
    for _k, depths in ties:
        d = depths[:, None] - depths[None, :]
        if len(depths) >= 2 and (d == 64).any() and ((d > 0) & (d % 64 != 0)).any():
            assert depths[0] == IS.STILL_FROM
            n += 1
    assert n >= 10
    E = IS.expect(S)
    assert len(IS.candidates(S, 1)) >= 10 and (E["camera"] == 1).sum() == 0
    assert (E["camera"] == 0).sum() >= 10 and (E["camera"] == 2).sum() >= 10
    # the tie-break matters: a walk that ends before the still stretch's second frame makes other points
    assert not np.array_equal(IS.expect(S, maxWalk=IS.STILL_FROM)["M"], E["M"])


def test_walk_bound_of_the_oracle():
    """opu_intracam_new_points_walk's maxWalk (oracle.intracam_new_points(maxWalk=...)): None (the unbounded entry), 0 and anything
    beyond the longest track are the unbounded walk; a bound of one node keeps the first triangulation (no refinement), so every point it makes passes the same gates with the same first frame."""
    S = IS.scene("deep")
    E = IS.expect(S)
    for w in (0, -3, 100, 1 << 20):
        Ew = IS.expect(S, maxWalk=w)
        assert np.array_equal(Ew["slot"], E["slot"]) and np.array_equal(Ew["M"], E["M"]) and np.array_equal(Ew["cov"], E["cov"]), w
    E1 = IS.expect(S, maxWalk=1)
    assert len(E1["slot"]) >= 10 and S["cover"]["refined_elsewhere"] >= 5
