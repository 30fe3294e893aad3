"""tests/register_rounds_ref.py (the second visits of the registration, played sequentially) against what is pinned already, and the table
sets the device tests of tests/test_register_wide_gpu.py run on:
  * a round over EVERY point with a feature, each in the loop of its first camera, is the single pass: it must leave what
    oracle.register_decide_static leaves (9, 12, 13 and 16 cameras);
  * the cover conditions of the device cases, asserted on the restatement alone: features attached (at most RvAttached's 256 a round),
    a point that registers and joins the next list, a chain of walks that takes more than two sweeps, and 0 / 1 / several conflicts.
Random tables give many conflicts and no long chain, so the seeds and densities in CASES were chosen here until the counts fitted, and three
things are put in by hand, each by its own rule (build): a chain of walks, candidates owned by points below mapBase, and -- for the cases
that want exactly 0 or 1 conflict -- the candidates behind the surplus conflicts struck from the search's table.  The expected values are
always the restatement's over the finished input.  The device tests import CASES, build() and expected()."""
import functools
import itertools

import numpy as np
import pytest

from tests.register_rounds_ref import _candidate, _kind, revisit_list, revisit_round, sweeps_to_settle
from tests.test_register_decide_gpu import _case


@pytest.mark.parametrize("C,seed,map_base", [(9, 21, 0), (12, 22, 7), (13, 23, 0), (16, 24, 3)])
def test_a_round_over_every_first_visit_is_the_single_pass(C, seed, map_base):
    import oracle

    P, N = 600, 150
    slot, flags, merg, mf, pf, s2m = _case(seed, P, C, N, 0.1)
    o_pf, o_s2m = pf.copy(), [x.copy() for x in s2m]
    att_o, reg_o = oracle.register_decide_static(slot, flags, merg, mf, o_pf, o_s2m, map_base=map_base, kinds=1)
    has = (pf >= 0).any(axis=1)
    lst = np.nonzero(has)[0]
    next_loop = np.where(has, (pf >= 0).argmax(axis=1), 0).astype(np.int32)
    att = np.zeros((P, C), dtype=np.uint8)
    visit = np.zeros(P, dtype=np.int32)
    r = revisit_round(slot, flags, merg, mf, pf, s2m, att, visit, next_loop, lst, 1, map_base, P, lst)
    assert att_o.sum() > 50
    assert np.array_equal(att, att_o) and np.array_equal(r["regOut"], reg_o) and np.array_equal(pf, o_pf)
    assert all(np.array_equal(s2m[c], o_s2m[c]) for c in range(C))
    assert r["counts"][:2] == [int(att_o.sum()), int(reg_o.sum())]
    assert np.array_equal(visit[reg_o == 1], next_loop[reg_o == 1])


# ---- the device cases.  C cameras, P points, N slots, cap: the lists' capacity; first: the firstRound form of the list; dens / dens2: share of the
# slots the first / the second search's candidates fall on; merge2: share of mergeable candidates in the second search; keep_reg: the share of the registered points that
# is marked for a second visit (default: all); conflicts: None as the tables give them, else candidates are struck from the second search until exactly that many are left; chain: a planted chain of walks
CASES = {
    "c9_cap64": dict(C=9, seed=102, P=700, N=300, cap=64, keep_reg=0.3, kinds=1, map_base=0, first=True, dens=0.25, dens2=0.9, merge2=0.5, conflicts=None, chain=True),
    "c12_cap256": dict(C=12, seed=201, P=900, N=300, cap=256, kinds=3, map_base=7, first=True, dens=0.3, dens2=0.9, merge2=0.4, conflicts=1, chain=False),
    "c13_cap320": dict(C=13, seed=301, P=2500, N=400, cap=320, kinds=2, map_base=0, first=False, dens=0.3, dens2=0.9, merge2=0.5, conflicts=0, chain=False),
    "c16_cap1024": dict(C=16, seed=401, P=3000, N=500, cap=1024, kinds=3, map_base=5, first=True, dens=0.3, dens2=0.5, merge2=0.3, conflicts=None, chain=True),
    "c8_cap256": dict(C=8, seed=501, P=900, N=300, cap=256, kinds=1, map_base=0, first=True, dens=0.3, dens2=0.9, merge2=0.5, conflicts=None, chain=True),
}
FREE_NEXT_ROWS = 3   # the device cases named in SHORT_NEXT hand the walks a next list with this many free rows: the joiners beyond are counted
SHORT_NEXT = ("c12_cap256",)


def _play(S):
    """the list and the round of the state S, played by the restatement on copies"""
    pf, s2m, att, visit = S["pf"].copy(), [x.copy() for x in S["s2m"]], S["att"].copy(), S["visit"].copy()
    reg_in, reg_out = S["reg"].copy(), np.ones(S["P"], np.uint8)
    L = revisit_list(pf, att, reg_in, False, reg_out, visit, None, S["cap"], S["first"])
    next_loop = np.full(S["P"], 77, np.int32)              # (77: what the device test fills the unlisted points' entries with)
    for p, b in L["nextLoop"].items():
        next_loop[p] = b
    lst = sorted(L["members"])
    after_list = dict(visit=visit.copy(), reg_in=reg_in.copy(), reg_out=reg_out.copy(), pf=pf.copy())
    sweeps = sweeps_to_settle(S["slot"], S["flags"], S["merg"], S["mf"], pf, s2m, next_loop, lst, S["kinds"])
    R = revisit_round(S["slot"], S["flags"], S["merg"], S["mf"], pf, s2m, att, visit, next_loop, lst, S["kinds"], S["map_base"], S["free_next"],
                      S["cur"], regOut=reg_out)
    return dict(list=L, round=R, pf=pf, s2m=s2m, att=att, visit=visit, reg_in=reg_in, reg_out=reg_out, next_loop=next_loop, sweeps=sweeps,
                after_list=after_list)


def _plant_chain(S, E):
    """Five listed points a < b < d, e (in the rounds' order) and four unmapped features nobody else looks at, in cameras i0 < i1 < i2 < i3
    where none of the five holds a feature: a takes X (i1); b takes Y (i0), is cut short at X -- and had Z (i2) behind it; d is cut short at Y
    (three walks each cut short by the one before); e takes Z and W (i3), which it reaches only once b's walk is known to end at X: after
    two sweeps the owners are not final."""
    C, N, slot, flags, merg = S["C"], S["N"], S["slot"], S["flags"], S["merg"]
    kind = 1 if S["kinds"] == 2 else 0
    order = sorted(E["list"]["members"], key=lambda p: (E["next_loop"][p], p))
    rows = [p for p in order if (int(S["mf"][p]) & 7) == kind]
    free = {p: [i for i in range(C) if S["pf"][p, i] < 0] for p in rows}
    found = None
    for kb, b in enumerate(rows):
        for i0, i1, i2 in itertools.combinations(free[b], 3):
            a = next((p for p in rows[:kb] if i1 in free[p]), None)
            d = next((p for p in rows[kb + 1:] if i0 in free[p]), None)
            e = next(((p, i3) for p in rows[kb + 1:] if p != d and i2 in free[p] for i3 in free[p] if i3 > i2), None)
            if a is not None and d is not None and e is not None:
                found = (a, b, d, e[0], (i0, i1, i2, e[1]))
                break
        if found:
            break
    assert found, "no rows to plant the chain in"
    a, b, d, e, cams = found
    four = (a, b, d, e)
    feats = []
    for i in cams:   # an unmapped slot of the camera; whoever else looked at it looks at nothing
        s = int(np.nonzero(S["s2m"][i] < 0)[0][-1])
        slot[slot[:, i] == s, i] = -3
        feats.append(s)
    (i0, i1, i2, i3), (Y, X, Z, W) = cams, feats
    for p in four:
        slot[p, :] = -3
    for p, i, s in ((a, i1, X), (b, i0, Y), (b, i1, X), (b, i2, Z), (d, i0, Y), (e, i2, Z), (e, i3, W)):
        slot[p, i], merg[p, i] = s, 1
        flags[p, i] = (flags[p, i] & ~2) | (2 * kind)


def below_base(S, members):
    """the candidates of the listed rows that carry a point of the map BELOW the pass's first (mapped all the same: the walk ends there)"""
    out = []
    for p in sorted(members):
        kind = _kind(S["mf"], p, S["kinds"])
        for i in range(S["C"]):
            sl = _candidate(S["slot"], S["flags"], S["pf"], p, i, S["N"], kind) if kind >= 0 else -1
            if sl >= 0 and 0 <= S["s2m"][i][sl] < S["map_base"]:
                out.append((p, i, sl))
    return out


def _plant_below_base(S, E):
    """every eighth listed row's first unmapped candidate is given to a point of the map below mapBase"""
    for p in sorted(E["list"]["members"])[::8]:
        kind = _kind(S["mf"], p, S["kinds"])
        for i in range(S["C"]):
            sl = _candidate(S["slot"], S["flags"], S["pf"], p, i, S["N"], kind) if kind >= 0 else -1
            if sl >= 0 and S["s2m"][i][sl] < 0:
                S["s2m"][i][sl] = p % S["map_base"]
                break


@functools.lru_cache(maxsize=None)
def build(name):
    """The state a round of second visits starts from: random search tables, the single pass over them (oracle.register_decide_static), then a
    SECOND search's tables (fresh candidates for every row: a listed point finds new ones, a current point's row says what it wanted)."""
    import oracle

    K = CASES[name]
    C, seed, P, N, cap, kinds, map_base = (K[k] for k in ("C", "seed", "P", "N", "cap", "kinds", "map_base"))
    slot, flags, merg, mf, pf, s2m = _case(seed, P, C, N, K["dens"], p_dyn=0.5 if kinds > 1 else 0.0)
    att, reg = oracle.register_decide_static(slot, flags, merg, mf, pf, s2m, map_base=map_base, kinds=kinds)
    if "keep_reg" in K:   # a short list over a long table: only this share of the points that registered is marked for a second visit
        reg[np.random.default_rng(seed + 3000).random(P) >= K["keep_reg"]] = 0
    slot2, flags2, _, _, _, _ = _case(seed + 1000, P, C, N, K["dens2"], p_dyn=0.5 if kinds > 1 else 0.0)
    rng = np.random.default_rng(seed + 2000)
    slot2[pf >= 0] = -1                                    # (the search leaves -1 where the point holds a feature)
    slot2[rng.random((P, C)) < 0.01] = N                   # no slot of the frame: passed by
    slot2[rng.random((P, C)) < 0.01] = N + 7
    merg2 = np.where(rng.random((P, C)) < K["merge2"], 1, rng.choice([0, 2], (P, C))).astype(np.uint8)
    visit0 = np.full(P, -5, np.int32)
    if not K["first"]:                                     # the later-round form reads the loop of the latest registering visit
        visit0 = np.zeros(P, np.int32)
        revisit_list(pf, att, reg.copy(), True, None, visit0, None, cap, True)
    cur = np.nonzero((pf >= 0).any(axis=1) & ((mf & 2) == 0))[0].astype(np.int32)
    S = dict(C=C, P=P, N=N, cap=cap, kinds=kinds, map_base=map_base, first=K["first"], slot=slot2, flags=flags2, merg=merg2, mf=mf, pf=pf, s2m=s2m,
             att=att, reg=reg, visit=visit0, cur=cur, free_next=FREE_NEXT_ROWS if name in SHORT_NEXT else cap)
    if map_base > 0:
        _plant_below_base(S, _play(S))
    if K["chain"]:
        _plant_chain(S, _play(S))
    if K["conflicts"] is not None:   # strike the candidates behind the conflicts, one at a time, until the wanted number is left
        for _ in range(200):
            R = _play(S)["round"]
            if R["counts"][2] <= K["conflicts"]:
                break
            q, i = R["witness"][-1]
            slot2[q, i] = -3
        assert _play(S)["round"]["counts"][2] == K["conflicts"]
    for v in list(S.values()) + S["s2m"]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def expected(name):
    """the list and the round of build(name), played by the restatement (computed once; nobody writes to it)"""
    return _play(build(name))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_device_case_attaches_registers_and_fits(name):
    S, E = build(name), expected(name)
    n_att, n_reg, _ = E["round"]["counts"]
    assert E["list"]["overflow"] == 0 and 20 <= len(E["list"]["members"]) <= S["cap"], len(E["list"]["members"])
    assert 20 <= n_att <= 256, n_att                      # RvAttached holds 256: the conflict scan sees no more
    assert n_reg >= 1 and len(E["round"]["next"]) >= 1
    assert len(S["cur"]) > 2 * max(256, (S["cap"] + 63) // 64 * 64)   # the scan reads rows beyond the two a thread asked for ahead
    if S["free_next"] < S["cap"]:
        assert E["round"]["overflow"] >= 1
    if S["map_base"] > 0:   # features carried by a point of the map below the pass's first: mapped all the same
        assert len(below_base(S, E["list"]["members"])) >= 5
    if S["kinds"] > 1:
        assert (E["reg_out"][(S["mf"] & 7) == 1] == 1).any()   # a certainly dynamic point registered


def test_the_device_cases_cover_long_chains_and_every_conflict_count():
    E = {n: expected(n) for n in CASES}
    wide = [n for n in CASES if CASES[n]["C"] > 8]
    conflicts = sorted(E[n]["round"]["counts"][2] for n in wide)
    assert 0 in conflicts and 1 in conflicts and max(conflicts) >= 3, conflicts
    # a chain that takes more than two sweeps: three walks each cut short by the one before, and owners that are not final after two sweeps
    assert any(E[n]["round"]["chain"] >= 2 and E[n]["sweeps"] >= 4 for n in wide), {n: (E[n]["round"]["chain"], E[n]["sweeps"]) for n in wide}
    lens = {n: len(E[n]["list"]["members"]) for n in CASES}
    assert lens["c13_cap320"] > 256 and lens["c16_cap1024"] > 320, lens   # (rows in the threads beyond the first 256 / 320)
