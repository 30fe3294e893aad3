"""The registration's search, current-points list and second visits at 9 to 16 cameras -- the paths no frame loop of the suite takes (every
rig there has at most 8 cameras): k_register_search at feature counts on the staging boundary and over camera ranges of 16-wide tables,
k_register_list's three row readers, and k_revisit_list / k_revisit_decide<16> against the sequential walk of tests/register_rounds_ref.py.
Every input is a small table or a small synthetic rig; every expected value comes from oracle/ or from plain Python.  Integers, bytes and
bit-for-bit doubles throughout."""
import functools

import numpy as np
import pytest

import coslam_amd
import oracle
from tests.register_rounds_ref import _candidate, _kind
from tests.test_register_gpu import H, MODES, PIXEL_ERR_VAR, W, _rig, assert_tables_equal
from tests.test_register_rounds_ref_cpu import CASES, build, expected

pytestmark = pytest.mark.gpu

TABLES = ("slot", "flags", "m", "var", "dist")


# ---- the search ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rig_of(n_cams, N, P):
    return _rig(n_cams, N, P, seed=300 + 17 * n_cams + N)


@functools.lru_cache(maxsize=None)
def _oracle_of(n_cams, N, P, mode):
    Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf = _rig_of(n_cams, N, P)
    return oracle.register_search(W, H, Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf, *MODES[mode])


@pytest.mark.parametrize("mode", ["static", "dynamic", "active"])
@pytest.mark.parametrize("n_cams,N,P", [(9, 513, 65), (12, 512, 64), (13, 1025, 130), (16, 513, 130), (16, 1, 1)])
def test_search_at_nine_to_sixteen_cameras_on_the_staging_boundary(hip, mode, n_cams, N, P):
    """N = 512: one full stage; 513 and 1025: a last stage of ONE feature; P = 65 and 130: a last tile of one and two points"""
    Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf = _rig_of(n_cams, N, P)
    o = _oracle_of(n_cams, N, P, mode)
    g = coslam_amd.register_search(W, H, Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf, *MODES[mode])
    assert_tables_equal(g, o, f"{mode} {n_cams}x{N}x{P}")
    if P > 1:
        assert (o["slot"] >= 0).sum() > P and (o["slot"][:, n_cams - 1] >= 0).any()


def test_search_with_an_empty_camera_and_a_list_that_ends_on_its_last_slot(hip):
    """camera 10 of 12 has no feature in this frame: every pair searched there answers -4; camera 11's only live slot is N - 1, the one
    feature of the last stage (N = 513): every pair searched there finds it; camera 3's slot N - 1 is live among the others"""
    n_cams, N, P = 12, 513, 65
    Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf = _rig_of(n_cams, N, P)
    state = [s.copy() for s in state]
    state[10][:] = -1
    state[11][:] = -1
    state[11][N - 1] = 0
    state[3][N - 1] = 1
    sS, mD, sM = MODES["static"]
    o = oracle.register_search(W, H, Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf, sS, mD, sM)
    g = coslam_amd.register_search(W, H, Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf, sS, mD, sM)
    assert_tables_equal(g, o, "empty camera / last slot")
    full = _oracle_of(n_cams, N, P, "static")["slot"]
    searched = full >= 0            # (the pairs that are searched do not depend on the lists)
    assert searched[:, 10].sum() > 5 and (g["slot"][searched[:, 10], 10] == -4).all() and not (g["slot"][:, 10] >= 0).any()
    assert searched[:, 11].sum() > 5 and (g["slot"][searched[:, 11], 11] == N - 1).all()


class _DevRig:
    """a rig's records on the device and the cs_register_cam array over them"""

    def __init__(self, n_cams, N, P):
        import torch

        self.n_cams, self.N, self.P = n_cams, N, P
        Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf = _rig_of(n_cams, N, P)
        self.dev = torch.device("cuda:0")
        d = self.d
        self.K, self.R, self.t = d(Ks.reshape(n_cams, 9)), d(Rs.reshape(n_cams, 9)), d(ts)
        self.xy, self.st, self.s2m, self.dyn = [d(a) for a in xy], [d(a) for a in state], [d(a) for a in s2m], [d(a) for a in dyn]
        self.cams = [dict(K=self.K[c].data_ptr(), R=self.R[c].data_ptr(), t=self.t[c].data_ptr(), xy=self.xy[c].data_ptr(), state=self.st[c].data_ptr(),
                          slot2map=self.s2m[c].data_ptr(), isDynamic=self.dyn[c].data_ptr()) for c in range(n_cams)]
        self.M, self.cov, self.pf = d(Ms), d(covs.reshape(P, 9)), d(pf)
        self.stream = torch.cuda.current_stream().cuda_stream

    def d(self, a):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def tables(self, rows=None):
        """output tables full of sentinels"""
        import torch

        n, C = self.P if rows is None else rows, self.n_cams
        return dict(slot=torch.full((n, C), -77, dtype=torch.int32, device=self.dev), flags=torch.full((n, C), -77, dtype=torch.int32, device=self.dev),
                    m=torch.full((n, C, 2), 7.5, dtype=torch.float64, device=self.dev), var=torch.full((n, C, 4), 7.5, dtype=torch.float64, device=self.dev),
                    dist=torch.full((n, C), 7.5, dtype=torch.float64, device=self.dev))

    def a_pass(self, T, mode, P=None, **more):
        sS, mD, sM = MODES[mode]
        return dict(P=self.P if P is None else P, sigmaSearch=sS, maxDist=mD, sigmaMerge=sM, M=self.M.data_ptr(), cov=self.cov.data_ptr(),
                    pointFeat=self.pf.data_ptr(), **{k: T[k].data_ptr() for k in TABLES}, **more)


def _host(T):
    return {k: T[k].cpu().numpy() for k in TABLES}


def test_search_over_camera_ranges_of_sixteen_wide_tables(hip):
    """cs_register_search_passes_range_dev: the columns of cameras cam0 .. cam0 + nCamsRun - 1 are the full run's (which is the oracle's),
    every other column keeps what the caller wrote"""
    import torch

    from coslam_amd.register import register_search_passes_dev

    n_cams, N, P = 16, 513, 130
    G = _DevRig(n_cams, N, P)
    full = G.tables()
    register_search_passes_dev(G.stream, G.cams, N, W, H, [G.a_pass(full, "static")], cam0=0, nCamsRun=16)
    torch.cuda.synchronize()
    full = _host(full)
    assert_tables_equal(full, _oracle_of(n_cams, N, P, "static"), "range (0, 16)")
    for cam0, n_run in ((9, 7), (15, 1), (5, 0)):
        T = G.tables()
        register_search_passes_dev(G.stream, G.cams, N, W, H, [G.a_pass(T, "static")], cam0=cam0, nCamsRun=n_run)
        torch.cuda.synchronize()
        T = _host(T)
        inside = np.zeros(n_cams, dtype=bool)
        inside[cam0:cam0 + n_run] = True
        for k in TABLES:
            assert np.array_equal(T[k][:, inside], full[k][:, inside]), (cam0, n_run, k)
            sentinel = -77 if k in ("slot", "flags") else 7.5
            assert (T[k][:, ~inside] == sentinel).all(), (cam0, n_run, k)
    with pytest.raises(coslam_amd.CoslamHipError):
        register_search_passes_dev(G.stream, G.cams, N, W, H, [G.a_pass(G.tables(), "static")], cam0=9, nCamsRun=8)


def test_two_passes_in_one_launch_at_thirteen_cameras(hip):
    """the static scale over all 130 rows and the dynamic scale with mapFlags over a compact list of 70 of them, in ONE launch: each pass
    leaves the bytes of its own launch -- and the unlisted rows of the list pass's tables keep the caller's"""
    import torch

    from coslam_amd.register import register_search_passes_dev

    n_cams, N, P = 13, 1025, 130
    G = _DevRig(n_cams, N, P)
    rng = np.random.default_rng(5)
    mf = np.where(rng.random(P) < 0.4, 1, rng.choice([0, 2, 4, 5], P)).astype(np.uint8)
    rows = np.sort(rng.choice(P, 70, replace=False)).astype(np.int32)
    d_mf, d_list = G.d(mf), G.d(rows)
    more = dict(mapFlags=d_mf.data_ptr(), maxDistDynamic=5 * PIXEL_ERR_VAR, list=d_list.data_ptr())
    sep, fus = [G.tables(), G.tables()], [G.tables(), G.tables()]
    register_search_passes_dev(G.stream, G.cams, N, W, H, [G.a_pass(sep[0], "static")])
    register_search_passes_dev(G.stream, G.cams, N, W, H, [G.a_pass(sep[1], "dynamic", P=70, **more)])
    register_search_passes_dev(G.stream, G.cams, N, W, H, [G.a_pass(fus[0], "static"), G.a_pass(fus[1], "dynamic", P=70, **more)])
    torch.cuda.synchronize()
    for a, b in zip(sep, fus):
        for k in TABLES:
            assert np.array_equal(a[k].cpu().numpy().view(np.uint8), b[k].cpu().numpy().view(np.uint8)), k
    assert_tables_equal(_host(fus[0]), _oracle_of(n_cams, N, P, "static"), "pass 0")
    sl = fus[1]["slot"].cpu().numpy()
    unlisted = np.setdiff1d(np.arange(P), rows)
    assert (sl[unlisted] == -77).all() and (sl[rows] != -77).all() and (sl[rows] >= 0).sum() > 70
    # the certainly dynamic points were searched with their own scale, every other listed point with the pass's
    Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf = _rig_of(n_cams, N, P)
    sS, mD, sM = MODES["dynamic"]
    o_pass, o_dyn = _oracle_of(n_cams, N, P, "dynamic"), oracle.register_search(W, H, Ks, Rs, ts, xy, state, s2m, dyn, Ms, covs, pf, sS, 5 * PIXEL_ERR_VAR, sM)
    dyn_rows, rest = rows[(mf[rows] & 7) == 1], rows[(mf[rows] & 7) != 1]
    g = _host(fus[1])
    assert len(dyn_rows) > 10 and len(rest) > 10 and not np.array_equal(o_pass["dist"][dyn_rows], o_dyn["dist"][dyn_rows])
    assert_tables_equal({k: g[k][dyn_rows] for k in TABLES}, {k: o_dyn[k][dyn_rows] for k in TABLES}, "the dynamic points of the list")
    assert_tables_equal({k: g[k][rest] for k in TABLES}, {k: o_pass[k][rest] for k in TABLES}, "the other points of the list")


# ---- the current-points list ---------------------------------------------------------------------------------------------------------------
def _list_ref(pf, mf, map_count, cap, old_list, old_count, slot_table):
    """k_register_list in numpy: the live, not-false points with a feature, in map order, at most cap of them; the rows that left the list
    and the rows beyond the cap lose their candidates.  Returns (list padded with -1, count, overflow); slot_table in place."""
    n_map = len(pf)
    live = min(map_count, n_map)
    cur = np.nonzero((np.arange(n_map) < live) & ((mf & 2) == 0) & (pf >= 0).any(axis=1))[0]
    old = old_list[:min(max(old_count, 0), n_map)]
    old = old[(old >= 0) & (old < n_map)]
    slot_table[np.setdiff1d(old, cur)] = -1
    slot_table[cur[cap:]] = -1
    lst = np.full(n_map, -1, np.int32)
    lst[:min(len(cur), cap)] = cur[:cap]
    return lst, min(len(cur), cap), max(len(cur) - cap, 0)


def _offset_tensor(a, off, dev):
    """`a` on the device, its first element `off` ints behind a 16-byte boundary"""
    import torch

    buf = torch.zeros(a.size + 4, dtype=torch.int32, device=dev)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * off
    return v


@pytest.mark.parametrize("n_cams", [1, 3, 4, 8, 9, 12, 13, 16])
def test_current_points_list_by_every_row_reader(hip, n_cams):
    """4 and 8 cameras: rows as one or two 16-byte loads; 12 and 16: the int4 loop; every other count, and every count with pointFeat and
    slotTable one int off the boundary: the scalar loop.  A first call without a cap, a second with fewer current points and a cap below
    their number: list, count, overflow and the rows of slotTable are the restatement's, whichever reader ran."""
    import torch

    from coslam_amd.register import register_list_current_dev

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for n_map in (1, 63, 64, 65, 1025, 65536):
        rng = np.random.default_rng(1000 * n_cams + n_map)
        pf2 = np.where(rng.random((n_map, n_cams)) < 0.3 / n_cams, rng.integers(0, 500, (n_map, n_cams)), -1).astype(np.int32)
        pf2[n_map - 1, n_cams - 1] = 3                       # the table's last entry decides its last row
        pf1 = pf2.copy()
        extra = rng.random(n_map) < 0.1
        pf1[extra, rng.integers(0, n_cams, int(extra.sum()))] = 7
        mf = np.where(rng.random(n_map) < 0.1, 2, rng.choice([0, 1, 4], n_map)).astype(np.uint8)
        mf[n_map - 1] = 0
        for map_count in (n_map + 10, max(n_map * 3 // 4, 1)) if n_map > 1 else (11, 0):
            got = []
            for off in (0, 1):
                d_pf1, d_pf2 = _offset_tensor(pf1, off, dev), _offset_tensor(pf2, off, dev)
                table = np.full((n_map, n_cams), 7, np.int32)
                d_table = _offset_tensor(table, off, dev)
                d_mf = torch.from_numpy(mf).to(dev)
                d_cnt = torch.tensor([map_count], dtype=torch.int32, device=dev)
                d_list = torch.full((n_map,), -1, dtype=torch.int32, device=dev)
                d_n, d_over = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
                want_l, want_n, want_o = _list_ref(pf1, mf, map_count, n_map, np.full(n_map, -1, np.int32), 0, table)
                register_list_current_dev(s, n_cams, n_map, d_cnt.data_ptr(), d_pf1.data_ptr(), d_mf.data_ptr(), d_list.data_ptr(), d_n.data_ptr(),
                                          d_table.data_ptr(), d_overflow=d_over.data_ptr())
                torch.cuda.synchronize()
                what = f"{n_cams} cameras, {n_map} points, count {map_count}, offset {off}"
                assert np.array_equal(d_list.cpu().numpy(), want_l) and d_n.item() == want_n and d_over.item() == 0, what
                assert np.array_equal(d_table.cpu().numpy(), table), what
                cap = max(want_n // 2, 1)
                want_l2, want_n2, want_o2 = _list_ref(pf2, mf, map_count, cap, want_l, want_n, table)
                register_list_current_dev(s, n_cams, n_map, d_cnt.data_ptr(), d_pf2.data_ptr(), d_mf.data_ptr(), d_list.data_ptr(), d_n.data_ptr(),
                                          d_table.data_ptr(), listCap=cap, d_overflow=d_over.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(d_list.cpu().numpy(), want_l2) and d_n.item() == want_n2 and d_over.item() == want_o2, what
                assert np.array_equal(d_table.cpu().numpy(), table), what
                got.append((d_list.cpu().numpy(), d_table.cpu().numpy(), want_n2, want_o2))
                if n_map >= 1025 and map_count > n_map:
                    assert want_o2 > 0 and (table == -1).any() and (table == 7).any(), what     # the cap cut the list; rows left it
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and got[0][2:] == got[1][2:]
    with pytest.raises(coslam_amd.CoslamHipError):   # the bitmap holds 65536 points
        register_list_current_dev(s, n_cams, 65537, 0, d_pf2.data_ptr(), d_mf.data_ptr(), d_list.data_ptr(), d_n.data_ptr(), 0)


# ---- the second visits: list and walks ------------------------------------------------------------------------------------------------------
GARBAGE = 0x5A5A5A5A


def _run_second_visits(name):
    """cs_register_revisit_list_dev then cs_register_revisit_decide_next_dev on build(name) against expected(name)"""
    import torch

    from coslam_amd.register import register_decide_scratch_bytes, register_revisit_decide_next_dev, register_revisit_list_dev

    S, E = build(name), expected(name)
    C, P, N, cap = S["C"], S["P"], S["N"], S["cap"]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    d = lambda a: torch.from_numpy(np.array(a)).to(dev)   # noqa: E731  (a copy: the cases' arrays are read-only)
    d_slot, d_flags, d_merg, d_mf, d_pf, d_att = d(S["slot"]), d(S["flags"]), d(S["merg"]), d(S["mf"]), d(S["pf"]), d(S["att"])
    d_s2m = [d(x) for x in S["s2m"]]
    d_reg_in, d_reg_out = d(S["reg"]), torch.ones(P, dtype=torch.uint8, device=dev)
    d_visit, d_next = d(S["visit"]), torch.full((P,), 77, dtype=torch.int32, device=dev)
    d_list = torch.full((cap,), 31337, dtype=torch.int32, device=dev)
    d_lcnt = torch.zeros(4, dtype=torch.int32, device=dev)
    # ---- the list
    register_revisit_list_dev(s, C, P, cap, S["first"], d_pf.data_ptr(), d_att.data_ptr(), d_reg_in.data_ptr(), False, d_visit.data_ptr(), d_next.data_ptr(),
                              d_list.data_ptr(), d_lcnt.data_ptr(), d_regOutClear=d_reg_out.data_ptr())
    torch.cuda.synchronize()
    L, A = E["list"], E["after_list"]
    lst = d_list.cpu().numpy()
    assert d_lcnt.cpu().tolist() == [L["n"], L["overflow"], 0, 0]
    assert set(lst[:L["n"]].tolist()) == L["members"] and len(set(lst[:L["n"]].tolist())) == L["n"] and (lst[L["n"]:] == -1).all()
    assert np.array_equal(d_visit.cpu().numpy(), A["visit"]) and np.array_equal(d_next.cpu().numpy(), E["next_loop"])
    assert np.array_equal(d_reg_in.cpu().numpy(), A["reg_in"]) and not d_reg_out.cpu().numpy().any()
    # ---- the walks
    n_scr = register_decide_scratch_bytes(C, N, P)
    d_scr = torch.full((n_scr // 4,), GARBAGE, dtype=torch.int32, device=dev)
    d_cur = d(S["cur"])
    d_cur_n = torch.tensor([len(S["cur"]) + 5], dtype=torch.int32, device=dev)     # (a count beyond the capacity: the capacity holds)
    d_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    used = cap - S["free_next"]
    d_nlist = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    d_nlist[:used] = 424242
    d_ncnt = torch.tensor([used], dtype=torch.int32, device=dev)
    d_over = torch.zeros(1, dtype=torch.int32, device=dev)
    register_revisit_decide_next_dev(s, C, N, P, cap, S["map_base"], S["kinds"], d_list.data_ptr(), d_next.data_ptr(), d_visit.data_ptr(), d_slot.data_ptr(),
                                     d_flags.data_ptr(), d_merg.data_ptr(), d_mf.data_ptr(), d_pf.data_ptr(), [x.data_ptr() for x in d_s2m], d_att.data_ptr(),
                                     d_reg_out.data_ptr(), d_scr.data_ptr(), d_cur.data_ptr(), d_cur_n.data_ptr(), len(S["cur"]), d_cnt.data_ptr(),
                                     d_listCount=d_lcnt.data_ptr(), d_nextList=d_nlist.data_ptr(), d_nextCount=d_ncnt.data_ptr(), d_overflow=d_over.data_ptr())
    torch.cuda.synchronize()
    R = E["round"]
    cnt = d_cnt.cpu().tolist()
    print(f"{name}: listed {L['n']}, device counts {cnt}, sequential {R['counts']}; next list {d_ncnt.item() - used} of {len(R['next'])} joiners, "
          f"beyond it {d_over.item()}")
    assert np.array_equal(d_pf.cpu().numpy(), E["pf"]), f"{name}: pointFeat differs in {int((d_pf.cpu().numpy() != E['pf']).sum())} entries"
    for c in range(C):
        assert np.array_equal(d_s2m[c].cpu().numpy(), E["s2m"][c]), f"{name}: slot2map of camera {c}"
    assert np.array_equal(d_att.cpu().numpy(), E["att"]) and np.array_equal(d_reg_out.cpu().numpy(), E["reg_out"])
    assert np.array_equal(d_visit.cpu().numpy(), E["visit"])
    assert cnt[:3] == R["counts"] and cnt[3] == 0, (cnt, R["counts"])
    # the next round's list: as a set; with too few free rows any of the joiners may hold them, the rest is counted
    nl = d_nlist.cpu().numpy()
    n_app = min(len(R["next"]), S["free_next"])
    appended = nl[used:used + n_app].tolist()
    assert d_ncnt.item() == used + len(R["next"]) and d_over.item() == R["overflow"] == len(R["next"]) - n_app
    assert len(set(appended)) == n_app and set(appended) <= R["next"] and (nl[:used] == 424242).all() and (nl[used + n_app:] == -1).all()
    if R["overflow"] == 0:
        assert set(appended) == R["next"]
    want_next = E["next_loop"].copy()
    for p in appended:
        want_next[p] = R["nextLoop"][p]
    assert np.array_equal(d_next.cpu().numpy(), want_next)
    # the scratch: only the owners of the round's own candidates were touched
    mine = np.zeros(C * N, dtype=bool)
    for p in L["members"]:
        kind = _kind(S["mf"], p, S["kinds"])
        for i in range(C):
            sl = _candidate(S["slot"], S["flags"], S["pf"], p, i, N, kind) if kind >= 0 else -1
            if sl >= 0:
                mine[i * N + sl] = True
    scr = d_scr.cpu().numpy()
    head = 4 + C * P + P
    owners = scr[head:head + 3 * C * N].reshape(3, C * N)
    assert (owners[:, ~mine] == GARBAGE).all() and (owners[:, mine] != GARBAGE).all()
    assert (scr[:head] == GARBAGE).all() and (scr[head + 3 * C * N:] == GARBAGE).all()
    return E


@pytest.mark.parametrize("name", sorted(CASES))
def test_second_visit_list_and_walks_equal_the_sequential_walk(hip, name):
    """c9_cap64, c12_cap256: k_revisit_decide<16> at 256 threads; c13_cap320: at 320, from the later-round form of the list; c16_cap1024: at
    1024; c8_cap256: the 8-camera instantiation before the same sequential walk"""
    E = _run_second_visits(name)
    assert E["round"]["counts"][0] >= 20


# ---- all rounds of the second visits in one launch, at more than 8 cameras ---------------------------------------------------------------
ROUNDS = 4
SIGMA = 10.0


class _RoundsState:
    """A frame's state behind the single pass, built by hand: a TrackHistory of C cameras over tests/poseupdate_scene.Scene (six frames pushed,
    the feature references advanced frame by frame), the newest frame with some of the map points' features detached -- unmapped features
    that sit where their points project: what a second visit finds -- and round 0's list filled here: the launch reads it, the single pass
    (which would have written it) is not part of this test."""

    def __init__(self, C, n_map, cap, n_listed, seed):
        import torch

        from coslam_amd.poseupdate import TrackHistory
        from coslam_amd.register import register_cams, register_decide_scratch_bytes, register_passes
        from tests.poseupdate_scene import Scene

        self.C, self.N, self.n_map, self.cap = C, 128, n_map, cap
        N, T = self.N, 6
        self.cur = T - 1
        ps = Scene(nC=C, N=N, nMap=n_map, T=T, seed=seed)
        dev = self.dev = torch.device("cuda:0")
        s = self.s = torch.cuda.current_stream().cuda_stream
        d = self.d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        rng = np.random.default_rng(seed)
        self.th = TrackHistory(C, N, 16)
        self.d_K, self.d_iK = d(ps.K.reshape(9)), d(ps.iK.reshape(9))
        stat = np.stack([np.where(ps.slotPt[c] >= 0, ~ps.moving[np.clip(ps.slotPt[c], 0, None)], True) for c in range(C)]).astype(np.uint8)
        self.d_stat, self.d_rep = d(stat), torch.zeros((C, N), dtype=torch.float64, device=dev)
        self.d_fref = torch.full((n_map, C, 4), -1, dtype=torch.int32, device=dev)
        self.d_rstat = torch.zeros((n_map, C), dtype=torch.uint8, device=dev)
        self.d_fref_counts = torch.zeros(5, dtype=torch.int32, device=dev)
        d_fl_push = d(ps.flags0)
        self.keep = []
        for f in range(T):
            recs = ps.frame(f)
            if f == self.cur:   # the newest frame: three in ten of the features that carry a map point lose it
                pf_whole = Scene.point_feat(recs, n_map)
                for r in recs:
                    r["slot2map"][(r["slot2map"] >= 0) & (rng.random(N) < 0.3)] = -1
            t = [{k: d(v) for k, v in r.items()} for r in recs]
            d_R, d_t = d(np.stack([ps.Re[f][c].reshape(9) for c in range(C)])), d(np.stack([ps.te[f][c] for c in range(C)]))
            cams = [dict(K=self.d_K.data_ptr(), iK=self.d_iK.data_ptr(), xy=t[c]["xy"].data_ptr(), state=t[c]["state"].data_ptr(),
                         slot2map=t[c]["slot2map"].data_ptr(), trackSpan=t[c]["trackSpan"].data_ptr(), reprojErr=self.d_rep[c].data_ptr(),
                         isStatic=self.d_stat[c].data_ptr()) for c in range(C)]
            self.th.detect_dynamic_dev(s, cams, d_R.data_ptr(), d_t.data_ptr(), n_map, d_fl_push.data_ptr(), f, minLen=1 << 30)   # (pushes the frame)
            pf = Scene.point_feat(recs, n_map)
            d_pf = d(pf)
            self.th.feat_ref_advance_dev(s, cams, n_map, d_pf.data_ptr(), f, self.d_fref.data_ptr(), d_refStatic=self.d_rstat.data_ptr(),
                                         d_counts=self.d_fref_counts.data_ptr())
            self.keep += [t, d_R, d_t, d_pf]
        torch.cuda.synchronize()
        self.pu_cams, self.d_pf, self.d_s2m = cams, d_pf, [t[c]["slot2map"] for c in range(C)]
        self.reg_cams = register_cams([dict(K=self.d_K.data_ptr(), R=d_R[c].data_ptr(), t=d_t[c].data_ptr(), xy=t[c]["xy"].data_ptr(),
                                            state=t[c]["state"].data_ptr(), slot2map=t[c]["slot2map"].data_ptr(), isStatic=self.d_stat[c].data_ptr())
                                       for c in range(C)])
        self.d_map, self.d_cov, self.d_mf = d(ps.map0), d(ps.cov0), d(ps.flags0)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        self.out = dict(slot=torch.full((n_map, C), -1, dtype=torch.int32, device=dev), flags=z((n_map, C), torch.int32),
                        m=z((n_map, C, 2), torch.float64), var=z((n_map, C, 4), torch.float64), dist=z((n_map, C), torch.float64))
        self.d_mergeable = z((n_map, C), torch.uint8)
        self.d_cache = z(self.th.mergability_cache_bytes(n_map), torch.uint8)
        self.d_att, self.d_rv_reg = z((n_map, C), torch.uint8), z(n_map, torch.uint8)
        self.d_scr = z(register_decide_scratch_bytes(C, N, n_map), torch.uint8)
        self.d_rv_counts = z(4, torch.int32)
        # the frame's current points, and round 0's list: points that hold a feature; a row's next loop is the first camera that holds one
        held = (pf >= 0).any(axis=1) & ((ps.flags0 & 2) == 0)
        cur_pts = np.nonzero(held)[0].astype(np.int32)
        self.d_curlist, self.d_curcount = d(cur_pts), d(np.array([len(cur_pts)], np.int32))
        lost = ((pf_whole >= 0) & (pf < 0)).any(axis=1)     # (first the points one of whose features was detached: they have something to find)
        listed = np.concatenate([cur_pts[lost[cur_pts]], cur_pts[~lost[cur_pts]]])[:n_listed]
        assert len(listed) == n_listed <= cap, (len(cur_pts), n_listed)
        lists = np.full((ROUNDS, cap), -1, np.int32)
        lists[0, :n_listed] = listed
        counts = np.zeros(ROUNDS + 1, np.int32)
        counts[0] = n_listed
        nxt, visit = np.zeros(n_map, np.int32), np.full(n_map, -1, np.int32)
        nxt[held] = (pf[held] >= 0).argmax(axis=1)
        self.d_lists, self.d_rvcounts, self.d_next, self.d_visit = d(lists), d(counts), d(nxt), d(visit)
        self.pass_dict = dict(P=cap, sigmaSearch=SIGMA, maxDist=3 * PIXEL_ERR_VAR, sigmaMerge=SIGMA, M=self.d_map.data_ptr(), cov=self.d_cov.data_ptr(),
                              pointFeat=self.d_pf.data_ptr(), **{k: self.out[k].data_ptr() for k in TABLES}, mapFlags=self.d_mf.data_ptr(),
                              maxDistDynamic=4 * PIXEL_ERR_VAR)
        self.passes = [register_passes([dict(self.pass_dict, list=self.d_lists[r].data_ptr())]) for r in range(ROUNDS)]
        # what a sequence of rounds may write (the segment pools apart): snapshot / put back / compare
        self.tensors = dict(pf=self.d_pf, map=self.d_map, cov=self.d_cov, mapFlags=self.d_mf, refStatic=self.d_rstat, rv_counts=self.d_rv_counts,
                            fref_counts=self.d_fref_counts, rvcounts=self.d_rvcounts, mergeable=self.d_mergeable, merge_cache=self.d_cache,
                            rv_reg=self.d_rv_reg, att=self.d_att, visit=self.d_visit, next=self.d_next, featRef=self.d_fref, lists=self.d_lists,
                            scratch=self.d_scr, **{k: self.out[k] for k in TABLES}, **{f"s2m{c}": self.d_s2m[c] for c in range(C)})

    def snapshot(self):
        self.torch_sync()
        return {k: v.clone() for k, v in self.tensors.items()}

    def put_back(self, snap):
        for k, v in self.tensors.items():
            v.copy_(snap[k])
        self.torch_sync()

    def torch_sync(self):
        import torch

        torch.cuda.synchronize()

    def state(self):
        """every array the launches may write, as tests/test_revisit_rounds_gpu.py's _state compares them: a reference's segment by WHETHER one is
        linked behind, the lists as sets; the scratch is working memory"""
        self.torch_sync()
        out = {k: v.cpu().numpy() for k, v in self.tensors.items() if k not in ("scratch", "featRef", "lists")}
        fref = self.d_fref.cpu().numpy()
        out["featRef"], out["featRef_linked"] = fref[:, :, :3], fref[:, :, 3] >= 0
        out["lists"] = np.sort(self.d_lists.cpu().numpy(), axis=1)
        return out

    def launch_per_step(self):
        """the four launches per round the one launch replaces"""
        from coslam_amd.register import register_revisit_decide_next_dev, register_search_passes_dev

        C, N, n_map, cap, s, o = self.C, self.N, self.n_map, self.cap, self.s, self.out
        cnt = self.d_rvcounts.data_ptr()
        for r in range(ROUNDS):
            lst = self.d_lists[r].data_ptr()
            register_search_passes_dev(s, self.reg_cams, N, W, H, self.passes[r])
            self.th.register_mergability_running_dev(s, self.pu_cams, n_map, self.d_map.data_ptr(), self.d_cov.data_ptr(), o["slot"].data_ptr(), SIGMA,
                                                     self.d_cache.data_ptr(), self.d_mergeable.data_ptr(), tolPix=0.0, d_counts=0, cam0=0, nCamsRun=C,
                                                     d_list=lst, nList=cap, d_flags=o["flags"].data_ptr())
            more = r + 1 < ROUNDS
            register_revisit_decide_next_dev(s, C, N, n_map, cap, 0, 3, lst, self.d_next.data_ptr(), self.d_visit.data_ptr(), o["slot"].data_ptr(),
                                             o["flags"].data_ptr(), self.d_mergeable.data_ptr(), self.d_mf.data_ptr(), self.d_pf.data_ptr(),
                                             [x.data_ptr() for x in self.d_s2m], self.d_att.data_ptr(), self.d_rv_reg.data_ptr(), self.d_scr.data_ptr(),
                                             self.d_curlist.data_ptr(), self.d_curcount.data_ptr(), len(self.d_curlist), self.d_rv_counts.data_ptr(),
                                             d_listCount=cnt + 4 * r, d_nextList=self.d_lists[r + 1].data_ptr() if more else 0,
                                             d_nextCount=cnt + 4 * (r + 1) if more else 0, d_overflow=cnt + 4 * ROUNDS)
            self.th.feat_ref_advance_refine_dev(s, self.pu_cams, n_map, self.d_pf.data_ptr(), self.cur, self.d_fref.data_ptr(), self.d_rstat.data_ptr(),
                                                lst, cap, False, self.d_rv_reg.data_ptr(), True, self.d_map.data_ptr(), self.d_cov.data_ptr(), SIGMA,
                                                d_counts=self.d_fref_counts.data_ptr())

    def one_launch(self):
        from coslam_amd.register import register_revisit_rounds_dev

        register_revisit_rounds_dev(self.s, self.th, self.reg_cams, self.pu_cams, W, H, self.passes[0], self.n_map, self.cur, 0, 3, self.d_map.data_ptr(),
                                    self.d_cov.data_ptr(), SIGMA, 0.0, self.d_cache.data_ptr(), self.d_mergeable.data_ptr(), self.d_lists.data_ptr(),
                                    self.d_rvcounts.data_ptr(), self.cap, ROUNDS, self.d_visit.data_ptr(), self.d_next.data_ptr(), self.d_mf.data_ptr(),
                                    self.d_pf.data_ptr(), [x.data_ptr() for x in self.d_s2m], self.d_att.data_ptr(), self.d_rv_reg.data_ptr(),
                                    self.d_scr.data_ptr(), self.d_curlist.data_ptr(), self.d_curcount.data_ptr(), len(self.d_curlist),
                                    self.d_rv_counts.data_ptr(), self.d_fref.data_ptr(), d_refStatic=self.d_rstat.data_ptr(),
                                    d_frefCounts=self.d_fref_counts.data_ptr())


@pytest.mark.parametrize("C,n_map,cap,n_listed", [(9, 400, 64, 40), (16, 400, 64, 40), (9, 600, 1024, 257), (16, 500, 1024, 300)])
def test_all_rounds_in_one_launch_at_more_than_eight_cameras(hip, C, n_map, cap, n_listed):
    """k_revisit_rounds<16>: lists of 64 rows walk a row per thread and carry no extra LDS; lists of 1024 rows with more than 256 listed are
    walked in turns (rv_decide_rows_looped<16, 256>) with 68 KB of row state in LDS -- more than a launch carries by default.  Both sequences
    from ONE snapshot; an empty round 0 changes nothing."""
    S = _RoundsState(C, n_map, cap, n_listed, seed=40 + C)
    snap = S.snapshot()
    before = S.state()
    S.launch_per_step()
    old = S.state()
    S.put_back(snap)
    S.one_launch()
    new = S.state()
    print(f"{C} cameras, lists of {cap}: listed per round and beyond {new['rvcounts'].tolist()}, attached / registered / conflicts / unsettled "
          f"{new['rv_counts'].tolist()}, references {new['fref_counts'].tolist()}")
    for k in old:
        assert np.array_equal(old[k], new[k]), f"{k} differs in {int((np.asarray(old[k]) != np.asarray(new[k])).sum())} entries"
    assert new["rvcounts"][0] == n_listed and new["rvcounts"][1] > 0 and new["rvcounts"][ROUNDS] == 0    # a second round ran; nothing beyond the lists
    assert new["rv_counts"][0] > 0 and new["rv_counts"][1] > 0 and new["rv_counts"][3] == 0              # features attached, points registered
    assert not np.array_equal(before["pf"], new["pf"]) and not np.array_equal(before["map"], new["map"])   # ... and refined
    # an empty round 0 (a later round's count left standing): the launch leaves at once
    S.put_back(snap)
    S.d_rvcounts[0] = 0
    S.d_rvcounts[1] = 5
    quiet = S.state()
    S.one_launch()
    after = S.state()
    for k in quiet:
        assert np.array_equal(quiet[k], after[k]), f"{k} changed by a launch over an empty list"
    S.th.close()
