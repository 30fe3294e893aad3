"""The self-settling registration decision (cs_register_decide_kinds_rounds_dev, nSweeps 0) as ONE launch that settles only the ACTIVE
walks -- those that reach an unmapped, mergeable candidate with no mapped candidate in front of it -- against the sequential restatement
(oracle.register_decide_static): no active walk, few of them (the owners in the resolver's LDS table), more than the table holds and more
than the workgroup has threads (the owners in the scratch, the rows in turns), every camera count's layout of points over workgroups, a
scratch left behind by a call of another shape, the dynamic points, one camera's loop, a map offset, the second visits' first list."""
import numpy as np
import pytest

from tests.test_register_decide_gpu import _case

pytestmark = pytest.mark.gpu

# what the launch is built around (csrc/register.hip): a workgroup of 256 threads resolves the list; the LDS table holds 512 candidates
WG, LDS_ENTRIES = 256, 512


def _n_active(t, kinds=1):
    """the walks that can claim a feature: a visited point whose first candidate that is mapped or mergeable is unmapped"""
    slot, flags, merg, mf, pf, s2m = t
    P, C = slot.shape
    N, n = len(s2m[0]), 0
    for p in range(P):
        k = int(mf[p]) & 7
        kind = 0 if (k == 0 and kinds & 1) else (1 if (k == 1 and kinds & 2) else -1)
        if kind < 0 or not (pf[p] >= 0).any():
            continue
        for i in range(C):
            s = int(slot[p, i])
            if pf[p, i] >= 0 or s < 0 or s >= N or ((int(flags[p, i]) >> 1) & 1) != kind:
                continue
            if s2m[i][s] >= 0:
                break
            if merg[p, i] == 1:
                n += 1
                break
    return n


def _expect(t, kinds=1, map_base=0, only_cam=-1):
    import oracle

    slot, flags, merg, mf, pf, s2m = t
    o_pf, o_s2m = pf.copy(), [x.copy() for x in s2m]
    if only_cam < 0:
        att, reg = oracle.register_decide_static(slot, flags, merg, mf, o_pf, o_s2m, map_base=map_base, kinds=kinds)
    else:
        # the restatement plays every camera's loop; ONE loop of it: the points without a feature in that camera are not visited (marked
        # uncertain), and the visited ones' features in the other cameras are hidden (no feature, no candidate: the walk passes such a camera
        # by either way), so that no other loop lists anybody before this one
        sl, mfo = slot.copy(), mf.copy()
        mfo[pf[:, only_cam] < 0] = 4
        hide = pf >= 0
        hide[:, only_cam] = False
        o_pf[hide], sl[hide] = -1, -1
        att, reg = oracle.register_decide_static(sl, flags, merg, mfo, o_pf, o_s2m, map_base=map_base, kinds=kinds)
        o_pf[hide] = pf[hide]
    return dict(att=att, reg=reg, pf=o_pf, s2m=o_s2m)


def _run(t, kinds=1, map_base=0, only_cam=-1, scratch=None, lists=None):
    import torch

    from coslam_amd.register import register_decide_kinds_rounds_dev, register_decide_scratch_bytes, register_decide_static_dev

    slot, flags, merg, mf, pf, s2m = t
    P, C = slot.shape
    N = len(s2m[0])
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    d_slot, d_flags, d_merg, d_mf, d_pf = d(slot), d(flags), d(merg), d(mf), d(pf)
    d_s2m = [d(x) for x in s2m]
    d_att, d_reg = torch.full((P, C), 3, dtype=torch.uint8, device=dev), torch.full((P,), 3, dtype=torch.uint8, device=dev)   # (cleared by the launch)
    nbytes = register_decide_scratch_bytes(C, N, P)
    d_scr = torch.zeros(nbytes, dtype=torch.uint8, device=dev) if scratch is None else scratch
    assert d_scr.numel() >= nbytes
    d_cnt = torch.full((4,), 9, dtype=torch.int32, device=dev)
    s_ = torch.cuda.current_stream().cuda_stream
    out = {}
    if lists is None:
        register_decide_static_dev(s_, C, N, P, map_base, d_slot.data_ptr(), d_flags.data_ptr(), d_merg.data_ptr(), d_mf.data_ptr(), d_pf.data_ptr(),
                                   [x.data_ptr() for x in d_s2m], d_att.data_ptr(), d_reg.data_ptr(), d_scr.data_ptr(), d_cnt.data_ptr(), n_sweeps=0,
                                   only_cam=only_cam, kinds=kinds)
    else:
        cap, rounds = lists
        d_lists = torch.zeros((rounds, cap), dtype=torch.int32, device=dev)      # (not -1: the launch has to clear them)
        d_lcnt = torch.full((rounds + 1,), 7, dtype=torch.int32, device=dev)
        d_lcnt[rounds] = 0
        d_visit, d_next = torch.full((P,), -5, dtype=torch.int32, device=dev), torch.full((P,), -5, dtype=torch.int32, device=dev)
        register_decide_kinds_rounds_dev(s_, C, N, P, map_base, d_slot.data_ptr(), d_flags.data_ptr(), d_merg.data_ptr(), d_mf.data_ptr(), d_pf.data_ptr(),
                                         [x.data_ptr() for x in d_s2m], d_att.data_ptr(), d_reg.data_ptr(), d_scr.data_ptr(), d_lists.data_ptr(), cap, rounds,
                                         d_lcnt.data_ptr(), d_visit.data_ptr(), d_next.data_ptr(), d_counts=d_cnt.data_ptr(), kinds=kinds)
        out.update(dev=dict(pf=d_pf, att=d_att, reg=d_reg), lists_d=d_lists, lcnt_d=d_lcnt, visit_d=d_visit, next_d=d_next)
    torch.cuda.synchronize()
    words = d_scr[:nbytes].view(torch.int32)
    out.update(att=d_att.cpu().numpy(), reg=d_reg.cpu().numpy(), pf=d_pf.cpu().numpy(), s2m=[x.cpu().numpy() for x in d_s2m], cnt=d_cnt.cpu().tolist(),
               unsettled=int(words[-1].item()), timeouts=int(words[-2].item()), head=words[:2].cpu().tolist(), scratch=d_scr)
    return out


def _check(g, want, label=""):
    assert np.array_equal(g["att"], want["att"]), label
    assert np.array_equal(g["reg"], want["reg"]), label
    assert np.array_equal(g["pf"], want["pf"]), label
    for c in range(len(want["s2m"])):
        assert np.array_equal(g["s2m"][c], want["s2m"][c]), (label, c)
    assert g["cnt"][0] == int(want["att"].sum()) and g["cnt"][1] == int(want["reg"].sum()), (label, g["cnt"])
    assert g["cnt"][3] == 1 and 2 <= g["cnt"][2] <= 64, (label, g["cnt"])
    assert g["unsettled"] == 0 and g["timeouts"] == 0, label
    assert g["head"] == [0, 0], (label, g["head"])     # the ticket and the list count are left at 0 for the next call


def _blank(P, C, N):
    """every point certainly static with a feature of this frame in the LAST camera (all walks in map order), no candidate anywhere, no
    feature mapped"""
    slot, flags = np.full((P, C), -3, np.int32), np.zeros((P, C), np.int32)
    merg, mf = np.ones((P, C), np.uint8), np.zeros(P, np.uint8)
    pf = np.full((P, C), -1, np.int32)
    pf[:, C - 1] = np.arange(P) % N
    return slot, flags, merg, mf, pf, [np.full(N, -1, np.int32) for _ in range(C)]


def test_no_active_walk(hip):
    P, C, N = 300, 3, 64
    t = _case(21, P, C, N, 0.9)
    mapped = (t[0], t[1], t[2], t[3], t[4], [np.arange(N, dtype=np.int32) % P for _ in range(C)])          # every candidate carries a point
    unmergeable = (t[0], t[1], np.zeros_like(t[2]), t[3], t[4], t[5])                                       # nothing mergeable over its track
    slot, flags, merg, mf, pf, s2m = _blank(P, C, N)                                                       # a mergeable candidate BEHIND a mapped one
    pf[:, C - 1], pf[:, 0] = -1, np.arange(P) % N
    slot[:, 1], slot[:, 2] = np.arange(P) % 7, 10 + np.arange(P) % 50
    s2m[1][:7] = 3
    behind = (slot, flags, merg, mf, pf, s2m)
    for label, tt in (("mapped", mapped), ("unmergeable", unmergeable), ("behind", behind)):
        assert _n_active(tt) == 0, label
        g = _run(tt)
        _check(g, _expect(tt), label)
        assert g["cnt"][:2] == [0, 0] and not g["att"].any() and np.array_equal(g["pf"], tt[4]), label


def test_two_walks_want_one_feature_in_both_orders(hip):
    P, C, N = 300, 3, 64
    for first_cam_of_10, winner in ((0, 10), (2, 200)):
        slot, flags, merg, mf, pf, s2m = _blank(P, C, N)
        pf[:] = -1
        pf[10, first_cam_of_10], pf[200, 0] = 4, 9          # the order of a walk: (its first camera with a feature, the point)
        slot[10, 1] = slot[200, 1] = 5
        t = (slot, flags, merg, mf, pf, s2m)
        assert _n_active(t) == 2
        g, want = _run(t), _expect(t)
        _check(g, want, str(winner))
        assert g["s2m"][1][5] == winner and g["cnt"][:2] == [1, 1]


def test_a_chain_of_walks_that_cut_each_other_short(hip):
    """A takes f; B wants f first and would go on to g; C wants g and would go on to h; D wants h: the sweeps see B at g, then C at h, before
    they see them stopped -- four sweeps until one changes nothing"""
    P, C, N = 300, 4, 64
    slot, flags, merg, mf, pf, s2m = _blank(P, C, N)
    a, b, c, d = 20, 90, 150, 280
    slot[a, 0] = 1
    slot[b, 0], slot[b, 1] = 1, 2
    slot[c, 1], slot[c, 2] = 2, 3
    slot[d, 2] = 3
    t = (slot, flags, merg, mf, pf, s2m)
    assert _n_active(t) == 4
    g, want = _run(t), _expect(t)
    _check(g, want)
    assert g["cnt"][2] > 3 and g["s2m"][0][1] == a and g["s2m"][1][2] == c and g["s2m"][2][3] == c and g["cnt"][:2] == [3, 2]


def test_more_active_walks_than_the_workgroup_or_the_table_holds(hip):
    t = _case(5, 600, 3, 64, 0.9)                            # (163 active walks: 64 features are soon taken)
    _check(_run(t), _expect(t), "dense")
    t = _case(5, 1500, 3, 200, 0.9)
    assert _n_active(t) > WG                                 # the rows in turns, the owners in the scratch
    _check(_run(t), _expect(t), "turns")
    t = _case(31, 400, 8, 2000, 0.2)
    n = _n_active(t)
    assert n <= WG and n * 8 > LDS_ENTRIES, n                # a thread per row, but more candidates than the LDS table may hold
    _check(_run(t), _expect(t), "table")
    t = _case(32, 300, 3, 500, 0.3)
    n = _n_active(t)
    assert 8 < n and n * 3 <= LDS_ENTRIES, n                 # ... and the usual frame: the owners in LDS
    _check(_run(t), _expect(t), "lds")


@pytest.mark.parametrize("P,C,N", [(300, 1, 64), (130, 5, 64), (257, 5, 100), (75, 8, 64), (40, 16, 64), (700, 16, 300)])
def test_every_camera_count_and_a_ragged_last_workgroup(hip, P, C, N):
    """a workgroup takes 256 // C whole points: P is no multiple of that, and 256 none of C"""
    assert P % (WG // C) != 0
    t = _case(40 + C, P, C, N, 0.5)
    _check(_run(t), _expect(t))


def test_a_scratch_left_by_a_call_of_another_shape(hip):
    import torch

    from coslam_amd.register import register_decide_scratch_bytes

    shapes = [(17, 600, 3, 64, 0.9), (18, 150, 8, 300, 0.3), (19, 300, 3, 500, 0.3), (17, 600, 3, 64, 0.9)]
    big = max(register_decide_scratch_bytes(C, N, P) for _, P, C, N, _ in shapes)
    scr = torch.zeros(big, dtype=torch.uint8, device="cuda:0")
    for seed, P, C, N, dens in shapes:
        t = _case(seed, P, C, N, dens)
        want = _expect(t)
        _check(_run(t, scratch=scr), want, f"reused {P}x{C}x{N}")
        _check(_run(t), want, f"fresh {P}x{C}x{N}")


def test_dynamic_points_one_cameras_loop_and_a_map_offset(hip):
    for kinds in (2, 3):
        t = _case(50 + kinds, 900, 4, 400, 0.1, p_dyn=0.4)
        want = _expect(t, kinds=kinds)
        _check(_run(t, kinds=kinds), want, f"kinds {kinds}")
        assert want["att"][(t[3] & 7) == 1].sum() > 20
    t = _case(61, 500, 4, 300, 0.2)
    want = _expect(t, only_cam=1)
    assert want["att"].sum() > 10
    _check(_run(t, only_cam=1), want, "only_cam")
    want = _expect(t, map_base=7)
    assert want["att"].sum() > 10
    _check(_run(t, map_base=7), want, "map_base")


def test_the_second_visits_first_list(hip):
    """list 0, its count and visitLoop / nextLoop of the listed points: what cs_register_revisit_list_dev(firstRound = 1) builds from the
    same result"""
    import torch

    from coslam_amd.register import register_revisit_list_dev

    for seed, P, C, N, dens, cap in ((71, 600, 3, 64, 0.9, 1024), (72, 300, 4, 500, 0.3, 256)):
        t = _case(seed, P, C, N, dens)
        g = _run(t, kinds=3, lists=(cap, 3))
        _check(g, _expect(t, kinds=3), str(seed))
        dev = torch.device("cuda:0")
        lst = torch.zeros(cap, dtype=torch.int32, device=dev)
        visit, nxt = torch.full((P,), -5, dtype=torch.int32, device=dev), torch.full((P,), -5, dtype=torch.int32, device=dev)
        lcnt = torch.zeros(4, dtype=torch.int32, device=dev)
        register_revisit_list_dev(torch.cuda.current_stream().cuda_stream, C, P, cap, True, g["dev"]["pf"].data_ptr(), g["dev"]["att"].data_ptr(),
                                  g["dev"]["reg"].data_ptr(), True, visit.data_ptr(), nxt.data_ptr(), lst.data_ptr(), lcnt.data_ptr())
        torch.cuda.synchronize()
        n = int(lcnt[0].item())
        got_cnt, got = g["lcnt_d"].cpu().tolist(), g["lists_d"].cpu().numpy()
        assert n > 3 and got_cnt == [n, 0, 0, 0], (n, got_cnt)
        listed = np.sort(lst.cpu().numpy()[:n])
        assert np.array_equal(np.sort(got[0, :n]), listed) and (got[0, n:] == -1).all() and (got[1:] == -1).all()
        assert np.array_equal(g["next_d"].cpu().numpy()[listed], nxt.cpu().numpy()[listed])
        regd = np.nonzero(g["reg"])[0]
        assert np.array_equal(g["visit_d"].cpu().numpy()[regd], visit.cpu().numpy()[regd])
