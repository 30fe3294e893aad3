"""Planted cases of the merge map update: a golden scene of tests/golden/mergeconstraints_golden.npz with its slot table and
match list edited so that the ASSEMBLED merge list holds the case; every builder asserts on the restatement's list that it does."""
import numpy as np

from tests import mergeconstraints_ref as ref


def _f2(S):
    return S["frame0"] + S["nF"] - 1


def _cur(S, m, c):
    r = S["featRef"][m][c]
    return 0 <= int(r[0]) < S["N"] and int(r[1]) == _f2(S)


def _tracks(S):
    """[(match index, m1, m2)] of the matches that become tracks"""
    iC, jC, out = S["maxiCam"], S["maxjCam"], []
    for k, (a, b) in enumerate(S["matches"]):
        if 0 <= a < S["N"] and 0 <= b < S["N"] and S["state"][iC][a] in (0, 1) and S["state"][jC][b] in (0, 1):
            m1, m2 = int(S["slot2map"][iC][a]), int(S["slot2map"][jC][b])
            if m1 >= 0 and m2 >= 0:
                out.append((k, m1, m2))
    return out


def _edited(S, slot_edits, extra):
    s2m = np.array(S["slot2map"], np.int32)
    for c, s, m in slot_edits:
        s2m[c][s] = m
    return dict(S, slot2map=s2m, matches=np.concatenate([np.asarray(S["matches"], np.int32), np.array(extra, np.int32).reshape(-1, 2)]))


def _free_slot(S, c, taken):
    """a tracked slot of camera c that no match uses and no point of a track owns"""
    col = 0 if c == S["maxiCam"] else 1
    used = set(int(m[col]) for m in S["matches"]) | set(taken)
    pts = set(m for _, m1, m2 in _tracks(S) for m in (m1, m2))
    return next(s for s in range(S["N"]) if S["state"][c][s] in (0, 1) and s not in used and int(S["slot2map"][c][s]) >= 0
                and int(S["slot2map"][c][s]) not in pts)


def shared_row(S, f1):
    """a second track with the m1 of the first: the rows (m1, c) are named by two tracks, with different sources"""
    iC, jC = S["maxiCam"], S["maxjCam"]
    tr = _tracks(S)
    (_, A, _), (k2, _, B2) = tr[0], tr[1]
    a2 = _free_slot(S, iC, ())
    P = _edited(S, [(iC, a2, A)], [[a2, int(S["matches"][k2][1])]])
    v = ref.assemble(P, f1)["views"]
    rows = {}
    for i, e in enumerate(v):
        rows.setdefault((e[3], e[1]), []).append(i)
    assert any(len(set(v[i][0] for i in ix)) > 1 and len(set(v[i][4] for i in ix)) > 1 for (m, _), ix in rows.items() if m == A)
    return P


def slot_in_two_tracks(S, f1):
    """the m2 of the first track matched a second time from another point: its features are views of two tracks"""
    iC, jC = S["maxiCam"], S["maxjCam"]
    k, _, _ = _tracks(S)[0]
    a2 = _free_slot(S, iC, ())
    P = _edited(S, [], [[a2, int(S["matches"][k][1])]])
    v = ref.assemble(P, f1)["views"]
    slots = {}
    for e in v:
        slots.setdefault((e[1], e[2]), set()).add(e[3])
    assert any(len(p) > 1 for p in slots.values())
    return P


def from_is_an_m1(S, f1):
    """track 1 = (A, B) with A and B both seen by one camera c (A's row in c takes B's); a later track (C, A): C's row in c must take A's row
    AS IT STOOD, not B's -- the gather-before-scatter case"""
    iC, jC = S["maxiCam"], S["maxjCam"]
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    A = B = c0 = None
    for _, m1, m2 in _tracks(S):
        both = [c for c in ids if _cur(S, m1, c) and _cur(S, m2, c)]
        if both and m1 != m2:
            A, B, c0 = m1, m2, both[0]
            break
    assert A is not None, "no track whose two points share a camera"
    a2, b2 = _free_slot(S, iC, ()), _free_slot(S, jC, ())
    P = _edited(S, [(jC, b2, A)], [[a2, b2]])
    v = ref.assemble(P, f1)["views"]
    C = int(S["slot2map"][iC][a2])
    first = max(i for i, e in enumerate(v) if e[3] == A and e[1] == c0 and e[4] == B)
    later = [i for i, e in enumerate(v) if e[3] == C and e[1] == c0 and e[4] == A]
    assert later and later[-1] > first and not np.array_equal(S["featRef"][A][c0], S["featRef"][B][c0])
    return P, (A, B, C, c0)


def detached_then_named_again(S, f1):
    """a detached view (the second feature of its track in camera c) whose slot a LATER track names without the mark: the slot stays detached"""
    iC, jC = S["maxiCam"], S["maxjCam"]
    A0 = ref.assemble(S, f1)
    det = next(e for e in A0["views"] if e[5] & ref.VIEW_DETACHED and e[4] != e[3])       # B's feature in c, behind A's
    t, c, s, B = det[0], det[1], det[2], det[4]
    k = _tracks(S)[t][0]
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    named = set(m for _, m1, m2 in _tracks(S) for m in (m1, m2))
    C = next(m for m in range(S["nMap"]) if m not in named and not any(_cur(S, m, cc) and _cur(S, B, cc) for cc in ids)
             and any(_cur(S, m, cc) for cc in ids))
    a2 = _free_slot(S, iC, ())
    P = _edited(S, [(iC, a2, C)], [[a2, int(S["matches"][k][1])]])
    v = ref.assemble(P, f1)["views"]
    same = [e for e in v if (e[1], e[2]) == (c, s)]
    assert same[0][5] & ref.VIEW_DETACHED and not same[-1][5] & ref.VIEW_DETACHED and same[-1][0] > same[0][0]
    return P, (c, s)
