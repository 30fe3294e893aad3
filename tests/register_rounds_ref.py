"""The SECOND VISITS of the registration, one round, played sequentially (TEST INFRASTRUCTURE; plain Python, index work only).

A round visits the points that registered in the round before (round 0: the single pass) again, in the loop of their next camera, one after
the other in the order (loop, point) -- the order CoSLAM::curStaticPointsRegInGroup's camera loops would reach them in.  revisit_list restates
how a round's list is drawn (k_revisit_list), revisit_round the walks, the next round's list and the two conflict terms the device counts
(k_revisit_decide / k_revisit_rounds: coslam_amd/csrc/register_rows_dev.h).  The device settles the walks with Jacobi sweeps over order keys;
here a walk simply sees what the walks before it left."""
import numpy as np


def _kind(mapFlags, p, kinds):
    """0: certainly static and asked for, 1: certainly dynamic and asked for, -1: the point does not walk"""
    fl = int(mapFlags[p]) & 7
    if fl == 0 and (kinds & 1):
        return 0
    if fl == 1 and (kinds & 2):
        return 1
    return -1


def _candidate(slot, flags, pointFeat, p, i, N, kind):
    """the slot the walk of p looks at in camera i, or -1: it holds a feature there, nothing was found, or the feature is of the other type"""
    if pointFeat[p, i] >= 0:
        return -1
    s = int(slot[p, i])
    if s < 0 or s >= N:
        return -1
    if ((int(flags[p, i]) >> 1) & 1) != kind:
        return -1
    return s


def revisit_list(pointFeat, attached, regIn, keepIn, regOutClear, visitLoop, nextLoop, cap, first_round):
    """k_revisit_list.  A point marked in regIn is listed when a camera behind the loop of its latest registering visit holds a feature of
    it; that camera is the loop of the visit listed here.  first_round: the loop of the latest visit is the first camera whose feature was
    there BEFORE the frame attached any (written to visitLoop); later rounds read visitLoop.  regIn is cleared unless keepIn, regOutClear
    (or None) is cleared for every point.  Returns dict(members: every point that wants a row, as a set; nextLoop: {point: loop};
    n: rows filled = min(len(members), cap); overflow: the points beyond cap).  nextLoop is NOT written here: with an overflow, which
    members get a row is the device's order of arrival -- the caller writes the loops of the rows it finds on the list."""
    P, C = pointFeat.shape
    members, loops = set(), {}
    for p in range(P):
        if regOutClear is not None:
            regOutClear[p] = 0
        if not regIn[p]:
            continue
        if not keepIn:
            regIn[p] = 0
        if first_round:
            own = [c for c in range(C) if pointFeat[p, c] >= 0 and not attached[p, c]]
            last = own[0] if own else -1
            visitLoop[p] = last
        else:
            last = int(visitLoop[p])
        if last < 0:
            continue
        later = [c for c in range(last + 1, C) if pointFeat[p, c] >= 0]
        if not later:
            continue
        members.add(p)
        loops[p] = later[0]
    return dict(members=members, nextLoop=loops, n=min(len(members), cap), overflow=max(len(members) - cap, 0))


def revisit_round(slot, flags, mergeable, mapFlags, pointFeat, slot2map, attached, visitLoop, nextLoop, lst, kinds, map_base, cap_next, cur_list,
                  regOut=None):
    """One round.  slot / flags / mergeable: the search's P x C tables over the listed rows; slot2map: C arrays of N owners (map indices,
    the pass's points are map_base .. map_base + P - 1); lst: the listed points (entries < 0 or >= P are no rows); cur_list: the frame's
    current points (who else wanted a feature).  pointFeat, slot2map, attached, visitLoop and regOut (made here when None) are updated in
    place; nextLoop is read only.  Returns dict(next: the points that join the next round's list, as a set; nextLoop: {point: loop} for
    them; overflow: how many of them lie beyond cap_next; counts: [features attached, points registered, conflicts]; regOut;
    chain: the longest chain of walks each cut short by the one before it; witness: the (point, camera) entries of `slot` behind every
    conflict counted, for a test that wants to build an input with a given number of them)."""
    P, C = slot.shape
    N = len(slot2map[0])
    if regOut is None:
        regOut = np.zeros(P, dtype=np.uint8)
    rows = sorted({int(p) for p in lst if 0 <= int(p) < P}, key=lambda p: (int(nextLoop[p]), p))
    # the state the round starts from: the first conflict term asks what a feature's owner did EARLIER IN THIS FRAME
    att0, pf0, vis0 = attached.copy(), pointFeat.copy(), np.array(visitLoop).copy()
    conflicts, witness = 0, []
    taken = {}          # (camera, slot) -> (loop, point, chain length of the walk that took it), this round's attachments in order
    n_att = n_reg = 0
    chain_max = 0
    joiners, loops = [], {}
    for p in rows:
        kind = _kind(mapFlags, p, kinds)
        if kind < 0:
            continue
        loop = int(nextLoop[p])
        # ---- conflict term 1: a candidate that carries a point NOW -- did it when this visit takes place?  Not if the owner took it in a
        # visit of this frame that comes AFTER this one in the reference's order (its loop, then its index): the reference would have found
        # the feature unmapped here.  Every candidate of the row is asked, reached by the walk or not.
        for i in range(C):
            s = _candidate(slot, flags, pf0, p, i, N, kind)
            if s < 0:
                continue
            own = int(slot2map[i][s])
            if (i, s) in taken or own < 0:
                continue            # (taken: it was unmapped when the round began)
            own -= map_base
            if 0 <= own < P and att0[own, i] and pf0[own, i] == s and (int(vis0[own]), own) > (loop, p):
                conflicts += 1
                witness.append((p, i))
        # ---- the walk
        reg, chain = False, 0
        for i in range(C):
            s = _candidate(slot, flags, pointFeat, p, i, N, kind)
            if s < 0:
                continue
            if slot2map[i][s] >= 0:                 # it carries a point: the walk ends
                if (i, s) in taken:
                    chain = taken[(i, s)][2] + 1    # cut short by a walk of this round (itself cut short by chain - 1 others)
                break
            if mergeable[p, i] == 1:
                slot2map[i][s] = map_base + p
                pointFeat[p, i] = s
                attached[p, i] = 1
                taken[(i, s)] = (loop, p, None)
                reg = True
                n_att += 1
        for k, v in taken.items():                  # what this walk took carries its chain length
            if v[2] is None:
                taken[k] = (v[0], v[1], chain)
        chain_max = max(chain_max, chain)
        if reg:
            n_reg += 1
            regOut[p] = 1
            visitLoop[p] = loop
            later = [c for c in range(loop + 1, C) if pointFeat[p, c] >= 0]
            if later:
                joiners.append(p)
                loops[p] = later[0]
    # ---- conflict term 2: a feature attached in this round was unmapped until now.  A current point q whose candidate it was, whose
    # (first) visit of this frame comes AFTER the attaching visit and who holds no feature in that camera, walked past it -- in the
    # reference's order its walk ends there.  Counted where q attached something in a camera behind it.  The loop of q's first visit: the
    # first camera holding a feature of q that was not attached in this frame.
    for q in cur_list:
        q = int(q)
        if q < 0 or q >= P:
            continue
        own = [c for c in range(C) if pointFeat[q, c] >= 0 and not attached[q, c]]
        if not own:
            continue
        lq = own[0]
        for (i, s), (loop, p, _) in taken.items():
            if int(slot[q, i]) != s or pointFeat[q, i] >= 0:
                continue
            if (lq, q) < (loop, p) or ((lq, q) == (loop, p)):
                continue
            if attached[q, i + 1:].any():
                conflicts += 1
                witness.append((q, i))
    return dict(next=set(joiners), nextLoop=loops, overflow=max(len(joiners) - cap_next, 0), counts=[n_att, n_reg, conflicts], regOut=regOut,
                chain=chain_max, witness=witness)


def sweeps_to_settle(slot, flags, mergeable, mapFlags, pointFeat, slot2map, nextLoop, lst, kinds):
    """How hard a round's input is for a solver that evaluates every walk against the owners of the sweep before (a measure of the TEST
    INPUT, not an expected value): the number of sweeps until one changes no owner, that one included.  2: the first sweep's owners were
    final.  4 and more: after two sweeps a walk was still cut short by a claim of a walk that is itself cut short in front of it."""
    P, C = slot.shape
    N = len(slot2map[0])
    inf = 1 << 62
    walks = []
    for p in sorted({int(p) for p in lst if 0 <= int(p) < P}):
        kind = _kind(mapFlags, p, kinds)
        if kind < 0:
            continue
        steps = []
        for i in range(C):
            s = _candidate(slot, flags, pointFeat, p, i, N, kind)
            if s >= 0:
                steps.append(((i, s), ((int(nextLoop[p]) * P + p) * C + i), slot2map[i][s] >= 0, mergeable[p, i] == 1))
        walks.append(steps)
    prev, n = {}, 0
    while True:
        nxt = {}
        for steps in walks:
            for f, order, mapped, can in steps:
                if mapped or prev.get(f, inf) < order:
                    break
                if can:
                    nxt[f] = min(nxt.get(f, inf), order)
        n += 1
        if nxt == prev:
            return n
        prev = nxt
