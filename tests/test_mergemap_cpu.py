"""The merge map update on the host: the plain restatement tests/mergemap_ref.py of cs_merge_constraints_apply_map_dev gives the
post-state the reference's own objects hold behind mergeMapPoints and the duplicate marks (tests/golden/mergeconstraints_golden.npz: cur_mpt,
pfeat, detached); a moved reference carries its whole chain; the library exports what the header declares."""
import os
import re

import numpy as np
import pytest

import coslam_amd
from tests import mergeconstraints_ref as ref
from tests import mergemap_ref as mref
from tests.mergeconstraints_golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = load()
IDS = range(len(SCENES))


@pytest.mark.parametrize("sc", IDS)
def test_restatement_gives_the_recorded_post_state(sc):
    """cur_mpt on the slots that are features, pfeat as {slot, frame} of every row, the detached nodes; and apply_views agrees"""
    S, G = SCENES[sc]
    f1 = int(G["first_frame"])
    A = ref.assemble(S, f1)
    T = mref.apply_map(S, A["views"], f1=f1)
    cur = np.where(np.isin(S["state"], (0, 1)), T["slot2map"], -1)
    assert np.array_equal(cur, G["cur_mpt"])
    pfeat = np.where(T["featRef"][:, :, :1] >= 0, T["featRef"][:, :, :2], -1)
    assert np.array_equal(pfeat, G["pfeat"])
    assert [list(d) for d in T["detached"]] == sorted(G["detached"].tolist())
    cur2, pfeat2, det2 = ref.apply_views(S, A["views"], f1)
    assert np.array_equal(cur, np.array(cur2)) and np.array_equal(pfeat, np.array(pfeat2)) and T["detached"] == det2
    f2 = S["frame0"] + S["nF"] - 1
    named = set((v[3], v[1]) for v in A["views"])
    for m in range(S["nMap"]):
        for c in range(S["nC"]):
            if (m, c) in named:
                assert T["pointFeat"][m][c] == T["featRef"][m][c][0] and T["featRef"][m][c][1] == f2
            else:
                assert T["pointFeat"][m][c] == mref.point_feat(S)[m][c] and np.array_equal(T["featRef"][m][c], S["featRef"][m][c])
    if A["verdict"] != ref.VERDICT_MERGE:
        assert A["views"] == [] and T["counts"] == [0] * 6
        for k, v in mref.tables(S).items():
            assert np.array_equal(T[k], v), k
    else:
        assert T["counts"][0] == len(A["views"]) and T["counts"][2] == sum(1 for d in T["detached"] if d[1] == f2)
        assert T["counts"][1] > 0 and T["counts"][4] == 0 and np.array_equal(T["M"], S["M"])


def _moved_chains(sc):
    """-> the moved references of scene sc that have a linked segment"""
    S, G = SCENES[sc]
    f1 = int(G["first_frame"])
    A = ref.assemble(S, f1)
    T = mref.apply_map(S, A["views"], f1=f1)
    win = {}
    for v in A["views"]:
        win[(v[3], v[1])] = v
    f2 = S["frame0"] + S["nF"] - 1
    n_seg = 0
    for (m1, c), v in win.items():
        after, before = T["featRef"][m1][c], S["featRef"][v[4]][c]
        assert mref.walk_chain(S, c, after) == mref.walk_chain(S, c, before) and after[0] == v[2]
        n_seg += int(before[3]) >= 0 and v[4] != m1
        for f in range(S["frame0"], f2):                      # the walk the assembly itself uses, at every frame of the store
            assert ref.find_prev(S, c, after, f, 1 << 30) == ref.find_prev(S, c, before, f, 1 << 30)
    return n_seg


def test_a_moved_reference_carries_its_chain():
    """the chain behind (m1, c) after the call is, node for node, the chain behind (from, c) before it -- linked segments among them"""
    n_seg = [_moved_chains(sc) for sc in IDS]
    assert sum(n_seg) > 0, n_seg


def test_last_one_wins_and_gather_before_scatter():
    """hand-made lists over scene 0's tables: two views of one (m1, c), one slot in two tracks, a `from` that is another track's m1, a
    detached view that is not the last of its slot, entries outside the tables, a pointMap with a duplicate"""
    S, _ = SCENES[0]
    nC, N, nMap = S["nC"], S["N"], S["nMap"]
    rows = [(m, c) for m in range(nMap) for c in range(nC) if S["featRef"][m][c][0] >= 0]
    (a, ca), (b, cb) = rows[0], next(r for r in rows if r[0] != rows[0][0] and r[1] == rows[0][1])
    assert ca == cb
    c = ca
    sa, sb = int(S["featRef"][a][c][0]), int(S["featRef"][b][c][0])
    m3 = next(m for m in range(nMap) if m not in (a, b))
    views = [[0, c, sb, a, b, 1, -1],        # a takes b's reference in c ...
             [1, c, sa, b, a, 1, -1],        # ... and b takes a's: each must get the OTHER's old row
             [2, c, sa, m3, a, 2, -1],       # the same slot in a later track, detached
             [3, c, sa, m3, b, 0, -1],       # a later view of (m3, c) and of the slot: wins the row, the slot stays detached
             [4, nC, 0, a, b, 0, -1], [5, c, N, a, b, 0, -1], [6, c, 0, nMap, b, 0, -1], [7, c, 0, a, -1, 2, -1]]
    pm = [a, b, a, nMap, -1]
    sp = np.arange(15, dtype=np.float64).reshape(5, 3) + 0.5
    T = mref.apply_map(S, views, pm, sp)
    assert np.array_equal(T["featRef"][a][c], S["featRef"][b][c]) and np.array_equal(T["featRef"][b][c], S["featRef"][a][c])
    assert np.array_equal(T["featRef"][m3][c], S["featRef"][b][c]) and T["pointFeat"][m3][c] == sa
    assert T["slot2map"][c][sb] == a and T["slot2map"][c][sa] == -1
    assert np.array_equal(T["M"][a], sp[2]) and np.array_equal(T["M"][b], sp[1])
    assert T["counts"] == [4, 3, 1, 0, 2, 4 + 2 + 1 + 2]


def test_symbol_wrapper_and_sequence_exist():
    """the new entry is declared and exported, MergeConstraints.apply_map wraps it, MergeCamGroups is exported"""
    hdr = open(os.path.join(ROOT, "include", "coslam_hip.h")).read()
    assert re.search(r"\bcs_merge_constraints_apply_map_dev\(", hdr)
    assert hasattr(coslam_amd.lib(), "cs_merge_constraints_apply_map_dev")
    assert callable(getattr(coslam_amd.MergeConstraints, "apply_map", None))
    assert hasattr(coslam_amd, "MergeCamGroups") and callable(getattr(coslam_amd.MergeCamGroups, "run", None))
    shim = open(os.path.join(ROOT, "include", "shim", "app", "CoSLAMMergeConstraints.h")).read()
    assert "cs_merge_constraints_apply_map_dev" in shim
