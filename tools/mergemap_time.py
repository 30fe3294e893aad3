#!/usr/bin/env python
"""Stand-alone timing of the merge map update: cs_merge_constraints_apply_map_dev alone, at the two sizes of
tools/mergeconstraints_time.py (8 cameras in two groups of 4 with about 2000 slots per camera, 40 and 400 matches), with the solved
coordinates (behind cs_merge_constraints_solve) and without.  HIP events around back-to-back calls after a warm-up, the median of 7 blocks
with their spread.  Every call applies the same list to the same tables: the first one merges, the later ones do the same gathers, bids and
writes over the merged state.  For scale: the assembly in front of it is recorded at 139 / 372 us, the solve at 3.8 ms.  Nothing is gated."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import coslam_amd
from tests import mergeconstraints_ref as ref
from tests.mergeconstraints_dev import DeviceScene
from tests.mergeconstraints_golden_util import expand
from tests.mergeconstraints_scenes import make_scene
from tests.mergemap_dev import MapTables, with_tables

dev = torch.device("cuda:0")

def timed(run, reps=10, blocks=7, warm=3):
    for _ in range(warm): run()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): run()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return np.median(out), min(out), max(out)


for n_match in (40, 400):
    spec = dict(groups=[[0, 1, 2, 3], [4, 6, 5, 7]], g=(0, 1), ij=(1, 5), nF=12, gaps=(2, 3, 4), moved=[{0, 5}, set(), set(range(8))],
                nA=1700 - n_match, nB=1700 - n_match, nMatch=n_match, plant="mixed")
    S = with_tables(expand(make_scene(0, spec, np.random.default_rng(7))))
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    f1 = int(S["key_frames"][ref.first_constrain(S["key_frames"], S["self_motion"], ids)[0]])
    f2 = S["frame0"] + S["nF"] - 1
    D = DeviceScene(S, dev)
    mc = coslam_amd.MergeConstraints(S["nC"], S["N"], len(S["matches"]), S["nMap"])
    s = torch.cuda.current_stream().cuda_stream
    mc.assemble(D.th, D.cams, D.featRef.data_ptr(), S["nMap"], D.M.data_ptr(), D.groups.data_ptr(), S["gId1"], S["gId2"], S["maxiCam"], S["maxjCam"],
                f1, f2, S["matches"], stream_ptr=s)
    h = mc.header()
    T = MapTables(D)
    ptrs = [D.slot2map[c].data_ptr() for c in range(S["nC"])]
    run = lambda: mc.apply_map(ptrs, T.pointFeat.data_ptr(), D.featRef.data_ptr(), T.refStatic.data_ptr(), S["nMap"], D.M.data_ptr(), True,
                               T.counts.data_ptr(), stream_ptr=s)
    a = timed(run)                                   # no solve yet: the list alone
    mc.solve()
    T.counts.zero_()
    run()
    torch.cuda.synchronize()
    one = T.counts.tolist()
    b = timed(run)
    print(f"{S['nC']} cameras x {S['N']} slots, {S['nMap']} map points, {len(S['matches'])} matches: verdict {h.verdict}, {h.nMergeViews} merge-list "
          f"entries, {h.P} problem points; one call: {one[0]} views applied, {one[1]} references moved, {one[2]} features detached, {one[3]} f1 nodes "
          f"marked, {one[4]} map rows written, {one[5]} entries lost", flush=True)
    print(f"  cs_merge_constraints_apply_map_dev, list only:        {a[0]:.1f} us per call (blocks {a[1]:.1f} .. {a[2]:.1f})", flush=True)
    print(f"  cs_merge_constraints_apply_map_dev, list and points:  {b[0]:.1f} us per call (blocks {b[1]:.1f} .. {b[2]:.1f})", flush=True)
    mc.close(); D.th.close()
