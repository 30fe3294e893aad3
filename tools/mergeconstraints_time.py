#!/usr/bin/env python
"""Stand-alone timing of the merge constraints: cs_merge_constraints_assemble_dev and cs_merge_info_dev at 8 cameras in two
groups of 4 with about 2000 slots per camera, 40 and 400 matches.  HIP events around back-to-back calls after a warm-up, the median of 7
blocks with their spread.  For scale: cs_merge_apply_run_dev, which consumes the constraints, is recorded at 3463 us.
Nothing is gated.  cs_merge_constraints_solve between them waits (it reads the problem back and runs the existing robust BA twice):
it is timed on the host clock, the median of 5 calls after one of warm-up."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import coslam_amd
from tests import mergeconstraints_ref as ref
from tests.mergeconstraints_dev import DeviceScene
from tests.mergeconstraints_golden_util import expand
from tests.mergeconstraints_scenes import make_scene

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
    S = expand(make_scene(0, spec, np.random.default_rng(7)))
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    f1 = int(S["key_frames"][ref.first_constrain(S["key_frames"], S["self_motion"], ids)[0]])
    f2 = S["frame0"] + S["nF"] - 1
    D = DeviceScene(S, dev)
    mc = coslam_amd.MergeConstraints(S["nC"], S["N"], len(S["matches"]), S["nMap"])
    dm = torch.from_numpy(np.ascontiguousarray(S["matches"], np.int32)).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    cams = coslam_amd.merge.merge_cams(D.cams)
    run_a = lambda: mc.assemble(D.th, cams, D.featRef.data_ptr(), S["nMap"], D.M.data_ptr(), D.groups.data_ptr(), S["gId1"], S["gId2"], S["maxiCam"],
                                S["maxjCam"], f1, f2, dm, stream_ptr=s)
    run_i = lambda: mc.info(D.groups.data_ptr(), S["gId1"], S["gId2"], stream_ptr=s)
    a = timed(run_a)
    h = mc.header()
    i = timed(run_i)
    print(f"{S['nC']} cameras x {S['N']} slots, {S['nMap']} map points, {len(S['matches'])} matches ({h.skippedMatches} skipped): verdict {h.verdict}, "
          f"{h.nMergedTracks} merged + {h.nUnmerged} unmerged tracks, {h.nPrevViews} views in the first-constrained frame -> {h.P} points, "
          f"{h.nObs} measurements, {h.nPose} poses", flush=True)
    print(f"  cs_merge_constraints_assemble_dev: {a[0]:.1f} us per call (blocks {a[1]:.1f} .. {a[2]:.1f})", flush=True)
    mc.solve()
    w = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter(); mc.solve(); w.append((time.perf_counter() - t0) * 1e3)
    st = [mc.solution(k)["stats"] for k in (0, 1)]
    print(f"  cs_merge_constraints_solve (host clock, read-back + two solves + upload): {np.median(w):.2f} ms per call ({min(w):.2f} .. {max(w):.2f}); "
          f"LM steps {st[0].nIterTotal} + {st[1].nIterTotal}, cost {st[0].cost0:.1f} -> {st[1].cost:.1f}, {st[1].nOutliers} outliers", flush=True)
    print(f"  cs_merge_info_dev ({mc.header().nInfo} infos): {i[0]:.1f} us per call (blocks {i[1]:.1f} .. {i[2]:.1f})", flush=True)
    mc.close(); D.th.close()
