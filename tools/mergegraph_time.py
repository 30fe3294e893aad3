#!/usr/bin/env python
"""Stand-alone timing of the merge key-graph relaxation (cs_posegraph_relax_scaled_dev: computeNewCameraRotations +
computeNewCameraTranslations4) on merge graphs of 8 x 6, 8 x 24 and 16 x 24 (cameras x key frames): HIP events around back-to-back
calls after a warm-up, median of 5 blocks; numpy's dense lstsq of the same two systems on the host beside it."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import coslam_amd
from coslam_amd.synth import make_merge_pose_graph
from tests import mergegraph_ref as ref

dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
for shape in ((8, 6, 3, 4), (8, 24, 15, 4), (16, 24, 15, 8)):
    m = make_merge_pose_graph(*shape, seed=1)
    h = coslam_amd.PoseGraphs([(m["fixed"], m["id1"], m["id2"])], scale_ids=[m["scale_id"]])
    d = {k: T(m[k]) for k in ("nodeR", "nodeT", "edgeR", "edgeT")}
    nR, nT, eS = torch.zeros_like(d["nodeR"]), torch.zeros_like(d["nodeT"]), torch.zeros(len(m["id1"]), dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    run = lambda: h.relax_scaled_dev(s, d["nodeR"].data_ptr(), d["nodeT"].data_ptr(), d["edgeR"].data_ptr(), d["edgeT"].data_ptr(),
                                     nR.data_ptr(), nT.data_ptr(), eS.data_ptr())
    for _ in range(5): run()
    torch.cuda.synchronize()
    h.status(s)
    reps, blocks = 20, []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): run()
        e1.record(); torch.cuda.synchronize()
        blocks.append(e0.elapsed_time(e1) / reps * 1e3)
    t0 = time.perf_counter()
    A, b, _ = ref.rotation_system(m["fixed"], m["nodeR"], m["id1"], m["id2"], m["edgeR"])
    At, bt, _, _ = ref.translation4_system(m["fixed"], m["nodeT"], m["id1"], m["id2"], m["edgeR"], m["edgeT"], m["scale_id"])
    t1 = time.perf_counter()
    x = np.linalg.lstsq(A, b, rcond=None)[0]
    xt = np.linalg.lstsq(At, bt, rcond=None)[0]
    t2 = time.perf_counter()
    err = np.abs(nT.cpu().numpy()[m["fixed"] == 0].reshape(-1) - xt[:3 * int((m["fixed"] == 0).sum())]).max()
    print(f"{shape[0]} x {shape[1]}: {h.counts()} {h.scaled_counts()}  relax_scaled_dev {np.median(blocks):.1f} us per call "
          f"(blocks {min(blocks):.1f} .. {max(blocks):.1f}); numpy dense lstsq of the 9n and the 3n+1 system: {(t2 - t1) * 1e3:.1f} ms "
          f"(+ {(t1 - t0) * 1e3:.0f} ms to fill them); |dt| between the two {err:.1e}", flush=True)
    h.close()
