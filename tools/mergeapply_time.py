#!/usr/bin/env python
"""Stand-alone timing of a merge's device sequence: cs_merge_apply_run_dev at 8 cameras x 24 key frames x 5 frames per
interval, and cs_recompute_map_points_keyfrms_dev over 10 000 points beside cs_refine_map_points_ref_dev over the same rows (the only
yardstick there is: all frames, at most histLen nodes, no head test).  HIP events around back-to-back calls after a warm-up, the median of
7 blocks with their spread.  Nothing is gated: no comparable figure existed before."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import coslam_amd
from coslam_amd.synth import make_merge_pose_graph
from tests.mergeapply_dev import load_history
from tests.mergeapply_golden_util import inv_k

dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
K0 = np.array([520.0, 0.0, 320.0, 0.0, 515.0, 240.0, 0.0, 0.0, 1.0])


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


n_cams, n_key, step = 8, 24, 5
m = make_merge_pose_graph(n_cams, n_key, 15, 4, seed=1, frames_per_interval=step)
ch = m["chains"]
nF = (n_key - 1) * step + 1
frame0 = 1000
key_frames = np.array([frame0 + k * step for k in range(n_key)], np.int32)
# 10 000 points: every camera sees a point over a window of 4-9 key-frame intervals that ends at a key frame; a slot per point
nP, N = 10000, 10000
rng = np.random.default_rng(2)
ref = np.full((nP, n_cams, 4), -1, np.int32)
ref[:, :, 1:3] = 0
hk = rng.integers(9, n_key, nP)
span = rng.integers(4, 10, nP)
for c in range(n_cams):
    ref[:, c, 0] = np.arange(nP)
    ref[:, c, 1] = frame0 + hk * step
    ref[:, c, 2] = frame0 + (hk - span) * step
X = np.stack([rng.uniform(-1.5, 1.5, nP), rng.uniform(-1.5, 1.5, nP), rng.uniform(14, 20, nP)], axis=1)
hR, hT = ch["nodeR"].reshape(n_cams, nF, 3, 3), ch["nodeT"].reshape(n_cams, nF, 3)
Xc = np.einsum("cfij,pj->cfpi", hR, X) + hT[:, :, None, :]
xy = np.concatenate([K0[0] * Xc[..., 0] / Xc[..., 2] + K0[2], K0[4] * Xc[..., 1] / Xc[..., 2] + K0[5]], axis=2) + rng.normal(size=(n_cams, nF, 2 * N)) * 0.3
S = dict(K=np.tile(K0, (n_cams, 1)), iK=np.tile(inv_k(K0), (n_cams, 1)), histR=ch["nodeR"].reshape(n_cams, nF, 9), histT=ch["nodeT"].reshape(n_cams, nF, 3),
         histXY=xy, N=N, nC=n_cams, nF=nF, frame0=frame0, featRef=ref, segPool=np.full((n_cams, 0, 4), -1, np.int32))
th, cams, keep = load_history(S, dev, hist_len=64)
plan = dict(fixed_kf=0, node_kf=m["node_kf"], node_cam=m["node_cam"], fixed=m["fixed"], id1=m["id1"], id2=m["id2"], scale_id=m["scale_id"])
ma = coslam_amd.MergeApply(plan, key_frames, n_cams)
sc = m["scale_id"] >= 0
dR, dT = T(m["edgeR"][sc]), T(m["edgeT"][sc])
s = torch.cuda.current_stream().cuda_stream
span0 = (torch.zeros((n_cams, nF, 9), dtype=torch.float64, device=dev), torch.zeros((n_cams, nF, 3), dtype=torch.float64, device=dev))
th.get_span_dev(s, frame0, nF, span0[0].data_ptr(), span0[1].data_ptr())


def run_apply():   # (every call starts from the drifted poses: the span is put back first, inside the timed region -- one small copy launch)
    th.set_span_dev(s, frame0, nF, span0[0].data_ptr(), span0[1].data_ptr())
    ma.run(th, dR, dT)


med, lo, hi = timed(run_apply)
ma.status()
print(f"cs_merge_apply_run_dev {n_cams} cameras x {n_key} key frames x {step} frames per interval ({n_cams * nF} poses, incl. one set_span): "
      f"{med:.1f} us per call (blocks {lo:.1f} .. {hi:.1f})", flush=True)
d_ref, d_M, d_cov = T(ref), T(X + 0.02), torch.zeros((nP, 9), dtype=torch.float64, device=dev)
d_ff, d_lf, d_fl = T(ref[:, 0, 2].copy()), T(ref[:, 0, 1].copy()), torch.zeros(nP, dtype=torch.uint8, device=dev)
d_cnt, d_keys = torch.zeros(4, dtype=torch.int32, device=dev), T(key_frames)
run_rk = lambda: coslam_amd.recompute_map_points_keyfrms_dev(th, s, cams, d_ref.data_ptr(), nP, None, d_ff.data_ptr(), d_lf.data_ptr(), d_fl.data_ptr(),
                                                             frame0, frame0 + nF - 1, d_keys.data_ptr(), n_key, d_M.data_ptr(), d_cov.data_ptr(), 3.0, True,
                                                             d_cnt.data_ptr())
med, lo, hi = timed(run_rk)
print(f"cs_recompute_map_points_keyfrms_dev {nP} points x {n_cams} cameras, chains of 20-45 frames (4-9 key nodes): {med:.1f} us per call "
      f"(blocks {lo:.1f} .. {hi:.1f}); counts of one call {(d_cnt // (3 + 7 * 10)).tolist()}", flush=True)
run_rf = lambda: th.refine_map_points_ref_dev(s, cams, d_ref.data_ptr(), nP, d_M.data_ptr(), d_cov.data_ptr(), 3.0)
med, lo, hi = timed(run_rf)
print(f"cs_refine_map_points_ref_dev over the same rows (every frame a node, histLen 64): {med:.1f} us per call (blocks {lo:.1f} .. {hi:.1f})", flush=True)
ma.close(); th.close()
