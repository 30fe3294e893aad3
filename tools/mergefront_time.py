#!/usr/bin/env python
"""Stand-alone timing of the merge front: 700 key points per camera (dim 64; 250 true pairs at 0.3 px of noise, 150 gross
outliers, 300 points without a partner), 1 / 8 / 64 jobs (the same camera pair: job k draws its own samples), 200 and 2000 hypotheses.
Timed, HIP events around back-to-back calls after a warm-up, the median of 7 blocks with their spread:
  descriptors   cs_merge_front_match_dev (validity, the search, the ordered list and its point rows)
  ransac        cs_merge_front_from_matches_dev on the list the first stage left (hypotheses, scoring, best, refit, seeds; includes the
                upload of the match lists)
  whole         cs_merge_front_run_dev
and, wall clock, `read-back`: cs_merge_front_results plus the seed rows of every job.  Next to them the numpy restatement
(tests/mergefront_ref.py) on the same inputs, one job, on the CPU.  Nothing is gated."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import coslam_amd
from tests import mergefront_dev as D
from tests import mergefront_ref as R
from tests import mergefront_scenes as S


def timed(run, reps=5, blocks=7, warm=2):
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


sc = S.two_view_scene(250, 150, 0.3, 0, 64, 300)
cams = [sc["cam1"], sc["cam2"]]
dc, keep = D.upload_cams(cams)
print(f"key points {len(cams[0]['pts'])} / {len(cams[1]['pts'])}, dim 64, planted matches {len(sc['matches'])} ({int(sc['truth'].sum())} true)")
for nh in (200, 2000):
    t0 = time.perf_counter()
    ref = R.front_job(cams[0], cams[1], n_ransac=nh, seed=1, k=0)
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    R.match_surf(cams[0]["pts"], cams[0]["desc"], cams[1]["pts"], cams[1]["desc"])
    t_ms = time.perf_counter() - t0
    print(f"numpy restatement, 1 job, {nh} hypotheses: {t_ref * 1e3:.0f} ms (matchSurf {t_ms * 1e3:.0f} ms): surfNum {ref['surf_num']}, inliers {ref['inlier_num']}, "
          f"rounds {ref['rounds']}")
    for nj in (1, 8, 64):
        mf = coslam_amd.MergeFront(2, 700, 64, 64, nh)
        pairs = [(0, 1)] * nj
        mf.match(dc, pairs)
        n = int(mf.counts(1)[0])
        lists = [mf.matches(k, n)[0] for k in range(nj)]
        a = timed(lambda: mf.match(dc, pairs))
        b = timed(lambda: mf.from_matches(dc, pairs, lists, n_ransac=nh, seed=1))
        c = timed(lambda: mf.enqueue(dc, pairs, n_ransac=nh, seed=1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = mf.results(nj)
        for k, r in enumerate(res): mf.seeds(k, r["inlier_num"])
        t_rb = time.perf_counter() - t0
        inl = [r["inlier_num"] for r in res]
        print(f"jobs {nj:2d} hyp {nh:4d}: descriptors {a[0]:8.1f} us [{a[1]:.1f} .. {a[2]:.1f}]  ransac {b[0]:8.1f} us [{b[1]:.1f} .. {b[2]:.1f}]  "
              f"whole {c[0]:8.1f} us [{c[1]:.1f} .. {c[2]:.1f}]  read-back {t_rb * 1e6:8.1f} us  surfNum {res[0]['surf_num']} inliers {min(inl)} .. {max(inl)} "
              f"rounds {min(r['rounds'] for r in res)} .. {max(r['rounds'] for r in res)}")
        mf.close()
