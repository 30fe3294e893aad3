#!/usr/bin/env python
"""Stand-alone timing of the merge matcher at two sizes: the golden scale (120 slots per camera) and 2000 slots per camera,
small images of 192 x 144, one job.  Timed: the blocks (k_mm_prep + the cutter: cs_merge_match_run_dev with no job), the whole stage
(blocks, candidate list, matcher), and k_merge_match alone on the list the stage left (cs_merge_match_from_pairs_dev); the candidate list
is the difference.  HIP events around back-to-back calls after a warm-up, the median of 7 blocks with their spread.  Recorded with them:
the candidates that passed the epipolar / NCC test, the matches, and the matcher's round count.  Two textures: white noise blurred once
(decorrelates within a few pixels) and a smooth one (blurred 12 times: far more pairs pass nccMin).  Nothing is gated.

--front: descriptors -> pair choice on the scene of tests/mergefront_e2e.py (3 entries: skipped, no E, the true pair), the stretch of
MergeCamGroups.run_from_descriptors up to the counts merge_match_select reads: host-fed (MergeFront.run -> MergeMatcher.run -> counts) against
device-fed (MergeFront.enqueue -> MergeMatcher.run_front -> counts, results).  Wall time per call (median of 30 after 5, with the spread),
the calls that synchronise the stream, and how many of them found work in flight (the waits that stall the host)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import coslam_amd
from tests import mergematch_dev as D
from tests import mergematch_ref as R

WS, HS = 192, 144


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


def smooth(img, times):
    f = img.astype(np.float64)
    for _ in range(times):
        f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5.0
    f = (f - f.min()) / (f.max() - f.min())
    return np.ascontiguousarray((f * 255).astype(np.uint8))


def front_mode():
    import time
    from tests import mergefront_dev as FD, mergefront_e2e as FE, mergematch_e2e as E2

    S, cams, infos, front_cams, _want = FE.build()
    dc, keep = D.upload_cams(cams)
    fc, keep2 = FD.upload_cams(front_cams)
    pairs = [(int(i[1]), int(i[4])) for i in infos]
    mm = coslam_amd.MergeMatcher(S["nC"], S["N"], 4, S["N"], 1 << 14, S["N"])
    mf = coslam_amd.MergeFront(S["nC"], S["N"], FE.DIM, 4, FE.N_RANSAC)
    stream = torch.cuda.current_stream()
    waits = dict(calls=0, stalled=0)

    def counted(obj, name):
        inner = getattr(obj, name)

        def call(*a, **k):
            waits["calls"] += 1
            waits["stalled"] += 0 if stream.query() else 1
            return inner(*a, **k)
        setattr(obj, name, call)
    counted(mf, "results"), counted(mf, "_down"), counted(mm, "counts")

    def host_fed():
        got = mf.run(fc, pairs, n_ransac=FE.N_RANSAC, seed=FE.GEN_SEED)
        jl = [dict(iCam=p[0], jCam=p[1], E=g["E"], seeds=g["seeds"]) for p, g in zip(pairs, got) if g["surf_num"] >= 25 and g["emat_ok"]]
        mm.run(dc, E2.WS, E2.HS, jl)
        return mm.counts(len(jl))[-1]

    def device_fed():
        mf.enqueue(fc, pairs, n_ransac=FE.N_RANSAC, seed=FE.GEN_SEED)
        mm.run_front(dc, E2.WS, E2.HS, pairs, mf)
        cnt = mm.counts(len(pairs))
        mf.results(len(pairs))
        return cnt[-1]

    rows = []
    for name, run in (("host-fed jobs", host_fed), ("device-fed jobs", device_fed)) if hasattr(coslam_amd.lib(), "cs_merge_match_run_front_dev") \
            else (("host-fed jobs", host_fed),):
        for _ in range(5): last = run()
        ts = []
        for _ in range(30):
            torch.cuda.synchronize()
            waits.update(calls=0, stalled=0)
            t0 = time.perf_counter()
            last = run()
            ts.append((time.perf_counter() - t0) * 1e6)
        rows.append(last.tolist())
        print(f"{name:16s}: {np.median(ts):8.1f} us wall per call ({min(ts):.1f} .. {max(ts):.1f}); {waits['calls']} synchronising calls, "
              f"{waits['stalled']} with work in flight; true pair's count row {last.tolist()}")
    assert all(r == rows[0] for r in rows)
    print(f"seed rows the host-fed path downloads and uploads again: {len(pairs)} x {mf.max_pts} x 32 = {len(pairs) * mf.max_pts * 32} bytes down")
    mm.close(), mf.close()


if "--front" in sys.argv:
    front_mode()
    sys.exit(0)

for N in (120, 2000):
    for name, blur in (("noise", 0), ("smooth", 12)):
        cams, job, _ = R.shifted_pair_scene(N=N, seed=N, n_seeds=min(40, N // 3))
        if blur:
            rng = np.random.default_rng(N)
            big = smooth(rng.normal(0, 1, (HS + 64, WS + 64)), blur)
            cams[0]["imgSmall"] = np.ascontiguousarray(big[32:32 + HS, 32:32 + WS])
            cams[1]["imgSmall"] = np.ascontiguousarray(big[32 + 7:32 + 7 + HS, 32 - 12:32 - 12 + WS])
        mm = coslam_amd.MergeMatcher(2, N, 1, 64, 1 << 21, N)
        dc, keep = D.upload_cams(cams)
        mm.run(dc, WS, HS, [job])
        cnt = mm.counts(1)[0]
        p = [mm.buf.pairs], [mm.buf.pairCount]
        a = timed(lambda: mm.run(dc, WS, HS, []))
        b = timed(lambda: mm.run(dc, WS, HS, [job]))
        c = timed(lambda: mm.from_pairs(p[0], p[1], [dc[0]["xy"]], [dc[1]["xy"]], [job["seeds"]]))
        cnt2 = mm.counts(1)[0]
        assert list(cnt) == list(cnt2)
        print(f"{N} slots per camera, {name} texture, {len(job['seeds'])} seeds: {cnt[2]} candidates, {cnt[0]} matches, {cnt[3]} rounds, flags {cnt[1]}")
        print(f"  blocks (prep + cutter, 2 cameras):   {a[0]:.1f} us per call (blocks {a[1]:.1f} .. {a[2]:.1f})")
        print(f"  whole stage (uploads included):      {b[0]:.1f} us per call (blocks {b[1]:.1f} .. {b[2]:.1f})")
        print(f"  k_merge_match alone (uploads incl.): {c[0]:.1f} us per call (blocks {c[1]:.1f} .. {c[2]:.1f})")
        print(f"  candidate list (difference):         {b[0] - a[0] - c[0]:.1f} us", flush=True)
        mm.close()
