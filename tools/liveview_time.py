"""diagnostic: stand-alone device time of cs_liveview_frame_dev / cs_map_counts_dev / cs_liveview_trails_dev (coslam_amd/csrc/liveview.hip) on
an otherwise empty chip -- 65536 map rows, 8 and 16 cameras, 10 % of the rows taking part, 200 of them dynamic; frames that publish a
snapshot into the pinned ring and frames that do not; the trails at trjLen 150 over 200 ids.
    python tools/liveview_time.py [repetitions: 200]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from coslam_amd.liveview import LiveHeader, LiveView, MapCounts, map_counts_dev, map_counts_scratch_bytes  # noqa: E402

N_MAP, N_DYN, TRJ = 65536, 200, 150
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)


def scene(nC):
    rng = np.random.RandomState(nC)
    pf = np.full((N_MAP, nC), -1, np.int32)
    rows = np.sort(rng.permutation(N_MAP)[:N_MAP // 10])
    for r in rows:
        cams = np.nonzero(rng.uniform(size=nC) < 0.4)[0]
        pf[r, cams if len(cams) else [0]] = rng.randint(0, 2000)
    flags = np.zeros(N_MAP, np.uint8)
    flags[rng.permutation(rows)[:N_DYN]] = 1
    return pf, flags, rng.normal(size=(N_MAP, 3)), len(rows)


def timed(fn, reps=REPS):
    s = torch.cuda.current_stream()
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, (t1 - t0) * 1e6 / reps


print(f"{torch.cuda.get_device_name(0)}; {N_MAP} map rows, {N_MAP // 10} taking part, {N_DYN} dynamic, {REPS} back-to-back calls; "
      "microseconds per call (device: between two events around the calls; host: the enqueue)")
for nC in (8, 16):
    pf, flags, pts, n_cur = scene(nC)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_pf, d_flags, d_pts = up(pf), up(flags), up(pts)
    d_count = torch.tensor([N_MAP], dtype=torch.int32, device=dev)
    d_R, d_t = torch.zeros((nC, 9), dtype=torch.float64, device=dev), torch.zeros((nC, 3), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for every, what in ((1, "every frame published"), (1 << 30, "no frame published")):
        view = LiveView(nC, 8192, 1024, depth=4, trail_depth=TRJ, every=every)
        frame = [1]

        def one():
            view.frame_dev(st, frame[0], N_MAP, d_count.data_ptr(), d_pf.data_ptr(), d_flags.data_ptr(), d_pts.data_ptr(), d_R.data_ptr(),
                           d_t.data_ptr())
            frame[0] += 1

        d, h = timed(one)
        line = f"{nC:2d} cameras, cs_liveview_frame_dev, {what}: {d:7.1f} device / {h:5.1f} host"
        if every == 1:
            snap = view.snapshot()
            line += f"; {C.sizeof(LiveHeader) + 32 * snap['nCur']} bytes per published frame (nCur {snap['nCur']} of {n_cur}, nDyn {snap['nDyn']})"
            n, ids, lens = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (1, 1024, 1024))
            tp = torch.zeros((1024, TRJ, 3), dtype=torch.float64, device=dev)
            d, h = timed(lambda: view.trails_dev(st, TRJ, n.data_ptr(), ids.data_ptr(), lens.data_ptr(), tp.data_ptr()))
            line += f"\n{nC:2d} cameras, cs_liveview_trails_dev, trjLen {TRJ}: {d:7.1f} device / {h:5.1f} host; {int(n.item())} trails of {int(lens.max().item())} points"
        print(line)
        view.close()
    scr = torch.zeros(map_counts_scratch_bytes(), dtype=torch.uint8, device=dev)
    out = torch.zeros(C.sizeof(MapCounts), dtype=torch.uint8, device=dev)
    d, h = timed(lambda: map_counts_dev(st, nC, N_MAP, d_count.data_ptr(), d_pf.data_ptr(), d_flags.data_ptr(), out.data_ptr(), scr.data_ptr()))
    c = MapCounts.from_buffer_copy(out.cpu().numpy().tobytes())
    print(f"{nC:2d} cameras, cs_map_counts_dev: {d:7.1f} device / {h:5.1f} host; nStatic {c.nStatic}, nDynamic {c.nDynamic}")
