"""diagnostic: stand-alone device time of cs_view_overlap_costs_dev / cs_camera_grouping_dev (coslam_amd/csrc/grouping.hip) on an otherwise
empty chip -- 8 and 16 cameras, N = 2000 slots, 2000 shared points per pair (every point held by every camera), the counting path (ratio 0) and the hull path (a positive ratio), with the pixels uniform in the image (a hull of a few dozen
vertices) and on a circle (every point a hull vertex: the Quickhull rounds' worst shape that a rig could meet).
    python tools/grouping_time.py [repetitions: 200]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from coslam_amd.grouping import (CameraGroups, camera_grouping_dev, camera_grouping_scratch_bytes, grouping_cams,  # noqa: E402
                                 view_overlap_costs_dev)
import ctypes as C  # noqa: E402

W, H, N = 640, 480, 2000
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)


def scene(nC, shape, n_map=65536):
    """N map points, spread over the whole map, each held by ALL cameras (a slot carries one point: this is the most a pair can share),
    so every one of the nC (nC - 1) ordered pairs has a hull of N points to take"""
    rng = np.random.RandomState(nC)
    pf = np.full((n_map, nC), -1, np.int32)
    xy = np.zeros((nC, 2, N))
    rows = rng.permutation(n_map)[:N]
    for c in range(nC):
        pf[rows, c] = rng.permutation(N)
    for c in range(nC):
        if shape == "uniform":
            xy[c, 0], xy[c, 1] = rng.uniform(0, W, N), rng.uniform(0, H, N)
        else:
            a = rng.uniform(0, 2 * np.pi, N)
            xy[c, 0], xy[c, 1] = W / 2 + 200 * np.cos(a), H / 2 + 200 * np.sin(a)
    R = np.tile(np.eye(3).reshape(9), (nC, 1))
    t = np.stack([[np.cos(2 * np.pi * c / nC), 0.0, np.sin(2 * np.pi * c / nC)] for c in range(nC)])
    return pf, xy, R, t


def timed(fn):
    s = torch.cuda.current_stream()
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(s)
    for _ in range(REPS):
        fn()
    e1.record(s)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS, (t1 - t0) * 1e6 / REPS


print(f"{torch.cuda.get_device_name(0)}; N = {N} slots, 65536 map rows, {N} shared points per pair, {REPS} back-to-back calls; microseconds per call")
for nC in (8, 16):
    for shape in ("uniform", "circle"):
        pf, xy, R, t = scene(nC, shape)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_pf, d_xy, d_R, d_t = up(pf), up(xy), up(R), up(t)
        d_flags, d_count = torch.zeros(pf.shape[0], dtype=torch.uint8, device=dev), torch.tensor([pf.shape[0]], dtype=torch.int32, device=dev)
        cams = grouping_cams([dict(xy=d_xy[c].data_ptr(), R=d_R[c].data_ptr(), t=d_t[c].data_ptr()) for c in range(nC)])
        v, n = torch.zeros(nC * nC, dtype=torch.float64, device=dev), torch.zeros(nC * nC, dtype=torch.int32, device=dev)
        a = torch.zeros(nC * nC, dtype=torch.float64, device=dev)
        g = torch.zeros(C.sizeof(CameraGroups), dtype=torch.uint8, device=dev)
        scr = torch.zeros(camera_grouping_scratch_bytes(nC, N), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        common = (st, cams, N, pf.shape[0], d_count.data_ptr(), d_pf.data_ptr(), d_flags.data_ptr(), W, H, v.data_ptr(), n.data_ptr(), scr.data_ptr())
        for ratio in (0.0, 0.2):
            dc, hc = timed(lambda: view_overlap_costs_dev(*common, minOverlapNum=0, minOverlapAreaRatio=ratio))
            dg, hg = timed(lambda: camera_grouping_dev(*common, 1.0, g.data_ptr(), minOverlapNum=0, minOverlapAreaRatio=ratio))
            torch.cuda.synchronize()
            G = CameraGroups.from_bytes(g.cpu().numpy().tobytes())
            if ratio > 0:
                view_overlap_costs_dev(*common, minOverlapNum=0, minOverlapAreaRatio=ratio, d_hullArea=a.data_ptr())
                torch.cuda.synchronize()
                area = f", hull area of pair (0, 1) {float(a[1]) / (W * H):.3f} W H"
            else:
                area = ""
            print(f"{nC:2d} cameras, {shape:7s} pixels, ratio {ratio:.1f} ({'hull path: 2 launches' if ratio > 0 else 'counting path: 1 launch'}): "
                  f"costs {dc:7.1f} device / {hc:5.1f} host, grouping {dg:7.1f} device / {hg:5.1f} host; {G.groupNum} groups, "
                  f"nShare(0, 1) = {int(n[1])}{area}")
