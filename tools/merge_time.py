"""diagnostic: stand-alone device time of cs_merge_check_dev (coslam_amd/csrc/merge.hip) on an otherwise empty chip -- 8 and 16 cameras,
N = 2000 slots, every slot a feature with its own map point, every camera seeing every point (all cameras at one place, looking one way), in
three settings: all singleton groups with the projections uniform over the image (hulls of a few dozen vertices), all singleton groups with
all projections on a circle (every point a hull vertex: the Quickhull rounds' and the pixel test's worst shape), and ONE group (the
predicated exit: every workgroup leaves after one word).
    python tools/merge_time.py [repetitions: 200]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from coslam_amd.grouping import CameraGroups  # noqa: E402
from coslam_amd.merge import MergeCandidates, merge_cams, merge_check_dev, merge_check_scratch_bytes  # noqa: E402

W, H, N, F = 640, 480, 2000, 500.0
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)


def scene(nC, shape):
    """nC cameras with K (F, W / 2, H / 2), R = I, t = 0; camera c's N slots carry map rows c N .. (c + 1) N - 1, whose points project -- into
    EVERY camera -- uniformly over the image or onto a circle; the feature pixels uniform over the image"""
    rng = np.random.RandomState(nC)
    if shape == "uniform":
        px, py = rng.uniform(1, W - 1, nC * N), rng.uniform(1, H - 1, nC * N)
    else:
        a = rng.uniform(0, 2 * np.pi, nC * N)
        px, py = W / 2 + 200 * np.cos(a), H / 2 + 200 * np.sin(a)
    d = rng.uniform(4, 8, nC * N)
    pts = np.stack([(px - W / 2) / F * d, (py - H / 2) / F * d, d], axis=1)
    xy = np.stack([np.stack([rng.uniform(0, W, N), rng.uniform(0, H, N)]) for _ in range(nC)])   # x[N] then y[N]
    s2m = np.arange(nC * N, dtype=np.int32).reshape(nC, N)
    K = np.tile(np.array([F, 0, W / 2, 0, F, H / 2, 0, 0, 1.0]), (nC, 1))
    R = np.tile(np.eye(3).reshape(9), (nC, 1))
    return pts, xy, s2m, K, R, np.zeros((nC, 3))


def record(groups):
    g = CameraGroups()
    g.groupNum = len(groups)
    for k, cams in enumerate(groups):
        g.num[k] = len(cams)
        for q, c in enumerate(cams):
            g.camIds[k][q], g.groupId[c] = c, k
    return np.frombuffer(bytes(g), dtype=np.uint8).copy()


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


print(f"{torch.cuda.get_device_name(0)}; N = {N} slots per camera, every slot a feature, every point in every image, {REPS} back-to-back calls "
      f"after 10 of warm-up; microseconds per call")
for nC in (8, 16):
    for shape, groups in (("uniform", [[c] for c in range(nC)]), ("circle", [[c] for c in range(nC)]), ("uniform", [list(range(nC))])):
        pts, xy, s2m, K, R, t = scene(nC, shape)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_pts, d_xy, d_s2m, d_K, d_R, d_t = up(pts), up(xy), up(s2m), up(K), up(R), up(t)
        d_state = torch.zeros((nC, N), dtype=torch.int32, device=dev)
        d_flags, d_count = torch.zeros(len(pts), dtype=torch.uint8, device=dev), torch.tensor([len(pts)], dtype=torch.int32, device=dev)
        d_groups = up(record(groups))
        cams = merge_cams([dict(xy=d_xy[c].data_ptr(), state=d_state[c].data_ptr(), slot2map=d_s2m[c].data_ptr(), K=d_K[c].data_ptr(),
                                R=d_R[c].data_ptr(), t=d_t[c].data_ptr()) for c in range(nC)])
        out = torch.zeros(C.sizeof(MergeCandidates), dtype=torch.uint8, device=dev)
        scr = torch.zeros(merge_check_scratch_bytes(nC, N), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        dd, hh = timed(lambda: merge_check_dev(st, cams, N, len(pts), d_count.data_ptr(), d_pts.data_ptr(), d_flags.data_ptr(), W, H,
                                               d_groups.data_ptr(), 1, out.data_ptr(), scr.data_ptr()))
        torch.cuda.synchronize()
        m = MergeCandidates.from_bytes(out.cpu().numpy().tobytes())
        print(f"{nC:2d} cameras, {len(groups):2d} group(s), {shape:7s} projections: {dd:8.1f} device / {hh:5.1f} host; nMergeInfo {m.nMergeInfo}, "
              f"nInCam(0, 1) = {m.nInCam[0][1]}, inNum(0, 1) = {m.inNum[0][1]} of {m.nFeat[1]}")
