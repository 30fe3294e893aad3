"""The run's result files from the frame loops (CoSLAM::exportResults behind the reference's frame loop, src/gui/CoSLAMThread.cpp):
FrameLoop.export_results / tools/cxx/frame_loop.cpp with COSLAM_EXPORT_DIR, through cs_loop_export_results over the pose history's store
and its whole-run archive (cs_track_history_set_archive), the feature references and the map.  The files are pinned against a host
restatement written by the host writer (export_results_v1) from what the test watched the loop do frame by frame."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILES = lambda n_cams: ["input_videos.txt", "mappts.txt"] + [f"{c}_campose.txt" for c in range(n_cams)] + [f"{c}_featpts.txt" for c in range(n_cams)]  # noqa: E731


def _setup():
    import torch

    import bench

    dev = torch.device("cuda", 0)
    frames = bench.render_video(list(range(bench.N_CAMS)), bench.N_FRAMES)
    video = {c: torch.from_numpy(frames[c]).to(dev) for c in range(bench.N_CAMS)}
    return bench, bench.build_scene(), video


def _loop(bench, sc, video, **kw):
    from coslam_amd.frameloop import FrameLoop, LoopConfig

    cfg = LoopConfig(n_cams=bench.N_CAMS, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                     n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG, **kw)
    loop = FrameLoop(cfg, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0,
                     associate=bench.associate)
    loop.first_frame()
    return loop


def _read(d, n_cams):
    return {f: open(os.path.join(d, f), "rb").read() for f in FILES(n_cams)}


@pytest.mark.timeout(600)
def test_export_leaves_the_state_untouched(hip, tmp_path):
    """120 frames with a 64-frame store: with the archive on (frames 0..56 copied into it as they leave the store) and the export run,
    the loop ends in the digest of the same run with both off"""
    bench, sc, video = _setup()
    digests = []
    for export in (0, 256):
        loop = _loop(bench, sc, video, hist=64, hist_store=64, export_frames=export)
        for n in range(120):
            loop.step(n + 1, n % bench.KEY_EVERY == 0)
        loop.drain()
        if export:
            assert loop.pose_upd.archive_frames == 121 - 64
            st = loop.export_results(tmp_path / "out")
            assert st["features_from_archive"] > 0
            assert st["points"] > 0 and st["features"] > 0
            assert all(os.path.getsize(tmp_path / "out" / f) > 0 for f in FILES(bench.N_CAMS))
        digests.append(loop.digest())
        del loop
    assert digests[0] == digests[1]


def _chains(fref, segs, seg_cnt, seg_cap, flags, cur):
    """the resolution rule, restated: (camera, frame, slot, point) of every node of every certainly static point's chains"""
    out = []
    n_map, NA = fref.shape[:2]
    for p in np.nonzero((flags & 7) == 0)[0]:
        for c in range(NA):
            slot, frame, first, seg = (int(v) for v in fref[p, c])
            if slot < 0:
                continue
            runs = [(slot, first, frame)]
            n_seg = min(int(seg_cnt[c]), seg_cap)
            hops = 0
            while 0 <= seg < n_seg and hops <= n_seg:
                g = segs[c, seg]
                runs.append((int(g[0]), int(g[2]), int(g[1])))
                seg, hops = int(g[3]), hops + 1
            for s, lo, hi in runs:
                f = np.arange(max(lo, 0), min(hi, cur) + 1)
                if len(f):
                    out.append(np.stack([np.full(len(f), c), f, np.full(len(f), s), np.full(len(f), p)], 1))
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


@pytest.mark.timeout(900)
def test_archived_poses_are_final_and_the_files_match_a_host_restatement(hip, tmp_path):
    """200 frames with a 64-frame store: frames spill into the archive from frame 64 on, BA windows are applied, bMerge runs every 50th
    frame.  <c>_campose.txt holds, for every frame, the last pose the store showed of it; all six files are byte-identical to what
    export_results_v1 writes from a numpy restatement of the resolution rule over the recorded pixels, the references and the pools."""
    import torch

    import coslam_amd

    bench, sc, video = _setup()
    T, STORE = 200, 64
    loop = _loop(bench, sc, video, hist=64, hist_store=STORE, export_frames=256, merge_every=50)
    NA, N, h = bench.N_CAMS, loop.cfg.n_feat, loop.pose_upd
    poses, xy, unified = {}, {}, {}
    dR, dT = torch.zeros((NA, STORE, 9), dtype=torch.float64, device=loop.dev), torch.zeros((NA, STORE, 3), dtype=torch.float64, device=loop.dev)

    def watch(i):
        torch.cuda.synchronize()
        xy[i] = loop.d_xy.cpu().numpy().copy()
        first = max(0, i - STORE + 1)
        n = i - first + 1
        h.get_span_dev(loop.pose_s.cuda_stream, first, n, dR.data_ptr(), dT.data_ptr())
        torch.cuda.synchronize()
        R, t = dR.cpu().numpy(), dT.cpu().numpy()
        for k in range(n):
            poses[first + k] = (R[:, k].copy(), t[:, k].copy())
        if i > 0 and i % loop.cfg.merge_every == 0:   # a bMerge frame: points unified away (cs_register_decide_merge_dev's d_counts[2], this frame's)
            unified[i] = int(loop._dec["mcnt"][2].item())

    watch(0)
    for n in range(T):
        loop.step(n + 1, n % bench.KEY_EVERY == 0)
        watch(n + 1)
    loop.drain()
    assert loop.applied > 0 and h.archive_frames == T + 1 - STORE and h.first_frame == 0
    st = loop.export_results(tmp_path / "dev", video_paths=[f"/data/cam{c}.avi" for c in range(NA)], start_frame_in_video=7)

    # the restatement
    fref = loop.d_fref.cpu().numpy()
    flags = loop.d_mapflags.cpu().numpy()
    segs = h.segments()
    seg_cnt, seg_cap = h.segment_counts()
    nodes = _chains(fref, segs, seg_cnt, seg_cap, flags, T)
    nodes = nodes[np.lexsort((nodes[:, 3], nodes[:, 2], nodes[:, 1], nodes[:, 0]))]   # camera, frame, slot, point
    pts = np.unique(nodes[:, 3])
    M, cov = loop.d_map.cpu().numpy(), loop.d_cov.cpu().numpy().reshape(-1, 9)
    frames = np.arange(0, T + 1)
    cams = []
    for c in range(NA):
        nc_ = nodes[nodes[:, 0] == c]
        ptr = np.searchsorted(nc_[:, 1], np.arange(0, T + 2)).astype(np.int32)
        fxy = np.array([[xy[f][c][s], xy[f][c][N + s]] for _, f, s, _ in nc_], np.float64).reshape(-1, 2)
        cams.append(dict(videoFilePath=f"/data/cam{c}.avi", K=sc.K, kc=np.zeros(5), W=bench.W, H=bench.H, startFrameInVideo=7,
                         poseFrame=frames, poseR=np.stack([poses[f][0][c] for f in frames]), poseT=np.stack([poses[f][1][c] for f in frames]),
                         featPtr=ptr, featPointId=nc_[:, 3].astype(np.int64), featXY=fxy))
    coslam_amd.export_results_v1(tmp_path / "host", cams, T, pts.astype(np.int64), M[pts], cov[pts])
    a, b = _read(tmp_path / "dev", NA), _read(tmp_path / "host", NA)
    for f in FILES(NA):
        assert a[f] == b[f], f
    # the run exercised the hard cases
    spilled = T + 1 - STORE
    assert st["points"] == len(pts) and st["features"] == len(nodes)
    assert st["features_from_archive"] == int((nodes[:, 1] < spilled).sum()) > 0
    assert int(loop.d_fref_counts[2].item()) > 0, "no re-linked segment"
    assert sorted(unified) == [50, 100, 150, 200] and sum(unified.values()) > 0, f"no unification: {unified}"


@pytest.mark.timeout(600)
def test_a_full_archive_fails_the_push_loudly(hip, tmp_path):
    """an archive too small for the run: the push that would overflow it fails with cs_last_error's message, nothing is dropped silently"""
    import coslam_amd

    bench, sc, video = _setup()
    loop = _loop(bench, sc, video, hist=64, hist_store=64, export_frames=4)
    with pytest.raises(coslam_amd.CoslamHipError, match="archive is full"):
        for n in range(80):
            loop.step(n + 1, n % bench.KEY_EVERY == 0)
    loop.drain()
    assert loop.pose_upd.archive_frames == 4


@pytest.mark.timeout(1200)
def test_the_cxx_loop_writes_the_python_loops_files(hip, tmp_path):
    """tools/cxx/frame_loop.bin with COSLAM_EXPORT_DIR over bench.py's workload writes the files the Python loop writes after the same
    frames"""
    import bench

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "cxx", "frame_loop.bin")
    assert os.path.exists(exe), "tools/cxx/frame_loop.bin missing: __graft_entry__.build()"
    wl = str(tmp_path / "workload.bin")
    frames = bench.render_video(list(range(bench.N_CAMS)), bench.N_FRAMES)
    sc = bench.build_scene()
    bench.export_workload(wl, sc, frames, bench.build_joint_problem(sc), bench.build_ic_problem(sc), 0)
    del frames
    steps, warm = 40, 10
    # a 64-frame store in both loops: ~40 frames leave it, through each loop's archive
    env = dict(os.environ, COSLAM_EXPORT_DIR=str(tmp_path / "cxx"), COSLAM_EXPORT_FRAMES="512", COSLAM_HIST_STORE="64",
               HSA_KERNARG_POOL_SIZE=str(64 << 20))
    out = subprocess.run([exe, wl, str(steps), str(warm), "0", "2"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    m = re.search(r"exported frames 0\.\.(\d+) \((\d+) archived\)", out.stderr)
    n_frames = j["frames_run"]
    assert m and int(m.group(1)) == n_frames and int(m.group(2)) == n_frames + 1 - 64 > 0, out.stderr[-2000:]
    _, sc, video = _setup()
    loop = _loop(bench, sc, video, hist=64, hist_store=64, export_frames=512)
    for n in range(n_frames):
        loop.step(n + 1, n % bench.KEY_EVERY == 0)
    loop.export_results(tmp_path / "py")
    assert loop.pose_upd.archive_frames == n_frames + 1 - 64
    a, b = _read(tmp_path / "cxx", bench.N_CAMS), _read(tmp_path / "py", bench.N_CAMS)
    for f in FILES(bench.N_CAMS):
        assert a[f] == b[f], f
