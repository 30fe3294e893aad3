"""The frame loop with its key frames where CoSLAM::genNewMapPoints' decision puts them (reference src/app/SL_CoSLAM.cpp:1294-1346: one
camera's mapped points decreased -> addKeyFrame for all cameras -> requestForBA) instead of bench.py's fixed cadence: LoopConfig.keyframe_drives.
The decision runs on the device (cs_keyframe_ready_dev, pinned against the reference's own functions: tests/test_register_decide_gpu.py), the
host reads `decrease` back, pushes the frame into the window's ring and requests the bundle adjustment; RobustBundleRTS::output() is applied
through cs_ba_output_apply_frames_dev with the window's key frames as a list, every one of them held against the record's header."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
def test_the_decision_places_the_key_frames_and_their_windows_are_applied(hip):
    import torch

    import bench
    from coslam_amd.frameloop import FrameLoop, LoopConfig

    dev = torch.device("cuda", 0)
    NA = bench.N_CAMS
    frames = bench.render_video(list(range(NA)), bench.N_FRAMES)
    video = {c: torch.from_numpy(frames[c]).to(dev) for c in range(NA)}
    sc = bench.build_scene()
    # m_mappedPtsReduceRatio raised from 0.93: in this synthetic world the mapped points of a camera never fall below 0.93 of a key frame's
    # (DESIGN.md 3.15); at 1.2, with the key-pose state re-based at frame 60, the decision fires in a burst and then at long intervals
    cfg = LoopConfig(n_cams=NA, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                     n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG, keyframe_drives=True,
                     keyframe_ratio=1.2)
    loop = FrameLoop(cfg, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0,
                     associate=bench.associate)
    loop.first_frame()
    BASE, T = 60, 300
    for i in range(1, BASE + 1):
        loop.step(i, True)           # (the caller's cadence is ignored: 60 calls saying "key frame" ...)
    loop.drain()
    early = loop.keyframe_stats()["key_frames_placed_by_the_decision"]
    assert loop.n_pushed == len(early) <= 2, early   # (... and the decision's one or two: the first tracked frame maps fewer features than initMap did)
    loop.enable_keyframe_decision(BASE, BASE & 1)   # the key-pose state as a key frame added at frame 60 would leave it
    for i in range(BASE + 1, T + 1):
        loop.step(i, False)
    loop.drain()
    st = loop.keyframe_stats()
    placed = st["key_frames_placed_by_the_decision"]
    n_kf = cfg.n_key_frames
    assert len(placed) > n_kf and len(set(np.diff(placed).tolist())) > 1, placed          # key frames, and not on a cadence
    assert st["frames_with_decrease_ie_key_frames_added"] == len(placed) == loop.n_pushed - len(early)  # the device's bookkeeping and the host's agree
    assert st["last_key_frame_per_camera"] == [placed[-1]] * NA                            # addKeyFrame: a key pose for ALL cameras
    every = early + placed
    assert loop.n_windows == len(every) - n_kf + 1
    lag_frames = loop.lag * cfg.key_every
    due = sum(1 for f in every[n_kf - 1:] if f + lag_frames <= T)
    assert loop.applied == due >= 4 and st["windows_not_applied_history_too_short"] == 0   # (the camera graphs reach back through the kept history)
    assert loop.out.wait_errors() == 0        # no wait gave up, and every applied record carried exactly the window's key frames
    assert loop.last_apply["first_key_frame"] in every
    R = loop.d_R[T & 1].cpu().numpy().reshape(NA, 3, 3)
    t = loop.d_t[T & 1].cpu().numpy()
    tt = np.stack([sc.pose(c, loop.vid(T))[1] for c in range(NA)])
    assert np.isfinite(R).all() and float(np.abs(t - tt).max()) < 0.1


@pytest.mark.timeout(300)
def test_the_fused_registration_launches_end_where_the_launch_per_step_sequence_does(hip):
    """LoopConfig.fused_registration (the second visits' lists built by the walks: cs_register_decide_kinds_rounds_dev /
    cs_register_revisit_decide_next_dev; advance + refine as one launch: cs_feat_ref_advance_refine_dev) against the launch-per-step
    sequence (cs_register_revisit_list_dev, cs_feat_ref_advance_list_dev, cs_refine_map_points_ref_dev): two Python loops on the same
    video, 110 frames with a bMerge frame among them and no key-frame solves (their write-back is thread-timed) -- the feature table, the
    slot tables, the map, the covariances, the flags, the feature references, their types and the second visits' counters are
    byte-identical after every tenth frame."""
    import torch

    import bench
    from coslam_amd.frameloop import FrameLoop, LoopConfig

    dev = torch.device("cuda", 0)
    NA = bench.N_CAMS
    frames = bench.render_video(list(range(NA)), bench.N_FRAMES)
    video = {c: torch.from_numpy(frames[c]).to(dev) for c in range(NA)}

    def make(fused):
        sc = bench.build_scene()
        cfg = LoopConfig(n_cams=NA, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                         n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG, fused_registration=fused)
        lp = FrameLoop(cfg, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0, associate=bench.associate)
        lp.first_frame()
        return lp

    def state(lp):
        # (a reference's `seg` is an index into the camera's pool, handed out by an atomic: which of two re-links of a frame gets which index
        # depends on the launch's shape -- the references are compared by slot / frame / first frame and by WHETHER something is linked behind,
        # the pools by their fill; what the chains hold is compared through the refined points and covariances)
        fref = lp.d_fref.cpu().numpy()
        return [t.cpu().numpy() for t in (lp.d_pf, lp.d_map, lp.d_cov, lp.d_mapflags, lp.d_rstat, lp.d_rv_counts, lp.d_fref_counts)] + \
               [np.stack([x.cpu().numpy() for x in lp.d_slot2map]), fref[:, :, :3], fref[:, :, 3] >= 0, lp.pose_upd.segment_counts()[0]]

    A, B = make(True), make(False)
    for i in range(1, 111):
        A.step(i, False), B.step(i, False)
        if i % 10 == 0:
            torch.cuda.synchronize()
            for k, (x, y) in enumerate(zip(state(A), state(B))):
                assert np.array_equal(x, y), f"frame {i}: array {k} differs in {int((x != y).sum())} entries"
    rv = A.d_rv_counts.cpu().tolist()
    assert rv[0] > 0 and rv[1] > 0 and A.n_merge_frames == B.n_merge_frames >= 2      # second visits attached features; frames 50 and 100 carried bMerge
    assert int(A.d_rvcounts[A.cfg.revisit_rounds].item()) == 0                         # no point beyond the lists


@pytest.mark.timeout(300)
def test_the_decision_places_the_key_frames_without_a_host_wait_per_frame(hip):
    """LoopConfig.keyframe_lag = 2 (the Python loop): the host never drains the device to learn `decrease` -- the word of
    frame i goes into pinned memory behind an event, and what the host acts on at frame i is the decision of frame i - 2, whose event has
    long fired; the key frame's own records and poses come out of a ring of three snapshots, its window is requested two frames late and
    applied at the frame it would have been.  Same world as the test above: the device's bookkeeping and the host's agree on every key
    frame but the ones still in the ring when the run ends, every window that is due is applied, no wait gives up, the rig stays put."""
    import torch

    import bench
    from coslam_amd.frameloop import FrameLoop, LoopConfig

    dev = torch.device("cuda", 0)
    NA = bench.N_CAMS
    frames = bench.render_video(list(range(NA)), bench.N_FRAMES)
    video = {c: torch.from_numpy(frames[c]).to(dev) for c in range(NA)}
    sc = bench.build_scene()
    D = 2
    cfg = LoopConfig(n_cams=NA, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                     n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG, keyframe_drives=True,
                     keyframe_ratio=1.2, keyframe_lag=D)
    loop = FrameLoop(cfg, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0,
                     associate=bench.associate)
    # a decision lag of a whole apply lag would key every window's apply in the past (bundle adjustment silently off): refused before any
    # GPU work
    late = LoopConfig(n_cams=NA, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                      n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG, keyframe_drives=True,
                      keyframe_ratio=1.2, keyframe_lag=loop.lag * cfg.key_every)
    with pytest.raises(ValueError, match="keyframe_lag"):
        FrameLoop(late, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0,
                  associate=bench.associate)
    loop.first_frame()
    BASE, T = 60, 300
    for i in range(1, BASE + 1):
        loop.step(i, True)
    loop.drain()
    early = list(loop.keyframe_stats()["key_frames_placed_by_the_decision"])
    loop.enable_keyframe_decision(BASE, BASE & 1)
    for i in range(BASE + 1, T + 1):
        loop.step(i, False)
    loop.drain()
    st = loop.keyframe_stats()
    placed = [f for f in st["key_frames_placed_by_the_decision"] if f not in early]
    n_kf = cfg.n_key_frames
    assert st["decision_lag_frames"] == D and len(placed) > n_kf and len(set(np.diff(placed).tolist())) > 1, placed
    said = st["frames_with_decrease_ie_key_frames_added"]        # the device's count (since the re-base) covers the last D frames too
    assert 0 <= said - len(placed) <= D and loop.n_pushed == len(early) + len(placed), (said, len(placed), loop.n_pushed)
    assert st["last_key_frame_per_camera"][0] >= placed[-1]
    every = early + placed
    assert loop.n_windows == len(every) - n_kf + 1
    lag_frames = loop.lag * cfg.key_every
    due = sum(1 for f in every[n_kf - 1:] if f + lag_frames <= T)
    assert loop.applied == due >= 4 and st["windows_not_applied_history_too_short"] == 0
    assert loop.out.wait_errors() == 0
    assert st["host_waits_that_blocked"] is not None   # (how often the host found the event of frame i - 2 still pending: it runs ahead of the device, so
    # it usually does and then waits for THAT frame -- the device keeps two frames queued; tools/r06_kflag.py times the modes against each other)
    R = loop.d_R[T & 1].cpu().numpy().reshape(NA, 3, 3)
    t = loop.d_t[T & 1].cpu().numpy()
    tt = np.stack([sc.pose(c, loop.vid(T))[1] for c in range(NA)])
    assert np.isfinite(R).all() and float(np.abs(t - tt).max()) < 0.1
    print("key frames placed", placed[:12], "... host waits that blocked:", st["host_waits_that_blocked"], "of", T - BASE)
