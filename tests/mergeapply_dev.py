"""Device-side helpers of tests/test_mergeapply_gpu.py (and tools/mergeapply_time.py): a scene in the layout of tests/mergeapply_ref.py
(frame-indexed histR / histT / histXY, featRef, segPool) into a cs_track_history, and one call of cs_recompute_map_points_keyfrms_dev."""
import numpy as np


def load_history(S, dev, hist_len=16, store_len=None, pool_rows=None):
    """-> (TrackHistory, cams, keep): every frame of S pushed in order (cs_detect_dynamic_dev pushes; its test is switched off by minLen), the
    scene's poses written over the pushed ones, the linked segments loaded.  The store holds the newest store_len frames (default: all)."""
    import torch

    from coslam_amd.poseupdate import TrackHistory

    nC, nF, N, frame0 = S["nC"], S["nF"], S["N"], S["frame0"]
    ref, pool = S["featRef"], S["segPool"] if pool_rows is None else pool_rows
    span = np.full((nC, 2 * N), -1, np.int32)
    for c in range(nC):
        for sl, fr, fi, _ in ref[:, c]:
            if 0 <= sl < N:
                span[c, sl], span[c, N + sl] = fi, fr
        for sl, la, fi, _ in pool[c]:
            if 0 <= sl < N:
                span[c, sl], span[c, N + sl] = fi, la
    store = nF if store_len is None else store_len
    th = TrackHistory(nC, N, hist_len, storeLen=max(store, hist_len))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    keep = dict(K=t(S["K"]), iK=t(S["iK"]), span=t(span), fl=torch.zeros(1, dtype=torch.uint8, device=dev),
                stat=torch.ones((nC, N), dtype=torch.uint8, device=dev), s2m=torch.full((nC, N), -1, dtype=torch.int32, device=dev), misc=[])
    eye = t(np.tile(np.eye(3).reshape(9), (nC, 1)))
    zero = torch.zeros((nC, 3), dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    xy_all = t(S["histXY"])
    st_all = t((S["histXY"][:, :, :N] > -1e8).astype(np.int32) - 1)
    keep["misc"] += [xy_all, st_all, eye, zero]
    for i in range(nF):
        cams = [dict(K=keep["K"][c].data_ptr(), iK=keep["iK"][c].data_ptr(), xy=xy_all[c, i].data_ptr(), state=st_all[c, i].data_ptr(),
                     slot2map=keep["s2m"][c].data_ptr(), trackSpan=keep["span"][c].data_ptr(), isStatic=keep["stat"][c].data_ptr())
                for c in range(nC)]
        th.detect_dynamic_dev(s, cams, eye.data_ptr(), zero.data_ptr(), 1, keep["fl"].data_ptr(), frame0 + i, minLen=1 << 30)
    held = min(nF, max(store, hist_len))
    cam_i = np.repeat(np.arange(nC), held).astype(np.int32)
    frm_i = np.tile(frame0 + nF - held + np.arange(held), nC).astype(np.int32)
    d = [t(cam_i), t(frm_i), t(S["histR"][:, nF - held:].reshape(-1, 9)), t(S["histT"][:, nF - held:].reshape(-1, 3))]
    th.set_poses_dev(s, len(cam_i), *[x.data_ptr() for x in d])
    torch.cuda.synchronize()
    if pool.shape[1] > 0:
        th.load_segments(np.ascontiguousarray(pool, dtype=np.int32))
    keep["misc"] += d
    cams = [dict(K=keep["K"][c].data_ptr(), iK=keep["iK"][c].data_ptr()) for c in range(nC)]
    return th, cams, keep


def recompute_dev(th, cams, S, dev, M0=None, cov0=None, update_cov=True, key_frames=None, map_count=None, f_start=None, f_end=None,
                  feat_ref=None, d_guard=None):
    """one launch over scene S -> (M, cov, counts [4]) as numpy"""
    import torch

    from coslam_amd.merge import recompute_map_points_keyfrms_dev

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ref = S["featRef"] if feat_ref is None else feat_ref
    keys = np.ascontiguousarray(S["key_frames"] if key_frames is None else key_frames, dtype=np.int32)
    d_ref, d_keys = t(ref.astype(np.int32)), t(keys if len(keys) else np.zeros(1, np.int32))
    d_M, d_cov = t((S["M0"] if M0 is None else M0).copy()), t((S["cov0"] if cov0 is None else cov0).copy())
    d_ff, d_lf, d_fl = t(S["firstFrame"].astype(np.int32)), t(S["lastFrame"].astype(np.int32)), t(S["flags"].astype(np.uint8))
    d_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    d_mc = None if map_count is None else torch.tensor([map_count], dtype=torch.int32, device=dev)
    recompute_map_points_keyfrms_dev(th, torch.cuda.current_stream().cuda_stream, cams, d_ref.data_ptr(), ref.shape[0],
                                     None if d_mc is None else d_mc.data_ptr(), d_ff.data_ptr(), d_lf.data_ptr(), d_fl.data_ptr(),
                                     S["f_start"] if f_start is None else f_start, S["f_end"] if f_end is None else f_end, d_keys.data_ptr(),
                                     len(keys), d_M.data_ptr(), d_cov.data_ptr(), S["sigma"], update_cov, d_cnt.data_ptr(), d_guard)
    torch.cuda.synchronize()
    return d_M.cpu().numpy(), d_cov.cpu().numpy(), d_cnt.cpu().numpy().tolist()


def recompute_ref(S, ref_mod, M0=None, cov0=None, update_cov=True, key_frames=None, map_count=None, f_start=None, f_end=None, feat_ref=None,
                  store_len=None, seg_cap=None, detail=None):
    """the restatement over the same scene (the store's newest store_len frames only) -> (M, cov, counts)"""
    nF = S["nF"]
    held = nF if store_len is None else min(nF, store_len)
    M, cov = (S["M0"] if M0 is None else M0).copy(), (S["cov0"] if cov0 is None else cov0).copy()
    cnt = ref_mod.recompute_map_points_keyfrms(S["K"], S["iK"], S["histR"][:, nF - held:], S["histT"][:, nF - held:], S["histXY"][:, nF - held:],
                                               S["frame0"] + nF - held, S["featRef"] if feat_ref is None else feat_ref, S["segPool"], map_count,
                                               S["firstFrame"], S["lastFrame"], S["flags"], S["f_start"] if f_start is None else f_start,
                                               S["f_end"] if f_end is None else f_end, S["key_frames"] if key_frames is None else key_frames,
                                               M, cov, S["sigma"], update_cov, seg_cap=seg_cap, detail=detail)
    return M, cov, cnt
