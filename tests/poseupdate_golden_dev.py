"""The launch-and-compare loops of the map-point kernels against fixtures in the layout of tests/golden/update_points_golden.npz,
update_points_relink_golden.npz, classify_golden.npz and classify_relink_golden.npz: the ring builders and, per operation, one function
that takes the loaded fixture, launches every scene and compares bit for bit.  tests/test_poseupdate_gpu.py runs them over the 2-5
camera fixtures, tests/test_poseupdate_wide_gpu.py over the 7-13 camera ones and over the 14 / 16 camera scenes of
tests/poseupdate_wide_scenes.py (same layout, the oracle's answers as the expectation).  The fixtures' arrays are never written."""
import numpy as np
import pytest



def golden_ring(g, sc, dev, s):
    """the history of golden scene sc: the ring filled frame by frame with placeholder poses, then given the scene's poses (the way
    test_update_new_poses_points_reproduces_the_reference_on_its_golden_scenes builds it)"""
    import torch

    from coslam_amd.poseupdate import TrackHistory

    G = lambda k: g[f"s{sc}_{k}"]   # noqa: E731
    hR, hT, hXY, span = G("histR"), G("histT"), G("histXY"), G("trackSpan")
    nC, H = hR.shape[0], hR.shape[1]
    N = hXY.shape[2] // 2
    cur, nMap = int(G("curFrame")), G("M0").shape[0]
    th = TrackHistory(nC, N, H + 3)
    keep = dict(K=torch.from_numpy(G("K").copy()).to(dev), iK=torch.from_numpy(G("iK").copy()).to(dev), fl=torch.from_numpy(G("flags").copy()).to(dev),
                span=torch.from_numpy(span.copy()).to(dev), scratch=torch.ones((nC, N), dtype=torch.uint8, device=dev),
                s2m=torch.full((nC, N), -1, dtype=torch.int32, device=dev), misc=[])
    eye = torch.from_numpy(np.tile(np.eye(3).reshape(9), (nC, 1))).to(dev)
    zero = torch.zeros((nC, 3), dtype=torch.float64, device=dev)
    for j in range(H - 1, -1, -1):
        xy = torch.from_numpy(hXY[:, j].copy()).to(dev)
        st = torch.from_numpy(((span[:, :N] >= 0) & (span[:, :N] <= cur - j)).astype(np.int32) - 1).to(dev)
        keep["misc"] += [xy, st]
        cams = [dict(K=keep["K"][c].data_ptr(), iK=keep["iK"][c].data_ptr(), xy=xy[c].data_ptr(), state=st[c].data_ptr(),
                     slot2map=keep["s2m"][c].data_ptr(), trackSpan=keep["span"][c].data_ptr(), isStatic=keep["scratch"][c].data_ptr()) for c in range(nC)]
        th.detect_dynamic_dev(s, cams, eye.data_ptr(), zero.data_ptr(), nMap, keep["fl"].data_ptr(), cur - j, minLen=1 << 30)
    cam_i = np.repeat(np.arange(nC), H).astype(np.int32)
    frm_i = np.tile(cur - np.arange(H), nC).astype(np.int32)
    d = [torch.from_numpy(a).to(dev) for a in (cam_i, frm_i, hR.reshape(-1, 9).copy(), hT.reshape(-1, 3).copy())]
    th.set_poses_dev(s, len(cam_i), *[x.data_ptr() for x in d])
    keep["misc"] += d + [eye, zero]
    cams = [dict(K=keep["K"][c].data_ptr(), iK=keep["iK"][c].data_ptr(), trackSpan=keep["span"][c].data_ptr(), isStatic=keep["scratch"][c].data_ptr())
            for c in range(nC)]
    return th, cams, keep


def relink_ring(g, sc, dev, s):
    """the history of scene sc of tests/golden/update_points_relink_golden.npz: every segment's pixels on its own slot, the ring filled frame
    by frame (slots dead outside their segments), the scene's poses, the pool of linked segments loaded"""
    import torch

    from coslam_amd.poseupdate import TrackHistory

    G = lambda k: g[f"s{sc}_{k}"]   # noqa: E731
    hR, hT, hXY, ref, pool = G("histR"), G("histT"), np.nan_to_num(G("histXY"), nan=-1e9), G("featRef"), G("segPool")
    nC, H = hR.shape[0], hR.shape[1]
    N = hXY.shape[2] // 2
    cur, nMap = int(G("curFrame")), G("M0").shape[0]
    # first | last frame of every slot's segment (what trackSpan would have held while the segment's track was alive)
    span = np.full((nC, 2 * N), -1, np.int32)
    for c in range(nC):
        for sl, fr, fi, _ in ref[:, c]:
            if sl >= 0:
                span[c, sl], span[c, N + sl] = fi, fr
        for sl, la, fi, _ in pool[c]:
            if sl >= 0:
                span[c, sl], span[c, N + sl] = fi, la
    th = TrackHistory(nC, N, 64, storeLen=H + 3)   # walks of 64 nodes over a store deeper than the history
    keep = dict(K=torch.from_numpy(G("K").copy()).to(dev), iK=torch.from_numpy(G("iK").copy()).to(dev), fl=torch.from_numpy(G("flags").copy()).to(dev),
                span=torch.from_numpy(span).to(dev), fstat=torch.from_numpy(G("featStatic").copy()).to(dev),
                scratch=torch.ones((nC, N), dtype=torch.uint8, device=dev), s2m=torch.full((nC, N), -1, dtype=torch.int32, device=dev), misc=[])
    eye = torch.from_numpy(np.tile(np.eye(3).reshape(9), (nC, 1))).to(dev)
    zero = torch.zeros((nC, 3), dtype=torch.float64, device=dev)
    for j in range(H - 1, -1, -1):
        f = cur - j
        xy = torch.from_numpy(hXY[:, j].copy()).to(dev)
        st = torch.from_numpy(((span[:, :N] >= 0) & (span[:, :N] <= f) & (f <= span[:, N:])).astype(np.int32) - 1).to(dev)
        keep["misc"] += [xy, st]
        cams = [dict(K=keep["K"][c].data_ptr(), iK=keep["iK"][c].data_ptr(), xy=xy[c].data_ptr(), state=st[c].data_ptr(),
                     slot2map=keep["s2m"][c].data_ptr(), trackSpan=keep["span"][c].data_ptr(), isStatic=keep["scratch"][c].data_ptr()) for c in range(nC)]
        th.detect_dynamic_dev(s, cams, eye.data_ptr(), zero.data_ptr(), nMap, keep["fl"].data_ptr(), f, minLen=1 << 30)
    cam_i = np.repeat(np.arange(nC), H).astype(np.int32)
    frm_i = np.tile(cur - np.arange(H), nC).astype(np.int32)
    d = [torch.from_numpy(a).to(dev) for a in (cam_i, frm_i, hR.reshape(-1, 9).copy(), hT.reshape(-1, 3).copy())]
    th.set_poses_dev(s, len(cam_i), *[x.data_ptr() for x in d])
    torch.cuda.synchronize()
    th.load_segments(pool)
    keep["misc"] += d + [eye, zero]
    cams = [dict(K=keep["K"][c].data_ptr(), iK=keep["iK"][c].data_ptr(), trackSpan=keep["span"][c].data_ptr(), isStatic=keep["fstat"][c].data_ptr())
            for c in range(nC)]
    return th, cams, keep


def update_points_on(g):
    """cs_update_new_poses_points_dev and cs_refine_map_points_dev (k_update_points) on every scene of g: points, covariances and counts
    bit for bit.  The ring is filled frame by frame with placeholder poses and then given the scene's poses through
    cs_track_history_set_poses_dev, the way the adjusted poses arrive after a bundle adjustment.  Returns the points re-triangulated."""
    import torch

    from coslam_amd.poseupdate import TrackHistory

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    touched = 0
    for sc in range(int(g["n_scenes"])):
        G = lambda k: g[f"s{sc}_{k}"]   # noqa: E731
        hR, hT, hXY, span = G("histR"), G("histT"), G("histXY"), G("trackSpan")
        nC, H = hR.shape[0], hR.shape[1]
        N = hXY.shape[2] // 2
        cur, nMap = int(G("curFrame")), G("M0").shape[0]
        th = TrackHistory(nC, N, H + 3)   # (a ring deeper than the history: the unused entries are never walked)
        d_K = torch.from_numpy(G("K").copy()).to(dev)
        d_iK = torch.from_numpy(G("iK").copy()).to(dev)
        d_fl = torch.from_numpy(G("flags").copy()).to(dev)
        d_span = torch.from_numpy(span.copy()).to(dev)
        d_fstat = torch.from_numpy(G("featStatic").copy()).to(dev)
        d_scratch = torch.ones((nC, N), dtype=torch.uint8, device=dev)
        d_s2m = torch.full((nC, N), -1, dtype=torch.int32, device=dev)
        eye = torch.from_numpy(np.tile(np.eye(3).reshape(9), (nC, 1))).to(dev)
        zero = torch.zeros((nC, 3), dtype=torch.float64, device=dev)
        keep = []
        for j in range(H - 1, -1, -1):   # oldest first; entry j = frame cur - j
            xy = torch.from_numpy(hXY[:, j].copy()).to(dev)
            alive = ((span[:, :N] >= 0) & (span[:, :N] <= cur - j)).astype(np.int32) - 1   # 0 tracked / -1 dead at that frame
            st = torch.from_numpy(alive).to(dev)
            keep += [xy, st]
            cams = [dict(K=d_K[c].data_ptr(), iK=d_iK[c].data_ptr(), xy=xy[c].data_ptr(), state=st[c].data_ptr(),
                         slot2map=d_s2m[c].data_ptr(), trackSpan=d_span[c].data_ptr(), isStatic=d_scratch[c].data_ptr()) for c in range(nC)]
            th.detect_dynamic_dev(s, cams, eye.data_ptr(), zero.data_ptr(), nMap, d_fl.data_ptr(), cur - j, minLen=1 << 30)
        assert th.frames == H
        # the poses: every (camera, frame) of the history plus pairs the ring does not hold (skipped)
        cam_i = np.repeat(np.arange(nC), H).astype(np.int32)
        frm_i = np.tile(cur - np.arange(H), nC).astype(np.int32)
        cam_i = np.concatenate([cam_i, [0, 1, nC, -1]]).astype(np.int32)
        frm_i = np.concatenate([frm_i, [cur - H, cur + 1, cur, cur]]).astype(np.int32)
        Rq = np.concatenate([hR.reshape(-1, 9), np.full((4, 9), 777.0)])
        tq = np.concatenate([hT.reshape(-1, 3), np.full((4, 3), 777.0)])
        d_ci, d_fi = torch.from_numpy(cam_i).to(dev), torch.from_numpy(frm_i).to(dev)
        d_Rq, d_tq = torch.from_numpy(Rq).to(dev), torch.from_numpy(tq).to(dev)
        th.set_poses_dev(s, len(cam_i), d_ci.data_ptr(), d_fi.data_ptr(), d_Rq.data_ptr(), d_tq.data_ptr())
        d_M = torch.from_numpy(G("M0").copy()).to(dev)
        d_cov = torch.from_numpy(G("cov0").copy()).to(dev)
        d_pf = torch.from_numpy(G("pointFeat").copy()).to(dev)
        d_lf = torch.from_numpy(G("lastFrame").copy()).to(dev)
        d_ic = torch.from_numpy(G("isCurrent").copy()).to(dev)
        d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        cams = [dict(K=d_K[c].data_ptr(), iK=d_iK[c].data_ptr(), trackSpan=d_span[c].data_ptr(), isStatic=d_fstat[c].data_ptr())
                for c in range(nC)]
        th.update_new_poses_points_dev(s, cams, d_pf.data_ptr(), nMap, d_M.data_ptr(), d_cov.data_ptr(), d_fl.data_ptr(),
                                       float(G("sigma")), d_lastFrame=d_lf.data_ptr(), d_isCurrent=d_ic.data_ptr(),
                                       firstKeyFrame=int(G("firstKey")), d_counts=d_cnt.data_ptr())
        torch.cuda.synchronize()
        M, cov = d_M.cpu().numpy(), d_cov.cpu().numpy()
        n_ref = int((G("M_ref") != G("M0")).any(axis=1).sum())
        assert int(d_cnt.sum()) == n_ref, f"scene {sc}: {d_cnt.tolist()} points re-triangulated, the reference touched {n_ref}"
        dM, dC = np.abs(M - G("M_ref")).max(), np.abs(cov - G("cov_ref")).max()
        assert np.array_equal(M, G("M_ref")) and np.array_equal(cov, G("cov_ref")), f"scene {sc}: max |dM| {dM:.3e}, max |dcov| {dC:.3e}"
        touched += n_ref
        # CoSLAM::refineMapPoint on the same history: the reference's own function (src/app/SL_CoSLAM.cpp:666-713) was run on a copy
        # of every point two cameras see; the selected points bit for bit, the others untouched
        d_M2 = torch.from_numpy(G("M0").copy()).to(dev)
        d_cov2 = torch.from_numpy(G("cov0").copy()).to(dev)
        d_sel = torch.from_numpy(G("refine_select").copy()).to(dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        th.refine_map_points_dev(s, cams, d_pf.data_ptr(), nMap, d_M2.data_ptr(), d_cov2.data_ptr(), float(G("sigma")),
                                 d_select=d_sel.data_ptr(), d_count=d_n.data_ptr())
        torch.cuda.synchronize()
        assert int(d_n.item()) == int(G("refine_select").sum())
        M2, cov2 = d_M2.cpu().numpy(), d_cov2.cpu().numpy()
        assert np.array_equal(M2, G("M_refine")) and np.array_equal(cov2, G("cov_refine")), \
            f"scene {sc} refine: max |dM| {np.abs(M2 - G('M_refine')).max():.3e}"
        th.close()
    return touched


def classify_on(g, min_examined=50):
    """cs_map_points_classify_dev (k_classify_select, k_map_points_classify) on every scene of g: positions and covariances bit for bit,
    types, uncertain flags, bNewPt, staticFrameNum, the detached features (table and slot2map), the features' types; every scene must
    examine more than min_examined points.  Returns the points examined."""
    import torch

    from coslam_amd.poseupdate import TrackHistory

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    examined = 0
    for sc in range(int(g["n_scenes"])):
        G = lambda k: g[f"s{sc}_{k}"]   # noqa: E731
        hR, hT, hXY, span = G("histR"), G("histT"), G("histXY"), G("trackSpan")
        nC, H = hR.shape[0], hR.shape[1]
        N = hXY.shape[2] // 2
        cur, nMap = int(G("curFrame")), G("M0").shape[0]
        th = TrackHistory(nC, N, H)
        d_K = torch.from_numpy(G("K").copy()).to(dev)
        d_iK = torch.from_numpy(G("iK").copy()).to(dev)
        d_fl0 = torch.zeros(nMap, dtype=torch.uint8, device=dev)
        d_span = torch.from_numpy(span.copy()).to(dev)
        d_scratch = torch.ones((nC, N), dtype=torch.uint8, device=dev)
        d_none = torch.full((nC, N), -1, dtype=torch.int32, device=dev)
        keep = []
        for j in range(H - 1, -1, -1):   # oldest first; entry j = frame cur - j, with that frame's poses
            xy = torch.from_numpy(hXY[:, j].copy()).to(dev)
            st = torch.zeros((nC, N), dtype=torch.int32, device=dev)
            Rj, tj = torch.from_numpy(hR[:, j].copy()).to(dev), torch.from_numpy(hT[:, j].copy()).to(dev)
            keep += [xy, st, Rj, tj]
            cams = [dict(K=d_K[c].data_ptr(), iK=d_iK[c].data_ptr(), xy=xy[c].data_ptr(), state=st[c].data_ptr(),
                         slot2map=d_none[c].data_ptr(), trackSpan=d_span[c].data_ptr(), isStatic=d_scratch[c].data_ptr()) for c in range(nC)]
            th.detect_dynamic_dev(s, cams, Rj.data_ptr(), tj.data_ptr(), nMap, d_fl0.data_ptr(), cur - j, minLen=1 << 30)
        assert th.frames == H
        pf = G("pointFeat")
        s2m = np.where(pf.T >= 0, np.arange(N, dtype=np.int32)[None, :], -1).astype(np.int32)   # slot = point index in these scenes
        d_s2m = torch.from_numpy(np.ascontiguousarray(s2m)).to(dev)
        d_fstat = torch.from_numpy(G("featStatic").copy()).to(dev)
        d_M, d_cov = torch.from_numpy(G("M0").copy()).to(dev), torch.from_numpy(G("cov0").copy()).to(dev)
        d_fl, d_new = torch.from_numpy(G("flags").copy()).to(dev), torch.from_numpy(G("newPt").copy()).to(dev)
        d_sfn, d_first = torch.from_numpy(G("staticFrameNum").copy()).to(dev), torch.from_numpy(G("firstFrame").copy()).to(dev)
        d_pf = torch.from_numpy(pf.copy()).to(dev)
        d_ff, d_f1 = torch.from_numpy(G("featFrame").copy()).to(dev), torch.from_numpy(G("featFirst").copy()).to(dev)
        d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        cams = [dict(K=d_K[c].data_ptr(), iK=d_iK[c].data_ptr(), trackSpan=d_span[c].data_ptr(), isStatic=d_fstat[c].data_ptr(),
                     slot2map=d_s2m[c].data_ptr()) for c in range(nC)]
        th.map_points_classify_dev(s, cams, d_pf.data_ptr(), nMap, cur, d_M.data_ptr(), d_cov.data_ptr(), d_fl.data_ptr(), d_new.data_ptr(),
                                   d_sfn.data_ptr(), d_first.data_ptr(), float(G("pixelVar")), d_featFrame=d_ff.data_ptr(),
                                   d_featFirst=d_f1.data_ptr(), d_counts=d_cnt.data_ptr())
        torch.cuda.synchronize()
        M, cov, fl = d_M.cpu().numpy(), d_cov.cpu().numpy(), d_fl.cpu().numpy()
        assert np.array_equal(fl, G("flags_ref")), f"scene {sc}: types differ at {np.nonzero(fl != G('flags_ref'))[0][:8]}"
        assert np.array_equal(d_new.cpu().numpy(), G("newPt_ref")) and np.array_equal(d_sfn.cpu().numpy(), G("staticFrameNum_ref"))
        dM, dC = np.abs(M - G("M_ref")).max(), np.abs(cov - G("cov_ref")).max()
        assert np.array_equal(M, G("M_ref")) and np.array_equal(cov, G("cov_ref")), f"scene {sc}: max |dM| {dM:.3e}, max |dcov| {dC:.3e}"
        pf_out = d_pf.cpu().numpy()
        assert np.array_equal((pf_out >= 0).astype(np.uint8), G("hasFeature_ref"))
        assert np.array_equal(d_s2m.cpu().numpy() >= 0, pf_out.T >= 0)
        assert np.array_equal(d_fstat.cpu().numpy(), G("featStatic_ref"))
        cnt = d_cnt.tolist()
        assert cnt[1] == int((((fl & 2) != 0) & ((G("flags") & 2) == 0)).sum()) and cnt[0] > min_examined
        examined += cnt[0]
        with pytest.raises(Exception):   # the history's newest entry is not the frame that is asked for
            th.map_points_classify_dev(s, cams, d_pf.data_ptr(), nMap, cur + 1, d_M.data_ptr(), d_cov.data_ptr(), d_fl.data_ptr(),
                                       d_new.data_ptr(), d_sfn.data_ptr(), d_first.data_ptr())
        # nothing to examine (every point certain and static, or false): an empty worklist, not one byte of the map changes
        d_fl2 = torch.from_numpy(np.where(np.arange(nMap) % 5 == 0, 2, 0).astype(np.uint8)).to(dev)
        before = [x.clone() for x in (d_M, d_cov, d_new, d_sfn, d_pf, d_s2m, d_fstat)]
        th.map_points_classify_dev(s, cams, d_pf.data_ptr(), nMap, cur, d_M.data_ptr(), d_cov.data_ptr(), d_fl2.data_ptr(), d_new.data_ptr(),
                                   d_sfn.data_ptr(), d_first.data_ptr(), float(G("pixelVar")), d_featFrame=d_ff.data_ptr(),
                                   d_featFirst=d_f1.data_ptr(), d_counts=d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert d_cnt.tolist() == [0, 0] and all(torch.equal(a, b) for a, b in zip(before, (d_M, d_cov, d_new, d_sfn, d_pf, d_s2m, d_fstat)))
        assert np.array_equal(d_fl2.cpu().numpy(), np.where(np.arange(nMap) % 5 == 0, 2, 0))
        th.close()
    return examined


def classify_refs_on(g, min_examined=50, differs_without_refs=True):
    """cs_map_points_classify_dev behind cs_track_history_set_classify_refs on every scene of g, with the table at this frame and with
    the live references one frame behind; and without the references, where some points must come out differently (differs_without_refs:
    not in scenes whose features are all of this frame with nothing linked behind).  Returns (points examined, stale views detached)."""
    import torch

    from tests.test_oracle_cpu import classify_relink_expect, shifted_refs

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    examined = stale_detached = 0
    for sc in range(int(g["n_scenes"])):
        G = lambda k: g[f"s{sc}_{k}"]   # noqa: E731
        cur, nMap = int(G("curFrame")), G("M0").shape[0]
        for behind in (False, True):
            th, cams, keep = relink_ring(g, sc, dev, s)
            nC = len(cams)
            ref0 = shifted_refs(G)[0] if behind else G("featRef").copy()
            d_ref, d_rstat = torch.from_numpy(ref0.copy()).to(dev), torch.from_numpy(G("refStatic").copy()).to(dev)
            d_s2m = torch.from_numpy(G("slot2map").copy()).to(dev)
            for c in range(nC):
                cams[c]["slot2map"] = d_s2m[c].data_ptr()
            d_M, d_cov = torch.from_numpy(G("M0").copy()).to(dev), torch.from_numpy(G("cov0").copy()).to(dev)
            d_fl, d_new = torch.from_numpy(G("flags").copy()).to(dev), torch.from_numpy(G("newPt").copy()).to(dev)
            d_sfn, d_first = torch.from_numpy(G("staticFrameNum").copy()).to(dev), torch.from_numpy(G("firstFrame").copy()).to(dev)
            d_pf = torch.from_numpy(G("pointFeat").copy()).to(dev)
            d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
            th.set_classify_refs(d_ref.data_ptr(), d_rstat.data_ptr())
            th.map_points_classify_dev(s, cams, d_pf.data_ptr(), nMap, cur, d_M.data_ptr(), d_cov.data_ptr(), d_fl.data_ptr(), d_new.data_ptr(),
                                       d_sfn.data_ptr(), d_first.data_ptr(), float(G("pixelVar")), d_counts=d_cnt.data_ptr())
            torch.cuda.synchronize()
            M, cov, fl = d_M.cpu().numpy(), d_cov.cpu().numpy(), d_fl.cpu().numpy()
            assert np.array_equal(fl, G("flags_ref")), f"scene {sc} behind {behind}: types differ at {np.nonzero(fl != G('flags_ref'))[0][:8]}"
            assert np.array_equal(d_new.cpu().numpy(), G("newPt_ref")) and np.array_equal(d_sfn.cpu().numpy(), G("staticFrameNum_ref"))
            dM, dC = np.abs(M - G("M_ref")).max(), np.abs(cov - G("cov_ref")).max()
            assert np.array_equal(M, G("M_ref")) and np.array_equal(cov, G("cov_ref")), f"scene {sc}: max |dM| {dM:.3e}, max |dcov| {dC:.3e}"
            pf, ref = d_pf.cpu().numpy(), d_ref.cpu().numpy()
            has, dyn = classify_relink_expect(G, pf, ref, keep["fstat"].cpu().numpy(), d_rstat.cpu().numpy())
            assert np.array_equal(has, G("hasFeature_ref")) and np.array_equal(dyn, G("featDyn_ref") * has)
            gone = (ref0[:, :, 0] >= 0) & (ref[:, :, 0] < 0)
            assert np.array_equal(gone, (G("hasFeature_ref") == 0) & (ref0[:, :, 0] >= 0))
            assert np.array_equal(ref[~gone], ref0[~gone])                                   # every other reference stands as it was
            assert int((d_s2m.cpu().numpy() >= 0).sum()) == int((pf >= 0).sum())
            cnt = d_cnt.tolist()
            assert cnt[1] == int((((fl & 2) != 0) & ((G("flags") & 2) == 0)).sum()) and cnt[0] > min_examined
            if not behind:
                examined += cnt[0]
                stale_detached += int((gone & (G("pointFeat") < 0)).sum())
            # without the references the same call sees this frame's features only: some points come out differently
            if behind and differs_without_refs:
                th.set_classify_refs(None)
                d_M2, d_cov2, d_fl2 = torch.from_numpy(G("M0").copy()).to(dev), torch.from_numpy(G("cov0").copy()).to(dev), torch.from_numpy(G("flags").copy()).to(dev)
                d_new2, d_sfn2, d_pf2 = torch.from_numpy(G("newPt").copy()).to(dev), torch.from_numpy(G("staticFrameNum").copy()).to(dev), torch.from_numpy(G("pointFeat").copy()).to(dev)
                th.map_points_classify_dev(s, cams, d_pf2.data_ptr(), nMap, cur, d_M2.data_ptr(), d_cov2.data_ptr(), d_fl2.data_ptr(), d_new2.data_ptr(),
                                           d_sfn2.data_ptr(), d_first.data_ptr(), float(G("pixelVar")))
                torch.cuda.synchronize()
                assert not np.array_equal(d_fl2.cpu().numpy(), G("flags_ref")) or not np.array_equal(d_M2.cpu().numpy(), G("M_ref"))
            th.close()
    return examined, stale_detached


def relink_chains_on(g):
    """cs_update_new_poses_points_ref_dev / cs_refine_map_points_ref_dev / cs_feat_ref_advance_refine_dev / cs_check_unify_ref_dev on every
    scene of g (features as references over a segment pool).  Returns (points re-triangulated, pairs judged)."""
    import torch

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    n_upd = n_uni = 0
    for sc in range(int(g["n_scenes"])):
        G = lambda k: g[f"s{sc}_{k}"]   # noqa: E731
        th, cams, keep = relink_ring(g, sc, dev, s)
        ref = G("featRef")
        nMap, nC = ref.shape[0], ref.shape[1]
        d_ref = d(ref)
        d_M, d_cov = d(G("M0")), d(G("cov0"))
        d_lf, d_ic, d_cnt = d(G("lastFrame")), d(G("isCurrent")), torch.zeros(2, dtype=torch.int32, device=dev)
        th.update_new_poses_points_ref_dev(s, cams, d_ref.data_ptr(), nMap, d_M.data_ptr(), d_cov.data_ptr(), keep["fl"].data_ptr(), float(G("sigma")),
                                           d_lastFrame=d_lf.data_ptr(), d_isCurrent=d_ic.data_ptr(), firstKeyFrame=int(G("firstKey")),
                                           d_counts=d_cnt.data_ptr())
        torch.cuda.synchronize()
        M, cov = d_M.cpu().numpy(), d_cov.cpu().numpy()
        n_ref = int((G("M_ref") != G("M0")).any(axis=1).sum())
        assert int(d_cnt.sum()) == n_ref, (sc, d_cnt.tolist(), n_ref)
        assert np.array_equal(M, G("M_ref")) and np.array_equal(cov, G("cov_ref")), f"scene {sc}: max |dM| {np.abs(M - G('M_ref')).max():.3e}"
        n_upd += n_ref
        d_M2, d_cov2, d_sel, d_n = d(G("M0")), d(G("cov0")), d(G("refine_select")), torch.zeros(1, dtype=torch.int32, device=dev)
        th.refine_map_points_ref_dev(s, cams, d_ref.data_ptr(), nMap, d_M2.data_ptr(), d_cov2.data_ptr(), float(G("sigma")), d_select=d_sel.data_ptr(),
                                     d_count=d_n.data_ptr())
        torch.cuda.synchronize()
        assert int(d_n.item()) == int(G("refine_select").sum())
        assert np.array_equal(d_M2.cpu().numpy(), G("M_refine")) and np.array_equal(d_cov2.cpu().numpy(), G("cov_refine")), sc
        # ... and as ONE launch with the references' advance in front (cs_feat_ref_advance_refine_dev): on tables that are already at this
        # frame the advance changes nothing -- live heads are "tracked on", stale ones stay -- so the refined points are the reference's again;
        # the marks are consumed when asked
        cur = int(G("curFrame"))
        pf = np.where(ref[:, :, 1] == cur, ref[:, :, 0], -1).astype(np.int32)
        for clear in (False, True):
            d_M3, d_cov3, d_sel3, d_ref3, d_pf3 = d(G("M0")), d(G("cov0")), d(G("refine_select")), d(ref), d(pf)
            d_list = torch.arange(nMap, dtype=torch.int32, device=dev)
            d_fc = torch.zeros(5, dtype=torch.int32, device=dev)
            for c in range(nC):
                cams[c]["trackSpan"] = keep["span"][c].data_ptr()
            th.feat_ref_advance_refine_dev(s, cams, nMap, d_pf3.data_ptr(), cur, d_ref3.data_ptr(), 0, d_list.data_ptr(), nMap, True, d_sel3.data_ptr(), clear,
                                           d_M3.data_ptr(), d_cov3.data_ptr(), float(G("sigma")), d_counts=d_fc.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(d_M3.cpu().numpy(), G("M_refine")) and np.array_equal(d_cov3.cpu().numpy(), G("cov_refine")), (sc, clear)
            assert np.array_equal(d_ref3.cpu().numpy(), ref) and d_fc.tolist() == [0, 0, 0, 0, 0]
            assert int(d_sel3.sum().item()) == (0 if clear else int(G("refine_select").sum()))
        nP = len(G("unify_ok"))
        a = np.stack([np.where(G("unify_has1")[q][:, None] > 0, ref[G("unify_pts")[q][0]], -1) for q in range(nP)]).astype(np.int32)
        b = np.stack([np.where(G("unify_has2")[q][:, None] > 0, ref[G("unify_pts")[q][1]], -1) for q in range(nP)]).astype(np.int32)
        d_a, d_b, d_M1, d_M2u = d(a), d(b), d(G("unify_M1")), d(G("unify_M2"))
        d_ok = torch.zeros(nP, dtype=torch.uint8, device=dev)
        d_Mu, d_covu = torch.zeros((nP, 3), dtype=torch.float64, device=dev), torch.zeros((nP, 9), dtype=torch.float64, device=dev)
        th.check_unify_ref_dev(s, cams, nP, d_a.data_ptr(), d_b.data_ptr(), d_M1.data_ptr(), d_M2u.data_ptr(), float(G("sigma")), d_ok.data_ptr(),
                               d_Mu.data_ptr(), d_covu.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_ok.cpu().numpy().astype(bool), G("unify_ok").astype(bool)), sc
        assert np.array_equal(d_Mu.cpu().numpy(), G("unify_M")) and np.array_equal(d_covu.cpu().numpy(), G("unify_cov"), equal_nan=True), sc
        n_uni += nP
        th.close()
    return n_upd, n_uni


def check_unify_on(g):
    """cs_check_unify_dev (k_check_unify) on every scene's pairs: verdict, unified point and covariance bit for bit (NaN covariances of
    a rotation-only rig included).  Returns (pairs, pairs that unify)."""
    import torch

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    n_all = n_yes = 0
    for sc in range(int(g["n_scenes"])):
        G = lambda k: g[f"s{sc}_{k}"]   # noqa: E731
        nP = len(G("unify_ok"))
        if nP == 0:
            continue
        th, cams, keep = golden_ring(g, sc, dev, s)
        pf = G("pointFeat")
        a = np.stack([np.where(G("unify_has1")[q] > 0, pf[G("unify_pts")[q][0]], -1) for q in range(nP)]).astype(np.int32)
        b = np.stack([np.where(G("unify_has2")[q] > 0, pf[G("unify_pts")[q][1]], -1) for q in range(nP)]).astype(np.int32)
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
        d_a, d_b, d_M1, d_M2 = d(a), d(b), d(G("unify_M1")), d(G("unify_M2"))
        d_ok = torch.zeros(nP, dtype=torch.uint8, device=dev)
        d_M, d_cov = torch.zeros((nP, 3), dtype=torch.float64, device=dev), torch.zeros((nP, 9), dtype=torch.float64, device=dev)
        th.check_unify_dev(s, cams, nP, d_a.data_ptr(), d_b.data_ptr(), d_M1.data_ptr(), d_M2.data_ptr(), float(G("sigma")), d_ok.data_ptr(),
                           d_M.data_ptr(), d_cov.data_ptr())
        torch.cuda.synchronize()
        ok, M, cov = d_ok.cpu().numpy(), d_M.cpu().numpy(), d_cov.cpu().numpy()
        assert np.array_equal(ok.astype(bool), G("unify_ok").astype(bool)), (sc, np.nonzero(ok.astype(bool) != G("unify_ok").astype(bool))[0][:5])
        assert np.array_equal(M, G("unify_M")), sc
        assert np.array_equal(cov, G("unify_cov"), equal_nan=True), sc
        n_all += nP
        n_yes += int(ok.sum())
    return n_all, n_yes
