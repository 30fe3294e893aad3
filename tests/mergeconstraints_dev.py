"""Device-side helpers of tests/test_mergeconstraints_gpu.py, tests/test_mergeconstraints_solve_gpu.py and tools/mergeconstraints_time.py: a scene
in the layout of tests/mergeconstraints_ref.py into a cs_track_history and device tables, and one call of cs_merge_constraints_assemble_dev."""
import numpy as np

from tests.mergeapply_golden_util import inv_k


class DeviceScene:
    """the scene's tables in device memory; .tables() names the tensors the assembly must leave as they are"""

    def __init__(self, S, dev, hist_len=16, store_len=None):
        import torch

        from coslam_amd.merge import _camera_groups_record
        from coslam_amd.poseupdate import TrackHistory

        nC, nF, N, frame0 = S["nC"], S["nF"], S["N"], S["frame0"]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.S, self.dev = S, dev
        store = nF if store_len is None else store_len
        self.th = TrackHistory(nC, N, hist_len, storeLen=max(store, hist_len))
        self.K = t(np.asarray(S["K"], np.float64))
        self.iK = t(np.stack([inv_k(k) for k in np.asarray(S["K"], np.float64)]))
        self.xy = t(np.asarray(S["histXY"], np.float64))
        self.state = t(np.asarray(S["state"], np.int32))
        self.slot2map = t(np.asarray(S["slot2map"], np.int32))
        self.featRef = t(np.asarray(S["featRef"], np.int32))
        self.M = t(np.asarray(S["M"], np.float64))
        self.groups = t(np.frombuffer(bytes(_camera_groups_record(S["groups"])), np.uint8).copy())
        span = t(np.full((nC, 2 * N), -1, np.int32))
        fl = torch.zeros(1, dtype=torch.uint8, device=dev)
        stat = torch.ones((nC, N), dtype=torch.uint8, device=dev)
        none = torch.full((nC, N), -1, dtype=torch.int32, device=dev)
        st_all = t((np.asarray(S["histXY"])[:, :, :N] != -1.0).astype(np.int32) - 1)
        eye = t(np.tile(np.eye(3).reshape(9), (nC, 1)))
        zero = torch.zeros((nC, 3), dtype=torch.float64, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        for i in range(nF):
            cams = [dict(K=self.K[c].data_ptr(), iK=self.iK[c].data_ptr(), xy=self.xy[c, i].data_ptr(), state=st_all[c, i].data_ptr(),
                         slot2map=none[c].data_ptr(), trackSpan=span[c].data_ptr(), isStatic=stat[c].data_ptr()) for c in range(nC)]
            self.th.detect_dynamic_dev(s, cams, eye.data_ptr(), zero.data_ptr(), 1, fl.data_ptr(), frame0 + i, minLen=1 << 30)
        held = min(nF, max(store, hist_len))
        cam_i = np.repeat(np.arange(nC), held).astype(np.int32)
        frm_i = np.tile(frame0 + nF - held + np.arange(held), nC).astype(np.int32)
        d = [t(cam_i), t(frm_i), t(np.asarray(S["histR"], np.float64)[:, nF - held:].reshape(-1, 9)),
             t(np.asarray(S["histT"], np.float64)[:, nF - held:].reshape(-1, 3))]
        self.th.set_poses_dev(s, len(cam_i), *[x.data_ptr() for x in d])
        torch.cuda.synchronize()
        self.pool = np.ascontiguousarray(S["segPool"], dtype=np.int32)
        self.n_seg = int(max([0] + [int((self.pool[c, :, 0] >= 0).sum()) for c in range(nC)]))
        if self.n_seg:
            self.th.load_segments(np.ascontiguousarray(self.pool[:, :self.n_seg]))
        self._keep = [span, fl, stat, none, st_all, eye, zero] + d
        self.cams = [dict(xy=self.xy[c, nF - 1].data_ptr(), state=self.state[c].data_ptr(), slot2map=self.slot2map[c].data_ptr(),
                          K=self.K[c].data_ptr()) for c in range(nC)]

    def tables(self):
        return dict(K=self.K, xy=self.xy, state=self.state, slot2map=self.slot2map, featRef=self.featRef, M=self.M, groups=self.groups)

    def snapshot(self):
        """copies of every input table (host), the history's poses of the whole store and its segments"""
        import torch

        out = {k: v.cpu().numpy().copy() for k, v in self.tables().items()}
        S = self.S
        nC, nF = S["nC"], S["nF"]
        R = torch.zeros((nC, nF, 9), dtype=torch.float64, device=self.dev)
        T = torch.zeros((nC, nF, 3), dtype=torch.float64, device=self.dev)
        self.th.get_span_dev(torch.cuda.current_stream().cuda_stream, S["frame0"], nF, R.data_ptr(), T.data_ptr())
        torch.cuda.synchronize()
        out["histR"], out["histT"] = R.cpu().numpy(), T.cpu().numpy()
        if self.n_seg:
            out["segs"] = self.th.segments()
        return out


def assemble_dev(D, f1, matches=None, max_matches=None, f2=None, gids=None):
    """one assembly over the device scene D -> (MergeConstraints, problem dict, views)"""
    from coslam_amd.merge import MergeConstraints

    S = D.S
    m = np.asarray(S["matches"] if matches is None else matches, np.int32).reshape(-1, 2)
    mc = MergeConstraints(S["nC"], S["N"], max(1, len(m)) if max_matches is None else max_matches, max(1, S["nMap"]))
    g1, g2, iC, jC = (S["gId1"], S["gId2"], S["maxiCam"], S["maxjCam"]) if gids is None else gids
    mc.assemble(D.th, D.cams, D.featRef.data_ptr(), S["nMap"], D.M.data_ptr(), D.groups.data_ptr(), g1, g2, iC, jC, f1,
                S["frame0"] + S["nF"] - 1 if f2 is None else f2, m)
    return mc, mc.problem(), mc.views()


def same_problem(P, A):
    """the device's problem P against the restatement's (or the golden's) A, bit for bit"""
    h = P["header"]
    assert (h.verdict, h.avgErr) == (A["verdict"], A["avgErr"]), (h.verdict, h.avgErr, A["verdict"], A["avgErr"])
    assert (h.nMergedTracks, h.skippedMatches) == (A["nMergedTracks"], A["skipped"])
    assert [h.camIds[i] for i in range(h.nCamIds)] == list(A["cam_ids"])
    if A["verdict"] != 1:
        assert (h.nPose, h.P, h.nObs, h.nUnmerged, h.nPrevViews, h.nMergeViews) == (0, 0, 0, 0, 0, 0)
        return
    assert (h.nPose, h.P, h.nObs, h.nUnmerged, h.nPrevViews) == (len(A["order"]), len(A["pointMap"]), len(A["obs_cam"]), A["nUnmerged"], A["nPrevViews"])
    for k in ("Ks", "Rs", "Ts", "pts", "obs_xy"):
        assert np.array_equal(P[k], np.array(A[k], np.float64).reshape(P[k].shape)), k
    for k in ("pointMap", "obs_ptr", "obs_cam"):
        assert np.array_equal(P[k], np.array(A[k], np.int32)), k
