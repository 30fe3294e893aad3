"""ctypes mirror of cs_merge_check_dev (include/coslam_hip.h): MergeCameraGroup::checkPossibleMergable (reference
src/app/SL_MergeCameraGroup.cpp:56-177) on the device -- which camera pairs of two separated camera groups see the same part of the map
again and stand close enough, over a key frame's record of the groups; one launch, no wait."""
import ctypes as C

from ._lib import check, lib

MAX_CAMS = 16
MAX_INFO = 256


class MergeCam(C.Structure):
    _c_type_ = "cs_merge_cam"
    _fields_ = [("xy", C.c_void_p), ("state", C.c_void_p), ("slot2map", C.c_void_p), ("K", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p)]


class MergeInfo(C.Structure):
    """MergeInfo::set(frame1, cam1, gid1, frame2, cam2, gid2)."""

    _c_type_ = "cs_merge_info"
    _fields_ = [(n, C.c_int) for n in ("frame1", "cam1", "gid1", "frame2", "cam2", "gid2")]

    def as_tuple(self):
        return tuple(int(getattr(self, n)) for n, _ in self._fields_)


class MergeCandidates(C.Structure):
    _c_type_ = "cs_merge_candidates"
    _fields_ = [("frame", C.c_int), ("groupNum", C.c_int), ("nMergeInfo", C.c_int), ("reserved", C.c_int), ("info", MergeInfo * MAX_INFO),
                ("nFeat", C.c_int * MAX_CAMS), ("nInCam", (C.c_int * MAX_CAMS) * MAX_CAMS), ("inNum", (C.c_int * MAX_CAMS) * MAX_CAMS),
                ("fromTo", (C.c_ubyte * MAX_CAMS) * MAX_CAMS), ("camDist", (C.c_double * MAX_CAMS) * MAX_CAMS)]

    @classmethod
    def from_bytes(cls, buf):
        return cls.from_buffer_copy(bytes(buf))

    def infos(self):
        """[(frame1, cam1, gid1, frame2, cam2, gid2), ...] in the reference's loop order"""
        return [self.info[k].as_tuple() for k in range(self.nMergeInfo)]

    def tables(self, nCams):
        """dict of nested lists cut to the rig: nFeat [nCams], nInCam / inNum / fromTo / camDist [nCams][nCams]"""
        r = range(nCams)
        return dict(nFeat=[int(self.nFeat[c]) for c in r], nInCam=[[int(self.nInCam[i][j]) for j in r] for i in r],
                    inNum=[[int(self.inNum[i][j]) for j in r] for i in r], fromTo=[[int(self.fromTo[i][j]) for j in r] for i in r],
                    camDist=[[float(self.camDist[i][j]) for j in r] for i in r])


def merge_cams(cams):
    """list of dicts of DEVICE pointers (ints) with the field names of cs_merge_cam -> the ctypes array (build once)"""
    if isinstance(cams, C.Array):
        return cams
    arr = (MergeCam * len(cams))()
    for a, c in zip(arr, cams):
        for n, _ in MergeCam._fields_:
            v = c.get(n)
            setattr(a, n, int(v) if v else None)
    return arr


def merge_check_scratch_bytes(nCams, N):
    """bytes of device scratch: zero it once before the first call, every call leaves it zeroed"""
    return lib().cs_merge_check_scratch_bytes(int(nCams), int(N))


def merge_check_dev(stream_ptr, cams, N, nMap, d_mapCount, d_mapPts, d_mapFlags, W, H, d_groups, frame, d_out, d_scratch, minInNum=10,
                    minInAreaRatio=0.5, maxCamDist=6.0, allPairs=False, device=0):
    """cs_merge_check_dev: checkPossibleMergable(minInNum, minInAreaRatio, maxCamDist) over the record d_groups (a CameraGroups in device
    memory) into d_out (a MergeCandidates in device memory).  cams: a merge_cams() array or a list of dicts.  The defaults are the
    reference's call (10, 0.5, Param::maxDistRatio = 6.0 taken as a distance)."""
    arr = merge_cams(cams)
    check(lib().cs_merge_check_dev(int(device), stream_ptr, len(arr), arr if len(arr) else None, int(N), int(nMap), d_mapCount, d_mapPts, d_mapFlags,
                                   int(W), int(H), d_groups, int(frame), int(minInNum), minInAreaRatio, maxCamDist, 1 if allPairs else 0, d_out,
                                   d_scratch),
          "cs_merge_check_dev")


def merge_keygraph_plan(frames, groups, cam_ids, first_constrain, camid1, camid2, infos, n_max_keyfrm=100):
    """cs_merge_keygraph_plan (host code): MergeCameraGroup::searchFirstKeyFrameForMerge + the topology of _constructGraphForKeyFrms.
    frames: the key frames' frame numbers, oldest first, the current key frame last; groups: per key frame a CameraGroups record or a list of
    camera-id lists; cam_ids ascending; first_constrain: index of the first-constrained key frame; infos: [(frame1, cam1, frame2, cam2)] of the
    valid merge infos.  Returns dict(fixed_kf, node_kf, node_cam, fixed, id1, id2, scale_id, n_constraint); raises CoslamHipError where the
    reference would assert (no key frame to hold fixed)."""
    import numpy as np

    from .grouping import CameraGroups

    nk = len(frames)
    recs = (CameraGroups * max(nk, 1))()
    for k, g in enumerate(groups):
        if isinstance(g, CameraGroups):
            recs[k] = g
            continue
        C.memset(C.byref(recs[k]), 0xFF, C.sizeof(CameraGroups))     # unused entries -1
        recs[k].groupNum = len(g)
        for i in range(MAX_CAMS):
            recs[k].num[i] = len(g[i]) if i < len(g) else 0
        for i, cams in enumerate(g):
            for j, c in enumerate(cams):
                recs[k].camIds[i][j] = int(c)
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    ids = np.ascontiguousarray(cam_ids, dtype=np.int32)
    inf = np.ascontiguousarray(np.asarray(infos, dtype=np.int32).reshape(-1, 4))
    n_cap = max(nk * len(ids), 1)
    e_cap = 2 * n_cap + len(inf) + 1
    node_kf, node_cam, fixed = np.zeros(n_cap, np.int32), np.zeros(n_cap, np.int32), np.zeros(n_cap, np.uint8)
    id1, id2, sid = np.zeros(e_cap, np.int32), np.zeros(e_cap, np.int32), np.zeros(e_cap, np.int32)
    fx, nn, ne, nc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    p = lambda v: v.ctypes.data  # noqa: E731
    check(lib().cs_merge_keygraph_plan(nk, p(fr), recs, len(ids), p(ids), int(first_constrain), int(camid1), int(camid2), len(inf), p(inf),
                                       int(n_max_keyfrm), C.byref(fx), n_cap, C.byref(nn), p(node_kf), p(node_cam), p(fixed), e_cap, C.byref(ne),
                                       p(id1), p(id2), p(sid), C.byref(nc)), "cs_merge_keygraph_plan")
    n, e = nn.value, ne.value
    return dict(fixed_kf=fx.value, node_kf=node_kf[:n].copy(), node_cam=node_cam[:n].copy(), fixed=fixed[:n].copy(), id1=id1[:e].copy(),
                id2=id2[:e].copy(), scale_id=sid[:e].copy(), n_constraint=nc.value)


class MergePoseCorrection:
    """The pose correction of a camera-group merge on the device (MergeCameraGroup::recomputeKeyCamPoses + recomputeAllCameraPoses,
    src/app/SL_MergeCameraGroup.cpp:1083-1116): relax the key-frame graph with its shared-scale constraint edges, write the corrected key
    poses into the fixed nodes of the per-camera chains, relax the chains -- four launches on one stream, no wait between them.
    key_graph: (fixed, id1, id2, scale_id) as merge_keygraph_plan gives them; chain_graphs: [(fixed, id1, id2)] per camera
    (_constructGraphForAllFrms); key_node[i]: the flat chain node that key-graph node i is (or < 0)."""

    def __init__(self, key_graph, chain_graphs, key_node, device=0):
        import numpy as np
        import torch

        from .posegraph import PoseGraphs

        fixed, id1, id2, sid = key_graph
        self.device = int(device)
        self.key = PoseGraphs([(fixed, id1, id2)], device=device, scale_ids=[sid])
        self.chains = PoseGraphs(chain_graphs, device=device)
        self.scaled_rows = np.nonzero(np.asarray(sid) >= 0)[0]
        dev = torch.device("cuda", self.device)
        self._torch = torch
        self.d_key_node = torch.as_tensor(np.ascontiguousarray(key_node, dtype=np.int32), device=dev)
        assert len(self.d_key_node) == self.key.n_nodes
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)  # noqa: E731
        nk, ek, nc, ec = self.key.n_nodes, self.key.n_edges, self.chains.n_nodes, self.chains.n_edges
        self.kR, self.kT, self.keR, self.keT, self.knR, self.knT, self.keS = z(nk, 9), z(nk, 3), z(ek, 9), z(ek, 3), z(nk, 9), z(nk, 3), z(ek)
        self.cR, self.cT, self.ceR, self.ceT, self.cnR, self.cnT = z(nc, 9), z(nc, 3), z(max(ec, 1), 9), z(max(ec, 1), 3), z(nc, 9), z(nc, 3)

    def run(self, keyR, keyT, constraintR, constraintT, chainR, chainT):
        """current poses of the key-graph nodes and of all chain nodes, MergeInfo::R / t of the constraint edges (in edge order) ->
        dict(keyR, keyT, edgeS, chainR, chainT) (numpy).  Every plain edge's transform is taken from the current poses on the device."""
        from .posegraph import posegraph_set_poses_dev

        torch = self._torch
        up = lambda d, h: d.copy_(torch.as_tensor(h, dtype=torch.float64).reshape(d.shape))  # noqa: E731
        up(self.kR, keyR), up(self.kT, keyT), up(self.cR, chainR), up(self.cT, chainT)
        rows = torch.as_tensor(self.scaled_rows, device=self.keR.device)
        self.keR[rows] = torch.as_tensor(constraintR, dtype=torch.float64).reshape(-1, 9).to(self.keR.device)
        self.keT[rows] = torch.as_tensor(constraintT, dtype=torch.float64).reshape(-1, 3).to(self.keT.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        P = lambda t: t.data_ptr()  # noqa: E731
        self.key.edges_dev(s, P(self.kR), P(self.kT), P(self.keR), P(self.keT))          # constraint rows stay as written
        self.chains.edges_dev(s, P(self.cR), P(self.cT), P(self.ceR), P(self.ceT))       # from the poses BEFORE the correction
        self.key.relax_scaled_dev(s, P(self.kR), P(self.kT), P(self.keR), P(self.keT), P(self.knR), P(self.knT), P(self.keS))
        posegraph_set_poses_dev(s, self.key.n_nodes, P(self.d_key_node), P(self.knR), P(self.knT), P(self.cR), P(self.cT), device=self.device)
        self.chains.relax_dev(s, P(self.cR), P(self.cT), P(self.ceR), P(self.ceT), P(self.cnR), P(self.cnT))
        self.key.status(s)
        self.chains.status(s)
        n = lambda t: t.cpu().numpy()  # noqa: E731
        return dict(keyR=n(self.knR), keyT=n(self.knT), edgeS=n(self.keS), chainR=n(self.cnR), chainT=n(self.cnT))

    def close(self):
        self.key.close()
        self.chains.close()


def _camera_groups_record(groups, group_id=None):
    """a list of camera-id lists (or a CameraGroups) -> a CameraGroups record, unused entries -1 / 0"""
    from .grouping import CameraGroups

    if isinstance(groups, CameraGroups):
        return CameraGroups.from_buffer_copy(bytes(groups))
    rec = CameraGroups()
    C.memset(C.byref(rec), 0xFF, C.sizeof(CameraGroups))
    rec.groupNum = len(groups)
    for g in range(MAX_CAMS):
        rec.num[g] = len(groups[g]) if g < len(groups) else 0
    for g, cams in enumerate(groups):
        for i, c in enumerate(cams):
            rec.camIds[g][i] = int(c)
            rec.groupId[int(c)] = g
    if group_id is not None:
        for c, g in enumerate(group_id):
            rec.groupId[c] = int(g)
    return rec


def merge_matched_groups(groups, gid1, gid2, camid1, camid2):
    """cs_merge_matched_groups (host code): MergeCameraGroup::mergeMatchedGroups + the m_groupId loop of CoSLAM::mergeCamGroups.  groups: a
    CameraGroups record or a list of camera-id lists; gid1 / gid2: the group ids of the valid merge infos.  Returns dict(record, groups,
    group_id [16], merged_gid); raises CoslamHipError where the reference asserts (neither camera in a group)."""
    import numpy as np

    rec = _camera_groups_record(groups)
    a, b = np.ascontiguousarray(gid1, dtype=np.int32).reshape(-1), np.ascontiguousarray(gid2, dtype=np.int32).reshape(-1)
    assert len(a) == len(b)
    gid, mg = np.zeros(MAX_CAMS, np.int32), C.c_int(-1)
    p = lambda v: v.ctypes.data if len(v) else None  # noqa: E731
    check(lib().cs_merge_matched_groups(C.byref(rec), len(a), p(a), p(b), int(camid1), int(camid2), gid.ctypes.data, C.byref(mg)),
          "cs_merge_matched_groups")
    return dict(record=rec, groups=rec.groups(), group_id=gid, merged_gid=mg.value)


def recompute_map_points_keyfrms_dev(history, stream_ptr, cams, d_featRef, nMap, d_mapCount, d_firstFrame, d_lastFrame, d_mapFlags, f_start,
                                     f_end, d_keyFrames, nKey, d_mapPts, d_mapCov, pixelErrVar, updateCov=True, d_counts=None, d_guard=None):
    """cs_recompute_map_points_keyfrms_dev: CoSLAM::getMapPts(f_start, f_end) + MergeCameraGroup::recomputeMapPoints -- every certain-static
    map point of the span triangulated again from its key-frame views (updateStaticPointPositionAtKeyFrms) over the history's poses, in
    place, one launch.  history: a TrackHistory; cams: K, iK per camera; d_keyFrames: ascending int32 frame numbers in device memory."""
    from .poseupdate import poseupdate_cams

    check(lib().cs_recompute_map_points_keyfrms_dev(history._h, stream_ptr, poseupdate_cams(cams), d_featRef, int(nMap), d_mapCount, d_firstFrame,
                                                    d_lastFrame, d_mapFlags, int(f_start), int(f_end), d_keyFrames, int(nKey), d_mapPts, d_mapCov,
                                                    pixelErrVar, 1 if updateCov else 0, d_counts, d_guard), "cs_recompute_map_points_keyfrms_dev")


def _stream(device, stream_ptr):
    """the stream a call goes to: the caller's, or torch's current stream of the device"""
    import torch

    return torch.cuda.current_stream(device).cuda_stream if stream_ptr is None else stream_ptr


class _MergeHandle:
    """What the handle classes below share: the library `_L`, the handle `_m` of the C type `_prefix`, its device."""

    _prefix = None    # "cs_merge_front", ...: <prefix>_create / _destroy / _buffers_get / _download
    _Buffers = None   # the ctypes mirror of <prefix>_buffers where the handle exports its buffers (-> self.buf)
    _m = None

    def _create(self, device, *args):
        self._L, self.device = lib(), int(device)
        self._m = getattr(self._L, self._prefix + "_create")(self.device, *args)
        if not self._m:
            check(-1, self._prefix + "_create")
        if self._Buffers is not None:
            self.buf = self._Buffers()
            check(getattr(self._L, self._prefix + "_buffers_get")(self._m, C.byref(self.buf)), self._prefix + "_buffers_get")

    def _stream(self, stream_ptr):
        return _stream(self.device, stream_ptr)

    def _down(self, ptr, n, dtype, stream_ptr=None):
        import numpy as np

        out = np.zeros(n, dtype)
        if out.nbytes:
            check(getattr(self._L, self._prefix + "_download")(self._m, self._stream(stream_ptr), ptr, out.ctypes.data, out.nbytes),
                  self._prefix + "_download")
        return out

    def close(self):
        if self._m:
            getattr(self._L, self._prefix + "_destroy")(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MergeApply(_MergeHandle):
    """cs_merge_apply: a merge's pose correction fed from and written to a TrackHistory, and the map behind it -- from "valid MergeInfo {R, t}
    exist" to "history and map are the merged ones" on one stream, no host wait.  plan: merge_keygraph_plan's dict (node_kf counted over ALL
    key frames given to the plan); key_frames: the frame numbers of those key frames, oldest first, the current key frame last; n_cams: the
    history's cameras (every one gets its chain, also those outside the plan).  MergePoseCorrection is the host-fed form of the same solve."""

    _prefix = "cs_merge_apply"

    def __init__(self, plan, key_frames, n_cams, device=0):
        import numpy as np
        import torch

        self.n_cams = int(n_cams)
        fx = int(plan["fixed_kf"]) if "fixed_kf" in plan else int(np.min(plan["node_kf"]))
        self.key_frames = np.ascontiguousarray(np.asarray(key_frames, dtype=np.int32)[fx:])
        node_kf = np.ascontiguousarray(np.asarray(plan["node_kf"], dtype=np.int32) - fx)
        node_cam = np.ascontiguousarray(plan["node_cam"], dtype=np.int32)
        fixed = np.ascontiguousarray(plan["fixed"], dtype=np.uint8)
        id1, id2 = np.ascontiguousarray(plan["id1"], dtype=np.int32), np.ascontiguousarray(plan["id2"], dtype=np.int32)
        sid = np.ascontiguousarray(plan["scale_id"], dtype=np.int32)
        self.n_edges, self.n_constraint = len(id1), int((sid >= 0).sum())
        p = lambda v: v.ctypes.data  # noqa: E731
        self._create(device, self.n_cams, len(self.key_frames), p(self.key_frames), len(node_kf), p(node_kf), p(node_cam), p(fixed), len(id1), p(id1),
                     p(id2), p(sid))
        dev = torch.device("cuda", self.device)
        self._torch = torch
        self.d_edgeS = torch.zeros(max(self.n_edges, 1), dtype=torch.float64, device=dev)
        self.d_key_frames = torch.as_tensor(self.key_frames, device=dev)
        self._keep = None

    @property
    def guard_ptr(self):
        """device pointer of the guard word (1 when the last run's solves failed)"""
        return int(self._L.cs_merge_apply_guard(self._m) or 0)

    def run(self, history, info_R, info_T, stream_ptr=None):
        """cs_merge_apply_run_dev: info_R [nConstraint][9] / info_T [nConstraint][3] = MergeInfo::R / t of the constraint edges in edge order
        (torch device tensors, or host arrays that are uploaded first).  Enqueues only; the solved scales land in self.d_edgeS."""
        torch = self._torch
        dev = self.d_edgeS.device
        dR = torch.as_tensor(info_R, dtype=torch.float64).reshape(-1, 9).to(dev).contiguous()
        dT = torch.as_tensor(info_T, dtype=torch.float64).reshape(-1, 3).to(dev).contiguous()
        assert dR.shape[0] == self.n_constraint and dT.shape[0] == self.n_constraint
        self._keep = (dR, dT)
        check(self._L.cs_merge_apply_run_dev(self._m, history._h, self._stream(stream_ptr), dR.data_ptr(), dT.data_ptr(), self.d_edgeS.data_ptr()),
              "cs_merge_apply_run_dev")

    def run_dev(self, history, d_infoR, d_infoT, stream_ptr=None):
        """cs_merge_apply_run_dev with MergeInfo::R / t given as DEVICE POINTERS ([nConstraint][9] / [3] doubles in edge order), e.g.
        MergeConstraints.buf.infoR / infoT as cs_merge_info_dev left them.  Enqueues only."""
        check(self._L.cs_merge_apply_run_dev(self._m, history._h, self._stream(stream_ptr), d_infoR, d_infoT, self.d_edgeS.data_ptr()),
              "cs_merge_apply_run_dev")

    def recompute(self, history, cams, d_featRef, nMap, d_mapCount, d_firstFrame, d_lastFrame, d_mapFlags, d_mapPts, d_mapCov, f_start,
                  pixelErrVar, updateCov=True, d_counts=None, stream_ptr=None):
        """MergeCameraGroup::recomputeMapPoints behind run(), guarded by its solves: f_end = the current key frame; the caller forms
        f_start = max(fixed frame, last release frame) as CoSLAM::mergeCamGroups does (reference src/app/SL_CoSLAM.cpp:1430-1434)."""
        recompute_map_points_keyfrms_dev(history, self._stream(stream_ptr), cams, d_featRef, nMap, d_mapCount, d_firstFrame, d_lastFrame, d_mapFlags, f_start,
                                         int(self.key_frames[-1]), self.d_key_frames.data_ptr(), len(self.key_frames), d_mapPts, d_mapCov,
                                         pixelErrVar, updateCov, d_counts, self.guard_ptr)

    def status(self, stream_ptr=None):
        """cs_merge_apply_status: waits; raises CoslamHipError (CS_ERR_NUMERIC) naming the failed graph"""
        check(self._L.cs_merge_apply_status(self._m, self._stream(stream_ptr)), "cs_merge_apply_status")


def merge_first_constrain(frames, self_motion, cam_ids):
    """cs_merge_first_constrain (host code): MergeCameraGroup::buildIdMapForSelfKeyPoses(camIds, 2).  frames: the key frames' numbers, oldest
    first, the current key frame last; self_motion [nKey][nCams]: KeyPose::bSelfMotion; cam_ids ascending.  Returns (index of the
    first-constrained key frame -- merge_keygraph_plan's first_constrain --, [(frame, cam)] in the pose order of the merge's bundle
    adjustment); raises CoslamHipError where no camera has a self-motion key frame behind the current one."""
    import numpy as np

    fr = np.ascontiguousarray(frames, dtype=np.int32)
    sm = np.ascontiguousarray(np.asarray(self_motion) != 0, dtype=np.uint8).reshape(len(fr), -1)
    ids = np.ascontiguousarray(cam_ids, dtype=np.int32)
    of, oc = np.zeros(2 * max(len(ids), 1), np.int32), np.zeros(2 * max(len(ids), 1), np.int32)
    fc = C.c_int(-1)
    p = lambda v: v.ctypes.data  # noqa: E731
    check(lib().cs_merge_first_constrain(len(fr), p(fr), p(sm), sm.shape[1], len(ids), p(ids), C.byref(fc), p(of), p(oc)), "cs_merge_first_constrain")
    return fc.value, [(int(f), int(c)) for f, c in zip(of[:2 * len(ids)], oc[:2 * len(ids)])]


MERGE_OK, MERGE_REJECT, MERGE_FEW, MERGE_BAD_GROUPS = 1, 0, -1, -2
MERGE_VIEW_FROM_M2, MERGE_VIEW_DETACHED, MERGE_VIEW_PREV, MERGE_VIEW_PREV_DETACHED = 1, 2, 4, 8


class MergeConstraintsHeader(C.Structure):
    _c_type_ = "cs_merge_constraints_header"
    _fields_ = [(n, C.c_int) for n in ("verdict", "nPose", "P", "nObs", "nMergedTracks", "nUnmerged", "nPrevViews", "skippedMatches", "nMergeViews",
                                       "f1", "f2", "nCamIds")] + [("camIds", C.c_int * MAX_CAMS), ("nInfo", C.c_int), ("reserved", C.c_int),
                                                                  ("avgErr", C.c_double)]


class MergeConstraintsBuffers(C.Structure):
    _c_type_ = "cs_merge_constraints_buffers"
    _fields_ = [(n, C.c_void_p) for n in ("header", "views", "Ks", "Rs", "Ts", "pts", "pointMap", "obsPtr", "obsCam", "obsXY", "info", "infoValid",
                                          "infoR", "infoT")] + [(n, C.c_int) for n in ("maxPoints", "maxObs", "maxViews", "maxInfo")] + \
               [(n, C.c_void_p) for n in ("solvedRs", "solvedTs", "solvedPts", "outlier")]


class MergeConstraints(_MergeHandle):
    """cs_merge_constraints: MergeCameraGroup::genMergeInfoVer2 on the device, from the matched features of two cameras to the merge's
    bundle-adjustment problem (assemble) and from a set of poses to the MergeInfo {R, t} list (info).  The buffers stay in device memory
    (d_info_R / d_info_T are what MergeApply.run takes); problem() / views() / infos() download them for a host-side caller."""

    _prefix, _Buffers = "cs_merge_constraints", MergeConstraintsBuffers

    def __init__(self, n_cams, N, max_matches, max_map, device=0):
        self.n_cams, self.N = int(n_cams), int(N)
        self._create(device, self.n_cams, self.N, int(max_matches), int(max_map))
        self._keep = None

    def assemble(self, history, cams, d_featRef, nMap, d_mapPts, d_groups, gId1, gId2, maxiCam, maxjCam, f1, f2, matches, stream_ptr=None):
        """cs_merge_constraints_assemble_dev.  cams: a merge_cams() array or a list of dicts of device pointers (xy, state, slot2map, K of the
        current key frame); matches: an int32 [K][2] slot-pair table.  A torch DEVICE tensor is taken as it is and must be ready on the
        stream the launch goes to (nothing is copied, the call only enqueues); a host array goes through cs_merge_constraints_assemble,
        which copies it into the handle's own table on that same stream in front of the launch."""
        import numpy as np
        import torch

        arr = merge_cams(cams)
        head = (self._m, history._h, self._stream(stream_ptr), arr, d_featRef, int(nMap), d_mapPts, d_groups, int(gId1), int(gId2), int(maxiCam),
                int(maxjCam), int(f1), int(f2))
        if isinstance(matches, torch.Tensor) and matches.is_cuda:
            dm = matches.to(torch.int32).reshape(-1, 2).contiguous()
            self._keep = dm
            check(self._L.cs_merge_constraints_assemble_dev(*head, dm.data_ptr() if dm.shape[0] else None, int(dm.shape[0])),
                  "cs_merge_constraints_assemble_dev")
        else:
            hm = np.ascontiguousarray(np.asarray(matches, dtype=np.int32).reshape(-1, 2))
            check(self._L.cs_merge_constraints_assemble(*head, hm.ctypes.data if len(hm) else None, len(hm)), "cs_merge_constraints_assemble")

    def info(self, d_groups, gId1, gId2, d_Rs=None, d_Ts=None, stream_ptr=None):
        """cs_merge_info_dev from the poses d_Rs / d_Ts (device pointers, [nPose][9] / [3] in the assembled order; default: the assembled,
        unsolved poses).  Enqueues only."""
        check(self._L.cs_merge_info_dev(self._m, self._stream(stream_ptr), d_groups, int(gId1), int(gId2), self.buf.Rs if d_Rs is None else d_Rs,
                                        self.buf.Ts if d_Ts is None else d_Ts), "cs_merge_info_dev")

    def solve(self, stream_ptr=None):
        """cs_merge_constraints_solve: the two solves of :646-647 on the assembled problem (the existing robust BA, fed the problem read
        back to the host); waits.  Nothing is solved behind a verdict other than MERGE_OK; a failed solve raises CoslamHipError."""
        check(self._L.cs_merge_constraints_solve(self._m, self._stream(stream_ptr)), "cs_merge_constraints_solve")

    def solution(self, which):
        """-> dict(Rs, Ts, pts, outlier, stats) of solve `which` (0: maxErr 800, 1 x 100; 1: maxErr 30, 5 x 30) of the last solve()"""
        import numpy as np

        from .ba import BAStats

        h = self.header()
        Rs, Ts, pts = np.zeros((h.nPose, 9)), np.zeros((h.nPose, 3)), np.zeros((h.P, 3))
        out, st = np.zeros(max(h.nObs, 1), np.int32), BAStats()
        p = lambda v: v.ctypes.data  # noqa: E731
        check(self._L.cs_merge_constraints_solution(self._m, int(which), p(Rs), p(Ts), p(pts), p(out), C.byref(st)),
              "cs_merge_constraints_solution")
        return dict(Rs=Rs, Ts=Ts, pts=pts, outlier=out[:h.nObs], stats=st)

    def info_solved(self, d_groups, gId1, gId2, stream_ptr=None):
        """cs_merge_constraints_info_dev: the MergeInfo list from the SOLVED poses; nInfo = 0 behind a rejected verdict, a failed solve or
        no solve at all.  Enqueues only."""
        check(self._L.cs_merge_constraints_info_dev(self._m, self._stream(stream_ptr), d_groups, int(gId1),
                                                    int(gId2)), "cs_merge_constraints_info_dev")

    def apply_map(self, d_slot2map, d_pointFeat, d_featRef, d_refStatic, nMap, d_mapPts=None, apply_points=True, d_counts=None, stream_ptr=None):
        """cs_merge_constraints_apply_map_dev: the merge list (mergeMapPoints, the duplicate marks) and -- behind a successful solve() --
        the solved coordinates onto the live tables.  d_slot2map: one device pointer per camera (or a merge_cams() array / list of dicts
        with a slot2map field); d_pointFeat, d_refStatic, d_mapPts, d_counts ([6] int32) may be None.  The verdict is read on the device;
        enqueues only."""
        vp = C.c_void_p
        if isinstance(d_slot2map, C.Array) and d_slot2map._type_ is MergeCam:
            ptrs = [d_slot2map[c].slot2map for c in range(len(d_slot2map))]
        else:
            ptrs = [p.get("slot2map") if isinstance(p, dict) else p for p in d_slot2map]
        if len(ptrs) != self.n_cams:
            raise ValueError(f"apply_map: {len(ptrs)} slot2map pointers, the handle has {self.n_cams} cameras")
        arr = (vp * self.n_cams)(*[vp(int(p)) if p else None for p in ptrs])
        check(self._L.cs_merge_constraints_apply_map_dev(self._m, self._stream(stream_ptr), arr, d_pointFeat, d_featRef, d_refStatic, int(nMap),
                                                         d_mapPts, 1 if apply_points else 0, d_counts),
              "cs_merge_constraints_apply_map_dev")

    def header(self, stream_ptr=None):
        """the header on the host; waits for the stream"""
        h = MergeConstraintsHeader()
        check(self._L.cs_merge_constraints_header_get(self._m, self._stream(stream_ptr), C.byref(h)),
              "cs_merge_constraints_header_get")
        return h

    def problem(self, stream_ptr=None):
        """-> dict(header, Ks, Rs, Ts, pts, pointMap, obs_ptr, obs_cam, obs_xy) as numpy, cut to the header's counts"""
        import numpy as np

        h, b = self.header(stream_ptr), self.buf
        d = self._down
        return dict(header=h, Ks=d(b.Ks, 9 * h.nPose, np.float64).reshape(-1, 9), Rs=d(b.Rs, 9 * h.nPose, np.float64).reshape(-1, 9),
                    Ts=d(b.Ts, 3 * h.nPose, np.float64).reshape(-1, 3), pts=d(b.pts, 3 * h.P, np.float64).reshape(-1, 3),
                    pointMap=d(b.pointMap, h.P, np.int32), obs_ptr=d(b.obsPtr, h.P + 1, np.int32) if h.verdict == MERGE_OK else np.zeros(1, np.int32),
                    obs_cam=d(b.obsCam, h.nObs, np.int32), obs_xy=d(b.obsXY, 2 * h.nObs, np.float64).reshape(-1, 2))

    def views(self, stream_ptr=None):
        """the merge list -> int32 [nMergeViews][7]: track, cam, slot, point, from, flags, prevSlot"""
        import numpy as np

        h = self.header(stream_ptr)
        return self._down(self.buf.views, 8 * h.nMergeViews, np.int32).reshape(-1, 8)[:, :7]

    def infos(self, stream_ptr=None):
        """-> (int32 [nInfo][7]: frame1, cam1, gid1, frame2, cam2, gid2, valid; R [nInfo][9]; t [nInfo][3])"""
        import numpy as np

        h, b = self.header(stream_ptr), self.buf
        ints = self._down(b.info, 6 * h.nInfo, np.int32).reshape(-1, 6)
        valid = self._down(b.infoValid, h.nInfo, np.uint8).astype(np.int32).reshape(-1, 1)
        return np.concatenate([ints, valid], axis=1), self._down(b.infoR, 9 * h.nInfo, np.float64).reshape(-1, 9), \
            self._down(b.infoT, 3 * h.nInfo, np.float64).reshape(-1, 3)


MERGE_HOLD_OFF = 130   # CoSLAM::mergeCamGroups: `curFrame < m_lastFrmGroupMerge + 130` (reference src/app/SL_CoSLAM.cpp:1381)


class MergeCamGroups:
    """CoSLAM::mergeCamGroups (reference src/app/SL_CoSLAM.cpp:1375-1446) behind its matcher, as one call: from the chosen camera pair with
    its feature matches to the merged history, map, tables and groups.  It owns a MergeConstraints handle (and, per run, a
    MergeApply handle, whose graphs depend on the key frames) and keeps last_merge_frame for the reference's hold-off of 130 frames.
    The closing currentMapPointsRegister(20.0, true) of :1439 is cs_register_decide_merge_dev and stays the caller's."""

    def __init__(self, n_cams, N, max_matches, max_map, device=0, last_merge_frame=-(1 << 30)):
        self.n_cams, self.N, self.device = int(n_cams), int(N), int(device)
        self.mc = MergeConstraints(n_cams, N, max_matches, max_map, device=device)
        self.ma = None
        self.last_merge_frame = int(last_merge_frame)
        self._keep = None

    def run(self, history, tables, groups, key_frames, self_motion, key_groups, pair, matches, pixelErrVar, last_release_frame=None,
            n_max_keyfrm=100, stream_ptr=None):
        """history: the TrackHistory, its newest frame the current key frame.  tables: dict of DEVICE pointers -- cams (per camera a dict
        xy, state, slot2map, K, iK of the current key frame), featRef, pointFeat (or None), refStatic (or None), nMap, mapPts, mapCov,
        mapCount (or None), firstFrame, lastFrame, mapFlags.  groups: the current record (a CameraGroups or a list of camera-id lists).
        key_frames: frame numbers oldest first, the current key frame last; self_motion [nKey][nCams]; key_groups: per key frame its record
        (what merge_keygraph_plan takes).  pair: (gId1, gId2, maxiCam, maxjCam); matches: int32 [K][2] slot pairs (host or device tensor).

        Enqueues merge_first_constrain, assemble, solve, info_solved, apply_map, merge_keygraph_plan, MergeApply.run_dev on the handle's
        d_infoR / d_infoT, MergeApply.recompute behind its guard, merge_matched_groups.  The merge list is applied only behind a verdict
        of MERGE_OK and two successful solves: otherwise history, map and tables are untouched, the hold-off is not armed and `status`
        names the cause ("held_off", "rejected", "solve_failed").  "pose_failed": the pose graphs failed numerically behind the applied
        list -- their guard kept the history and the re-triangulation from being written.

        -> dict(status, merged, verdict, header (dict of the counts), apply_counts [6], recompute_counts [4], solver (BAStats of both solves),
        groups, group_id, merged_gid, record)"""
        import numpy as np
        import torch

        from ._lib import CoslamHipError

        frames = [int(f) for f in key_frames]
        cur = frames[-1]
        rep = dict(status="held_off", merged=False, verdict=None, header=None, apply_counts=[0] * 6, recompute_counts=[0] * 4, solver=None,
                   groups=None, group_id=None, merged_gid=-1, record=None, error=None)
        if cur < self.last_merge_frame + MERGE_HOLD_OFF:
            return rep
        s = _stream(self.device, stream_ptr)
        dev = torch.device("cuda", self.device)
        gId1, gId2, iCam, jCam = (int(v) for v in pair)
        rec = _camera_groups_record(groups)
        glist = rec.groups()
        ids = sorted(set(glist[gId1]) | set(glist[gId2]))
        d_groups = torch.from_numpy(np.frombuffer(bytes(rec), np.uint8).copy()).to(dev)
        d_counts = torch.zeros(10, dtype=torch.int32, device=dev)
        self._keep = (d_groups, d_counts)
        T, mc = tables, self.mc
        k, _order = merge_first_constrain(frames, self_motion, ids)
        mc.assemble(history, [dict(xy=c["xy"], state=c["state"], slot2map=c["slot2map"], K=c["K"]) for c in T["cams"]], T["featRef"], T["nMap"],
                    T["mapPts"], d_groups.data_ptr(), gId1, gId2, iCam, jCam, frames[k], cur, matches, stream_ptr=s)
        try:
            mc.solve(stream_ptr=s)
        except CoslamHipError as e:
            rep.update(status="solve_failed", error=str(e))
        h = mc.header(stream_ptr=s)
        rep["verdict"] = int(h.verdict)
        rep["header"] = {n: int(getattr(h, n)) for n in ("nPose", "P", "nObs", "nMergedTracks", "nUnmerged", "nPrevViews", "skippedMatches",
                                                         "nMergeViews", "f1", "f2", "nCamIds")}
        rep["header"]["avgErr"] = float(h.avgErr)
        if rep["status"] == "solve_failed":
            return rep
        if h.verdict != MERGE_OK:
            rep["status"] = "rejected"
            return rep
        rep["solver"] = [mc.solution(w)["stats"] for w in (0, 1)]
        mc.info_solved(d_groups.data_ptr(), gId1, gId2, stream_ptr=s)
        ints, _R, _t = mc.infos(stream_ptr=s)
        if len(ints) == 0 or not (ints[:, 6] == 1).all():
            raise CoslamHipError("MergeCamGroups.run: the MergeInfo list is empty or holds an entry outside the pose order")
        mc.apply_map([c["slot2map"] for c in T["cams"]], T.get("pointFeat"), T["featRef"], T.get("refStatic"), T["nMap"], T["mapPts"], True,
                     d_counts.data_ptr(), stream_ptr=s)
        plan = merge_keygraph_plan(frames, key_groups, ids, k, iCam, jCam, ints[:, [0, 1, 3, 4]], n_max_keyfrm=n_max_keyfrm)
        if self.ma is not None:
            self.ma.close()
        self.ma = ma = MergeApply(plan, frames, self.n_cams, device=self.device)
        ma.run_dev(history, mc.buf.infoR, mc.buf.infoT, stream_ptr=s)
        fixed_frame = int(ma.key_frames[0])
        f_start = fixed_frame if last_release_frame is None else max(fixed_frame, int(last_release_frame))
        ma.recompute(history, [dict(K=c["K"], iK=c["iK"]) for c in T["cams"]], T["featRef"], T["nMap"], T.get("mapCount"), T["firstFrame"],
                     T["lastFrame"], T["mapFlags"], T["mapPts"], T["mapCov"], f_start, pixelErrVar, True, d_counts[6:].data_ptr(), stream_ptr=s)
        try:
            ma.status(stream_ptr=s)
        except CoslamHipError as e:
            rep.update(status="pose_failed", error=str(e))
        cnt = d_counts.cpu().tolist()
        rep["apply_counts"], rep["recompute_counts"] = cnt[:6], cnt[6:]
        if rep["status"] == "pose_failed":
            return rep
        valid = ints[ints[:, 2] >= 0]
        got = merge_matched_groups(rec, valid[:, 2], valid[:, 5], iCam, jCam)
        rep.update(status="merged", merged=True, groups=got["groups"], group_id=got["group_id"], merged_gid=got["merged_gid"], record=got["record"])
        self.last_merge_frame = cur
        return rep

    def run_from_seeds(self, matcher, match_cams, Ws, Hs, infos, surf_num, emat_ok, jobs, history, tables, groups, key_frames, self_motion,
                             key_groups, pixelErrVar, epi_max=20.0, ncc_min=0.45, max_disp=150.0, last_release_frame=None, n_max_keyfrm=100,
                             stream_ptr=None):
        """mergeCamGroups from the gate's list on: matcher -> counts (the one wait in front of the choice) -> merge_match_select -> run() with the
        chosen pair and the chosen job's matches handed over as a DEVICE table (never copied through the host).
        infos: the gate's list [(frame1, cam1, gid1, frame2, cam2, gid2)]; surf_num / emat_ok per entry (the host front: matchSURFPoints' count,
        computeEMat > 0); jobs: per entry None (skipped by the front) or dict(E, seeds) -- iCam / jCam are the entry's cameras.
        -> run()'s dict, plus choice (merge_match_select's dict), match_counts [nJobs][4] and job_of_entry; status "no_pair" when nothing
        was chosen (choice.status 0 or -1): nothing is enqueued behind the matcher then."""
        import torch

        s = _stream(self.device, stream_ptr)
        job_of, jl = [-1] * len(infos), []
        for e, (inf, j) in enumerate(zip(infos, jobs)):
            if j is None or surf_num[e] < 25 or not emat_ok[e]:
                continue
            job_of[e] = len(jl)
            jl.append(dict(iCam=int(inf[1]), jCam=int(inf[4]), E=j["E"], seeds=j.get("seeds")))
            if jl[-1]["seeds"] is None:
                jl[-1].pop("seeds")
        if jl:
            matcher.run(match_cams, Ws, Hs, jl, epi_max, ncc_min, max_disp, stream_ptr=s)
        cnt = matcher.counts(len(jl), stream_ptr=s)
        ncc = [int(cnt[k][0]) if k >= 0 else 0 for k in job_of]
        elig = [1 if k >= 0 and cnt[k][1] == 0 else 0 for k in job_of]
        ok = [1 if (emat_ok[e] and job_of[e] >= 0) else 0 for e in range(len(infos))]
        rec = _camera_groups_record(groups)
        choice = merge_match_select(infos, surf_num, ok, ncc, [int(rec.num[g]) for g in range(MAX_CAMS)], elig)
        if choice["status"] != 1:
            return dict(status="no_pair", merged=False, choice=choice, match_counts=cnt, job_of_entry=job_of)
        k = job_of[choice["entry"]]
        d_matches = torch.as_tensor(_DeviceInt32View(matcher.matches_ptr(k), int(cnt[k][0])), device=torch.device("cuda", self.device))
        rep = self.run(history, tables, groups, key_frames, self_motion, key_groups,
                       (choice["maxgId1"], choice["maxgId2"], choice["maxiCam"], choice["maxjCam"]), d_matches, pixelErrVar,
                       last_release_frame=last_release_frame, n_max_keyfrm=n_max_keyfrm, stream_ptr=s)
        rep.update(choice=choice, match_counts=cnt, job_of_entry=job_of, matches_ptr=matcher.matches_ptr(k))
        return rep

    def run_from_descriptors(self, front, front_cams, matcher, match_cams, Ws, Hs, infos, history, tables, groups, key_frames, self_motion,
                             key_groups, pixelErrVar, ratio=0.8, max_dist=0.6, n_ransac=200, max_epi_err=2.0, min_inlier_num=15, seed=0,
                             epi_max=20.0, ncc_min=0.45, max_disp=150.0, last_release_frame=None, n_max_keyfrm=100, stream_ptr=None,
                             device_jobs=False, min_surf_num=25):
        """mergeCamGroups from the gate's list and the key frames' key points + descriptors: MergeFront.run over every entry's camera pair
        (matchSURFPoints, computeEMat, getMatchedPts), then run_from_seeds with what it returned.  front: a MergeFront;
        front_cams: per camera dict(pts, desc: device pointers, n, K).  E and the seeds pass through the front's one read-back (the matcher's
        job table takes them from host memory).  -> run_from_seeds' dict, plus front (MergeFront.run's list).
        device_jobs=True: front.enqueue -> matcher.run_front, the matcher's jobs filled on the device from the front's buffers, and ONE wait
        (matcher.counts, then front.results without another): no seed rows come to the host.  Entry e is job e: match_counts is
        [nEntries][4], job_of_entry[e] is e, or -1 for a skipped or seed-overflowed entry, and the front's records carry no `seeds`."""
        import torch

        s = _stream(self.device, stream_ptr)
        if device_jobs:
            pairs = [(int(inf[1]), int(inf[4])) for inf in infos]
            front.enqueue(front_cams, pairs, ratio, max_dist, n_ransac, max_epi_err, min_inlier_num, seed, stream_ptr=s)
            matcher.run_front(match_cams, Ws, Hs, pairs, front, min_surf_num, epi_max, ncc_min, max_disp, stream_ptr=s)
            cnt = matcher.counts(len(infos), stream_ptr=s)          # the one wait
            got = front.results(len(infos), stream_ptr=s)
            skipped = [bool(cnt[e][1] & MERGE_MATCH_SKIPPED) for e in range(len(infos))]
            job_of = [-1 if cnt[e][1] & (MERGE_MATCH_SKIPPED | MERGE_MATCH_SEEDS_OVERFLOW) else e for e in range(len(infos))]
            ncc = [int(cnt[e][0]) for e in range(len(infos))]
            elig = [1 if cnt[e][1] == 0 else 0 for e in range(len(infos))]
            ok = [1 if (got[e]["emat_ok"] and not skipped[e]) else 0 for e in range(len(infos))]
            rec = _camera_groups_record(groups)
            choice = merge_match_select(infos, [g["surf_num"] for g in got], ok, ncc, [int(rec.num[g]) for g in range(MAX_CAMS)], elig)
            if choice["status"] != 1:
                return dict(status="no_pair", merged=False, choice=choice, match_counts=cnt, job_of_entry=job_of, front=got)
            k = choice["entry"]
            d_matches = torch.as_tensor(_DeviceInt32View(matcher.matches_ptr(k), int(cnt[k][0])), device=torch.device("cuda", self.device))
            rep = self.run(history, tables, groups, key_frames, self_motion, key_groups,
                           (choice["maxgId1"], choice["maxgId2"], choice["maxiCam"], choice["maxjCam"]), d_matches, pixelErrVar,
                           last_release_frame=last_release_frame, n_max_keyfrm=n_max_keyfrm, stream_ptr=s)
            rep.update(choice=choice, match_counts=cnt, job_of_entry=job_of, matches_ptr=matcher.matches_ptr(k), front=got)
            return rep
        got = front.run(front_cams, [(int(inf[1]), int(inf[4])) for inf in infos], ratio, max_dist, n_ransac, max_epi_err, min_inlier_num, seed,
                        stream_ptr=s)
        rep = self.run_from_seeds(matcher, match_cams, Ws, Hs, infos, [g["surf_num"] for g in got], [g["emat_ok"] for g in got],
                                  [dict(E=g["E"], seeds=g["seeds"]) for g in got], history, tables, groups, key_frames, self_motion,
                                  key_groups, pixelErrVar, epi_max=epi_max, ncc_min=ncc_min, max_disp=max_disp,
                                  last_release_frame=last_release_frame, n_max_keyfrm=n_max_keyfrm, stream_ptr=s)
        rep["front"] = got
        return rep

    def close(self):
        if self.ma is not None:
            self.ma.close()
            self.ma = None
        if self.mc is not None:
            self.mc.close()
            self.mc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MERGE_MATCH_MAX_JOBS = 256
MERGE_MATCH_PAIRS_OVERFLOW, MERGE_MATCH_MATCHES_OVERFLOW, MERGE_MATCH_SKIPPED, MERGE_MATCH_SEEDS_OVERFLOW = 1, 2, 4, 8


class MergeMatchCam(C.Structure):
    """xy / state / imgSmall device pointers, K a HOST pointer."""

    _c_type_ = "cs_merge_match_cam"
    _fields_ = [("xy", C.c_void_p), ("state", C.c_void_p), ("K", C.c_void_p), ("imgSmall", C.c_void_p), ("imgScale", C.c_double)]


class MergeMatchJob(C.Structure):
    _c_type_ = "cs_merge_match_job"
    _fields_ = [("iCam", C.c_int), ("jCam", C.c_int), ("E", C.c_double * 9), ("nSeeds", C.c_int), ("seeds", C.c_void_p)]


class MergeMatchFrontJob(C.Structure):
    _c_type_ = "cs_merge_match_front_job"
    _fields_ = [("F", C.c_double * 9), ("nSeeds", C.c_int), ("flags", C.c_int)]


class MergeMatchBuffers(C.Structure):
    _c_type_ = "cs_merge_match_buffers"
    _fields_ = [(n, C.c_void_p) for n in ("matches", "scores", "counts", "pairs", "pairCount", "blocks", "abc", "valid")] + \
               [(n, C.c_int) for n in ("nCams", "N", "maxJobs", "maxSeeds", "pairCap", "maxMatches")]


class MergeMatchChoice(C.Structure):
    _c_type_ = "cs_merge_match_choice"
    _fields_ = [(n, C.c_int) for n in ("status", "entry", "maxk", "maxiCam", "maxjCam", "maxgId1", "maxgId2", "gid1", "gid2", "camid1", "camid2")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class _DeviceInt32View:
    """a [rows][2] int32 table in device memory as torch.as_tensor takes it (no copy)"""

    def __init__(self, ptr, rows):
        self.__cuda_array_interface__ = dict(shape=(int(rows), 2), typestr="<i4", data=(int(ptr), False), version=2, strides=None)


def merge_match_fmat(K1, K2, E):
    """cs_merge_match_fmat (host code): F of matchFeaturePointsNCC = iK1^T E^T iK2"""
    import numpy as np

    a, b, e = (np.ascontiguousarray(v, dtype=np.float64).reshape(9) for v in (K1, K2, E))
    F = np.zeros(9)
    p = lambda v: v.ctypes.data  # noqa: E731
    check(lib().cs_merge_match_fmat(p(a), p(b), p(e), p(F)), "cs_merge_match_fmat")
    return F


def merge_match_select(infos, surf_num, emat_ok, ncc_num, group_size, eligible=None):
    """cs_merge_match_select (host code): matchMergableCameras' loop over the gate's list.  infos: [(frame1, cam1, gid1, frame2, cam2, gid2)]
    (MergeCandidates.infos()); per entry the SURF match count, whether computeEMat succeeded, the NCC match count and (optionally) whether
    the job may be chosen (a flagged job may not); group_size[g] = camGroups[g].num.  -> dict(status, entry, maxk, maxiCam, maxjCam, maxgId1,
    maxgId2, gid1, gid2, camid1, camid2); status 1: chosen, 0: nothing matched, -1: the reference's undefined run (no pair)."""
    import numpy as np

    n = len(infos)
    arr = (MergeInfo * max(n, 1))()
    for a, t in zip(arr, infos):
        for (name, _), v in zip(MergeInfo._fields_, t):
            setattr(a, name, int(v))
    sn = np.ascontiguousarray(surf_num, dtype=np.int32).reshape(-1)
    ok = np.ascontiguousarray(np.asarray(emat_ok) != 0, dtype=np.uint8).reshape(-1)
    nn = np.ascontiguousarray(ncc_num, dtype=np.int32).reshape(-1)
    assert len(sn) == n and len(ok) == n and len(nn) == n
    gs = np.zeros(MAX_CAMS, np.int32)
    gs[:len(group_size)] = np.asarray(group_size, dtype=np.int32)
    el = None if eligible is None else np.ascontiguousarray(np.asarray(eligible) != 0, dtype=np.uint8).reshape(-1)
    p = lambda v: v.ctypes.data if v is not None and len(v) else None  # noqa: E731
    out = MergeMatchChoice()
    check(lib().cs_merge_match_select(n, arr, p(sn), p(ok), p(nn), p(el), p(gs), C.byref(out)), "cs_merge_match_select")
    return out.as_dict()


class MergeMatcher(_MergeHandle):
    """cs_merge_match: MergeCameraGroup::matchFeaturePointsNCC on the device for the candidate camera pairs of a key frame -- blocks from
    the key frame's small images, the epipolar / NCC candidate lists, the seed-guided greedy one-to-one matching.  The
    outputs stay in device memory: matches_ptr(k) is what MergeConstraints.assemble / MergeCamGroups.run take as a device table."""

    _prefix, _Buffers = "cs_merge_match", MergeMatchBuffers

    def __init__(self, n_cams, N, max_jobs, max_seeds, pair_cap, max_matches, device=0):
        self.n_cams, self.N = int(n_cams), int(N)
        self.max_jobs, self.max_seeds, self.pair_cap, self.max_matches = int(max_jobs), int(max_seeds), int(pair_cap), int(max_matches)
        self._create(device, self.n_cams, self.N, self.max_jobs, self.max_seeds, self.pair_cap, self.max_matches)
        self._keep = None

    def _cams(self, cams):
        import numpy as np

        ca = (MergeMatchCam * max(len(cams), 1))()
        keep = []
        for a, c in zip(ca, cams):
            K = np.ascontiguousarray(c["K"], dtype=np.float64).reshape(9)
            keep.append(K)
            a.xy, a.state, a.K, a.imgSmall, a.imgScale = int(c["xy"]) or None, int(c["state"]) or None, K.ctypes.data, int(c["imgSmall"]) or None, float(c["imgScale"])
        return ca, keep

    def run_front(self, cams, Ws, Hs, pairs, front, min_surf_num=25, epi_max=20.0, ncc_min=0.45, max_disp=150.0, stream_ptr=None):
        """cs_merge_match_run_front_dev: run() with E, the seed count and the seed rows of job k taken ON THE DEVICE from what
        front.enqueue left (front: a MergeFront, or a dict results / seeds (device pointers) / rows (seed rows per job)); pairs:
        [(iCam, jCam)], entry k is job k.  A job with surf_num < min_surf_num or without E is skipped (counts row [0, 4, 0, 0]), one with
        more inliers than max_seeds gets [0, 8, 0, 0].  Enqueues only."""
        if len(cams) != self.n_cams:
            raise ValueError(f"MergeMatcher.run_front: {len(cams)} cameras, the handle has {self.n_cams}")
        ca, _keep = self._cams(cams)
        ja = (MergeFrontJob * max(len(pairs), 1))()
        for a, (i, j) in zip(ja, pairs):
            a.iCam, a.jCam = int(i), int(j)
        src = front if isinstance(front, dict) else dict(results=front.buf.results, seeds=front.buf.seeds, rows=front.max_pts)
        check(self._L.cs_merge_match_run_front_dev(self._m, self._stream(stream_ptr), ca, int(Ws), int(Hs), len(pairs), ja if len(pairs) else None,
                                                   int(src["results"]) or None, int(src["seeds"]) or None, int(src["rows"]), int(min_surf_num),
                                                   epi_max, ncc_min, max_disp), "cs_merge_match_run_front_dev")

    def front_jobs(self, n_jobs, stream_ptr=None):
        """cs_merge_match_front_jobs: what the last run_front made of jobs 0 .. n_jobs - 1 -> dict(F float64 [n][9], n_seeds, flags); waits"""
        import numpy as np

        arr = (MergeMatchFrontJob * max(int(n_jobs), 1))()
        check(self._L.cs_merge_match_front_jobs(self._m, self._stream(stream_ptr), int(n_jobs), arr), "cs_merge_match_front_jobs")
        rows = arr[:int(n_jobs)]
        return dict(F=np.array([list(r.F) for r in rows], dtype=np.float64).reshape(-1, 9), n_seeds=np.array([r.nSeeds for r in rows], np.int32),
                    flags=np.array([r.flags for r in rows], np.int32))

    def run(self, cams, Ws, Hs, jobs, epi_max=20.0, ncc_min=0.45, max_disp=150.0, stream_ptr=None):
        """cs_merge_match_run_dev.  cams: per camera a dict xy, state, imgSmall (device pointers), K (9 doubles, HOST array), imgScale;
        jobs: [dict(iCam, jCam, E [9], seeds [n][4] = x1, y1, x2, y2)].  The defaults are the reference's call (20.0, 0.45, 150).
        Enqueues only."""
        import numpy as np

        ca, keep = self._cams(cams)
        ja = (MergeMatchJob * max(len(jobs), 1))()
        for a, j in zip(ja, jobs):
            sd = np.ascontiguousarray(np.asarray(j.get("seeds", np.zeros((0, 4))), dtype=np.float64).reshape(-1, 4))
            keep.append(sd)
            a.iCam, a.jCam, a.nSeeds, a.seeds = int(j["iCam"]), int(j["jCam"]), len(sd), (sd.ctypes.data if len(sd) else None)
            a.E[:] = [float(v) for v in np.asarray(j["E"], dtype=np.float64).reshape(9)]
        if len(cams) != self.n_cams:
            raise ValueError(f"MergeMatcher.run: {len(cams)} cameras, the handle has {self.n_cams}")
        check(self._L.cs_merge_match_run_dev(self._m, self._stream(stream_ptr), ca, int(Ws), int(Hs), len(jobs), ja if len(jobs) else None, epi_max,
                                             ncc_min, max_disp), "cs_merge_match_run_dev")

    def from_pairs(self, d_pairs, d_pair_count, d_xy1, d_xy2, seeds=None, max_disp=150.0, stream_ptr=None):
        """cs_merge_match_from_pairs_dev: the matcher alone.  Per job a device pointer to its cs_ncc_pair records, to its count, to the
        positions of both cameras (2N doubles each); seeds: per job a host [n][4] array or None.  Enqueues only."""
        import numpy as np

        vp = C.c_void_p
        n = len(d_pairs)
        arr = lambda v: (vp * max(n, 1))(*[vp(int(x)) if x else None for x in v])  # noqa: E731
        sds = [np.ascontiguousarray(np.asarray(s if s is not None else np.zeros((0, 4)), dtype=np.float64).reshape(-1, 4))
               for s in (seeds if seeds is not None else [None] * n)]
        ns = (C.c_int * max(n, 1))(*[len(s) for s in sds])
        sp = (vp * max(n, 1))(*[vp(s.ctypes.data) if len(s) else None for s in sds])
        check(self._L.cs_merge_match_from_pairs_dev(self._m, self._stream(stream_ptr), n, arr(d_pairs), arr(d_pair_count), arr(d_xy1), arr(d_xy2), ns,
                                                    sp, max_disp), "cs_merge_match_from_pairs_dev")

    def counts(self, n_jobs, stream_ptr=None):
        """cs_merge_match_counts: the stage's one host wait -> int32 [n_jobs][4] = matches kept, flags, candidates, rounds"""
        import numpy as np

        out = np.zeros((max(int(n_jobs), 1), 4), np.int32)
        check(self._L.cs_merge_match_counts(self._m, self._stream(stream_ptr), int(n_jobs), out.ctypes.data),
              "cs_merge_match_counts")
        return out[:int(n_jobs)]

    def matches_ptr(self, job):
        """device pointer of job's [maxMatches][2] int32 slot pairs"""
        return int(self.buf.matches) + 8 * self.max_matches * int(job)

    def matches(self, job, count, stream_ptr=None):
        """-> (int32 [count][2] slot pairs in acceptance order, float64 [count] scores) of one job; waits"""
        import numpy as np

        m = self._down(self.matches_ptr(job), 2 * int(count), np.int32, stream_ptr).reshape(-1, 2)
        return m, self._down(int(self.buf.scores) + 8 * self.max_matches * int(job), int(count), np.float64, stream_ptr)

    def blocks(self, stream_ptr=None):
        """-> (uint8 [nCams][N][128], float64 [nCams][N][4], int32 [nCams][N]) of the last run; waits"""
        import numpy as np

        n = self.n_cams * self.N
        return self._down(self.buf.blocks, n * 128, np.uint8, stream_ptr).reshape(self.n_cams, self.N, 128), \
            self._down(self.buf.abc, n * 4, np.float64, stream_ptr).reshape(self.n_cams, self.N, 4), \
            self._down(self.buf.valid, n, np.int32, stream_ptr).reshape(self.n_cams, self.N)

    def pairs(self, slot, stream_ptr=None):
        """the candidate list at batch slot `slot` of the last batch -> (total that passed, records cut to pairCap as a structured array
        i, j, epi, ncc); the list's order is not defined; waits"""
        import numpy as np

        dt = np.dtype([("i", np.int32), ("j", np.int32), ("epi", np.float64), ("ncc", np.float64)])
        total = int(self._down(int(self.buf.pairCount) + 4 * int(slot), 1, np.int32, stream_ptr)[0])
        return total, self._down(int(self.buf.pairs) + dt.itemsize * self.pair_cap * int(slot), min(total, self.pair_cap), dt, stream_ptr)


def ncc_small_image_dev(stream_ptr, d_img, W, H, scale, d_small, device=0):
    """cs_ncc_small_image_dev: SingleSLAM's small image, cv::resize(img, small, Size((int)(W s), (int)(H s))) -> (Ws, Hs); enqueues only"""
    ws, hs = C.c_int(), C.c_int()
    check(lib().cs_ncc_small_dims(int(W), int(H), scale, C.byref(ws), C.byref(hs)), "cs_ncc_small_dims")
    check(lib().cs_ncc_small_image_dev(int(device), stream_ptr, d_img, int(W), int(H), scale, d_small),
          "cs_ncc_small_image_dev")
    return ws.value, hs.value


MERGE_FRONT_MAX_JOBS = 256
MERGE_FRONT_TOO_FEW, MERGE_FRONT_NO_MODEL = 1, 2


class MergeFrontCam(C.Structure):
    """pts / desc device pointers, K a HOST pointer."""

    _c_type_ = "cs_merge_front_cam"
    _fields_ = [("pts", C.c_void_p), ("desc", C.c_void_p), ("K", C.c_void_p), ("n", C.c_int)]


class MergeFrontJob(C.Structure):
    _c_type_ = "cs_merge_front_job"
    _fields_ = [("iCam", C.c_int), ("jCam", C.c_int)]


class MergeFrontResult(C.Structure):
    _c_type_ = "cs_merge_front_result"
    _fields_ = [(n, C.c_int) for n in ("surfNum", "ematOk", "inlierNum", "rounds", "bestHyp", "flags")] + [("E", C.c_double * 9), ("epiErr", C.c_double)]


class MergeFrontBuffers(C.Structure):
    _c_type_ = "cs_merge_front_buffers"
    _fields_ = [(n, C.c_void_p) for n in ("matches", "dist", "count", "inlierFlag", "seeds", "newMatches", "results", "hypSample", "hypCount",
                                          "hypE", "pix", "valid")] + [(n, C.c_int) for n in ("nCams", "maxPts", "dimDesc", "maxJobs", "maxHyp")]


class MergeFront(_MergeHandle):
    """cs_merge_front: the front of matchMergableCameras on the device -- matchSurf over the descriptors of every candidate camera pair, the
    RANSAC of estimateEMat with its local refit, the inliers' seed rows.  From key points + descriptors to what MergeMatcher.run
    and merge_match_select take per job: E, seeds, surf_num, emat_ok."""

    _prefix, _Buffers = "cs_merge_front", MergeFrontBuffers

    def __init__(self, n_cams, max_pts, dim_desc, max_jobs, max_hyp, device=0):
        self.n_cams, self.max_pts, self.dim, self.max_jobs, self.max_hyp = int(n_cams), int(max_pts), int(dim_desc), int(max_jobs), int(max_hyp)
        self._create(device, self.n_cams, self.max_pts, self.dim, self.max_jobs, self.max_hyp)

    def _tables(self, cams, pairs):
        import numpy as np

        if len(cams) != self.n_cams:
            raise ValueError(f"MergeFront: {len(cams)} cameras, the handle has {self.n_cams}")
        ca, keep = (MergeFrontCam * max(len(cams), 1))(), []
        for a, c in zip(ca, cams):
            K = np.ascontiguousarray(c["K"], dtype=np.float64).reshape(9)
            keep.append(K)
            a.pts, a.desc, a.K, a.n = int(c["pts"]) or None, int(c.get("desc") or 0) or None, K.ctypes.data, int(c["n"])
        ja = (MergeFrontJob * max(len(pairs), 1))()
        for a, (i, j) in zip(ja, pairs):
            a.iCam, a.jCam = int(i), int(j)
        return ca, ja, keep

    def enqueue(self, cams, pairs, ratio=0.8, max_dist=0.6, n_ransac=200, max_epi_err=2.0, min_inlier_num=15, seed=0, stream_ptr=None):
        """cs_merge_front_run_dev.  cams: per camera a dict pts [n][2] f64, desc [n][dim] f32 (device pointers), n, K (9 doubles, HOST array);
        pairs: [(iCam, jCam)].  The defaults are the reference's call (0.8, 0.6; 200, 2.0, 15).  Enqueues only."""
        ca, ja, _keep = self._tables(cams, pairs)
        check(self._L.cs_merge_front_run_dev(self._m, self._stream(stream_ptr), ca, len(pairs), ja if len(pairs) else None, ratio, max_dist,
                                             int(n_ransac), max_epi_err, int(min_inlier_num), int(seed)), "cs_merge_front_run_dev")

    def match(self, cams, pairs, ratio=0.8, max_dist=0.6, stream_ptr=None):
        """cs_merge_front_match_dev: the descriptor stage alone.  Enqueues only."""
        ca, ja, _keep = self._tables(cams, pairs)
        check(self._L.cs_merge_front_match_dev(self._m, self._stream(stream_ptr), ca, len(pairs), ja if len(pairs) else None, ratio,
                                               max_dist), "cs_merge_front_match_dev")

    def from_matches(self, cams, pairs, matches, n_ransac=200, max_epi_err=2.0, min_inlier_num=15, seed=0, stream_ptr=None):
        """cs_merge_front_from_matches_dev: the RANSAC stage alone (computeEMat's shape); matches: per job a host int [n][2].  Enqueues only."""
        import numpy as np

        vp = C.c_void_p
        ca, ja, _keep = self._tables(cams, pairs)
        ms = [np.ascontiguousarray(np.asarray(m, dtype=np.int32).reshape(-1, 2)) for m in matches]
        n = len(pairs)
        if len(ms) != n:
            raise ValueError("MergeFront.from_matches: one match list per job")
        mp = (vp * max(n, 1))(*[vp(m.ctypes.data) if len(m) else None for m in ms])
        nm = (C.c_int * max(n, 1))(*[len(m) for m in ms])
        check(self._L.cs_merge_front_from_matches_dev(self._m, self._stream(stream_ptr), ca, n, ja if n else None, mp, nm, int(n_ransac), max_epi_err,
                                                      int(min_inlier_num), int(seed)),
              "cs_merge_front_from_matches_dev")

    def results(self, n_jobs, stream_ptr=None):
        """cs_merge_front_results: the stage's one host wait -> [dict(surf_num, emat_ok, inlier_num, rounds, best_hyp, flags, E [9], epi_err)]"""
        import numpy as np

        arr = (MergeFrontResult * max(int(n_jobs), 1))()
        check(self._L.cs_merge_front_results(self._m, self._stream(stream_ptr), int(n_jobs), arr), "cs_merge_front_results")
        return [dict(surf_num=int(r.surfNum), emat_ok=int(r.ematOk), inlier_num=int(r.inlierNum), rounds=int(r.rounds), best_hyp=int(r.bestHyp),
                     flags=int(r.flags), E=np.array(list(r.E)), epi_err=float(r.epiErr)) for r in arr[:int(n_jobs)]]

    def run(self, cams, pairs, ratio=0.8, max_dist=0.6, n_ransac=200, max_epi_err=2.0, min_inlier_num=15, seed=0, stream_ptr=None):
        """enqueue + results + the seed rows of every job -> per job what MergeCamGroups.run_from_seeds takes: dict(E, seeds [inlier_num][4],
        surf_num, emat_ok) (plus the rest of the result record)"""
        self.enqueue(cams, pairs, ratio, max_dist, n_ransac, max_epi_err, min_inlier_num, seed, stream_ptr)
        import numpy as np

        out = self.results(len(pairs), stream_ptr)
        rows = self._down(self.buf.seeds, 4 * self.max_pts * len(pairs), np.float64, stream_ptr).reshape(len(pairs), self.max_pts, 4)
        for k, r in enumerate(out):      # (one download for every job's rows)
            r["seeds"] = np.ascontiguousarray(rows[k, :r["inlier_num"]])
        return out

    def counts(self, n_jobs, stream_ptr=None):
        """matchSurf's count of jobs 0 .. n_jobs - 1; waits"""
        import numpy as np

        return self._down(self.buf.count, int(n_jobs), np.int32, stream_ptr)

    def matches(self, job, count, stream_ptr=None):
        """-> (int32 [count][2] in ascending i, float32 [count] distances) of one job; waits"""
        import numpy as np

        return self._down(int(self.buf.matches) + 8 * self.max_pts * int(job), 2 * int(count), np.int32, stream_ptr).reshape(-1, 2), \
            self._down(int(self.buf.dist) + 4 * self.max_pts * int(job), int(count), np.float32, stream_ptr)

    def inlier_flags(self, job, count, stream_ptr=None):
        import numpy as np

        return self._down(int(self.buf.inlierFlag) + self.max_pts * int(job), int(count), np.uint8, stream_ptr)

    def seeds(self, job, count, stream_ptr=None):
        """-> float64 [count][4] rows {x1, y1, x2, y2} of the inliers in match order; waits"""
        import numpy as np

        return self._down(int(self.buf.seeds) + 32 * self.max_pts * int(job), 4 * int(count), np.float64, stream_ptr).reshape(-1, 4)

    def new_matches(self, job, count, stream_ptr=None):
        import numpy as np

        return self._down(int(self.buf.newMatches) + 8 * self.max_pts * int(job), 2 * int(count), np.int32, stream_ptr).reshape(-1, 2)

    def hypotheses(self, slot, n_hyp, stream_ptr=None):
        """the hypotheses at batch slot `slot` of the last batch -> (int32 [n_hyp][8] samples, int32 [n_hyp] counts, float64 [n_hyp][9]); waits"""
        import numpy as np

        b, h = self.max_hyp * int(slot), int(n_hyp)
        return self._down(int(self.buf.hypSample) + 32 * b, 8 * h, np.int32, stream_ptr).reshape(-1, 8), \
            self._down(int(self.buf.hypCount) + 4 * b, h, np.int32, stream_ptr), \
            self._down(int(self.buf.hypE) + 72 * b, 9 * h, np.float64, stream_ptr).reshape(-1, 9)

    def point_rows(self, slot, count, stream_ptr=None):
        """the rows {x1, y1, x2, y2} of every match at batch slot `slot`; waits"""
        import numpy as np

        return self._down(int(self.buf.pix) + 32 * self.max_pts * int(slot), 4 * int(count), np.float64, stream_ptr).reshape(-1, 4)
