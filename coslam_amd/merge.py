"""ctypes mirror of cs_merge_check_dev (include/coslam_hip.h): MergeCameraGroup::checkPossibleMergable (reference
src/app/SL_MergeCameraGroup.cpp:56-177) on the device -- which camera pairs of two separated camera groups see the same part of the map
again and stand close enough, over a key frame's record of the groups; one launch, no wait."""
import ctypes as C

from ._lib import check, lib

MAX_CAMS = 16
MAX_INFO = 256


class MergeCam(C.Structure):
    """== cs_merge_cam (include/coslam_hip.h)."""

    _fields_ = [("xy", C.c_void_p), ("state", C.c_void_p), ("slot2map", C.c_void_p), ("K", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p)]


class MergeInfo(C.Structure):
    """== cs_merge_info: MergeInfo::set(frame1, cam1, gid1, frame2, cam2, gid2)."""

    _fields_ = [(n, C.c_int) for n in ("frame1", "cam1", "gid1", "frame2", "cam2", "gid2")]

    def as_tuple(self):
        return tuple(int(getattr(self, n)) for n, _ in self._fields_)


class MergeCandidates(C.Structure):
    """== cs_merge_candidates (include/coslam_hip.h)."""

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
    fn = lib().cs_merge_check_scratch_bytes
    fn.restype = C.c_size_t
    return int(fn(int(nCams), int(N)))


def merge_check_dev(stream_ptr, cams, N, nMap, d_mapCount, d_mapPts, d_mapFlags, W, H, d_groups, frame, d_out, d_scratch, minInNum=10,
                    minInAreaRatio=0.5, maxCamDist=6.0, allPairs=False, device=0):
    """cs_merge_check_dev: checkPossibleMergable(minInNum, minInAreaRatio, maxCamDist) over the record d_groups (a CameraGroups in device
    memory) into d_out (a MergeCandidates in device memory).  cams: a merge_cams() array or a list of dicts.  The defaults are the
    reference's call (10, 0.5, Param::maxDistRatio = 6.0 taken as a distance)."""
    vp = C.c_void_p
    arr = merge_cams(cams)
    check(lib().cs_merge_check_dev(int(device), vp(stream_ptr), len(arr), arr if len(arr) else None, int(N), int(nMap), vp(d_mapCount), vp(d_mapPts),
                                   vp(d_mapFlags), int(W), int(H), vp(d_groups), int(frame), int(minInNum), C.c_double(minInAreaRatio),
                                   C.c_double(maxCamDist), 1 if allPairs else 0, vp(d_out), vp(d_scratch)),
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
    p = lambda v: C.c_void_p(v.ctypes.data)  # noqa: E731
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
