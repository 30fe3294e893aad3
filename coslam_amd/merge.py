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
