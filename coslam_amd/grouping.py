"""ctypes mirror of cs_view_overlap_costs_dev / cs_camera_grouping_dev (include/coslam_hip.h): CoSLAM::getViewOverlapCosts and
CoSLAM::cameraGrouping (reference src/app/SL_CoSLAM.cpp:1543-1630, :1632-1697) on the device -- the shared-point counts and hull areas of
every camera pair of the frame, the distance cut and the connected components in the reference's order of discovery."""
import ctypes as C

from ._lib import check, lib

MAX_CAMS = 16


class GroupingCam(C.Structure):
    _c_type_ = "cs_grouping_cam"
    _fields_ = [("xy", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p)]


class CameraGroups(C.Structure):
    """CameraGroup m_groups[] / m_groupNum / m_groupId[]."""

    _c_type_ = "cs_camera_groups"
    _fields_ = [("groupNum", C.c_int), ("num", C.c_int * MAX_CAMS), ("camIds", (C.c_int * MAX_CAMS) * MAX_CAMS), ("groupId", C.c_int * MAX_CAMS)]

    def groups(self):
        """[[camera, ...], ...] in the order of discovery"""
        return [[int(self.camIds[g][k]) for k in range(self.num[g])] for g in range(self.groupNum)]

    @classmethod
    def from_bytes(cls, buf):
        return cls.from_buffer_copy(bytes(buf))


def grouping_cams(cams):
    """list of dicts of DEVICE pointers (ints) with the field names of cs_grouping_cam -> the ctypes array (build once)"""
    if isinstance(cams, C.Array):
        return cams
    arr = (GroupingCam * len(cams))()
    for a, c in zip(arr, cams):
        for n, _ in GroupingCam._fields_:
            v = c.get(n)
            setattr(a, n, int(v) if v else None)
    return arr


def camera_grouping_scratch_bytes(nCams, N):
    """bytes of device scratch of the two entries: zero it once before the first call, every call leaves it zeroed"""
    return lib().cs_camera_grouping_scratch_bytes(int(nCams), int(N))


def _common(stream_ptr, cams, N, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_list, d_listCount, W, H, minOverlapNum, minOverlapAreaRatio, d_vcosts,
            d_nShare, d_hullArea, d_scratch, device):
    arr = grouping_cams(cams)
    return (int(device), stream_ptr, len(arr), arr if len(arr) else None, int(N), int(nMap), d_mapCount, d_pointFeat, d_mapFlags, d_list, d_listCount,
            int(W), int(H), int(minOverlapNum), minOverlapAreaRatio, d_vcosts, d_nShare, d_hullArea, d_scratch)


def view_overlap_costs_dev(stream_ptr, cams, N, nMap, d_mapCount, d_pointFeat, d_mapFlags, W, H, d_vcosts, d_nShare, d_scratch, minOverlapNum=0,
                           minOverlapAreaRatio=0.0, d_hullArea=None, d_list=None, d_listCount=None, device=0):
    """cs_view_overlap_costs_dev.  cams: a grouping_cams() array or a list of dicts.  The hull path runs when minOverlapAreaRatio > 0 or
    d_hullArea is given."""
    check(lib().cs_view_overlap_costs_dev(*_common(stream_ptr, cams, N, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_list, d_listCount, W, H,
                                                   minOverlapNum, minOverlapAreaRatio, d_vcosts, d_nShare, d_hullArea, d_scratch, device)),
          "cs_view_overlap_costs_dev")


def camera_grouping_dev(stream_ptr, cams, N, nMap, d_mapCount, d_pointFeat, d_mapFlags, W, H, d_vcosts, d_nShare, d_scratch, initCamTranslation,
                        d_groups, maxDistRatio=6.0, minOverlapNum=0, minOverlapAreaRatio=0.0, d_hullArea=None, d_list=None, d_listCount=None,
                        device=0):
    """cs_camera_grouping_dev: the costs (the reference's call is (0, 0.0)), the distance cut, the components into d_groups (a CameraGroups
    in device memory)."""
    check(lib().cs_camera_grouping_dev(*_common(stream_ptr, cams, N, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_list, d_listCount, W, H,
                                                minOverlapNum, minOverlapAreaRatio, d_vcosts, d_nShare, d_hullArea, d_scratch, device),
                                       initCamTranslation, maxDistRatio, d_groups),
          "cs_camera_grouping_dev")
