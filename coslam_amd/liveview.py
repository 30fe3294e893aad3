"""ctypes mirror of cs_liveview_* / cs_map_counts_dev (include/coslam_hip.h): CoSLAM::getNumDynamicStaticPoints and
CoSLAM::storeDynamicPoints (reference src/app/SL_CoSLAM.cpp:1447-1471, :1900-1911) and the display's getDynTracks
(src/gui/GLScenePane.cpp:19-52) on the device -- per frame the counts, the dynamic points into a device ring, and on publishing frames a
snapshot (header + the current map points) into a ring in pinned host memory that a consumer reads when it wants."""
import ctypes as C

import numpy as np

from ._lib import CoslamHipError, check, lib
from .grouping import MAX_CAMS, CameraGroups


class MapCounts(C.Structure):
    """m_nStatic, m_nDynamic, m_nStaticFeat[], m_nDynamicFeat[]."""

    _c_type_ = "cs_map_counts"
    _fields_ = [("nStatic", C.c_int), ("nDynamic", C.c_int), ("nStaticFeat", C.c_int * MAX_CAMS), ("nDynamicFeat", C.c_int * MAX_CAMS)]

    def as_dict(self, nCams=MAX_CAMS):
        return dict(nStatic=int(self.nStatic), nDynamic=int(self.nDynamic), nStaticFeat=[int(x) for x in self.nStaticFeat[:nCams]],
                    nDynamicFeat=[int(x) for x in self.nDynamicFeat[:nCams]])


class LiveHeader(C.Structure):
    _c_type_ = "cs_live_header"
    _fields_ = [("frame", C.c_int), ("mapCount", C.c_int), ("nCur", C.c_int), ("nDyn", C.c_int), ("curOverflow", C.c_int),
                ("dynOverflow", C.c_int), ("nCams", C.c_int), ("every", C.c_int), ("counts", MapCounts), ("R", (C.c_double * 9) * MAX_CAMS),
                ("t", (C.c_double * 3) * MAX_CAMS), ("groups", CameraGroups), ("curOverflowTotal", C.c_int),
                ("dynOverflowTotal", C.c_int), ("reserved", C.c_int)]


LIVE_POINT_DTYPE = np.dtype([("M", "<f8", 3), ("id", "<i4"), ("camMask", "<u2"), ("flags", "u1"), ("numVisCam", "u1")])
LIVE_DYN_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("id", "<i4"), ("reserved", "<i4")])
C_RECORD_TYPES = {"LIVE_POINT_DTYPE": "cs_live_point", "LIVE_DYN_DTYPE": "cs_live_dyn"}   # numpy record types -> their C types (tests/test_abi.py)


def map_counts_scratch_bytes():
    """bytes of device scratch of map_counts_dev: zero it once before the first call, every call leaves it zeroed"""
    return int(lib().cs_map_counts_scratch_bytes())


def map_counts_dev(stream_ptr, nCams, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_counts, d_scratch, device=0):
    """cs_map_counts_dev: getNumDynamicStaticPoints alone into d_counts (a MapCounts in device memory); one launch, no wait."""
    check(lib().cs_map_counts_dev(int(device), stream_ptr, int(nCams), int(nMap), d_mapCount, d_pointFeat, d_mapFlags, d_counts, d_scratch),
          "cs_map_counts_dev")


class LiveView:
    """cs_liveview: the per-frame step and its two rings.  frame_dev() enqueues and never waits; newest() asks an event; snapshot() gives
    COPIES of a published frame's header and records; trails() is getDynTracks over the device ring."""

    def __init__(self, nCams, cur_cap, dyn_cap, depth=4, trail_depth=150, every=1, device=0):
        L = lib()
        self.nCams, self.cur_cap, self.dyn_cap, self.depth, self.trail_depth, self.every = nCams, cur_cap, dyn_cap, depth, trail_depth, every
        self.h = L.cs_liveview_create(int(device), int(nCams), int(cur_cap), int(dyn_cap), int(depth), int(trail_depth), int(every))
        if not self.h:
            raise CoslamHipError("cs_liveview_create failed: " + L.cs_last_error().decode("utf-8", "replace"))

    def close(self):
        if self.h:
            lib().cs_liveview_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frame_dev(self, stream_ptr, frame, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_mapPts, d_R, d_t, d_groups=None):
        check(lib().cs_liveview_frame_dev(self.h, stream_ptr, int(frame), int(nMap), d_mapCount, d_pointFeat, d_mapFlags, d_mapPts, d_R, d_t,
                                          d_groups), "cs_liveview_frame_dev")

    def newest(self):
        """the newest published frame that has landed on the host, or -1 (never waits)"""
        return int(lib().cs_liveview_newest(self.h))

    def fetch(self, frame):
        """(LiveHeader, records) as VIEWS of the pinned ring: valid until `depth` more snapshots have been published"""
        hp, pp = C.c_void_p(), C.c_void_p()
        check(lib().cs_liveview_fetch(self.h, int(frame), C.byref(hp), C.byref(pp)), "cs_liveview_fetch")
        hdr = LiveHeader.from_address(hp.value)
        n = max(0, min(int(hdr.nCur), self.cur_cap))
        buf = (C.c_char * (32 * self.cur_cap)).from_address(pp.value)
        return hdr, np.frombuffer(buf, dtype=LIVE_POINT_DTYPE, count=n)

    def snapshot(self, frame=None):
        """a published frame (None: the newest that has landed) as a dict of copies, or None when there is none yet"""
        if frame is None:
            frame = self.newest()
            if frame < 0:
                return None
        hdr, pts = self.fetch(frame)
        nC = self.nCams
        out = dict(frame=int(hdr.frame), mapCount=int(hdr.mapCount), nCur=int(hdr.nCur), nDyn=int(hdr.nDyn), curOverflow=int(hdr.curOverflow),
                   dynOverflow=int(hdr.dynOverflow), curOverflowTotal=int(hdr.curOverflowTotal), dynOverflowTotal=int(hdr.dynOverflowTotal), nCams=int(hdr.nCams), every=int(hdr.every), R=np.array(hdr.R, dtype=np.float64)[:nC].copy(),
                   t=np.array(hdr.t, dtype=np.float64)[:nC].copy(), groups=CameraGroups.from_bytes(bytes(hdr.groups)).groups(),
                   points=pts.copy())
        out.update(hdr.counts.as_dict(nC))
        return out

    def rings(self):
        """dict(h_ring, slot_bytes, d_entries, d_counts, d_frames): addresses of the pinned ring and of the device ring of dynamic lists"""
        a, b, c, d, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        check(lib().cs_liveview_rings(self.h, C.byref(a), C.byref(n), C.byref(b), C.byref(c), C.byref(d)), "cs_liveview_rings")
        return dict(h_ring=a.value, slot_bytes=int(n.value), d_entries=b.value, d_counts=c.value, d_frames=d.value)

    def ring_bytes(self):
        """a copy of the whole pinned ring (tests: what a call left untouched)"""
        r = self.rings()
        return bytes((C.c_char * (r["slot_bytes"] * self.depth)).from_address(r["h_ring"]))

    def dyn_list(self, stream_ptr, frames_back=0):
        """(frame, entries as LIVE_DYN_DTYPE) of the dynamic list `frames_back` calls before the newest (waits for the stream)"""
        n, f = C.c_int(0), C.c_int(-1)
        out = np.zeros(self.dyn_cap, dtype=LIVE_DYN_DTYPE)
        check(lib().cs_liveview_dyn_fetch(self.h, stream_ptr, int(frames_back), self.dyn_cap, out.ctypes.data, C.byref(n), C.byref(f)),
              "cs_liveview_dyn_fetch")
        return int(f.value), out[:max(0, min(int(n.value), self.dyn_cap))].copy()

    def trails_dev(self, stream_ptr, trj_len, d_nTrails, d_trailId, d_trailLen, d_trailPts):
        check(lib().cs_liveview_trails_dev(self.h, stream_ptr, int(trj_len), d_nTrails, d_trailId, d_trailLen, d_trailPts),
              "cs_liveview_trails_dev")

    def trails(self, stream_ptr, trj_len, max_trails=None):
        """getDynTracks: [(id, [[x, y, z], ...] newest first), ...] in ascending id order (waits for the stream)"""
        cap = self.dyn_cap if max_trails is None else int(max_trails)
        n = C.c_int(0)
        ids, lens = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        pts = np.zeros((max(cap, 1), max(int(trj_len), 1), 3), np.float64)
        check(lib().cs_liveview_trails(self.h, stream_ptr, int(trj_len), cap, C.byref(n), ids.ctypes.data, lens.ctypes.data, pts.ctypes.data),
              "cs_liveview_trails")
        k = min(int(n.value), cap)
        return [(int(ids[q]), pts[q, :int(lens[q])].copy()) for q in range(k)]
