"""SURF key points and descriptors on the device: ::detectSURFPoints of mergeCamGroups, the images' way into the merge
chain (Surf.front_cams -> MergeFront.run / MergeCamGroups.run_from_descriptors)."""
import ctypes as C

from ._lib import check
from .merge import _MergeHandle

SURF_MAX_OCTAVES, SURF_MAX_LAYERS = 5, 6


class SurfBuffers(C.Structure):
    _c_type_ = "cs_surf_buffers"
    _NL = SURF_MAX_OCTAVES * SURF_MAX_LAYERS
    _fields_ = [(n, C.c_void_p) for n in ("pts", "desc", "size", "angle", "response", "laplacian", "octave", "layer", "cell", "count", "overflow",
                                          "integral", "det", "lap")] + \
               [(n, C.c_int) for n in ("nCams", "W", "H", "maxPts", "nOctaves", "nOctaveLayers", "dimDesc", "mapElems")] + \
               [("mapW", C.c_int * SURF_MAX_OCTAVES), ("mapH", C.c_int * SURF_MAX_OCTAVES), ("mapOff", C.c_int * _NL),
                ("layerSize", C.c_int * _NL), ("layerFits", C.c_int * _NL)]


class Surf(_MergeHandle):
    """cs_surf: integral image -> fast-Hessian layers -> maxima in ascending (octave, layer, row, column) -> orientation -> descriptors, for
    all cameras of a call in each launch.  keep="strongest": a camera with more than max_pts maxima keeps those of the largest response
    (still in ascending order) instead of the first max_pts.  Rows beyond a camera's count hold NaN key points and zero descriptors, so front_cams() hands
    {pts, desc, n = max_pts} on with no wait."""

    _prefix, _Buffers = "cs_surf", SurfBuffers

    KEEP = {"first": 0, "strongest": 1}   # CS_SURF_KEEP_FIRST, CS_SURF_KEEP_STRONGEST

    def __init__(self, n_cams, W, H, max_pts, n_octaves=4, n_octave_layers=2, dim_desc=64, device=0, keep="first"):
        if keep not in self.KEEP:
            raise ValueError(f"Surf: keep is 'first' or 'strongest', not {keep!r}")
        self.n_cams, self.W, self.H, self.max_pts = int(n_cams), int(W), int(H), int(max_pts)
        self.n_octaves, self.n_layers, self.dim = int(n_octaves), int(n_octave_layers), int(dim_desc)
        self._create(device, self.n_cams, self.W, self.H, self.max_pts, self.n_octaves, self.n_layers, self.dim)
        self.keep = keep
        if keep != "first":   # beyond max_pts: the strongest responses instead of the first of the list
            check(self._L.cs_surf_keep_set(self._m, self.KEEP[keep]), "cs_surf_keep_set")

    def _table(self, images):
        """images: per camera a device pointer (int), a torch uint8 tensor, or None (camera skipped) -> the host pointer table"""
        if len(images) != self.n_cams:
            raise ValueError(f"Surf: {len(images)} images, the handle has {self.n_cams} cameras")
        ptrs = [None if im is None else (int(im) if isinstance(im, int) else int(im.data_ptr())) for im in images]
        return (C.c_void_p * self.n_cams)(*ptrs)

    def enqueue(self, images, threshold, upright=False, pitch=None, stream_ptr=None):
        """cs_surf_run_dev.  Enqueues only."""
        check(self._L.cs_surf_run_dev(self._m, self._stream(stream_ptr), self._table(images), self.W if pitch is None else int(pitch),
                                      float(threshold), 1 if upright else 0), "cs_surf_run_dev")

    def integral(self, images, pitch=None, stream_ptr=None):
        """cs_surf_integral_dev: the integral images alone.  Enqueues only."""
        check(self._L.cs_surf_integral_dev(self._m, self._stream(stream_ptr), self._table(images), self.W if pitch is None else int(pitch)),
              "cs_surf_integral_dev")

    def layers(self, images, pitch=None, stream_ptr=None):
        """cs_surf_layers_dev: the integral images and the layer maps.  Enqueues only."""
        check(self._L.cs_surf_layers_dev(self._m, self._stream(stream_ptr), self._table(images), self.W if pitch is None else int(pitch)),
              "cs_surf_layers_dev")

    def detect(self, images, threshold, pitch=None, stream_ptr=None):
        """cs_surf_detect_dev: integral images, layer maps and key-point lists.  Enqueues only."""
        check(self._L.cs_surf_detect_dev(self._m, self._stream(stream_ptr), self._table(images), self.W if pitch is None else int(pitch),
                                         float(threshold)), "cs_surf_detect_dev")

    def counts(self, stream_ptr=None):
        """cs_surf_counts: the stage's one host wait -> (count int32 [n_cams], overflow int32 [n_cams])"""
        import numpy as np

        cnt, ovf = np.zeros(self.n_cams, np.int32), np.zeros(self.n_cams, np.int32)
        check(self._L.cs_surf_counts(self._m, self._stream(stream_ptr), cnt.ctypes.data, ovf.ctypes.data), "cs_surf_counts")
        return cnt, ovf

    def rows(self, c, n, stream_ptr=None):
        """the first n rows of camera c's key-point arrays -> dict of numpy arrays; waits"""
        import numpy as np

        b, at, n = self.buf, int(c) * self.max_pts, int(n)
        if not 0 <= int(c) < self.n_cams or not 0 <= n <= self.max_pts:
            raise ValueError("Surf.rows: camera or row count out of range")
        down = lambda p, per, dt, size: self._down(int(p) + at * per * size, n * per, dt, stream_ptr)   # noqa: E731
        return dict(pts=down(b.pts, 2, np.float64, 8).reshape(-1, 2), desc=down(b.desc, self.dim, np.float32, 4).reshape(-1, self.dim),
                    size=down(b.size, 1, np.float64, 8), angle=down(b.angle, 1, np.float64, 8), response=down(b.response, 1, np.float64, 8),
                    laplacian=down(b.laplacian, 1, np.uint8, 1), octave=down(b.octave, 1, np.int32, 4), layer=down(b.layer, 1, np.int32, 4),
                    cell=down(b.cell, 2, np.int32, 4).reshape(-1, 2))

    def keypoints(self, c, stream_ptr=None):
        """the key points of camera c: the first count rows; waits"""
        return self.rows(c, self.counts(stream_ptr)[0][int(c)], stream_ptr)

    def integral_image(self, c, stream_ptr=None):
        import numpy as np

        n = (self.H + 1) * (self.W + 1)
        return self._down(int(self.buf.integral) + 4 * n * int(c), n, np.uint32, stream_ptr).reshape(self.H + 1, self.W + 1)

    def layer_map(self, c, o, l, stream_ptr=None):
        """-> (det f64 [mapH][mapW], laplacian u8) of layer l of octave o of camera c; waits"""
        import numpy as np

        off = self.buf.mapOff[o * SURF_MAX_LAYERS + l]
        if off < 0:
            raise ValueError(f"Surf.layer_map: no layer {l} of octave {o}")
        mh, mw = self.buf.mapH[o], self.buf.mapW[o]
        at = int(c) * self.buf.mapElems + off
        return self._down(int(self.buf.det) + 8 * at, mh * mw, np.float64, stream_ptr).reshape(mh, mw), \
            self._down(int(self.buf.lap) + at, mh * mw, np.uint8, stream_ptr).reshape(mh, mw)

    def front_cams(self, Ks, counts=None):
        """-> the camera list MergeFront.run / MergeCamGroups.run_from_descriptors take: pts / desc device pointers, n = max_pts (the
        padding rows are NaN: the front's `valid` rule drops them), no wait; counts: n = counts[c] instead (the caller has waited)"""
        if len(Ks) != self.n_cams:
            raise ValueError("Surf.front_cams: one K per camera")
        return [dict(pts=int(self.buf.pts) + 16 * self.max_pts * c, desc=int(self.buf.desc) + 4 * self.dim * self.max_pts * c,
                     n=self.max_pts if counts is None else int(counts[c]), K=Ks[c]) for c in range(self.n_cams)]
