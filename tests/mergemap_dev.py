"""Device-side helpers of tests/test_mergemap_gpu.py, tests/test_mergemap_e2e_gpu.py, tests/test_mergemap_shim_gpu.py and tools/mergemap_time.py:
the live tables of a scene next to tests/mergeconstraints_dev.py's DeviceScene, one call of cs_merge_constraints_apply_map_dev, the handle's
buffers as bytes, and a scene with every table MergeCamGroups.run takes."""
import ctypes as C

import numpy as np

from tests import mergemap_ref as mref
from tests.mergeconstraints_ref import cam_ids_in_both_groups

SIGMA = 3.0   # the pixel error variance of the re-triangulation in these tests


def ref_static_pattern(S):
    """a planted refStatic table: every row another byte, so a moved row shows"""
    m, c = np.meshgrid(np.arange(S["nMap"]), np.arange(S["nC"]), indexing="ij")
    return ((m * 37 + c * 11 + 1) % 251).astype(np.uint8)


def with_tables(S):
    """S with the two tables the assembly does not take: pointFeat derived from the references, refStatic planted"""
    return dict(S, pointFeat=mref.point_feat(S), refStatic=ref_static_pattern(S))


class MapTables:
    """pointFeat / refStatic / counts in device memory; slot2map, featRef and M are the DeviceScene's own tensors"""

    def __init__(self, D, counts0=(0, 0, 0, 0, 0, 0)):
        import torch

        S = D.S
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(D.dev)  # noqa: E731
        self.D = D
        self.pointFeat, self.refStatic = t(np.asarray(S["pointFeat"], np.int32)), t(np.asarray(S["refStatic"], np.uint8))
        self.counts = t(np.asarray(counts0, np.int32))

    def apply(self, mc, apply_points=True, nMap=None, with_optional=True):
        D = self.D
        mc.apply_map([D.slot2map[c].data_ptr() for c in range(D.S["nC"])], self.pointFeat.data_ptr() if with_optional else None,
                     D.featRef.data_ptr(), self.refStatic.data_ptr() if with_optional else None, D.S["nMap"] if nMap is None else nMap,
                     D.M.data_ptr(), apply_points, self.counts.data_ptr() if with_optional else None)

    def download(self):
        import torch

        torch.cuda.synchronize()
        D = self.D
        n = lambda x: x.cpu().numpy().copy()  # noqa: E731
        return dict(slot2map=n(D.slot2map), featRef=n(D.featRef), refStatic=n(self.refStatic), pointFeat=n(self.pointFeat), M=n(D.M),
                    counts=n(self.counts).tolist())


TABLES = ("slot2map", "featRef", "refStatic", "pointFeat", "M")


def same_tables(got, want):
    """the device's tables against the restatement's, bit for bit"""
    for k in TABLES:
        w = np.ascontiguousarray(want[k]).astype(got[k].dtype).reshape(got[k].shape)
        assert got[k].tobytes() == w.tobytes(), (k, np.argwhere(got[k] != w)[:8].tolist())
    assert got["counts"] == [int(v) for v in want["counts"]], (got["counts"], want["counts"])


def handle_bytes(mc):
    """every buffer of the handle the map update reads or could touch, as bytes"""
    h, b = mc.header(), mc.buf
    d = mc._down
    nv, P, nO = max(h.nMergeViews, 0), max(h.P, 0), max(h.nObs, 0)
    parts = [bytes(h), d(b.views, 8 * nv, np.int32), d(b.pointMap, P, np.int32), d(b.pts, 3 * P, np.float64), d(b.solvedPts, 3 * P, np.float64),
             d(b.obsPtr, P + 1, np.int32), d(b.obsCam, nO, np.int32), d(b.obsXY, 2 * nO, np.float64), d(b.outlier, nO, np.int32),
             d(b.Rs, 9 * 32, np.float64), d(b.Ts, 3 * 32, np.float64), d(b.solvedRs, 9 * 32, np.float64), d(b.solvedTs, 3 * 32, np.float64),
             d(b.infoR, 9 * 48, np.float64), d(b.infoT, 3 * 48, np.float64)]
    return b"".join(p if isinstance(p, bytes) else p.tobytes() for p in parts)


def poke(dst_ptr, arr):
    """a host array to a device address of the handle (hand-made lists are a test's business: the library has no upload for them)"""
    import torch

    torch.cuda.synchronize()
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    arr = np.ascontiguousarray(arr)
    rc = C.CDLL(path).hipMemcpy(C.c_void_p(int(dst_ptr)), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1)
    assert rc == 0, rc
    return arr


class Live:
    """a scene in device memory with every table MergeCamGroups.run takes"""

    def __init__(self, S):
        import torch

        from tests.mergeconstraints_dev import DeviceScene

        self.S = S = with_tables(S)
        self.dev = dev = torch.device("cuda:0")
        self.D = D = DeviceScene(S, dev)
        nMap, nC = S["nMap"], S["nC"]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.pointFeat, self.refStatic = t(np.asarray(S["pointFeat"], np.int32)), t(np.asarray(S["refStatic"], np.uint8))
        self.cov = torch.zeros((nMap, 9), dtype=torch.float64, device=dev)
        f2 = S["frame0"] + S["nF"] - 1
        self.first, self.last = t(np.full(nMap, S["frame0"], np.int32)), t(np.full(nMap, f2, np.int32))
        self.flags = torch.zeros(nMap, dtype=torch.uint8, device=dev)
        self.cams = [dict(D.cams[c], iK=D.iK[c].data_ptr()) for c in range(nC)]
        self.tables = dict(cams=self.cams, featRef=D.featRef.data_ptr(), pointFeat=self.pointFeat.data_ptr(), refStatic=self.refStatic.data_ptr(),
                           nMap=nMap, mapPts=D.M.data_ptr(), mapCov=self.cov.data_ptr(), mapCount=None, firstFrame=self.first.data_ptr(),
                           lastFrame=self.last.data_ptr(), mapFlags=self.flags.data_ptr())
        self.ids = cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
        self.key_groups = [[sorted(c for g in S["groups"] for c in g)]] + [S["groups"]] * (len(S["key_frames"]) - 1)   # one group in the oldest
        self.pair = (S["gId1"], S["gId2"], S["maxiCam"], S["maxjCam"])

    def run(self, mg, **kw):
        S = self.S
        return mg.run(self.D.th, self.tables, S["groups"], S["key_frames"], S["self_motion"], self.key_groups, self.pair, S["matches"], SIGMA, **kw)

    def state(self):
        """history, map and tables as host arrays"""
        import torch

        torch.cuda.synchronize()
        out = self.D.snapshot()
        out.update(refStatic=self.refStatic.cpu().numpy(), pointFeat=self.pointFeat.cpu().numpy(), cov=self.cov.cpu().numpy())
        return out

    def close(self):
        self.D.th.close()
