"""tests/golden/mergegraph_golden.npz from the reference's own computeNewCameraRotations + computeNewCameraTranslations4
(oracle/_ref/ref_mergegraph_test golden; the driver: tests/cxx/ref_mergegraph_test.cpp; tests/golden/fixtures.py lists the maker).  Data only.
Flat arrays as in posegraph_golden.npz: graph g owns nodes [node_ptr[g], node_ptr[g+1]) and edges [edge_ptr[g],
edge_ptr[g+1]); id1 / id2 are local to the graph; scale_id < 0 is a plain edge; edgeS is CamPoseEdge::s."""
import struct

import numpy as np

from tests.golden.fixtures import driver_output

NAMES = ["merge_2x3", "merge_3x4", "merge_8x6", "merge_16x4", "merge_8x24", "two_scales", "shared_scale", "fixed_id2", "fixed_id1"]


def mergegraph_case():
    raw = driver_output("ref_mergegraph_test", "golden")
    ng, _ = struct.unpack_from("ii", raw, 0)
    assert ng == len(NAMES)
    o = 8
    node_ptr, edge_ptr, n_fixed, n_constraint = [0], [0], [], []
    fixed, ncons, frame, cam, R, t, nR, nt = [], [], [], [], [], [], [], []
    id1, id2, sid, econs, eR, eT, eS = [], [], [], [], [], [], []
    for _g in range(ng):
        n, e, nf, nc = struct.unpack_from("iiii", raw, o)
        o += 16
        n_fixed.append(nf), n_constraint.append(nc)
        for _i in range(n):
            a = struct.unpack_from("iiii", raw, o)
            v = np.frombuffer(raw, np.float64, 24, o + 16)
            o += 16 + 192
            fixed.append(a[0]), ncons.append(a[1]), frame.append(a[2]), cam.append(a[3])
            R.append(v[:9]), t.append(v[9:12]), nR.append(v[12:21]), nt.append(v[21:24])
        for _k in range(e):
            a = struct.unpack_from("iiii", raw, o)
            v = np.frombuffer(raw, np.float64, 13, o + 16)
            o += 16 + 104
            id1.append(a[0]), id2.append(a[1]), sid.append(a[2]), econs.append(a[3])
            eR.append(v[:9]), eT.append(v[9:12]), eS.append(v[12])
        node_ptr.append(node_ptr[-1] + n), edge_ptr.append(edge_ptr[-1] + e)
    assert o == len(raw)
    i32 = lambda v: np.array(v, np.int32)  # noqa: E731
    return dict(names=np.array(NAMES), node_ptr=i32(node_ptr), edge_ptr=i32(edge_ptr), n_fixed=i32(n_fixed), n_constraint=i32(n_constraint),
                fixed=np.array(fixed, np.uint8), node_constraint=np.array(ncons, np.uint8), frame=i32(frame), cam=i32(cam),
                nodeR=np.array(R), nodeT=np.array(t), newR=np.array(nR), newT=np.array(nt), id1=i32(id1), id2=i32(id2),
                scale_id=i32(sid), edge_constraint=np.array(econs, np.uint8), edgeR=np.array(eR), edgeT=np.array(eT), edgeS=np.array(eS))
