"""cs_posegraph_*_scaled (pose graphs with shared-scale constraint edges: computeNewCameraRotations +
computeNewCameraTranslations4, reference src/slam/SL_GlobalPoseEstimation.cpp:52-219, 361-525) against the reference's own
outputs (tests/golden/mergegraph_golden.npz) and the numpy restatement (tests/mergegraph_ref.py), and MergePoseCorrection.

Tolerance: TOL_R / TOL_T of tests/test_posegraph_gpu.py, by the same argument: the reference factorises the over-determined
system with a QR, the kernel its normal equations (L D L^T of the node matrix, then the Schur complement of the scales); the
golden systems have full column rank (asserted in tests/test_mergegraph_cpu.py) and cond(A^T A) <= 1.3e4.  The scales are
unknowns of the translation system: TOL_T."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import coslam_amd
import oracle
from coslam_amd._lib import check
from coslam_amd.synth import make_merge_pose_graph, make_pose_graphs
from tests import mergegraph_ref as ref
from tests.cxx_build import build_shim_test
from tests.test_mergegraph_cpu import golden_graphs

pytestmark = pytest.mark.gpu

TOL_R, TOL_T = 1e-10, 1e-9
INVALID, NUMERIC = -1, -5


def _handle(ds):
    return coslam_amd.PoseGraphs([(d["fixed"], d["id1"], d["id2"]) for d in ds], scale_ids=[d["scale_id"] for d in ds])


def _cat(ds, key):
    return np.concatenate([d[key] for d in ds])


@pytest.fixture(scope="module")
def gold():
    return golden_graphs()


def test_every_golden_graph_in_one_launch(hip, gold):
    h = _handle(gold)
    newR, newT, edgeS = h.relax(_cat(gold, "nodeR"), _cat(gold, "nodeT"), _cat(gold, "edgeR"), _cat(gold, "edgeT"))
    wR, wT, wS = _cat(gold, "newR"), _cat(gold, "newT"), _cat(gold, "edgeS")
    n0 = e0 = 0
    for d in gold:
        ns, es = slice(n0, n0 + len(d["fixed"])), slice(e0, e0 + len(d["id1"]))
        n0, e0 = ns.stop, es.stop
        print(f"{d['name']}: |dR| {np.abs(newR[ns] - wR[ns]).max():.2e} |dt| {np.abs(newT[ns] - wT[ns]).max():.2e} "
              f"|ds| {np.abs(edgeS[es] - wS[es]).max():.2e}")
    assert np.abs(newR - wR).max() < TOL_R and np.abs(newT - wT).max() < TOL_T and np.abs(edgeS - wS).max() < TOL_T
    fx = _cat(gold, "fixed") != 0
    assert np.array_equal(newR[fx], _cat(gold, "nodeR")[fx]) and np.array_equal(newT[fx], _cat(gold, "nodeT")[fx])   # bit for bit
    for q in newR[~fx]:
        Q = q.reshape(3, 3)
        assert np.abs(Q @ Q.T - np.eye(3)).max() < 1e-14 and np.linalg.det(Q) > 0.999
    e0 = 0
    for d in gold:
        s = edgeS[e0:e0 + len(d["id1"])]
        e0 += len(d["id1"])
        assert np.all(s[d["scale_id"] < 0] == 0)
        for i in set(d["scale_id"][d["scale_id"] >= 0]):
            assert len(set(s[d["scale_id"] == i])) == 1 and s[d["scale_id"] == i][0] != 0    # equal on the edges that share an id
    h.close()


@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (3, 4, 2, 1), (8, 6, 3, 4)])
def test_synthetic_merge_graphs_match_the_restatement(hip, shape):
    m = make_merge_pose_graph(*shape, seed=11)
    h = _handle([m])
    out = h.relax(m["nodeR"], m["nodeT"], m["edgeR"], m["edgeT"])
    wR, wT, wS, A = ref.relax_scaled(m["fixed"], m["nodeR"], m["nodeT"], m["id1"], m["id2"], m["edgeR"], m["edgeT"], m["scale_id"])
    assert np.linalg.matrix_rank(A) == A.shape[1]
    d = [np.abs(a - b).max() for a, b in zip(out, (wR, wT, wS))]
    print(f"{shape}: {h.counts()} {h.scaled_counts()} |dR| {d[0]:.2e} |dt| {d[1]:.2e} |ds| {d[2]:.2e}")
    assert d[0] < TOL_R and d[1] < TOL_T and d[2] < TOL_T
    drift = m["node_cam"] >= shape[3]
    assert np.abs(out[1] - m["nodeT"])[drift].max() > 1e-2                    # the drifted group was pulled back
    again = h.relax(m["nodeR"], m["nodeT"], m["edgeR"], m["edgeT"])           # no atomics, fixed summation order
    assert all(np.array_equal(a, b) for a, b in zip(out, again))
    h.close()


def test_plain_graphs_in_a_scaled_handle_give_the_plain_handles_bits(hip, gold):
    pg = make_pose_graphs(n_cams=3, n_frames=21, key_every=5, seed=4, loop_edges=3)
    m = gold[2]
    graphs = [pg["graphs"][0], (m["fixed"], m["id1"], m["id2"])] + pg["graphs"][1:]
    sids = [None, m["scale_id"], None, None]
    n1, e1 = pg["node_ptr"][1], pg["edge_ptr"][1]
    ins = lambda a, b, cut: np.concatenate([a[:cut], b, a[cut:]])  # noqa: E731
    h = coslam_amd.PoseGraphs(graphs, scale_ids=sids)
    newR, newT, edgeS = h.relax(ins(pg["nodeR"], m["nodeR"], n1), ins(pg["nodeT"], m["nodeT"], n1), ins(pg["edgeR"], m["edgeR"], e1),
                                ins(pg["edgeT"], m["edgeT"], e1))
    p = coslam_amd.PoseGraphs(pg["graphs"])
    pR, pT = p.relax(pg["nodeR"], pg["nodeT"], pg["edgeR"], pg["edgeT"])
    nm = len(m["fixed"])
    assert np.array_equal(np.delete(newR, slice(n1, n1 + nm), 0), pR) and np.array_equal(np.delete(newT, slice(n1, n1 + nm), 0), pT)
    assert np.abs(newR[n1:n1 + nm] - m["newR"]).max() < TOL_R and np.abs(newT[n1:n1 + nm] - m["newT"]).max() < TOL_T
    assert h.counts()["components"] == p.counts()["components"] + 1
    # scale_ids given but no scaled edge at all: the plain handle's bits again
    q = coslam_amd.PoseGraphs(pg["graphs"], scale_ids=[None] * 3)
    qR, qT, qS = q.relax(pg["nodeR"], pg["nodeT"], pg["edgeR"], pg["edgeT"])
    assert np.array_equal(qR, pR) and np.array_equal(qT, pT) and not qS.any()
    for x in (h, p, q):
        x.close()


def test_scaled_counts(hip, gold):
    by = {d["name"]: d for d in gold}
    h = _handle([by["merge_8x24"]])
    c = h.scaled_counts()
    print(h.counts(), c)
    assert c["scales"] == 1 and c["max_interior_half_bandwidth"] <= 3 * 8 + 2 and 0 < c["border_nodes"] <= 16
    assert h.counts()["components"] == 1
    h.close()
    d = by["shared_scale"]
    h = _handle([d])
    plain = coslam_amd.PoseGraphs([(d["fixed"], d["id1"], d["id2"])])
    assert plain.counts()["components"] == 2 and h.counts()["components"] == 1 and h.scaled_counts()["scales"] == 1
    h.close(), plain.close()
    h = _handle([by["two_scales"]])
    assert h.scaled_counts()["scales"] == 2
    h.close()


def test_edges_dev_leaves_constraint_rows_as_written(hip, gold):
    import torch

    d = gold[1]
    h = _handle([d])
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    nR, nT = t(d["nodeR"]), t(d["nodeT"])
    eR, eT = torch.full((len(d["id1"]), 9), 7.5, dtype=torch.float64, device=dev), torch.full((len(d["id1"]), 3), -2.5, dtype=torch.float64, device=dev)
    h.edges_dev(torch.cuda.current_stream().cuda_stream, nR.data_ptr(), nT.data_ptr(), eR.data_ptr(), eT.data_ptr())
    torch.cuda.synchronize()
    eR, eT = eR.cpu().numpy(), eT.cpu().numpy()
    sc = d["scale_id"] >= 0
    assert np.all(eR[sc] == 7.5) and np.all(eT[sc] == -2.5)
    assert np.abs(eR[~sc] - d["edgeR"][~sc]).max() < 1e-14 and np.abs(eT[~sc] - d["edgeT"][~sc]).max() < 1e-13   # getRigidTransFromTo
    h.close()


def _create_rc(graphs, sids):
    try:
        coslam_amd.PoseGraphs(graphs, scale_ids=sids).close()
    except coslam_amd.CoslamHipError as e:
        return str(e)
    return None


def test_refusals_at_create(hip):
    chain = lambda n: (np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32))  # noqa: E731
    fixed = np.array([1, 0, 0, 0, 0, 1], np.uint8)
    id1, id2 = chain(6)
    ok = [-1, 0, -1, 0, -1]
    assert _create_rc([(fixed, id1, id2)], [ok]) is None
    msg = _create_rc([(fixed, id1, id2)], [[-1, 5, -1, -1, -1]])               # id >= the graph's edge count
    assert msg and f"code {INVALID}" in msg and "scale id 5" in msg
    id1b, id2b = np.append(id1, 0).astype(np.int32), np.append(id2, 5).astype(np.int32)
    msg = _create_rc([(fixed, id1b, id2b)], [[-1, 0, -1, -1, -1, 2]])          # id 2: only the fixed-fixed edge 0 -> 5
    assert msg and f"code {INVALID}" in msg and "fixed nodes only" in msg
    n = 12
    f12 = np.zeros(n, np.uint8)
    f12[0] = 1
    a, b = chain(n)
    msg = _create_rc([(f12, a, b)], [[0, 1, 2, 3, 4, -1, -1, -1, -1, -1, -1]])  # five scales in one component (the cap is 4)
    assert msg and f"code {INVALID}" in msg and "at most 4" in msg
    assert _create_rc([(f12, a, b)], [[0, 1, 2, 3, -1, -1, -1, -1, -1, -1, -1]]) is None
    # a scaled handle does not go through the plain relax
    h = coslam_amd.PoseGraphs([(fixed, id1, id2)], scale_ids=[ok])
    z = np.zeros
    with pytest.raises(coslam_amd.CoslamHipError, match="relax_scaled"):
        check(coslam_amd.lib().cs_posegraph_relax(h._h, *[x.ctypes.data_as(C.c_void_p) for x in
                                                          (z((6, 9)), z((6, 3)), z((5, 9)), z((5, 3)), z((6, 9)), z((6, 3)))]),
              "cs_posegraph_relax")
    h.close()


def test_undetermined_scale_fails_its_graph_only(hip, gold):
    bad = dict(gold[0])
    bad["edgeT"] = bad["edgeT"].copy()
    bad["edgeT"][bad["scale_id"] >= 0] = 0.0                                   # every edge of the scale has t = 0: a zero column
    ds = [gold[1], bad, gold[5]]
    h = _handle(ds)
    with pytest.raises(coslam_amd.CoslamHipError) as ei:
        h.relax(_cat(ds, "nodeR"), _cat(ds, "nodeT"), _cat(ds, "edgeR"), _cat(ds, "edgeT"))
    assert f"code {NUMERIC}" in str(ei.value) and "graph 1" in str(ei.value) and "scale" in str(ei.value)
    # the launch's other graphs were solved: read them back through the device form
    import torch

    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    ins = [t(_cat(ds, k)) for k in ("nodeR", "nodeT", "edgeR", "edgeT")]
    outs = [torch.zeros_like(ins[0]), torch.zeros_like(ins[1]), torch.zeros(len(ins[2]), dtype=torch.float64, device=dev)]
    s = torch.cuda.current_stream().cuda_stream
    h.relax_scaled_dev(s, *[x.data_ptr() for x in ins + outs])
    nf, first = C.c_int(), C.c_int()
    rc = coslam_amd.lib().cs_posegraph_status(h._h, C.c_void_p(s), C.byref(nf),
                                              C.byref(first))
    assert rc == NUMERIC and nf.value == 1 and first.value == 1
    newR, newT = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    n1, n2 = len(ds[0]["fixed"]), len(ds[0]["fixed"]) + len(ds[1]["fixed"])
    for sl, d in ((slice(0, n1), ds[0]), (slice(n2, None), ds[2])):
        assert np.abs(newR[sl] - d["newR"]).max() < TOL_R and np.abs(newT[sl] - d["newT"]).max() < TOL_T
    assert np.all(np.isfinite(newR)) and np.all(np.isfinite(newT))
    h.close()


def test_merge_pose_correction(hip):
    """2 cameras x 3 key frames x 5 frames per interval: key graph -> corrected key poses into the chains' fixed nodes -> chains"""
    m = make_merge_pose_graph(2, 3, 1, 1, seed=5, frames_per_interval=5)
    ch = m["chains"]
    plan = coslam_amd.merge_keygraph_plan(m["frames"], m["groups"], m["cam_ids"], m["first_constrain"], m["camid1"], m["camid2"], m["infos"])
    assert plan["fixed_kf"] == 0 and np.array_equal(plan["id1"], m["id1"]) and np.array_equal(plan["scale_id"], m["scale_id"])
    mc = coslam_amd.MergePoseCorrection((plan["fixed"], plan["id1"], plan["id2"], plan["scale_id"]), ch["graphs"], ch["key_node"])
    sc = m["scale_id"] >= 0
    out = mc.run(m["nodeR"], m["nodeT"], m["edgeR"][sc], m["edgeT"][sc], ch["nodeR"], ch["nodeT"])
    wR, wT, wS, _A = ref.relax_scaled(m["fixed"], m["nodeR"], m["nodeT"], m["id1"], m["id2"], m["edgeR"], m["edgeT"], m["scale_id"])
    assert np.abs(out["keyR"] - wR).max() < TOL_R and np.abs(out["keyT"] - wT).max() < TOL_T and np.abs(out["edgeS"] - wS).max() < TOL_T
    # the chains: the oracle's relaxation with those key poses held (edges from the poses BEFORE the correction)
    cR, cT = ch["nodeR"].copy(), ch["nodeT"].copy()
    cR[ch["key_node"]], cT[ch["key_node"]] = wR, wT
    for c, (fixed, id1, id2) in enumerate(ch["graphs"]):
        ns = slice(ch["node_ptr"][c], ch["node_ptr"][c + 1])
        R0, T0 = ch["nodeR"][ns].reshape(-1, 3, 3), ch["nodeT"][ns]
        eR = np.einsum("eij,ekj->eik", R0[id2], R0[id1])
        eT = T0[id2] - np.einsum("eij,ej->ei", eR, T0[id1])
        rc, oR, oT = oracle.posegraph_relax(fixed, cR[ns], cT[ns], id1, id2, eR.reshape(-1, 9), eT)
        assert rc == 0
        assert np.abs(out["chainR"][ns] - oR).max() < TOL_R and np.abs(out["chainT"][ns] - oT).max() < TOL_T
        moved = np.abs(out["chainT"][ns] - ch["nodeT"][ns]).max(axis=1)
        if c == 1:                                                           # the drifted camera: its non-key frames moved
            assert moved[fixed == 0][-4:].min() > 1e-3
    mc.close()


def test_cxx_shim_relax_scaled_pose_graph(hip, gold, tmp_path):
    d = gold[0]
    exe = build_shim_test("mergegraph_shim_test.cpp", tmp_path, hip_runtime=False)
    n, e = len(d["fixed"]), len(d["id1"])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("ii", n, e))
        for i in range(n):
            f.write(struct.pack("i", int(d["fixed"][i])) + d["nodeR"][i].tobytes() + d["nodeT"][i].tobytes())
        for k in range(e):
            f.write(struct.pack("iii", int(d["id1"][k]), int(d["id2"][k]), int(d["scale_id"][k])) + d["edgeR"][k].tobytes() + d["edgeT"][k].tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    v = np.frombuffer(raw, np.float64, 12 * n + e)
    pose = v[:12 * n].reshape(n, 12)
    assert np.abs(pose[:, :9] - d["newR"]).max() < TOL_R and np.abs(pose[:, 9:] - d["newT"]).max() < TOL_T
    assert np.abs(v[12 * n:] - d["edgeS"]).max() < TOL_T
    assert struct.unpack_from("i", raw, 8 * (12 * n + e))[0] == 1            # relaxPoseGraphs still refuses the graph
