"""cs_recompute_map_points_keyfrms_dev, cs_merge_apply_* and the sequence run -> recompute -> merge_matched_groups on the device
against the reference's own function (tests/golden/mergeapply_golden.npz), the restatement (tests/mergeapply_ref.py) bit for bit, and the
host-fed pose correction (MergePoseCorrection: the same kernels on the same inputs, bit for bit).

Every history is created with histLen = 16 over a store that holds the whole run: the nodes the walks choose lie beyond histLen, where the
bounded walks of cs_refine_map_points_ref_dev stop."""
import numpy as np
import pytest

import coslam_amd
from coslam_amd.synth import make_merge_pose_graph
from tests import mergeapply_e2e as e2e
from tests import mergeapply_planted as planted
from tests import mergeapply_ref as ref
from tests.cxx_build import build_shim_test
from tests.mergeapply_dev import load_history, recompute_dev, recompute_ref
from tests.mergeapply_golden_util import GOLDEN, inv_k, scene

pytestmark = pytest.mark.gpu

INVALID, NUMERIC = -1, -5
TOL_R, TOL_T = 1e-10, 1e-9    # DESIGN 3.20's


def _dev():
    import torch

    return torch.device("cuda:0")


def _check(S, dev, **kw):
    """device against restatement, bit for bit; returns (M, cov, counts, detail)"""
    store = kw.pop("store_len", None)
    pool_rows = kw.pop("pool_rows", None)
    seg_cap = kw.pop("seg_cap", None)
    th, cams, _keep = load_history(S, dev, store_len=store, pool_rows=pool_rows)
    if pool_rows is not None:
        S = dict(S, segPool=pool_rows)
    det = {}
    M, cov, cnt = recompute_dev(th, cams, S, dev, **kw)
    wM, wcov, wcnt = recompute_ref(S, ref, store_len=store, seg_cap=seg_cap, detail=det, **kw)
    th.close()
    assert cnt == wcnt, (cnt, wcnt)
    assert np.array_equal(M, wM) and np.array_equal(cov, wcov), f"max |dM| {np.abs(M - wM).max():.3e}"
    return M, cov, cnt, det


def test_golden_scenes_reproduce_the_reference(hip):
    """the four scenes of the reference's own updateStaticPointPositionAtKeyFrms on getMapPts' rows: M and cov bit for bit, the counters the
    restatement's, updateCov = 0 leaves cov alone, and the bounded all-frames walk of cs_refine_map_points_ref_dev gives other points"""
    import torch

    g = np.load(GOLDEN)
    dev = _dev()
    n_filter = 0
    for sc in range(int(g["n_scenes"])):
        S = scene(g, sc)
        th, cams, _keep = load_history(S, dev)
        M, cov, cnt = recompute_dev(th, cams, S, dev)
        _wM, _wcov, wcnt = recompute_ref(S, ref)
        moved = (S["M_ref"] != S["M0"]).any(axis=1)
        print(f"scene {sc}: counts {cnt}, {int(moved.sum())} moved, max |dM| {np.abs(M - S['M_ref']).max():.3e}")
        assert np.array_equal(M, S["M_ref"]) and np.array_equal(cov, S["cov_ref"]), sc
        assert cnt == wcnt and cnt[0] == int(S["selected"].sum()) and cnt[1] == int(moved.sum())
        M2, cov2, cnt2 = recompute_dev(th, cams, S, dev, update_cov=False)
        assert np.array_equal(M2, S["M_ref"]) and np.array_equal(cov2, S["cov0"]) and cnt2 == cnt
        # the existing refinement over the same rows: all nodes of at most histLen = 16, no head test
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_ref, d_M, d_cov = t(S["featRef"]), t(S["M0"].copy()), t(S["cov0"].copy())
        d_sel = t(S["selected"].astype(np.uint8))
        th.refine_map_points_ref_dev(torch.cuda.current_stream().cuda_stream, cams, d_ref.data_ptr(), len(S["M0"]), d_M.data_ptr(), d_cov.data_ptr(),
                                     S["sigma"], d_select=d_sel.data_ptr())
        torch.cuda.synchronize()
        fp = S["filter_points"].astype(np.int64)
        n_filter += int((d_M.cpu().numpy()[fp] != S["M_ref"][fp]).any(axis=1).sum())
        th.close()
    assert n_filter >= 30, n_filter


def test_block_edges_of_a_walk(hip):
    """runs of 63 / 64 / 65 / 128 / 129 key-frame nodes, the widest angle planted at walk positions 0, 63, 64 and last"""
    S, want = planted.block_edges()
    _M, _cov, cnt, det = _check(S, _dev())
    assert cnt == [4, 4, 0, 0]
    for p in range(4):
        for c, n in enumerate(planted.RUNS):
            assert det[p]["walks"][c]["node"][1] == want[p][c] and len(det[p]["walks"][c]["nodes"]) == n


def test_equal_maxima_the_newest_wins(hip):
    S, want = planted.equal_maxima()
    _M, _cov, cnt, det = _check(S, _dev())
    assert cnt == [1, 1, 0, 0] and [det[0]["walks"][c]["node"][1] for c in range(3)] == want[0]
    for c in range(3):    # the tie is real: two nodes share the smallest cosine bit for bit
        cs = sorted(v for _, _, v in det[0]["walks"][c]["nodes"])
        assert cs[0] == cs[1]


def test_no_key_frames_nothing_written(hip):
    S = planted.many_cameras(3)
    M, cov, cnt, _ = _check(S, _dev(), key_frames=np.zeros(0, np.int32))
    assert cnt == [6, 0, 6, 0] and np.array_equal(M, S["M0"]) and np.array_equal(cov, S["cov0"])


def test_chain_whose_older_half_left_the_store(hip):
    S = planted.many_cameras(3)          # 40 frames, chains from frame0 + 2..6 to the head two frames back
    M, _cov, cnt, det = _check(S, _dev(), store_len=20)
    assert cnt[0] == 6 and cnt[1] == 6 and cnt[3] == 18            # every walk cut, the newer half used
    assert all(f >= S["frame0"] + 20 for p in det for _c, f, _s in det[p]["views"])
    assert not np.array_equal(M, recompute_ref(S, ref)[0])         # (the whole chain gives other views)


def test_corrupt_pools_end_the_walk(hip):
    """a segment index >= the pool's capacity and a two-segment cycle: the hop guard ends the walk, nothing faults, the counter says so"""
    S, _want = planted.equal_maxima()
    dev = _dev()
    th, _cams, _keep = load_history(S, dev)
    seg_cap = th.segment_counts()[1]
    th.close()
    pool = np.full((3, 2, 4), -1, np.int32)
    pool[:, :1] = S["segPool"][:, :1]
    pool[2, 0, 2] = pool[2, 0, 1] - 1                              # (two nodes per lap)
    pool[2, 1] = pool[2, 0]
    pool[2, 0, 3], pool[2, 1, 3] = 1, 0                            # camera 2: 0 -> 1 -> 0 -> ...
    fr = S["featRef"].copy()
    fr[0, 1, 3] = seg_cap + 7                                      # camera 1: outside the pool
    _M, _cov, cnt, det = _check(S, dev, feat_ref=fr, pool_rows=pool, seg_cap=seg_cap)
    assert cnt == [1, 1, 0, 2] and det[0]["walks"][1]["cut"] and det[0]["walks"][2]["cut"] and not det[0]["walks"][0]["cut"]


def test_selection_edges(hip):
    S = planted.many_cameras(3)
    fs, fe = S["frame0"] + 10, S["frame0"] + 30
    S["lastFrame"] = np.array([fs, fs - 1, fe + 5, fe + 5, fe + 5, fe + 5], np.int32)
    S["firstFrame"] = np.array([fs - 5, fs - 5, fe, fe + 1, fs, fs], np.int32)
    S["flags"] = np.array([0, 0, 0, 0, 0, 4], np.uint8)
    M, _cov, cnt, _ = _check(S, _dev(), f_start=fs, f_end=fe, map_count=4)
    assert cnt[0] == 2 and np.array_equal((M != S["M0"]).any(axis=1), [True, False, True, False, False, False])
    _M, _cov, cnt, _ = _check(S, _dev(), f_start=fs, f_end=fe, map_count=6)
    assert cnt[0] == 3                                             # row 4 joins; row 5 is uncertain


@pytest.mark.parametrize("n_cams", [9, 10, 12, 16])
def test_two_views_from_every_camera(hip, n_cams):
    S = planted.many_cameras(n_cams)
    M, _cov, cnt, det = _check(S, _dev())
    assert cnt == [6, 6, 0, 0] and all(len(det[p]["views"]) == 2 * n_cams for p in det)
    assert np.abs(M - S["X"]).max() < 0.1


# ---- MergeApply ---------------------------------------------------------------------------------------------------------------------------------

def _pose_scene(n_cams, n_key, step=4, seed=5, extra_cam=True, pre=5, split=1):
    """make_merge_pose_graph's chains as a history: `pre` older frames in front, one more camera the plan does not name"""
    m = make_merge_pose_graph(n_cams, n_key, 1, split, seed=seed, frames_per_interval=step)
    ch = m["chains"]
    n_all = (n_key - 1) * step + 1
    nC = n_cams + (1 if extra_cam else 0)
    rng = np.random.default_rng(seed)
    R, T = np.zeros((nC, pre + n_all, 9)), np.zeros((nC, pre + n_all, 3))
    R[:n_cams, pre:], T[:n_cams, pre:] = ch["nodeR"].reshape(n_cams, n_all, 9), ch["nodeT"].reshape(n_cams, n_all, 3)
    if extra_cam:
        R[n_cams, pre:], T[n_cams, pre:] = R[0, pre:], T[0, pre:] + np.array([3.0, 0.5, 0.0])
    R[:, :pre], T[:, :pre] = R[:, pre:pre + 1], T[:, pre:pre + 1] + rng.normal(size=(nC, pre, 3)) * 0.01
    frame0 = 700
    key_frames = np.array([frame0 + pre + k * step for k in range(n_key)], np.int32)
    S = dict(K=np.tile(planted.K0, (nC, 1)), iK=np.tile(inv_k(planted.K0), (nC, 1)), histR=R, histT=T, histXY=np.zeros((nC, pre + n_all, 2)), N=1,
             nC=nC, nF=pre + n_all, frame0=frame0, featRef=np.full((1, nC, 4), -1, np.int32), segPool=np.full((nC, 0, 4), -1, np.int32))
    plan = dict(fixed_kf=0, node_kf=m["node_kf"], node_cam=m["node_cam"], fixed=m["fixed"], id1=m["id1"], id2=m["id2"], scale_id=m["scale_id"])
    return m, S, plan, key_frames


def _span(th, dev, first, n):
    import torch

    dR = torch.zeros((th.nCams, n, 9), dtype=torch.float64, device=dev)
    dT = torch.zeros((th.nCams, n, 3), dtype=torch.float64, device=dev)
    th.get_span_dev(torch.cuda.current_stream().cuda_stream, first, n, dR.data_ptr(), dT.data_ptr())
    torch.cuda.synchronize()
    return dR.cpu().numpy(), dT.cpu().numpy()


@pytest.mark.parametrize("n_cams,n_key", [(3, 4), (8, 6)])
def test_merge_apply_equals_the_host_fed_correction(hip, n_cams, n_key):
    dev = _dev()
    m, S, plan, key_frames = _pose_scene(n_cams, n_key)
    ch, sc = m["chains"], m["scale_id"] >= 0
    mc = coslam_amd.MergePoseCorrection((plan["fixed"], plan["id1"], plan["id2"], plan["scale_id"]), ch["graphs"], ch["key_node"])
    want = mc.run(m["nodeR"], m["nodeT"], m["edgeR"][sc], m["edgeT"][sc], ch["nodeR"], ch["nodeT"])
    mc.close()
    th, _cams, _keep = load_history(S, dev)
    before_R, before_T = _span(th, dev, S["frame0"], S["nF"])
    ma = coslam_amd.MergeApply(plan, key_frames, S["nC"])
    ma.run(th, m["edgeR"][sc], m["edgeT"][sc])
    ma.status()
    R, T = _span(th, dev, S["frame0"], S["nF"])
    pre, n_all = 5, ch["node_ptr"][1]
    assert np.array_equal(R[:n_cams, pre:].reshape(-1, 9), want["chainR"]) and np.array_equal(T[:n_cams, pre:].reshape(-1, 3), want["chainT"])
    assert np.array_equal(ma.d_edgeS.cpu().numpy()[:len(want["edgeS"])], want["edgeS"])
    assert np.array_equal(R[:, :pre], before_R[:, :pre]) and np.array_equal(T[:, :pre], before_T[:, :pre])      # older than keyFrames[0]
    dR, dT = np.abs(R[n_cams, pre:] - before_R[n_cams, pre:]).max(), np.abs(T[n_cams, pre:] - before_T[n_cams, pre:]).max()
    print(f"camera outside camIds: |dR| {dR:.2e} |dt| {dT:.2e}")
    assert dR < 1e-12 and dT < 1e-12 and n_all == S["nF"] - pre
    assert np.abs(T[n_cams - 1, pre:] - before_T[n_cams - 1, pre:]).max() > 1e-3                                  # the drifted camera moved
    ma.close()
    th.close()


def test_merge_apply_refusals(hip):
    import torch

    dev = _dev()
    m, S, plan, key_frames = _pose_scene(3, 5)
    sc = m["scale_id"] >= 0
    L = coslam_amd.lib()
    # the fixed key frame pushed out of the store
    th, _cams, _keep = load_history(S, dev, store_len=16)
    first = S["frame0"] + S["nF"] - 16
    b = _span(th, dev, first, 16)
    ma = coslam_amd.MergeApply(plan, key_frames, S["nC"])
    with pytest.raises(coslam_amd.CoslamHipError) as ei:
        ma.run(th, m["edgeR"][sc], m["edgeT"][sc])
    assert f"code {INVALID}" in str(ei.value) and "left the store" in str(ei.value)
    a = _span(th, dev, first, 16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    th.close()
    # the newest frame is not the current key frame
    S2 = dict(S, nF=S["nF"] + 1, histR=np.concatenate([S["histR"], S["histR"][:, -1:]], axis=1),
              histT=np.concatenate([S["histT"], S["histT"][:, -1:]], axis=1), histXY=np.zeros((S["nC"], S["nF"] + 1, 2)))
    th, _cams, _keep = load_history(S2, dev)
    b = _span(th, dev, S2["frame0"], S2["nF"])
    with pytest.raises(coslam_amd.CoslamHipError) as ei:
        ma.run(th, m["edgeR"][sc], m["edgeT"][sc])
    assert f"code {INVALID}" in str(ei.value) and "newest frame" in str(ei.value)
    assert L.cs_last_error().decode().count("newest frame") == 1
    a = _span(th, dev, S2["frame0"], S2["nF"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    torch.cuda.synchronize()
    ma.close()
    th.close()


def test_failed_solve_leaves_history_and_map_alone(hip):
    """all constraint translations zero: the scale is undetermined, the key graph fails numerically (no device fault) -- status() says so, the
    guarded write-back and the guarded re-triangulation store nothing"""
    import torch

    dev = _dev()
    E = e2e.build()
    S = E["S"]
    M0, cov0 = e2e.start_points(E, ref)
    th, cams, _keep = load_history(S, dev)
    before = _span(th, dev, S["frame0"], S["nF"])
    ma = coslam_amd.MergeApply(E["plan"], S["key_frames"], S["nC"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_ref, d_M, d_cov = t(S["featRef"]), t(M0.copy()), t(cov0.copy())
    d_ff, d_lf, d_fl, d_cnt = t(S["firstFrame"]), t(S["lastFrame"]), t(S["flags"]), torch.zeros(4, dtype=torch.int32, device=dev)
    ma.run(th, E["infoR"], np.zeros_like(E["infoT"]))
    ma.recompute(th, cams, d_ref.data_ptr(), len(M0), None, d_ff.data_ptr(), d_lf.data_ptr(), d_fl.data_ptr(), d_M.data_ptr(), d_cov.data_ptr(),
                 S["f_start"], S["sigma"], d_counts=d_cnt.data_ptr())
    with pytest.raises(coslam_amd.CoslamHipError) as ei:
        ma.status()
    assert f"code {NUMERIC}" in str(ei.value) and "key-frame graph" in str(ei.value)
    after = _span(th, dev, S["frame0"], S["nF"])
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert np.array_equal(d_M.cpu().numpy(), M0) and np.array_equal(d_cov.cpu().numpy(), cov0) and d_cnt.tolist() == [0, 0, 0, 0]
    # the same handle, now with the real constraints: the guard opens again
    ma.run(th, E["infoR"], E["infoT"])
    ma.recompute(th, cams, d_ref.data_ptr(), len(M0), None, d_ff.data_ptr(), d_lf.data_ptr(), d_fl.data_ptr(), d_M.data_ptr(), d_cov.data_ptr(),
                 S["f_start"], S["sigma"], d_counts=d_cnt.data_ptr())
    ma.status()
    assert d_cnt.tolist()[0] == len(M0) and not np.array_equal(d_M.cpu().numpy(), M0)
    ma.close()
    th.close()


def test_end_to_end_run_recompute_groups(hip):
    """4 cameras in two groups, 6 key frames x 4 frames, 192 points on 64 slots: run -> recompute -> merge_matched_groups"""
    import torch

    dev = _dev()
    E = e2e.build()
    S = E["S"]
    M0, cov0 = e2e.start_points(E, ref)
    th, cams, _keep = load_history(S, dev)
    ma = coslam_amd.MergeApply(E["plan"], S["key_frames"], S["nC"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_ref, d_M, d_cov = t(S["featRef"]), t(M0.copy()), t(cov0.copy())
    d_ff, d_lf, d_fl, d_cnt = t(S["firstFrame"]), t(S["lastFrame"]), t(S["flags"]), torch.zeros(4, dtype=torch.int32, device=dev)
    ma.run(th, E["infoR"], E["infoT"])
    ma.recompute(th, cams, d_ref.data_ptr(), len(M0), None, d_ff.data_ptr(), d_lf.data_ptr(), d_fl.data_ptr(), d_M.data_ptr(), d_cov.data_ptr(),
                 S["f_start"], S["sigma"], d_counts=d_cnt.data_ptr())
    ma.status()
    got = coslam_amd.merge_matched_groups(E["groups"], [0], [1], E["m"]["camid1"], E["m"]["camid2"])
    R, T = _span(th, dev, S["frame0"], S["nF"])
    wR, wT = e2e.corrected_poses_host(E)
    print(f"poses against the host restatement: |dR| {np.abs(R - wR).max():.2e} |dt| {np.abs(T - wT).max():.2e}")
    assert np.abs(R - wR).max() < TOL_R and np.abs(T - wT).max() < TOL_T
    # the points: the restatement fed the DEVICE's corrected poses, bit for bit
    M, cov = M0.copy(), cov0.copy()
    cnt = ref.recompute_map_points_keyfrms(S["K"], S["iK"], R, T, S["histXY"], S["frame0"], S["featRef"], S["segPool"], None, S["firstFrame"],
                                           S["lastFrame"], S["flags"], S["f_start"], S["f_end"], S["key_frames"], M, cov, S["sigma"])
    assert d_cnt.tolist() == cnt and np.array_equal(d_M.cpu().numpy(), M) and np.array_equal(d_cov.cpu().numpy(), cov)
    want = ref.merge_matched_groups(E["groups"], [0], [1], E["m"]["camid1"], E["m"]["camid2"])
    assert got["groups"] == want[0] == [[0, 1, 2, 3]] and list(got["group_id"]) == want[1] and got["merged_gid"] == want[2] == 0
    before, after = e2e.reproj_median(E, M0, S["histR"], S["histT"]), e2e.reproj_median(E, d_M.cpu().numpy(), R, T)
    print(f"median reprojection error of the drifted group's points in the other group's cameras: {before:.3f} px -> {after:.3f} px")
    assert after < before
    ma.close()
    th.close()


def test_cxx_shim_merge_apply(hip, tmp_path):
    """include/shim/app/CoSLAMMergeApply.h driven like CoSLAM::mergeCamGroups (tests/cxx/mergeapply_shim_test.cpp) against MergeApply on the same
    history: the same kernels on the same inputs, bit for bit; the merged groups against the restatement"""
    import struct
    import subprocess

    from coslam_amd.merge import _camera_groups_record

    exe = build_shim_test("mergeapply_shim_test.cpp", tmp_path)
    dev = _dev()
    m, S, _plan, key_frames = _pose_scene(3, 4, extra_cam=False, pre=0)
    kf_of = {f: int(key_frames[k]) for k, f in enumerate(m["frames"])}
    infos = [(kf_of[f1], c1, kf_of[f2], c2) for f1, c1, f2, c2 in m["infos"]]
    cur = m["groups"][-1]
    gid = {c: g for g, cams in enumerate(cur) for c in cams}
    plan = coslam_amd.merge_keygraph_plan(key_frames, m["groups"], m["cam_ids"], m["first_constrain"], m["camid1"], m["camid2"], infos)
    sc = m["scale_id"] >= 0
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("8i", S["nC"], S["nF"], S["frame0"], len(key_frames), m["first_constrain"], m["camid1"], m["camid2"], len(infos)))
        f.write(key_frames.astype(np.int32).tobytes())
        for g in m["groups"]:
            f.write(bytes(_camera_groups_record(g)))
        for (f1, c1, f2, c2) in infos:
            f.write(struct.pack("6i", f1, c1, f2, c2, gid[c1], gid[c2]))
        f.write(np.ascontiguousarray(m["edgeR"][sc]).tobytes() + np.ascontiguousarray(m["edgeT"][sc]).tobytes())
        f.write(np.ascontiguousarray(S["histR"]).tobytes() + np.ascontiguousarray(S["histT"]).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    th, _cams, _keep = load_history(S, dev)
    ma = coslam_amd.MergeApply(plan, key_frames, S["nC"])
    ma.run(th, m["edgeR"][sc], m["edgeT"][sc])
    ma.status()
    R, T = _span(th, dev, S["frame0"], S["nF"])
    ma.close()
    th.close()
    raw = open(tmp_path / "out.bin", "rb").read()
    n = S["nC"] * S["nF"]
    v = np.frombuffer(raw, np.float64, 12 * n)
    assert np.array_equal(v[:9 * n].reshape(R.shape), R) and np.array_equal(v[9 * n:].reshape(T.shape), T)
    assert not np.array_equal(R, S["histR"])
    rec = coslam_amd.CameraGroups.from_bytes(raw[96 * n:96 * n + 4 * 289])
    tail = struct.unpack_from("19i", raw, 96 * n + 4 * 289)
    g1, g2 = [gid[c1] for _f1, c1, _f2, _c2 in infos], [gid[c2] for _f1, _c1, _f2, c2 in infos]
    want = ref.merge_matched_groups(cur, g1, g2, m["camid1"], m["camid2"])
    assert rec.groups() == want[0] and list(tail[:16]) == want[1] and tail[16] == want[2]
    assert tail[17] == int(key_frames[plan["fixed_kf"]]) and tail[18] == int(key_frames[-1])
