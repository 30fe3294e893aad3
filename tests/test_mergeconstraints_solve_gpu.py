"""Stage B of the merge constraints: the two solves, the MergeInfo list and the hand-over.  cs_merge_info_dev on the unsolved
poses is the list the reference's own genMergeInfoVer2 leaves when its solver changes nothing (tests/golden/mergeconstraints_golden.npz),
bit for bit; on a caller's poses it is the restatement's.  cs_merge_constraints_solve is two runs of the existing robust BA on the
assembled problem: bit for bit the host-fed path (cs_ba_robust_h on the downloaded problem), each run against oracle.ba_robust within the
bounds of tests/test_pose_ba_gpu.py::test_ba_matches_oracle.  d_infoR / d_infoT go into cs_merge_apply_run_dev as they are."""
import ctypes as C

import numpy as np
import pytest

import coslam_amd
import oracle

from tests import mergeconstraints_ref as ref
from tests.cxx_build import build_shim_test
from tests.mergeconstraints_dev import DeviceScene, assemble_dev
from tests.mergeconstraints_golden_util import expand, load
from tests.mergeconstraints_scenes import make_scene, write_input

pytestmark = pytest.mark.gpu

SCENES = load()


def _dev():
    import torch

    return torch.device("cuda:0")


@pytest.mark.parametrize("sc", range(len(SCENES)))
def test_info_on_the_unsolved_poses_equals_the_reference(hip, sc):
    S, G = SCENES[sc]
    D = DeviceScene(S, _dev())
    mc, P, _ = assemble_dev(D, int(G["first_frame"]))
    mc.info(D.groups.data_ptr(), S["gId1"], S["gId2"])
    ints, R, t = mc.infos()
    assert mc.header().nInfo == len(G["info_ints"]) == len(ints)
    assert np.array_equal(ints, G["info_ints"].astype(np.int32)) and np.array_equal(R, G["info_R"]) and np.array_equal(t, G["info_t"])
    if int(G["verdict"]) != 1:
        assert len(ints) == 0                                   # a rejected verdict yields no constraint
    mc.close()
    D.th.close()


def test_info_on_a_callers_poses(hip):
    """poses handed in from the caller's own device buffers (where a solve leaves them), in the assembled order"""
    import torch

    S, G = SCENES[1]
    D = DeviceScene(S, _dev())
    mc, P, _ = assemble_dev(D, int(G["first_frame"]))
    rng = np.random.default_rng(5)
    Rs, Ts = P["Rs"] + 1e-3 * rng.normal(size=P["Rs"].shape), P["Ts"] + 1e-2 * rng.normal(size=P["Ts"].shape)
    dR, dT = torch.from_numpy(Rs).to(_dev()), torch.from_numpy(Ts).to(_dev())
    mc.info(D.groups.data_ptr(), S["gId1"], S["gId2"], dR.data_ptr(), dT.data_ptr())
    ints, R, t = mc.infos()
    order = [tuple(int(v) for v in r) for r in G["order"]]
    wi, wR, wt = ref.merge_infos(S, Rs.tolist(), Ts.tolist(), order)
    assert np.array_equal(ints[:, :6], np.array(wi)) and (ints[:, 6] == 1).all()
    assert np.array_equal(R, np.array(wR)) and np.array_equal(t, np.array(wt))
    assert not np.array_equal(R, G["info_R"])
    mc.close()
    D.th.close()


@pytest.mark.parametrize("solved", (False, True))
def test_info_buffers_feed_merge_apply(hip, solved):
    """check -> constraints (-> solves) -> plan -> apply: the constraint edges of cs_merge_keygraph_plan are in the order of the MergeInfo
    list, so d_infoR / d_infoT go straight into cs_merge_apply_run_dev: the same history as with the downloaded values, and status CS_OK"""
    import torch

    S, G = SCENES[3]
    dev = _dev()
    D = DeviceScene(S, dev)
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    k, _order = coslam_amd.merge_first_constrain(S["key_frames"], S["self_motion"], ids)
    assert k >= 1                                                   # an older key frame is there to be held fixed
    mc, P, _ = assemble_dev(D, int(S["key_frames"][k]))
    if solved:
        mc.solve()
        mc.info_solved(D.groups.data_ptr(), S["gId1"], S["gId2"])
    else:
        mc.info(D.groups.data_ptr(), S["gId1"], S["gId2"])
    ints, R, t = mc.infos()
    assert len(ints) == len(G["info_ints"]) > 0 and (ints[:, 6] == 1).all()
    assert np.array_equal(R, G["info_R"]) != solved                 # the solves move the poses
    groups = [[sorted(c for g in S["groups"] for c in g)]] + [S["groups"]] * (len(S["key_frames"]) - 1)    # one group in the oldest key frame
    plan = coslam_amd.merge_keygraph_plan(S["key_frames"], groups, ids, k, S["maxiCam"], S["maxjCam"], ints[:, [0, 1, 3, 4]])
    assert plan["n_constraint"] == len(ints) and plan["fixed_kf"] == 0
    ma = coslam_amd.MergeApply(plan, S["key_frames"], S["nC"])
    s = torch.cuda.current_stream().cuda_stream
    f0, nF = int(S["key_frames"][0]), int(S["key_frames"][-1] - S["key_frames"][0] + 1)
    span = lambda: (torch.zeros((S["nC"], nF, 9), dtype=torch.float64, device=dev), torch.zeros((S["nC"], nF, 3), dtype=torch.float64, device=dev))  # noqa: E731
    R0, T0 = span()
    D.th.get_span_dev(s, f0, nF, R0.data_ptr(), T0.data_ptr())
    out = []
    for direct in (True, False):
        D.th.set_span_dev(s, f0, nF, R0.data_ptr(), T0.data_ptr())
        if direct:
            ma.run_dev(D.th, mc.buf.infoR, mc.buf.infoT)
        else:
            ma.run(D.th, R, t)
        ma.status()                                                 # CS_OK, or it raises
        Ra, Ta = span()
        D.th.get_span_dev(s, f0, nF, Ra.data_ptr(), Ta.data_ptr())
        torch.cuda.synchronize()
        out.append((Ra.cpu().numpy(), Ta.cpu().numpy(), ma.d_edgeS.cpu().numpy()))
    for a, b in zip(out[0], out[1]):
        assert a.tobytes() == b.tobytes()
    # The constraints are the relative poses of the poses the history holds, so the correction has nothing to correct.  The scene's
    # rotations are float32 values used as doubles: orthogonal only to a few 2^-24, and the relaxation returns the NEAREST rotation of
    # every free node, which moves an entry by at most that defect -- 8 x 2^-24 bounds it.  The translations solve a consistent linear
    # system: DESIGN 3.20's tolerance of this solver (1e-9), as tests/test_mergeapply_gpu.py uses it.
    print(f"correction from self-consistent constraints: |dR| {np.abs(out[0][0] - R0.cpu().numpy()).max():.2e}, "
          f"|dt| {np.abs(out[0][1] - T0.cpu().numpy()).max():.2e}, scales {out[0][2][np.asarray(plan['scale_id']) >= 0]}")
    if not solved:
        assert np.abs(out[0][0] - R0.cpu().numpy()).max() < 8 * 2.0 ** -24 and np.abs(out[0][1] - T0.cpu().numpy()).max() < 1e-9
    else:
        assert not np.array_equal(out[0][0], R0.cpu().numpy())        # a real correction
    ma.close()
    mc.close()
    D.th.close()


def _robust_h(ws, P, Rs, Ts, pts, max_err, max_iter, inner):
    """cs_ba_robust_h on host copies -> (Rs, Ts, pts, outlier, stats)"""
    from coslam_amd.ba import BAStats

    L = coslam_amd.lib()
    Rs, Ts, pts = Rs.copy(), Ts.copy(), pts.copy()
    n = len(P["obs_cam"])
    out, st = np.zeros(max(n, 1), np.int32), BAStats()
    p = lambda v: C.c_void_p(np.ascontiguousarray(v).ctypes.data)  # noqa: E731
    Ks, ptr, cam, xy = (np.ascontiguousarray(P[k]) for k in ("Ks", "obs_ptr", "obs_cam", "obs_xy"))
    rc = L.cs_ba_robust_h(ws._h, len(Rs), len(pts), n, p(Ks), p(Rs), p(Ts), p(pts), p(ptr), p(cam), p(xy), 1, 1, C.c_double(max_err), int(max_iter),
                          int(inner), p(out), C.byref(st))
    assert rc == 0, coslam_amd.lib().cs_last_error()
    return Rs, Ts, pts, out[:n], st


def _against_oracle(sol, P, Rs0, Ts0, pts0, max_err, max_iter, inner):
    """the bounds of tests/test_pose_ba_gpu.py::test_ba_matches_oracle"""
    R_o, T_o, M_o, out_o, st_o = oracle.ba_robust(P["Ks"], Rs0, Ts0, pts0, P["obs_ptr"], P["obs_cam"], P["obs_xy"], 1, 1, max_err, max_iter, inner)
    R_o, T_o, M_o = np.asarray(R_o).reshape(-1, 9), np.asarray(T_o).reshape(-1, 3), np.asarray(M_o).reshape(-1, 3)
    sane = np.linalg.norm(M_o, axis=1) < 1e3
    scale = max(1.0, np.abs(M_o[sane]).max())
    dR, dT, dM = np.max(np.abs(sol["Rs"] - R_o)), np.max(np.abs(sol["Ts"] - T_o)), np.max(np.abs(sol["pts"][sane] - M_o[sane]))
    print(f"solve ({max_err}, {max_iter}, {inner}) against the oracle: |dR| {dR:.2e} |dT| {dT:.2e} |dM| {dM:.2e} (scale {scale:.2f}), "
          f"{int((sol['outlier'] != out_o[:len(sol['outlier'])]).sum())} outlier flags differ of {len(sol['outlier'])}, "
          f"outliers {int(sol['outlier'].sum())}, outer rounds {sol['stats'].nOuter} / {st_o.nOuter}, cost {sol['stats'].cost:.6f} / {st_o.cost:.6f}")
    assert np.array_equal(sol["outlier"], out_o[:len(sol["outlier"])])
    assert sane.mean() > 0.97
    assert dR < 1e-6 and dT < 1e-6 * scale and dM < 1e-6 * scale


@pytest.mark.parametrize("sc", [i for i, (_, G) in enumerate(SCENES) if int(G["verdict"]) == 1])
def test_two_solves(hip, sc):
    """the handle's two solves: bit for bit the host-fed path on the downloaded problem (the second started from the device's first
    result), the device buffers hold the second result, and each solve against oracle.ba_robust from the same start"""
    from coslam_amd.ba import BAWorkspace

    S, G = SCENES[sc]
    D = DeviceScene(S, _dev())
    mc, P, _ = assemble_dev(D, int(G["first_frame"]))
    mc.solve()
    s0, s1 = mc.solution(0), mc.solution(1)
    ws = BAWorkspace()
    h0 = _robust_h(ws, P, P["Rs"], P["Ts"], P["pts"], 800.0, 1, 100)
    h1 = _robust_h(ws, P, s0["Rs"], s0["Ts"], s0["pts"], 30.0, 5, 30)
    for sol, h in ((s0, h0), (s1, h1)):
        for k, v in zip(("Rs", "Ts", "pts", "outlier"), h[:4]):
            assert sol[k].tobytes() == np.ascontiguousarray(v).tobytes(), k
        assert (sol["stats"].cost, sol["stats"].nIterTotal, sol["stats"].nOutliers) == (h[4].cost, h[4].nIterTotal, h[4].nOutliers)
    hd, b = mc.header(), mc.buf
    assert np.array_equal(mc._down(b.solvedRs, 9 * hd.nPose, np.float64).reshape(-1, 9), s1["Rs"])
    assert np.array_equal(mc._down(b.solvedTs, 3 * hd.nPose, np.float64).reshape(-1, 3), s1["Ts"])
    assert np.array_equal(mc._down(b.solvedPts, 3 * hd.P, np.float64).reshape(-1, 3), s1["pts"])
    assert np.array_equal(mc._down(b.outlier, hd.nObs, np.int32), s1["outlier"])
    assert np.array_equal(s1["Rs"][0], P["Rs"][0]) and np.array_equal(s1["pts"][0], P["pts"][0])       # nCamsCon = nPtsCon = 1
    assert not np.array_equal(s1["Rs"][1:], P["Rs"][1:])
    _against_oracle(s0, P, P["Rs"], P["Ts"], P["pts"], 800.0, 1, 100)
    _against_oracle(s1, P, s0["Rs"], s0["Ts"], s0["pts"], 30.0, 5, 30)
    mc.close()
    D.th.close()


def test_no_constraint_without_a_solve_or_behind_a_rejected_verdict(hip):
    """nInfo = 0 and the info buffers untouched: before any solve, behind a rejected verdict, and again after a new assembly"""
    S, G = SCENES[0]
    D = DeviceScene(S, _dev())
    mc, P, _ = assemble_dev(D, int(G["first_frame"]))
    b = mc.buf
    before = mc._down(b.infoR, 9 * 48, np.float64).tobytes()
    mc.info_solved(D.groups.data_ptr(), S["gId1"], S["gId2"])
    assert mc.header().nInfo == 0 and mc._down(b.infoR, 9 * 48, np.float64).tobytes() == before
    with pytest.raises(coslam_amd.CoslamHipError):
        mc.solution(1)
    mc.solve()
    mc.info_solved(D.groups.data_ptr(), S["gId1"], S["gId2"])
    assert mc.header().nInfo == len(G["info_ints"])
    mc.assemble(D.th, D.cams, D.featRef.data_ptr(), S["nMap"], D.M.data_ptr(), D.groups.data_ptr(), S["gId1"], S["gId2"], S["maxiCam"], S["maxjCam"],
                int(G["first_frame"]), S["frame0"] + S["nF"] - 1, S["matches"])
    mc.info_solved(D.groups.data_ptr(), S["gId1"], S["gId2"])          # the earlier solve is not this assembly's
    assert mc.header().nInfo == 0
    mc.close()
    D.th.close()
    S, G = SCENES[2]
    assert int(G["verdict"]) == 0
    D = DeviceScene(S, _dev())
    mc, P, _ = assemble_dev(D, int(G["first_frame"]))
    mc.solve()                                                          # nothing to solve: not an error
    mc.info_solved(D.groups.data_ptr(), S["gId1"], S["gId2"])
    assert mc.header().nInfo == 0 and mc.header().verdict == 0
    mc.close()
    D.th.close()


def test_noise_free_scene_measured(hip):
    """MEASURED, not asserted (docs/MEASUREMENTS.md): two groups of 2 cameras whose pixels are exact projections of the true points under
    the history's poses (rounded to float32), map points off by 3-5 cm: how far the constraints behind the two solves stand from the
    relative poses of the history, next to the unsolved ones (which ARE those relative poses)"""
    spec = dict(groups=[[0, 1], [3, 2]], g=(0, 1), ij=(0, 2), nF=10, gaps=(3, 2, 2), moved=[{0, 1, 2, 3}, {1}, set()], nA=60, nB=60, nMatch=12,
                plant="clean", noise=0.0)
    S = expand(make_scene(0, spec, np.random.default_rng(77)))
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    f1 = int(S["key_frames"][ref.first_constrain(S["key_frames"], S["self_motion"], ids)[0]])
    D = DeviceScene(S, _dev())
    mc, P, _ = assemble_dev(D, f1)
    assert P["header"].verdict == 1
    mc.info(D.groups.data_ptr(), S["gId1"], S["gId2"])
    _, R_true, t_true = mc.infos()
    mc.solve()
    mc.info_solved(D.groups.data_ptr(), S["gId1"], S["gId2"])
    ints, R, t = mc.infos()
    s1 = mc.solution(1)
    ang = [float(np.degrees(np.arccos(np.clip((np.trace(a.reshape(3, 3) @ b.reshape(3, 3).T) - 1) / 2, -1, 1)))) for a, b in zip(R, R_true)]
    rel_t = np.linalg.norm(t - t_true, axis=1) / np.maximum(np.linalg.norm(t_true, axis=1), 1e-12)
    print(f"noise-free scene: {P['header'].P} points, {P['header'].nObs} measurements, avgErr {P['header'].avgErr:.3f} px; cost {mc.solution(0)['stats'].cost0:.3f} -> "
          f"{s1['stats'].cost:.3e}, {int(s1['outlier'].sum())} outliers; {len(ints)} constraints against the history's relative poses: "
          f"rotation max {max(ang):.2e} deg, translation max |dt| / |t| {rel_t.max():.2e} (max |dt| {np.abs(t - t_true).max():.2e})")
    assert len(ints) == len(R_true) > 0
    mc.close()
    D.th.close()


@pytest.mark.parametrize("sc", (5, 2))
def test_cxx_shim_gen_merge_info(hip, tmp_path, sc):
    """include/shim/app/CoSLAMMergeConstraints.h driven like matchMergableCameras (tests/cxx/mergeconstraints_shim_test.cpp: the matches as
    the reference's list indices) against MergeConstraints on the same scene: first-constrained frame, verdict, avgErr, counts and the
    MergeInfo list behind the two solves, bit for bit; a rejected verdict returns false with no info"""
    import struct
    import subprocess

    exe = build_shim_test("mergeconstraints_shim_test.cpp", tmp_path)
    S, G = SCENES[sc]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("i", 1))
        write_input(f, S)
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    ok, verdict, first, n_info, P, n_obs, skipped, n_ids = struct.unpack_from("8i", raw, 0)
    avg = struct.unpack_from("d", raw, 32)[0]
    D = DeviceScene(S, _dev())
    mc, Pr, _ = assemble_dev(D, int(G["first_frame"]))
    mc.solve()
    mc.info_solved(D.groups.data_ptr(), S["gId1"], S["gId2"])
    ints, R, t = mc.infos()
    h = mc.header()
    assert (ok, verdict, n_info, P, n_obs, skipped, n_ids, avg) == (int(h.verdict == 1), h.verdict, h.nInfo, h.P, h.nObs, h.skippedMatches, h.nCamIds, h.avgErr)
    assert int(S["key_frames"][first]) == int(G["first_frame"]) and verdict == int(G["verdict"])
    rec = np.frombuffer(raw, np.dtype([("i", "<i4", 7), ("R", "<f8", 9), ("t", "<f8", 3)]), n_info, 40)
    assert np.array_equal(rec["i"], ints) and rec["R"].tobytes() == R.tobytes() and rec["t"].tobytes() == t.tobytes()
    assert (n_info > 0) == (verdict == 1) and len(raw) == 40 + n_info * rec.dtype.itemsize
    mc.close()
    D.th.close()
