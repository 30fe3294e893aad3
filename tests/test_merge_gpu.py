"""Merge candidates on the device (cs_merge_check_dev, coslam_amd/csrc/merge.hip) against the line-cited restatement of
MergeCameraGroup::checkPossibleMergable (tests/merge_ref.py; reference src/app/SL_MergeCameraGroup.cpp:56-177) with its exact-arithmetic hull
and pixel test: nMergeInfo, info[] (order included), nFeat, nInCam, inNum and fromTo EQUAL -- every decision of the planted scenes has a
margin of at least 1e-6 px (asserted on the restatement first; tests/test_merge_cpu.py says why that is four decades above f64 rounding) --
and camDist within 1e-12 * (1 + max|t|): fewer than 20 roundings of 1.1e-16 relative, two decades.  Kernel level over planted scenes and the
hand-counted lattice scene, then both frame loops with the check switched on."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import merge_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 0x5A


@pytest.fixture(scope="module")
def planted():
    scenes = M.scene_set()
    res = M.scene_results(scenes)
    M.assert_scene_conditions(scenes, res)        # on the restatement, before the kernel is looked at
    return scenes, res


def groups_record(groups, nCams):
    from coslam_amd.grouping import CameraGroups

    g = CameraGroups()
    g.groupNum = len(groups)
    for a in range(16):
        g.groupId[a] = -1
        for b in range(16):
            g.camIds[a][b] = -1
    for k, cams in enumerate(groups):
        g.num[k] = len(cams)
        for q, c in enumerate(cams):
            g.camIds[k][q] = c
            g.groupId[c] = k
    return g


class Dev:
    """a scene in device memory, and the entry's output (prefilled with a marker)"""

    def __init__(self, s):
        import torch

        from coslam_amd.merge import MergeCandidates, merge_cams, merge_check_scratch_bytes

        self.s, self.torch = s, torch
        dev = torch.device("cuda", 0)
        nC = s["nCams"]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.xy = up(s["xy"].transpose(0, 2, 1))   # the hand-back's layout: x[N] then y[N]
        self.state, self.s2m = up(s["state"].astype(np.int32)), up(s["slot2map"].astype(np.int32))
        self.K, self.R, self.t = up(s["K"]), up(s["R"]), up(s["t"])
        self.map, self.flags = up(s["mapPts"]), up(s["mapFlags"])
        self.mapCount = up(np.array([s["mapCount"]], dtype=np.int32))
        self.groups = up(np.frombuffer(bytes(groups_record(s["groups"], nC)), dtype=np.uint8).copy())
        self.cams = merge_cams([dict(xy=self.xy[c].data_ptr(), state=self.state[c].data_ptr(), slot2map=self.s2m[c].data_ptr(),
                                     K=self.K[c].data_ptr(), R=self.R[c].data_ptr(), t=self.t[c].data_ptr()) for c in range(nC)])
        self.out = torch.full((C.sizeof(MergeCandidates),), MARK, dtype=torch.uint8, device=dev)
        self.scratch = torch.zeros(merge_check_scratch_bytes(nC, s["N"]), dtype=torch.uint8, device=dev)   # zeroed ONCE
        self.stream = torch.cuda.current_stream().cuda_stream

    def check(self, par, all_pairs=False, **kw):
        from coslam_amd.merge import MergeCandidates, merge_check_dev

        s = self.s
        a = dict(stream_ptr=self.stream, cams=self.cams, N=s["N"], nMap=s["nMap"], d_mapCount=self.mapCount.data_ptr(), d_mapPts=self.map.data_ptr(),
                 d_mapFlags=self.flags.data_ptr(), W=s["W"], H=s["H"], d_groups=self.groups.data_ptr(), frame=s["frame"], d_out=self.out.data_ptr(),
                 d_scratch=self.scratch.data_ptr(), minInNum=par[0], minInAreaRatio=par[1], maxCamDist=par[2], allPairs=all_pairs)
        a.update(kw)
        merge_check_dev(**a)
        self.torch.cuda.synchronize()
        assert not self.scratch.any().item(), "the call left its scratch counters dirty"
        raw = self.out.cpu().numpy().tobytes()
        return MergeCandidates.from_bytes(raw), raw


def same_as_restatement(got, r, s, where):
    nC = s["nCams"]
    t = got.tables(nC)
    print(f"{where}: nMergeInfo {got.nMergeInfo} (restatement {len(r['info'])}), evaluated pairs {int((r['nInCam'] >= 0).sum())}, "
          f"largest |camDist - restatement| {float(np.abs(np.array(t['camDist']) - r['camDist']).max()):.3e}")
    assert (got.frame, got.groupNum, got.reserved) == (s["frame"], len(s["groups"]), 0), where
    assert got.nMergeInfo == len(r["info"]) and got.infos() == r["info"], where          # order included
    assert all(got.info[k].as_tuple() == (-1,) * 6 for k in range(got.nMergeInfo, 256)), where
    assert t["nFeat"] == r["nFeat"], where
    assert np.array_equal(np.array(t["nInCam"]), r["nInCam"]) and np.array_equal(np.array(t["inNum"]), r["inNum"]), where
    assert np.array_equal(np.array(t["fromTo"]), r["fromTo"]), where
    tol = 1e-12 * (1.0 + float(np.abs(s["t"]).max()))
    assert float(np.abs(np.array(t["camDist"]) - r["camDist"]).max()) <= tol, where
    for i in range(16):                      # behind the rig: -1 / 0
        for j in range(16):
            if i >= nC or j >= nC:
                assert got.nInCam[i][j] == -1 and got.inNum[i][j] == -1 and got.fromTo[i][j] == 0 and got.camDist[i][j] == 0.0
    assert all(got.nFeat[c] == -1 for c in range(nC, 16))


@pytest.mark.timeout(300)
def test_every_planted_scene_and_the_lattice_equal_the_restatement_with_and_without_all_pairs(hip, planted):
    scenes, res = planted
    assert hasattr(hip, "cs_merge_check_dev")
    for name, s, par in scenes:
        d = Dev(s)
        for ap in (False, True):
            got, _ = d.check(par, ap)
            same_as_restatement(got, res[name, ap], s, f"{name} allPairs={int(ap)}")
    s = M.lattice_scene()
    d = Dev(s)
    for ap in (False, True):
        got, _ = d.check(M.LATTICE_PARAMS, ap)
        same_as_restatement(got, M.check_possible_mergable(s, *M.LATTICE_PARAMS, all_pairs=ap), s, f"lattice allPairs={int(ap)}")
        assert got.nInCam[0][1] == 13 and got.inNum[0][1] == M.LATTICE_IN_NUM == 14 and got.fromTo[0][1] == 1   # the hand count
        assert got.nFeat[0] == 13 and got.nFeat[1] == 21 and got.inNum[1][0] == -1 and got.nMergeInfo == 0


@pytest.mark.timeout(300)
def test_two_calls_are_byte_identical_and_leave_the_scratch_zeroed(hip, planted):
    scenes, _ = planted
    for name, s, par in scenes:
        d = Dev(s)
        for ap in (False, True):
            a, b = d.check(par, ap)[1], d.check(par, ap)[1]      # (check() asserts the scratch after every call)
            assert a == b, (name, ap)


@pytest.mark.timeout(120)
def test_one_group_leaves_the_pair_tables_untouched_unless_all_pairs(hip, planted):
    scenes, res = planted
    name, s, par = [x for x in scenes if x[0] == "onegroup8"][0]
    d = Dev(s)
    got, _ = d.check(par, False)
    assert got.groupNum == 1 and got.nMergeInfo == 0
    t = got.tables(8)
    assert (np.array(t["nInCam"]) == -1).all() and (np.array(t["inNum"]) == -1).all() and not np.array(t["fromTo"]).any() and t["nFeat"] == [-1] * 8
    got, _ = d.check(par, True)
    same_as_restatement(got, res[name, True], s, "onegroup8 allPairs=1")
    assert (np.array(got.tables(8)["nInCam"])[~np.eye(8, dtype=bool)] >= 0).all() and got.nMergeInfo == 0


@pytest.mark.timeout(120)
def test_one_camera_gives_a_one_group_record(hip):
    s = M.planted_scene(11, 1, 200, 1000, [[0]], [0.0], {0: [(50, 0, M.FULL, None, "ok")]})
    d = Dev(s)
    for ap in (False, True):
        got, _ = d.check(M.DEFAULTS, ap)
        assert (got.frame, got.groupNum, got.nMergeInfo, got.reserved) == (s["frame"], 1, 0, 0)
        assert got.nInCam[0][0] == -1 and got.inNum[0][0] == -1 and got.fromTo[0][0] == 0 and got.camDist[0][0] == 0.0 and got.nFeat[0] == -1


@pytest.mark.timeout(120)
def test_bad_arguments_are_refused_with_a_message_and_no_launch(hip):
    import torch

    import coslam_amd
    from coslam_amd.merge import MergeCam

    s = M.lattice_scene()
    d = Dev(s)
    one = dict(xy=d.xy[0].data_ptr(), state=d.state[0].data_ptr(), slot2map=d.s2m[0].data_ptr(), K=d.K[0].data_ptr(), R=d.R[0].data_ptr(),
               t=d.t[0].data_ptr())
    for cams in ((MergeCam * 0)(), [one] * 17):
        with pytest.raises(coslam_amd.CoslamHipError, match="cameras"):
            d.check(M.DEFAULTS, cams=cams)
    for bad in (dict(d_out=0), dict(d_scratch=0), dict(d_groups=0), dict(d_mapPts=0), dict(cams=[one, dict(one, state=0)]),
                dict(cams=[one, dict(one, K=0)])):
        with pytest.raises(coslam_amd.CoslamHipError, match="null"):
            d.check(M.DEFAULTS, **bad)
    with pytest.raises(coslam_amd.CoslamHipError, match="N < 1"):
        d.check(M.DEFAULTS, N=0)
    with pytest.raises(coslam_amd.CoslamHipError, match="does not fit"):
        d.check(M.DEFAULTS, N=6000)
    torch.cuda.synchronize()
    assert (d.out == MARK).all().item() and not d.scratch.any().item()      # nothing ran


# ---- both frame loops with the check switched on (the bench workload) ------------------------------------------------------------------------
N_LOOP_FRAMES = 16     # key frames at 1, 6, 11, 16 (bench.KEY_EVERY = 5): the shortest run that holds four
CHECKED_KEY_FRAMES = (6, 16)


@pytest.fixture(scope="module")
def workload(tmp_path_factory):
    import torch

    import bench

    dev = torch.device("cuda", 0)
    frames = bench.render_video(list(range(bench.N_CAMS)), bench.N_FRAMES)
    video = {c: torch.from_numpy(frames[c]).to(dev) for c in range(bench.N_CAMS)}
    sc = bench.build_scene()
    wl = str(tmp_path_factory.mktemp("merge") / "workload.bin")
    bench.export_workload(wl, sc, frames, bench.build_joint_problem(sc), bench.build_ic_problem(sc), 0)
    return bench, sc, video, wl


def _loop(bench, sc, video, **kw):
    from coslam_amd.frameloop import FrameLoop, LoopConfig

    cfg = LoopConfig(n_cams=bench.N_CAMS, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                     n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG, **kw)
    loop = FrameLoop(cfg, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0,
                     associate=bench.associate)
    loop.first_frame()
    return loop


def _run_python_loop(bench, sc, video, watch=(), n_frames=N_LOOP_FRAMES, **kw):
    """n_frames of the loop; at the key frames in `watch` the tables the check reads are copied to the host right in front of its launch
    (a wait of the test's, at those frames only) -> digest, merge_stats(), {frame: (scene dict, the record the loop made of it)}"""
    from coslam_amd.grouping import CameraGroups
    from coslam_amd.merge import MergeCandidates

    loop = _loop(bench, sc, video, **kw)
    cfg, NA, N = loop.cfg, loop.cfg.n_cams, loop.cfg.n_feat
    snaps = {}
    if watch:
        launch = loop._merge_check

        def watched(f, dst, snap=None):
            if f in watch:
                assert snap is None
                loop.pose_s.synchronize()
                g = loop.grouping
                rec = CameraGroups.from_bytes(g["groups"][(g["calls"] - 1) % loop.GROUP_RING].cpu().numpy().tobytes())
                snaps[f] = [dict(nCams=NA, N=N, nMap=loop.n_map, W=cfg.W, H=cfg.H, mapCount=int(loop.d_mapcount.item()), mapPts=loop.d_map.cpu().numpy(),
                                 mapFlags=loop.d_mapflags.cpu().numpy(), xy=loop.d_xy.cpu().numpy().reshape(NA, 2, N).transpose(0, 2, 1),
                                 state=loop.d_state.cpu().numpy(), slot2map=loop.d_slot2map.cpu().numpy(),
                                 K=np.tile(loop.d_K1.cpu().numpy(), (NA, 1)), R=loop.d_R[dst].cpu().numpy(), t=loop.d_t[dst].cpu().numpy(),
                                 groups=rec.groups(), frame=f), loop.merge["calls"] % loop.MERGE_RING]
            launch(f, dst, snap)
            if f in watch:
                loop.pose_s.synchronize()
                snaps[f][1] = MergeCandidates.from_bytes(loop.merge["ring"][snaps[f][1]].cpu().numpy().tobytes())

        loop._merge_check = watched
    for n in range(n_frames):
        loop.step(n + 1, n % bench.KEY_EVERY == 0)
    loop.drain()
    return loop.digest(), loop.merge_stats(), snaps


@pytest.fixture(scope="module")
def python_cut_run(workload):
    bench, sc, video, _ = workload
    return _run_python_loop(bench, sc, video, watch=CHECKED_KEY_FRAMES, camera_grouping=True, merge_check=True, group_max_dist_ratio=1e-9)


@pytest.mark.timeout(600)
def test_python_loop_checks_every_key_frame_and_its_records_equal_the_restatement(hip, workload, python_cut_run):
    bench, sc, video, _ = workload
    NA = bench.N_CAMS
    _, st, snaps = python_cut_run
    key_frames = [n + 1 for n in range(N_LOOP_FRAMES) if n % bench.KEY_EVERY == 0]
    assert sorted(snaps) == list(CHECKED_KEY_FRAMES) and set(CHECKED_KEY_FRAMES) <= set(key_frames)
    for f, (s, rec) in sorted(snaps.items()):
        assert s["groups"] == [[c] for c in range(NA)] and rec.groupNum == NA          # every edge cut: eight singleton groups
        r = M.check_possible_mergable(s, loopcfg_defaults()[0], loopcfg_defaults()[1], loopcfg_defaults()[2])
        margins = [min(d["image_margin"] for d in r["detail"].values()), min(d["edge_margin"] for d in r["detail"].values()), r["dist_margin"]]
        print(f"key frame {f}: nFeat {r['nFeat']}, MergeInfo {len(r['info'])}, smallest margins (image, edge, distance) {margins}")
        same_as_restatement(rec, r, s, f"python loop, key frame {f}")
        assert max(r["nFeat"]) > 0 and int(r["nInCam"].max()) > 0
    assert st["key_frames_checked"] == len(key_frames) == 4 and st["key_frames_with_more_than_one_group"] == 4
    assert st["last_frame"] == key_frames[-1] and st["last_group_num"] == NA
    last = snaps[key_frames[-1]][1]
    assert st["last_info"] == [list(x) for x in last.infos()] and st["last_nInCam"] == last.tables(NA)["nInCam"]
    assert st["key_frames_with_a_candidate"] >= sum(1 for f in snaps if snaps[f][1].nMergeInfo > 0)
    assert (st["first_such_frame"] is None) == (st["key_frames_with_a_candidate"] == 0)
    # the reference's defaults (one group): the check changes nothing, and says so
    d_on, st_on, _ = _run_python_loop(bench, sc, video, camera_grouping=True, merge_check=True)
    d_off, st_off, _ = _run_python_loop(bench, sc, video, camera_grouping=True, merge_check=False)
    assert st_off is None and d_on == d_off
    assert st_on["key_frames_checked"] == 4 and st_on["key_frames_with_more_than_one_group"] == 0 and st_on["key_frames_with_a_candidate"] == 0
    assert st_on["last_info"] == [] and st_on["last_nFeat"] == [-1] * NA
    with pytest.raises(ValueError, match="camera_grouping"):
        _loop(bench, sc, video, merge_check=True)


def loopcfg_defaults():
    from coslam_amd.frameloop import LoopConfig

    c = LoopConfig(n_cams=2, W=64, H=48, levels=1, fw=2, fh=2, pts_stride=4, n_col_blk=1, n_row_blk=1, key_every=5, p_reg=16)
    assert (c.merge_min_in_num, c.merge_min_in_area_ratio, c.merge_max_cam_dist) == (10, 0.5, 6.0) and c.merge_check is False
    return c.merge_min_in_num, c.merge_min_in_area_ratio, c.merge_max_cam_dist


@pytest.mark.timeout(600)
def test_cxx_loop_keeps_its_digest_and_reports_what_the_python_loop_reports(hip, workload):
    """The C++ loop always plays its set-up (the window's five key-frame intervals and one set-up round: 50 frames) in front of warm-up and
    steps, so its shortest run is `<steps 1> <warm-up 0>`: 51 frames, key frames at 1, 6, ..., 51.  The Python loop is played over the same
    frames with every edge cut."""
    bench, sc, video, wl = workload
    exe = os.path.join(ROOT, "tools", "cxx", "frame_loop.bin")
    assert os.path.exists(exe), "tools/cxx/frame_loop.bin missing: __graft_entry__.build()"
    out = {}
    for name, env in (("off", dict(COSLAM_CAMERA_GROUPING="1")), ("on", dict(COSLAM_CAMERA_GROUPING="1", COSLAM_MERGE_CHECK="1")),
                      ("cut", dict(COSLAM_CAMERA_GROUPING="1", COSLAM_MERGE_CHECK="1", COSLAM_GROUP_MAX_DIST_RATIO="1e-9"))):
        p = subprocess.run([exe, wl, "1", "0", "0", "2"], env=dict(os.environ, HSA_KERNARG_POOL_SIZE=str(64 << 20), **env),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        out[name] = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    n_frames = out["off"]["frames_run"]
    n_key = (n_frames - 1) // bench.KEY_EVERY + 1
    assert all(o["frames_run"] == n_frames for o in out.values()) and n_key >= 4
    assert out["off"]["merge_check"] is None
    assert out["on"]["digest"] == out["off"]["digest"]          # the check only reads loop state
    on = out["on"]["merge_check"]
    assert on["key_frames_checked"] == n_key and on["key_frames_with_more_than_one_group"] == 0 and on["last_info"] == []
    _, st, _ = _run_python_loop(bench, sc, video, n_frames=n_frames, camera_grouping=True, merge_check=True, group_max_dist_ratio=1e-9)
    cut = out["cut"]["merge_check"]
    print(f"{n_frames} frames, {n_key} key frames; cut: {({k: cut[k] for k in cut if not k.startswith('last_n') and k not in ('last_inNum', 'last_fromTo')})}")
    assert cut["key_frames_checked"] == n_key and cut["key_frames_with_more_than_one_group"] == n_key and cut["last_group_num"] == bench.N_CAMS
    for k in ("key_frames_checked", "key_frames_with_more_than_one_group", "key_frames_with_a_candidate", "first_such_frame", "last_frame",
              "last_group_num", "last_info", "last_nFeat", "last_nInCam", "last_inNum", "last_fromTo"):
        assert cut[k] == st[k], (k, cut[k], st[k])
    p = subprocess.run([exe, wl, "4", "0"], env=dict(os.environ, COSLAM_MERGE_CHECK="1"), capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "COSLAM_CAMERA_GROUPING" in p.stderr      # refused without the grouping
