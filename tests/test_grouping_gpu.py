"""Camera grouping on the device (cs_view_overlap_costs_dev / cs_camera_grouping_dev, coslam_amd/csrc/grouping.hip) against the line-cited
restatement of CoSLAM::getViewOverlapCosts / cameraGrouping (tests/grouping_ref.py; reference src/app/SL_CoSLAM.cpp:1543-1697) with its
exact-arithmetic hull: counts, costs and groups EQUAL, hull areas within 1e-9 * W * H -- a shoelace sum over at most N <= 5000 vertices of
terms bounded by 2 W H carries a rounding error below 5000 * 2^-52 * 2 W H ~ 2.3e-12 W H, and a vertex wrongly kept or dropped by an f64
orientation test lies within rounding distance of an edge and moves the area by the same order; 1e-9 leaves more than two decades.
Kernel level over planted scenes, then both frame loops with the step switched on."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import grouping_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Dev:
    """a planted scene in device memory, and the two entries' outputs"""

    def __init__(self, s):
        import torch

        from coslam_amd.grouping import CameraGroups, camera_grouping_scratch_bytes, grouping_cams

        self.s, self.torch = s, torch
        dev = torch.device("cuda", 0)
        nC = s["nCams"]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.pf, self.flags, self.R, self.t = up(s["pointFeat"]), up(s["mapFlags"]), up(s["R"]), up(s["t"])
        self.xy = up(s["xy"].transpose(0, 2, 1))   # the hand-back's layout: x[N] then y[N]
        self.mapCount = up(np.array([s["mapCount"]], dtype=np.int32))
        lst = np.full(s["nMap"], -1, dtype=np.int32)
        lst[:len(s["rows"])] = s["rows"]
        self.list, self.listCount = up(lst), up(np.array([len(s["rows"])], dtype=np.int32))
        self.cams = grouping_cams([dict(xy=self.xy[c].data_ptr(), R=self.R[c].data_ptr(), t=self.t[c].data_ptr()) for c in range(nC)])
        self.vcosts = torch.full((nC * nC,), 7.0, dtype=torch.float64, device=dev)
        self.nShare = torch.full((nC * nC,), 7, dtype=torch.int32, device=dev)
        self.area = torch.full((nC * nC,), 7.0, dtype=torch.float64, device=dev)
        self.groups = torch.full((C.sizeof(CameraGroups),), 7, dtype=torch.uint8, device=dev)
        self.scratch = torch.zeros(camera_grouping_scratch_bytes(nC, s["N"]), dtype=torch.uint8, device=dev)   # zeroed ONCE
        self.stream = torch.cuda.current_stream().cuda_stream

    def costs(self, num, ratio, area=True, listed=False):
        from coslam_amd.grouping import view_overlap_costs_dev

        s = self.s
        view_overlap_costs_dev(self.stream, self.cams, s["N"], s["nMap"], self.mapCount.data_ptr(), self.pf.data_ptr(), self.flags.data_ptr(), s["W"],
                               s["H"], self.vcosts.data_ptr(), self.nShare.data_ptr(), self.scratch.data_ptr(), num, ratio,
                               self.area.data_ptr() if area else None, self.list.data_ptr() if listed else None,
                               self.listCount.data_ptr() if listed else None)
        return self.read(area)

    def grouping(self, num, ratio, area=False, listed=False, max_dist_ratio=6.0):
        from coslam_amd.grouping import CameraGroups, camera_grouping_dev

        s = self.s
        camera_grouping_dev(self.stream, self.cams, s["N"], s["nMap"], self.mapCount.data_ptr(), self.pf.data_ptr(), self.flags.data_ptr(), s["W"], s["H"],
                            self.vcosts.data_ptr(), self.nShare.data_ptr(), self.scratch.data_ptr(), s["initCamTranslation"], self.groups.data_ptr(),
                            max_dist_ratio, num, ratio, self.area.data_ptr() if area else None, self.list.data_ptr() if listed else None,
                            self.listCount.data_ptr() if listed else None)
        out = self.read(area)
        out["raw_groups"] = self.groups.cpu().numpy().tobytes()
        out["G"] = CameraGroups.from_bytes(out["raw_groups"])
        return out

    def read(self, area):
        self.torch.cuda.synchronize()
        nC = self.s["nCams"]
        out = dict(vcosts=self.vcosts.cpu().numpy().reshape(nC, nC), nShare=self.nShare.cpu().numpy().reshape(nC, nC))
        if area:
            out["area"] = self.area.cpu().numpy().reshape(nC, nC)
        assert not self.scratch[:4 * 257].any().item(), "the call left its scratch counters dirty"
        return out


def same_groups(got, ref, nC):
    g = got["G"]
    assert g.groupNum == len(ref["groups"])
    assert [g.num[k] for k in range(g.groupNum)] == [len(x) for x in ref["groups"]]
    assert g.groups() == ref["groups"]                      # camIds, first num entries, in the order of discovery
    assert [g.groupId[c] for c in range(nC)] == ref["groupId"]


@pytest.mark.timeout(600)
def test_counts_costs_areas_and_groups_equal_the_restatement_on_every_planted_scene(hip):
    scenes = G.scene_set()
    ref = G.scene_results(scenes)
    G.assert_scene_conditions(scenes, ref)        # on the restatement, before the kernel is looked at
    assert sorted(s["nCams"] for _, s in scenes) == [2, 3, 5, 8, 13, 16]
    worst = 0.0
    for name, s in scenes:
        d = Dev(s)
        nC, WH = s["nCams"], float(s["W"]) * s["H"]
        for th in ((0, 0.0), G.THRESHOLDS):
            r = ref[name, th]
            # getViewOverlapCosts alone: the restatement's costs BEFORE the distance cut
            v0, n0, a0 = G.view_overlap_costs(s["pointFeat"], s["mapFlags"], s["xy"], s["W"], s["H"], th[0], th[1], s["mapCount"], with_area=False) \
                if th[1] <= 0 else (None, None, None)
            for listed in (False, True):
                c = d.costs(th[0], th[1], area=True, listed=listed)
                delta = float(np.abs(c["area"] - r["area"]).max()) / WH
                worst = max(worst, delta)
                print(f"{name} thresholds {th} listed {listed}: largest |area - exact| / (W H) = {delta:.3e}")
                assert np.array_equal(c["nShare"], r["nShare"]), (name, th, listed)
                assert delta <= 1e-9, (name, th, listed, delta)
                if v0 is not None:
                    assert np.array_equal(c["vcosts"], v0), (name, th, listed)
                    c2 = d.costs(th[0], th[1], area=False, listed=listed)      # the counting path alone
                    assert np.array_equal(c2["vcosts"], v0) and np.array_equal(c2["nShare"], r["nShare"])
                g = d.grouping(th[0], th[1], area=False, listed=listed)
                assert np.array_equal(g["nShare"], r["nShare"]) and np.array_equal(g["vcosts"], r["vcosts"]), (name, th, listed)
                same_groups(g, r, nC)
    print(f"largest |area - exact| / (W H) over the set: {worst:.3e}")


@pytest.mark.timeout(300)
def test_two_calls_are_byte_identical_and_a_full_list_changes_nothing(hip):
    for name, s in G.scene_set():
        d = Dev(s)
        runs = []
        for listed in (False, False, True):
            g = d.grouping(*G.THRESHOLDS, area=True, listed=listed)
            runs.append((g["vcosts"].tobytes(), g["nShare"].tobytes(), g["area"].tobytes(), g["raw_groups"]))
        assert runs[0] == runs[1], name
        assert runs[0] == runs[2], name
        a = d.grouping(0, 0.0)
        b = d.grouping(0, 0.0, listed=True)
        assert a["raw_groups"] == b["raw_groups"] and a["vcosts"].tobytes() == b["vcosts"].tobytes()


@pytest.mark.timeout(120)
def test_one_camera_is_one_group_on_the_device(hip):
    s = G.planted_scene(5, 1, 200, 1000, 640, 480, [((0,), 50, None)])
    d = Dev(s)
    g = d.grouping(0, 0.0)
    assert g["G"].groups() == [[0]] and g["G"].groupId[0] == 0 and g["vcosts"][0, 0] == -1 and g["nShare"][0, 0] == 0


@pytest.mark.timeout(120)
def test_bad_arguments_are_refused_with_a_message_and_no_launch(hip):
    import coslam_amd
    from coslam_amd.grouping import GroupingCam, camera_grouping_dev, view_overlap_costs_dev

    s = G.planted_scene(6, 2, 200, 1000, 640, 480, [((0, 1), 50, None)])
    d = Dev(s)
    before = (d.vcosts.clone(), d.nShare.clone(), d.groups.clone())
    a = dict(stream_ptr=d.stream, N=s["N"], nMap=s["nMap"], d_mapCount=d.mapCount.data_ptr(), d_mapFlags=d.flags.data_ptr(), W=640, H=480,
             d_vcosts=d.vcosts.data_ptr(), d_nShare=d.nShare.data_ptr(), d_scratch=d.scratch.data_ptr())
    one = dict(xy=d.xy[0].data_ptr(), R=d.R[0].data_ptr(), t=d.t[0].data_ptr())
    for cams in ((GroupingCam * 0)(), [one] * 17):
        with pytest.raises(coslam_amd.CoslamHipError, match="cameras"):
            view_overlap_costs_dev(cams=cams, d_pointFeat=d.pf.data_ptr(), **a)
        with pytest.raises(coslam_amd.CoslamHipError, match="cameras"):
            camera_grouping_dev(cams=cams, d_pointFeat=d.pf.data_ptr(), initCamTranslation=1.0, d_groups=d.groups.data_ptr(), **a)
    with pytest.raises(coslam_amd.CoslamHipError, match="null"):
        view_overlap_costs_dev(cams=d.cams, d_pointFeat=0, **a)
    with pytest.raises(coslam_amd.CoslamHipError, match="null"):
        view_overlap_costs_dev(cams=d.cams, d_pointFeat=d.pf.data_ptr(), **dict(a, d_vcosts=0))
    with pytest.raises(coslam_amd.CoslamHipError, match="null"):
        view_overlap_costs_dev(cams=d.cams, d_pointFeat=d.pf.data_ptr(), **dict(a, d_scratch=0))
    with pytest.raises(coslam_amd.CoslamHipError, match="null"):
        camera_grouping_dev(cams=d.cams, d_pointFeat=d.pf.data_ptr(), initCamTranslation=1.0, d_groups=0, **a)
    with pytest.raises(coslam_amd.CoslamHipError, match="null"):
        camera_grouping_dev(cams=[one, dict(one, xy=0)], d_pointFeat=d.pf.data_ptr(), initCamTranslation=1.0, d_groups=d.groups.data_ptr(), **a)
    import torch

    torch.cuda.synchronize()
    assert torch.equal(before[0], d.vcosts) and torch.equal(before[1], d.nShare) and torch.equal(before[2], d.groups)   # nothing ran


# ---- both frame loops with the step switched on (the headline configuration) ---------------------------------------------------------------
def _setup():
    import torch

    import bench

    dev = torch.device("cuda", 0)
    frames = bench.render_video(list(range(bench.N_CAMS)), bench.N_FRAMES)
    video = {c: torch.from_numpy(frames[c]).to(dev) for c in range(bench.N_CAMS)}
    return bench, bench.build_scene(), video, frames


def _loop(bench, sc, video, **kw):
    from coslam_amd.frameloop import FrameLoop, LoopConfig

    cfg = LoopConfig(n_cams=bench.N_CAMS, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                     n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG, **kw)
    loop = FrameLoop(cfg, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0,
                     associate=bench.associate)
    loop.first_frame()
    return loop


def _run_python_loop(bench, sc, video, n_frames, check_every=0, **kw):
    """n_frames of the loop; at every check_every-th frame the tables the grouping reads are copied to the host right in front of its launch
    (a wait of the test's, at those frames only), and what the loop recorded for that frame is required to equal the restatement over them"""
    loop = _loop(bench, sc, video, **kw)
    cfg, NA, N = loop.cfg, loop.cfg.n_cams, loop.cfg.n_feat
    snap, checked = {}, []
    if check_every:
        launch = loop._camera_grouping

        def watched(i, dst):
            if i % check_every == 0:
                loop.pose_s.synchronize()
                snap[i] = dict(pf=loop.d_pf.cpu().numpy(), flags=loop.d_mapflags.cpu().numpy(), xy=loop.d_xy.cpu().numpy(),
                               count=int(loop.d_mapcount.item()), R=loop.d_R[dst].cpu().numpy(), t=loop.d_t[dst].cpu().numpy())
            launch(i, dst)

        loop._camera_grouping = watched
    for n in range(n_frames):
        i = n + 1
        loop.step(i, n % bench.KEY_EVERY == 0)
        if check_every and i % check_every == 0:
            loop.drain()
            st = loop.grouping_stats()
            s = snap.pop(i)
            assert st["last_frame"] == i and len(st["groups_per_frame"]) == i
            xy = s["xy"].reshape(NA, 2, N).transpose(0, 2, 1)   # x[N] then y[N] -> [N][2]
            r = G.camera_grouping(s["pf"], s["flags"], xy, cfg.W, cfg.H, s["R"], s["t"], st["init_cam_translation"], cfg.group_max_dist_ratio,
                                  cfg.group_min_overlap_num, cfg.group_min_overlap_area_ratio, s["count"], with_area=False)
            assert st["last_groups"] == r["groups"], (i, st["last_groups"], r["groups"])
            assert np.array_equal(np.array(st["last_vcosts"]), r["vcosts"]) and np.array_equal(np.array(st["last_nshare"]), r["nShare"]), i
            assert int(r["nShare"].max()) > 0
            checked.append((i, r["groups"], int(r["nShare"].max())))
    loop.drain()
    st = loop.grouping_stats()
    return loop.digest(), st, checked


@pytest.mark.timeout(1500)
def test_both_loops_group_the_cameras_as_the_restatement_does_and_end_in_the_digest_of_the_run_without_it(hip, tmp_path):
    """The C++ loop with COSLAM_CAMERA_GROUPING=1 and without; the Python loop over the same frames with LoopConfig.camera_grouping, checked
    against the restatement at every 20th frame, and without; the Python loop with every edge cut by distance.  How many groups the orbit
    has at the reference's defaults is recorded (printed), not asserted."""
    bench, sc, video, frames = _setup()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "cxx", "frame_loop.bin")
    assert os.path.exists(exe), "tools/cxx/frame_loop.bin missing: __graft_entry__.build()"
    wl = str(tmp_path / "workload.bin")
    bench.export_workload(wl, sc, frames, bench.build_joint_problem(sc), bench.build_ic_problem(sc), 0)
    del frames
    cxx = {}
    for on in ("1", "0"):
        env = dict(os.environ, COSLAM_CAMERA_GROUPING=on, HSA_KERNARG_POOL_SIZE=str(64 << 20))
        out = subprocess.run([exe, wl, "60", "10", "0", "2"], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        cxx[on] = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    assert cxx["0"]["camera_grouping"] is None
    assert cxx["1"]["digest"] == cxx["0"]["digest"]          # the step only reads loop state
    n_frames = cxx["1"]["frames_run"]
    assert n_frames >= 100
    cg = cxx["1"]["camera_grouping"]
    assert len(cg["groups_per_frame"]) == n_frames

    d_on, st, checked = _run_python_loop(bench, sc, video, n_frames, check_every=20, camera_grouping=True)
    assert len(checked) == n_frames // 20
    d_off, st_off, _ = _run_python_loop(bench, sc, video, n_frames, camera_grouping=False)
    assert st_off is None and d_on == d_off                  # nothing allocated, and the same state
    print("python loop, reference defaults (0, 0.0, 6.0): groups per frame", sorted(set(st["groups_per_frame"])), "last groups", st["last_groups"],
          "frames with more than one group", st["frames_with_more_than_one_group"], "first such frame", st["first_such_frame"],
          "group changes", st["group_changes"], "checked", checked)
    assert len(st["groups_per_frame"]) == n_frames
    assert st["frames_with_more_than_one_group"] == sum(1 for g in st["groups_per_frame"] if g > 1)
    assert cg["groups_per_frame"] == st["groups_per_frame"] and cg["last_groups"] == st["last_groups"]
    assert cg["frames_with_more_than_one_group"] == st["frames_with_more_than_one_group"] and cg["first_such_frame"] == st["first_such_frame"]
    assert cg["group_changes"] == st["group_changes"] and np.array_equal(np.array(cg["last_vcosts"]), np.array(st["last_vcosts"]))

    # every edge cut by distance: nCams singleton groups on every frame
    _, cut, checked = _run_python_loop(bench, sc, video, 60, check_every=20, camera_grouping=True, group_max_dist_ratio=1e-9)
    NA = bench.N_CAMS
    assert cut["groups_per_frame"] == [NA] * 60 and cut["last_groups"] == [[c] for c in range(NA)]
    assert cut["frames_with_more_than_one_group"] == 60 and cut["first_such_frame"] == 1 and cut["group_changes"] == 0
    assert all(n > 0 for _, _, n in checked)                 # (cut although the cameras share points)
