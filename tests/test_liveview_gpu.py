"""The live view on the device (cs_liveview_*, cs_map_counts_dev; coslam_amd/csrc/liveview.hip) against the line-cited restatement of the
curMapPts rule, CoSLAM::getNumDynamicStaticPoints, CoSLAM::storeDynamicPoints and getDynTracks (tests/liveview_ref.py; reference
src/app/SL_CoSLAM.cpp:1182-1197, :1447-1471, :1900-1911, src/gui/GLScenePane.cpp:19-52).  Everything is compared EXACTLY: the counts and
ids are integers and the coordinates are doubles that the kernels copy and never compute.  Kernel level over planted tables through the
C-ABI, then the shim's driver, then both frame loops with the step switched on."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import liveview_ref as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Dev:
    """planted tables in device memory and a view over them"""

    def __init__(self, s, cur_cap, dyn_cap, depth=2, trail_depth=2, every=1):
        import torch

        from coslam_amd.liveview import LiveView

        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.nC = s["nCams"]
        self.R = self.up(np.arange(9.0 * self.nC).reshape(self.nC, 9) + 0.125)
        self.t = self.up(-np.arange(3.0 * self.nC).reshape(self.nC, 3) - 0.5)
        self.view = LiveView(self.nC, cur_cap, dyn_cap, depth=depth, trail_depth=trail_depth, every=every)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.load(s)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def load(self, s):
        self.s = s
        self.pf, self.flags, self.pts = self.up(s["pointFeat"]), self.up(s["mapFlags"]), self.up(s["mapPts"])
        self.count = self.up(np.array([s["mapCount"]], dtype=np.int32))

    def frame(self, f, groups=None):
        self.view.frame_dev(self.stream, f, self.s["nMap"], self.count.data_ptr(), self.pf.data_ptr(), self.flags.data_ptr(), self.pts.data_ptr(),
                            self.R.data_ptr(), self.t.data_ptr(), groups)

    def expect(self):
        s = self.s
        return L.header_of(s["pointFeat"], s["mapFlags"], s["mapPts"], s["mapCount"], self.view.cur_cap, self.view.dyn_cap)

    def counts_only(self):
        from coslam_amd.liveview import MapCounts, map_counts_dev, map_counts_scratch_bytes

        torch = self.torch
        if not hasattr(self, "scr"):
            self.scr = torch.zeros(map_counts_scratch_bytes(), dtype=torch.uint8, device=self.dev)   # zeroed ONCE
        out = torch.full((C.sizeof(MapCounts),), 7, dtype=torch.uint8, device=self.dev)
        map_counts_dev(self.stream, self.nC, self.s["nMap"], self.count.data_ptr(), self.pf.data_ptr(), self.flags.data_ptr(), out.data_ptr(),
                       self.scr.data_ptr())
        torch.cuda.synchronize()
        assert not self.scr.any().item(), "the call left its scratch dirty"
        return MapCounts.from_buffer_copy(out.cpu().numpy().tobytes()).as_dict(self.nC)


def dyn_tuples(entries):
    return [(int(e["id"]), float(e["x"]), float(e["y"]), float(e["z"])) for e in entries]


def same_frame(d, f, want=None):
    """frame f's snapshot and dynamic list (the newest call's) equal the restatement; returns the snapshot's raw bytes"""
    want = want or d.expect()
    d.torch.cuda.synchronize()
    snap = d.view.snapshot(f)
    cnt = {k: want[k] for k in ("nStatic", "nDynamic", "nStaticFeat", "nDynamicFeat")}
    assert {k: snap[k] for k in cnt} == cnt
    assert d.counts_only() == cnt                               # the counts-only mode of the same kernel
    assert (snap["frame"], snap["mapCount"], snap["nCams"]) == (f, max(0, min(d.s["mapCount"], d.s["nMap"])), d.nC)
    assert (snap["nCur"], snap["curOverflow"], snap["nDyn"], snap["dynOverflow"]) == (want["nCur"], want["curOverflow"], want["nDyn"], want["dynOverflow"])
    p = snap["points"]
    got = [(int(q["id"]), tuple(float(v) for v in q["M"]), int(q["camMask"]), int(q["flags"]), int(q["numVisCam"])) for q in p]
    assert got == want["cur"]                                   # contents and order, camMask, flags, numVisCam; doubles bit for bit
    assert np.array_equal(snap["R"], d.R.cpu().numpy()) and np.array_equal(snap["t"], d.t.cpu().numpy())
    fr, dyn = d.view.dyn_list(d.stream, 0)
    assert fr == f and dyn_tuples(dyn) == want["dyn"]
    hdr, pts = d.view.fetch(f)
    return bytes(hdr) + pts.tobytes() + dyn.tobytes()


PLANTED_ROWS = (0, 63, 64, 255, 256, 1023, 1024, 2499)


@pytest.mark.timeout(120)
def test_order_across_workgroups_every_count_and_two_calls_give_the_same_bytes(hip):
    s = L.planted(11, 8, 2500, 2300, rows=PLANTED_ROWS)
    part = L.participating(s["pointFeat"], s["mapCount"])
    assert all(r in part for r in PLANTED_ROWS[:-1]) and 2499 not in part            # 2499 looks as if it took part: it is behind the count
    assert (s["pointFeat"][2300:] >= 0).any() and 700 < len(part) < 1200
    d = Dev(s, cur_cap=4096, dyn_cap=2048)
    want = d.expect()
    assert want["curOverflow"] == 0 and want["dynOverflow"] == 0 and want["nDyn"] > 100
    assert {p[3] for p in want["cur"]} == set(range(8))                              # every flag combination takes part
    d.frame(0)
    a = same_frame(d, 0, want)
    d.frame(1)
    b = same_frame(d, 1, want)
    strip = lambda raw: raw[4:]   # noqa: E731  (the header's first word is the frame number)
    assert strip(a) == strip(b)


@pytest.mark.timeout(120)
def test_sixteen_cameras_reach_bit_15_and_the_last_camera_s_counts(hip):
    s = L.planted(12, 16, 70, 70, rows=(0, 63, 64, 69))
    s["pointFeat"][69, 15] = 5
    s["mapFlags"][69] = 0
    d = Dev(s, cur_cap=128, dyn_cap=64)
    want = d.expect()
    assert want["cur"][-1][0] == 69 and want["cur"][-1][2] & 0x8000 and want["nStaticFeat"][15] > 0
    d.frame(0)
    same_frame(d, 0, want)


@pytest.mark.timeout(120)
def test_two_cameras_one_point_and_the_empty_map(hip):
    one = dict(nCams=2, nMap=1, mapCount=1, pointFeat=np.array([[-1, 3]], np.int32), mapFlags=np.array([1], np.uint8),
               mapPts=np.array([[1.5, -2.25, 1e300]]))
    d = Dev(one, cur_cap=4, dyn_cap=4)
    d.frame(0)
    same_frame(d, 0)
    assert d.expect()["dyn"] == [(0, 1.5, -2.25, 1e300)]
    d.load(dict(one, mapCount=0))                                # a table with rows, and no map point
    d.frame(1)
    same_frame(d, 1)
    assert d.view.snapshot(1)["nCur"] == 0 and d.view.snapshot(1)["nStatic"] == 0
    e = Dev(dict(one, nMap=0, mapCount=0), cur_cap=4, dyn_cap=4)   # nMap = 0: the tables are never read
    e.frame(0)
    same_frame(e, 0)
    assert e.view.trails(e.stream, 1) == []


@pytest.mark.timeout(120)
def test_one_camera_has_no_dynamic_list_while_dynamic_current_points_exist(hip):
    s = L.planted(13, 1, 300, 290, rows=(0, 255, 256))
    d = Dev(s, cur_cap=512, dyn_cap=64)
    want = d.expect()
    assert want["nDynamic"] > 10 and want["dyn"] == [] and want["nCur"] > 50
    d.frame(0)
    same_frame(d, 0, want)
    assert d.view.trails(d.stream, 1) == []


def caps_tables(nC=2):
    rows = [((0, 1), 1)] * 9 + [((1,), 0)] * 11
    pf = np.full((len(rows), nC), -1, np.int32)
    flags = np.zeros(len(rows), np.uint8)
    for r, (cams, fl) in enumerate(rows):
        pf[r, list(cams)] = r
        flags[r] = fl
    return dict(nCams=nC, nMap=len(rows), mapCount=len(rows), pointFeat=pf, mapFlags=flags, mapPts=np.arange(60.0).reshape(20, 3) + 0.5)


@pytest.mark.timeout(120)
def test_past_a_cap_the_first_entries_are_kept_the_rest_counted_and_the_next_slots_left_alone(hip):
    small = dict(caps_tables(), mapCount=3)                      # 3 current points, all dynamic: fits
    d = Dev(small, cur_cap=8, dyn_cap=4, depth=2, trail_depth=2)
    d.frame(0)
    same_frame(d, 0)
    d.frame(1)                                                   # snapshot slot 1, dynamic slot 1
    same_frame(d, 1)
    ring1 = d.view.ring_bytes()
    sb = d.view.rings()["slot_bytes"]
    fr1, dyn1 = d.view.dyn_list(d.stream, 0)
    d.load(caps_tables())                                        # 20 current points for 8 slots, 9 dynamic ones for 4
    want = d.expect()
    assert (want["nCur"], want["curOverflow"], want["nDyn"], want["dynOverflow"]) == (8, 12, 4, 5)
    assert [p[0] for p in want["cur"]] == list(range(8)) and [q[0] for q in want["dyn"]] == [0, 1, 2, 3]
    d.frame(2)                                                   # slot 0 of both rings: slot 1 lies right behind it
    same_frame(d, 2, want)
    snap = d.view.snapshot(2)
    assert (snap["curOverflowTotal"], snap["dynOverflowTotal"]) == (12, 5)
    ring2 = d.view.ring_bytes()
    assert ring2[sb:] == ring1[sb:] and ring2[:sb] != ring1[:sb]  # the following slot's header and list are untouched
    fr, dyn = d.view.dyn_list(d.stream, 1)
    assert fr == fr1 == 1 and dyn.tobytes() == dyn1.tobytes()    # ... and so is the following slot of the device ring


def run_sequence(d, seq):
    lists = []
    for f, s in enumerate(seq):
        d.load(s)
        d.frame(f)
        lists.append(L.store_dynamic_points(s["pointFeat"], s["mapFlags"], s["mapPts"], s["mapCount"]))
    return lists


def trail_tuples(trails):
    return [(pid, [tuple(float(v) for v in p) for p in pts]) for pid, pts in trails]


@pytest.mark.timeout(120)
def test_trails_over_a_ring_that_wraps(hip):
    import coslam_amd

    seq = L.trail_sequence(6)
    d = Dev(seq[0], cur_cap=8, dyn_cap=8, depth=2, trail_depth=4)
    assert d.view.trails(d.stream, 3) == []                      # an empty ring
    lists = run_sequence(d, seq)
    held = lists[-4:]                                            # the ring holds trailDepth frames
    A, B, Cc, D = 1, 3, 4, 6
    t4 = L.get_dyn_tracks(held, 4)
    assert [pid for pid, _ in t4] == [A, B, D]                   # C is static at the newest frame: no trail; ascending ids
    assert [len(p) for _, p in t4] == [4, 3, 1]                  # B's gap at frame 4 is skipped; D first appears at the newest frame
    assert any(pid == Cc for pid, *_ in lists[3]) and all(pid != Cc for pid, *_ in lists[5])
    for trj in (0, 3, 4):
        want = L.get_dyn_tracks(held, trj)
        assert want == L.get_dyn_tracks(lists, trj)              # (trjLen <= trailDepth: the frames dropped off the ring are never reached)
        assert trail_tuples(d.view.trails(d.stream, trj)) == want, trj
    with pytest.raises(coslam_amd.CoslamHipError, match="trjLen"):
        d.view.trails(d.stream, 5)
    # the device form into the caller's buffers
    torch = d.torch
    n = torch.full((1,), -7, dtype=torch.int32, device=d.dev)
    ids, lens = torch.zeros(8, dtype=torch.int32, device=d.dev), torch.zeros(8, dtype=torch.int32, device=d.dev)
    pts = torch.zeros((8, 3, 3), dtype=torch.float64, device=d.dev)
    d.view.trails_dev(d.stream, 3, n.data_ptr(), ids.data_ptr(), lens.data_ptr(), pts.data_ptr())
    torch.cuda.synchronize()
    want = L.get_dyn_tracks(held, 3)
    k = int(n.item())
    got = [(int(ids[q]), [tuple(float(v) for v in p) for p in pts[q, :int(lens[q])].cpu().numpy()]) for q in range(k)]
    assert got == want


@pytest.mark.timeout(120)
def test_the_ring_protocol_publishes_every_third_frame_and_names_only_landed_frames(hip):
    import coslam_amd
    from coslam_amd.liveview import LiveHeader

    seq = L.trail_sequence(6) + L.trail_sequence(1)              # frames 0 .. 6
    d = Dev(seq[0], cur_cap=8, dyn_cap=8, depth=2, trail_depth=8, every=3)
    assert d.view.newest() == -1
    r = d.view.rings()
    lists = []
    for f, s in enumerate(seq):
        d.load(s)
        d.frame(f)
        n = d.view.newest()                                      # no wait in front of this: whatever it names must be there already
        if n >= 0:
            assert n % 3 == 0 and n <= f
            hdr = LiveHeader.from_buffer_copy(C.string_at(r["h_ring"] + (n // 3 % 2) * r["slot_bytes"], C.sizeof(LiveHeader)))
            assert hdr.frame == n and hdr.nCams == 2 and hdr.every == 3
        lists.append(L.store_dynamic_points(s["pointFeat"], s["mapFlags"], s["mapPts"], s["mapCount"]))
    d.torch.cuda.synchronize()
    assert d.view.newest() == 6
    for f in (1, 2, 4, 5, 7):                                    # never published
        with pytest.raises(coslam_amd.CoslamHipError, match="not in the ring"):
            d.view.fetch(f)
    with pytest.raises(coslam_amd.CoslamHipError, match="not in the ring"):
        d.view.fetch(0)                                          # overwritten by frame 6 (depth 2)
    for f in (3, 6):
        s = seq[f]
        want = L.header_of(s["pointFeat"], s["mapFlags"], s["mapPts"], s["mapCount"], 8, 8)
        snap = d.view.snapshot(f)
        assert snap["frame"] == f and [int(q["id"]) for q in snap["points"]] == [p[0] for p in want["cur"]] and snap["nDynamic"] == want["nDynamic"]
    for back in range(7):                                        # the dynamic ring took EVERY frame
        fr, dyn = d.view.dyn_list(d.stream, back)
        assert fr == 6 - back and dyn_tuples(dyn) == lists[6 - back]
    assert trail_tuples(d.view.trails(d.stream, 7)) == L.get_dyn_tracks(lists, 7)
    with pytest.raises(coslam_amd.CoslamHipError, match="increase"):
        d.frame(6)


@pytest.mark.timeout(120)
def test_the_groups_record_travels_in_the_header(hip):
    from coslam_amd.grouping import CameraGroups

    s = L.trail_sequence(1)[0]
    d = Dev(s, cur_cap=8, dyn_cap=8)
    g = CameraGroups()
    g.groupNum, g.num[0], g.num[1] = 2, 1, 1
    g.camIds[0][0], g.camIds[1][0], g.groupId[0], g.groupId[1] = 0, 1, 0, 1
    dg = d.up(np.frombuffer(bytes(g), dtype=np.uint8).copy())
    d.frame(0, dg.data_ptr())
    d.frame(1)
    d.torch.cuda.synchronize()
    assert d.view.snapshot(0)["groups"] == [[0], [1]] and bytes(d.view.fetch(0)[0].groups) == bytes(g)
    assert d.view.snapshot(1)["groups"] == [] and not any(bytes(d.view.fetch(1)[0].groups))   # none given: groupNum = 0


@pytest.mark.timeout(120)
def test_the_shim_s_m_dynPts_and_dynTracks_equal_the_restatement(hip):
    exe = os.path.join(ROOT, "tests", "cxx", "liveview_shim_test.bin")
    assert os.path.exists(exe), "tests/cxx/liveview_shim_test.bin missing: __graft_entry__.build()"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    seq = L.trail_sequence(6)
    lists = [L.store_dynamic_points(s["pointFeat"], s["mapFlags"], s["mapPts"], s["mapCount"]) for s in seq]
    assert [[tuple(p) for p in fr] for fr in got["m_dynPts"]] == lists
    for key, trj in (("dynTracks", 4), ("dynTracks3", 3)):
        want = L.get_dyn_tracks(lists[-4:], trj)
        assert [[tuple(p) for p in tr] for tr in got[key]] == [[(pid,) + xyz for xyz in pts] for pid, pts in want]
    c = L.num_dynamic_static_points(seq[5]["pointFeat"], seq[5]["mapFlags"], 8)
    assert {k: got[k] for k in c} == c


# ---- both frame loops with the step switched on (the grouping tests' configuration) ---------------------------------------------------------
def _setup():
    import torch

    import bench

    dev = torch.device("cuda", 0)
    frames = bench.render_video(list(range(bench.N_CAMS)), bench.N_FRAMES)
    video = {c: torch.from_numpy(frames[c]).to(dev) for c in range(bench.N_CAMS)}
    return bench, bench.build_scene(), video, frames


def _python_loop(bench, sc, video, n_frames, **kw):
    """n_frames of the loop; with the live view on, the tables it reads are copied to the host right in front of every launch (a wait of the
    test's) and the frame's dynamic list taken from them by the restatement"""
    from coslam_amd.frameloop import FrameLoop, LoopConfig

    cfg = LoopConfig(n_cams=bench.N_CAMS, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                     n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG, **kw)
    loop = FrameLoop(cfg, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0,
                     associate=bench.associate)
    loop.first_frame()
    seen = []
    if loop.live is not None:
        launch = loop._live_view

        def watched(i, dst):
            loop.pose_s.synchronize()
            seen.append(dict(frame=i, pointFeat=loop.d_pf.cpu().numpy(), mapFlags=loop.d_mapflags.cpu().numpy(), mapPts=loop.d_map.cpu().numpy(),
                             mapCount=int(loop.d_mapcount.item()), R=loop.d_R[dst].cpu().numpy(), t=loop.d_t[dst].cpu().numpy()))
            launch(i, dst)

        loop._live_view = watched
    for n in range(n_frames):
        loop.step(n + 1, n % bench.KEY_EVERY == 0)
    loop.drain()
    return loop, seen


@pytest.mark.timeout(900)
def test_both_loops_publish_what_the_restatement_says_and_end_in_the_digest_of_the_run_without_the_step(hip, tmp_path):
    bench, sc, video, frames = _setup()
    exe = os.path.join(ROOT, "tools", "cxx", "frame_loop.bin")
    assert os.path.exists(exe), "tools/cxx/frame_loop.bin missing: __graft_entry__.build()"
    wl = str(tmp_path / "workload.bin")
    bench.export_workload(wl, sc, frames, bench.build_joint_problem(sc), bench.build_ic_problem(sc), 0)
    del frames
    cxx = {}
    for on in ("1", "0"):
        env = dict(os.environ, COSLAM_LIVE_VIEW=on, COSLAM_CAMERA_GROUPING=on, COSLAM_LIVE_VIEW_EVERY="3", HSA_KERNARG_POOL_SIZE=str(64 << 20))
        out = subprocess.run([exe, wl, "1", "0", "0", "2"], env=env, capture_output=True, text=True, timeout=300)   # (the set-up rounds are the run)
        assert out.returncode == 0, out.stderr[-2000:]
        cxx[on] = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    assert "live_view" not in cxx["0"] and cxx["1"]["digest"] == cxx["0"]["digest"]   # the step only reads loop state
    n_frames = cxx["1"]["frames_run"]
    assert 30 <= n_frames <= 80
    lv = cxx["1"]["live_view"]
    assert lv["frames"] == n_frames and lv["frames_published"] == n_frames // 3 and lv["frame"] == n_frames // 3 * 3

    loop, seen = _python_loop(bench, sc, video, n_frames, live_view=True, camera_grouping=True, live_view_every=3)
    off, _ = _python_loop(bench, sc, video, n_frames)
    assert off.live is None and off.live_snapshot() is None and off.live_stats() is None
    assert loop.digest() == off.digest()
    assert len(seen) == n_frames
    cfg = loop.cfg
    # the last published snapshot against the restatement over the loop's own tables of that frame
    last = n_frames // 3 * 3
    snap, s = loop.live_snapshot(), seen[last - 1]
    assert snap["frame"] == last == s["frame"]
    want = L.header_of(s["pointFeat"], s["mapFlags"], s["mapPts"], s["mapCount"], loop.live.cur_cap, loop.live.dyn_cap)
    for k in ("nCur", "nDyn", "curOverflow", "dynOverflow", "nStatic", "nDynamic", "nStaticFeat", "nDynamicFeat"):
        assert snap[k] == want[k], k
    got = [(int(q["id"]), tuple(float(v) for v in q["M"]), int(q["camMask"]), int(q["flags"]), int(q["numVisCam"])) for q in snap["points"]]
    assert got == want["cur"] and snap["nCur"] > 100 and snap["mapCount"] == s["mapCount"]
    assert np.array_equal(snap["R"], s["R"].reshape(cfg.n_cams, 9)) and np.array_equal(snap["t"], s["t"].reshape(cfg.n_cams, 3))
    assert len(snap["groups"]) >= 1 and sorted(c for g in snap["groups"] for c in g) == list(range(cfg.n_cams))   # the frame's groups record
    # the trails against getDynTracks over every frame's list
    lists = [L.store_dynamic_points(q["pointFeat"], q["mapFlags"], q["mapPts"], q["mapCount"])[:loop.live.dyn_cap] for q in seen]
    for trj in (150, 7):
        assert trail_tuples(loop.live_trails(trj)) == L.get_dyn_tracks(lists[-cfg.live_view_trail_depth:], trj), trj
    st = loop.live_stats()
    print("python loop:", st, "dynamic points per frame (min, max):", min(len(x) for x in lists), max(len(x) for x in lists))
    print("c++ loop:", lv)
    for k in ("frames", "frames_published", "frame", "nCur", "nDyn", "curOverflow", "dynOverflow", "curOverflowTotal", "dynOverflowTotal", "nStatic",
              "nDynamic", "nStaticFeat", "nDynamicFeat", "trails", "longest_trail"):
        assert lv[k] == st[k], k                                 # the C++ report's counts equal the Python loop's for the same run
