"""All rounds of the second visits of a frame in ONE launch (cs_register_revisit_rounds_dev, k_revisit_rounds) against the launches it replaces:
per round a search, a whole-track mergability, the walks with the next round's list and an advance + refine launch (the fused form the frame
loops ran before).  Two Python loops on the same video from the bootstrap frame on -- the frames where the lists are long -- with the state
compared after every tenth frame (feature references by slot / frame / first frame and whether a segment is linked behind, the lists as sets);
both sequences from one snapshot with lists of 32 rows, so that the points beyond them are counted; an empty round 0 writes nothing; bad
arguments are refused."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _loop(cls, video, cap=None):
    import bench
    from coslam_amd.frameloop import LoopConfig

    NA = bench.N_CAMS
    sc = bench.build_scene()
    cfg = LoopConfig(n_cams=NA, W=bench.W, H=bench.H, levels=bench.LEVELS, fw=bench.FW, fh=bench.FH, pts_stride=bench.PTS_STRIDE,
                     n_col_blk=bench.N_COL_BLK, n_row_blk=bench.N_ROW_BLK, key_every=bench.KEY_EVERY, p_reg=bench.P_REG)
    lp = cls(cfg, sc, video, None, bench.klt_config(), bench.reg_covariances(len(sc.points)), rank=0, world=1, device=0, associate=bench.associate)
    if cap is not None:
        lp.RV_CAP = cap
    lp.first_frame()
    return lp


def _per_round_class():
    """FrameLoop whose fused registration plays the rounds with the launches the one launch replaces, four per round: search, mergability,
    walks, advance + refine (the fused form as it was before; not the COSLAM_FUSED_ROUNDS=0 mode, whose lists are built by launches of their own)"""
    from coslam_amd.frameloop import FrameLoop
    from coslam_amd.register import register_decide_kinds_rounds_dev, register_passes, register_revisit_decide_next_dev, register_search_passes_dev

    class PerRound(FrameLoop):
        def _decide_fused(self, i, dst, D):
            cfg, NA, R, ps, o = self.cfg, self.cfg.n_cams, self.cfg.revisit_rounds, self.pose_s.cuda_stream, self.reg_out
            cap, base = self.RV_CAP, self.d_rvlists.data_ptr()
            D["s2m"] = register_decide_kinds_rounds_dev(ps, NA, cfg.n_feat, self.n_map, 0, o["slot"].data_ptr(), o["flags"].data_ptr(),
                                                        self.d_mergeable.data_ptr(), self.d_mapflags.data_ptr(), self.d_pf.data_ptr(), D["s2m"],
                                                        D["att"].data_ptr(), D["reg"].data_ptr(), D["scr"].data_ptr(), base, cap, R,
                                                        self.d_rvcounts.data_ptr(), self.d_rv_visit.data_ptr(), self.d_rv_next.data_ptr(),
                                                        d_counts=D["cnt"].data_ptr(), device=self.device)

            def adv(lst, n, all_, sel, clr):
                self.pose_upd.feat_ref_advance_refine_dev(ps, self.pu_args, self.n_map, self.d_pf.data_ptr(), i, self.d_fref.data_ptr(),
                                                          self.d_rstat.data_ptr(), lst, n, all_, sel, clr, self.d_map.data_ptr(), self.d_cov.data_ptr(),
                                                          self.sig_pix, d_counts=self.d_fref_counts.data_ptr())

            adv(self.d_curlist.data_ptr(), cfg.p_reg, True, D["reg"].data_ptr(), False)
            if not getattr(self, "_skip_rounds", False):
                self._rounds_old(i, dst, D)

        def _rounds_old(self, i, dst, D):
            cfg, NA, R, ps, o = self.cfg, self.cfg.n_cams, self.cfg.revisit_rounds, self.pose_s.cuda_stream, self.reg_out
            cap, base = self.RV_CAP, self.d_rvlists.data_ptr()

            def adv(lst, n, all_, sel, clr):
                self.pose_upd.feat_ref_advance_refine_dev(ps, self.pu_args, self.n_map, self.d_pf.data_ptr(), i, self.d_fref.data_ptr(),
                                                          self.d_rstat.data_ptr(), lst, n, all_, sel, clr, self.d_map.data_ptr(), self.d_cov.data_ptr(),
                                                          self.sig_pix, d_counts=self.d_fref_counts.data_ptr())

            if not hasattr(self, "_pr_passes"):
                self._pr_passes = [register_passes([dict(self._cur_pass_dict(), P=cap, list=base + 4 * r * cap)]) for r in range(R)]
            cnt = self.d_rvcounts.data_ptr()
            for r in range(R):
                lst = base + 4 * r * cap
                register_search_passes_dev(ps, self.reg_args[dst], cfg.n_feat, cfg.W, cfg.H, self._pr_passes[r], device=self.device)
                self.pose_upd.register_mergability_running_dev(ps, self.pu_args, self.n_map, self.d_map.data_ptr(), self.d_cov.data_ptr(),
                                                               o["slot"].data_ptr(), self.sig_pix, self.d_merge_cache.data_ptr(),
                                                               self.d_mergeable.data_ptr(), tolPix=0.0, d_counts=0, cam0=0, nCamsRun=NA, d_list=lst,
                                                               nList=cap, d_flags=o["flags"].data_ptr())
                more = r + 1 < R
                register_revisit_decide_next_dev(ps, NA, cfg.n_feat, self.n_map, cap, 0, 3, lst, self.d_rv_next.data_ptr(), self.d_rv_visit.data_ptr(),
                                                 o["slot"].data_ptr(), o["flags"].data_ptr(), self.d_mergeable.data_ptr(), self.d_mapflags.data_ptr(),
                                                 self.d_pf.data_ptr(), D["s2m"], D["att"].data_ptr(), self.d_rv_reg[0].data_ptr(), D["scr"].data_ptr(),
                                                 self.d_curlist.data_ptr(), self.d_curcount.data_ptr(), cfg.p_reg, self.d_rv_counts.data_ptr(),
                                                 device=self.device, d_listCount=cnt + 4 * r, d_nextList=lst + 4 * cap if more else 0,
                                                 d_nextCount=cnt + 4 * (r + 1) if more else 0, d_overflow=cnt + 4 * R)
                adv(lst, cap, False, self.d_rv_reg[0].data_ptr(), True)

        def _cur_pass_dict(self):
            p = self.rv_passes[0][0]
            return {n: getattr(p, n) for n, _ in p._fields_}

    return PerRound


def _state(lp):
    # (a reference's `seg` is an index into the camera's pool handed out by an atomic: compared by WHETHER something is linked behind, the pools by
    # their fill -- as tests/test_keyframe_drives_gpu.py does; the lists are compared as sets: their order is the order of the appends)
    fref = lp.d_fref.cpu().numpy()
    o = lp.reg_out
    cap, R = lp.RV_CAP, lp.cfg.revisit_rounds
    lists = lp.d_rvlists.view(-1)[: R * cap].view(R, cap).cpu().numpy()
    arrs = [t.cpu().numpy() for t in (lp.d_pf, lp.d_map, lp.d_cov, lp.d_mapflags, lp.d_rstat, lp.d_rv_counts, lp.d_fref_counts, lp.d_rvcounts,
                                      lp.d_mergeable, lp.d_merge_cache, lp.d_rv_reg[0], o["slot"], o["flags"], o["dist"], o["m"], o["var"])]
    return arrs + [np.stack([x.cpu().numpy() for x in lp.d_slot2map]), fref[:, :, :3], fref[:, :, 3] >= 0, lp.pose_upd.segment_counts()[0],
                   np.sort(lists, axis=1)]


def _video():
    import torch

    import bench

    frames = bench.render_video(list(range(bench.N_CAMS)), bench.N_FRAMES)
    return {c: torch.from_numpy(frames[c]).to(torch.device("cuda", 0)) for c in range(bench.N_CAMS)}


def _run_pair(cap, n_frames):
    import torch

    from coslam_amd.frameloop import FrameLoop

    video = _video()
    A, B = _loop(FrameLoop, video, cap), _loop(_per_round_class(), video, cap)
    for i in range(1, n_frames + 1):
        A.step(i, False), B.step(i, False)
        if i % 10 == 0 or i <= 3:
            torch.cuda.synchronize()
            for k, (x, y) in enumerate(zip(_state(A), _state(B))):
                assert np.array_equal(x, y), f"frame {i}: array {k} differs in {int((x != y).sum())} entries"
    return A, B


@pytest.mark.timeout(600)
def test_one_launch_leaves_the_bytes_of_the_launch_per_step_rounds(hip):
    A, B = _run_pair(None, 110)
    rv = A.d_rv_counts.cpu().tolist()
    assert rv[0] > 0 and rv[1] > 0    # the rounds attached features and registered points (the bootstrap frames: long lists)
    assert A.n_merge_frames == B.n_merge_frames >= 2


def _snapshot_class():
    """FrameLoop whose fused registration, behind the single pass, plays the rounds BOTH ways from one snapshot of the state: the launch per step
    first (what it leaves is kept), then the state is put back and the one launch runs; the loop goes on from the one launch's state"""
    import torch

    from coslam_amd.register import register_revisit_rounds_dev

    PerRound = _per_round_class()

    class Snap(PerRound):
        def _rounds_new(self, i, dst, D):
            cfg, o = self.cfg, self.reg_out
            register_revisit_rounds_dev(self.pose_s.cuda_stream, self.pose_upd, self.reg_args[dst], self.pu_args, cfg.W, cfg.H, self.rv_passes[0],
                                        self.n_map, i, 0, 3, self.d_map.data_ptr(), self.d_cov.data_ptr(), self.sig_pix, 0.0,
                                        self.d_merge_cache.data_ptr(), self.d_mergeable.data_ptr(), self.d_rvlists.data_ptr(), self.d_rvcounts.data_ptr(),
                                        self.RV_CAP, cfg.revisit_rounds, self.d_rv_visit.data_ptr(), self.d_rv_next.data_ptr(), self.d_mapflags.data_ptr(),
                                        self.d_pf.data_ptr(), D["s2m"], D["att"].data_ptr(), self.d_rv_reg[0].data_ptr(), D["scr"].data_ptr(),
                                        self.d_curlist.data_ptr(), self.d_curcount.data_ptr(), cfg.p_reg, self.d_rv_counts.data_ptr(), self.d_fref.data_ptr(),
                                        d_refStatic=self.d_rstat.data_ptr(), d_frefCounts=self.d_fref_counts.data_ptr())

        def _decide_fused(self, i, dst, D):
            R = self.cfg.revisit_rounds
            self._skip_rounds = True
            super()._decide_fused(i, dst, D)   # (the single pass and its advance + refine only)
            self._skip_rounds = False
            o = self.reg_out
            keep = [self.d_pf, self.d_slot2map, D["att"], self.d_map, self.d_cov, self.d_fref, self.d_rstat, self.d_rv_reg[0], self.d_rvlists,
                    self.d_rvcounts, self.d_rv_visit, self.d_rv_next, o["slot"], o["flags"], o["dist"], o["m"], o["var"], self.d_mergeable,
                    self.d_merge_cache, self.d_rv_counts, self.d_fref_counts, D["scr"]]
            torch.cuda.synchronize()   # (the loop's launches run on its own stream, the copies on the current one)
            snap = [t.clone() for t in keep]
            torch.cuda.synchronize()
            self._rounds_old(i, dst, D)
            torch.cuda.synchronize()
            old = self.d_rvcounts.cpu().tolist()
            for t, c in zip(keep, snap):
                t.copy_(c)
            torch.cuda.synchronize()
            self._rounds_new(i, dst, D)
            torch.cuda.synchronize()
            new = self.d_rvcounts.cpu().tolist()
            self.compared.append((i, old[: R + 1], new[: R + 1]))

    return Snap


@pytest.mark.timeout(600)
def test_points_beyond_a_short_list_are_counted_alike(hip):
    """lists of 32 rows from the bootstrap frame on: round 0's list overflows.  Both sequences start from ONE snapshot taken behind the single
    pass, so list 0 is the same; round 1's count (appended by round 0's walks inside the one launch) and the points beyond the lists do not
    depend on the order of the appends and are compared exactly.  (Round 1's list is drawn from round 0's listed rows, so it never holds more
    than they do.)"""
    video = _video()
    lp = _loop(_snapshot_class(), video, 32)
    lp.compared = []
    for i in range(1, 11):
        lp.step(i, False)
    lp.drain()
    R = lp.cfg.revisit_rounds
    assert lp.compared, "no fused registration ran"
    for i, old, new in lp.compared:
        assert old == new, (i, old, new)
    assert any(new[0] > 32 for _, _, new in lp.compared) and any(new[1] > 0 for _, _, new in lp.compared), lp.compared   # overflow; round 1 ran
    assert lp.compared[-1][2][R] > 0


def _call(lp, **over):
    from coslam_amd.register import register_revisit_rounds_dev

    cfg, o, i = lp.cfg, lp.reg_out, lp._last_frame
    kw = dict(stream_ptr=lp.pose_s.cuda_stream, history=lp.pose_upd, reg_cams=lp.reg_args[i & 1], pu_cams=lp.pu_args, W=cfg.W, H=cfg.H,
              search_pass=lp.rv_passes[0], nMap=lp.n_map, curFrame=i, mapBase=0, kinds=3, d_mapPts=lp.d_map.data_ptr(), d_mapCov=lp.d_cov.data_ptr(),
              pixelErrVar=lp.sig_pix, tolPix=0.0, d_mergeCache=lp.d_merge_cache.data_ptr(), d_mergeable=lp.d_mergeable.data_ptr(),
              d_rvLists=lp.d_rvlists.data_ptr(), d_rvCounts=lp.d_rvcounts.data_ptr(), cap=lp.RV_CAP, nRounds=cfg.revisit_rounds,
              d_visitLoop=lp.d_rv_visit.data_ptr(), d_nextLoop=lp.d_rv_next.data_ptr(), d_mapFlags=lp.d_mapflags.data_ptr(), d_pointFeat=lp.d_pf.data_ptr(),
              d_slot2map=lp._D["s2m"], d_attached=lp._D["att"].data_ptr(),
              d_regOut=lp.d_rv_reg[0].data_ptr(), d_decideScratch=lp._D["scr"].data_ptr(), d_curList=lp.d_curlist.data_ptr(),
              d_curCount=lp.d_curcount.data_ptr(), curCap=cfg.p_reg, d_rvCnt=lp.d_rv_counts.data_ptr(), d_featRef=lp.d_fref.data_ptr(),
              d_refStatic=lp.d_rstat.data_ptr(), d_frefCounts=lp.d_fref_counts.data_ptr())
    kw.update(over)
    return register_revisit_rounds_dev(**kw)


def _captured_loop():
    """a default loop 40 frames in, with the arguments of its last fused registration kept (lp._D, lp._last_frame)"""
    from coslam_amd.frameloop import FrameLoop

    class Keep(FrameLoop):
        def _decide_fused(self, i, dst, D):
            self._D, self._last_frame = D, i
            return super()._decide_fused(i, dst, D)

    lp = _loop(Keep, _video())
    for i in range(1, 41):
        lp.step(i, False)
    lp.drain()
    return lp


@pytest.mark.timeout(300)
def test_an_empty_round_zero_writes_nothing_and_bad_arguments_are_refused(hip):
    import torch

    from coslam_amd._lib import CoslamHipError

    lp = _captured_loop()
    assert lp._last_frame % 50 != 0
    lp.d_rvcounts.zero_()
    torch.cuda.synchronize()
    before = _state(lp)
    _call(lp)
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(before, _state(lp))):
        assert np.array_equal(x, y), f"array {k} changed by a launch over an empty list"
    bad = [dict(nRounds=0), dict(nRounds=9), dict(cap=0), dict(cap=1025), dict(kinds=0), dict(kinds=4), dict(nMap=0), dict(mapBase=-1),
           dict(tolPix=-1.0), dict(curFrame=lp._last_frame + 1), dict(d_mapPts=lp.d_cov.data_ptr()), dict(d_rvCounts=0), dict(d_featRef=0),
           dict(d_decideScratch=0), dict(d_mergeCache=0), dict(W=0)]
    for b in bad:
        with pytest.raises(CoslamHipError):
            _call(lp, **b)
    p = type(lp.rv_passes[0][0])()
    C.memmove(C.addressof(p), C.addressof(lp.rv_passes[0][0]), C.sizeof(p))
    p.maxDist = 0.0
    with pytest.raises(CoslamHipError):
        _call(lp, search_pass=p)
    torch.cuda.synchronize()
