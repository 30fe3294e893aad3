"""k_revisit_rounds in a workgroup of 256 threads: a list of up to 256 rows is walked a row per thread, a longer one in turns with the rows'
state in LDS.  The one launch against the launch-per-step rounds (tests/test_revisit_rounds_gpu.py's PerRound) over the bootstrap frame and
the two behind it, where round 0 lists hundreds of rows, with lists that end just below, at and just above the workgroup's thread count
and with the default capacity.  Both sequences of a frame start from ONE snapshot taken behind the single pass (with a list that
overflows, which points are listed depends on the order of the single pass's appends), every state array is compared after both
(the lists as sets), the points beyond the lists among them.  A launch over an empty round 0 leaves every table as it was, a later round's
count included.  Six frames are rendered: the four the loops step through and the two the tracker reads ahead of them."""
import numpy as np
import pytest

from tests.test_revisit_rounds_gpu import _call, _loop, _snapshot_class, _state

pytestmark = pytest.mark.gpu

N_RENDERED = 6    # frames 0..3 are stepped through, the tracker runs two frames ahead
RR_THREADS = 256  # coslam_amd/csrc/poseupdate.hip
# what _state returns, in its order (checked against its length below: an array added there must be named here)
STATE = ("pointFeat", "map", "cov", "mapFlags", "refStatic", "rv_counts", "fref_counts", "rvcounts", "mergeable", "merge_cache", "rv_reg", "slot",
         "flags", "dist", "m", "var", "slot2map", "featRef", "featRef_linked", "segment_fill", "lists")


def _named(state):
    assert len(state) == len(STATE), "tests/test_revisit_rounds_gpu.py's _state changed: name its arrays in STATE"
    return dict(zip(STATE, state))


@pytest.fixture(scope="module")
def video(hip):
    import torch

    import bench

    frames = bench.render_video(list(range(bench.N_CAMS)), N_RENDERED)
    return {c: torch.from_numpy(frames[c]).to(torch.device("cuda", 0)) for c in range(bench.N_CAMS)}


def _both_ways_class():
    """the existing test's snapshot loop (the rounds BOTH ways from one snapshot of the state behind the single pass: the launch per step first,
    then the state is put back and the one launch runs), keeping every state array of both instead of the lists' counts"""
    import torch

    Snap = _snapshot_class()

    class BothWays(Snap):
        def _decide_fused(self, i, dst, D):
            self._skip_rounds = True
            super(Snap, self)._decide_fused(i, dst, D)   # (PerRound's: the single pass and its advance + refine only)
            self._skip_rounds = False
            o = self.reg_out
            keep = [self.d_pf, *self.d_slot2map, D["att"], self.d_map, self.d_cov, self.d_fref, self.d_rstat, self.d_rv_reg[0], self.d_rvlists,
                    self.d_rvcounts, self.d_rv_visit, self.d_rv_next, o["slot"], o["flags"], o["dist"], o["m"], o["var"], self.d_mergeable,
                    self.d_merge_cache, self.d_rv_counts, self.d_fref_counts, D["scr"], self.d_mapflags]
            torch.cuda.synchronize()   # (the loop's launches run on its own stream, the copies on the current one)
            snap = [t.clone() for t in keep]
            torch.cuda.synchronize()
            self._rounds_old(i, dst, D)
            torch.cuda.synchronize()
            old = _named(_state(self))
            for t, c in zip(keep, snap):
                t.copy_(c)
            torch.cuda.synchronize()
            self._rounds_new(i, dst, D)
            torch.cuda.synchronize()
            self.compared.append((i, old, _named(_state(self))))

    return BothWays


@pytest.mark.timeout(120)
@pytest.mark.parametrize("cap", [RR_THREADS - 1, RR_THREADS, RR_THREADS + 1, 1024])
def test_one_launch_of_256_threads_against_the_launch_per_step_rounds(video, cap):
    lp = _loop(_both_ways_class(), video, cap)
    lp.compared = []
    R = lp.cfg.revisit_rounds
    for i in range(1, 4):
        lp.step(i, False)
    lp.drain()
    assert len(lp.compared) >= 3, "the fused registration did not run on every frame"
    listed = []
    for i, old, new in lp.compared:
        for k in STATE:
            if k == "segment_fill":   # (the segment pools are not among the arrays put back between the two sequences)
                continue
            x, y = old[k], new[k]
            assert np.array_equal(x, y), f"cap {cap}, frame {i}: {k} differs in {int((np.asarray(x) != np.asarray(y)).sum())} entries"
        listed.append(new["rvcounts"][: R + 1].tolist())   # (listed per round, then the points beyond the lists)
    # round 0 listed more rows than the workgroup has threads: the list of 257 and the default one are walked in turns, the points beyond
    # the three short lists are counted (alike in both: compared above)
    assert max(l[0] for l in listed) > RR_THREADS + 1, listed
    if cap < 1024:
        assert listed[-1][R] > 0, listed
    assert any(l[1] > 0 for l in listed), listed   # a second round ran


@pytest.mark.timeout(120)
def test_an_empty_round_zero_leaves_every_table_untouched(video):
    import torch

    from coslam_amd.frameloop import FrameLoop

    class Keep(FrameLoop):
        def _decide_fused(self, i, dst, D):
            self._D, self._last_frame = D, i
            return super()._decide_fused(i, dst, D)

    lp = _loop(Keep, video)
    for i in range(1, 4):
        lp.step(i, False)
    lp.drain()
    # round 0 empty, round 1's count NOT: the launch leaves on round 0's count and must not take up a later round's
    lp.d_rvcounts.zero_()
    lp.d_rvcounts[1] = 5
    lp.d_rvlists.view(-1)[lp.RV_CAP: lp.RV_CAP + 5] = torch.arange(5, dtype=lp.d_rvlists.dtype, device=lp.d_rvlists.device)
    torch.cuda.synchronize()
    before = _named(_state(lp))
    assert before["rvcounts"][1] == 5
    _call(lp)
    torch.cuda.synchronize()
    after = _named(_state(lp))
    for k in STATE:
        assert np.array_equal(before[k], after[k]), f"{k} changed by a launch over an empty list"
