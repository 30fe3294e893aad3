"""cs_newpts_intracam_dev (k_intracam_newpts_try + k_intracam_newpts_commit) beyond one camera and one commit pass: the
planted scenes of tests/intracam_scenes.py -- 2 to 16 cameras with their own K, 1 to 3 commit passes, a ragged last workgroup, a wrapped
ring, walks over the centre table and the ring, every walk bound, cameras that stood still -- against the C oracle called camera by camera,
bit for bit.  tests/test_intracam_newpts_cpu.py asserts, on the oracle alone, that the scenes hold what these tests need."""
import numpy as np
import pytest

from tests import intracam_scenes as IS

pytestmark = pytest.mark.gpu

BASE = IS.BASE
ROOMY = 4096   # cap - base with room for every scene's points


class Rig:
    """a scene's ring on the device, fed frame by frame with every frame's real pose, and its cameras' tables"""

    def __init__(self, S):
        import torch

        from coslam_amd.poseupdate import TrackHistory

        self.S, self.torch = S, torch
        self.dev = dev = torch.device("cuda:0")
        self.stream = torch.cuda.current_stream().cuda_stream
        nC, N = S["nC"], S["N"]
        d = self.d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
        self.th = TrackHistory(nC, N, S["walk"], storeLen=S["store"])
        self.K, self.iK, self.span, self.fstat = d(S["K"]), d(S["iK"]), d(S["trackSpan"]), d(S["isStatic"])
        fl0 = torch.zeros(64, dtype=torch.uint8, device=dev)
        scr = torch.ones((nC, N), dtype=torch.uint8, device=dev)          # the feed's isStatic (the dynamic test writes it; it is off)
        s2m = torch.full((nC, N), -1, dtype=torch.int32, device=dev)
        keep = []
        for f, R, t, xy, st in IS.frames(S):
            dR, dt, dxy, dst = d(R), d(t), d(xy), d(st)
            keep += [dR, dt, dxy, dst]
            cams = [dict(K=self.row(self.K, c), iK=self.row(self.iK, c), xy=self.row(dxy, c), state=self.row(dst, c), slot2map=self.row(s2m, c),
                         trackSpan=self.row(self.span, c), isStatic=self.row(scr, c)) for c in range(nC)]
            self.th.detect_dynamic_dev(self.stream, cams, dR.data_ptr(), dt.data_ptr(), 64, fl0.data_ptr(), f, minLen=1 << 30)
        torch.cuda.synchronize()
        assert self.th.frames == S["stored"] and self.th.newest_frame == S["cur"]

    @staticmethod
    def row(x, c):
        return x.data_ptr() + c * x.stride(0) * x.element_size()

    def run(self, cap_extra=ROOMY, ready=None, readyMin=1, maxWalk=1024, **bad):
        """one call behind a map of BASE points, every output pre-filled with sentinels -> the arrays on the host.  `bad`: overrides for
        the refusal cases (mapCap, minTrackLen, scratch = None, a camera without isStatic)"""
        torch, dev, S, d = self.torch, self.dev, self.S, self.d
        nC, N = S["nC"], S["N"]
        cap = BASE + cap_extra
        n = max(cap, 1)
        o = dict(M=torch.full((n, 3), 7.0, dtype=torch.float64, device=dev), cov=torch.full((n, 9), 7.0, dtype=torch.float64, device=dev),
                 flags=torch.full((n,), 9, dtype=torch.uint8, device=dev), newPt=torch.full((n,), 9, dtype=torch.uint8, device=dev),
                 first=torch.full((n,), -5, dtype=torch.int32, device=dev), pointFeat=torch.full((n, nC), -9, dtype=torch.int32, device=dev),
                 counts=torch.full((3,), -3, dtype=torch.int32, device=dev), mapCount=torch.tensor([BASE], dtype=torch.int32, device=dev),
                 slot2map=d(S["slot2map"]))
        st = d(S["state"])
        scratch = torch.zeros(self.th.newpts_intracam_scratch_bytes(), dtype=torch.uint8, device=dev)
        d_ready = None if ready is None else torch.tensor(list(ready), dtype=torch.int32, device=dev)
        cams = [dict(K=self.row(self.K, c), iK=self.row(self.iK, c), state=self.row(st, c), slot2map=self.row(o["slot2map"], c),
                     trackSpan=self.row(self.span, c), isStatic=None if bad.get("no_isStatic") == c else self.row(self.fstat, c)) for c in range(nC)]
        self.last = o
        self.th.newpts_intracam_dev(self.stream, cams, o["M"].data_ptr(), o["cov"].data_ptr(), o["flags"].data_ptr(), o["newPt"].data_ptr(),
                                    o["first"].data_ptr(), o["pointFeat"].data_ptr(), bad.get("mapCap", cap), o["mapCount"].data_ptr(),
                                    None if bad.get("no_scratch") else scratch.data_ptr(), IS.SIGMA,
                                    d_ready=None if d_ready is None else d_ready.data_ptr(), readyMin=readyMin,
                                    minTrackLen=bad.get("minTrackLen", IS.MIN_TRACK_LEN), maxWalk=maxWalk, maxEpiErr=IS.MAX_EPI_ERR,
                                    d_counts=o["counts"].data_ptr())
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    def close(self):
        self.th.close()


_rigs = {}


def rig(name):
    """the scene's ring, fed once and shared by the tests (the call reads it only)"""
    if name not in _rigs:
        _rigs[name] = Rig(IS.scene(name))
    return _rigs[name]


def check(S, o, E, cap_extra=ROOMY):
    """every array of a call against the expectation E, of which the first min(A, cap_extra) points are kept"""
    nC, N = S["nC"], S["N"]
    A = len(E["slot"])
    kept = min(A, cap_extra)
    tag = (S["name"], cap_extra, kept, A)
    assert int(o["mapCount"][0]) == BASE + kept, (tag, int(o["mapCount"][0]))
    assert o["counts"].tolist() == [E["candidates"], kept, A - kept], (tag, o["counts"].tolist())
    lo, hi = BASE, BASE + kept
    assert np.array_equal(o["M"][lo:hi], E["M"][:kept]) and np.array_equal(o["cov"][lo:hi], E["cov"][:kept]), tag
    assert np.array_equal(o["first"][lo:hi], E["first"][:kept]), tag
    assert (o["flags"][lo:hi] == 0).all() and (o["newPt"][lo:hi] == 1).all(), tag
    pf = np.full((kept, nC), -1, np.int32)
    pf[np.arange(kept), E["camera"][:kept]] = E["slot"][:kept]
    assert np.array_equal(o["pointFeat"][lo:hi], pf), tag
    s2m = S["slot2map"].copy()
    s2m[E["camera"][:kept], E["slot"][:kept]] = BASE + np.arange(kept)
    assert np.array_equal(o["slot2map"], s2m), tag
    for rows in (slice(0, lo), slice(hi, None)):
        assert (o["M"][rows] == 7.0).all() and (o["cov"][rows] == 7.0).all() and (o["flags"][rows] == 9).all() and (o["newPt"][rows] == 9).all(), tag
        assert (o["first"][rows] == -5).all() and (o["pointFeat"][rows] == -9).all(), tag
    return kept


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("name", ["three", "two_pass", "ragged", "sixteen", "wrapped", "deep", "still"])
def test_scene_reproduces_the_oracle_camera_by_camera(name):
    """Every scene with room for all its points: mapCount, counts, the appended rows in (camera, slot) order -- position and covariance
    bit for bit, first frame, static, bNewPt, the slot in the point's own pointFeat column and -1 in every other --, slot2map of the
    right camera only, sentinels everywhere else; and a second call on fresh copies gives the same bytes."""
    S, r = IS.scene(name), rig(name)
    E = IS.expect(S)
    o = r.run()
    assert check(S, o, E) == len(E["slot"]) >= 10
    assert np.isfinite(o["M"]).all() and np.isfinite(o["cov"]).all()
    assert same_bytes(o, r.run())


@pytest.mark.parametrize("ready,readyMin", [([0, 2, 1], 1), ([0, 2, 1], 2), ([0, 0, 0], 1)])
def test_three_cameras_only_the_ready_ones_contribute(ready, readyMin):
    """d_ready as the loop passes it (the key-frame codes) with readyMin 1 and 2: a camera below readyMin adds no point, no candidate
    count, and its slot2map stays as given."""
    S, r = IS.scene("three"), rig("three")
    E = IS.expect(S, ready=ready, readyMin=readyMin)
    o = r.run(ready=ready, readyMin=readyMin)
    check(S, o, E)
    for c in range(S["nC"]):
        if ready[c] < readyMin:
            assert np.array_equal(o["slot2map"][c], S["slot2map"][c]) and (E["camera"] == c).sum() == 0
    assert same_bytes(o, r.run(ready=ready, readyMin=readyMin))


def test_two_passes_capacity_cut_on_either_side_of_the_pass_boundary():
    """two_pass (1024 + 576 entries): room for 0, 1, a1 - 1, a1, a1 + 1, A - 1, A, A + 1 points, a1 the successes of pass 1 and A all of
    them -- the kept points are always the first of the (camera, slot) order, the rest is counted as dropped and leaves no trace."""
    S, r = IS.scene("two_pass"), rig("two_pass")
    E = IS.expect(S)
    a1, A = int(IS.per_pass(S, E)[0]), len(E["slot"])
    assert 2 < a1 < A - 2
    for room in (0, 1, a1 - 1, a1, a1 + 1, A - 1, A, A + 1):
        o = r.run(cap_extra=room)
        assert check(S, o, E, cap_extra=room) == min(room, A)
        if room in (a1, A - 1):
            assert same_bytes(o, r.run(cap_extra=room))


@pytest.mark.parametrize("maxWalk", IS.DEEP_WALKS)
def test_deep_walk_bound(maxWalk):
    """deep (jp up to 99; centres of depths < 64 from the table, the others from the ring): every walk bound against the oracle with the
    same bound."""
    S, r = IS.scene("deep"), rig("deep")
    E = IS.expect(S, maxWalk=maxWalk)
    o = r.run(maxWalk=maxWalk)
    assert check(S, o, E) >= 4
    assert same_bytes(o, r.run(maxWalk=maxWalk))


def test_still_cameras_first_of_equal_cosines_and_nothing_from_a_camera_that_never_moved():
    """still: camera 0's widest parallax is a stretch of 70 bit-identical poses -- equal cosines within a lane and across lanes of the
    walk, the first in walk order wins: its points equal the oracle's.  Camera 1 never moved: it adds nothing, and no NaN reaches any
    array.  Camera 2 is the control."""
    S, r = IS.scene("still"), rig("still")
    E = IS.expect(S)
    o = r.run()
    kept = check(S, o, E)
    cam = E["camera"]
    assert (cam == 0).sum() >= 10 and (cam == 1).sum() == 0 and (cam == 2).sum() >= 10
    rows0 = BASE + np.nonzero(cam == 0)[0]
    assert np.array_equal(o["M"][rows0], E["M"][cam == 0]) and np.array_equal(o["cov"][rows0], E["cov"][cam == 0])
    assert np.array_equal(o["slot2map"][1], S["slot2map"][1]) and (o["pointFeat"][BASE:BASE + kept, 1] == -1).all()
    assert not any(np.isnan(o[k]).any() for k in ("M", "cov"))


def test_refusals_carry_a_message_and_launch_nothing():
    """mapCap < 1, maxWalk < 2, minTrackLen < 1, a null scratch, a camera with a null isStatic, a history without a frame: an error with
    a message, and every output array -- counts and mapCount included -- still holds what it held."""
    from coslam_amd._lib import CoslamHipError
    from coslam_amd.poseupdate import TrackHistory

    S, r = IS.scene("three"), rig("three")

    def refused(who, words, **kw):
        with pytest.raises(CoslamHipError) as ei:
            who.run(**kw)
        assert "cs_newpts_intracam_dev" in str(ei.value) and words in str(ei.value), str(ei.value)
        r.torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in who.last.items()}
        assert (o["M"] == 7.0).all() and (o["cov"] == 7.0).all() and (o["flags"] == 9).all() and (o["newPt"] == 9).all()
        assert (o["first"] == -5).all() and (o["pointFeat"] == -9).all() and (o["counts"] == -3).all() and int(o["mapCount"][0]) == BASE
        assert np.array_equal(o["slot2map"], S["slot2map"])

    refused(r, "bad arguments", mapCap=0)
    refused(r, "bad arguments", mapCap=-4)
    refused(r, "bad arguments", maxWalk=1)
    refused(r, "bad arguments", minTrackLen=0)
    refused(r, "bad arguments", no_scratch=True)
    refused(r, "null pointer in camera 1", no_isStatic=1)
    empty = Rig.__new__(Rig)
    empty.__dict__.update(r.__dict__)
    empty.th = TrackHistory(S["nC"], S["N"], S["walk"], storeLen=S["store"])
    refused(empty, "no frame")
    empty.th.close()
    # the next good call on the same stream sees the scene as it was
    check(S, r.run(), IS.expect(S))
