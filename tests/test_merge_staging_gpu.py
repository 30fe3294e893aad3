"""The staging rule of the merge handles (coslam_amd/csrc/dev_arena.h: CsStage) at the three entry points that copy host tables
of the caller's: MergeFront.from_matches (job table, counts, match lists), MergeMatcher.from_pairs with seeds (job table, seed rows) and
MergeConstraints.assemble with a host match list.  A call only enqueues, so its uploads may still read their staging copies when the next
call arrives -- on whatever stream that one runs.  Two calls on two streams with no wait between them, then the first inputs again: every
time the handle must hold, byte for byte, what a fresh handle computes from those inputs alone on the default stream."""
import ctypes

import numpy as np
import pytest

import coslam_amd

pytestmark = pytest.mark.gpu


def _bytes(d):
    return {k: bytes(v) if isinstance(v, ctypes.Structure) else np.asarray(v).tobytes() for k, v in d.items()}


def _front():
    """two cameras, 37 points each, 32 and 20 matches, 50 hypotheses"""
    from tests import mergefront_dev as D
    from tests import mergefront_scenes as S

    sc = S.two_view_scene(24, 8, 0.3, 3)
    dc, keep = D.upload_cams([sc["cam1"], sc["cam2"]])
    X = dict(pairs=[(0, 1)], matches=[sc["matches"]], seed=5)
    Y = dict(pairs=[(1, 0)], matches=[np.ascontiguousarray(sc["matches"][12:, ::-1])], seed=9)

    def call(mf, q, s):
        mf.from_matches(dc, q["pairs"], q["matches"], n_ransac=50, seed=q["seed"], stream_ptr=s)

    return lambda: coslam_amd.MergeFront(2, 64, 64, 1, 50), call, lambda mf: _bytes(D.layers(mf, 0, 0, 50, mf.results(1)[0])), X, Y, keep.clear


def _matcher():
    """nine candidates, two seeds: the seeds' displacement decides which diagonal of the candidates survives the guide"""
    import torch

    from tests import mergematch_dev as D

    N, dev = 8, torch.device("cuda:0")
    x = 50.0 * np.arange(N)
    xy1, xy2 = np.stack([x, np.full(N, 100.0)]), np.stack([x + 3.0, np.full(N, 100.0)])
    cands = [(0, 0, 0.9), (0, 1, 0.8), (1, 1, 0.7), (1, 2, 0.95), (2, 2, 0.6), (2, 3, 0.5), (3, 3, 0.4), (3, 4, 0.3), (4, 4, 0.2)]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    d1, d2 = t(xy1.reshape(-1)), t(xy2.reshape(-1))
    lists = [t(np.frombuffer(D.pair_records(c).tobytes() + b"\0" * 24, np.uint8).copy()) for c in (cands, cands[::-1])]
    n = t(np.array([len(cands)], np.int32))
    X = dict(pairs=lists[0], seeds=np.array([[0.0, 100.0, 3.0, 100.0], [400.0, 100.0, 403.0, 100.0]]))        # keeps (i, i)
    Y = dict(pairs=lists[1], seeds=np.array([[0.0, 100.0, 53.0, 100.0], [400.0, 100.0, 453.0, 100.0]]))      # keeps (i, i + 1)

    def call(mm, q, s):
        mm.from_pairs([q["pairs"].data_ptr()], [n.data_ptr()], [d1.data_ptr()], [d2.data_ptr()], [q["seeds"]], 20.0, stream_ptr=s)

    def read(mm):
        cnt = mm.counts(1)
        m, sc = mm.matches(0, cnt[0][0])
        return _bytes(dict(counts=cnt, matches=m, scores=sc))

    return lambda: coslam_amd.MergeMatcher(1, N, 1, 2, 16, N), call, read, X, Y, lists.clear


def _constraints():
    """the smallest scene of the golden file (3 cameras, 66 slots, 10 matches): all of its matches, and six of them"""
    import torch

    from tests.mergeconstraints_dev import DeviceScene
    from tests.mergeconstraints_golden_util import load

    S, G = load()[0]
    D = DeviceScene(S, torch.device("cuda:0"))
    f1, f2 = int(G["first_frame"]), S["frame0"] + S["nF"] - 1
    X, Y = S["matches"], np.ascontiguousarray(S["matches"][:6][::-1])

    def call(mc, m, s):
        mc.assemble(D.th, D.cams, D.featRef.data_ptr(), S["nMap"], D.M.data_ptr(), D.groups.data_ptr(), S["gId1"], S["gId2"], S["maxiCam"],
                    S["maxjCam"], f1, f2, m, stream_ptr=s)

    make = lambda: coslam_amd.MergeConstraints(S["nC"], S["N"], len(X), S["nMap"])  # noqa: E731
    return make, call, lambda mc: _bytes(dict(mc.problem(), views=mc.views())), X, Y, D.th.close


@pytest.mark.parametrize("case", [_front, _matcher, _constraints])
def test_a_call_on_another_stream_waits_for_the_staged_uploads_of_the_one_before(hip, case):
    import torch

    make, call, read, X, Y, done = case()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()   # the scene's device tables are ready, whatever stream reads them
    h = make()
    call(h, X, s1.cuda_stream)
    call(h, Y, s2.cuda_stream)   # no wait in between: the handle's own rule is all that orders the two
    torch.cuda.synchronize()
    got = {"Y": read(h)}
    call(h, X, s1.cuda_stream)
    torch.cuda.synchronize()
    got["X"] = read(h)
    want = {}
    for name, q in (("Y", Y), ("X", X)):
        fresh = make()
        call(fresh, q, None)
        want[name] = read(fresh)
        fresh.close()
    h.close()
    done()
    assert want["X"] != want["Y"], "the two inputs must tell a stale table from a fresh one"
    for name in ("Y", "X"):
        for k in want[name]:
            assert got[name][k] == want[name][k], (name, k)
