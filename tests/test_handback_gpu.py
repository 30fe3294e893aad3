"""cs_klt_handback_dev (on-device GPUKLT::addToFeaturePoints + SingleSLAM::chooseStaticFeatPts + the Ms/ms packing of
poseUpdate3D) against the oracle's restatement of those host loops: every output array bit for bit (binary64, same
operation order), over several frames of evolving track state, with and without lens distortion."""
import numpy as np
import pytest

import coslam_amd
import oracle

pytestmark = pytest.mark.gpu

W, H, N, P = 640, 480, 2000, 900


def _frame(rng, prev_status):
    f = np.zeros(N, dtype=coslam_amd.KLT_TrackedFeature)
    # tracked slots mostly stay tracked; some die, dead ones are refilled as new
    r = rng.uniform(size=N)
    st = np.where(prev_status >= 0, np.where(r < 0.9, 0, -1), np.where(r < 0.6, 1, -1)).astype(np.int32)
    f["status"] = st
    f["pos"] = rng.uniform(0.005, 0.995, (N, 2)).astype(np.float32)
    f["gain"] = 1.0
    f["fed"] = -1
    return f


@pytest.mark.parametrize("distort,n_cams", [(False, 1), (True, 3), (False, 8)])
def test_handback_matches_oracle_over_a_sequence(hip, distort, n_cams):
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7 + n_cams)
    K = np.array([[0.82 * W, 0.3, W / 2.0 + 1.5], [0, 0.8 * W, H / 2.0 - 2.0], [0, 0, 1.0]])
    kud = np.zeros(7)
    if distort:
        kud[:3] = [0.08, 0.02, -0.01]   # pushes border points outwards: some land at >= W | H and are dropped
    mapPts = rng.uniform(-5, 5, (P, 3))
    d_K, d_kud, d_map = (torch.from_numpy(a.copy()).to(dev) for a in (K.ravel(), kud, mapPts))
    st_o = [dict(s2m=np.full(N, -1, np.int32), tl=np.full(2 * N, -1, np.int32), xy=np.zeros(2 * N), prev=np.full(N, -1, np.int32),
                 stat=(rng.uniform(size=N) < 0.3).astype(np.uint8)) for _ in range(n_cams)]
    d = [dict(dest=torch.zeros(N * 5, dtype=torch.int32, device=dev), s2m=torch.full((N,), -1, dtype=torch.int32, device=dev),
              tl=torch.full((2 * N,), -1, dtype=torch.int32, device=dev), xy=torch.zeros(2 * N, dtype=torch.float64, device=dev),
              state=torch.zeros(N, dtype=torch.int32, device=dev), selBlk=torch.zeros(192, dtype=torch.int32, device=dev),
              Ms=torch.zeros(192 * 3, dtype=torch.float64, device=dev), ms=torch.zeros(192 * 2, dtype=torch.float64, device=dev),
              sel=torch.zeros(192, dtype=torch.int32, device=dev), npts=torch.zeros(1, dtype=torch.int32, device=dev),
              opt=torch.zeros(96, dtype=torch.uint8, device=dev), stat=torch.from_numpy(st_o[c]["stat"]).to(dev))
         for c in range(n_cams)]
    d_pf = torch.full((P, n_cams), -7, dtype=torch.int32, device=dev)   # P x nCams table, one column per camera
    stream = torch.cuda.current_stream().cuda_stream
    total_dropped = 0
    for frame in range(6):
        feats = []
        for c in range(n_cams):
            f = _frame(rng, st_o[c]["prev"])
            feats.append(f)
            d[c]["dest"].copy_(torch.from_numpy(f.view(np.int32).copy()))
            if frame == 1:   # "map initialisation": associate a third of the live slots with map points, on both sides
                live = np.nonzero(st_o[c]["tl"][:N] >= 0)[0]
                pick = rng.choice(live, size=len(live) // 3, replace=False)
                st_o[c]["s2m"][pick] = rng.integers(0, P, len(pick))
                d[c]["s2m"].copy_(torch.from_numpy(st_o[c]["s2m"]))
        cams = [dict(dest=x["dest"].data_ptr(), K=d_K.data_ptr(), kud=d_kud.data_ptr(), mapPts=d_map.data_ptr(),
                     isStatic=x["stat"].data_ptr(), slot2map=x["s2m"].data_ptr(), trackSpan=x["tl"].data_ptr(),
                     xy=x["xy"].data_ptr(), state=x["state"].data_ptr(), selBlk=x["selBlk"].data_ptr(), Ms=x["Ms"].data_ptr(),
                     ms=x["ms"].data_ptr(), sel=x["sel"].data_ptr(), npts=x["npts"].data_ptr(), opt=x["opt"].data_ptr(),
                     pointFeat=d_pf.data_ptr() + 4 * c, pointFeatStride=n_cams, nPointFeat=P)
                for c, x in enumerate(d)]
        coslam_amd.handback_dev(stream, cams, N, W, H, 16, 12, 192, frame=10 + frame)
        torch.cuda.synchronize()
        for c in range(n_cams):
            o = st_o[c]
            r = oracle.handback(feats[c], W, H, K, kud, mapPts, o["s2m"], o["tl"], o["xy"], 10 + frame, isStatic=o["stat"])
            o["prev"] = np.where(r["state"] == -2, o["prev"], feats[c]["status"]).astype(np.int32)
            g = d[c]
            assert np.array_equal(g["state"].cpu().numpy(), r["state"]), (frame, c)
            assert np.array_equal(g["tl"].cpu().numpy(), o["tl"]) and np.array_equal(g["s2m"].cpu().numpy(), o["s2m"])
            assert np.array_equal(g["xy"].cpu().numpy(), o["xy"]), (frame, c)
            assert np.array_equal(g["selBlk"].cpu().numpy(), r["selBlk"]), (frame, c)
            assert np.array_equal(d_pf[:, c].cpu().numpy(), oracle.point_features(r["state"], o["s2m"], P)), (frame, c)
            n = int(g["npts"].item())
            assert n == r["npts"]
            assert np.array_equal(g["sel"].cpu().numpy()[:n], r["sel"])
            assert np.array_equal(g["Ms"].cpu().numpy().reshape(-1, 3)[:n], r["Ms"])
            assert np.array_equal(g["ms"].cpu().numpy().reshape(-1, 2)[:n], r["ms"])
            opt = np.frombuffer(g["opt"].cpu().numpy().tobytes(), dtype=np.uint8)
            assert np.array_equal(opt, np.frombuffer(bytes(coslam_amd.IntraCamPoseOption()), dtype=np.uint8))
            total_dropped += int((r["state"] == -2).sum())
            if frame >= 2:
                assert n > 20
    if distort:
        assert total_dropped > 0   # the out >= W | H rule was exercised


GUARD, SEL_MARK, F_MARK = 8, -12345, -777.25


def _candidates(o, stat, frame, N):
    """the slots chooseStaticFeatPts votes with (non-empty track; mapped, marked static or born in this frame) -> their indices"""
    f1 = o["tl"][:N]
    return np.nonzero((f1 >= 0) & ((o["s2m"] >= 0) | (stat != 0) | (f1 == frame)))[0]


def _run_edges(Wi, Hi, Ni, n_cams, nCol, nRow, stride, distort=False, n_frames=3, seed=0, pos_hi=0.9999):
    """A sequence like the one above at any shape, every output against the oracle bit for bit, sel / Ms / ms with guard elements behind
    the ptsStride rows.  -> counts of what the edges are about, over all frames and cameras: candidates outside the block grid,
    candidates with a negative coordinate inside (-block, 0) (truncated to block 0) and at or below -block (rejected), the largest
    number of mapped blocks, the smallest / largest npts."""
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1000 + seed)
    K = np.array([[0.82 * Wi, 0.3, Wi / 2.0 + 1.5], [0, 0.8 * Wi, Hi / 2.0 - 2.0], [0, 0, 1.0]])
    kud = np.zeros(7)
    if distort:
        kud[:3] = np.array([0.08, 0.02, -0.01]) * float(distort)    # (True: the distortion of the test above; 2.0: twice that)
    nBlk, blkW, blkH = nCol * nRow, Wi // nCol, Hi // nRow
    mapPts = rng.uniform(-5, 5, (P, 3))
    d_K, d_kud, d_map = (torch.from_numpy(a.copy()).to(dev) for a in (K.ravel(), kud, mapPts))
    st_o = [dict(s2m=np.full(Ni, -1, np.int32), tl=np.full(2 * Ni, -1, np.int32), xy=np.zeros(2 * Ni), prev=np.full(Ni, -1, np.int32),
                 stat=(rng.uniform(size=Ni) < 0.3).astype(np.uint8)) for _ in range(n_cams)]
    i32, f64 = torch.int32, torch.float64
    d = [dict(dest=torch.zeros(Ni * 5, dtype=i32, device=dev), s2m=torch.full((Ni,), -1, dtype=i32, device=dev),
              tl=torch.full((2 * Ni,), -1, dtype=i32, device=dev), xy=torch.zeros(2 * Ni, dtype=f64, device=dev),
              state=torch.zeros(Ni, dtype=i32, device=dev), selBlk=torch.full((nBlk + GUARD,), SEL_MARK, dtype=i32, device=dev),
              Ms=torch.full(((stride + GUARD) * 3,), F_MARK, dtype=f64, device=dev), ms=torch.full(((stride + GUARD) * 2,), F_MARK, dtype=f64, device=dev),
              sel=torch.full((stride + GUARD,), SEL_MARK, dtype=i32, device=dev), npts=torch.full((1 + GUARD,), SEL_MARK, dtype=i32, device=dev),
              opt=torch.zeros(96, dtype=torch.uint8, device=dev), stat=torch.from_numpy(st_o[c]["stat"]).to(dev))
         for c in range(n_cams)]
    d_pf = torch.full((P, n_cams), -7, dtype=i32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    cnt = dict(outside=0, neg_kept=0, neg_rejected=0, mapped_blocks=0, npts_min=1 << 30, npts_max=0, dropped=0)
    for frame in range(n_frames):
        feats = []
        for c in range(n_cams):
            f = np.zeros(Ni, dtype=coslam_amd.KLT_TrackedFeature)
            r = rng.uniform(size=Ni)
            f["status"] = np.where(st_o[c]["prev"] >= 0, np.where(r < 0.9, 0, -1), np.where(r < 0.6, 1, -1)).astype(np.int32)
            f["pos"] = rng.uniform(0.0005, pos_hi, (Ni, 2)).astype(np.float32)
            f["gain"], f["fed"] = 1.0, -1
            feats.append(f)
            d[c]["dest"].copy_(torch.from_numpy(f.view(np.int32).copy()))
            if frame == 1:   # "map initialisation": two thirds of the live slots get a map point, on both sides
                live = np.nonzero(st_o[c]["tl"][:Ni] >= 0)[0]
                pick = rng.choice(live, size=2 * len(live) // 3, replace=False)
                st_o[c]["s2m"][pick] = rng.integers(0, P, len(pick))
                d[c]["s2m"].copy_(torch.from_numpy(st_o[c]["s2m"]))
        cams = [dict(dest=x["dest"].data_ptr(), K=d_K.data_ptr(), kud=d_kud.data_ptr(), mapPts=d_map.data_ptr(),
                     isStatic=x["stat"].data_ptr(), slot2map=x["s2m"].data_ptr(), trackSpan=x["tl"].data_ptr(),
                     xy=x["xy"].data_ptr(), state=x["state"].data_ptr(), selBlk=x["selBlk"].data_ptr(), Ms=x["Ms"].data_ptr(),
                     ms=x["ms"].data_ptr(), sel=x["sel"].data_ptr(), npts=x["npts"].data_ptr(), opt=x["opt"].data_ptr(),
                     pointFeat=d_pf.data_ptr() + 4 * c, pointFeatStride=n_cams, nPointFeat=P)
                for c, x in enumerate(d)]
        coslam_amd.handback_dev(stream, cams, Ni, Wi, Hi, nCol, nRow, stride, frame=10 + frame)
        torch.cuda.synchronize()
        for c in range(n_cams):
            o, g = st_o[c], d[c]
            r = oracle.handback(feats[c], Wi, Hi, K, kud, mapPts, o["s2m"], o["tl"], o["xy"], 10 + frame, isStatic=o["stat"],
                                nColBlk=nCol, nRowBlk=nRow, ptsStride=stride)
            o["prev"] = np.where(r["state"] == -2, o["prev"], feats[c]["status"]).astype(np.int32)
            key = (frame, c)
            assert np.array_equal(g["state"].cpu().numpy(), r["state"]), key
            assert np.array_equal(g["tl"].cpu().numpy(), o["tl"]) and np.array_equal(g["s2m"].cpu().numpy(), o["s2m"]), key
            assert np.array_equal(g["xy"].cpu().numpy(), o["xy"]), key
            selBlk = g["selBlk"].cpu().numpy()
            assert np.array_equal(selBlk[:nBlk], r["selBlk"]) and (selBlk[nBlk:] == SEL_MARK).all(), key
            assert np.array_equal(d_pf[:, c].cpu().numpy(), oracle.point_features(r["state"], o["s2m"], P)), key
            npts = g["npts"].cpu().numpy()
            n = int(npts[0])
            assert n == r["npts"] and (npts[1:] == SEL_MARK).all(), key
            sel, Ms, ms = g["sel"].cpu().numpy(), g["Ms"].cpu().numpy().reshape(-1, 3), g["ms"].cpu().numpy().reshape(-1, 2)
            assert np.array_equal(sel[:n], r["sel"]) and np.array_equal(Ms[:n], r["Ms"]) and np.array_equal(ms[:n], r["ms"]), key
            # nothing behind the ptsStride rows is written (and nothing behind the n selected ones)
            assert (sel[n:] == SEL_MARK).all() and (Ms[n:] == F_MARK).all() and (ms[n:] == F_MARK).all(), key
            opt = np.frombuffer(g["opt"].cpu().numpy().tobytes(), dtype=np.uint8)
            assert np.array_equal(opt, np.frombuffer(bytes(coslam_amd.IntraCamPoseOption()), dtype=np.uint8)), key
            # what this frame's vote met
            cand = _candidates(o, o["stat"], 10 + frame, Ni)
            x, y = o["xy"][cand], o["xy"][Ni + cand]
            bx, by = np.trunc(x / blkW).astype(np.int64), np.trunc(y / blkH).astype(np.int64)
            cnt["outside"] += int(((bx >= nCol) | (by >= nRow)).sum())
            inside = (bx >= 0) & (by >= 0) & (bx < nCol) & (by < nRow)
            cnt["neg_kept"] += int((inside & ((x < 0) | (y < 0))).sum())
            cnt["neg_rejected"] += int(((bx < 0) | (by < 0)).sum())
            mapped_blocks = int(((r["selBlk"] >= 0) & (o["s2m"][np.maximum(r["selBlk"], 0)] >= 0)).sum())
            assert n == min(mapped_blocks, stride), key
            if mapped_blocks > stride:   # the cut: the first ptsStride mapped blocks in block order
                first = [int(s_) for s_ in r["selBlk"] if s_ >= 0 and o["s2m"][s_] >= 0][:stride]
                assert list(sel[:n]) == first, key
            cnt["mapped_blocks"] = max(cnt["mapped_blocks"], mapped_blocks)
            cnt["npts_min"], cnt["npts_max"] = min(cnt["npts_min"], n), max(cnt["npts_max"], n)
            cnt["dropped"] += int((r["state"] == -2).sum())
            # the selected slots are a subset of the candidates inside the grid: a rejected slot is never selected
            assert set(r["selBlk"][r["selBlk"] >= 0]) <= set(cand[inside]), key
            # the sel / Ms / ms rows are reset for the next frame's guard check
            g["sel"].fill_(SEL_MARK), g["Ms"].fill_(F_MARK), g["ms"].fill_(F_MARK)
    return cnt


def test_handback_ragged_image_rejects_slots_outside_the_block_grid(hip):
    """322 x 250 with 16 x 12 blocks: blocks of 20 x 20 cover 320 x 240; a live slot at x >= 320 or y >= 240 is in no block
    (bx >= nColBlk || by >= nRowBlk)."""
    cnt = _run_edges(322, 250, 2000, 2, 16, 12, 192, seed=1)
    assert cnt["outside"] > 0 and cnt["npts_max"] > 20


def test_handback_grid_that_exactly_covers_the_image(hip):
    """101 x 67 with 5 x 3 blocks: 20 x 22 px blocks cover 100 x 66, all but the last pixel column and row; 100 x 66 is covered exactly
    (a point at >= W | H is dropped before the vote: nothing can be outside the grid)."""
    cnt = _run_edges(101, 67, 400, 1, 5, 3, 192, seed=2)
    assert cnt["npts_max"] == 15 and cnt["mapped_blocks"] == 15 and cnt["outside"] > 0
    cnt = _run_edges(100, 66, 400, 1, 5, 3, 192, seed=2)
    assert cnt["npts_max"] == 15 and cnt["mapped_blocks"] == 15 and cnt["outside"] == 0


def test_handback_cuts_the_correspondences_at_pts_stride(hip):
    """ptsStride 32 against about 150 mapped blocks: npts == 32, the first 32 in block order, nothing behind row 32."""
    cnt = _run_edges(640, 480, 2000, 2, 16, 12, 32, seed=3)
    assert cnt["mapped_blocks"] > 100 and cnt["npts_max"] == 32


def test_handback_largest_grid(hip):
    """32 x 32 = 1024 blocks is the largest grid; 33 x 32 is refused."""
    cnt = _run_edges(640, 480, 2000, 1, 32, 32, 1024, seed=4)
    assert cnt["mapped_blocks"] > 300 and cnt["npts_max"] == cnt["mapped_blocks"]
    with pytest.raises(coslam_amd.CoslamHipError, match="code -1"):
        _run_edges(640, 480, 64, 1, 33, 32, 192, n_frames=1)
    with pytest.raises(coslam_amd.CoslamHipError, match="code -1"):
        _run_edges(640, 480, 64, 1, 16, 12, 0, n_frames=1)        # no room for a correspondence


@pytest.mark.parametrize("n_slots", [70, 1024, 1025])
def test_handback_slot_counts(hip, n_slots):
    """70 slots (most of the 1024 threads idle), exactly one pass of the 1024 threads, one slot into the second pass"""
    cnt = _run_edges(640, 480, n_slots, 1, 16, 12, 192, seed=5 + n_slots)
    assert cnt["npts_max"] > 10


def test_handback_sixteen_cameras_and_seventeen_refused(hip):
    cnt = _run_edges(320, 240, 300, 16, 16, 12, 192, seed=6)
    assert cnt["npts_max"] > 20
    with pytest.raises(coslam_amd.CoslamHipError, match="code -1"):
        _run_edges(320, 240, 64, 17, 16, 12, 192, n_frames=1)


def test_handback_negative_undistorted_coordinates(hip):
    """With the distortion on, points near the left and top borders are pushed to negative pixels.  (int)(x / blkW) truncates toward
    zero: a candidate in (-blkW, 0) votes in block column 0, one at or beyond -blkW is in no block.  20 x 15 px blocks meet both."""
    cnt = _run_edges(640, 480, 2000, 1, 32, 32, 192, distort=2.0, seed=7, pos_hi=0.995)
    assert cnt["neg_kept"] > 0 and cnt["neg_rejected"] > 0 and cnt["dropped"] > 0


def test_handback_feeds_the_batched_pose_solve(hip):
    """Three cameras over four frames, the arrays laid out as coslam_amd/frameloop.py lays them out ([camera][ptsStride] rows): hand-back
    writes Ms / ms / npts / opt of every camera, cs_pose_intracam_batch_dev reads them straight away on the same stream, started from
    the previous frame's poses.  Against oracle.handback followed by oracle.intracam_estimate per camera."""
    import torch

    from coslam_amd.handback import handback_cams
    from coslam_amd.pose import IntraCamPoseOption, intraCamEstimate_batch_dev
    from tests import pose_cases as pc
    from tests.pose_batch_dev import check_against_oracle

    S, want = pc.chain_by_oracle()
    NA, Ni, stride = pc.CHAIN["n_cams"], pc.CHAIN["N"], pc.CHAIN["stride"]
    dev = torch.device("cuda:0")
    i32, f64 = torch.int32, torch.float64
    z = lambda shape, ty, v=0: torch.full(shape if isinstance(shape, tuple) else (shape,), v, dtype=ty, device=dev)   # noqa: E731
    d_Ms, d_ms, d_sel = z((NA, stride, 3), f64, float("nan")), z((NA, stride, 2), f64, float("nan")), z((NA, stride), i32, -1)
    d_npts, d_opt, d_ok = z(NA, i32), z((NA, 96), torch.uint8), z(NA, i32, -1)
    d_K = torch.from_numpy(np.stack([k.reshape(9) for k in S["K"]])).to(dev)
    d_kud, d_map = z(7, f64), torch.from_numpy(S["points"].copy()).to(dev)
    d_R, d_t = [z((NA, 9), f64), z((NA, 9), f64)], [z((NA, 3), f64), z((NA, 3), f64)]
    d_dest, d_s2m, d_tl = z((NA, Ni * 5), i32), z((NA, Ni), i32, -1), z((NA, 2 * Ni), i32, -1)
    d_xy, d_state, d_selBlk = z((NA, 2 * Ni), f64), z((NA, Ni), i32), z((NA, 192), i32)
    cams = handback_cams([dict(dest=d_dest[c].data_ptr(), K=d_K[c].data_ptr(), kud=d_kud.data_ptr(), mapPts=d_map.data_ptr(),
                                                  slot2map=d_s2m[c].data_ptr(), trackSpan=d_tl[c].data_ptr(), xy=d_xy[c].data_ptr(),
                                                  state=d_state[c].data_ptr(), selBlk=d_selBlk[c].data_ptr(), Ms=d_Ms[c].data_ptr(),
                                                  ms=d_ms[c].data_ptr(), sel=d_sel[c].data_ptr(), npts=d_npts[c:c + 1].data_ptr(),
                                                  opt=d_opt[c].data_ptr()) for c in range(NA)])
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    worst = [0.0, 0.0]
    for f in range(pc.CHAIN["n_frames"]):
        src, dst = (f + 1) & 1, f & 1
        with torch.cuda.stream(s):
            d_dest.copy_(torch.from_numpy(np.stack([r.view(np.int32).reshape(-1) for r in S["feats"][f]])).to(dev))
            if f == 1:   # the map is initialised behind frame 0
                d_s2m.copy_(torch.from_numpy(np.stack([np.where(want[0][c]["tl"][:Ni] >= 0, np.arange(Ni), -1).astype(np.int32) for c in range(NA)])).to(dev))
            if f > 0:    # the previous frame's poses are where this frame's solve starts
                d_R[src].copy_(torch.from_numpy(np.stack([S["pose"][f - 1][c][0].reshape(9) for c in range(NA)])).to(dev))
                d_t[src].copy_(torch.from_numpy(np.stack([S["pose"][f - 1][c][1] for c in range(NA)])).to(dev))
            coslam_amd.handback_dev(s.cuda_stream, cams, Ni, pc.W, pc.H, pc.CHAIN["nColBlk"], pc.CHAIN["nRowBlk"], stride, frame=10 + f)
            if f > 0:
                intraCamEstimate_batch_dev(s.cuda_stream, NA, stride, d_K.data_ptr(), d_R[src].data_ptr(), d_t[src].data_ptr(), d_npts.data_ptr(), 0,
                                           d_Ms.data_ptr(), d_ms.data_ptr(), pc.TAU, d_R[dst].data_ptr(), d_t[dst].data_ptr(), d_opt.data_ptr(),
                                           d_ok.data_ptr())
        s.synchronize()
        npts = d_npts.cpu().numpy()
        for c in range(NA):
            w = want[f][c]
            n = w["hb"]["npts"]
            assert npts[c] == n and np.array_equal(d_sel[c].cpu().numpy()[:n], w["hb"]["sel"]), (f, c)
            assert np.array_equal(d_Ms[c].cpu().numpy()[:n], w["hb"]["Ms"]) and np.array_equal(d_ms[c].cpu().numpy()[:n], w["hb"]["ms"]), (f, c)
            assert np.array_equal(d_s2m[c].cpu().numpy(), w["s2m"]) and np.array_equal(d_xy[c].cpu().numpy(), w["xy"]), (f, c)
        if f == 0:
            assert (npts == 0).all()
            continue
        assert 64 < npts.min() and npts.max() < stride          # the loops' case: fewer points than the stride, four waves
        probs = [w["problem"] for w in want[f]]
        sol = [oracle.intracam_estimate(p[0], p[1], p[2], len(p[3]), None, p[3], p[4], pc.TAU) for p in probs]
        raw = d_opt.cpu().numpy().tobytes()
        got = dict(ok=d_ok.cpu().numpy(), R=d_R[dst].cpu().numpy().reshape(NA, 3, 3), t=d_t[dst].cpu().numpy(),
                   opt=[IntraCamPoseOption.from_buffer_copy(raw[96 * c: 96 * c + 96]) for c in range(NA)])
        _, wR, wt = check_against_oracle(f"chain frame {f}", got, sol)
        worst = [max(worst[0], wR), max(worst[1], wt)]
        for c in range(NA):   # ... and it is the pose of this frame (0.3 px noise)
            assert np.max(np.abs(got["R"][c] - S["pose"][f][c][0])) < 2e-3 and np.max(np.abs(got["t"][c] - S["pose"][f][c][1])) < 2e-2
    print(f"chain: largest |dR| {worst[0]:.2e}, |dt| {worst[1]:.2e}")


def test_handback_argument_checks(hip):
    with pytest.raises(coslam_amd.CoslamHipError):
        coslam_amd.handback_dev(0, [dict(dest=1)], N, W, H)          # null pointers in the record
    with pytest.raises(coslam_amd.CoslamHipError):
        coslam_amd.handback_dev(0, [], N, W, H)                      # no cameras
