"""cs_pose_intracam_batch_dev -- the entry both frame loops solve their cameras through -- against the oracle, problem by problem.

Every problem of a batch has its own calibration, start pose and point count; all padding (rows npts..ptsStride-1 of Ms, ms and
prevErrs) is not-a-number, so a lane that reads a row it does not own poisons its problem; every output array sits between guard
elements.  The cases and the reason they are fit to be compared (tests/test_pose_cases_cpu.py: the oracle agrees with itself on each
when the points are reversed) are in tests/pose_cases.py; the tolerances are those of tests/test_pose_ba_gpu.py.

Measured on the MI355X: in no batch did a problem leave the oracle's iteration path (0 problems on the 1e-6 bound everywhere); the largest
differences were 8.4e-10 in R and 8.1e-9 in t (the options batch), 1.1e-10 / 1.1e-9 in the hand-back chain."""

import numpy as np
import pytest

import coslam_amd
from tests import pose_cases as pc
from tests.pose_batch_dev import check_against_oracle, option, run_batch, solve_by_oracle

pytestmark = pytest.mark.gpu

_built = {}


def _problems(name):
    """(stride, built problems, the oracle's solutions): computed once per batch and shared"""
    if name not in _built:
        stride, cases = pc.BATCHES[name]
        probs = [pc.build(c) for c in cases]
        _built[name] = (stride, probs, solve_by_oracle(probs))
    return _built[name]


@pytest.mark.parametrize("name", list(pc.BATCHES))
def test_batch_matches_oracle_problem_by_problem(hip, name):
    stride, probs, want = _problems(name)
    counts = [len(p[3]) for p in probs]
    # what the batch is there to reach
    if name in ("loop192", "sixteen"):
        assert stride > 64 and min(counts) < stride                   # the 256-thread template with npts < ptsStride ...
    if name == "loop192":
        assert sum(1 for n in counts if n <= 64) >= 5 and 0 in counts  # ... also with one wave's worth of points or fewer, and none
    if name == "wave64":
        assert stride <= 64 and len(probs) > 1 and counts[0] == stride  # the one-wave template, more than one workgroup
    if name == "trips600":
        assert {255, 256, 257, 513, 600} <= set(counts)                 # one trip | two | three
    if name == "lds4096":
        assert stride == 4096 and counts == [4096, 4095]
    if name == "sixteen":
        assert len(probs) == 16 and len(set(counts)) > 8
    got = run_batch(probs, stride)
    check_against_oracle(name, got, want)


@pytest.mark.parametrize("all_out,one_round", [(None, False), (4, False), (4, True)])
def test_previous_errors_are_read_with_the_stride(hip, all_out, one_round):
    """prevErrs[ptsStride * pb + i] seeds the weights.  Problem `all_out` has every previous error >= tau: every weight of its first
    round is 0, the round leaves the start pose as it is (one_round stops there: the start pose bit for bit, err0 == 0), and the next
    rounds take their weights from the residuals like any other problem."""
    stride, probs, _ = _problems("loop192")
    prev = pc.prev_errors(pc.BATCHES["loop192"][1], all_out)
    opts = [option((("maxIterRW", 1),) if one_round and j == all_out else ()) for j in range(len(probs))]
    got = run_batch(probs, stride, prev=prev, opts=opts)
    want = solve_by_oracle(probs, prev=prev, opts=opts)
    check_against_oracle(f"prev{all_out}{'r1' if one_round else ''}", got, want, opts=opts)
    nil = _problems("loop192")[2]
    assert any(np.max(np.abs(w[1] - v[1])) > 1e-9 for w, v in zip(want, nil))   # the previous errors do change the answer
    if all_out is not None:
        assert (prev[all_out] >= pc.TAU).all() and want[all_out][0] and got["ok"][all_out] == 1
        if one_round:
            o = got["opt"][all_out]
            assert o.err0 == 0 and o.err == 0 and o.nIterLM == 0 and o.nIterRW == 1
            assert np.array_equal(got["R"][all_out], probs[all_out][1]) and np.array_equal(got["t"][all_out], probs[all_out][2])
            assert np.array_equal(want[all_out][1], probs[all_out][1])


def test_options_per_problem(hip):
    """optAll[pb] is the problem's own record, in and out: default, one re-weighting round, one LM step per round, lambda0 = 1, and no
    round at all (the start pose comes back).  Every output field against the oracle run with the same record."""
    stride, cases, fields = pc.OPTION_BATCH
    probs = [pc.build(c) for c in cases]
    opts = [option(f) for f in fields]
    want = solve_by_oracle(probs, opts=opts)
    got = run_batch(probs, stride, opts=opts)
    check_against_oracle("options", got, want, opts=opts)
    # the records differ from one another as the settings say
    og = got["opt"]
    assert og[1].nIterRW == 1 and want[1][3].nIterRW == 1 and og[0].nIterRW > 1
    assert og[2].nIterLM <= 1 and og[2].maxIterLM == 1
    assert og[3].maxIterRW == 5 and og[3].nIterRW > 1
    assert og[4].nIterRW == 0 and og[4].errRW == -1 and got["ok"][4] == 1
    assert got["R"][4].tobytes() == np.ascontiguousarray(probs[4][1]).tobytes() and got["t"][4].tobytes() == np.ascontiguousarray(probs[4][2]).tobytes()
    assert want[4][1].tobytes() == got["R"][4].tobytes()


def test_a_failing_solve_among_valid_neighbours(hip):
    """One measurement of one problem is not-a-number: every sum of that problem is, every LM step is rejected until lambda passes 1e18
    (retTypeLM -1 after 21 steps), ok is 0 and R_opt / t_opt are the start pose restored from R_tmp / t_tmp.  Its neighbours -- one of
    them started 0.9 rad and 4 units away -- are solved as if it were not there."""
    stride, cases = pc.FAILURE_BATCH
    good = [pc.build(c) for c in cases]
    probs = list(good)
    f = pc.FAILURE_INDEX
    probs[f] = pc.failing(*good[f])
    assert np.isnan(probs[f][4]).sum() == 1 and not np.isnan(probs[f][4][pc.FAIL_AT - 1]).any()
    want = solve_by_oracle(probs)
    got = run_batch(probs, stride)
    check_against_oracle("failure", got, want)
    o = got["opt"][f]
    assert got["ok"][f] == 0 and o.retTypeLM == -1 and o.nIterLM == 21 and o.nIterRW == 0
    assert want[f][3].retTypeLM == -1 and not want[f][0]
    assert got["R"][f].tobytes() == np.ascontiguousarray(probs[f][1]).tobytes()
    assert got["t"][f].tobytes() == np.ascontiguousarray(probs[f][2]).tobytes()
    assert [int(k) for k in got["ok"]] == [1, 0, 1, 1]
    # the neighbours: the same bytes as in a batch in which the problem is healthy
    ref = run_batch(good, stride)
    for j in range(len(probs)):
        assert (got["raw"][j] == ref["raw"][j]) == (j != f)
    # the far start converged to the true pose (0.3 px noise)
    far = pc.FAR_INDEX
    Rgt, tgt = good[far][5], good[far][6]
    assert np.linalg.norm(good[far][2] - tgt) > 3.0
    assert np.max(np.abs(got["R"][far] - Rgt)) < 1e-3 and np.max(np.abs(got["t"][far] - tgt)) < 1e-2
    # ... and through the host-pointer entry
    K, R0, t0, Ms, ms = probs[f][:5]
    ok, R, t, oh = coslam_amd.intraCamEstimate(K, R0, t0, len(Ms), None, Ms, ms, pc.TAU)
    assert not ok and oh.retTypeLM == -1 and oh.nIterLM == 21 and R.tobytes() == got["R"][f].tobytes() and t.tobytes() == got["t"][f].tobytes()


def test_a_problem_gives_the_same_bytes_wherever_it_stands(hip):
    """Workgroups share nothing: the same problem as workgroup 0 and as workgroup 15, between other neighbours and in front of other
    padding, gives identical bytes in R_opt, t_opt and the record."""
    stride, probs, _ = _problems("sixteen")
    x = probs[3]
    assert 64 < len(x[3]) < stride
    a = run_batch([x] + probs[4:] + probs[:3], stride)                          # x first, not-a-number behind its rows
    b = run_batch(probs[8:] + probs[:3] + probs[4:8] + [x], stride, pad=1e300)    # x last, huge finite numbers behind its rows
    assert a["raw"][0] == b["raw"][15]
    assert a["opt"][0].nIterRW > 1 and a["ok"][0] == 1
    assert a["raw"][1] != a["raw"][0]


@pytest.mark.parametrize("j", [0, 6, 7])
def test_batched_solve_equals_the_host_entry_bit_for_bit(hip, j):
    """More than 64 points at stride 192 run the 256-thread template with one point per lane -- and so does cs_pose_intracam on the
    same problem with ptsStride == npts: identical bytes."""
    stride, probs, _ = _problems("loop192")
    K, R0, t0, Ms, ms = probs[j][:5]
    assert 64 < len(Ms) <= stride
    got = run_batch(probs, stride)
    ok, R, t, o = coslam_amd.intraCamEstimate(K, R0, t0, len(Ms), None, Ms, ms, pc.TAU)
    og = got["opt"][j]
    assert int(ok) == got["ok"][j] and R.tobytes() == got["raw"][j][0] and t.tobytes() == got["raw"][j][1]
    assert bytes(o) == got["raw"][j][2], [(f, getattr(o, f), getattr(og, f)) for f, _ in o._fields_]


def test_batch_argument_checks(hip):
    import torch

    dev = torch.device("cuda:0")
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    opt = torch.from_numpy(np.frombuffer(bytes(option()), dtype=np.uint8).copy()).to(dev)
    p = buf.data_ptr()
    names = ("K", "R0", "t0", "npts", "prev", "Ms", "ms", "R", "t", "opt", "ok")

    def call(nProb=1, stride=8, **null):
        ptr = {k: (opt.data_ptr() if k == "opt" else p + 512 * i) for i, k in enumerate(names)}
        ptr.update({k: 0 for k in null})
        coslam_amd.pose.intraCamEstimate_batch_dev(0, nProb, stride, ptr["K"], ptr["R0"], ptr["t0"], ptr["npts"], ptr["prev"], ptr["Ms"],
                                                   ptr["ms"], pc.TAU, ptr["R"], ptr["t"], ptr["opt"], ptr["ok"])

    call()                       # (npts[0] == 0: a valid, empty problem)
    call(prev=True)              # prevErrs may be null
    torch.cuda.synchronize()
    for kw in (dict(nProb=0), dict(nProb=-1), dict(stride=0), dict(stride=-5), dict(stride=4097)):
        with pytest.raises(coslam_amd.CoslamHipError, match="code -1"):
            call(**kw)
    for k in names:
        if k != "prev":
            with pytest.raises(coslam_amd.CoslamHipError, match="code -1"):
                call(**{k: True})
    call(stride=4096)            # the largest stride is accepted
    torch.cuda.synchronize()
