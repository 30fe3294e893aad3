"""Precondition of the pose solve's GPU tests, on the CPU: every committed case of tests/pose_cases.py solved by the oracle with its
points in the given order and in reversed order.  The two runs differ ONLY in the order of the sums over the points -- the one thing the
device's tree sums change against the serial loop -- so a case on which the oracle disagrees with itself says nothing about a kernel.
Such a case gets another seed in tests/pose_cases.py; the bounds below are the tight ones of the GPU tests and stay."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import pose_cases as pc


def _opt(fields):
    o = oracle.PoseOption()
    oracle.lib().okp_option_default(C.byref(o))
    for k, v in fields:
        setattr(o, k, v)
    return o


def _variants():
    """(id, built problem, previous errors or None, option fields)"""
    out = []
    for name, (_, cases) in pc.BATCHES.items():
        out += [(f"{name}[{j}]", pc.build(c), None, ()) for j, c in enumerate(cases)]
    cases = pc.BATCHES["loop192"][1]
    for all_out in (None, 4):
        out += [(f"prev{all_out}[{j}]", pc.build(c), e, ()) for j, (c, e) in enumerate(zip(cases, pc.prev_errors(cases, all_out)))]
    out += [(f"options[{j}]", pc.build(c), None, f) for j, (c, f) in enumerate(zip(pc.OPTION_BATCH[1], pc.OPTION_BATCH[2]))]
    out += [(f"failure[{j}]", pc.build(c), None, ()) for j, c in enumerate(pc.FAILURE_BATCH[1])]
    out.append(("failing", pc.failing(*pc.build(pc.FAIL_CASE)), None, ()))
    out += [(f"host[{c['seed']}-{c['npts']}]", pc.build(c), None, ()) for c in pc.HOST_CASES]
    _, chain = pc.chain_by_oracle()
    out += [(f"chain[{f}][{c}]", x["problem"] + (None, None), None, ()) for f, fr in enumerate(chain) for c, x in enumerate(fr) if x["problem"]]
    return out


def test_every_committed_case_is_in_the_list():
    n_chain = pc.CHAIN["n_cams"] * (pc.CHAIN["n_frames"] - 1)
    assert len(_variants()) == len(pc.ALL_CASES) + 2 * len(pc.BATCHES["loop192"][1]) + 1 + n_chain


def test_oracle_agrees_with_itself_on_reversed_points():
    worst_R = worst_t = 0.0
    bad = []
    for name, (K, R0, t0, Ms, ms, _, _), prev, fields in _variants():
        n = len(Ms)
        a = oracle.intracam_estimate(K, R0, t0, n, prev, Ms, ms, pc.TAU, opt=_opt(fields))
        b = oracle.intracam_estimate(K, R0, t0, n, None if prev is None else prev[::-1].copy(), Ms[::-1].copy(), ms[::-1].copy(), pc.TAU,
                                     opt=_opt(fields))
        dR, dt = np.max(np.abs(a[1] - b[1])), np.max(np.abs(a[2] - b[2]))
        same = a[0] == b[0] and all(getattr(a[3], f) == getattr(b[3], f) for f in ("nIterRW", "nIterLM", "retTypeLM"))
        print(f"{name}: npts {n} dR {dR:.2e} dt {dt:.2e} ok {a[0]} RW {a[3].nIterRW} LM {a[3].nIterLM} ret {a[3].retTypeLM}")
        worst_R, worst_t = max(worst_R, dR), max(worst_t, dt)
        if not (same and dR <= 1e-8 and dt <= 1e-7):
            bad.append((name, dR, dt, same))
    print(f"largest self-difference: R {worst_R:.2e}, t {worst_t:.2e}")
    assert not bad, bad


def test_what_the_gpu_tests_expect_of_the_oracle():
    """the expectations the GPU tests take from the oracle, as the oracle gives them on the CPU"""
    # the failing solve: not-a-number sums reject every step until lambda passes 1e18
    K, R0, t0, Ms, ms, _, _ = pc.failing(*pc.build(pc.FAIL_CASE))
    ok, R, t, o = oracle.intracam_estimate(K, R0, t0, len(Ms), None, Ms, ms, pc.TAU)
    assert not ok and o.retTypeLM == -1 and o.nIterLM == 21 and o.nIterRW == 0
    assert R.tobytes() == np.ascontiguousarray(R0).tobytes() and t.tobytes() == np.ascontiguousarray(t0).tobytes()
    # the far start converges to the true pose
    K, R0, t0, Ms, ms, Rgt, tgt = pc.build(pc.FAR_START)
    assert np.linalg.norm(t0 - tgt) > 3.0
    ang = np.arccos((np.trace(R0.T @ Rgt) - 1) / 2)
    assert 0.8 < ang < 1.0
    ok, R, t, o = oracle.intracam_estimate(K, R0, t0, len(Ms), None, Ms, ms, pc.TAU)
    assert ok and np.max(np.abs(R - Rgt)) < 1e-3 and np.max(np.abs(t - tgt)) < 1e-2
    # maxIterRW = 0 returns the start pose
    o0 = _opt((("maxIterRW", 0),))
    ok, R, t, o = oracle.intracam_estimate(K, R0, t0, len(Ms), None, Ms, ms, pc.TAU, opt=o0)
    assert ok and o.nIterRW == 0 and np.array_equal(R, R0) and np.array_equal(t, t0) and o0.nIterRW == 0
    # every previous error >= tau: every weight 0 in the first round, which therefore stays at the start pose
    cases = pc.BATCHES["loop192"][1]
    prev = pc.prev_errors(cases, 4)
    assert (prev[4] >= pc.TAU).all() and len(prev[4]) == 63 and 0 < (prev[0] >= pc.TAU).sum() < len(prev[0])
    K, R0, t0, Ms, ms, _, _ = pc.build(cases[4])
    o1 = _opt((("maxIterRW", 1),))
    ok, R, t, o = oracle.intracam_estimate(K, R0, t0, len(Ms), prev[4], Ms, ms, pc.TAU, opt=o1)
    assert ok and o.err0 == 0 and o.nIterLM == 0 and np.max(np.abs(R - R0)) == 0 and np.array_equal(t, t0)


@pytest.mark.parametrize("npts", [4096, 4097, 5000, 6000])
def test_large_cases_hold_what_they_ask_for(npts):
    c = next(c for c in pc.HOST_CASES if c["npts"] == npts)
    assert len(pc.build(c)[3]) == npts
