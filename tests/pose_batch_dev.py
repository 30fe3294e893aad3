"""cs_pose_intracam_batch_dev on problems of tests/pose_cases.py: the device arrays of a batch (every padding element not-a-number,
guard elements around every output array), the launch, and the comparison with the oracle that tests/test_pose_batch_gpu.py and the
hand-back chain of tests/test_handback_gpu.py share."""
import ctypes as C

import numpy as np

import oracle
from coslam_amd.pose import IntraCamPoseOption, intraCamEstimate_batch_dev
from tests.pose_cases import TAU

GUARD = 16                     # guard elements in front of and behind every output array
R_MARK, OK_MARK, OPT_MARK = -777.25, -77, 0xA5
FLOAT_FIELDS = ("lambda0", "lambda_", "err0", "err", "errRW")
INT_FIELDS = ("retTypeLM", "npts", "nIterLM", "nIterRW")
INPUT_FIELDS = ("maxIterLM", "maxIterRW", "epsErrorChangeLM", "epsParamChangeLM", "epsErrorChangeRW", "verboseLM")


def option(fields=()):
    o = IntraCamPoseOption()
    for k, v in fields:
        setattr(o, k, v)
    return o


def run_batch(problems, stride, prev=None, opts=None, pad=np.nan, stream=None):
    """problems: [(K, R0, t0, Ms, ms, ...)]; prev: None or one float64[npts] per problem; opts: None or one IntraCamPoseOption per
    problem.  Rows npts..stride-1 of Ms, ms and prevErrs hold `pad`.  -> dict(ok int32[n], R [n, 3, 3], t [n, 3], opt [records],
    raw = the bytes of R, t and the records)"""
    import torch

    dev = torch.device("cuda:0")
    n = len(problems)
    Ks = np.stack([np.asarray(p[0], dtype=np.float64).reshape(9) for p in problems])
    R0 = np.stack([np.asarray(p[1], dtype=np.float64).reshape(9) for p in problems])
    t0 = np.stack([np.asarray(p[2], dtype=np.float64).reshape(3) for p in problems])
    npts = np.array([len(p[3]) for p in problems], dtype=np.int32)
    assert npts.max() <= stride
    Ms, ms, pe = np.full((n, stride, 3), pad), np.full((n, stride, 2), pad), np.full((n, stride), pad)
    for j, p in enumerate(problems):
        Ms[j, :npts[j]], ms[j, :npts[j]] = p[3], p[4]
        if prev is not None:
            pe[j, :npts[j]] = prev[j]
    opts = opts or [IntraCamPoseOption() for _ in range(n)]
    opt_in = np.frombuffer(b"".join(bytes(o) for o in opts), dtype=np.uint8)
    ins = [torch.from_numpy(a.copy()).to(dev) for a in (Ks, R0, t0, npts, Ms, ms, pe)]
    d_K, d_R0, d_t0, d_n, d_Ms, d_ms, d_pe = ins
    d_R = torch.full((GUARD + 9 * n + GUARD,), R_MARK, dtype=torch.float64, device=dev)
    d_t = torch.full((GUARD + 3 * n + GUARD,), R_MARK, dtype=torch.float64, device=dev)
    d_ok = torch.full((GUARD + n + GUARD,), OK_MARK, dtype=torch.int32, device=dev)
    d_opt = torch.full((96 * (GUARD + n + GUARD),), OPT_MARK, dtype=torch.uint8, device=dev)
    d_opt[96 * GUARD: 96 * (GUARD + n)] = torch.from_numpy(opt_in.copy()).to(dev)
    s = torch.cuda.current_stream() if stream is None else stream
    intraCamEstimate_batch_dev(s.cuda_stream, n, stride, d_K.data_ptr(), d_R0.data_ptr(), d_t0.data_ptr(), d_n.data_ptr(),
                               d_pe.data_ptr() if prev is not None else 0, d_Ms.data_ptr(), d_ms.data_ptr(), TAU,
                               d_R.data_ptr() + 8 * GUARD, d_t.data_ptr() + 8 * GUARD, d_opt.data_ptr() + 96 * GUARD, d_ok.data_ptr() + 4 * GUARD)
    s.synchronize()
    # nothing outside the n records of an output array is written, and no input is
    for arr, mark, front, size in ((d_R, R_MARK, GUARD, 9 * n), (d_t, R_MARK, GUARD, 3 * n), (d_ok, OK_MARK, GUARD, n),
                                   (d_opt, OPT_MARK, 96 * GUARD, 96 * n)):
        h = arr.cpu().numpy()
        assert len(h) > front + size and (h[:front] == mark).all() and (h[front + size:] == mark).all(), "guard elements written"
    for a, d_a in zip((Ks, R0, t0, npts, Ms, ms, pe), ins):
        assert d_a.cpu().numpy().tobytes() == a.tobytes(), "an input array was written"
    R = d_R.cpu().numpy()[GUARD: GUARD + 9 * n].reshape(n, 3, 3)
    t = d_t.cpu().numpy()[GUARD: GUARD + 3 * n].reshape(n, 3)
    raw_opt = d_opt.cpu().numpy()[96 * GUARD: 96 * (GUARD + n)].tobytes()
    out_opts = [IntraCamPoseOption.from_buffer_copy(raw_opt[96 * j: 96 * j + 96]) for j in range(n)]
    return dict(ok=d_ok.cpu().numpy()[GUARD: GUARD + n].copy(), R=R.copy(), t=t.copy(), opt=out_opts,
                raw=[(R[j].tobytes(), t[j].tobytes(), raw_opt[96 * j: 96 * j + 96]) for j in range(n)])


def solve_by_oracle(problems, prev=None, opts=None):
    """every problem on its own: [(ok, R, t, record)]"""
    return [oracle.intracam_estimate(p[0], p[1], p[2], len(p[3]), None if prev is None else prev[j], p[3], p[4], TAU,
                                     opt=None if opts is None else opts[j]) for j, p in enumerate(problems)]


def _close(a, b, rel):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rel * max(1.0, abs(b))


def check_against_oracle(name, got, want, opts=None, max_loose=1):
    """The assertions of tests/test_pose_ba_gpu.py on every problem of a batch: ok equal, |dR| and |dt| < 1e-6 always; where the
    iteration path is the oracle's, |dR| < 1e-8, |dt| < 1e-7 and every field of the record the oracle's (sums of squared errors to 1e-8
    relative, lambda to rounding, the counters equal).  At most `max_loose` problems of a batch may leave the oracle's iteration path.
    -> (problems on the loose bound, largest |dR|, largest |dt|)"""
    loose, worst_R, worst_t = [], 0.0, 0.0
    for j, (ok_o, R_o, t_o, o_o) in enumerate(want):
        R_g, t_g, o_g = got["R"][j], got["t"][j], got["opt"][j]
        assert bool(got["ok"][j]) == ok_o and got["ok"][j] in (0, 1), (name, j)
        assert o_g.npts == o_o.npts, (name, j)
        o_in = IntraCamPoseOption() if opts is None else opts[j]
        assert all(getattr(o_g, f) == getattr(o_in, f) for f in INPUT_FIELDS), (name, j)   # the settings pass through
        if not ok_o:
            # a failed solve hands back the last accepted pose, and the oracle's record (not-a-number where the oracle's is)
            assert R_g.tobytes() == R_o.tobytes() and t_g.tobytes() == t_o.tobytes(), (name, j)
            assert all(getattr(o_g, f) == getattr(o_o, f) for f in INT_FIELDS), (name, j)
            assert all(_close(getattr(o_g, f), getattr(o_o, f), 1e-12) for f in FLOAT_FIELDS), (name, j)
            continue
        dR, dt = np.max(np.abs(R_g - R_o)), np.max(np.abs(t_g - t_o))
        worst_R, worst_t = max(worst_R, dR), max(worst_t, dt)
        same_path = o_g.nIterRW == o_o.nIterRW and o_g.nIterLM == o_o.nIterLM
        print(f"{name}[{j}]: npts {o_o.npts} dR {dR:.2e} dt {dt:.2e} rounds {o_g.nIterRW}/{o_o.nIterRW} LM {o_g.nIterLM}/{o_o.nIterLM} "
              f"err {o_g.err:.9g}/{o_o.err:.9g}" + ("" if same_path else "   <-- the iteration path differs: 1e-6 bound"))
        assert dR < 1e-6 and dt < 1e-6, (name, j, dR, dt)
        assert np.allclose(R_g @ R_g.T, np.eye(3), rtol=0, atol=1e-9), (name, j)
        if not same_path:
            loose.append(j)
            continue
        assert dR < 1e-8 and dt < 1e-7, (name, j, dR, dt)
        assert o_g.retTypeLM == o_o.retTypeLM, (name, j)
        for f in ("err0", "err", "errRW"):
            assert _close(getattr(o_g, f), getattr(o_o, f), 1e-8), (name, j, f, getattr(o_g, f), getattr(o_o, f))
        for f in ("lambda0", "lambda_"):   # powers of ten away from the start value, along the same accept / reject sequence
            a, b = getattr(o_g, f), getattr(o_o, f)
            assert abs(a - b) <= 1e-12 * abs(b), (name, j, f, a, b)
    print(f"{name}: {len(loose)} of {len(want)} problems on the 1e-6 bound {loose}; largest |dR| {worst_R:.2e}, |dt| {worst_t:.2e}")
    assert len(loose) <= max_loose, (name, loose)
    return loose, worst_R, worst_t
