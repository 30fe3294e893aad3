"""include/shim/app/CoSLAMMergeMatch.h (tests/cxx/mergematch_shim_test.cpp): matchFeaturePointsNCC with the reference's argument shapes --
SURF positions and the inlier Matching in, a Matching of LIST indices out -- against the restatement tests/mergematch_ref.py, bit for bit."""
import struct
import subprocess

import numpy as np
import pytest

from tests import mergematch_ref as R
from tests.cxx_build import build_shim_test

pytestmark = pytest.mark.gpu


def test_cxx_shim_match_feature_points_ncc(hip, tmp_path):
    exe = build_shim_test("mergematch_shim_test.cpp", tmp_path)
    N, WS, HS = 70, 192, 144
    cams, job, _ = R.shifted_pair_scene(N=N, n_cams=3, pair=(2, 0), seed=21)
    ref = R.match_job(cams, WS, HS, job)
    assert len(ref["matches"]) > 20
    # SURF point lists with the seeds somewhere inside, and the inlier Matching that names them
    rng = np.random.default_rng(1)
    ns = len(job["seeds"])
    surf1, surf2 = rng.uniform(0, 600, (ns + 9, 2)), rng.uniform(0, 600, (ns + 5, 2))
    i1, i2 = rng.permutation(ns + 9)[:ns], rng.permutation(ns + 5)[:ns]
    surf1[i1], surf2[i2] = job["seeds"][:, :2], job["seeds"][:, 2:]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("4id", 3, N, WS, HS, cams[0]["imgScale"]))
        for c in cams:
            f.write(np.asarray(c["K"], np.float64).tobytes() + np.ascontiguousarray(c["xy"], np.float64).tobytes())
            f.write(np.asarray(c["state"], np.int32).tobytes() + np.ascontiguousarray(c["imgSmall"], np.uint8).tobytes())
        f.write(struct.pack("2i", job["iCam"], job["jCam"]) + np.asarray(job["E"], np.float64).tobytes())
        f.write(struct.pack("i", len(surf1)) + surf1.tobytes() + struct.pack("i", len(surf2)) + surf2.tobytes())
        f.write(struct.pack("i", ns) + np.stack([i1, i2], 1).astype(np.int32).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "shim ok" in out.stdout, out.stdout + out.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    n, flags, cand, rounds = struct.unpack_from("4i", raw, 0)
    assert (n, flags, cand) == (len(ref["matches"]), 0, len(ref["cands"])) and rounds >= 1
    rec = np.frombuffer(raw, np.dtype([("a", np.int32), ("b", np.int32), ("s", np.float64)]), n, 16)
    slots = np.frombuffer(raw, np.int32, 2 * n, 16 + 16 * n).reshape(-1, 2)
    assert 16 + 16 * n + 8 * n == len(raw)
    rank = [np.cumsum(R.valid_mask(cams[c]["state"])) - 1 for c in (job["iCam"], job["jCam"])]
    want = ref["matches"]
    assert slots.tolist() == [[a, b] for a, b, _ in want]
    assert rec["a"].tolist() == [int(rank[0][a]) for a, _, _ in want] and rec["b"].tolist() == [int(rank[1][b]) for _, b, _ in want]
    assert rec["s"].tobytes() == np.array([s for _, _, s in want]).tobytes()
    assert any(int(rank[0][a]) != a for a, _, _ in want)          # rank != slot: dead slots between live ones
