"""include/shim/app/CoSLAMMergeMatch.h (tests/cxx/mergematch_front_shim_test.cpp): matchFeaturePointsNCCFront -- the job's E and seeds from
device memory in the merge front's layout -- gives matchFeaturePointsNCC's Matching bit for bit, and a job the front gave up comes back
empty and flagged.  The program checks itself."""
import struct
import subprocess

import numpy as np
import pytest

from tests import mergematch_ref as R
from tests.cxx_build import build_shim_test

pytestmark = pytest.mark.gpu


def test_cxx_shim_match_feature_points_ncc_front(hip, tmp_path):
    exe = build_shim_test("mergematch_front_shim_test.cpp", tmp_path)
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
    out = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "shim ok" in out.stdout, (out.returncode, out.stdout + out.stderr)
