"""include/shim/app/CoSLAMMergeFront.h (tests/cxx/mergefront_shim_test.cpp): matchSURFPoints and computeEMat with the reference's argument
shapes -- Mat_d point lists, vector<float> descriptors, Matching in and out -- against the restatement tests/mergefront_ref.py on one scene
(a noisy RANSAC case of tests/mergefront_scenes.py, whose cover conditions make the comparison exact)."""
import struct
import subprocess

import numpy as np
import pytest

from tests import mergefront_scenes as S
from tests.cxx_build import build_shim_test

pytestmark = pytest.mark.gpu


def test_cxx_shim_match_surf_points_and_compute_emat(hip, tmp_path):
    exe = build_shim_test("mergefront_shim_test.cpp", tmp_path)
    nt, no, noise, seed, nr, gs = S.NOISY[0]
    sc, exp = S.ransac_case(nt, no, noise, seed, nr, gs)
    a, b = sc["cam1"], sc["cam2"]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("6iQ", 3, 2, 0, 64, nr, 15, gs) + S.K.tobytes() + struct.pack("2i", len(a["pts"]), len(b["pts"])))
        f.write(np.ascontiguousarray(a["pts"], np.float64).tobytes() + np.ascontiguousarray(b["pts"], np.float64).tobytes())
        f.write(np.ascontiguousarray(a["desc"], np.float32).tobytes() + np.ascontiguousarray(b["desc"], np.float32).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "shim ok" in out.stdout, out.stdout + out.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    n, m = struct.unpack_from("2i", raw, 0)
    item = np.dtype([("a", np.int32), ("b", np.int32), ("d", np.float64)])
    matches = np.frombuffer(raw, item, n, 8)
    off = 8 + 16 * n
    E = np.frombuffer(raw, np.float64, 9, off)
    rec = struct.unpack_from("6i", raw, off + 72)
    new = np.frombuffer(raw, item, m, off + 72 + 104)
    seeds = np.frombuffer(raw, np.float64, 4 * m, off + 72 + 104 + 16 * m).reshape(-1, 4)
    assert off + 72 + 104 + 16 * m + 32 * m == len(raw)
    assert n == len(sc["matches"]) and np.array_equal(np.stack([matches["a"], matches["b"]], 1), sc["matches"])
    assert m == exp["inlier_num"] and rec == (n, 1, m, exp["rounds"], exp["best_hyp"], 0)
    assert np.array_equal(np.stack([new["a"], new["b"]], 1), exp["new_matches"]) and seeds.tobytes() == np.ascontiguousarray(exp["seeds"]).tobytes()
    assert np.abs(E * np.sign(E @ exp["E"]) - exp["E"]).max() <= S.E_TOL
