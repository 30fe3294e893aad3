"""include/shim/app/CoSLAMMergeConstraints.h through mergeMapPoints (tests/cxx/mergemap_shim_test.cpp) against coslam_amd.MergeCamGroups on the
same scene: the same kernels and solves on the same inputs, so the tables, the counts and the solved coordinates agree bit for bit; a
rejected verdict leaves every table as it was."""
import struct
import subprocess

import numpy as np
import pytest

import coslam_amd
from tests import mergemap_ref as mref
from tests.cxx_build import build_shim_test
from tests.mergeconstraints_golden_util import load
from tests.mergeconstraints_scenes import write_input
from tests.mergemap_dev import Live

pytestmark = pytest.mark.gpu

SCENES = load()


@pytest.mark.parametrize("sc", (3, 2))
def test_cxx_shim_merge_map_points(hip, tmp_path, sc):
    exe = build_shim_test("mergemap_shim_test.cpp", tmp_path)
    S, G = SCENES[sc]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("i", 1))
        write_input(f, S)
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    ok, verdict, n_info, nMap, nC, N = struct.unpack_from("6i", raw, 0)
    assert (nMap, nC, N) == (S["nMap"], S["nC"], S["N"]) and verdict == int(G["verdict"]) and ok == int(verdict == 1)
    off, got = 24, {}
    for k, dt, n in (("counts", np.int32, 6), ("slot2map", np.int32, nC * N), ("featRef", np.int32, nMap * nC * 4), ("pointFeat", np.int32, nMap * nC),
                     ("refStatic", np.uint8, nMap * nC), ("M", np.float64, 3 * nMap)):
        got[k] = np.frombuffer(raw, dt, n, off)
        off += got[k].nbytes
    assert off == len(raw)
    A = Live(S)
    mg = coslam_amd.MergeCamGroups(S["nC"], S["N"], max(1, len(S["matches"])), S["nMap"])
    rep = A.run(mg)
    a = A.state()
    assert rep["verdict"] == verdict and (rep["status"] == "merged") == bool(ok)
    for k in ("slot2map", "featRef", "pointFeat", "refStatic"):
        assert got[k].tobytes() == a[k].tobytes(), k
    assert got["counts"].tolist() == rep["apply_counts"]
    if ok:
        # MergeCamGroups goes on to re-triangulate the map; the shim's call stops behind the solved coordinates: those of ITS handle
        want = mref.apply_map(A.S, mg.mc.views().tolist(), mg.mc.problem()["pointMap"], mg.mc.solution(1)["pts"])
        assert got["M"].tobytes() == want["M"].tobytes() and n_info == len(G["info_ints"]) and rep["apply_counts"][4] > 0
    else:
        assert got["M"].tobytes() == np.asarray(S["M"], np.float64).tobytes() == a["M"].tobytes() and got["counts"].tolist() == [0] * 6
    mg.close()
    A.close()
