"""include/shim/app/CoSLAMSurf.h (tests/cxx/surf_shim_test.cpp): detectSURFPoints(ImgG, Mat_d, vector<float>) with the reference's argument
shapes -- through the handle cached per image size and through a caller-held cs_surf* -- against coslam_amd.Surf on one 160 x 120 texture."""
import struct
import subprocess

import numpy as np
import pytest

import coslam_amd
from tests import surf_scenes as S
from tests.cxx_build import build_shim_test
from tests.test_surf_gpu import upload

pytestmark = pytest.mark.gpu


def test_cxx_shim_detect_surf_points(hip, tmp_path):
    exe = build_shim_test("surf_shim_test.cpp", tmp_path)
    W, H = 160, 120
    img = S.scene(W, H)[0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("2id", W, H, S.THRESHOLD) + img.tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "shim ok" in out.stdout, out.stdout + out.stderr
    raw, off = open(tmp_path / "out.bin", "rb").read(), 0
    t, p = upload([img])
    for dim, upright in ((64, False), (128, True)):
        n, d = struct.unpack_from("2i", raw, off)
        pts = np.frombuffer(raw, np.float64, 2 * n, off + 8).reshape(-1, 2)
        desc = np.frombuffer(raw, np.float32, n * d, off + 8 + 16 * n).reshape(-1, d)
        off += 8 + 16 * n + 4 * n * d
        sf = coslam_amd.Surf(1, W, H, 512, dim_desc=dim)
        sf.enqueue(t, S.THRESHOLD, upright=upright, pitch=p)
        want = sf.keypoints(0)
        live = np.isfinite(want["pts"][:, 0])
        assert d == dim and n == int(live.sum()) > 20
        assert pts.tobytes() == want["pts"][live].tobytes() and desc.tobytes() == want["desc"][live].tobytes()
        sf.close()
    assert off == len(raw)
