"""Images into the merge chain: coslam_amd.Surf -> MergeFront on the device against tests/surf_ref.py -> tests/mergefront_ref.py.
The scenes (tests/surf_scenes.py) assert on the restatements alone what makes the demands fair: enough matches, nearly all of them on the
planted shift, descriptor decisions 1e-3 away from their thresholds (the descriptor tolerance is 2.4e-7), a stable eight-point solve."""
import numpy as np
import pytest

import coslam_amd
from tests import mergefront_scenes as FS
from tests import surf_scenes as S
from tests.test_surf_gpu import upload

pytestmark = pytest.mark.gpu
MAX_PTS = 256


def test_descriptor_stage_gives_the_restatements_match_list(hip):
    (img1, r1), (img2, r2), want = S.shifted_pair()
    FS.assert_descriptor_cover(want, 0.8, 0.6, r1["desc"])
    sf = coslam_amd.Surf(2, S.E2E_W, S.E2E_H, MAX_PTS)
    mf = coslam_amd.MergeFront(2, MAX_PTS, 64, 1, 8)
    t, p = upload([img1, img2])
    Ks = [S.K300().reshape(9)] * 2
    sf.enqueue(t, S.THRESHOLD, pitch=p)
    mf.match(sf.front_cams(Ks), [(0, 1)])                       # n = max_pts: NaN padding, no wait in between
    n = int(mf.counts(1)[0])
    got = mf.matches(0, n)
    assert n == len(want["matches"]) >= 28 and np.array_equal(got[0], want["matches"])
    assert np.abs(got[1] - want["dist"]).max() <= 1e-5
    cnt = sf.counts()[0]
    assert list(cnt) == [r1["count"], r2["count"]]
    mf.match(sf.front_cams(Ks, counts=cnt), [(0, 1)])           # n = count: the same list
    got2 = mf.matches(0, int(mf.counts(1)[0]))
    assert np.array_equal(got2[0], got[0]) and got2[1].tobytes() == got[1].tobytes()
    sf.close(), mf.close()


def test_whole_front_from_two_images(hip):
    img1, r1, img2, r2, want = S.banded_pair()
    sf = coslam_amd.Surf(2, S.E2E_W, S.E2E_H, MAX_PTS)
    mf = coslam_amd.MergeFront(2, MAX_PTS, 64, 1, S.N_RANSAC)
    t, p = upload([img1, img2])
    sf.enqueue(t, S.THRESHOLD, pitch=p)
    got = mf.run(sf.front_cams([S.K300().reshape(9)] * 2), [(0, 1)], n_ransac=S.N_RANSAC)[0]
    print("front:", {k: got[k] for k in ("surf_num", "emat_ok", "inlier_num", "rounds", "best_hyp")}, "restatement:",
          {k: want[k] for k in ("surf_num", "emat_ok", "inlier_num", "rounds", "best_hyp")})
    assert (got["surf_num"], got["emat_ok"], got["inlier_num"]) == (want["surf_num"], want["emat_ok"], want["inlier_num"])
    assert got["emat_ok"] == 1 and got["inlier_num"] >= 18
    dE = float(np.abs(got["E"] * np.sign(got["E"] @ want["E"]) - want["E"]).max())
    print(f"largest difference of E up to sign: {dE:.3e}")
    assert dE <= FS.E_TOL
    sf.close(), mf.close()
