"""Images into the device-fed matcher: the matcher cameras of tests/surf_scenes.banded_pair() PLANTED on the SURF
restatement's key points -- slot k of a camera is its key point k, the slots behind the count are dead -- with the small images the
oracle's resize gives.  The cover condition of the comparison is asserted here, on the restatements alone.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

from tests import mergematch_ref as MR
from tests import surf_scenes as S

N, SCALE, MIN_MATCHES = 256, 0.3, 10


@functools.lru_cache(maxsize=None)
def build():
    """-> (img1, img2, cams: mergematch_ref cameras [xy [2][N], state, K, imgSmall, imgScale], Ws, Hs, the restatement front's job, the
    restatement matcher's matches).  Asserts that every key point is finite and that the host-fed matcher finds >= 10 matches."""
    import oracle

    img1, r1, img2, r2, job = S.banded_pair()
    W, H = S.E2E_W, S.E2E_H
    Ws, Hs = int(W * SCALE), int(H * SCALE)
    cams = []
    for img, r in ((img1, r1), (img2, r2)):
        n = r["count"]
        assert n <= N and np.isfinite(r["pts"]).all()
        xy = np.zeros((2, N))
        xy[:, :n] = r["pts"].T
        state = np.full(N, -1, np.int32)
        state[:n] = 0
        small = oracle.resize_linear_u8(img, Ws / W, Hs / H)
        assert small.shape == (Hs, Ws)
        cams.append(dict(xy=xy, state=state, K=S.K300().reshape(9), imgSmall=small, imgScale=SCALE))
    ref = MR.match_job(cams, Ws, Hs, dict(iCam=0, jCam=1, E=job["E"], seeds=job["seeds"]))
    assert len(ref["matches"]) >= MIN_MATCHES, len(ref["matches"])
    return img1, img2, cams, Ws, Hs, job, ref["matches"]
