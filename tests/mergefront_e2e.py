"""The end-to-end scene of the merge front: tests/mergematch_e2e.py's two-group scene with key points and descriptors PLANTED
on the current key frame -- every LIVE slot (state 0 / 1) is a key point of its camera (a point's index is its slot's rank), the two slots of a planted match carry one descriptor (plus noise), every
other slot a descriptor of its own; cameras 1 and 2 share 30 descriptors between slots that have nothing to do with each other (enough SURF
matches, no essential matrix).  The cover conditions of the comparison are asserted here, on the restatement alone."""
import functools

import numpy as np

from tests import mergefront_ref as FR
from tests import mergefront_scenes as FS
from tests import mergematch_e2e as E2
from tests import mergematch_ref as MR

DIM, N_RANSAC, GEN_SEED = 64, 1000, 1      # (the scene's matches carry ~0.7 px of noise: 200 hypotheses leave the winner 13 of 30 inliers)


@functools.lru_cache(maxsize=None)
def build(gen_seed=GEN_SEED):
    """-> (S, match_cams, infos, front_cams [pts, desc, K per camera], want: the restatement front's per-entry dict(E, seeds, surf_num, emat_ok))"""
    S, cams, entry, job = E2.build()
    nC, N = S["nC"], S["N"]
    rng = np.random.default_rng(4242)
    desc = [FS.unit_rows(rng, N, DIM) for _ in range(nC)]
    iC, jC = S["maxiCam"], S["maxjCam"]
    for a, b in np.asarray(S["matches"]):
        desc[jC][b] = desc[iC][a] + rng.normal(0, 0.004, DIM).astype(np.float32)
    st = np.asarray(S["state"])
    pa, pb = (rng.permutation(np.nonzero(MR.valid_mask(st[c]))[0])[:30] for c in (1, 2 if jC != 2 else 3))
    for a, b in zip(pa, pb):
        desc[2 if jC != 2 else 3][b] = desc[1][a] + rng.normal(0, 0.004, DIM).astype(np.float32)
    other = 2 if jC != 2 else 3
    live = [np.nonzero(MR.valid_mask(c["state"]))[0] for c in cams]
    front_cams = [dict(pts=np.ascontiguousarray(np.asarray(c["xy"], np.float64).reshape(2, N).T[live[k]]), desc=np.ascontiguousarray(desc[k][live[k]]),
                       K=np.asarray(c["K"], np.float64)) for k, c in enumerate(cams)]
    f2, g1, g2 = entry[0], S["gId1"], S["gId2"]
    infos = [(f2, 1, g1, f2, 3 if other == 2 else 2, g2), (f2, 1, g1, f2, other, g2), entry]
    want = []
    for k, inf in enumerate(infos):
        a, b = front_cams[inf[1]], front_cams[inf[4]]
        r = FR.front_job(a, b, n_ransac=N_RANSAC, seed=gen_seed, k=k)
        FS.assert_descriptor_cover(r["match"], 0.8, 0.6, a["desc"])
        want.append(r)
    # ---- cover: entry 0 has too few SURF matches, entry 1 enough of them and no E, entry 2 is the true pair with exact flags
    assert want[0]["surf_num"] < 25 - 3 and want[1]["surf_num"] >= 25 + 3 and want[1]["inlier_num"] <= 15 - 3 and want[1]["emat_ok"] == 0
    t = want[2]
    assert t["surf_num"] >= 25 + 3 and t["emat_ok"] == 1 and t["inlier_num"] >= 15 + 3
    cnt = t["hyp_count"].astype(np.int64)
    assert cnt[t["best_hyp"]] - np.delete(cnt, t["best_hyp"]).max() >= 3
    iK1, iK2 = (MR.inv33(front_cams[c]["K"]).reshape(3, 3) for c in (iC, jC))
    for E in t["round_E"]:
        e = FR.epi_err(FR.fmat(iK1, iK2, E), t["pix"])
        assert not (np.abs(e - 2.0) < FS.THRESH_BAND).any()
    # ---- the matcher behind it: no candidate within 1e-6 px of epiMax under the restatement's E
    F = MR.fmat(cams[iC]["K"], cams[jC]["K"], t["E"]).reshape(3, 3)
    x1, x2 = np.asarray(cams[iC]["xy"], np.float64).reshape(2, N), np.asarray(cams[jC]["xy"], np.float64).reshape(2, N)
    l = F @ np.stack([x2[0], x2[1], np.ones(N)])                       # epipolarError(F, p1, p2): the line of p2, [3][N2]
    num = np.abs(x1[0][:, None] * l[0][None] + x1[1][:, None] * l[1][None] + l[2][None])
    epi = num / np.sqrt(l[0] ** 2 + l[1] ** 2)[None]
    assert not (np.abs(epi - 20.0) < 1e-6).any()
    return S, cams, infos, front_cams, want
