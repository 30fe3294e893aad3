"""The planted scene of the images-in test of the device-fed matcher (tests/mergematch_front_scene.py): its cover condition on the
restatements alone, and the flag values of the C interface."""
import numpy as np

from tests import mergematch_front_scene as P


def test_planted_cameras_give_the_host_fed_matcher_enough_matches():
    img1, img2, cams, Ws, Hs, job, matches = P.build()
    assert (Ws, Hs) == (96, 72) and img1.shape == img2.shape == (240, 320)
    assert job["emat_ok"] == 1 and job["inlier_num"] >= 18 and len(job["seeds"]) == job["inlier_num"]
    assert len(matches) >= P.MIN_MATCHES
    for c in cams:
        live = c["state"] == 0
        assert live.sum() >= 28 and (c["state"][~live] == -1).all() and not c["xy"][:, ~live].any()
    rows = {m[0] for m in matches}, {m[1] for m in matches}
    assert len(rows[0]) == len(rows[1]) == len(matches)                       # one-to-one


def test_flag_values_of_the_device_fed_jobs():
    import re

    from coslam_amd import _lib, merge

    m = re.search(r"enum\s*\{([^}]*CS_MERGE_MATCH_SKIPPED[^}]*)\}", _lib.header_text())
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in m.group(1).split(",")))
    assert vals == {"CS_MERGE_MATCH_PAIRS_OVERFLOW": 1, "CS_MERGE_MATCH_MATCHES_OVERFLOW": 2, "CS_MERGE_MATCH_SKIPPED": 4,
                    "CS_MERGE_MATCH_SEEDS_OVERFLOW": 8}
    assert (merge.MERGE_MATCH_SKIPPED, merge.MERGE_MATCH_SEEDS_OVERFLOW) == (4, 8)
    assert np.dtype(np.float64).itemsize * 9 + 8 == _lib.ctypes.sizeof(merge.MergeMatchFrontJob) == 80
