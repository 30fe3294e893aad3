"""The strongest-first choice of the SURF stage on the CPU: the restatement tests/surf_select_ref.py against what it claims
to be, and the C interface that carries the choice (header and built library)."""
import re

import numpy as np
import pytest

from tests import surf_ref as R
from tests import surf_scenes as S
from tests import surf_select_ref as SR

# the committed 96 x 64 scene (seed 0) has no maximum above the threshold; 14 is the first seed of surf_scenes.texture at which that size has
# eight, and scene() holds it to the same cover conditions
SEED_96 = 14
SCENES = [((96, 64), SEED_96), ((161, 123), None)]


def cut_sizes(total):
    return [1, total // 2, total - 1, total, total + 1]


@pytest.mark.parametrize("wh,seed", SCENES)
def test_kept_set_is_the_top_k_in_ascending_order(wh, seed):
    img, ref = S.scene(*wh, seed=seed)
    total = ref["count"]
    assert total >= 8
    assert len(set(ref["response"].tolist())) == total          # (no equal responses here: the top-k is one set)
    for max_pts in cut_sizes(total):
        got = SR.run(img, S.THRESHOLD, max_pts)
        k = min(total, max_pts)
        assert (got["count"], got["overflow"], got["total"]) == (k, total - k, total)
        kept = got["kept"]
        assert np.array_equal(kept, np.sort(np.argsort(-ref["response"], kind="stable")[:k])) and (np.diff(kept) > 0).all()
        for key in ("pts", "size", "response", "laplacian", "octave", "layer", "cell", "angle", "desc"):
            assert got[key].tobytes() == np.ascontiguousarray(ref[key][kept]).tobytes(), key      # a row depends on its own key point only
        if max_pts < total:
            assert got["response"].min() > np.delete(ref["response"], kept).max()


@pytest.mark.parametrize("wh,seed", SCENES)
def test_no_overflow_is_the_first_rows_rule(wh, seed):
    img, ref = S.scene(*wh, seed=seed)
    for max_pts in (ref["count"], ref["count"] + 1, 4 * ref["count"]):
        a, b = SR.run(img, S.THRESHOLD, max_pts), R.run(img, S.THRESHOLD, max_pts=max_pts)
        assert a["count"] == b["count"] == ref["count"] and a["overflow"] == b["overflow"] == 0
        for key in ("pts", "size", "response", "laplacian", "octave", "layer", "cell", "angle", "desc"):
            assert a[key].tobytes() == b[key].tobytes(), key


def test_a_tie_at_the_cut_goes_to_the_earlier_row():
    assert SR.select([3.0, 5.0, 5.0, 7.0, 5.0, 1.0], 2).tolist() == [1, 3]
    assert SR.select([3.0, 5.0, 5.0, 7.0, 5.0, 1.0], 3).tolist() == [1, 2, 3]
    assert SR.select([5.0, 5.0, 5.0], 1).tolist() == [0] and SR.select([5.0, 5.0], 2).tolist() == [0, 1] and SR.select([], 3).tolist() == []
    kp = R.detect(R.integral(SR.tie_image()), S.THRESHOLD)
    r = kp["response"]
    assert len(r) == 4 and r[0].tobytes() == r[1].tobytes() and r[2] > r[0] > r[3]      # the equals are ranks 1 and 2: a cut of 2 parts them
    assert SR.select(r, 2).tolist() == [0, 2] and SR.select(r, 3).tolist() == [0, 1, 2] and SR.select(r, 1).tolist() == [2]


def test_the_choice_is_declared_and_exported():
    import coslam_amd
    from coslam_amd import _lib

    txt = _lib.header_text()
    m = re.search(r"enum\s*\{([^}]*CS_SURF_KEEP_FIRST[^}]*)\}", txt)
    assert m, "CS_SURF_KEEP_FIRST is not declared"
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in m.group(1).split(",")))
    assert vals == {"CS_SURF_KEEP_FIRST": 0, "CS_SURF_KEEP_STRONGEST": 1}
    decl = _lib.declarations()
    assert decl["cs_surf_keep_set"][1] == [_lib.ctypes.c_void_p, _lib.ctypes.c_int] and decl["cs_surf_keep_set"][0] is _lib.ctypes.c_int
    assert len(decl["cs_surf_create"][1]) == 8                  # its signature stays
    for fn in ("cs_merge_match_run_front_dev", "cs_merge_match_front_jobs"):
        assert fn in decl, fn
    assert len(decl["cs_merge_match_run_front_dev"][1]) == 14
    L = coslam_amd.lib()
    for fn in ("cs_surf_keep_set", "cs_merge_match_run_front_dev", "cs_merge_match_front_jobs"):
        assert hasattr(L, fn), fn                               # exported by the built library
    assert L.cs_surf_keep_set(None, 1) == -1 and b"cs_surf_keep_set" in L.cs_last_error()       # (refused without a device)
