"""coslam_amd.Surf(keep="strongest") against the restatement tests/surf_select_ref.py: counts and key-point lists bit for bit;
angles and descriptors bit-equal to the same rows of a keep="first" run of the device that holds every maximum (a row depends on its own
key point only).  And keep="first" still is what tests/test_surf_gpu.py demands of it."""
import numpy as np
import pytest

import coslam_amd
from tests import surf_ref as R
from tests import surf_scenes as S
from tests import surf_select_ref as SR
from tests.test_surf_gpu import check_padding, compare_lists, upload
from tests.test_surf_select_cpu import SCENES, cut_sizes

pytestmark = pytest.mark.gpu

LIST_KEYS = ("pts", "size", "response", "laplacian", "octave", "layer", "cell")


def device_rows(img, max_pts, keep, pitch=None, threshold=S.THRESHOLD):
    H, W = img.shape
    sf = coslam_amd.Surf(1, W, H, max_pts, keep=keep)
    t, p = upload([img], pitch)
    sf.enqueue(t, threshold, pitch=p)
    cnt, ovf = sf.counts()
    rows = sf.rows(0, max_pts)
    sf.close()
    return int(cnt[0]), int(ovf[0]), rows


def assert_rows_equal(rows, want, full, kept, n):
    """the first n device rows: lists against the restatement `want`, angles / descriptors against rows `kept` of the device run `full`"""
    for key in LIST_KEYS:
        assert rows[key][:n].tobytes() == np.ascontiguousarray(want[key]).tobytes(), key
    assert rows["angle"][:n].tobytes() == np.ascontiguousarray(full["angle"][kept]).tobytes()
    assert rows["desc"][:n].tobytes() == np.ascontiguousarray(full["desc"][kept]).tobytes()
    check_padding(rows, n)


@pytest.mark.parametrize("wh,seed,pitch", [(SCENES[0][0], SCENES[0][1], None), (SCENES[1][0], SCENES[1][1], 176)])
def test_strongest_rows_are_the_restatements(hip, wh, seed, pitch):
    img, ref = S.scene(*wh, seed=seed)
    total = ref["count"]
    assert total >= 8
    n_full, ovf_full, full = device_rows(img, total + 3, "first", pitch)
    assert (n_full, ovf_full) == (total, 0)
    for max_pts in cut_sizes(total):
        want = SR.run(img, S.THRESHOLD, max_pts)
        n, ovf, rows = device_rows(img, max_pts, "strongest", pitch)
        print(f"{wh} max_pts {max_pts}: count {n} overflow {ovf} (restatement {want['count']}, {want['overflow']}), kept {want['kept'].tolist()}")
        assert (n, ovf) == (want["count"], want["overflow"]) == (min(total, max_pts), max(0, total - max_pts))
        assert_rows_equal(rows, want, full, want["kept"], n)
        if max_pts >= total:          # no overflow: every buffer is keep="first"'s, byte for byte
            n1, ovf1, first = device_rows(img, max_pts, "first", pitch)
            assert (n1, ovf1) == (n, ovf) and all(first[k].tobytes() == rows[k].tobytes() for k in first)


def test_a_tie_at_the_cut_keeps_the_earlier_row(hip):
    img = SR.tie_image()
    r = R.detect(R.integral(img), S.THRESHOLD)["response"]
    assert len(r) == 4 and r[0].tobytes() == r[1].tobytes() and r[2] > r[0] > r[3]      # the equals are ranks 1 and 2: a cut of 2 parts them
    _n, _o, full = device_rows(img, 8, "first")
    for max_pts, kept in ((2, [0, 2]), (3, [0, 1, 2]), (1, [2])):
        want = SR.run(img, S.THRESHOLD, max_pts)
        assert want["kept"].tolist() == kept
        n, ovf, rows = device_rows(img, max_pts, "strongest")
        assert (n, ovf) == (max_pts, 4 - max_pts)
        assert_rows_equal(rows, want, full, want["kept"], n)
    assert device_rows(img, 2, "first")[2]["cell"].tolist() == [[20, 24], [20, 56]]      # (what the default keeps: both equals)


def test_three_cameras_one_skipped_one_short_one_overflowing(hip):
    W, H = 161, 123
    (im_a, ref_a), (im_b, ref_b) = S.scene(W, H, seed=1), S.scene(W, H, seed=2)
    max_pts = ref_a["count"] + 2
    assert 8 <= ref_a["count"] < max_pts < ref_b["count"]
    want_b = SR.run(im_b, S.THRESHOLD, max_pts)
    sf = coslam_amd.Surf(3, W, H, max_pts, keep="strongest")
    t, p = upload([None, im_a, im_b], 176)
    for _again in range(2):          # (a second call of the handle starts from fresh counts)
        sf.enqueue(t, S.THRESHOLD, pitch=p)
    cnt, ovf = sf.counts()
    assert cnt.tolist() == [0, ref_a["count"], max_pts] and ovf.tolist() == [0, 0, ref_b["count"] - max_pts]
    check_padding(sf.rows(0, max_pts), 0)
    rows_a, rows_b = sf.rows(1, max_pts), sf.rows(2, max_pts)
    compare_lists(rows_a, ref_a, ref_a["count"])
    check_padding(rows_a, ref_a["count"])
    for key in LIST_KEYS:
        assert rows_a[key][:cnt[1]].tobytes() == np.ascontiguousarray(ref_a[key]).tobytes(), key
        assert rows_b[key].tobytes() == np.ascontiguousarray(want_b[key]).tobytes(), key
    tol = S.descriptor_study()["tol"]
    assert np.abs(rows_b["angle"] - want_b["angle"]).max() <= 1e-9 and np.abs(rows_b["desc"] - want_b["desc"]).max() <= tol
    Ks = [S.K300(W, H)] * 3
    fc = sf.front_cams(Ks)
    assert [c["n"] for c in fc] == [max_pts] * 3
    assert [c["pts"] for c in fc] == [int(sf.buf.pts) + 16 * max_pts * c for c in range(3)]
    assert [c["desc"] for c in fc] == [int(sf.buf.desc) + 4 * 64 * max_pts * c for c in range(3)]
    sf.close()


def test_keep_first_is_untouched(hip):
    """the assertions of tests/test_surf_gpu.py's test_key_point_lists and test_max_pts_below_the_count_keeps_the_first_rows on one scene"""
    W, H, pitch, max_pts = 161, 123, 176, 64
    img, ref = S.scene(W, H)
    sf = coslam_amd.Surf(1, W, H, max_pts, keep="first")
    t, p = upload([img], pitch)
    sf.detect(t, S.THRESHOLD, p)
    cnt, ovf = sf.counts()
    assert (cnt[0], ovf[0]) == (ref["count"], 0) and ref["count"] > 20
    rows = sf.rows(0, max_pts)
    diff = compare_lists(rows, ref, ref["count"])
    assert max(diff.values()) == 0.0
    check_padding(rows, ref["count"])
    assert not rows["angle"][:cnt[0]].any()
    sf.close()
    keep = 10
    sf = coslam_amd.Surf(1, W, H, keep)
    sf.enqueue(t, S.THRESHOLD, pitch=p)
    cnt, ovf = sf.counts()
    assert (cnt[0], ovf[0]) == (keep, ref["count"] - keep) and ovf[0] > 0
    rows = sf.rows(0, keep)
    compare_lists(rows, ref, keep)
    assert np.abs(rows["desc"] - ref["desc"][:keep]).max() <= S.descriptor_study()["tol"]
    sf.close()
    with pytest.raises(ValueError):
        coslam_amd.Surf(1, W, H, keep, keep="weakest")
