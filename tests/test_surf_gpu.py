"""coslam_amd.Surf against the numpy restatement tests/surf_ref.py: integral images, layer maps and key-point lists are held
EXACTLY (integers, f64 in one expression order, orders from scans); angles within 1e-9 rad and descriptors within the tolerance of the
study in tests/surf_scenes.py, on scenes whose cover conditions keep every decision away from an ulp of atan2 / cos / sin."""
import numpy as np
import pytest

import coslam_amd
from tests import surf_ref as R
from tests import surf_scenes as S

pytestmark = pytest.mark.gpu


def upload(imgs, pitch=None):
    """u8 images (None: camera skipped) -> (torch tensors with the row pitch, the pitch)"""
    import torch

    W = next(im for im in imgs if im is not None).shape[1]
    pitch = W if pitch is None else pitch
    out = []
    for im in imgs:
        if im is None:
            out.append(None)
            continue
        buf = np.full((im.shape[0], pitch), 77, np.uint8)      # (the padding of a row is not zero)
        buf[:, :W] = im
        out.append(torch.as_tensor(buf, device="cuda"))
    return out, pitch


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


@pytest.mark.parametrize("W,H,pitch,kind", [(96, 64, None, "texture"), (161, 123, 176, "texture"), (1024, 1024, None, "white"),
                                            (640, 480, None, "noise")])
def test_integral_image_is_exact(hip, W, H, pitch, kind):
    img = S.scene(W, H)[0] if kind == "texture" else np.full((H, W), 255, np.uint8) if kind == "white" else noise(W, H, 3)
    sf = coslam_amd.Surf(1, W, H, 16, n_octaves=1, n_octave_layers=1)
    t, p = upload([img], pitch)
    sf.integral(t, p)
    got = sf.integral_image(0)
    assert got.dtype == np.uint32 and np.array_equal(got, R.integral(img))
    if kind == "white":
        assert int(got[-1, -1]) == 255 * W * H
    sf.close()


def check_maps(sf, c, img):
    I = R.integral(img)
    for o in range(sf.n_octaves):
        for l in range(sf.n_layers + 2):
            det, lap = sf.layer_map(c, o, l)
            wd, wl = R.layer_map(I, o, l)
            assert det.tobytes() == wd.tobytes() and np.array_equal(lap, wl), (c, o, l)
            assert bool(sf.buf.layerFits[o * 6 + l]) == R.layer_fits(img.shape[1], img.shape[0], o, l)


@pytest.mark.parametrize("W,H,pitch", [(96, 64, None), (161, 123, 176)])
def test_layer_maps_and_laplacian_bytes_are_bit_equal(hip, W, H, pitch):
    img = S.scene(W, H)[0]
    if (W, H) == (96, 64):      # L < 64: octave 2's upper layers (84, 108) do not fit -- no middle layer is left there -- and octave 3 vanishes
        assert [[R.layer_fits(W, H, o, l) for l in range(4)] for o in range(4)] == [[True] * 4, [True] * 4, [True, True, False, False], [False] * 4]
    sf = coslam_amd.Surf(1, W, H, 64)
    t, p = upload([img], pitch)
    sf.detect(t, S.THRESHOLD, p)
    check_maps(sf, 0, img)
    sf.close()


def test_layer_maps_of_three_cameras_and_of_the_last_two_of_sixteen(hip):
    W, H = 160, 120
    imgs = [S.texture(W, H, seed) for seed in (11, 12, 13)]
    sf = coslam_amd.Surf(3, W, H, 64, n_octaves=3)
    t, p = upload(imgs)
    sf.detect(t, S.THRESHOLD, p)
    for c in range(3):
        check_maps(sf, c, imgs[c])
    sf.close()
    sf = coslam_amd.Surf(16, W, H, 64, n_octaves=3)
    t, p = upload([None] * 14 + imgs[:2])
    sf.enqueue(t, S.THRESHOLD, pitch=p)
    cnt, ovf = sf.counts()
    assert not cnt[:14].any() and not ovf.any()
    for c in (14, 15):
        check_maps(sf, c, imgs[c - 14])
        assert cnt[c] == len(R.detect(R.integral(imgs[c - 14]), S.THRESHOLD, 3)["x"]) > 5
    assert not np.isfinite(sf.rows(3, 64)["pts"]).any() and not sf.rows(3, 64)["desc"].any()
    assert not sf.layer_map(0, 0, 0)[0].any()          # a skipped camera's maps are never written
    sf.close()


def compare_lists(got, ref, n):
    """count rows of the device against the restatement -> the largest differences of x, y, size, response"""
    assert np.array_equal(got["octave"][:n], ref["octave"][:n]) and np.array_equal(got["layer"][:n], ref["layer"][:n])
    assert np.array_equal(got["cell"][:n], ref["cell"][:n]) and np.array_equal(got["laplacian"][:n], ref["laplacian"][:n])
    key = [tuple(r) for r in np.column_stack([got["octave"][:n], got["layer"][:n], got["cell"][:n]])]
    assert key == sorted(key) and len(set(key)) == n                   # ascending (octave, layer, row, column)
    live = np.isfinite(ref["pts"][:n, 0])                              # (a zero-norm descriptor gives its key point NaN coordinates)
    assert np.array_equal(np.isfinite(got["pts"][:n, 0]), live)
    diff = dict(xy=float(np.max(np.abs(got["pts"][:n][live] - ref["pts"][:n][live]), initial=0.0)),
                size=float(np.max(np.abs(got["size"][:n] - ref["size"][:n]), initial=0.0)),
                response=float(np.max(np.abs(got["response"][:n] - ref["response"][:n]), initial=0.0)))
    print("largest differences:", diff)
    assert max(diff.values()) <= 1e-9
    return diff


def check_padding(rows, n):
    assert np.isnan(rows["pts"][n:]).all() and np.isnan(rows["size"][n:]).all() and np.isnan(rows["angle"][n:]).all()
    assert np.isnan(rows["response"][n:]).all() and not rows["desc"][n:].any()
    assert not rows["octave"][n:].any() and not rows["layer"][n:].any() and not rows["cell"][n:].any() and not rows["laplacian"][n:].any()


@pytest.mark.parametrize("W,H,pitch,max_pts", [(161, 123, 176, 64), (320, 240, None, 256)])
def test_key_point_lists(hip, W, H, pitch, max_pts):
    img, ref = S.scene(W, H)
    sf = coslam_amd.Surf(1, W, H, max_pts)
    t, p = upload([img], pitch)
    sf.detect(t, S.THRESHOLD, p)
    cnt, ovf = sf.counts()
    assert (cnt[0], ovf[0]) == (ref["count"], 0) and ref["count"] > 20
    rows = sf.rows(0, max_pts)
    diff = compare_lists(rows, ref, ref["count"])
    assert max(diff.values()) == 0.0                                   # equality is expected
    check_padding(rows, ref["count"])
    assert not rows["angle"][:cnt[0]].any()                            # the detect stage alone leaves angle 0
    sf.close()


def test_max_pts_below_the_count_keeps_the_first_rows(hip):
    W, H, keep = 161, 123, 10
    img, ref = S.scene(W, H)
    sf = coslam_amd.Surf(1, W, H, keep)
    t, p = upload([img])
    sf.enqueue(t, S.THRESHOLD, pitch=p)
    cnt, ovf = sf.counts()
    assert (cnt[0], ovf[0]) == (keep, ref["count"] - keep) and ovf[0] > 0
    rows = sf.rows(0, keep)
    compare_lists(rows, ref, keep)
    assert np.abs(rows["desc"] - ref["desc"][:keep]).max() <= S.descriptor_study()["tol"]
    sf.close()
    sf = coslam_amd.Surf(1, W, H, keep + 6)                            # and padding behind a short list
    sf.enqueue(t, 1.0e7, pitch=p)
    assert sf.counts()[0][0] == 0
    check_padding(sf.rows(0, keep + 6), 0)
    sf.close()


@pytest.mark.parametrize("W,H", [(64, 48), (24, 24)])
def test_a_flat_image_and_a_tiny_image_give_no_key_points(hip, W, H):
    img = np.full((H, W), 90, np.uint8) if W == 64 else S.texture(W, H, 0, 90.0)
    thr = 1.0 if W == 64 else S.THRESHOLD
    assert R.run(img, thr)["count"] == 0
    sf = coslam_amd.Surf(2, W, H, 32)
    t, p = upload([img, img])
    sf.enqueue(t, thr, pitch=p)
    cnt, ovf = sf.counts()
    assert not cnt.any() and not ovf.any()
    for c in range(2):
        check_padding(sf.rows(c, 32), 0)
    sf.close()


@pytest.mark.parametrize("dim", [64, 128])
@pytest.mark.parametrize("upright", [False, True])
def test_angles_and_descriptors(hip, dim, upright):
    tol = S.descriptor_study(dim)
    print("descriptor study:", tol)
    assert tol["tol"] == max(100.0 * tol["d"], 2.4e-7)
    for W, H in ((160, 120), (320, 240)) if (dim, upright) == (64, False) else ((160, 120),):
        img, ref = S.scene(W, H, dim=dim, upright=upright)
        sf = coslam_amd.Surf(1, W, H, 256, dim_desc=dim)
        t, p = upload([img])
        sf.enqueue(t, S.THRESHOLD, upright=upright, pitch=p)
        n = sf.counts()[0][0]
        assert n == ref["count"] > 20
        rows = sf.rows(0, 256)
        compare_lists(rows, ref, n)
        da = float(np.max(np.abs(rows["angle"][:n] - ref["angle"])))
        dd = float(np.max(np.abs(rows["desc"][:n].astype(np.float64) - ref["desc"].astype(np.float64))))
        print(f"{W} x {H} dim {dim} upright {upright}: largest angle difference {da:.3e} rad, descriptor difference {dd:.3e}")
        assert da <= 1e-9 and dd <= tol["tol"]
        assert np.abs(np.linalg.norm(rows["desc"][:n].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
        if upright:
            assert not rows["angle"][:n].any()
        check_padding(rows, n)
        sf.close()


def test_two_runs_give_byte_equal_buffers(hip):
    W, H = 160, 120
    imgs = [S.scene(W, H)[0], S.texture(W, H, 11)]
    t, p = upload(imgs)
    snaps = []
    for _ in range(2):
        sf = coslam_amd.Surf(2, W, H, 64)
        for _again in range(2):          # (and a second call of one handle overwrites the first)
            sf.enqueue(t, S.THRESHOLD, pitch=p)
        rows = [sf.rows(c, 64) for c in range(2)]
        snaps.append(b"".join(r[k].tobytes() for r in rows for k in sorted(r)) + sf.counts()[0].tobytes())
        sf.close()
    assert snaps[0] == snaps[1]


def test_refusals(hip):
    import ctypes as C

    import torch

    L = coslam_amd.lib()
    for args in ((0, 32, 32, 8, 4, 2, 64), (17, 32, 32, 8, 4, 2, 64), (1, 0, 32, 8, 4, 2, 64), (1, 32, 32, 0, 4, 2, 64), (1, 32, 32, 32769, 4, 2, 64),
                 (1, 32, 32, 8, 0, 2, 64), (1, 32, 32, 8, 6, 2, 64), (1, 32, 32, 8, 4, 0, 64), (1, 32, 32, 8, 4, 5, 64), (1, 32, 32, 8, 4, 2, 96),
                 (1, 4105, 4105, 8, 4, 2, 64)):
        assert not L.cs_surf_create(0, *args), args
        assert b"cs_surf_create" in L.cs_last_error()
    sf = coslam_amd.Surf(1, 32, 32, 8)
    img = torch.zeros((32, 32), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    tab = (C.c_void_p * 1)(img.data_ptr())
    assert L.cs_surf_run_dev(None, s, tab, 32, 1.0, 0) == -1 and L.cs_surf_run_dev(sf._m, s, None, 32, 1.0, 0) == -1
    assert L.cs_surf_run_dev(sf._m, s, tab, 31, 1.0, 0) == -1 and b"pitch" in L.cs_last_error()
    for thr in (-1.0, float("nan"), float("inf")):
        assert L.cs_surf_run_dev(sf._m, s, tab, 32, thr, 0) == -1 and b"threshold" in L.cs_last_error()
        assert L.cs_surf_detect_dev(sf._m, s, tab, 32, thr) == -1
    assert L.cs_surf_integral_dev(sf._m, s, tab, 16) == -1
    assert L.cs_surf_counts(None, s, None, None) == -1 and L.cs_surf_buffers_get(None, None) == -1
    host = np.zeros(4, np.int32)
    assert L.cs_surf_download(sf._m, s, int(sf.buf.count) + (1 << 40), host.ctypes.data, 4) == -1
    with pytest.raises(ValueError):
        sf.enqueue([img, img], 1.0)
    sf.close()
