"""The SURF stage without a device: the C interface against the header, the refusals that need no device, the loud failure
without one, and known answers of the numpy restatement tests/surf_ref.py -- which is the definition the GPU tests hold the kernels to."""
import ctypes as C
import math

import numpy as np
import pytest

import coslam_amd
from coslam_amd import _lib
from tests import surf_ref as R
from tests import surf_scenes as S


def test_symbols_constants_and_the_buffers_mirror():
    L = coslam_amd.lib()
    decl = _lib.declarations()
    names = ["cs_surf_create", "cs_surf_destroy", "cs_surf_run_dev", "cs_surf_integral_dev", "cs_surf_layers_dev", "cs_surf_detect_dev", "cs_surf_counts",
             "cs_surf_buffers_get", "cs_surf_download"]
    for n in names:
        assert n in decl and hasattr(L, n), n
    assert len(decl["cs_surf_create"][1]) == 8 and decl["cs_surf_create"][0] is C.c_void_p
    assert len(decl["cs_surf_run_dev"][1]) == 6 and decl["cs_surf_run_dev"][1][4] is C.c_double
    hdr = open(_lib.HEADER_PATH).read()
    for name, val in (("CS_SURF_MAX_OCTAVES", R.MAX_OCTAVES), ("CS_SURF_MAX_LAYERS", R.MAX_LAYERS), ("CS_SURF_ORI_SAMPLES", len(R.ORI_GRID)),
                      ("CS_SURF_ORI_WINDOWS", R.N_WINDOWS)):
        assert f"#define {name} {val}" in hdr, name
    from coslam_amd.surf import SURF_MAX_LAYERS, SURF_MAX_OCTAVES, SurfBuffers

    assert (SURF_MAX_OCTAVES, SURF_MAX_LAYERS) == (R.MAX_OCTAVES, R.MAX_LAYERS) and len(R.ORI_GRID) == 109
    assert C.sizeof(SurfBuffers) == 14 * 8 + 4 * (8 + 5 + 5 + 3 * 30)          # (the layout itself: tests/test_abi.py, from the compiler)
    assert coslam_amd.Surf._prefix == "cs_surf"


def test_refusals_that_need_no_device():
    L = coslam_amd.lib()
    for args in ((0, 32, 32, 8, 4, 2, 64), (17, 32, 32, 8, 4, 2, 64), (1, 0, 32, 8, 4, 2, 64), (1, 32, -1, 8, 4, 2, 64), (1, 32, 32, 0, 4, 2, 64),
                 (1, 32, 32, 32769, 4, 2, 64), (1, 32, 32, 8, 0, 2, 64), (1, 32, 32, 8, 6, 2, 64), (1, 32, 32, 8, 4, 0, 64), (1, 32, 32, 8, 4, 5, 64),
                 (1, 32, 32, 8, 4, 2, 96)):
        assert not L.cs_surf_create(0, *args), args
        assert b"cs_surf_create: bad argument" in L.cs_last_error()
    assert not L.cs_surf_create(0, 1, 4105, 4105, 8, 4, 2, 64) and b"2^32" in L.cs_last_error()      # 4105^2 255 >= 2^32 > 4104^2 255
    tab = (C.c_void_p * 1)(None)
    assert L.cs_surf_run_dev(None, None, tab, 32, 1.0, 0) == -1 and b"null handle" in L.cs_last_error()
    assert L.cs_surf_integral_dev(None, None, tab, 32) == -1 and L.cs_surf_layers_dev(None, None, tab, 32) == -1 and L.cs_surf_detect_dev(None, None, tab, 32, 1.0) == -1
    assert L.cs_surf_counts(None, None, None, None) == -1 and L.cs_surf_buffers_get(None, None) == -1
    assert L.cs_surf_download(None, None, None, None, 0) == -1
    L.cs_surf_destroy(None)
    with pytest.raises(ValueError):
        R.integral(np.zeros((4105, 4105), np.uint8))


def test_no_device_means_a_loud_failure():
    if coslam_amd.lib().cs_device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(coslam_amd.CoslamHipError, match="cs_surf_create"):
        coslam_amd.Surf(1, 64, 48, 32)


# ---- the restatement's known answers -------------------------------------------------------------------------------------------------
def test_integral_image_against_cumsum():
    rng = np.random.default_rng(1)
    for img in (rng.integers(0, 256, (37, 53), dtype=np.uint8), np.full((300, 200), 255, np.uint8)):
        I = R.integral(img)
        assert I.dtype == np.uint32 and not I[0].any() and not I[:, 0].any()
        assert np.array_equal(I[1:, 1:].astype(np.int64), img.astype(np.int64).cumsum(0).cumsum(1))
        H, W = img.shape
        assert R.box(I, -5, -7, H + 9, W + 3) == int(img.sum()) and R.box(I, H, 0, H + 4, W) == 0           # clamped, never out of range
        assert R.box(I, 3, 4, 11, 9) == int(img[3:11, 4:9].sum())
    assert int(R.integral(np.full((300, 200), 255, np.uint8))[-1, -1]) == 255 * 300 * 200


def blob_sizes(sigmas, cx=81.0, cy=59.0):
    """a single blob of each sigma: found within 0.5 px of its centre -> its sizes"""
    sizes = []
    for sigma in sigmas:
        kp = R.detect(R.integral(S.blob(160, 120, cx, cy, sigma)), 50.0)
        assert len(kp["x"]) >= 1, f"sigma {sigma}: no key point"
        k = int(np.argmax(kp["response"]))
        assert math.hypot(kp["x"][k] - cx, kp["y"][k] - cy) <= 0.5, (sigma, kp["x"][k], kp["y"][k])
        assert kp["laplacian"][k] == 0              # a bright blob: dx + dy < 0
        sizes.append(float(kp["size"][k]))
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sigmas), sizes
    return sizes


def test_a_single_blob_is_found_at_its_centre_and_size_grows_with_sigma():
    """sigma 2 is near the smallest scale the first octave selects: at the blob's centre the layers L = 9, 15, 21 give 133.0, 150.7, 87.7.
    Sizes come out near 6.5 sigma (13.3, 19.2, 30.0, 44.5).  The larger blobs are found in octave 1, whose even windows are centred half
    a pixel off their sample: detect() reports the window's centre, and over centres on and off the sample grid the error stays below
    0.08 px (without that correction it is 0.5 px per axis)."""
    assert blob_sizes((2.0, 3.0, 4.5, 7.0))[0] < 15.0
    assert blob_sizes((2.0, 3.0, 4.5, 7.0), 80.25, 59.4)[0] < 15.0          # a centre off every sample grid


def test_order_capacity_and_unit_norm():
    img, ref = S.scene(160, 120)
    key = [tuple(r) for r in np.column_stack([ref["octave"], ref["layer"], ref["cell"]])]
    assert key == sorted(key) and ref["count"] > 20
    assert np.abs(np.linalg.norm(ref["desc"].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    cut = R.run(img, S.THRESHOLD, max_pts=7)
    assert (cut["count"], cut["overflow"]) == (7, ref["count"] - 7) and np.array_equal(cut["desc"], ref["desc"][:7])
    assert R.run(np.full((48, 64), 90, np.uint8), 1.0)["count"] == 0
    assert R.run(S.texture(24, 24, 0, 90.0), S.THRESHOLD)["count"] == 0


def test_shift_invariance_is_exact():
    """an upright run on a texture and on the same texture shifted by (16, 8) pixels, multiples of the coarsest sample step: away from the
    borders the key points are the shifted ones, with bit-equal descriptors"""
    dx, dy = 16, 8
    (_, a), (_, b) = S.scene(320, 240, upright=True), S.scene(320, 240, upright=True, shift=(dx, dy))
    index = {(int(o), int(l), int(r), int(c)): k for k, (o, l, (r, c)) in enumerate(zip(b["octave"], b["layer"], b["cell"]))}
    n = 0
    for k in range(a["count"]):
        o, x, y, s = int(a["octave"][k]), a["x"][k], a["y"][k], a["s"][k]
        # what a key point reads: the upright descriptor window (10 s) with its Haar boxes (s + 1) and a pixel of rounding; the upper
        # layer's filter (L / 2) about the 27 samples (a step further out)
        reach = max(11.0 * s + 3.0, R.layer_size(o, a["layer"][k] + 1) / 2 + 2 * (1 << o) + 1)
        if not (reach + dx < x < 320 - reach and reach + dy < y < 240 - reach):
            continue
        j = index.get((o, int(a["layer"][k]), int(a["cell"][k][0]) - (dy >> o), int(a["cell"][k][1]) - (dx >> o)))
        assert j is not None, k
        # (column + offset) x step rounds at the magnitude of the column: the shifted coordinate is the same to two ulps of 320
        assert abs(b["x"][j] - (x - dx)) <= 2.5e-13 and abs(b["y"][j] - (y - dy)) <= 2.5e-13
        assert b["size"][j] == a["size"][k] and b["response"][j] == a["response"][k] and b["laplacian"][j] == a["laplacian"][k]
        assert a["desc"][k].tobytes() == b["desc"][j].tobytes()
        n += 1
    assert n >= 20, n


def test_every_scene_meets_its_cover_conditions():
    for W, H in S.SEEDS:
        for dim, upright in ((64, False), (128, True)):
            _img, ref = S.scene(W, H, dim=dim, upright=upright)          # (scene() asserts them)
            assert not S.cover_failures(ref["info"], S.THRESHOLD, oriented=not upright)
    assert S.scene(320, 240)[1]["count"] > 80 and max(S.scene(320, 240)[1]["octave"]) >= 2
    assert S.find_seed(160, 120, tries=1) == S.SEEDS[(160, 120)]        # the committed seed is the first that passes
    assert len(S.shifted_pair()[2]["matches"]) >= 28


def test_the_descriptor_tolerance_study():
    for dim in (64, 128):
        st = S.descriptor_study(dim)
        print(f"dim {dim}: largest change d = {st['d']:.3e}, serial against kernel-shaped summation {st['shape']:.3e}, GPU tolerance {st['tol']:.3e}")
        assert st["tol"] == max(100.0 * st["d"], 2.4e-7) and 0.0 < st["d"] < 1e-9 and st["shape"] <= 2.4e-7
