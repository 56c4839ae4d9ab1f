"""CPU: the yardstick of the SIFT kernels, tests/sift_ref.py, checked on its own -- against scipy's Gaussian filter, on a blob whose keypoint is known, under a rotation
of the input, and the integer form of Lowe's ratio test against the float form -- so that it does not rest on one reading of the algorithm; then the host-side pieces
that need no GPU (the --md_keypoints option, the argument checks of the new entry points, the constants' bookkeeping)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape,sigma", [((23, 31), 1.2262734984654078), ((9, 4), 3.0908), ((5, 1), 1.6), ((40, 17), 2.0)])
def test_blur_equals_scipy_mirror(shape, sigma):
    """the separable blur with reflect-101 borders is scipy's gaussian_filter1d(mode="mirror") at the same radius, rows then columns; among the shapes images
    narrower than the kernel, where the reflection repeats"""
    from scipy.ndimage import gaussian_filter1d
    T = len(R.gauss_taps(sigma))
    assert T == (int(np.rint(8 * sigma + 1)) | 1) and T % 2 == 1
    x = np.arange(T) - T // 2
    taps = np.exp(-(x * x) / (2 * sigma * sigma))
    taps /= taps.sum()                                            # the taps before their rounding to fp32
    assert np.abs(R.gauss_taps(sigma) - taps).max() <= 2.0 ** -24
    img = np.random.default_rng(3).uniform(0, 1, shape)
    want = gaussian_filter1d(gaussian_filter1d(img, sigma, axis=1, mode="mirror", radius=T // 2), sigma, axis=0, mode="mirror", radius=T // 2)
    assert np.abs(R.blur(img, taps) - want).max() <= 1e-12


def test_pyramid_geometry():
    """6 images per octave, round(log2(min side)) - 1 octaves, floor(n / 2) sizes, the next octave is every second pixel of layer 3; sigma_i as published"""
    base = R.base_image(np.random.default_rng(0).integers(0, 256, (37, 53, 3), dtype=np.uint8))
    assert base.shape == (74, 106)
    pyr = R.pyramid(base)
    assert [g.shape for g in pyr] == [(6, 74, 106), (6, 37, 53), (6, 18, 26), (6, 9, 13), (6, 4, 6)]
    assert np.array_equal(pyr[1][0], pyr[0][3][::2, ::2][:37, :53])
    s = R.sigmas()
    k = 2 ** (1 / 3)
    assert abs(s[0] - np.sqrt(1.6 ** 2 - 1)) < 1e-15 and all(abs(s[i] ** 2 + (1.6 * k ** (i - 1)) ** 2 - (1.6 * k ** i) ** 2) < 1e-12 for i in range(1, 6))
    assert R.extrema(R.dog(pyr[3])).shape == (0, 3) and R.extrema(R.dog(pyr[4])).shape == (0, 3)          # sides under 11: nothing, and no index error


def test_base_image_is_exact_in_fp32():
    img = np.random.default_rng(1).integers(0, 256, (11, 7, 3), dtype=np.uint8)
    b64, b32 = R.base_image(img), R.base_image(img, np.float32)
    assert np.array_equal(b64, b32.astype(np.float64)) and np.array_equal(b64 * 16, np.rint(b64 * 16))
    g = R.gray_u8(img)
    assert np.array_equal(b64[1::2, 1::2][:-1, :-1] * 16, 9 * g[:-1, :-1] + 3 * g[:-1, 1:] + 3 * g[1:, :-1] + g[1:, 1:])
    assert b64[0, 0] == g[0, 0] and b64[-1, -1] == g[-1, -1]                                                       # clamped at the edge


def test_blob_gives_a_keypoint_at_its_centre():
    """one Gaussian blob on a flat background: the strongest keypoint lies within half a pixel -- the refinement's own convergence bound -- of the blob's centre, and
    its size is the scale of a blob of that width"""
    h, w, cy, cx, s = 48, 56, 22.0, 30.0, 3.0
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    a = 60 + 150 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    img = np.repeat(np.rint(a).astype(np.uint8)[..., None], 3, 2)
    kp, desc = R.detect_and_compute(img)
    assert len(kp) >= 1 and desc.shape == (len(kp), 128) and desc.dtype == np.uint8
    best = kp[np.argmax(kp[:, 4])]
    assert abs(best[0] - cx) <= 0.5 and abs(best[1] - cy) <= 0.5, best
    assert 0.5 * s * np.sqrt(2) * 2 <= best[2] <= 2.0 * s * np.sqrt(2) * 2, best         # diameter 2 sigma_DoG, sigma_DoG ~ sqrt(2) s for a Gaussian blob


def test_rot90_rotates_keypoints_and_keeps_descriptors():
    """np.rot90 of the input (counter-clockwise) moves a keypoint (x, y) to (y, W - 1/2 - x) -- the 2x upsampling puts pixel centres at quarter positions --, lowers
    its angle by 90 degrees and leaves size, response and descriptor alone, to within fp64 noise.  Checked on the first octave (the upsampled image): every later
    octave starts from every SECOND pixel counted from the top left corner, which a rotation of an even-sized image maps onto the other half of the pixels, so
    those octaves see different samples -- a property of the algorithm, not of this restatement."""
    img = R.synthetic("noise", 40, 52, 11)
    H, W = img.shape[:2]
    kp, desc = R.detect_and_compute(img)
    kq, desq = R.detect_and_compute(np.ascontiguousarray(np.rot90(img)))
    a, b = kp[:, 5] == -1, kq[:, 5] == -1
    kp, desc, kq, desq = kp[a], desc[a], kq[b], desq[b]
    assert len(kp) >= 20 and len(kp) == len(kq)
    want = np.stack([kp[:, 1], W - 0.5 - kp[:, 0], kp[:, 2], (kp[:, 3] - 90.0) % 360.0, kp[:, 4]], 1)
    used = set()
    for row, d in zip(want, desc):
        dist = np.abs(kq[:, 0] - row[0]) + np.abs(kq[:, 1] - row[1]) + R.angle_diff(kq[:, 3], row[3])
        j = int(np.argmin(dist))
        assert j not in used
        used.add(j)
        assert abs(kq[j, 0] - row[0]) <= 1e-9 and abs(kq[j, 1] - row[1]) <= 1e-9 and abs(kq[j, 2] - row[2]) <= 1e-9 and abs(kq[j, 4] - row[4]) <= 1e-12, (kq[j], row)
        assert R.angle_diff(kq[j, 3], row[3]) <= 1e-7, (kq[j], row)
        assert np.abs(desq[j].astype(int) - d.astype(int)).max() <= 1          # a value within fp64 noise of x.5 may round the other way


def test_integer_ratio_test_equals_the_float_form():
    """16 d1 < 9 d2 on squared integer distances is sqrt(d1) < 0.75 sqrt(d2), the comparison of the reference's loop; ties go to the lower index"""
    rng = np.random.default_rng(5)
    des2 = rng.integers(0, 256, (300, 128), dtype=np.uint8)
    des1 = np.clip(des2[rng.integers(0, 300, 200)].astype(int) + rng.integers(-40, 41, (200, 128)) * (rng.random((200, 1)) < 0.7), 0, 255).astype(np.uint8)
    des2[17] = des2[5]                                                       # duplicate rows: the tie rule
    des1[0] = des2[5]
    idx, dist = R.knn2(des1, des2)
    assert idx[0].tolist() == [5, 17] and dist[0].tolist() == [0, 0]
    full = ((des1[:, None].astype(np.int64) - des2[None].astype(np.int64)) ** 2).sum(-1)
    assert np.array_equal(np.sort(full, 1)[:, :2], dist)
    passed = R.ratio_matches(idx, dist)
    flt = np.nonzero(np.sqrt(dist[:, 0].astype(np.float64)) < 0.75 * np.sqrt(dist[:, 1].astype(np.float64)))[0]
    assert np.array_equal(passed, flt) and 0 < len(passed) < len(des1)
    # around the threshold itself: d2 = 16 k, d1 = 9 k - 1, 9 k, 9 k + 1
    for k in (1, 7, 1000, 92160):
        d = np.array([[9 * k - 1, 16 * k], [9 * k, 16 * k], [9 * k + 1, 16 * k]])
        assert R.ratio_matches(np.zeros_like(d), d).tolist() == [0]
    assert len(R.ratio_matches(*R.knn2(des1, des2[:1]))) == 0 and len(R.ratio_matches(*R.knn2(des1, des2[:0]))) == 0      # fewer than two neighbours: no match


def test_constants_are_recorded_with_their_shares():
    """the margins and tolerances of the GPU test are positive, and the recorded shares of the fp32 run against the fp64 run stay within a quarter of the two caps
    (5 % of candidates inside the margin, 10 % of end-to-end points)"""
    assert all(v > 0 for v in R.MARGIN.values()) and all(v > 0 for v in R.TOL.values())
    assert set(R.MEASURED_SHARES["stages"]) == set(R.case_inputs()) == set(R.MEASURED_SHARES["end_to_end"])
    for v in R.MEASURED_SHARES["stages"].values():
        assert v["inside_margin"] / v["candidates"] <= 0.05 / 4 and v["max_u8_diff"] <= 1
    for v in R.MEASURED_SHARES["end_to_end"].values():
        assert v["differ"] / max(v["points"], 1) <= 0.10 / 4 and v["points"] >= 5
    crop = R.case_inputs()["crop"]
    assert crop.dtype == np.uint8 and crop.ndim == 3 and crop.shape[0] <= 96 and crop.shape[1] <= 128


def test_md_keypoints_option_defaults_to_default():
    spec = importlib.util.spec_from_file_location("ffn_metrics_main_sift", os.path.join(ROOT, "evaluation", "metrics", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args(["--path", "x.json"]).md_keypoints == "default"
    assert ap.parse_args(["--path", "x.json", "--md_keypoints", "sift"]).md_keypoints == "sift"
    with pytest.raises(SystemExit):
        ap.parse_args(["--path", "x.json", "--md_keypoints", "orb"])


def test_host_module_agrees_with_the_restatement_on_host_side_rules():
    """taps, sigmas, octave count, keypoint order and the ratio rule of freefine_amd/sift.py are the restatement's (these run on the host in both)"""
    from freefine_amd import sift as S
    for s in R.sigmas():
        assert np.array_equal(S.gauss_taps(s), R.gauss_taps(s)) and len(S.gauss_taps(s)) <= 63
    assert S.sigmas() == R.sigmas() and all(S.n_octaves(hw) == R.n_octaves(hw) for hw in ((74, 106), (96, 128), (1024, 1024), (8, 300)))
    rng = np.random.default_rng(2)
    kp = np.round(rng.uniform(0, 4, (60, 7)), 0).astype(np.float32)         # many ties in every column
    kp = np.concatenate([kp, kp[:7]])
    desc = rng.integers(0, 256, (len(kp), 128), dtype=np.uint8)
    a, b = S.sort_keypoints(kp, desc), R.sort_keypoints(kp, desc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) < len(kp)
    rec = np.zeros((3, 27), np.float32)
    rec[0, :11] = [1, 2, 10, 12, 6.5, 5.25, 3.0, 0.05, 2, 30.0, 200.0]
    rec[2, :10] = [1, 1, 7, 8, 4.0, 3.5, 2.0, 0.02, 1, 0.0]
    assert np.array_equal(S.records_to_keypoints(rec, 1), R.records_to_keypoints(rec, 1).astype(np.float32))
    idx, dist = np.array([[3, 1], [0, -1], [2, 5]]), np.array([[9, 16], [0, 2 ** 31 - 1], [8, 16]])
    assert S.ratio_pairs(idx, dist).tolist() == [[2, 2]] and S.ratio_pairs(idx, dist, 0.8).tolist() == [[0, 3], [2, 2]]


def test_sift_entry_points_check_their_arguments_before_any_launch():
    """no GPU needed: every refusal comes back as FFN_EINVAL with a message naming the entry, nothing is launched"""
    import ctypes
    from freefine_amd import _lib
    lib = _lib.load()
    assert lib.ffn_version() >= 12
    p = 0x10000                                                              # never dereferenced: validation fails first
    taps = (ctypes.c_float * 65)()
    count = ctypes.c_int(0)
    calls = [(lib.ffn_sift_base(None, p, p, 8, 8, 2), b"sift_base"), (lib.ffn_sift_base(None, 0, p, 8, 8, 3), b"sift_base"),
             (lib.ffn_gauss_blur_f32(None, p, p, p + 4096, 8, 8, ctypes.addressof(taps), 4), b"gauss_blur_f32"),
             (lib.ffn_gauss_blur_f32(None, p, p, p + 4096, 8, 8, ctypes.addressof(taps), 65), b"gauss_blur_f32"),
             (lib.ffn_gauss_blur_f32(None, p, p, p, 8, 8, ctypes.addressof(taps), 5), b"gauss_blur_f32"),
             (lib.ffn_decimate2_f32(None, p, p + 4096, 1, 8), b"decimate2_f32"),
             (lib.ffn_sift_extrema(None, p, p, 8, 8, p, 0, p, ctypes.byref(count)), b"sift_extrema"),
             (lib.ffn_sift_refine_orient(None, p, p, 0, 8, 0, p, 3, p), b"sift_refine_orient"),
             (lib.ffn_sift_describe(None, p, 8, 8, 0, 0, 3, p, 0), b"sift_describe"),
             (lib.ffn_knn2_u8(None, p, 2, p + 2, 2, p, p), b"knn2_u8"), (lib.ffn_knn2_u8(None, p, -1, p, 2, p, p), b"knn2_u8")]
    for i, (rc, _) in enumerate(calls):
        assert rc == -22, i
    assert lib.ffn_sift_base(None, p, p, 8, 8, 2) == -22 and b"sift_base" in lib.ffn_last_error()
    assert lib.ffn_knn2_u8(None, p, 2, p + 2, 2, p, p) == -22 and b"knn2_u8" in lib.ffn_last_error()
    assert lib.ffn_sift_refine_orient(None, 0, 0, 8, 8, 0, 0, 0, 0) == 0 and lib.ffn_sift_describe(None, 0, 8, 8, 0, 0, 0, 0, 0) == 0 and lib.ffn_knn2_u8(None, 0, 0, 0, 0, 0, 0) == 0
