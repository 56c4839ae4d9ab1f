"""GPU: the SIFT stages of freefine_amd/sift.py (csrc/sift.h) against the fp64 restatement tests/sift_ref.py, each stage fed the DEVICE's own upstream output
(downloaded), so that one stage's rounding is never another stage's error.  Inputs: sift_ref.case_inputs() -- seeded blobs / sheared checkerboard / low-pass noise at
37 x 53, 48 x 64 and 64 x 48 (odd sizes; the last octaves fall below the 11 pixels a candidate needs) and one real 96 x 128 crop (tests/golden/g17_sift_crop.npz).

Bounds: the base image, the DoG, the candidate set and the matcher are bit-exact; the blur is within 2 (T + 1) 2^-24 max|x| (two passes of T non-negative taps that sum
to 1); refinement, orientation and descriptor compare discrete outcomes outside sift_ref.MARGIN and continuous outputs within sift_ref.TOL -- each 4 x the largest
deviation of the restatement's fp32 run from its fp64 run on these inputs (sift_ref.measure) --, quantised descriptor elements within 1.  Two caps: at most 5 % of an
input's candidates inside the margin, at most 10 % of the end-to-end points different."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["blobs_37x53", "checker_48x64", "noise_64x48", "crop"]
_CACHE = {}


def stages(gpu, name):
    """every stage of the device on input `name`, downloaded; computed once and shared, never modified"""
    if name not in _CACHE:
        from freefine_amd import sift as S
        sift = S.HipSift(gpu)
        img = R.case_inputs()[name]
        base = sift.base(img)
        first = sift.blur(base, R.sigmas()[0])
        pyr = sift.pyramid(base)
        octs = []
        for o, G in enumerate(pyr):
            D, cand = sift.extrema(G)
            rec = sift.refine(D, G, o, cand)
            kp = S.records_to_keypoints(rec.cpu().numpy(), o)
            desc, raw = sift.describe(G, o, kp, want_raw=True)
            octs.append(dict(G=G.cpu().numpy(), D=D.cpu().numpy(), cand=cand.cpu().numpy(), rec=rec.cpu().numpy(), kp=kp, desc=desc.cpu().numpy(), raw=raw.cpu().numpy()))
        _CACHE[name] = dict(img=img, base=base.cpu().numpy(), first=first.cpu().numpy(), octs=octs, sift=sift)
    return _CACHE[name]


@pytest.mark.parametrize("name", NAMES)
def test_base_image_bit_exact(gpu, name):
    st = stages(gpu, name)
    assert np.array_equal(st["base"], R.base_image(st["img"], np.float32))
    assert np.array_equal(st["base"].astype(np.float64), R.base_image(st["img"]))
    assert np.array_equal(st["sift"].base(np.ascontiguousarray(st["img"][..., 1])).cpu().numpy(), R.base_image(st["img"][..., 1], np.float32))     # one channel: taken as gray


@pytest.mark.parametrize("name", NAMES)
def test_blur_within_rounding_bound_and_pyramid_geometry(gpu, name):
    st = stages(gpu, name)
    octs = st["octs"]
    assert len(octs) == R.n_octaves(st["base"].shape) and octs[-1]["G"].shape[1] < 11             # the last octave is below the 11 pixels a candidate needs
    sig = R.sigmas()
    pairs = [(st["base"], st["first"], sig[0])]
    assert np.array_equal(octs[0]["G"][0], st["first"])
    for o, q in enumerate(octs):
        G = q["G"]
        assert G.shape[0] == 6
        pairs += [(G[i], G[i + 1], sig[i + 1]) for i in range(5)]
        if o + 1 < len(octs):
            assert np.array_equal(octs[o + 1]["G"][0], R.decimate(G[3]))
    worst = 0.0
    for src, got, s in pairs:
        taps = R.gauss_taps(s)
        want = R.blur(src.astype(np.float64), taps.astype(np.float64))
        bound = 2 * (len(taps) + 1) * 2.0 ** -24 * np.abs(src).max()
        err = np.abs(got.astype(np.float64) - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (src.shape, len(taps), err, bound)
    print(f"{name}: blur error at most {worst:.3f} of the bound over {len(pairs)} blurs")


@pytest.mark.parametrize("name", NAMES)
def test_dog_and_candidates_bit_identical(gpu, name):
    st = stages(gpu, name)
    total = 0
    for q in st["octs"]:
        assert np.array_equal(q["D"], q["G"][1:] - q["G"][:-1])
        want = R.extrema(q["D"])
        got = q["cand"].astype(np.int64)
        assert len(got) == len(want) and set(map(tuple, got)) == set(map(tuple, want)) and len(set(map(tuple, got))) == len(got)
        if q["D"].shape[1] < 11 or q["D"].shape[2] < 11:
            assert len(got) == 0
        total += len(got)
    assert total >= 10, total


@pytest.mark.parametrize("name", NAMES)
def test_refinement_and_orientation(gpu, name):
    st = stages(gpu, name)
    n = inside = kept = 0
    worst = dict(xy=0.0, size=0.0, angle=0.0, response=0.0)
    for o, q in enumerate(st["octs"]):
        ref = R.refine(q["D"].astype(np.float64), q["G"].astype(np.float64), o, q["cand"])
        for got, want in zip(q["rec"].astype(np.float64), ref):
            n += 1
            if R.inside_margin(want):
                inside += 1
                continue
            w = want["rec"]
            assert bool(got[0]) == want["keep"], (o, got, w, want["slack"])
            if not want["keep"]:
                assert not got.any()
                continue
            kept += 1
            assert tuple(got[1:4]) == tuple(w[1:4]) and got[8] == w[8], (o, got, w, want["slack"])          # final cell, number of peaks
            npk = int(w[8])
            dev = dict(xy=max(abs(got[4] - w[4]), abs(got[5] - w[5])), size=abs(got[6] - w[6]), response=abs(got[7] - w[7]),
                       angle=float(np.max(R.angle_diff(got[9:9 + npk], w[9:9 + npk]), initial=0.0)))
            for k, v in dev.items():
                worst[k] = max(worst[k], v / R.TOL[k])
                assert v <= R.TOL[k], (o, k, v, R.TOL[k], got, w)
            assert not got[9 + npk:].any()
    print(f"{name}: {n} candidates, {kept} kept, {inside} inside the margin; largest deviation / tolerance {worst}")
    assert n >= 10 and kept >= 5
    assert inside <= 0.05 * n, (inside, n)


@pytest.mark.parametrize("name", NAMES)
def test_descriptor(gpu, name):
    st = stages(gpu, name)
    n = skipped = 0
    worst = 0.0
    for o, q in enumerate(st["octs"]):
        raw, u8, rq = R.describe(q["G"].astype(np.float64), o, q["kp"])
        for i in range(len(q["kp"])):
            n += 1
            if abs(rq[i] - np.floor(rq[i]) - 0.5) < R.MARGIN["desc_radius"]:           # the window's radius rounds either way
                skipped += 1
                continue
            err = np.abs(q["raw"][i].astype(np.float64) - raw[i]).max()
            worst = max(worst, err / R.TOL["desc"])
            assert err <= R.TOL["desc"], (o, i, err, q["kp"][i])
            assert np.abs(q["desc"][i].astype(int) - u8[i].astype(int)).max() <= 1
            assert np.array_equal(q["desc"][i], np.clip(np.rint(q["raw"][i]), 0, 255).astype(np.uint8))
    print(f"{name}: {n} descriptors, {skipped} with a radius inside the margin; largest deviation / tolerance {worst:.3f}")
    assert n >= 5 and skipped <= 0.05 * n


def test_matcher_bit_exact_with_ties_and_short_sets(gpu):
    from freefine_amd import sift as S
    st = stages(gpu, "crop")
    sift = st["sift"]
    des1 = np.concatenate([q["desc"] for q in st["octs"]])
    kp2, des2 = sift.detect_and_compute(R.edited(st["img"]))
    filler = np.random.default_rng(9).integers(0, 256, (300, 128), dtype=np.uint8)
    des2 = np.concatenate([des2, filler, des2[3:5], des1[:2]])                  # duplicate rows: equal distances, the lower index wins
    des1 = np.concatenate([des1, des2[3:4]])
    assert len(des1) > 256 or len(des2) > 256                                   # more rows than one workgroup has threads
    for d2 in (des2, des2[:300], des2[:257], des2[:2], des2[:1], des2[:0]):
        idx, dist = (t.cpu().numpy() for t in sift.knn2(des1, d2))
        widx, wdist = R.knn2(des1, d2)
        assert idx.dtype == np.int32 and np.array_equal(idx, widx) and np.array_equal(dist, wdist), len(d2)
        pairs = sift.match_ratio(des1, d2)
        rows = R.ratio_matches(widx, wdist)
        assert np.array_equal(pairs[:, 0], rows) and np.array_equal(pairs[:, 1], widx[rows, 0])
        if len(d2) < 2:
            assert len(pairs) == 0
    idx, dist = (t.cpu().numpy() for t in sift.knn2(des1, des2))
    assert idx[-1].tolist() == [3, len(des2) - 4] and dist[-1].tolist() == [0, 0]
    assert len(sift.match_ratio(des1[:0], des2)) == 0 and S.ratio_pairs(idx, dist).shape[1] == 2


def test_two_runs_give_identical_bytes_and_overflow_is_an_error(gpu):
    from freefine_amd import _lib
    st = stages(gpu, "noise_64x48")
    sift = st["sift"]
    a, b = sift.detect_and_compute(st["img"]), sift.detect_and_compute(st["img"])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[0]) >= 20
    want = R.sort_keypoints(np.concatenate([q["kp"] for q in st["octs"]]), np.concatenate([q["desc"] for q in st["octs"]]))
    assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1])
    import torch
    G = torch.from_numpy(st["octs"][0]["G"]).to(gpu)
    n = len(st["octs"][0]["cand"])
    assert n > 4
    D, cand = sift.extrema(G, cap=n)                                            # exactly enough room
    assert len(cand) == n
    with pytest.raises(_lib.FreeFineHipError, match="rc=-28"):                  # FFN_ENOSPC, never a silently short list
        sift.extrema(G, cap=n - 1)
    D2 = torch.empty_like(D)
    lst = torch.full((n + 8, 3), -7, dtype=torch.int32, device=gpu)
    counter = torch.zeros(1, dtype=torch.int32, device=gpu)
    count = ctypes.c_int(0)
    rc = sift.lib.ffn_sift_extrema(torch.cuda.current_stream().cuda_stream, G.data_ptr(), D2.data_ptr(), G.shape[1], G.shape[2], lst.data_ptr(), 4, counter.data_ptr(),
                                   ctypes.byref(count))
    assert rc == -28 and count.value == n and b"sift_extrema" in sift.lib.ffn_last_error()
    assert (lst[4:] == -7).all().item() and (lst[:4] != -7).all().item()       # nothing written past the list


@pytest.mark.parametrize("name", NAMES)
def test_sift_matches_end_to_end_against_fp64(gpu, name):
    from freefine_amd import sift as S
    st = stages(gpu, name)
    img, gen = st["img"], R.edited(st["img"])
    mask = np.zeros(img.shape[:2])
    mask[4:-4, 4:-4] = 1.0
    got = S.sift_matches(img, gen, mask, st["sift"])
    want, fell_back = R.sift_matches(img, gen, mask)
    assert not fell_back and got.dtype.kind == "i" and got.shape[1] == 2 and (mask[got[:, 0], got[:, 1]] > 0.5).all()
    a, b = set(map(tuple, got.tolist())), set(map(tuple, want.tolist()))
    print(f"{name}: {len(got)} points on the device, {len(want)} in fp64, {len(a ^ b)} differ")
    assert len(b) >= 5 and len(a ^ b) <= 0.10 * max(len(a), len(b))
    if not (a ^ b):
        assert np.array_equal(got, want)                                       # keypoint order


def test_calculate_md_with_sift_keypoints(gpu, tmp_path):
    """the tiny synthetic pipeline end to end: calculate_md(..., keypoints="sift") runs, every keypoint it uses lies in the mask, a HipSift object does the same,
    and a pair with no matches (a flat edited image has no keypoints at all) takes the fallback: the source image's detections in the mask, strongest first"""
    import torch
    from PIL import Image
    from freefine_amd import metrics as FM, ops, sift as S
    from golden_cases import rect_mask, rng_tensor
    from test_pipeline_gpu import make_pipe
    pipe = make_pipe(gpu, "tiny", "edit", torch.float32)
    E = 2
    noise = rng_tensor(41, (E, 4, 16, 16))
    img = R.synthetic("noise", 128, 128, 21)
    mask = rect_mask(128, 128, 30, 100, 24, 96, 255)
    Image.fromarray(img).save(tmp_path / "img.png")
    Image.fromarray(np.full_like(img, 90)).save(tmp_path / "flat.png")
    Image.fromarray(mask).save(tmp_path / "mask.png")
    sample = dict(ori_img_path=str(tmp_path / "img.png"), gen=str(tmp_path / "img.png"), ori_mask_path=str(tmp_path / "mask.png"), edit_param=[5, 12, 0, 0, 0, 0, 1, 1, 1],
                  obj_label="a cup")
    data = {"0": {"instances": {"0": {"0": sample}}}}
    seen = []
    real = ops.dift_match

    def spy(rows_s, rows_e, hw, HW, kps):
        seen.append(np.asarray(kps).copy())
        return real(rows_s, rows_e, hw, HW, kps)
    ops.dift_match = spy
    try:
        md = FM.calculate_md(data, "gen", pipe, keypoints="sift", ensemble_size=E, noise=noise)
        md_obj = FM.calculate_md(data, "gen", pipe, keypoints=S.HipSift(gpu), ensemble_size=E, noise=noise)
        flat = {"0": {"instances": {"0": {"0": dict(sample, gen=str(tmp_path / "flat.png"))}}}}
        md_flat = FM.calculate_md(flat, "gen", pipe, keypoints="sift", ensemble_size=E, noise=noise)
    finally:
        ops.dift_match = real
    assert len(seen) == 3 and all(1 <= len(k) <= 30 and (mask[k[:, 0], k[:, 1]] > 127).all() for k in seen)
    assert abs(md - 13.0) <= 1e-6 and md_obj == md and np.isfinite(md_flat)     # an image against itself with the same noise: every keypoint matches itself
    sift = S.HipSift(gpu)
    pts, fell_back = S.sift_matches(img, img, mask / 255.0, sift, return_fallback=True)
    assert not fell_back and np.array_equal(seen[0], pts[:30]) and np.array_equal(seen[1], seen[0])
    pts, fell_back = S.sift_matches(img, np.full_like(img, 90), mask / 255.0, sift, return_fallback=True)
    assert fell_back and np.array_equal(seen[2], pts[:30])
    kp, _ = sift.detect_and_compute(img)
    inside = kp[(mask[kp[:, 1].astype(int), kp[:, 0].astype(int)] > 127)]
    strongest = inside[np.argsort(-inside[:, 4], kind="stable")]
    assert np.array_equal(pts, np.stack([strongest[:, 1].astype(np.int64), strongest[:, 0].astype(np.int64)], 1))
    with pytest.raises(ValueError, match="sift"):
        FM.calculate_md(data, "gen", pipe, keypoints="orb")
