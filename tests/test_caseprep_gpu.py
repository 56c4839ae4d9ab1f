"""GPU: the device case preparation of the GeoBench harness (csrc/caseprep.h through freefine_amd.ops and geobench.DevicePrep) against the numpy functions of
src/utils/vis_utils.py, computed on the CPU in the same test.  Every comparison is BYTE EQUALITY: no byte may differ, there is no allowance.  (Both sides are
pinned to the numpy restatement of the cv2 calls, not to OpenCV.)"""
import os

import numpy as np
import pytest
import torch

from src.utils import vis_utils as V

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
torch.set_grad_enabled(False)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# Lanczos-4
# ---------------------------------------------------------------------------------------------------------------------
def lanczos_taps_image(img, dsize):
    """the fp64 image before rounding, in the kernel's own order: vertical first, then horizontal, each sum from 0 over taps in ascending j"""
    from freefine_amd import ops
    w, h = dsize
    H, W = img.shape[:2]
    iy, wy = ops.lanczos4_taps(h, H)
    ix, wx = ops.lanczos4_taps(w, W)
    f = img.astype(np.float64)
    v = np.zeros((h, W, img.shape[2]))
    for j in range(8):
        v = v + wy[:, j][:, None, None] * f[iy[:, j]]
    out = np.zeros((h, w, img.shape[2]))
    for j in range(8):
        out = out + wx[:, j][None, :, None] * v[:, ix[:, j]]
    return out


def half_integer_margin(pre):
    """smallest distance of a pre-rounding value from a half-integer (where a last-bit difference in the sum could flip the byte)"""
    return float(np.abs(np.abs(pre - np.floor(pre) - 0.5)).min())


LANCZOS = [((37, 53), (64, 48)), ((20, 9), (7, 31)), ((5, 3), (11, 13)), ((1024, 768), (512, 512))]      # (H, W) -> (h, w)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("src,dst", LANCZOS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lanczos4_resize_is_the_numpy_function_byte_for_byte(gpu, src, dst, C):
    from freefine_amd import ops
    rng = np.random.default_rng(src[0] * 7 + C)
    img = rng.integers(0, 256, src + (C,), dtype=np.uint8)
    dsize = (dst[1], dst[0])
    pre = lanczos_taps_image(img, dsize)
    margin = half_integer_margin(pre)
    print(f"lanczos {src} -> {dst} C={C}: closest approach to a half-integer {margin:.3e}")
    assert margin > 1e-9                     # the condition on the input: summation order (einsum vs the 8-tap loop) cannot flip a byte
    want = V._resize_lanczos4(img, dsize)
    got = _np(ops.resize_lanczos4_u8(_dev(img, gpu), dsize))
    assert got.shape == want.shape and got.dtype == np.uint8
    print(f"  mismatching bytes vs _resize_lanczos4: {int((got != want).sum())}")
    assert np.array_equal(got, np.clip(np.rint(pre), 0, 255).astype(np.uint8))        # the ordered tap loop, restated in numpy
    assert np.array_equal(got, want)


def test_lanczos4_equal_size_is_a_copy_and_batches_are_independent(gpu):
    from freefine_amd import ops
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)
    t = _dev(img, gpu)
    same = ops.resize_lanczos4_u8(t, (48, 64))
    assert same.data_ptr() != t.data_ptr() and np.array_equal(_np(same), V._resize_lanczos4(img, (48, 64))) and np.array_equal(_np(same), img)
    pair = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    for b in range(2):
        assert half_integer_margin(lanczos_taps_image(pair[b], (48, 64))) > 1e-9
    got = _np(ops.resize_lanczos4_u8(_dev(pair, gpu), (48, 64)))
    assert got.shape == (2, 64, 48, 3)
    for b in range(2):
        assert np.array_equal(got[b], V._resize_lanczos4(pair[b], (48, 64)))


# ---------------------------------------------------------------------------------------------------------------------
# nearest
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((37, 53), (64, 48)), ((300, 300), (512, 512))], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nearest_resize_and_mask_binarisation(gpu, src, dst):
    from freefine_amd import ops
    rng = np.random.default_rng(5)
    dsize = (dst[1], dst[0])
    for shape in (src + (3,), src + (1,), src):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(_np(ops.resize_nearest_u8(_dev(img, gpu), dsize)), V._resize_nearest(img, dsize))
    mask = (rng.integers(0, 4, src + (3,)) == 0).astype(np.uint8) * rng.integers(1, 256, src + (3,), dtype=np.uint8)      # three channels, values 0 / 1 .. 255
    want = V._resize_nearest(mask, dsize)
    want[want > 0] = 1                                                                                                   # read_and_resize_mask
    got = _np(ops.resize_nearest_u8(_dev(mask, gpu), dsize, binarise=True))
    assert set(np.unique(got)) == {0, 1} and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# dilation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 15, 16, 30])
def test_dilation_is_the_maximum_filter(gpu, k):
    from freefine_amd import ops
    rng = np.random.default_rng(k)
    flat = (rng.integers(0, 12, (9, 40)) == 0).astype(np.uint8) * rng.integers(1, 256, (9, 40), dtype=np.uint8)       # 2-D, k may exceed a side
    assert np.array_equal(_np(ops.dilate_u8(_dev(flat, gpu), k)), V.dilate_mask(flat, k))
    rgb = (rng.integers(0, 40, (33, 47, 3)) == 0).astype(np.uint8) * rng.integers(1, 256, (33, 47, 3), dtype=np.uint8)
    assert np.array_equal(_np(ops.dilate_u8(_dev(rgb, gpu), k)), V.dilate_mask(rgb, k))
    one = np.zeros((9, 40), np.uint8)
    one[4, 20] = 200                                                             # a single set pixel: the window's asymmetry for even k
    got = _np(ops.dilate_u8(_dev(one, gpu), k))
    assert np.array_equal(got, V.dilate_mask(one, k))
    cols = np.nonzero(got[4])[0]
    assert (cols.min(), cols.max()) == (20 - (k - k // 2 - 1), 20 + k // 2)      # k = 2: 20 .. 21; k = 16: 13 .. 28 (-7 .. +8)
    edge = np.zeros((21, 26, 3), np.uint8)
    edge[0, :, 0] = edge[-1, :, 1] = 1
    edge[:, 0, 2] = edge[:, -1, 0] = 3                                           # touches all four borders
    assert np.array_equal(_np(ops.dilate_u8(_dev(edge, gpu), k)), V.dilate_mask(edge, k))
    batch = np.stack([rgb, rgb[::-1].copy()])
    got = _np(ops.dilate_u8(_dev(batch, gpu), k))
    assert np.array_equal(got[0], V.dilate_mask(batch[0], k)) and np.array_equal(got[1], V.dilate_mask(batch[1], k))


def test_mask_with_dilation_and_forbidden_area(gpu, tmp_path):
    from PIL import Image
    from freefine_amd import geobench
    mask = np.zeros((90, 70), np.uint8)
    mask[30:50, 20:45] = 255
    path = str(tmp_path / "m.png")
    Image.fromarray(mask).save(path)
    forbid = np.zeros((64, 64, 3), bool)
    forbid[:, 30:] = True
    prep = geobench.DevicePrep(gpu)
    for k, fa in ((None, None), (15, None), (30, forbid), (None, forbid)):
        want = V.read_and_resize_mask_with_dilation(path, (64, 64), dilation_factor=k, forbit_area=fa)
        got = geobench._prep_mask(geobench._decode_mask(path), (64, 64), prep, dilation_factor=k, forbit_area=fa)
        assert got.dtype == want.dtype and np.array_equal(got, want), (k, fa is not None)


# ---------------------------------------------------------------------------------------------------------------------
# coarse edit
# ---------------------------------------------------------------------------------------------------------------------
def _edit_inputs(H, W, seed, box):
    rng = np.random.default_rng(seed)
    img, bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = np.zeros((H, W), np.uint8)
    mask[box[0]:box[1], box[2]:box[3]] = 1
    return img, mask, bg


def _assert_edit(got, want, what):
    for name, g, w in zip(("final", "target mask", "trans_hole"), got, want):
        g = _np(g)
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), (what, name, int((g != w).sum()))


PARAMS = [(0.5, 0.5, 0, 1, 1), (7, -3, 25.0, 1.2, 0.8), (30, 0, 90, 1, 1), (-25, 10, 45, 0.5, 1.5), (50, 0, 0, 1, 1),      # (50, 0): half out of the frame
          (7, -3, 0, 0, 0, 25.0, 1.2, 0.8, 1)]                                                                               # the 9-tuple form


@pytest.mark.parametrize("ep", PARAMS, ids=str)
def test_coarse_edit_is_re_edit_2d_byte_for_byte(gpu, ep):
    from freefine_amd import ops
    img, mask, bg = _edit_inputs(48, 80, 2, (10, 30, 20, 60))
    want = V.re_edit_2d(img, mask, ep, bg)
    if ep == PARAMS[0]:      # the half-pixel shift: the blend of every interior pixel is a multiple of 1/4, exact .5 ties are rounded to even
        assert want[1][11:30, 21:60].all()
    _assert_edit(ops.coarse_edit_2d(_dev(img, gpu), _dev(mask, gpu), ep, _dev(bg, gpu)), want, ep)
    m3 = np.repeat(mask[:, :, None], 3, axis=2) * 255                            # a three-channel 0 / 255 mask: channel 0 is used
    _assert_edit(ops.coarse_edit_2d(_dev(img, gpu), _dev(m3, gpu), ep, _dev(bg, gpu)), V.re_edit_2d(img, m3, ep, bg), (ep, "3ch"))


def test_coarse_edit_second_view_batch_and_full_size(gpu):
    from freefine_amd import ops
    img, mask, bg = _edit_inputs(48, 80, 3, (10, 30, 20, 60))
    rng = np.random.default_rng(9)
    img_a = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    mask_a = (rng.integers(0, 3, (48, 80, 3)) == 0).astype(np.uint8)            # per-channel, as numpy's where broadcasts it
    ep = (7, -3, 25.0, 1.2, 0.8)
    want = V.re_edit_3d(img, mask, ep, bg, img_a, mask_a)
    _assert_edit(ops.coarse_edit_2d(_dev(img, gpu), _dev(mask, gpu), ep, _dev(bg, gpu), _dev(img_a, gpu), _dev(mask_a, gpu)), want, "re_edit_3d")
    want1 = V.re_edit_3d(img, mask, ep, bg, img_a, mask_a[:, :, :1])
    _assert_edit(ops.coarse_edit_2d(_dev(img, gpu), _dev(mask, gpu), ep, _dev(bg, gpu), _dev(img_a, gpu), _dev(mask_a[:, :, :1], gpu)), want1, "re_edit_3d 1ch")
    # B = 3, another image, mask and parameter set per case
    cases = [_edit_inputs(48, 80, 20 + b, box) for b, box in enumerate([(10, 30, 20, 60), (0, 12, 0, 9), (40, 48, 70, 80)])]
    eps = [PARAMS[1], PARAMS[3], PARAMS[5]]
    got = ops.coarse_edit_2d(_dev(np.stack([c[0] for c in cases]), gpu), _dev(np.stack([c[1] for c in cases]), gpu), eps,
                             _dev(np.stack([c[2] for c in cases]), gpu))
    for b in range(3):
        _assert_edit([g[b] for g in got], V.re_edit_2d(cases[b][0], cases[b][1], eps[b], cases[b][2]), ("batch", b))
    # once at 512 x 512
    img, mask, bg = _edit_inputs(512, 512, 4, (100, 290, 150, 380))
    ep = (-60.5, 33.25, -37.0, 1.3, 0.7)
    _assert_edit(ops.coarse_edit_2d(_dev(img, gpu), _dev(mask, gpu), ep, _dev(bg, gpu)), V.re_edit_2d(img, mask, ep, bg), "512")


def test_coarse_edit_reproduces_the_reference_tower_example(gpu):
    """the statement tests/test_vis_utils_cpu.py makes for the host path (tests/golden/g12_tower_coarse_edit.npz, the reference's own input -> output set), for
    the device path: target mask exact over the full frame, coarse image exact inside it."""
    from freefine_amd import ops
    g = np.load(os.path.join(GOLD, "g12_tower_coarse_edit.npz"))
    sm640 = np.unpackbits(g["source_mask_640"]).reshape(640, 640).astype(np.uint8) * 255
    tm = np.unpackbits(g["target_mask_512"]).reshape(512, 512).astype(np.uint8) * 255
    param = tuple(g["edit_param"].tolist())
    sm_dev = ops.resize_nearest_u8(_dev(sm640, gpu), (512, 512), binarise=True)
    sm = _np(sm_dev)
    zero = torch.zeros((512, 512, 3), dtype=torch.uint8, device=gpu)
    _, tmask, _ = ops.coarse_edit_2d(zero, sm_dev, param, zero)
    assert np.array_equal(_np(tmask), tm)
    x0, x1 = (int(v) for v in g["crop"])
    src_c, co_c = g["source_crop"], g["coarse_crop"]
    bg = np.full_like(src_c, 7)
    final, tmask_c, hole = (_np(t) for t in ops.coarse_edit_2d(_dev(src_c, gpu), _dev(sm[:, x0:x1], gpu), param, _dev(bg, gpu)))
    band = np.zeros((512, x1 - x0), bool)
    band[:, :x1 - x0 - 50] = True
    inside = (tm[:, x0:x1] > 0) & band
    assert inside.sum() > 25000 and np.array_equal(tmask_c[band] > 0, tm[:, x0:x1][band] > 0)
    assert np.array_equal(final[inside], co_c[inside])
    assert (final[~(tmask_c > 0)] == 7).all()
    assert (hole[(sm[:, x0:x1] > 0) & ~(tmask_c > 0)] == 0).all()


def test_empty_mask_and_unsupported_images_are_refused(gpu):
    from freefine_amd import _lib, ops
    img = torch.zeros((48, 80, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        ops.coarse_edit_2d(img, torch.zeros((48, 80), dtype=torch.uint8, device=gpu), (1, 1, 0, 1, 1), img)
    tall = torch.zeros((_lib.IMGPREP_MAX_SIDE + 1, 4, 3), dtype=torch.uint8, device=gpu)
    two = torch.zeros((8, 8, 2), dtype=torch.uint8, device=gpu)
    for fn in (lambda: ops.resize_lanczos4_u8(tall, (8, 8)), lambda: ops.resize_lanczos4_u8(two, (4, 4)), lambda: ops.resize_nearest_u8(tall, (8, 8)),
               lambda: ops.resize_nearest_u8(two, (4, 4)), lambda: ops.dilate_u8(tall, 3), lambda: ops.dilate_u8(two, 3),
               lambda: ops.coarse_edit_2d(tall, tall[:, :, 0].contiguous(), (1, 1, 0, 1, 1), tall)):
        with pytest.raises(_lib.FreeFineHipError, match="rc=-22"):
            fn()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# loaders and the harness
# ---------------------------------------------------------------------------------------------------------------------
def test_loaders_on_the_device_equal_the_host_loaders(gpu, tmp_path):
    from freefine_amd import geobench
    root = str(tmp_path / "geo")
    geobench.make_synthetic_dataset(root, n_images=2, edits_per_image=2, size=160, seed=3, with_3d=True)
    prep = geobench.DevicePrep(gpu)
    cl = geobench.CaseList(V.load_json(os.path.join(root, "annotations_2d.json")), os.path.join(root, geobench.GEN_SUBDIR))
    assert len(cl) == 4
    for loader in (geobench.load_case, geobench.load_case_3d_depth):
        for case in cl.cases:
            host, dev = loader(case, root, (128, 128)), loader(case, root, (128, 128), prep=prep)
            assert set(host) == set(dev)
            for k, v in host.items():
                if isinstance(v, np.ndarray):
                    assert isinstance(dev[k], np.ndarray) and dev[k].dtype == v.dtype and np.array_equal(dev[k], v), (loader.__name__, k)
                else:
                    assert dev[k] == v, k
    for case in cl.cases[:2]:        # the 3d_rgb reader: decoded only on the thread, resized on the device afterwards
        host = geobench.read_case_3d_rgb(case, root, (128, 128))
        dev = geobench._resize_case_3d_rgb(geobench.read_case_3d_rgb(case, root, (128, 128), prep=None), prep)
        for k in ("ori_img", "ori_mask", "bg"):
            assert host[k].shape[:2] == (128, 128) and np.array_equal(host[k], dev[k]), k
    icl = geobench.InpaintCaseList(V.load_json(os.path.join(root, "annotations_2d.json")), os.path.join(root, "none"))
    (himg, hhole), (dimg, dhole) = geobench.bggen_inputs(icl.cases, (128, 128)), geobench.bggen_inputs(icl.cases, (128, 128), prep)
    assert len(himg) == 2
    for a, b in zip(himg + hhole, dimg + dhole):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_harness_with_device_prep_writes_the_same_images(gpu, tmp_path):
    """geobench.run on one synthetic tree, prepared on the host and on the device: identical inputs, seeds and batch split -> identical PNG bytes"""
    from PIL import Image
    from freefine_amd import geobench
    from test_pipeline_gpu import make_pipe
    model = make_pipe(gpu, "tiny", "edit", graph=True)
    params = dict(num_step=10, start_step=7, end_step=10)
    imgs = {}
    for dev in (False, True):
        root = str(tmp_path / f"geo{int(dev)}")
        geobench.make_synthetic_dataset(root, n_images=2, edits_per_image=2, size=160, seed=3)
        res = geobench.run(model, root, batch=3, params=params, dsize=(128, 128), verbose=False, device_prep=dev)
        assert len(res) == 4
        imgs[dev] = {r["key"]: np.asarray(Image.open(r["gen_img_path"])) for r in res}
    assert set(imgs[False]) == set(imgs[True])
    for k, v in imgs[False].items():
        assert v.shape == (128, 128, 3) and np.array_equal(v, imgs[True][k]), k
