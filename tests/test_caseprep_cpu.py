"""CPU: host side of the device case preparation (freefine_amd.ops lanczos4_taps / nearest_indices / edit_inverse_affine, the ABI entries, the thread rule of
geobench.run(device_prep=True)).  The device kernels themselves: tests/test_caseprep_gpu.py."""
import os
import re
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ffn_resize_taps8_u8", "ffn_resize_gather_u8", "ffn_dilate_u8", "ffn_coarse_edit_2d")
# (n_dst, n_src) of every axis the GPU tests resize
PAIRS = [(64, 37), (48, 53), (7, 20), (31, 9), (11, 5), (13, 3), (512, 1024), (512, 768), (512, 300), (128, 160)]


def test_entries_are_declared_bound_and_exported():
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    declared = set(re.findall(r"\b(ffn_[a-z0-9_]+)\s*\(", header))
    for name in ENTRIES:
        assert name in declared and name in _lib.SYMBOLS, name
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfreefine_hip.so not built")
    lib = _lib.load()
    assert lib.ffn_version() >= 9
    for name in ENTRIES:
        assert hasattr(lib, name)


def test_bad_arguments_are_refused_before_any_launch():
    """no GPU needed: validation comes first.  A side above FFN_IMGPREP_MAX_SIDE, C = 2, k outside 1 .. 255, B = 0, null pointers."""
    import ctypes
    from freefine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfreefine_hip.so not built")
    lib = _lib.load()
    p, big = 0x10000, _lib.IMGPREP_MAX_SIDE + 1                  # never dereferenced
    assert lib.ffn_resize_taps8_u8(None, p, p, 1, big, 8, 3, 8, 8, p, p, p, p) == -22 and b"FFN_IMGPREP_MAX_SIDE" in lib.ffn_last_error()
    assert lib.ffn_resize_taps8_u8(None, p, p, 1, 8, 8, 3, 8, big, p, p, p, p) == -22
    assert lib.ffn_resize_taps8_u8(None, p, p, 1, 8, 8, 2, 8, 8, p, p, p, p) == -22 and b"C=2" in lib.ffn_last_error()
    assert lib.ffn_resize_taps8_u8(None, p, p, 1, 8, 8, 3, 8, 8, p, None, p, p) == -22
    assert lib.ffn_resize_gather_u8(None, p, p, 1, 8, big, 1, 8, 8, p, p, 0) == -22
    assert lib.ffn_resize_gather_u8(None, p, p, 0, 8, 8, 1, 8, 8, p, p, 0) == -22
    assert lib.ffn_resize_gather_u8(None, p, p, 1, 8, 8, 2, 8, 8, p, p, 0) == -22
    for k in (0, 256):
        assert lib.ffn_dilate_u8(None, p, p + 4096, p + 8192, 1, 8, 8, 1, k) == -22 and b"k=" in lib.ffn_last_error()
    assert lib.ffn_dilate_u8(None, p, p, p + 8192, 1, 8, 8, 1, 3) == -22
    assert lib.ffn_dilate_u8(None, p, p + 4096, p + 8192, 1, 8, 8, 2, 3) == -22
    assert lib.ffn_mask_bbox_u8(None, p, p, 1, 8, big, 1) == -22
    d = _lib.CoarseEditDesc()
    assert lib.ffn_coarse_edit_2d(None, None) == -22
    assert lib.ffn_coarse_edit_2d(None, ctypes.byref(d)) == -22
    for f in ("src_img", "src_mask", "bg", "inv", "final_img", "tmask", "trans_hole"):
        setattr(d, f, p)
    d.B, d.H, d.W, d.mask_c = 1, 8, big, 1
    assert lib.ffn_coarse_edit_2d(None, ctypes.byref(d)) == -22 and b"FFN_IMGPREP_MAX_SIDE" in lib.ffn_last_error()
    d.W, d.mask_c = 8, 2
    assert lib.ffn_coarse_edit_2d(None, ctypes.byref(d)) == -22
    d.mask_c, d.hole_mask, d.hole_mask_c = 1, p, 2
    assert lib.ffn_coarse_edit_2d(None, ctypes.byref(d)) == -22


@pytest.mark.parametrize("n_dst,n_src", PAIRS)
def test_lanczos4_taps_scatter_to_the_dense_matrix(n_dst, n_src):
    from freefine_amd import ops
    from src.utils.vis_utils import _lanczos4_matrix
    idx, wgt = ops.lanczos4_taps(n_dst, n_src)
    assert idx.dtype == np.int32 and wgt.dtype == np.float64 and idx.shape == wgt.shape == (n_dst, 8)
    assert idx.min() >= 0 and idx.max() <= n_src - 1
    M = np.zeros((n_dst, n_src))
    for j in range(8):
        np.add.at(M, (np.arange(n_dst), idx[:, j]), wgt[:, j])
    assert np.abs(M - _lanczos4_matrix(n_dst, n_src)).max() <= 1e-15


@pytest.mark.parametrize("n_dst,n_src", PAIRS)
def test_nearest_indices_are_those_of_resize_nearest(n_dst, n_src):
    from freefine_amd import ops
    from src.utils.vis_utils import _resize_nearest
    idx = ops.nearest_indices(n_dst, n_src)
    assert idx.dtype == np.int32 and idx.shape == (n_dst,)
    ramp = np.arange(n_src, dtype=np.int64)
    assert np.array_equal(idx, _resize_nearest(np.tile(ramp[:, None], (1, 2)), (2, n_dst))[:, 0])      # rows
    assert np.array_equal(idx, _resize_nearest(np.tile(ramp[None, :], (2, 1)), (n_dst, 2))[0])         # columns


def test_edit_inverse_affine_is_the_matrix_warp_affine_inverts():
    from freefine_amd import ops
    from src.utils import vis_utils as V
    mask = np.zeros((48, 80), np.uint8)
    mask[10:30, 20:60] = 1
    for ep in [(0.5, 0.5, 0, 1, 1), (7, -3, 25.0, 1.2, 0.8), (30, 0, 90, 1, 1), (-25, 10, 45, 0.5, 1.5), (7, -3, 0, 0, 0, 25.0, 1.2, 0.8, 1)]:
        p5 = ep if len(ep) == 5 else (ep[0], ep[1], ep[5], ep[6], ep[7])
        Ai = np.linalg.inv(np.vstack([V._affine_for_edit(mask, *p5), [0, 0, 1]]))
        got = ops.edit_inverse_affine((10, 29, 20, 59), ep)
        assert got.dtype == np.float64 and np.array_equal(got, Ai[:2].reshape(6))      # the same bits: the same expressions in the same order


def test_host_prep_loaders_equal_the_vis_utils_calls(tmp_path):
    """the default (host) route of the reworked loaders with REAL resizes (160 -> 128): what the vis_utils functions give when called as the drivers call them"""
    from freefine_amd import geobench
    from src.utils import vis_utils as V
    root = str(tmp_path / "geo")
    geobench.make_synthetic_dataset(root, n_images=1, edits_per_image=2, size=160, seed=4)
    cl = geobench.CaseList(V.load_json(os.path.join(root, "annotations_2d.json")), os.path.join(root, geobench.GEN_SUBDIR))
    for case in cl.cases:
        got = geobench.load_case(case, root, (128, 128))
        bg = V.read_and_resize_img(os.path.join(root, geobench.INP_SUBDIR, case["da_n"], case["ins_id"], "inp_img.png"), (128, 128))
        img, mask = V.read_and_resize_img(case["ori_img_path"], (128, 128)), V.read_and_resize_mask(case["ori_mask_path"], (128, 128))
        coarse, tmask = V.re_edit_2d(img, mask, case["edit_param"], bg)[:2]
        for k, want in dict(ori_img=img, ori_mask=mask, coarse_input=coarse, target_mask=tmask, cons_area=tmask, draw_mask=np.ones_like(mask)).items():
            assert got[k].dtype == want.dtype and np.array_equal(got[k], want), k
    imgs, holes = geobench.bggen_inputs(cl.cases[:1], (128, 128))
    assert np.array_equal(imgs[0], V.read_and_resize_img(cl.cases[0]["ori_img_path"], (128, 128)))
    assert np.array_equal(holes[0], V.read_and_resize_mask_with_dilation(cl.cases[0]["ori_mask_path"], (128, 128), dilation_factor=30))


class _FakeModel:
    device = "cpu"

    def FreeFine_generation(self, ori_img, *a, **kw):
        return ori_img

    def FreeFine_generation_batch(self, inputs, *a, **kw):
        return [c["ori_img"] for c in inputs]


def test_device_prep_issues_no_device_call_from_the_prefetch_thread(tmp_path, monkeypatch):
    """run(device_prep=True) with the ops replaced by host stand-ins that record the calling thread: every one of them runs on the consumer (this) thread, the
    prefetch thread only decodes, and the run's images equal those of a host-prep run."""
    import torch
    from PIL import Image
    from freefine_amd import geobench, ops
    from src.utils import vis_utils as V
    calls = []

    def note(name):
        calls.append((name, threading.current_thread()))

    def t2n(t):
        return t.numpy()

    def lanczos(img, dsize):
        note("resize_lanczos4_u8")
        return torch.from_numpy(V._resize_lanczos4(t2n(img), dsize))

    def nearest(img, dsize, binarise=False):
        note("resize_nearest_u8")
        m = V._resize_nearest(t2n(img), dsize)
        if binarise:
            m[m > 0] = 1
        return torch.from_numpy(m)

    def dilate(m, k):
        note("dilate_u8")
        return torch.from_numpy(V.dilate_mask(t2n(m), k))

    def edit(img, mask, ep, bg, hole_img=None, hole_mask=None):
        note("coarse_edit_2d")
        return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in V.re_edit_2d(t2n(img), t2n(mask), ep, t2n(bg)))
    for name, fn in dict(resize_lanczos4_u8=lanczos, resize_nearest_u8=nearest, dilate_u8=dilate, coarse_edit_2d=edit).items():
        monkeypatch.setattr(ops, name, fn)
    decodes = []
    real_imread = geobench._imread_bgr
    monkeypatch.setattr(geobench, "_imread_bgr", lambda p: (decodes.append(threading.current_thread()), real_imread(p))[1])
    outs = {}
    for dev in (False, True):
        root = str(tmp_path / f"geo{int(dev)}")
        geobench.make_synthetic_dataset(root, n_images=2, edits_per_image=2, size=80, seed=1)
        calls.clear()
        decodes.clear()
        res = geobench.run(_FakeModel(), root, batch=3, verbose=False, dsize=(64, 64), device_prep=dev)
        assert len(res) == 4
        outs[dev] = [np.asarray(Image.open(r["gen_img_path"])) for r in sorted(res, key=lambda r: r["key"])]
        assert decodes and all(t is not threading.current_thread() for t in decodes)          # files are read on the prefetch thread in both modes
        if dev:
            assert {n for n, _ in calls} == {"resize_lanczos4_u8", "resize_nearest_u8", "coarse_edit_2d"} and len(calls) == 4 * 4
            assert all(t is threading.current_thread() for _, t in calls)
        else:
            assert calls == []
    assert all(np.array_equal(a, b) for a, b in zip(outs[False], outs[True]))
    # the background stage: two resizes and the dilation per case, on the calling thread
    calls.clear()
    cases = [dict(ori_img_path=os.path.join(root, "source", "0000", "img.png"), ori_mask_path=os.path.join(root, "source", "0000", "mask_0.png"))]
    dev_in = geobench.bggen_inputs(cases, (64, 64), geobench.DevicePrep("cpu"))
    host_in = geobench.bggen_inputs(cases, (64, 64))
    assert [n for n, _ in calls] == ["resize_lanczos4_u8", "resize_nearest_u8", "dilate_u8"]
    assert np.array_equal(dev_in[0][0], host_in[0][0]) and np.array_equal(dev_in[1][0], host_in[1][0])
