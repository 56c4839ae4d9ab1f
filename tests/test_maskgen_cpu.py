"""CPU: automatic mask generation as far as it runs without a device -- tests/maskgen_ref.py (the project's restatement) pinned to what the reference's own
segment_anything/utils/amg.py computes (tests/golden/g19_amg.npz, tools/gen_golden_amg.py), the two ABI entries and their refusals, the host-side mask pool
and the command line.  The device: tests/test_maskgen_gpu.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import maskgen_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ffn_upsample_bicubic_stats", "ffn_box_nms")
_G19 = {}


def g19():
    if not _G19:
        _G19.update(np.load(os.path.join(ROOT, "tests", "golden", "g19_amg.npz")))
    return _G19


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_equals_the_reference_golden(name):
    """integers and the fp32 quotients exactly; the empty map's 0 / 0 as NaN"""
    G = g19()
    x, offset = G["stack_" + name], float(G["offset"])
    assert x.dtype == np.float32 and x.shape[0] == 7
    got, want = MR.stability_score(x, offset), G["stability_" + name]
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    assert np.isnan(want[0]) and not np.isnan(want[1:]).any()  # all below -offset: 0 / 0
    for rule, mask in (("gt", x > 0), ("ge", x >= 0)):
        box = MR.mask_to_box(mask)
        assert np.array_equal(box, G[f"box_{rule}_{name}"])
        assert np.array_equal(np.stack([MR.box_xyxy_to_xywh(b) for b in box]), G[f"xywh_{rule}_{name}"])
    # the fixture's special maps do what they are there for
    ge, gt = G["box_ge_" + name], G["box_gt_" + name]
    h, w = x.shape[1:]
    assert gt[0].tolist() == [0, 0, 0, 0] and gt[1].tolist() == [0, 0, w - 1, h - 1] and (gt[2, :2] == gt[2, 2:]).all()
    assert gt[3].tolist() == [0, 0, 0, 0] and ge[3].tolist() == [2, 1, w - 2, h - 2]          # exact zeros: in the project's mask, not in SAM's
    assert ge[5].tolist() == [0, 0, w - 1, h - 1]
    n_hi, n_lo = MR.stability_counts(x, offset)
    assert n_hi[4] == (x[4] > 1).sum() < (x[4] >= 1).sum() and n_lo[4] == (x[4] > -1).sum() < (x[4] >= -1).sum()       # the comparisons are strict
    # the statistics vector is these numbers
    st = MR.stats(x, offset)
    assert st.dtype == np.int32 and np.array_equal(st[:, 3:7], ge) and np.array_equal(st[:, 0], (x >= 0).sum((1, 2))) and (st[:, 7] == 0).all()
    assert np.array_equal(st[:, 1], n_hi) and np.array_equal(st[:, 2], n_lo)


def test_point_grids_equal_the_reference():
    from freefine_amd import sam
    for n in (1, 2, 5):
        want = g19()[f"grid_{n}"]
        assert want.shape == (n * n, 2) and want.dtype == np.float64
        assert np.array_equal(MR.build_point_grid(n), want) and np.array_equal(sam.build_point_grid(n), want)
    assert np.array_equal(sam.box_xyxy_to_xywh(np.array([3, 4, 10, 6])), [3, 4, 7, 2])


def test_greedy_nms_of_the_restatement():
    """the definition on cases small enough to read: duplicates, the NaN rule, an IoU equal to the threshold, ties, and a chain"""
    dup = [[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30]]
    assert MR.nms(dup, [0.9, 0.8, 0.7], 0.5) == [0, 2]
    assert MR.nms(dup, [0.5, 0.5, 0.5], 0.5) == [0, 2]                         # ties: the caller's order
    assert MR.nms([[5, 5, 5, 5], [5, 5, 5, 5]], [1.0, 0.5], 0.5) == [0, 1]     # 0 / 0 is NaN, which is not > thresh
    assert float(MR.iou_f32([0, 0, 2, 2], [0, 0, 2, 1])) == 0.5 and MR.nms([[0, 0, 2, 2], [0, 0, 2, 1]], [1.0, 0.5], 0.5) == [0, 1]
    chain = [[0, 0, 10, 10], [4, 0, 14, 10], [8, 0, 18, 10]]                   # 0 suppresses 1; 1 would have suppressed 2; 0 does not
    assert MR.iou_f32(chain[0], chain[1]) > 0.4 > MR.iou_f32(chain[0], chain[2])
    assert MR.nms(chain, [0.9, 0.8, 0.7], 0.4) == [0, 2]


def test_entries_are_declared_bound_and_exported():
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", header) and name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+FFN_BOX_NMS_MAX\s+16384", header) and _lib.BOX_NMS_MAX == 16384
    lib = _lib.load()
    assert lib.ffn_version() >= 14
    for name in ENTRIES:
        assert hasattr(lib, name)


def test_bad_arguments_are_refused_before_any_launch():
    """no GPU needed: validation comes first"""
    from freefine_amd import _lib
    lib = _lib.load()
    p, big = 0x10000, _lib.IMGPREP_MAX_SIDE + 1                  # never dereferenced
    ok = dict(src=p, stats=p, mask=None, N=1, h=8, w=8, H=16, W=16, offset=1.0)

    def stats(**kw):
        a = dict(ok, **kw)
        return lib.ffn_upsample_bicubic_stats(None, a["src"], a["stats"], a["mask"], a["N"], a["h"], a["w"], a["H"], a["W"], a["offset"])
    for bad in (dict(src=None), dict(stats=None), dict(N=0), dict(N=65536), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(h=big), dict(w=big), dict(H=big),
                dict(W=big), dict(offset=-0.5), dict(offset=float("nan")), dict(offset=float("inf"))):
        assert stats(**bad) == -22 and b"upsample_bicubic_stats" in lib.ffn_last_error(), bad
    assert stats(W=big) == -22 and b"FFN_IMGPREP_MAX_SIDE" in lib.ffn_last_error()
    assert stats(offset=-1.0) == -22 and b"offset" in lib.ffn_last_error()
    for args in ((None, p, 4, 0.5), (p, None, 4, 0.5), (p, p, 0, 0.5), (p, p, _lib.BOX_NMS_MAX + 1, 0.5), (p, p, 4, float("nan")), (p, p, 4, float("inf"))):
        assert lib.ffn_box_nms(None, *args) == -22 and b"box_nms" in lib.ffn_last_error(), args
    assert lib.ffn_box_nms(None, p, p, _lib.BOX_NMS_MAX + 1, 0.5) == -22 and b"FFN_BOX_NMS_MAX" in lib.ffn_last_error()


def test_nms_sweep_is_the_greedy_definition():
    """ops.nms_sweep on a hand-made bit matrix of 70 rows (two words): a kept row's bits remove, a removed row's bits do not"""
    from freefine_amd import ops
    sup = np.zeros((70, 2), dtype=np.uint64)
    sup[0, 0] = np.uint64(1 << 1)                               # 0 removes 1
    sup[1, 0] = np.uint64(1 << 2)                               # 1 would remove 2, but is gone
    sup[2, 1] = np.uint64(1 << (69 - 64))                       # 2 is kept and removes 69
    sup[3, 0] = np.uint64(1 << 63)                              # the top bit of a word
    assert ops.nms_sweep(sup) == [i for i in range(70) if i not in (1, 63, 69)]


def rec(mask):
    return dict(segmentation=(np.asarray(mask) * 255).astype(np.uint8))


def test_mask_pool_from_records():
    from src.demo.utils import mask_pool_from_records
    from src.utils.vis_utils import get_constrain_areas
    obj = np.zeros((10, 20), dtype=np.uint8)
    obj[2:8, 2:8] = 255
    part = np.zeros_like(obj)
    part[3:5, 3:8] = 1                                          # wholly inside the object
    straddle = np.zeros_like(obj)
    straddle[4, 2:12] = 1                                       # 10 pixels, 6 of them inside: 60 %
    other = np.zeros_like(obj)
    other[1:9, 12:18] = 1
    whole = np.ones_like(obj)
    empty = np.zeros_like(obj)
    records = [rec(m) for m in (part, straddle, other, whole, empty)]
    assert int((straddle & (obj > 0)).sum()) == 6 and int(straddle.sum()) == 10

    def same(pool, want):
        return len(pool) == len(want) and all(a.dtype == np.uint8 and a.max() <= 1 and np.array_equal(a, b) for a, b in zip(pool, want))
    own = (obj > 0).astype(np.uint8)
    assert same(mask_pool_from_records(records, obj), [own, other, whole])                               # 60 % inside: dropped at 0.5
    assert same(mask_pool_from_records(records, obj, inside_fraction=0.7), [own, straddle, other, whole])        # kept at 0.7
    assert same(mask_pool_from_records(records, obj, max_area_fraction=0.5), [own, other])
    assert same(mask_pool_from_records([], obj), [own])
    for kw in (dict(), dict(inside_fraction=0.7), dict(max_area_fraction=0.5)):
        pool = mask_pool_from_records(records, obj, **kw)
        cons = get_constrain_areas(mask_list=pool, ori_mask=obj.copy())
        assert cons.dtype == np.uint8 and cons.max() <= 1 and not (cons == 255).any()
        assert not cons[obj > 0].any() and cons[other > 0].all()
    # without the object's own mask the uint8 subtraction wraps: what the first entry is there for
    assert (get_constrain_areas(mask_list=[other], ori_mask=obj.copy()) == 255).any()


def test_mask_pool_tool_arguments(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mask_pool
    base = ["--image", "a.png", "--weights", "synthetic:tiny", "--out-dir", "pool"]
    cli = mask_pool.parse(base)
    assert (cli.points_per_side, cli.pred_iou_thresh, cli.stability_thresh, cli.nms_thresh, cli.precision) == (32, 0.88, 0.95, 0.7, "f32") and cli.out_dir == "pool"
    cli = mask_pool.parse(base + ["--points-per-side", "4", "--pred-iou-thresh", "0.1", "--stability-thresh", "0.7", "--nms-thresh", "0.3", "--precision", "x3"])
    assert (cli.points_per_side, cli.pred_iou_thresh, cli.stability_thresh, cli.nms_thresh, cli.precision) == (4, 0.1, 0.7, 0.3, "x3")
    for bad in (base[2:], base[:4], base + ["--points-per-side", "0"], base + ["--precision", "fp8"]):
        with pytest.raises(SystemExit) as e:
            mask_pool.parse(bad)
        assert e.value.code == 2
    assert "--points-per-side" in capsys.readouterr().err
