"""GPU: automatic mask generation (HipEfficientSam.generate) -- the statistics kernel against tests/maskgen_ref.py applied to the fp32 image that
ops.upsample_bicubic returns for the same source (integer for integer), box NMS against the restatement's greedy sweep (the kept list exactly), generate
against the restatement fed with the device's own decode_low output (record for record), decode_low against predict (bit for bit), the command line.
tests/test_maskgen_cpu.py pins the restatement to the reference's code.  Everything compared here is an integer, a byte or a bit pattern: no tolerances."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import maskgen_ref as MR
import sam_ref as SR
from test_maskgen_cpu import g19
from test_sam_cpu import g16
from test_sam_gpu import model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_CASES = {"a": (37, 300), "b": (70, 45)}     # 8 x 8 -> 37 x 300: wider than one 256-thread run with a ragged tail; 5 x 7 -> 70 x 45; odd heights, more rows than row blocks
_FULL = {}


def stats_case(name, gpu):
    """(source fp32 [7, h, w] on the device, offset, the fp32 image and byte mask of ops.upsample_bicubic), computed once: the fixture's six special maps and a
    seventh with rows of exact zeros above a block of +1 beside a block of -1, whose upsampled values fall exactly on 0 and on +-offset where all taps agree"""
    from freefine_amd import ops
    if name not in _FULL:
        G = g19()
        x = G["stack_" + name].copy()
        h, w = x.shape[1:]
        x[6] = 0.0
        x[6, 2:, :w // 2], x[6, 2:, w // 2:] = 1.0, -1.0
        src = torch.from_numpy(x).to(gpu)
        full, m8 = ops.upsample_bicubic(src, *STATS_CASES[name], mask=True)
        _FULL[name] = (src, float(G["offset"]), full.cpu().numpy(), m8.cpu().numpy())
    return _FULL[name]


@pytest.mark.parametrize("name", list(STATS_CASES))
def test_bicubic_stats_equal_the_restatement_on_the_stored_image(gpu, name):
    from freefine_amd import ops
    src, offset, full, m8 = stats_case(name, gpu)
    H, W = STATS_CASES[name]
    # the seventh map does put pixels exactly on the three thresholds, and beside them
    last = full[6]
    assert (last == 0).any() and (last == offset).any() and (last == -offset).any()
    assert ((last > offset) & (last < offset + 1e-5)).any() and ((last < -offset) & (last > -offset - 1e-5)).any()
    want = MR.stats(full, offset)
    got = ops.upsample_bicubic_stats(src, H, W, offset)
    assert got.shape == (7, 8) and got.dtype == torch.int32
    print(f"stats {name} {tuple(src.shape[1:])} -> {H}x{W}:\n{got.cpu().numpy()}")
    assert np.array_equal(got.cpu().numpy(), want)
    assert want[0].tolist() == [0] * 8 and want[1, 0] > 0.9 * H * W and want[1, 3:7].tolist() == [0, 0, W - 1, H - 1]      # empty and full maps
    assert 0 < want[2, 0] < H * W // 4 and want[3, 0] > 0 and want[5, 3:7].tolist() == [0, 0, W - 1, H - 1]
    st, mask = ops.upsample_bicubic_stats(src, H, W, offset, mask=True)
    assert torch.equal(st, got) and mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), m8)
    assert torch.equal(ops.upsample_bicubic_stats(src, H, W, offset), got)
    assert torch.equal(ops.upsample_bicubic_stats(src[2:3].contiguous(), H, W, offset), got[2:3])           # a map's row does not depend on its neighbours


@pytest.mark.parametrize("name", list(STATS_CASES))
def test_bicubic_stats_write_nothing_outside_their_outputs(gpu, name):
    """the entry on buffers with a canary before and after: one stats row (sentinel -7) and one image row of bytes (sentinel 77) on either side"""
    from freefine_amd import _lib
    lib = _lib.load()
    src, offset, full, m8 = stats_case(name, gpu)
    N, (h, w), (H, W) = src.shape[0], src.shape[1:], STATS_CASES[name]
    sbuf = torch.full((N + 2, 8), -7, dtype=torch.int32, device=gpu)
    mbuf = torch.full((N * H * W + 2 * W,), 77, dtype=torch.uint8, device=gpu)
    rc = lib.ffn_upsample_bicubic_stats(torch.cuda.current_stream().cuda_stream, src.data_ptr(), sbuf[1:].data_ptr(), mbuf[W:].data_ptr(), N, h, w, H, W, offset)
    assert rc == 0, lib.ffn_last_error()
    torch.cuda.synchronize()
    assert (sbuf[0] == -7).all() and (sbuf[-1] == -7).all() and (mbuf[:W] == 77).all() and (mbuf[-W:] == 77).all()
    assert np.array_equal(sbuf[1:-1].cpu().numpy(), MR.stats(full, offset)) and np.array_equal(mbuf[W:-W].view(N, H, W).cpu().numpy(), m8)


def nms_boxes(M, seed):
    """M boxes with integer corners in a 48-pixel square (overlaps are common), scores in steps of 0.05 (ties are common); from M = 64 on, placed far from them
    and from each other: a duplicate pair, two zero-area boxes at one spot, a pair whose IoU is exactly 0.5, a chain 0 -> 1 -> 2 in which 0 does not reach 2"""
    g = np.random.default_rng(seed)
    x1, y1 = g.integers(0, 40, M), g.integers(0, 40, M)
    boxes = np.stack([x1, y1, x1 + g.integers(3, 16, M), y1 + g.integers(3, 16, M)], axis=1).astype(np.float32)
    scores = (g.integers(0, 20, M) * 0.05).astype(np.float32)
    special = {}
    if M >= 64:
        rows = [[300, 0, 310, 10], [300, 0, 310, 10], [405, 5, 405, 5], [405, 5, 405, 5], [100, 100, 102, 102], [100, 100, 102, 101],
                [200, 0, 210, 10], [203, 0, 213, 10], [206, 0, 216, 10]]
        at = g.permutation(M)[:len(rows)]
        boxes[at] = np.array(rows, dtype=np.float32)
        scores[at] = np.array([0.5, 0.5, 0.3, 0.3, 0.7, 0.6, 0.99, 0.98, 0.97], dtype=np.float32)
        special = dict(zip(("dup0", "dup1", "zero0", "zero1", "half0", "half1", "chain0", "chain1", "chain2"), at.tolist()))
    return boxes, scores, special


@pytest.mark.parametrize("M", [1, 64, 65, 130])
def test_box_nms_keeps_what_the_greedy_definition_keeps(gpu, M):
    from freefine_amd import ops
    boxes, scores, sp = nms_boxes(M, 40 + M)
    want = MR.nms(boxes, scores, 0.5)
    got = ops.box_nms(torch.from_numpy(boxes).to(gpu), torch.from_numpy(scores).to(gpu), 0.5)
    assert got.dtype == torch.int64 and got.is_cuda
    print(f"box NMS M={M}: {len(want)} kept")
    assert got.tolist() == want
    assert len(want) < M or M == 1
    if sp:
        assert float(MR.iou_f32(boxes[sp["half0"]], boxes[sp["half1"]])) == 0.5
        kept = set(want)
        assert len(kept & {sp["dup0"], sp["dup1"]}) == 1 and min(sp["dup0"], sp["dup1"]) in kept          # tied scores: the caller's order decides
        assert {sp["zero0"], sp["zero1"], sp["half0"], sp["half1"], sp["chain0"], sp["chain2"]} <= kept and sp["chain1"] not in kept
    # at a threshold no IoU exceeds everything stays, in score order
    every = ops.box_nms(torch.from_numpy(boxes).to(gpu), torch.from_numpy(scores).to(gpu), 1.0)
    assert every.tolist() == np.argsort(-scores, kind="stable").tolist()


# ---------------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------------
GEN = dict(pred_iou_thresh=0.1, stability_score_thresh=0.7, stability_score_offset=0.05, box_nms_thresh=0.3)
LOGIT_SHIFT = 2.4
_NETS = {}


def shifted_net(gpu):
    """the tiny configuration on seeded weights (seed 0), with every mask logit lowered by LOGIT_SHIFT through the weights themselves: seeded random weights give
    masks that are noise over the whole image (every box is the image, NMS keeps one); lowered, a candidate keeps a few small islands, the boxes differ, and the
    stability and NMS filters have something to decide.  The shift: channel 0 of the last upscaling layer made the constant gelu(1), and channel 0 of every
    hypernetwork output made the constant -LOGIT_SHIFT / gelu(1) -- their product enters every logit."""
    from freefine_amd import sam
    if "net" not in _NETS:
        cfg = sam.sam_config("tiny")
        st = sam.synthetic_state(cfg, 0)
        one = float(F.gelu(torch.tensor(1.0)))
        u = "mask_decoder.final_output_upscaling_layers.1.0."
        st[u + "weight"][:, 0] = 0.0
        st[u + "bias"][0] = 1.0
        for i in range(cfg.num_masks + 1):
            q = f"mask_decoder.output_hypernetworks_mlps.{i}.fc."
            st[q + "weight"][0] = 0.0
            st[q + "bias"][0] = -LOGIT_SHIFT / one
        _NETS["net"] = sam.HipEfficientSam(cfg, st, device=gpu)
    return _NETS["net"]


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for a, b in zip(got, want):
        assert set(a) == set(b) == {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score"}
        assert a["segmentation"].dtype == np.uint8 and np.array_equal(a["segmentation"], b["segmentation"])
        assert {k: v for k, v in a.items() if k != "segmentation"} == {k: v for k, v in b.items() if k != "segmentation"}, (a["bbox"], b["bbox"])


@pytest.mark.parametrize("H,W", [(48, 64), (64, 48)])
def test_generate_equals_the_restatement_record_for_record(gpu, H, W, monkeypatch):
    from freefine_amd import ops
    net = shifted_net(gpu)
    img = SR.smooth_image(H, W, 500 + H)
    points = MR.build_point_grid(4) * np.array([[W, H]], dtype=np.float64)
    low, iou = net.decode_low(net.encode(img), points[None, :, None, :], np.ones((1, 16, 1), dtype=np.int64), (H, W))
    assert low.shape == (1, 16, 3, 32, 32) and iou.shape == (1, 16, 3)
    counts = {}
    upsample = lambda x: ops.upsample_bicubic(torch.from_numpy(x).to(gpu), H, W).cpu().numpy()
    want = MR.generate(low[0].cpu().numpy(), iou[0].cpu().numpy(), points, upsample, counts=counts, **GEN)
    print(f"generate {H}x{W}: {counts}; areas {[r['area'] for r in want]}")
    # the run decides something at every stage
    assert counts["iou"] >= 8 and 4 <= counts["stable"] < counts["iou"] and 2 <= counts["kept"] < counts["stable"]
    sizes = []
    real = ops.upsample_bicubic_stats
    monkeypatch.setattr(ops, "upsample_bicubic_stats", lambda x, *a, **k: (sizes.append(x.shape[0]), real(x, *a, **k))[1])
    got = net.generate(img, points_per_side=4, **GEN)
    same_records(got, want)
    assert all(r["segmentation"].shape == (H, W) and set(np.unique(r["segmentation"])) <= {0, 255} and r["area"] == int((r["segmentation"] > 0).sum()) for r in got)
    assert [r["predicted_iou"] for r in got] == sorted((r["predicted_iou"] for r in got), reverse=True)
    # the result does not depend on how the points are batched
    for batch in (3, 16):
        same_records(net.generate(img, points_per_side=4, points_per_batch=batch, **GEN), want)
    same_records(net.generate(img, point_grid=MR.build_point_grid(4), **GEN), want)
    # thresholds nothing passes: an empty list, and no launch over zero maps
    assert min(sizes) >= 1
    del sizes[:]
    nms_calls = []
    monkeypatch.setattr(ops, "box_nms", lambda *a, **k: nms_calls.append(a))
    assert net.generate(img, points_per_side=4, **dict(GEN, pred_iou_thresh=10.0)) == [] and sizes == []
    assert net.generate(img, points_per_side=4, **dict(GEN, stability_score_thresh=1.5)) == [] and sizes and min(sizes) >= 1 and nms_calls == []


def test_decode_low_is_predict_before_the_sort(gpu):
    G = g16()
    _, _, img, pts, lab = SR.g16_inputs("tiny_200x136_q2", int(G["seed_tiny"]))
    net = model("tiny", "f32", gpu)
    H, W = img.shape[1:3]
    emb = net.encode(img)
    _, iou_s, low_s, _, order = net.predict(emb, pts, lab, (H, W), details=True)
    low, iou = net.decode_low(emb, pts, lab, (H, W))
    assert low.shape == low_s.shape == (1, 2, 3, 32, 32) and iou.shape == (1, 2, 3) and low.is_contiguous()
    assert torch.equal(torch.take_along_dim(iou, order, dim=2), iou_s)
    assert torch.equal(torch.take_along_dim(low, order[..., None, None], dim=2), low_s)
    assert not torch.equal(order, torch.arange(3, device=order.device).expand_as(order))            # the sort did move something


def test_mask_pool_tool_writes_masks_and_records(gpu, tmp_path, capsys):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mask_pool
    src, out = tmp_path / "in.png", tmp_path / "pool"
    Image.fromarray(SR.smooth_image(40, 56, 7)).save(src)
    # seeded weights: masks of noise; the stability filter is switched off (threshold 0) so that some pass
    mask_pool.main(["--image", str(src), "--weights", "synthetic:tiny", "--out-dir", str(out), "--points-per-side", "4", "--pred-iou-thresh", "0.1",
                    "--stability-thresh", "0", "--nms-thresh", "0.7"])
    records = json.load(open(out / "records.json"))
    files = sorted(f for f in os.listdir(out) if f.endswith(".png"))
    assert len(records) >= 1 and files == [r["file"] for r in records] == [f"mask_{i:03d}.png" for i in range(len(records))]
    assert f"{len(records)} masks" in capsys.readouterr().out
    for r in records:
        m = np.asarray(Image.open(out / r["file"]))
        assert m.shape == (40, 56) and m.dtype == np.uint8 and int((m == 255).sum()) == r["area"] and "segmentation" not in r
        assert set(r) == {"file", "area", "bbox", "predicted_iou", "point_coords", "stability_score"}
