"""The project's numpy restatement of automatic mask generation, the yardstick of tests/test_maskgen_cpu.py and tests/test_maskgen_gpu.py.

Pinned to the reference's code by tests/golden/g19_amg.npz (tools/gen_golden_amg.py runs segment_anything/utils/amg.py itself): build_point_grid,
calculate_stability_score, batched_mask_to_box, box_xyxy_to_xywh.  Restated from its definition, because torchvision is not installed: greedy box NMS
(torchvision.ops.nms: boxes by descending score, a box goes when a kept one overlaps it with IoU > thresh; areas without "+ 1"), here in fp32 operation by
operation.  generate assembles them in the order of SamAutomaticMaskGenerator._process_batch / _process_crop for a single crop."""
import numpy as np


def build_point_grid(n):
    offset = 1 / (2 * n)
    side = np.linspace(offset, 1 - offset, n)
    return np.stack([np.tile(side[None, :], (n, 1)), np.tile(side[:, None], (1, n))], axis=-1).reshape(-1, 2)


def stability_counts(logits, offset, threshold=0.0):
    """fp32 [N, H, W] -> (n_hi, n_lo) int64 [N]: the strict comparisons of calculate_stability_score, the thresholds rounded to fp32 as torch rounds a scalar"""
    x = np.asarray(logits, dtype=np.float32)
    hi, lo = np.float32(threshold + offset), np.float32(threshold - offset)
    return (x > hi).sum((-2, -1)).astype(np.int64), (x > lo).sum((-2, -1)).astype(np.int64)


def stability_score(logits, offset, threshold=0.0):
    """calculate_stability_score: int32 / int32 in torch is the fp32 quotient of the two counts; 0 / 0 is NaN"""
    n_hi, n_lo = stability_counts(logits, offset, threshold)
    with np.errstate(divide="ignore", invalid="ignore"):
        return n_hi.astype(np.float32) / n_lo.astype(np.float32)


def mask_to_box(masks):
    """batched_mask_to_box: bool [N, H, W] -> int64 [N, 4] (x_min, y_min, x_max, y_max), maxima inclusive, an empty mask 0 0 0 0"""
    m = np.asarray(masks, dtype=bool)
    out = np.zeros((m.shape[0], 4), dtype=np.int64)
    for n in range(m.shape[0]):
        ys, xs = np.flatnonzero(m[n].any(1)), np.flatnonzero(m[n].any(0))
        if len(ys):
            out[n] = xs[0], ys[0], xs[-1], ys[-1]
    return out


def box_xyxy_to_xywh(box):
    out = np.array(box, copy=True)
    out[2], out[3] = out[2] - out[0], out[3] - out[1]
    return out


def stats(logits, offset):
    """what ffn_upsample_bicubic_stats answers for the fp32 image it did not store: int32 [N, 8] = area (>= 0), n_hi, n_lo, the box of >= 0, 0"""
    x = np.asarray(logits, dtype=np.float32)
    n_hi, n_lo = stability_counts(x, offset)
    on = x >= 0
    return np.concatenate([on.sum((-2, -1))[:, None], n_hi[:, None], n_lo[:, None], mask_to_box(on), np.zeros((len(x), 1), dtype=np.int64)], axis=1).astype(np.int32)


def iou_f32(a, b):
    """torchvision's box IoU of two XYXY boxes, every operation in fp32"""
    f = np.float32
    a, b = [f(v) for v in a], [f(v) for v in b]
    area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    iw, ih = max(min(a[2], b[2]) - max(a[0], b[0]), f(0)), max(min(a[3], b[3]) - max(a[1], b[1]), f(0))
    inter = iw * ih
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / ((area_a + area_b) - inter)


def nms(boxes, scores, thresh):
    """greedy NMS -> the kept indices into the caller's order, best first; ties keep the caller's order (a stable sort)"""
    boxes = np.asarray(boxes, dtype=np.float32)
    order = np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")
    keep = []
    for i in order:
        if not any(iou_f32(boxes[k], boxes[i]) > np.float32(thresh) for k in keep):
            keep.append(int(i))
    return keep


def generate(low, iou, points, upsample, pred_iou_thresh, stability_score_thresh, stability_score_offset, box_nms_thresh, counts=None):
    """low fp32 [n, 3, h, w], iou fp32 [n, 3] (the network's outputs for the n points, in its order), points float64 [n, 2]; upsample: fp32 [k, h, w] -> the fp32
    image [k, H, W] the masks are cut from -> records as HipEfficientSam.generate returns them.  Every candidate is upsampled here: the filters only select.
    counts (a dict) receives how many candidates each stage passed."""
    low, iou = np.asarray(low, dtype=np.float32), np.asarray(iou, dtype=np.float32).reshape(-1)
    n, nm = low.shape[:2]
    full = np.asarray(upsample(low.reshape(n * nm, *low.shape[2:])), dtype=np.float32)
    cand = np.repeat(np.asarray(points, dtype=np.float64), nm, axis=0)
    keep = np.flatnonzero(iou > np.float32(pred_iou_thresh)) if pred_iou_thresh > 0.0 else np.arange(n * nm)
    stab = stability_score(full[keep], stability_score_offset)
    stable = keep[stab >= np.float32(stability_score_thresh)] if stability_score_thresh > 0.0 else keep
    stab = stab[np.isin(keep, stable)]
    on = full[stable] >= 0
    boxes = mask_to_box(on)
    kept = nms(boxes, iou[stable], box_nms_thresh) if len(stable) else []
    if counts is not None:
        counts.update(candidates=n * nm, iou=len(keep), stable=len(stable), kept=len(kept))
    return [dict(segmentation=(on[k] * 255).astype(np.uint8), area=int(on[k].sum()), bbox=box_xyxy_to_xywh(boxes[k]).tolist(), predicted_iou=float(iou[stable[k]]),
                 point_coords=[cand[stable[k]].tolist()], stability_score=float(stab[k])) for k in kept]
