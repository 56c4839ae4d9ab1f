"""Clicks -> `ori_mask`: the host side of the reference application's click-to-mask step (src/demo/utils.py:40-100 there) without its user interface -- no
gradio, no cv2.  The network is freefine_amd.sam.HipEfficientSam; the mask these functions return is what FreeFine_generation takes as `ori_mask`.
mask_pool_from_records turns HipEfficientSam.generate's records into the `mask_pool` of get_constrain_areas (this project's rule: the reference has none)."""
import numpy as np

LABEL_POINT, LABEL_TOP_LEFT, LABEL_BOTTOM_RIGHT = 1, 2, 3


def box_from_clicks(p1, p2):
    """two clicks (x, y) in any order -> ((left, top), (right, bottom)): the reference swaps coordinates in three of its four cases (second click right / left of
    and below / above the first), which comes to the smaller and the larger value per axis"""
    (x1, y1), (x2, y2) = p1, p2
    return (min(x1, x2), min(y1, y2)), (max(x1, x2), max(y1, y2))


def segment_with_box(model, image, p1, p2):
    """model: HipEfficientSam; image uint8 [H, W, 3]; p1, p2: the two clicks -> uint8 [H, W], 255 inside the best mask of the box they span"""
    tl, br = box_from_clicks(p1, p2)
    return model.segment(image, np.array([tl, br], dtype=np.float32), np.array([LABEL_TOP_LEFT, LABEL_BOTTOM_RIGHT]))


def mask_pool_from_records(records, ori_mask, inside_fraction=0.5, max_area_fraction=None):
    """records: HipEfficientSam.generate's (each with a `segmentation` uint8 [H, W], non-zero inside); ori_mask: the edited object's mask [H, W], non-zero
    inside -> a list of 0 / 1 uint8 masks [H, W] fit for get_constrain_areas(mask_list=..., ori_mask=...), whose result keeps the removal mask's dilation out
    of the other objects and feeds `cons_area` of reduce_inp_artifacts.

      * The object's own mask always comes first: get_constrain_areas subtracts ori_mask from the union in uint8, and a pixel of the object outside the
        union would wrap to 255.
      * A generated mask of which MORE than inside_fraction lies inside ori_mask is dropped: it is the object, or a part of it, and must not constrain the
        object's own dilation.  Empty masks are dropped.
      * max_area_fraction (None = off): masks larger than that fraction of the image are dropped too.  With the default every segment is kept, so a sky or
        ground segment that surrounds the object BLOCKS the dilation on that side; whether such segments count as objects is the caller's choice.

    Nothing in the reference defines this filter: its drivers read the pool from the benchmark's annotations (prepare_mask_pool) and its notebooks build it by
    hand as [ori_mask] ("add more object mask if you have").  The rule above is this project's."""
    obj = (np.asarray(ori_mask) > 0).astype(np.uint8)
    assert obj.ndim == 2, "ori_mask [H, W]"
    pool = [obj]
    for rec in records:
        m = np.asarray(rec["segmentation"]) > 0
        assert m.shape == obj.shape, "a record's segmentation has the image's size"
        area = int(m.sum())
        if area == 0 or int((m & (obj > 0)).sum()) > inside_fraction * area:
            continue
        if max_area_fraction is not None and area > max_area_fraction * m.size:
            continue
        pool.append(m.astype(np.uint8))
    return pool
