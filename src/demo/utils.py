"""Clicks -> `ori_mask`: the host side of the reference application's click-to-mask step (src/demo/utils.py:40-100 there) without its user interface -- no
gradio, no cv2.  The network is freefine_amd.sam.HipEfficientSam; the mask these functions return is what FreeFine_generation takes as `ori_mask`."""
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
