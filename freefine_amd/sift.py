"""SIFT keypoints for the Mean Distance metric, on the device (csrc/sift.h; the C entry points are described in include/freefine_hip.h).

The reference takes MD's keypoints from cv2 (evaluation/metrics/MD/mean_distance.py:49-79 get_Matches): SIFT on the source and on the edited image, brute-force 2-NN
matching, Lowe's ratio test at 0.75, and of the surviving matches those whose source point lies in the object mask.  cv2 is not installed anywhere this project is
built, so this module is Lowe's SIFT with OpenCV's DEFAULT PARAMETERS (3 layers per octave, sigma 1.6, contrast threshold 0.04, edge threshold 10, first octave -1:
the image is upsampled 2x), restated and held stage by stage to an fp64 numpy restatement (tests/sift_ref.py).  PARITY WITH cv2's OWN OUTPUT IS UNMEASURED.  Known
differences from cv2's code: atan2f / expf instead of cv2's fastAtan2 and exp approximations, no nfeatures cap (cv2's default is none either).

Deviation from the reference: with no match, get_Matches falls back to ORB detections on the source image.  ORB is not restated; the fallback here is the source
image's own SIFT detections inside the mask, strongest response first.

Channel order: the reference hands PIL's RGB array to cv2, whose gray conversion weighs channel 0 as blue (0.114) and channel 2 as red (0.299).  Kept as it is.
"""
import ctypes as CT

import numpy as np
import torch

from . import _lib as L

SIGMA, NLAYERS = 1.6, 3
REC = 27            # SIFT_REFINE_FLOATS: keep, layer, row, col, x, y, size, response, npeaks, 18 angles
ENOSPC = -28        # FFN_ENOSPC


def gauss_taps(sigma):
    """fp32 taps of a Gaussian blur as OpenCV sizes it for float images: round(8 sigma + 1) | 1 taps, exp(-x^2 / 2 sigma^2) normalised (in fp64, then rounded)"""
    T = int(np.rint(8 * sigma + 1)) | 1
    x = np.arange(T) - T // 2
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return np.ascontiguousarray((k / k.sum()).astype(np.float32))


def sigmas():
    """[the base blur sqrt(1.6^2 - 1), then the incremental blurs sqrt((1.6 k^i)^2 - (1.6 k^(i - 1))^2), i = 1..5, k = 2^(1/3)]"""
    k = 2.0 ** (1.0 / NLAYERS)
    return [np.sqrt(max(SIGMA * SIGMA - 1.0, 0.01))] + [np.sqrt((SIGMA * k ** i) ** 2 - (SIGMA * k ** (i - 1)) ** 2) for i in range(1, NLAYERS + 3)]


def n_octaves(base_hw):
    return max(int(np.rint(np.log2(min(base_hw)) - 2)) + 1, 0)


def sort_keypoints(kp, desc=None):
    """OpenCV's keypoint order (x, y, size descending, angle, response descending, octave descending; then layer descending) with exact duplicates dropped: the
    order in which `kps[:max_points]` cuts, and what makes the result independent of the order in which the device compacted its candidates"""
    if len(kp) == 0:
        return (kp, desc) if desc is not None else kp
    order = np.lexsort((-kp[:, 6], -kp[:, 5], -kp[:, 4], kp[:, 3], -kp[:, 2], kp[:, 1], kp[:, 0]))
    kp = kp[order]
    keep = np.ones(len(kp), bool)
    keep[1:] = np.any(kp[1:, :4] != kp[:-1, :4], axis=1)
    return kp[keep] if desc is None else (kp[keep], desc[order][keep])


def records_to_keypoints(rec, octave):
    """[n, 27] records of ffn_sift_refine_orient (host array) -> float32 [m, 7] = (x, y, size, angle, response, octave - 1, layer), one row per orientation peak"""
    rec = rec[rec[:, 0] != 0]
    n = rec[:, 8].astype(np.int64)
    rows = np.repeat(np.arange(len(rec)), n)
    peak = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    out = np.empty((len(rows), 7), np.float32)
    out[:, 0:3] = rec[rows, 4:7]
    out[:, 3] = rec[rows, 9 + peak]
    out[:, 4] = rec[rows, 7]
    out[:, 5] = octave - 1
    out[:, 6] = rec[rows, 1]
    return out


class HipSift:
    """detect_and_compute(img_u8) -> (kp float32 [n, 7] = (x, y, size, angle, response, octave, layer), desc uint8 [n, 128]), host arrays in OpenCV's keypoint
    order.  x, y, size are in pixels of the image given; octave counts from -1 (the upsampled image) as cv2's does.  The stage methods below return device tensors
    so that each stage can be checked on the device's own upstream output.  Calling the object with (src_img, gen_img, mask) gives sift_matches' points: a
    HipSift is a `keypoints` callable for metrics.calculate_md."""

    def __init__(self, device=None, max_candidates=None):
        self.device = torch.device("cuda:0" if device is None else device)
        self.max_candidates = max_candidates            # per octave; None: a quarter of the octave's pixels, which the extrema of a 3x3x3 neighbourhood cannot exceed by much
        self.lib = L.load()

    # ---- stages --------------------------------------------------------------------------------------------------------------------------------------
    def base(self, img):
        img = np.ascontiguousarray(np.asarray(img))
        if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
            raise ValueError(f"HipSift: uint8 [H, W, 3] or [H, W] images; got dtype {img.dtype}, shape {img.shape}")
        H, W = img.shape[:2]
        d = torch.from_numpy(img).to(self.device)
        out = torch.empty(2 * H, 2 * W, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.ffn_sift_base(_stream(), d.data_ptr(), out.data_ptr(), H, W, 1 if img.ndim == 2 else 3), "ffn_sift_base")
        return out

    def blur(self, src, sigma=None, taps=None):
        """fp32 [H, W] device tensor -> its blur (a new tensor); taps: host float32 array, default gauss_taps(sigma)"""
        taps = gauss_taps(sigma) if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
        assert src.dtype == torch.float32 and src.ndim == 2 and src.is_contiguous()
        dst, tmp = torch.empty_like(src), torch.empty_like(src)
        with torch.cuda.device(self.device):
            L.check(self.lib.ffn_gauss_blur_f32(_stream(), src.data_ptr(), dst.data_ptr(), tmp.data_ptr(), src.shape[0], src.shape[1], taps.ctypes.data, len(taps)),
                    "ffn_gauss_blur_f32")
        return dst

    def pyramid(self, base):
        """base fp32 [2H, 2W] -> list over octaves of the 6 Gaussian images [6, h, w]; the next octave starts from every second pixel of layer 3"""
        inc = [gauss_taps(s) for s in sigmas()[1:]]
        first = self.blur(base, sigmas()[0])
        out = []
        for o in range(n_octaves(base.shape)):
            h, w = first.shape
            G = torch.empty(NLAYERS + 3, h, w, dtype=torch.float32, device=self.device)
            tmp = torch.empty(h, w, dtype=torch.float32, device=self.device)
            G[0].copy_(first)
            with torch.cuda.device(self.device):
                for i, t in enumerate(inc):
                    L.check(self.lib.ffn_gauss_blur_f32(_stream(), G[i].data_ptr(), G[i + 1].data_ptr(), tmp.data_ptr(), h, w, t.ctypes.data, len(t)), "ffn_gauss_blur_f32")
                out.append(G)
                if h < 2 or w < 2:
                    break
                first = torch.empty(h // 2, w // 2, dtype=torch.float32, device=self.device)
                L.check(self.lib.ffn_decimate2_f32(_stream(), G[NLAYERS].data_ptr(), first.data_ptr(), h, w), "ffn_decimate2_f32")
        return out

    def extrema(self, G, cap=None):
        """G [6, h, w] -> (D [5, h, w], cand int32 [n, 3] = (layer, row, col) in arrival order).  cap: the length of the list; a longer result raises
        FreeFineHipError (rc FFN_ENOSPC) -- never a silently short list"""
        _, h, w = G.shape
        if cap is None:
            cap = self.max_candidates or max(h * w // 4, 64)
        D = torch.empty(NLAYERS + 2, h, w, dtype=torch.float32, device=self.device)
        cand = torch.empty(cap, 3, dtype=torch.int32, device=self.device)
        counter = torch.empty(1, dtype=torch.int32, device=self.device)
        count = CT.c_int(0)
        with torch.cuda.device(self.device):
            L.check(self.lib.ffn_sift_extrema(_stream(), G.data_ptr(), D.data_ptr(), h, w, cand.data_ptr(), cap, counter.data_ptr(), CT.byref(count)), "ffn_sift_extrema")
        return D, cand[:count.value]

    def refine(self, D, G, octave, cand):
        """-> fp32 [n, 27] records (include/freefine_hip.h: ffn_sift_refine_orient)"""
        n = cand.shape[0]
        out = torch.zeros(n, REC, dtype=torch.float32, device=self.device)
        cand = cand.contiguous()
        with torch.cuda.device(self.device):
            L.check(self.lib.ffn_sift_refine_orient(_stream(), D.data_ptr(), G.data_ptr(), D.shape[1], D.shape[2], octave, cand.data_ptr(), n, out.data_ptr()),
                    "ffn_sift_refine_orient")
        return out

    def describe(self, G, octave, kp, want_raw=False):
        """kp: host float32 [n, 7] of this octave -> desc uint8 [n, 128] (and the fp32 values before the conversion), device tensors"""
        kp = np.ascontiguousarray(kp, dtype=np.float32).reshape(-1, 7)
        n = len(kp)
        desc = torch.zeros(n, 128, dtype=torch.uint8, device=self.device)
        raw = torch.zeros(n, 128, dtype=torch.float32, device=self.device) if want_raw else None
        if n:
            d = torch.from_numpy(kp).to(self.device)
            with torch.cuda.device(self.device):
                L.check(self.lib.ffn_sift_describe(_stream(), G.data_ptr(), G.shape[1], G.shape[2], octave, d.data_ptr(), n, desc.data_ptr(), 0 if raw is None else raw.data_ptr()),
                        "ffn_sift_describe")
        return (desc, raw) if want_raw else desc

    def knn2(self, des1, des2):
        """uint8 [n1, 128], [n2, 128] (host arrays or device tensors) -> (idx int32 [n1, 2], dist int32 [n1, 2]) device tensors: the two nearest rows of des2 by
        squared L2 distance, ties to the lower index; with fewer than two rows in des2 the missing ones are -1 at distance INT_MAX"""
        a, b = (torch.as_tensor(np.ascontiguousarray(d) if isinstance(d, np.ndarray) else d).to(self.device).contiguous().reshape(-1, 128) for d in (des1, des2))
        assert a.dtype == torch.uint8 and b.dtype == torch.uint8
        idx = torch.empty(a.shape[0], 2, dtype=torch.int32, device=self.device)
        dist = torch.empty(a.shape[0], 2, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.ffn_knn2_u8(_stream(), a.data_ptr() if a.numel() else 0, a.shape[0], b.data_ptr() if b.numel() else 0, b.shape[0], idx.data_ptr(), dist.data_ptr()),
                    "ffn_knn2_u8")
        return idx, dist

    # ---- the detector ------------------------------------------------------------------------------------------------------------------------------------
    def detect_and_compute(self, img):
        kps, descs = [], []
        for o, G in enumerate(self.pyramid(self.base(img))):
            D, cand = self.extrema(G)
            kp = records_to_keypoints(self.refine(D, G, o, cand).cpu().numpy(), o)
            kps.append(kp)
            descs.append(self.describe(G, o, kp).cpu().numpy())
        if not kps:
            return np.zeros((0, 7), np.float32), np.zeros((0, 128), np.uint8)
        return sort_keypoints(np.concatenate(kps), np.concatenate(descs))

    def match_ratio(self, des1, des2, ratio=0.75):
        """-> int array [m, 2] = (index into des1, index into des2) of the rows that pass Lowe's ratio test, in des1's order.  ratio 0.75 is tested in integers on
        the squared distances, 16 d1 < 9 d2, which is exactly sqrt(d1) < 0.75 sqrt(d2); another ratio in fp64"""
        if len(des1) == 0 or len(des2) < 2:
            return np.zeros((0, 2), np.int64)
        idx, dist = (t.cpu().numpy().astype(np.int64) for t in self.knn2(des1, des2))
        return ratio_pairs(idx, dist, ratio)

    def __call__(self, src_img, gen_img, mask):
        return sift_matches(src_img, gen_img, mask, self)


def ratio_pairs(idx, dist, ratio=0.75):
    idx, dist = np.asarray(idx, np.int64), np.asarray(dist, np.int64)
    if ratio == 0.75:
        ok = 16 * dist[:, 0] < 9 * dist[:, 1]
    else:
        ok = np.sqrt(dist[:, 0].astype(np.float64)) < ratio * np.sqrt(dist[:, 1].astype(np.float64))
    rows = np.nonzero(ok & (idx[:, 1] >= 0))[0]
    return np.stack([rows, idx[rows, 0]], 1)


def match_ratio(des1, des2, ratio=0.75, sift=None):
    """ratio-test matches of two descriptor sets on the device (HipSift.match_ratio)"""
    return (sift or HipSift()).match_ratio(des1, des2, ratio)


def sift_matches(im1, im2, mask, sift=None, return_fallback=False):
    """The counterpart of mean_distance.py:get_Matches.  im1, im2: uint8 images; mask: [H, W] array of im1's size, object where > 0.5.  im2 is resized to im1's
    size with PIL BILINEAR; SIFT on both; the ratio-test matches whose source point (x, y) has mask[int(y), int(x)] > 0.5 -> int array [[row, col], ...] =
    [[int(y), int(x)], ...] in keypoint order.  No such match: the source image's own detections inside the mask, strongest response first (the reference falls
    back to ORB there, which is not restated).  return_fallback: also say whether the fallback was taken."""
    from PIL import Image
    sift = sift or HipSift()
    im1 = np.asarray(im1)
    im2 = np.asarray(im2)
    if im2.shape[:2] != im1.shape[:2]:
        im2 = np.array(Image.fromarray(im2).resize((im1.shape[1], im1.shape[0]), Image.BILINEAR))
    mask = np.asarray(mask)
    kp1, d1 = sift.detect_and_compute(im1)
    kp2, d2 = sift.detect_and_compute(im2)
    rc = np.stack([kp1[:, 1].astype(np.int64), kp1[:, 0].astype(np.int64)], 1) if len(kp1) else np.zeros((0, 2), np.int64)
    rc = np.minimum(rc, np.array(mask.shape[:2]) - 1)            # a keypoint within rounding of the far edge
    inside = mask[rc[:, 0], rc[:, 1]] > 0.5 if len(rc) else np.zeros(0, bool)
    pairs = sift.match_ratio(d1, d2)
    rows = pairs[:, 0][inside[pairs[:, 0]]] if len(pairs) else pairs[:, 0]
    fell_back = len(rows) == 0
    if fell_back:
        order = np.argsort(-kp1[:, 4], kind="stable") if len(kp1) else np.zeros(0, np.int64)
        rows = order[inside[order]]
    pts = rc[rows].reshape(-1, 2)
    return (pts, fell_back) if return_fallback else pts


def _stream():
    return torch.cuda.current_stream().cuda_stream
