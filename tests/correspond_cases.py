"""The fp64 restatement of the correspondence outputs of the point-cloud warp (csrc/splat.h: splat_ids_kernel, splat_correspond_kernel), the cases and the
bounds, shared by tests/test_correspond_cpu.py (which holds the restatement itself to the caps, without a device) and tests/test_correspond_gpu.py.  numpy only.

ids.  ref_ids: pixel (row, col) has the fp64 NDC centre of test_splat_gpu.pix_ndc64; a point covers it iff z >= 0 and d2 < r2; the K covering points of smallest
(z, id) are listed in that order, -1 in the empty slots.  A pixel is AMBIGUOUS when
  * a candidate lies within test_splat_gpu.rim_band of the disc's rim (|d2 - r2| <= band: fp32 may decide the other way), or
  * two of the first K + 1 covering depths differ by less than fp32 rounding (0 < |dz| <= 2u |z|) -- the depths are fp32 inputs that every side compares
    exactly, so this only guards a side that would recompute them; depths that are EQUAL are not ambiguous: (depth, id) orders them, and that rule is what is
    under test (the depth-step case has whole columns of equal depths).

map.  map64: (x, y) = (W - 1 - u, H - 1 - v), u = ((x_ndc + o) W - o) / rng with rng = 2 max(1, W / H), o = rng / 2 (v likewise): the inverse of
PixToNonSquareNdc.  The kernel evaluates it in fp32: rng and o carry one rounding each when W / H is no binary fraction (relative u: 2u |u + 1/2| on the
quotient), t1 = x_ndc + o (u |t1|), t2 = t1 W (2u |t2| with t1's), t3 = t2 - o (u |t3|), u = t3 / rng (u |u|), x = (W - 1) - u (u |x|).  With |t2| / rng and
|t3| / rng <= |u| + 1 and |x| <= |u| + W:
    |x - x64| <= u (2 + 2 + 1 + 1) (|u| + 1) + u (|u| + W) <= 8 u max(W, |u| + 1)          map_bound; 3.1e-5 pixel at W = 64 inside the image
("a few fp32 roundings of a value of magnitude <= max(W, H)").

visible.  visible64: the point's nearest pixel (floor(y + 1/2), floor(x + 1/2)) lies inside the image and the point is among that pixel's ids.  A point is
AMBIGUOUS when x + 1/2 or y + 1/2 is within map_bound of an integer (fp32 may choose the neighbour) or its nearest pixel is an ambiguous pixel."""
import math

import numpy as np

import test_splat_gpu as S
import test_warp3d_gpu as T3

U = S.U
# (h, w, K, radius in pixels, transform): the five geometries of tests/test_warp3d_gpu.py, read off its parametrisation (not copied)
GEOMETRIES = list(T3.test_point_cloud_warp_matches_the_numpy_restatement.pytestmark[0].args[1])
assert len(GEOMETRIES) == 5 and [g[:3] for g in GEOMETRIES] == [(48, 48, 5), (64, 64, 5), (40, 72, 12), (72, 40, 30), (96, 96, 8)]
IDENT = [0, 0, 0, 0, 0, 0, 1, 1, 1]


def geometry(i):
    """-> img, depth, mask, f, radius (NDC), K, transform of geometry i, as tests/test_warp3d_gpu.py builds them"""
    h, w, K, r_px, tf = GEOMETRIES[i]
    img, depth, mask, f = T3._case(h, w, h + w + K)
    return img, depth, mask, f, r_px * 2.0 / min(h, w), K, tf


def step_case(h=63, w=65):
    """an object with a depth step -- the near half (the columns from the mask's middle rightwards) at 2, the far half at 3 -- to be rotated 40 degrees about y, so that
    the near part hides part of the far part.  Odd sides: on an even side the source row j = H / 2 is lifted to Y = 0 up to the rounding of (Y - c) + c, and a
    rotation about y leaves it there: its whole row of targets sits at y = H / 2 - 1/2 -+ 1e-8, exactly half-way between two pixels, and every one of its points
    is ambiguous (3 % of the object at 64 x 64, measured by tests/test_correspond_cpu.py before this case was chosen).
    -> img, depth, mask, f, radius (1.5 pixels: coarse_edit_3d's default), K, transform"""
    img, depth, mask, f = T3._case(h, w, 7)
    cols = np.nonzero(mask.any(0))[0]
    mid = (cols[0] + cols[-1] + 1) // 2
    depth = np.full((h, w), 3.0, np.float32)
    depth[:, mid:] = 2.0
    return img, depth, mask, f, 1.5 * 2.0 / min(h, w), 5, [0, 0, 0, 0, 40, 0, 1, 1, 1]


def oracle_proj(depth, mask, f, tf):
    """the projected points [n, 4] fp32 as the numpy oracle computes them (a stand-in, on a machine without a device, for the ones the library records)"""
    from oracle import warp3d as OW
    pts, keep = OW.lift(depth, mask, f, f)
    proj, *_ = OW.project(pts, tf)
    return np.concatenate([proj, np.zeros((len(proj), 1), np.float32)], 1), keep


def ref_ids(proj, W, H, radius, K, band):
    """-> ids [H, W, K] int64 (compositing order, -1 = empty), amb [H, W] bool"""
    p = np.asarray(proj, np.float64)
    r = float(np.float32(radius))
    r2 = r * r
    xf, yf = S.pix_ndc64(W, H), S.pix_ndc64(H, W)
    cand = np.nonzero(S.drawable(p))[0]
    cand = cand[np.lexsort((cand, p[cand, 2]))]
    ids = np.full((H, W, K), -1, np.int64)
    amb = np.zeros((H, W), bool)
    if len(cand) == 0:
        return ids, amb
    px, py, pz = p[cand, 0], p[cand, 1], p[cand, 2]
    for r0 in range(0, H, 8):
        rows = slice(r0, min(r0 + 8, H))
        d2 = (xf[None, :, None] - px) ** 2 + (yf[rows, None, None] - py) ** 2
        hit = d2 < r2
        amb[rows] = (np.abs(d2 - r2) <= band).any(-1)
        rank = np.cumsum(hit, -1)
        z_prev = None
        for k in range(K + 1):
            at = hit & (rank == k + 1)
            have = at.any(-1)
            j = np.argmax(at, -1)
            if k < K:
                ids[rows, :, k] = np.where(have, cand[j], -1)
            z_k = np.where(have, pz[j], np.inf)
            if z_prev is not None:
                with np.errstate(invalid="ignore"):
                    dz = z_k - z_prev
                    amb[rows] |= have & (dz > 0) & (dz <= 2 * U * np.abs(z_k))
            z_prev = z_k
    return ids, amb


def ndc_ranges(W, H):
    return 2.0 * max(1.0, W / H), 2.0 * max(1.0, H / W)


def map64(proj, W, H):
    """-> [n, 2] fp64 (x, y), NaN for the points the renderer does not draw"""
    p = np.asarray(proj, np.float64)
    rx, ry = ndc_ranges(W, H)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((p[:, 0] + rx / 2) * W - rx / 2) / rx
        v = ((p[:, 1] + ry / 2) * H - ry / 2) / ry
        out = np.stack([W - 1 - u, H - 1 - v], 1)
    out[~S.drawable(p)] = np.nan
    return out


def map_bound(xy64, W, H):
    """-> [n, 2]: the bound of |fp32 map - map64| per component (module docstring)"""
    u = np.stack([W - 1 - xy64[:, 0], H - 1 - xy64[:, 1]], 1)
    return 8 * U * np.maximum(np.array([W, H], np.float64), np.abs(u) + 1)


def map_f32(proj, W, H):
    """splat_correspond_kernel's arithmetic in numpy fp32 (no FMA contraction) -> [n, 2] fp32"""
    f = np.float32
    a = np.asarray(proj, np.float32)
    rx = f(W) / f(H) * f(2) if W > H else f(2)
    ry = f(H) / f(W) * f(2) if H > W else f(2)
    ox, oy = rx * f(0.5), ry * f(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((a[:, 0] + ox) * f(W) - ox) / rx
        v = ((a[:, 1] + oy) * f(H) - oy) / ry
        out = np.stack([f(W - 1) - u, f(H - 1) - v], 1).astype(np.float32)
    out[~S.drawable(a)] = np.nan
    return out


def nearest_pixel(xy):
    """(row, col, inside-the-image) of the nearest pixel, as the kernel takes it: floor(. + 1/2); points without a target are outside"""
    with np.errstate(invalid="ignore"):
        c, r = np.floor(xy[:, 0] + 0.5), np.floor(xy[:, 1] + 0.5)
    return r, c


def visible64(proj, ids, amb_pix, W, H):
    """-> visible [n] bool, ambiguous [n] bool"""
    xy = map64(proj, W, H)
    r, c = nearest_pixel(xy)
    with np.errstate(invalid="ignore"):
        inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    ri, ci = np.where(inside, r, 0).astype(np.int64), np.where(inside, c, 0).astype(np.int64)
    vis = inside & (ids[ri, ci] == np.arange(len(xy))[:, None]).any(-1)
    b = map_bound(np.nan_to_num(xy), W, H)
    with np.errstate(invalid="ignore"):
        frac = np.abs(xy + 0.5 - np.round(xy + 0.5))
        amb = np.isfinite(xy).all(1) & ((frac <= b).any(1) | (inside & amb_pix[ri, ci]))
    return vis, amb


def scatter(values, keep, H, W, fill):
    """per-point values [n, ...] -> an [H, W, ...] array with `fill` at the pixels `keep` (flat indices) does not name"""
    out = np.array(np.broadcast_to(fill, (H, W) + np.shape(values)[1:]), dtype=np.asarray(values).dtype)
    out.reshape((H * W,) + np.shape(values)[1:])[keep] = values
    return out


def identity_map(H, W):
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    return np.stack([xs, ys], -1)


def focal(h, w):
    return 0.5 * min(h, w) / math.tan(math.radians(30.0))
