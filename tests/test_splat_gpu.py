"""The point-cloud splat (csrc/splat.h: lift, project, bin count, bin fill, render) stage by stage against fp64, through the C ABI.

Reference.  ref_render below: numpy, fp64, vectorised over pixels x candidate points in chunks of eight rows.  It takes the projected points exactly as the
kernel gets them (fp32 values, widened), so the only thing it does differently is the arithmetic: pixel (row, col) has the NDC centre of pytorch3d's
PixToNonSquareNdc at u = W - 1 - col, v = H - 1 - row; a point covers it iff z >= 0 and d2 < r2 (r2 = the square of the fp32 radius); the K covering points
of smallest (z, id) are composited front to back with w = 1 - d2 / r2; idx_sum adds the ids and -1 per empty slot.

Inputs on which fp32 is exact (the "grid" cases).  W, H powers of two with max / min in {1, 2, 4}, g = 4 max(W, H), point coordinates integer multiples of
1 / g, radius = (2k + 1) / (2g).  Pixel centres are odd multiples of 1 / min(W, H), every intermediate of splat_pix_to_ndc is a small dyadic number, dx, dy
are multiples of 1 / g below 2^11 / g, so dx^2 + dy^2 < 2^24 / g^2 is exact with or without FMA contraction, and so is r2.  d2 is an even multiple of
1 / (4 g^2) and r2 an odd one: d2 == r2 cannot happen.  The covering set of every pixel is therefore the same in fp32 and in fp64 and the tests hold
covered and idx_sum to equality on every pixel (tests/test_splat_ref_cpu.py checks the exactness claim on every grid case).  The render cases feed hand-built
tile lists (the reference's true covering tiles plus superfluous entries, shuffled; validate_lists is called before every launch).

Bound of the float image, grid inputs, u = 2^-24, colours <= 255.  t = d2 / r2 carries one rounding (|dt| <= u); w = 1 - t is exact for t >= 1/2 and rounds
by u / 2 otherwise: |dw| <= 1.5 u.  1 - w adds u / 2: |d(1 - w)| <= 2u.  cum_k, a product of k such factors, all <= 1, with one rounding each:
|dcum_k| <= 3u k.  The term (cum w) f has two roundings: error <= 255 (3u k + 1.5 u + 2u); every one of the K additions rounds a partial sum <= 255 (the
weights cum_k w_k add up to 1 - prod(1 - w) <= 1).  Summed over k < K:
    |image - ref| <= 255 u (1.5 K^2 + 3 K + 1)              (the + 1 covers the second-order terms, < 3 u K of the whole)     0.0248 at K = 32
Random inputs (W, H not powers of two).  With A = max(1, S1 / S2) >= |centre|, splat_pix_to_ndc rounds five times: range = 2A (1 + d1), then
range i (d2), + offset (d3), / S1 (d4), - offset (d5); d1 is common to every term and contributes |centre| u, the others 2A u, (2A + A / S1) u twice, and
A u: |d centre| <= 9 A u for S1 >= 8.  Along the shorter or equal side (S1 <= S2) range = 2 and 2 i + 1 are exact, which leaves d4 and d5:
|d centre| <= 3 u.  dx = centre - px rounds once more, u |dx| <= 1.01 u r near the rim: e_x = (3 or 9 A_x) u + 1.01 u r, e_y likewise,
e = hypot(e_x, e_y).  d2 = dx^2 + dy^2 then errs by <= 2 (|dx| e_x + |dy| e_y) + e^2 <= 2 r e + e^2 (Cauchy-Schwarz, at d2 ~ r2) plus two roundings of
d2 itself, and r2 = r r by one:
    band = 1.01 (2 r e + e^2 + 3 u r2)
A pixel is AMBIGUOUS when a candidate (z >= 0) has |d2 - r2| <= band in fp64; such pixels are left out (at most 1 % per case -- asserted, on the reference
alone, here and in tests/test_splat_ref_cpu.py) and every other pixel is held as on the grid, with w now off by 1.5 u + b, b = band / r2:
    |image - ref| <= 255 (u (1.5 K^2 + 3 K + 1) + b K (K + 1) / 2)

ffn_splat_bin is held to properties (check_bin): segments full, ids valid and distinct per tile, the fill pass reproduces the counts, every (point, tile)
pair whose fp64 disc strictly covers a pixel centre of the tile is listed, and no listed tile lies outside the fp64 bounding box of the disc grown by two
pixels.  Lift: three roundings, |err| <= 4u |ref| per component.  Project (project_bound): q = P - c + t rounds twice, u |P - c| + u |q| -- small where the
subtraction cancels, so what is left of the cancellation is the error the operand P brings (none here: the test feeds fp32 points to both sides); the dot
product with a column of R rounds three products and two sums, 3u sum |q_j| |R_jk|; the scale and + c round once each; the bound is stated with
M = max |P|, |c|, |t| in place of |q| (|q| <= 3M), doubled for slack, and carried through the division by z_view.

Found by this module: splat_render_kernel drew whatever its list named -- a point with z < 0 listed for a tile was composited FIRST (smallest depth); only
splat_tile_box kept such points out, so the product path was right and the kernel alone was not.  With that kernel all five cases of
test_render_rejected_and_border_points failed on a device (30 or 31 pixels of wrong idx_sum each; test_bin_on_the_grid_cases, where the bin builds the
lists, passed).  The kernel now turns a point with z < 0 or NaN into one no pixel can reach while it stages the chunk.

Measured on an MI355X, worst |err| / bound over the cases of a group (asserted <= 1):
  k-boundaries   K = 1: 0.210   8: 0.024   9: 0.022   16: 0.009   17: 0.009   32: 0.003
  depth ties     0.022 (K = 8), 0.008 (K = 17)      list order 0.019      chunk boundary 0.023      empty tiles 0.006
  partial tiles / rejected / borders 0.043, the same through the bin 0.043      second grid pass 0.027
  random sizes through the bin 0.012 (40x72), 0.003 (21x37), 0.002 (72x40)      lift 0.390      project 0.021
The image bound is a worst case over K^2 roundings that all push the same way and the project bound is stated with max |P| for |q|, hence the small
figures; tests/test_splat_ref_cpu.py shows that each planted error still leaves them by far.  Ambiguous pixels: 0 of 2880, 0 of 777, 0 of 2880 on the
random cases; through the Python entry 0 of 777 (21x37) and 1 of 2880 (40x72); tests/test_warp3d_gpu.py 0 of 2304, 1 of 4096, 0 of 2880, 0 of 2880,
2 of 9216.  Wall time of the module: 4 s for its 52 tests (1.6 s of it the first test's library load), the slowest test 0.4 s.

Three one-token edits of splat.h and what this suite would do (read off the code, never run on a device):
  * `ci < qi[k]` -> `ci > qi[k]` (tie rule): nothing changes where depths differ; test_render_depth_ties fails in idx_sum and image on every pixel with
    more than K tied candidates (the larger ids survive), and in image alone on pixels with 2 .. K tied hits (same set, reversed compositing order).
    test_render_is_independent_of_list_order still passes: the reversed rule is just as deterministic.
  * `if (k < K)` -> `if (k <= K)` in the composite loop: for K in {8, 16, 32} k stops at KMAX = K and nothing changes; for K in {1, 9, 17} slot K is never
    filled by the insertion chain (it still runs to k < K) so it holds the initial id 0x7fffffff: every pixel's idx_sum drops by 1 and
    test_render_k_boundaries fails on all of them.  With the same edit in the insertion chain as well, K + 1 points are kept: pixels with more than K
    candidates gain a term, which test_splat_ref_cpu.py shows is beyond the bound, and idx_sum changes.
  * the `- 1` / `+ 1` margins of splat_tile_box removed: floorf / ceilf of the EXACT edges u, v still enclose every covered pixel centre, so the margins
    only pay for the rounding of u and v (about 1e-5 pixel).  On the grid cases u and v are exact and nothing changes; on the random cases a rim that
    close to a centre is a matter of luck.  test_bin_keeps_the_tile_a_rim_just_reaches plants it: rims a few ulps past a centre in the first pixel
    column / row of the next tile.  tests/test_splat_ref_cpu.py shows that the fp32 box without margins loses some of those tiles and fails the superset
    property there, and passes every other bin case.
"""
import ctypes as C
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
AMBIGUOUS_CAP = 0.01
K_EDGES = (1, 8, 9, 16, 17, 32)
CHUNK_LENGTHS = (255, 256, 257, 512, 513)
# name -> (W, H, k, points, seed): radius = (2k + 1) / (2g) is about 1.6 pixels
PARTIAL = {"8x8": (8, 8, 12, 300, 11), "8x32": (8, 32, 51, 500, 12), "32x8": (32, 8, 51, 500, 13), "32x64": (32, 64, 25, 1500, 14), "64x32": (64, 32, 25, 1500, 15)}
# name -> (W, H, radius in pixels, K, points, seed)
RANDOM = {"40x72": (40, 72, 3.0, 5, 800, 21), "21x37": (21, 37, 2.5, 8, 400, 22), "72x40": (72, 40, 2.0, 12, 2500, 23)}
BIN_SIZES = [(8, 8), (21, 37), (37, 21), (40, 72), (72, 40), (8, 72), (72, 8)]
WRAP_N = 4096 * 256 + 300
SENT_F, SENT_I, SENT_B = -7.0, 0x5A5A5A5, 0xAB


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference and the bounds (numpy only; shared with tests/test_splat_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def pix_ndc64(S1, S2):
    """fp64 NDC centres of pixels 0 .. S1 - 1 in image order (pixel i sits at u = S1 - 1 - i: +X left, +Y up)"""
    rng = 2.0 * max(1.0, S1 / S2)
    u = S1 - 1.0 - np.arange(S1)
    return -rng / 2 + (rng * u + rng / 2) / S1


def tiles_of(W, H):
    return (W + 15) // 16, (H + 15) // 16


def ref_render(proj, rgb, W, H, radius, K, band=0.0, tie_rev=False, back_to_front=False, draw_behind=False):
    """-> image [H, W, 3] f64, idx_sum [H, W] i64, covered [H, W] u8, count [H, W] (covering points), first [H, W] (id of the nearest, -1 = none),
    amb [H, W] bool, cover [tiles, n] bool (the fp64 disc of point p strictly covers a pixel centre of the tile).  tie_rev, back_to_front and draw_behind
    are the planted errors of the CPU module."""
    proj = np.asarray(proj, np.float64)
    rgb = np.asarray(rgb, np.float64)
    n = len(proj)
    r = float(np.float32(radius))
    r2 = r * r
    xf, yf = pix_ndc64(W, H), pix_ndc64(H, W)
    x, y, z = proj[:, 0], proj[:, 1], proj[:, 2]
    reach = math.sqrt(r2 + band) * 1.001
    with np.errstate(invalid="ignore"):
        ok = np.ones(n, bool) if draw_behind else (z >= 0)
        ok &= (x > xf.min() - reach) & (x < xf.max() + reach) & (y > yf.min() - reach) & (y < yf.max() + reach)      # NaN and inf fail these
    ids = np.nonzero(ok)[0]
    ids = ids[np.lexsort((-ids if tie_rev else ids, z[ids]))]                 # by (z, id); -0.0 == +0.0 as in the kernel
    m = len(ids)
    TW, TH = tiles_of(W, H)
    out = NS(image=np.zeros((H, W, 3)), idx_sum=np.full((H, W), -K, np.int64), covered=np.zeros((H, W), np.uint8), count=np.zeros((H, W), np.int64),
             first=np.full((H, W), -1, np.int64), amb=np.zeros((H, W), bool), cover=np.zeros((TW * TH, n), bool))
    if m == 0:
        return out
    px, py, col = x[ids], y[ids], rgb[ids]
    for r0 in range(0, H, 8):
        rows = slice(r0, min(r0 + 8, H))
        d2 = (xf[None, :, None] - px) ** 2 + (yf[rows, None, None] - py) ** 2                 # [rows, W, m]
        hit = d2 < r2
        out.amb[rows] = (np.abs(d2 - r2) <= band).any(-1)
        rank = np.cumsum(hit, -1)
        sel = hit & (rank <= K)
        cnt = rank[..., -1]
        w = np.where(sel, 1.0 - d2 / r2, 0.0)
        if back_to_front:
            w = w[..., ::-1]
        cum = np.concatenate([np.ones_like(w[..., :1]), np.cumprod(1.0 - w, -1)[..., :-1]], -1)
        out.image[rows] = (cum * w) @ (col[::-1] if back_to_front else col)
        out.idx_sum[rows] = (sel * ids).sum(-1) - (K - np.minimum(cnt, K))
        out.covered[rows] = cnt > 0
        out.count[rows] = cnt
        out.first[rows] = np.where(cnt > 0, ids[np.argmax(hit, -1)], -1)
        ty = r0 // 16
        for tx in range(TW):
            out.cover[ty * TW + tx, ids] |= hit[:, 16 * tx:16 * tx + 16].any((0, 1))
    return out


def image_bound(K, b=0.0):
    return 255.0 * (U * (1.5 * K * K + 3 * K + 1) + b * K * (K + 1) / 2)


def rim_band(W, H, radius):
    r = float(np.float32(radius))
    centre = lambda S1, S2: 3 * U if S1 <= S2 else 9 * U * S1 / S2       # noqa: E731
    ex, ey = centre(W, H) + 1.01 * U * r, centre(H, W) + 1.01 * U * r
    e = math.hypot(ex, ey)
    return 1.01 * (2 * r * e + e * e + 3 * U * r * r)


def mismatch(out, ref, K, b=0.0):
    """out = (image, idx_sum, covered) -> (pixels of wrong coverage, pixels of wrong idx_sum, worst |image err| / bound), ambiguous pixels left out"""
    image, idx_sum, covered = out
    keep = ~ref.amb
    err = np.abs(np.asarray(image, np.float64) - ref.image).max(-1)
    return (int((np.asarray(covered)[keep] != ref.covered[keep]).sum()), int((np.asarray(idx_sum).astype(np.int64)[keep] != ref.idx_sum[keep]).sum()),
            float(np.where(keep, err, 0.0).max() / image_bound(K, b)))


def passes(out, ref, K, b=0.0):
    cov, ids, ratio = mismatch(out, ref, K, b)
    return cov == 0 and ids == 0 and ratio <= 1.0 and ref.amb.mean() <= AMBIGUOUS_CAP


def hold(out, ref, K, b=0.0, what=""):
    cov, ids, ratio = mismatch(out, ref, K, b)
    print(f"SPLAT {what}: K = {K}  |err| / bound = {ratio:.3f}  ambiguous {int(ref.amb.sum())} of {ref.amb.size}")
    assert ref.amb.mean() <= AMBIGUOUS_CAP, (what, ref.amb.mean())
    assert cov == 0 and ids == 0, (what, cov, ids)
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# tile lists
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def validate_lists(offs, lst, n, tiles):
    offs, lst = np.asarray(offs), np.asarray(lst)
    assert offs.dtype == np.int32 and lst.dtype == np.int32 and offs.shape == (tiles + 1,)
    assert offs[0] == 0 and (np.diff(offs) >= 0).all() and offs[-1] <= len(lst)
    assert ((lst[:offs[-1]] >= 0) & (lst[:offs[-1]] < n)).all()


def build_lists(cover, always, extra_share, seed):
    """per tile: the covering points, every id of `always`, and a random share of the rest (a conservative bin may over-include), shuffled"""
    rng = np.random.default_rng(seed)
    tiles, n = cover.shape
    segs = []
    for t in range(tiles):
        take = cover[t] | (rng.random(n) < extra_share)
        take[always] = True
        segs.append(rng.permutation(np.nonzero(take)[0]))
    return pack_lists(segs)


def pack_lists(segs):
    offs = np.zeros(len(segs) + 1, np.int32)
    offs[1:] = np.cumsum([len(s) for s in segs])
    lst = np.concatenate(segs).astype(np.int32) if offs[-1] else np.zeros(0, np.int32)
    return offs, np.concatenate([lst, np.zeros(1, np.int32)])               # never an empty allocation


def segments(offs, lst):
    return [lst[offs[t]:offs[t + 1]] for t in range(len(offs) - 1)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# cases (read-only: they are cached and shared)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def rejected_points(W, H):
    """[m, 4] fp32: points no stage may draw.  z < 0 on pixel centres (drawn, they would win with weight 1); z = +-0.0 with the coordinates the project
    kernel's v * inv_tan / z gives; coordinates beyond 1e30"""
    xf, yf = pix_ndc64(W, H).astype(np.float32), pix_ndc64(H, W).astype(np.float32)
    inv_tan = np.float32(1.0 / math.tan(math.radians(30.0)))
    pts = [(xf[1], yf[1], -1.0), (xf[W // 2], yf[H // 2], -1e-30), (xf[W - 2], yf[H - 2], -np.inf), (xf[0], yf[H - 1], -2.5)]
    with np.errstate(divide="ignore", invalid="ignore"):
        for v0, v1 in [(0.3, -0.2), (0.0, 0.0), (-1.5, 0.0), (0.0, 0.25)]:
            for z0 in (np.float32(0.0), np.float32(-0.0)):
                pts.append((np.float32(v0) * inv_tan / z0, np.float32(v1) * inv_tan / z0, z0))
    pts += [(2e30, 0.0, 1.0), (0.0, -3e30, 1.0), (1e38, 1e38, 2.0), (-1e31, yf[1], 1.5), (xf[1], 1e31, 1.5)]
    out = np.zeros((len(pts), 4), np.float32)
    out[:, :3] = np.array(pts, np.float32)
    return out


@functools.lru_cache(maxsize=None)
def grid_case(W, H, k, n, seed, ramp=False, z="random", window=None, ring=None):
    """points on the 1 / g grid, spread over the image and a margin of k + 1 units around it (discs over every border, and discs that stay outside), the
    eight explicit border points (one unit outside each edge's middle and each corner) and the rejected points; ids shuffled.  ring = (col, row): 44 more
    points on the rim of that pixel's disc (0.9 r2 <= d2 < r2, weights below 0.1) and nearer than every other point: the one pixel on which the 33rd of
    more than 32 covering points is still visible in the image (elsewhere the product of 32 factors 1 - w has long vanished)"""
    rng = np.random.default_rng(seed)
    g = 4 * max(W, H)
    ax, ay = max(1, W // H) * g, max(1, H // W) * g                        # the image's half extents in grid units
    lo = np.array([-ax - k - 1, -ay - k - 1])
    hi = np.array([ax + k + 1, ay + k + 1])
    if window is not None:                                                  # fractions of the image (x0, x1, y0, y1), no margin
        lo = np.array([-ax + 2 * ax * window[0], -ay + 2 * ay * window[2]])
        hi = np.array([-ax + 2 * ax * window[1], -ay + 2 * ay * window[3]])
    f = rng.random((n, 2))
    if ramp:
        f[:, 0] = np.sqrt(f[:, 0])                                          # density rising linearly from 0 along x
    ij = np.floor(lo + (hi - lo + 1) * f).astype(np.int64)
    border = np.array([(sx * (ax + 1) * (sx != 0), sy * (ay + 1) * (sy != 0)) for sx in (-1, 0, 1) for sy in (-1, 0, 1) if sx or sy], np.int64)
    if ring is not None:
        cx, cy = np.round(pix_ndc64(W, H)[ring[0]] * g), np.round(pix_ndc64(H, W)[ring[1]] * g)
        rim = [(a, b) for a in range(-k, k + 1) for b in range(-k, k + 1) if 0.9 * (k + 0.5) ** 2 <= a * a + b * b < (k + 0.5) ** 2]
        ij = np.concatenate([ij, np.array(rim, np.int64) + np.array([cx, cy], np.int64)])
        n_ring = len(rim)
    if window is None:
        ij = np.concatenate([ij, border])
    pts = np.zeros((len(ij), 4), np.float32)
    pts[:, :2] = ij / float(g)
    pts[:, 2] = {"random": rng.uniform(1.0, 3.0, len(ij)), "equal": np.full(len(ij), 1.5), "two": rng.choice([1.5, 2.5], len(ij))}[z]
    if ring is not None and z == "random":
        pts[n:n + n_ring, 2] = rng.uniform(0.5, 0.9, n_ring)
    rej = rejected_points(W, H)
    proj = np.concatenate([pts, rej])
    kind = np.concatenate([np.zeros(len(ij) - (len(border) if window is None else 0), np.int8), np.ones(len(border) if window is None else 0, np.int8),
                           np.full(len(rej), 2, np.int8)])
    perm = rng.permutation(len(proj))
    proj, kind = proj[perm], kind[perm]
    rgb = rng.integers(0, 256, (len(proj), 3)).astype(np.float32)
    rgb[kind == 2] = 255.0
    return NS(W=W, H=H, g=g, k=k, radius=np.float32((2 * k + 1) / (2.0 * g)), proj=proj, rgb=rgb, n=len(proj), rejected=np.nonzero(kind == 2)[0],
              border=np.nonzero(kind == 1)[0], band=0.0, b=0.0)


def kb_case(z="random"):
    """32 x 32 (four tiles), density ramp: pixels with 0 .. more than 33 covering points"""
    return grid_case(32, 32, 10, 5200, 3, ramp=True, z=z, ring=(29, 16))


@functools.lru_cache(maxsize=None)
def chunk_case(L):
    """16 x 16, one tile, L points, all listed.  Point S (the smallest z of all) sits alone on the left; the last chunk of the list holds S and the
    next-nearest points, so that some lanes meet their first hit -- and some their nearest -- only there"""
    rng = np.random.default_rng(100 + L)
    W = H = 16
    g, k = 64, 12
    S = L // 2
    ij = np.stack([rng.integers(-20, 78, L), rng.integers(-77, 78, L)], 1)
    ij[S] = (-30, 0)
    proj = np.zeros((L, 4), np.float32)
    proj[:, :2] = ij / float(g)
    proj[:, 2] = rng.uniform(1.0, 3.0, L)
    proj[S, 2] = 0.5
    last = L - 256 * ((L - 1) // 256)                                       # entries of the last chunk
    by_z = np.argsort(proj[:, 2], kind="stable")
    lst = np.concatenate([rng.permutation(by_z[last:]), rng.permutation(by_z[:last])]).astype(np.int32)
    rgb = rng.integers(0, 256, (L, 3)).astype(np.float32)
    return NS(W=W, H=H, g=g, k=k, radius=np.float32((2 * k + 1) / (2.0 * g)), proj=proj, rgb=rgb, n=L, S=S, last=last, offs=np.array([0, L], np.int32),
              lst=lst, band=0.0, b=0.0, rejected=np.zeros(0, np.int64))


@functools.lru_cache(maxsize=None)
def random_case(W, H, r_px, n, seed):
    """random fp32 coordinates over the image and a margin of one radius, plus the rejected points"""
    rng = np.random.default_rng(seed)
    radius = np.float32(r_px * 2.0 / min(W, H))
    ax, ay = max(1.0, W / H) + float(radius), max(1.0, H / W) + float(radius)
    pts = np.zeros((n, 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = rng.uniform(-ax, ax, n), rng.uniform(-ay, ay, n), rng.uniform(1.0, 3.0, n)
    rej = rejected_points(W, H)
    proj = np.concatenate([pts, rej])
    kind = np.concatenate([np.zeros(n, np.int8), np.full(len(rej), 2, np.int8)])
    perm = rng.permutation(len(proj))
    proj, kind = proj[perm], kind[perm]
    rgb = rng.integers(0, 256, (len(proj), 3)).astype(np.float32)
    band = rim_band(W, H, radius)
    return NS(W=W, H=H, radius=radius, proj=proj, rgb=rgb, n=len(proj), rejected=np.nonzero(kind == 2)[0], band=band, b=band / float(radius) ** 2)


@functools.lru_cache(maxsize=None)
def bin_case(W, H, everywhere=False):
    """random fp32 points for the bin properties; `everywhere`: a radius at which the disc of a point near the centre touches every tile"""
    rng = np.random.default_rng(W * 131 + H)
    radius = np.float32(3.0 * max(W / H, H / W, 1.0)) if everywhere else np.float32(2.3 * 2.0 / min(W, H))
    ax, ay = max(1.0, W / H), max(1.0, H / W)
    n = 40 if everywhere else 700
    m = 0.1 if everywhere else float(radius) + 4.0 / min(W, H)
    pts = np.zeros((n, 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = rng.uniform(-ax - m, ax + m, n), rng.uniform(-ay - m, ay + m, n), rng.uniform(0.5, 3.0, n)
    proj = rng.permutation(np.concatenate([pts, rejected_points(W, H)]))
    return NS(W=W, H=H, radius=radius, proj=proj, n=len(proj))


@functools.lru_cache(maxsize=None)
def rim_case(W=72, H=40):
    """discs whose rim passes a pixel centre on the far side of a tile edge by less than 1e-6 NDC units (a few ulps): the point sits in one tile and just
    reaches the first pixel column (row) of the next, so the next tile must be listed and the rounding of splat_tile_box's u and v is all that could
    lose it.  72 x 40: the NDC range of x, 3.6, is not a binary fraction, so u does round"""
    rng = np.random.default_rng(61)
    radius = np.float32(2.3 * 2.0 / min(W, H))
    xf, yf = pix_ndc64(W, H), pix_ndc64(H, W)
    pts = []
    for centres, axis, S in ((xf, 0, W), (yf, 1, H)):
        for i in [e + d for e in range(15, S - 1, 16) for d in (0, 1)]:
            side = 1.0 if i % 16 == 0 else -1.0                            # +X is left, +Y is up: a larger coordinate is a SMALLER index
            for _ in range(150):
                p = np.zeros(4)
                p[axis] = centres[i] + side * (float(radius) - rng.uniform(0.0, 1e-6))
                p[1 - axis] = (yf if axis == 0 else xf)[rng.integers(0, H if axis == 0 else W)]
                p[2] = rng.uniform(0.5, 3.0)
                pts.append(p)
    proj = np.array(pts).astype(np.float32)
    return NS(W=W, H=H, radius=radius, proj=proj, n=len(proj))


@functools.lru_cache(maxsize=None)
def reference(kind, key, K):
    """one fp64 reference per (case, K), shared by the tests of both modules"""
    c = case_of(kind, key)
    return ref_render(c.proj, c.rgb, c.W, c.H, c.radius, K, band=c.band)


def case_of(kind, key):
    if kind == "kb":
        return kb_case(key)
    if kind == "chunk":
        return chunk_case(key)
    if kind == "partial":
        return grid_case(*PARTIAL[key])
    if kind == "empty":
        return grid_case(64, 32, 25, 300, 16, window=(0.55, 0.7, 0.1, 0.4))      # every disc inside tile (ty 1, tx 1): seven empty tiles
    if kind == "random":
        W, H, r_px, _, n, seed = RANDOM[key]
        return random_case(W, H, r_px, n, seed)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def lists_of(kind, key):
    c = case_of(kind, key)
    if kind == "chunk":
        return c.offs, np.concatenate([c.lst, np.zeros(1, np.int32)])
    return build_lists(reference(kind, key, 1).cover, c.rejected, 0.1, 7)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# bin: the fp64 tile set, the properties, a numpy fp32 restatement of splat_tile_box
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def drawable(proj):
    with np.errstate(invalid="ignore"):
        return (proj[:, 2] >= 0) & (np.abs(proj[:, 0]) < 1e30) & (np.abs(proj[:, 1]) < 1e30)


def disc_box64(proj, radius, W, H):
    """fp64 bounding box of every disc in pixel coordinates: (col_lo, col_hi, row_lo, row_hi), real numbers (a pixel centre sits at its integer index)"""
    p = np.asarray(proj, np.float64)
    r = float(np.float32(radius))
    rx, ry = 2.0 * max(1.0, W / H), 2.0 * max(1.0, H / W)
    col = lambda x: W - 1 - ((x + rx / 2) * W - rx / 2) / rx                # noqa: E731
    row = lambda y: H - 1 - ((y + ry / 2) * H - ry / 2) / ry                # noqa: E731
    return col(p[:, 0] + r), col(p[:, 0] - r), row(p[:, 1] + r), row(p[:, 1] - r)


def cover64(proj, W, H, radius):
    """[tiles, n] bool: the fp64 disc strictly covers a pixel centre of the tile"""
    return ref_render(proj, np.zeros((len(proj), 3)), W, H, radius, 1).cover


def check_bin(proj, W, H, radius, counts_a, counts_b, offs, lst, cover, guard=None):
    """the properties of the module docstring; lst was filled with -1 before the fill pass.  -> number of listed pairs"""
    n = len(proj)
    TW, TH = tiles_of(W, H)
    counts_a, counts_b, offs, lst = (np.asarray(v).astype(np.int64) for v in (counts_a, counts_b, offs, lst))
    assert (counts_a >= 0).all() and np.array_equal(counts_a, counts_b), "the fill pass must leave the counts of the count pass"
    total = int(offs[-1])
    assert np.array_equal(np.diff(offs), counts_a)
    assert ((lst[:total] >= 0) & (lst[:total] < n)).all(), "every slot of every segment written with a valid id"
    if guard is not None:
        assert (lst[total:] == guard).all(), "nothing written past the last segment"
    tile = np.repeat(np.arange(TW * TH), counts_a)
    pairs = tile * n + lst[:total]
    assert len(np.unique(pairs)) == total, "a point listed twice in one tile"
    t_need, p_need = np.nonzero(cover)
    missing = ~np.isin(t_need * n + p_need, pairs)
    assert not missing.any(), ("covering (tile, point) pairs not listed", list(zip(t_need[missing][:5], p_need[missing][:5])))
    ids = lst[:total]
    assert drawable(np.asarray(proj))[ids].all(), "a point behind the camera or not finite was binned"
    c_lo, c_hi, r_lo, r_hi = (v[ids] for v in disc_box64(proj, radius, W, H))
    tx, ty = tile % TW, tile // TW
    loose = (16 * tx > c_hi + 2) | (np.minimum(16 * tx + 15, W - 1) < c_lo - 2) | (16 * ty > r_hi + 2) | (np.minimum(16 * ty + 15, H - 1) < r_lo - 2)
    assert not loose.any(), ("listed tiles beyond the disc's box grown by two pixels", int(loose.sum()))
    return total


def tile_box_f32(proj, radius, W, H, margin=1):
    """splat_tile_box in numpy fp32 -> [tiles, n] bool (margin = 0: without its - 1 / + 1)"""
    f = np.float32
    a = np.asarray(proj, np.float32)
    radius = f(radius)
    TW, TH = tiles_of(W, H)
    out = np.zeros((TW * TH, len(a)), bool)
    rx = f(W) / f(H) * f(2) if W > H else f(2)
    ry = f(H) / f(W) * f(2) if H > W else f(2)
    ox, oy = rx * f(0.5), ry * f(0.5)
    for p in np.nonzero(drawable(a))[0]:
        x, y = a[p, 0], a[p, 1]
        u_lo, u_hi = ((x - radius + ox) * f(W) - ox) / rx, ((x + radius + ox) * f(W) - ox) / rx
        v_lo, v_hi = ((y - radius + oy) * f(H) - oy) / ry, ((y + radius + oy) * f(H) - oy) / ry
        if u_hi < -1 or u_lo > W or v_hi < -1 or v_lo > H:
            continue
        c0, c1 = W - 1 - int(math.floor(min(u_hi, f(W)))) - margin, W - 1 - int(math.ceil(max(u_lo, f(-1)))) + margin
        r0, r1 = H - 1 - int(math.floor(min(v_hi, f(H)))) - margin, H - 1 - int(math.ceil(max(v_lo, f(-1)))) + margin
        c0, r0, c1, r1 = max(c0, 0), max(r0, 0), min(c1, W - 1), min(r1, H - 1)
        if c0 > c1 or r0 > r1:
            continue
        for ty in range(r0 >> 4, (r1 >> 4) + 1):
            out[ty * TW + (c0 >> 4):ty * TW + (c1 >> 4) + 1, p] = True
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# lift and project in fp64
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def lift64(depth, idx, W, H, fx, fy):
    idx = np.asarray(idx, np.int64)
    z = np.asarray(depth, np.float64).reshape(-1)[idx]
    j, i = idx // W, idx % W
    fx, fy = float(np.float32(fx)), float(np.float32(fy))
    return np.stack([-(i - W / 2) * z / fx, -(j - H / 2) * z / fy, z, np.zeros_like(z)], 1)


def xform(center, translate, rotate, scale, tan_half_fov):
    """the fp32 fields of a SplatXform, as fp64 arrays"""
    f = lambda v: np.asarray(v, np.float32).astype(np.float64)            # noqa: E731
    return NS(c=f(center), t=f(translate), R=f(rotate).reshape(3, 3), s=f(scale), tan=float(np.float32(tan_half_fov)))


def project64(pts, X):
    v = ((np.asarray(pts, np.float64)[:, :3] - X.c + X.t) @ X.R) * X.s + X.c
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([v[:, 0] / X.tan / v[:, 2], v[:, 1] / X.tan / v[:, 2], v[:, 2]], 1)


def project_bound(pts, X):
    """-> (bound of ndc x, of ndc y, of z_view) per point, from the module docstring's derivation with |q| <= 3M"""
    P = np.asarray(pts, np.float64)[:, :3]
    M = max(np.abs(P).max(), np.abs(X.c).max(), np.abs(X.t).max())
    e_q = 2 * U * 2 * M + 2 * U * 3 * M                                     # 2 x (u |P - c| + u |q|)
    col = np.abs(X.R).sum(0)
    v = ((P - X.c + X.t) @ X.R) * X.s + X.c
    e_v = np.abs(X.s) * col * (e_q + 2 * 3 * U * 3 * M) + 2 * U * (np.abs(v - X.c) + np.abs(v))
    inv = 1.0 / X.tan
    z = np.abs(v[:, 2])
    e_ndc = [(e_v[:, a] + np.abs(v[:, a]) / z * e_v[:, 2]) * inv / z * (1 + 8 * U) + 4 * U * np.abs(v[:, a]) * inv / z for a in (0, 1)]
    return e_ndc[0], e_ndc[1], e_v[:, 2]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    from freefine_amd import _lib as L
    return torch, L, L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(torch, gpu, shape, dtype, value, guard):
    """a buffer of `shape` between two guard zones, all filled with `value` -> (whole flat buffer, view, check())"""
    size = int(np.prod(shape))
    whole = torch.full((guard + size + guard,), value, dtype=dtype, device=gpu)
    view = whole[guard:guard + size].view(*shape)

    def intact():
        return bool((whole[:guard] == value).all() and (whole[guard + size:] == value).all())
    return whole, view, intact


def render(gpu, proj, rgb, offs, lst, radius, K, W, H, prefilled=None):
    """ffn_splat_render into sentinel-filled, guarded outputs -> (image f32 [H, W, 3], idx_sum i32 [H, W], covered u8 [H, W]) as numpy"""
    torch, L, lib, stream = _dev()
    TW, TH = tiles_of(W, H)
    validate_lists(offs, lst, len(proj), TW * TH)
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (proj, rgb, offs, lst)]
    guard = 16 * (W + 16)
    _, image, ok0 = guarded(torch, gpu, (H, W, 3), torch.float32, SENT_F, 3 * guard)
    _, idx_sum, ok1 = guarded(torch, gpu, (H, W), torch.int32, SENT_I, guard)
    _, covered, ok2 = guarded(torch, gpu, (H, W), torch.uint8, SENT_B, guard)
    L.check(lib.ffn_splat_render(stream, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), float(radius), K, W, H, image.data_ptr(),
                                 idx_sum.data_ptr(), covered.data_ptr()), "splat_render")
    torch.cuda.synchronize()
    assert ok0() and ok1() and ok2(), "the sentinel outside H x W was overwritten"
    return image.cpu().numpy(), idx_sum.cpu().numpy(), covered.cpu().numpy()


def run_bin(gpu, proj, radius, W, H):
    """count pass, scan, fill pass as warp3d.py does them -> counts_a, counts_b, offs, lst (list filled with -1 first, 64 guard entries)"""
    torch, L, lib, stream = _dev()
    TW, TH = tiles_of(W, H)
    p = torch.from_numpy(np.ascontiguousarray(proj)).to(gpu)
    counts = torch.zeros(TW * TH, dtype=torch.int32, device=gpu)
    L.check(lib.ffn_splat_bin(stream, 0, p.data_ptr(), len(proj), float(radius), W, H, counts.data_ptr(), None, None), "splat_bin(count)")
    counts_a = counts.cpu().numpy()
    offs = np.zeros(TW * TH + 1, np.int32)
    offs[1:] = np.cumsum(counts_a)
    assert (counts_a >= 0).all() and int(counts_a.sum()) <= len(proj) * TW * TH
    lst = torch.full((int(offs[-1]) + 64,), -1, dtype=torch.int32, device=gpu)
    counts.zero_()
    offs_d = torch.from_numpy(offs).to(gpu)
    L.check(lib.ffn_splat_bin(stream, 1, p.data_ptr(), len(proj), float(radius), W, H, counts.data_ptr(), offs_d.data_ptr(), lst.data_ptr()), "splat_bin(fill)")
    torch.cuda.synchronize()
    return counts_a, counts.cpu().numpy(), offs, lst.cpu().numpy()


def make_xform(L, X):
    x = L.SplatXform()
    for a in range(3):
        x.center[a], x.translate[a], x.scale[a] = float(X.c[a]), float(X.t[a]), float(X.s[a])
    for a in range(9):
        x.rotate[a] = float(X.R.reshape(-1)[a])
    x.tan_half_fov = X.tan
    return x


def run_lift(gpu, depth, idx, W, H, fx, fy):
    torch, L, lib, stream = _dev()
    d, i = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).to(gpu), torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(gpu)
    _, pts, ok = guarded(torch, gpu, (len(idx), 4), torch.float32, SENT_F, 64)
    L.check(lib.ffn_splat_lift(stream, d.data_ptr(), i.data_ptr(), pts.data_ptr(), len(idx), W, H, float(fx), float(fy)), "splat_lift")
    torch.cuda.synchronize()
    assert ok()
    return pts.cpu().numpy()


def run_project(gpu, pts, X):
    torch, L, lib, stream = _dev()
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(gpu)
    _, proj, ok = guarded(torch, gpu, (len(pts), 4), torch.float32, SENT_F, 64)
    L.check(lib.ffn_splat_project(stream, p.data_ptr(), proj.data_ptr(), len(pts), C.byref(make_xform(L, X))), "splat_project")
    torch.cuda.synchronize()
    assert ok()
    return proj.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# render on the exact grid
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", K_EDGES)
def test_render_k_boundaries(gpu, K):
    """the template edges 8 | 9 and 16 | 17 and the extremes, each on pixels with fewer than, exactly and more than K covering points (the CPU module
    shows that compositing K - 1 or K + 1 points instead leaves the bound)"""
    c, ref = kb_case(), reference("kb", "random", K)
    assert (ref.count < K).any() and (ref.count == K).any() and (ref.count > K).any() and ref.count.max() > 32 and not ref.amb.any()
    offs, lst = lists_of("kb", "random")
    hold(render(gpu, c.proj, c.rgb, offs, lst, c.radius, K, c.W, c.H), ref, K, what="k-boundaries")


@pytest.mark.parametrize("z", ["equal", "two"])
@pytest.mark.parametrize("K", [8, 17])
def test_render_depth_ties(gpu, z, K):
    """every depth equal, then two depth values: (depth, id) alone decides which K points stay and in which order they composite; on pixels with more
    than K candidates slot K - 1 ties with the point just cut off"""
    c, ref = kb_case(z), reference("kb", z, K)
    assert (ref.count > K).sum() > 100
    offs, lst = lists_of("kb", z)
    hold(render(gpu, c.proj, c.rgb, offs, lst, c.radius, K, c.W, c.H), ref, K, what=f"ties ({z})")


def test_render_is_independent_of_list_order(gpu):
    """the tile lists are filled through atomics in any order: reversed and twice randomly permuted lists give the same bits"""
    K = 9
    c = kb_case("two")
    offs, lst = lists_of("kb", "two")
    base = render(gpu, c.proj, c.rgb, offs, lst, c.radius, K, c.W, c.H)
    hold(base, reference("kb", "two", K), K, what="order (base)")
    rng = np.random.default_rng(5)
    for how in ("reversed", "random", "random"):
        segs = [s[::-1] if how == "reversed" else rng.permutation(s) for s in segments(offs, lst)]
        o2, l2 = pack_lists(segs)
        assert np.array_equal(o2, offs) and not np.array_equal(l2, lst)
        other = render(gpu, c.proj, c.rgb, o2, l2, c.radius, K, c.W, c.H)
        for a, b in zip(base, other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), how


@pytest.mark.parametrize("L", CHUNK_LENGTHS)
def test_render_chunk_boundary(gpu, L):
    """one tile whose list ends exactly at, one short of and one past the 256-point LDS chunk (and the same at 512): the nearest point of some pixels,
    and the only point of others, is staged in the last chunk"""
    K = 8
    c, ref = chunk_case(L), reference("chunk", L, K)
    in_last = np.isin(ref.first, c.lst[L - c.last:])
    assert ((ref.first == c.S) & (ref.count == 1)).any() and ((ref.first == c.S) & (ref.count > 1)).any() and in_last.sum() >= 4
    assert (ref.count > K).any() and (ref.count == 0).any()
    offs, lst = lists_of("chunk", L)
    hold(render(gpu, c.proj, c.rgb, offs, lst, c.radius, K, c.W, c.H), ref, K, what=f"chunk {L}")


@pytest.mark.parametrize("name", list(PARTIAL))
def test_render_rejected_and_border_points(gpu, name):
    """partial tiles (8 x 8: one tile with 192 dead lanes; 8 x 32 / 32 x 8: dead columns / rows in every tile; 32 x 64 / 64 x 32: the non-square NDC range
    on either axis), discs over every border and corner, and in every tile's list the points that must not be drawn: z < 0, z = +-0 with the
    coordinates the projection gives them, coordinates beyond 1e30.  The sentinel outside H x W survives (render checks it)"""
    K = 5
    c, ref = case_of("partial", name), reference("partial", name, K)
    offs, lst = lists_of("partial", name)
    assert all(np.isin(c.rejected, s).all() for s in segments(offs, lst))
    hold(render(gpu, c.proj, c.rgb, offs, lst, c.radius, K, c.W, c.H), ref, K, what=f"partial {name}")


def test_render_overwrites_every_live_pixel_of_empty_tiles(gpu):
    K = 17
    c, ref = case_of("empty", None), reference("empty", None, K)
    offs, lst = lists_of("empty", None)
    TW, TH = tiles_of(c.W, c.H)
    untouched = [t for t in range(TW * TH) if not ref.cover[t].any()]
    assert len(untouched) == 7
    only = [s if t not in untouched else s[:0] for t, s in enumerate(segments(offs, lst))]        # really empty lists for the empty tiles
    out = render(gpu, c.proj, c.rgb, *pack_lists(only), c.radius, K, c.W, c.H)
    hold(out, ref, K, what="empty tiles")
    empty = ref.covered == 0
    assert (out[0][empty] == 0).all() and (out[1][empty] == -K).all() and (out[2][empty] == 0).all() and empty.sum() > 7 * 256


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# bin, and bin + render on sizes that cannot be exact
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", BIN_SIZES)
@pytest.mark.parametrize("everywhere", [False, True], ids=["discs", "everywhere"])
def test_bin_properties(gpu, W, H, everywhere):
    c = bin_case(W, H, everywhere)
    cover = cover64(c.proj, W, H, c.radius)
    if everywhere:
        assert cover.all(0).any(), "no disc touches every tile"
    counts_a, counts_b, offs, lst = run_bin(gpu, c.proj, c.radius, W, H)
    total = check_bin(c.proj, W, H, c.radius, counts_a, counts_b, offs, lst, cover, guard=-1)
    print(f"SPLAT bin {W}x{H}: {total} pairs listed, {int(cover.sum())} needed")


def test_bin_keeps_the_tile_a_rim_just_reaches(gpu):
    c = rim_case()
    cover = cover64(c.proj, c.W, c.H, c.radius)
    counts_a, counts_b, offs, lst = run_bin(gpu, c.proj, c.radius, c.W, c.H)
    check_bin(c.proj, c.W, c.H, c.radius, counts_a, counts_b, offs, lst, cover, guard=-1)


@pytest.mark.parametrize("name", list(PARTIAL))
def test_bin_on_the_grid_cases(gpu, name):
    """the border and the rejected points of the render cases through the bin, then the render on the lists the bin made"""
    K = 5
    c, ref = case_of("partial", name), reference("partial", name, K)
    counts_a, counts_b, offs, lst = run_bin(gpu, c.proj, c.radius, c.W, c.H)
    check_bin(c.proj, c.W, c.H, c.radius, counts_a, counts_b, offs, lst, ref.cover, guard=-1)
    hold(render(gpu, c.proj, c.rgb, offs, lst, c.radius, K, c.W, c.H), ref, K, what=f"bin + render {name}")


@pytest.mark.parametrize("name", list(RANDOM))
def test_render_random_sizes_through_the_bin(gpu, name):
    W, H, _, K, _, _ = RANDOM[name]
    c, ref = case_of("random", name), reference("random", name, K)
    assert ref.amb.mean() <= AMBIGUOUS_CAP and (ref.count > K).any() and (ref.count < K).any()
    counts_a, counts_b, offs, lst = run_bin(gpu, c.proj, c.radius, W, H)
    check_bin(c.proj, W, H, c.radius, counts_a, counts_b, offs, lst, ref.cover, guard=-1)
    hold(render(gpu, c.proj, c.rgb, offs, lst, c.radius, K, W, H), ref, K, c.b, what=f"random {name}")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# lift and project
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_lift_against_fp64(gpu):
    rng = np.random.default_rng(31)
    W, H, fx, fy = 53, 37, 41.7, 66.1
    depth = rng.uniform(0.5, 9.0, (H, W)).astype(np.float32)
    idx = rng.permutation(W * H)[:W * H // 3].astype(np.int32)                # unsorted, two pixels in three skipped
    out = run_lift(gpu, depth, idx, W, H, fx, fy)
    ref = lift64(depth, idx, W, H, fx, fy)
    err = np.abs(out - ref)
    print(f"SPLAT lift: |err| / bound = {(err / (4 * U * np.abs(ref) + 1e-300)).max():.3f}")
    assert (err <= 4 * U * np.abs(ref)).all() and (out[:, 3] == 0).all() and np.array_equal(out[:, 2], depth.reshape(-1)[idx])


def _project_case():
    from oracle import warp3d as OW
    rng = np.random.default_rng(32)
    n = 3000
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = rng.uniform(-1.0, 1.0, (n, 3)) * (0.8, 0.6, 0.4) + (0.3, -0.2, 3.0)
    X = xform(pts[:, :3].mean(0), (0.31, -0.17, 0.23), OW.euler_xyz_matrix(20, -35, 50).reshape(-1), (1.3, 0.7, 0.9), math.tan(math.radians(30.0)))
    return pts, X


def test_project_against_fp64(gpu):
    """rotation, anisotropic scale and translation; fp64 from the same fp32 SplatXform fields; z_view > 1 on every compared point"""
    pts, X = _project_case()
    ref = project64(pts, X)
    assert ref[:, 2].min() > 1.0
    out = run_project(gpu, pts, X)
    bx, by, bz = project_bound(pts, X)
    ratio = max((np.abs(out[:, a] - ref[:, a]) / b).max() for a, b in ((0, bx), (1, by), (2, bz)))
    print(f"SPLAT project: |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0 and (out[:, 3] == 0).all()


def test_project_behind_the_camera_and_at_zero_depth(gpu):
    """z_view < 0: the sign survives (the bin refuses the point); z_view = +-0: the coordinates are +-inf or NaN, never finite; none of them is binned"""
    pts = np.zeros((8, 4), np.float32)
    pts[:, :3] = [(0.5, 0.2, 1.0), (-0.5, 0.1, 0.25), (0.3, -0.2, 0.0), (0.0, 0.0, 0.0), (-1.5, 0.0, 0.0), (0.0, 0.25, 0.0), (0.1, 0.1, 3.0), (0.2, 0.0, 2.5)]
    tan = math.tan(math.radians(30.0))
    X0 = xform((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), np.eye(3).reshape(-1), (1.0, 1.0, 1.0), tan)       # z_view = z: rows 2 .. 5 land on +0.0 exactly
    out = run_project(gpu, pts, X0)
    at0 = np.array([2, 3, 4, 5])
    assert (out[at0, 2] == 0).all() and not np.isfinite(out[at0, :2]).any()
    Xb = xform((0.0, 0.0, 0.0), (0.0, 0.0, -4.0), np.eye(3).reshape(-1), (1.0, 1.0, 1.0), tan)          # z_view = z - 4 < 0 everywhere
    behind = run_project(gpu, pts, Xb)
    assert (behind[:, 2] < 0).all() and np.array_equal(behind[:, 2], pts[:, 2] - np.float32(4.0))
    Xn = xform((0.0, 0.0, -0.0), (0.0, 0.0, 0.0), np.eye(3).reshape(-1), (1.0, 1.0, -1.0), tan)         # (0 * -1) + -0.0 = -0.0
    neg0 = run_project(gpu, pts[at0], Xn)
    assert (neg0[:, 2] == 0).all() and np.signbit(neg0[:, 2]).all() and not np.isfinite(neg0[:, :2]).any()
    for proj in (out[at0], behind, neg0):
        counts_a, counts_b, offs, lst = run_bin(gpu, proj, 0.5, 32, 32)
        assert counts_a.sum() == 0 and counts_b.sum() == 0 and (lst == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the second grid-stride pass of lift, project and both bin passes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def wrap_case():
    """1200 x 960 depth plane, depths in {1, 2, 4}, fx = fy = 64, identity transform about 0, tan_half_fov = 1: pixel (i, j) projects EXACTLY to
    (-(i - 600) / 64, -(j - 480) / 64).  The first 4096 * 256 points lie at least 16 source pixels (a quarter NDC unit) outside the 32 x 32 target image
    (radius 10.5 / 128: the bin keeps within two target pixels = 1 / 8 NDC of a disc), the last 300 inside it"""
    rng = np.random.default_rng(41)
    W0, H0 = 1200, 960
    j, i = np.divmod(np.arange(W0 * H0), W0)
    di, dj = i - W0 // 2, j - H0 // 2
    off = np.nonzero((np.abs(di) > 80) | (np.abs(dj) > 80))[0]
    on = np.nonzero((np.abs(di) <= 64) & (np.abs(dj) <= 64))[0]
    idx = np.concatenate([rng.permutation(off)[:WRAP_N - 300], rng.permutation(on)[:300]]).astype(np.int32)
    assert len(idx) == WRAP_N
    depth = rng.choice([1.0, 2.0, 4.0], (H0, W0)).astype(np.float32)
    X = xform((0, 0, 0), (0, 0, 0), np.eye(3).reshape(-1), (1, 1, 1), 1.0)
    return NS(W0=W0, H0=H0, idx=idx, depth=depth, X=X, W=32, H=32, radius=np.float32(21 / 256.0), f=64.0)


def test_second_grid_pass_of_lift_project_and_bin(gpu):
    K = 5
    c = wrap_case()
    pts = run_lift(gpu, c.depth, c.idx, c.W0, c.H0, c.f, c.f)
    ref_pts = lift64(c.depth, c.idx, c.W0, c.H0, c.f, c.f)
    assert np.array_equal(pts.astype(np.float64), ref_pts), "this lift is exact in fp32"
    proj = run_project(gpu, pts, c.X)
    ref_proj = project64(ref_pts, c.X)
    assert np.array_equal(proj[:, :3].astype(np.float64), ref_proj) and (proj[:, 3] == 0).all(), "and so is this projection"
    counts_a, counts_b, offs, lst = run_bin(gpu, proj, c.radius, c.W, c.H)
    rgb = np.random.default_rng(42).integers(0, 256, (WRAP_N, 3)).astype(np.float32)
    ref = ref_render(proj, rgb, c.W, c.H, c.radius, K)
    check_bin(proj, c.W, c.H, c.radius, counts_a, counts_b, offs, lst, ref.cover, guard=-1)
    assert set(lst[:offs[-1]].tolist()) == set(range(WRAP_N - 300, WRAP_N)), "exactly the last 300 points are binned"
    assert ref.covered.sum() > 300 and not ref.amb.any()
    hold(render(gpu, proj, rgb, offs, lst, c.radius, K, c.W, c.H), ref, K, what="second grid pass")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu):
    torch, L, lib, stream = _dev()
    c = case_of("partial", "8x8")
    offs, lst = lists_of("partial", "8x8")
    W, H, n = c.W, c.H, c.n
    proj, rgb, offs_d, lst_d = (torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (c.proj, c.rgb, offs, lst))
    depth = torch.ones(H * W, device=gpu)
    idx = torch.arange(H * W, dtype=torch.int32, device=gpu)
    image = torch.full((H, W, 3), SENT_F, device=gpu)
    idx_sum = torch.full((H, W), SENT_I, dtype=torch.int32, device=gpu)
    covered = torch.full((H, W), SENT_B, dtype=torch.uint8, device=gpu)
    pts = torch.full((n, 4), SENT_F, device=gpu)
    out_proj = torch.full((n, 4), SENT_F, device=gpu)
    counts = torch.full((1,), SENT_I, dtype=torch.int32, device=gpu)
    out_lst = torch.full((len(lst),), SENT_I, dtype=torch.int32, device=gpu)
    x = make_xform(L, xform((0, 0, 0), (0, 0, 0), np.eye(3).reshape(-1), (1, 1, 1), 0.5))
    x_bad = [make_xform(L, xform((0, 0, 0), (0, 0, 0), np.eye(3).reshape(-1), (1, 1, 1), t)) for t in (0.0, -0.5)]
    p = lambda t: t.data_ptr()                                               # noqa: E731
    r = float(c.radius)

    def rend(K=5, radius=r, pr=p(proj), co=p(rgb), of=p(offs_d), li=p(lst_d), im=p(image), su=p(idx_sum), cv=p(covered)):
        return lib.ffn_splat_render(stream, pr, co, of, li, radius, K, W, H, im, su, cv)

    def binp(fill=0, nn=n, radius=r, pr=p(proj), cn=p(counts), of=None, li=None):
        return lib.ffn_splat_bin(stream, fill, pr, nn, radius, W, H, cn, of, li)

    def lift(nn=H * W, fx=10.0, fy=10.0, de=p(depth), ix=p(idx), ou=p(pts)):
        return lib.ffn_splat_lift(stream, de, ix, ou, nn, W, H, fx, fy)

    def projt(nn=n, xf=x, pi=p(proj), ou=p(out_proj)):
        return lib.ffn_splat_project(stream, pi, ou, nn, C.byref(xf) if xf is not None else None)

    # (entry, the word that tells this refusal's message from the entry's others, call)
    refused = [
        ("splat_render", "K=0 ", lambda: rend(K=0)), ("splat_render", "K=33 ", lambda: rend(K=33)), ("splat_render", "K=-1 ", lambda: rend(K=-1)),
        ("splat_render", "radius", lambda: rend(radius=0.0)), ("splat_render", "radius", lambda: rend(radius=-r)),
        *[("splat_render", "null operand", functools.partial(rend, **{k: None})) for k in ("pr", "co", "of", "li", "im", "su", "cv")],
        ("splat_bin", "radius", lambda: binp(radius=0.0)), ("splat_bin", "radius", lambda: binp(radius=-r)), ("splat_bin", "bad shape", lambda: binp(nn=0)),
        ("splat_bin", "null operand", lambda: binp(pr=None)), ("splat_bin", "null operand", lambda: binp(cn=None)),
        ("splat_bin", "filling pass", lambda: binp(fill=1)), ("splat_bin", "filling pass", lambda: binp(fill=1, of=p(offs_d))),
        ("splat_bin", "filling pass", lambda: binp(fill=1, li=p(out_lst))),
        ("splat_bin", "bad shape", lambda: binp(fill=1, nn=0, of=p(offs_d), li=p(out_lst))),
        ("splat_lift", "bad shape", lambda: lift(nn=0)), ("splat_lift", "focal length", lambda: lift(fx=0.0)), ("splat_lift", "focal length", lambda: lift(fy=0.0)),
        *[("splat_lift", "null operand", functools.partial(lift, **{k: None})) for k in ("de", "ix", "ou")],
        ("splat_project", "empty cloud", lambda: projt(nn=0)), ("splat_project", "tan_half_fov", lambda: projt(xf=x_bad[0])),
        ("splat_project", "tan_half_fov", lambda: projt(xf=x_bad[1])),
        ("splat_project", "null operand", lambda: projt(xf=None)), ("splat_project", "null operand", lambda: projt(pi=None)),
        ("splat_project", "null operand", lambda: projt(ou=None)),
    ]
    for i, (entry, word, call) in enumerate(refused):
        # another entry's refusal first (it writes nothing either), so that a message left over from the refusal before cannot pass for this one's
        assert lib.ffn_cast(stream, L.FFN_F32, L.FFN_F32, None, None, 0) != 0 and lib.ffn_last_error().decode().startswith("cast:")
        rc = call()
        msg = lib.ffn_last_error().decode()
        assert rc != 0 and msg.startswith(entry + ":") and word in msg, (i, entry, word, rc, msg)
    torch.cuda.synchronize()
    assert (image == SENT_F).all() and (idx_sum == SENT_I).all() and (covered == SENT_B).all()
    assert (pts == SENT_F).all() and (out_proj == SENT_F).all() and (counts == SENT_I).all() and (out_lst == SENT_I).all()
    # and the same operands are accepted when nothing is wrong with them
    assert rend() == 0 and lift() == 0 and projt() == 0
    torch.cuda.synchronize()
    assert (idx_sum != SENT_I).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# through the Python entry: the operands warp3d.py hands to project and render are recorded, and every stage is held to fp64 on them
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def entry_case(W, H, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = (2.0 + rng.random((H, W))).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)
    mask[H // 4:3 * H // 4, W // 5:4 * W // 5] = 255
    return img, depth, mask, 0.5 * min(H, W) / math.tan(math.radians(30.0))


class Recorder:
    """stands in for the library inside warp3d.py: forwards every call, and copies the operands of project and render to the host"""
    def __init__(self, torch, lib):
        self.torch, self.lib, self.calls = torch, lib, {}

    def __getattr__(self, name):
        real = getattr(self.lib, name)

        def call(*a):
            rc = real(*a)
            if name == "ffn_splat_project":
                n = a[3]
                x = a[4]._obj
                self.calls[name] = NS(pts=self.read(a[1], (n, 4)), proj=self.read(a[2], (n, 4)), n=n,
                                      X=xform(list(x.center), list(x.translate), list(x.rotate), list(x.scale), x.tan_half_fov))
            if name == "ffn_splat_render":                                  # while the caller's tensors are alive; n from the project call before it
                self.calls[name] = NS(rgb=self.read(a[2], (self.calls["ffn_splat_project"].n, 3)), radius=a[5], K=a[6], W=a[7], H=a[8])
            return rc
        return call

    def read(self, ptr, shape):
        """a device copy of the fp32 array at `ptr` (the library's own fp32 -> fp32 cast), brought to the host"""
        from freefine_amd import _lib as L
        out = self.torch.empty(shape, dtype=self.torch.float32, device="cuda")
        L.check(self.lib.ffn_cast(C.c_void_p(self.torch.cuda.current_stream().cuda_stream), L.FFN_F32, L.FFN_F32, ptr, out.data_ptr(), out.numel()), "cast")
        return out.cpu().numpy()


def run_entry(monkeypatch, gpu, fn):
    torch, L, lib, _ = _dev()
    from freefine_amd import warp3d
    rec = Recorder(torch, lib)
    monkeypatch.setattr(warp3d.L, "load", lambda: rec)
    try:
        result = fn(warp3d)
    finally:
        monkeypatch.undo()
    return result, rec.calls["ffn_splat_project"], rec.calls["ffn_splat_render"]


def hold_entry_stages(depth, keep, img, f, pr, rd):
    """lift, the centre, project: the recorded operands against fp64 of the test's own inputs"""
    H, W = depth.shape
    idx = np.nonzero(keep.reshape(-1))[0]
    assert pr.n == len(idx) and np.array_equal(rd.rgb, img.reshape(-1, 3).astype(np.float32)[idx])
    ref_pts = lift64(depth, idx, W, H, f, f)
    assert (np.abs(pr.pts - ref_pts) <= 4 * U * np.abs(ref_pts)).all()
    # the centre is a mean of n fp32 values: a reduction tree of depth d errs by <= d u max |P|, and 64 u covers any tree (not a serial sum)
    assert (np.abs(pr.X.c - ref_pts[:, :3].mean(0)) <= 64 * U * np.abs(ref_pts[:, :3]).max()).all()
    ref = project64(pr.pts, pr.X)
    assert ref[:, 2].min() > 0.5
    bounds = project_bound(pr.pts, pr.X)
    assert all((np.abs(pr.proj[:, a] - ref[:, a]) <= bounds[a]).all() for a in range(3))


def euler64(rx, ry, rz):
    """fp64 Rx Ry Rz of XYZ Euler angles in degrees (row-vector convention of pytorch3d's euler_angles_to_matrix)"""
    a, b, c = np.deg2rad([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def hold_host_operands(depth, keep, f, pr, tf, pixel_translation):
    """what warp3d.py computes on the host, as recorded in the SplatXform, against fp64 of the test's own inputs (|angles| <= 60 degrees here):
      R   an entry is at most two products of at most three sines / cosines; a factor errs by one ulp of the function and u |angle| <= 1.05 u of the
          angle in radians (2u together), a product of three by 6u + 2u of its own roundings, two of them and their sum by 17u: |R - R64| <= 20u
      s   the fp32 of the given factors
      t   relative: extent * tf, the extent being a difference of two lifted coordinates (4u |P| each) rounded once, the product once more and once when
          stored: |t - t64| <= (8u max |P| + 3u extent) |tf|, and exactly 0 where tf is 0;  in pixels: -+ tf * centre_z / f, rounded when stored
      c   hold_entry_stages"""
    H, W = depth.shape
    X = pr.X
    P = lift64(depth, np.nonzero(keep.reshape(-1))[0], W, H, f, f)[:, :3]
    assert np.abs(X.R - euler64(*tf[3:6])).max() <= 20 * U, np.abs(X.R - euler64(*tf[3:6])).max() / U
    assert np.array_equal(X.s, np.asarray(tf[6:9], np.float32).astype(np.float64))
    d = np.asarray(tf[:3], np.float64)
    if pixel_translation:
        want = np.array([-1.0, -1.0, 1.0]) * d * X.c[2] / float(f)
        tol = 2 * U * np.abs(want)
    else:
        ext = np.ptp(P, 0)
        want = ext * d
        tol = (8 * U * np.abs(P).max(0) + 3 * U * ext) * np.abs(d)
    assert (np.abs(X.t - want) <= tol).all(), (X.t, want, tol)
    assert np.isclose(X.tan, math.tan(math.radians(30.0)), rtol=2 * U)


def hold_uint8(out, want, keep, bound):
    """`.astype(np.uint8)` of the float image: the truncation of the fp64 value wherever that value is further than the bound from an integer, and
    within 1 + bound of it everywhere.  -> the number of values held to equality"""
    keep = np.broadcast_to(keep[..., None], want.shape)
    sure = keep & (np.abs(want - np.round(want)) > bound)
    assert np.array_equal(out[sure], np.floor(want[sure]).astype(np.uint8))
    assert (np.abs(out.astype(np.float64) - want)[keep] < 1 + bound).all()
    return int(sure.sum())


def test_point_cloud_warp_of_every_pixel(monkeypatch, gpu):
    """object_only = False on 21 x 37: all 777 pixels are lifted"""
    W, H, K = 21, 37, 8
    img, depth, mask, f = entry_case(W, H, 51)
    tf = [0.1, -0.05, 0.1, 12, -20, 8, 1.1, 0.9, 1.0]
    r = 2.5 * 2.0 / W
    (out, ref_mask, cov), pr, rd = run_entry(monkeypatch, gpu, lambda w: w.point_cloud_warp(img, depth, tf, f, f, mask, False, r, K, device=gpu, return_covered=True))
    hold_entry_stages(depth, np.ones((H, W), bool), img, f, pr, rd)
    assert (rd.K, rd.W, rd.H) == (K, W, H) and np.float32(rd.radius) == np.float32(r)
    hold_host_operands(depth, np.ones((H, W), bool), f, pr, tf, pixel_translation=False)
    band = rim_band(W, H, r)
    ref = ref_render(pr.proj, rd.rgb, W, H, r, K, band=band)
    keep = ~ref.amb
    print(f"SPLAT entry 21x37: ambiguous {int(ref.amb.sum())} of {ref.amb.size}")
    assert ref.amb.mean() <= AMBIGUOUS_CAP and ref.covered.sum() > 100
    assert np.array_equal(cov[keep], ref.covered[keep] * 255) and (ref_mask == 255).all()
    assert hold_uint8(out, ref.image, keep, image_bound(K, band / float(np.float32(r)) ** 2)) > 100


def test_coarse_edit_3d(monkeypatch, gpu):
    """the function the product calls, 40 x 72, translation in pixels: target_mask = the reference's covered set outside the ambiguous pixels, coarse =
    background bit for bit outside it and the warp inside, a 3-channel ori_mask = its first channel"""
    W, H, K = 40, 72, 5
    img, depth, mask, f = entry_case(W, H, 52)
    background = np.random.default_rng(53).integers(0, 256, (H, W, 3), dtype=np.uint8)
    tf = [6, -9, 4, 10, 25, -15, 1.2, 0.8, 1.0]
    (coarse, tgt), pr, rd = run_entry(monkeypatch, gpu, lambda w: w.coarse_edit_3d(img, mask, depth, tf, background, focal_length=f, points_per_pixel=K, device=gpu))
    hold_entry_stages(depth, mask > 0, img, f, pr, rd)
    r = np.float32(1.5 * 2.0 / W)
    assert (rd.K, rd.W, rd.H) == (K, W, H) and np.float32(rd.radius) == r
    hold_host_operands(depth, mask > 0, f, pr, tf, pixel_translation=True)                   # pixels -> world at the mean depth; +x left, +y up
    band = rim_band(W, H, r)
    ref = ref_render(pr.proj, rd.rgb, W, H, r, K, band=band)
    keep = ~ref.amb
    print(f"SPLAT entry 40x72: ambiguous {int(ref.amb.sum())} of {ref.amb.size}")
    assert ref.amb.mean() <= AMBIGUOUS_CAP and 200 < ref.covered.sum() < W * H - 200
    assert set(np.unique(tgt)) == {0, 255} and np.array_equal(tgt[keep], ref.covered[keep] * 255)
    assert np.array_equal(coarse[tgt == 0], background[tgt == 0])
    inside = keep & (tgt == 255)
    assert hold_uint8(coarse, ref.image, inside, image_bound(K, band / float(r) ** 2)) > 100
    from freefine_amd import warp3d
    m3 = np.stack([mask, 0 * mask, 255 - mask], -1)
    coarse3, tgt3 = warp3d.coarse_edit_3d(img, m3, depth, tf, background, focal_length=f, points_per_pixel=K, device=gpu)
    assert np.array_equal(coarse3, coarse) and np.array_equal(tgt3, tgt)
