"""The inputs, the reference and the bounds of tests/test_splat_gpu.py, checked without a device.  On every input that module uses: the grid cases are exact
in fp32 (fp32 numpy d2 == fp64 d2 on every pixel x point pair, no d2 == r2, fp32 pixel centres == fp64 ones) and have the pixels each test is about; the
random cases stay under the 1 % cap of ambiguous pixels; the hand-built tile lists are sufficient (a render restricted to each tile's list gives the
reference); the fp32 oracle/warp3d.splat agrees with the fp64 reference inside the bounds, so a kernel that passes is no worse than a plain fp32 evaluation;
every planted error is rejected; and the bin properties accept the fp64 tile set and a numpy fp32 restatement of splat_tile_box, and reject a bin that drops
a border tile."""
import numpy as np
import pytest

from oracle import warp3d as OW
from test_splat_gpu import (AMBIGUOUS_CAP, BIN_SIZES, CHUNK_LENGTHS, K_EDGES, PARTIAL, RANDOM, bin_case, case_of, check_bin, cover64, image_bound, lists_of,
                            lift64, mismatch, passes, pix_ndc64, project64, ref_render, reference, rim_case, segments, tile_box_f32, tiles_of, validate_lists, wrap_case)

GRID = [("kb", "random"), ("kb", "equal"), ("kb", "two"), ("empty", None)] + [("chunk", L) for L in CHUNK_LENGTHS] + [("partial", k) for k in PARTIAL]
SMALL = [("kb", "random", 9), ("kb", "equal", 8), ("kb", "two", 17), ("empty", None, 17)] + [("chunk", L, 8) for L in CHUNK_LENGTHS] + \
        [("partial", k, 5) for k in PARTIAL] + [("random", k, RANDOM[k][3]) for k in RANDOM]


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def as_out(ref):
    return ref.image, ref.idx_sum, ref.covered


def near(proj, W, H, radius):
    """the points that can matter: drawable and within two radii of the image"""
    xf, yf = pix_ndc64(W, H), pix_ndc64(H, W)
    m = 2 * float(radius)
    with np.errstate(invalid="ignore"):
        return np.nonzero((proj[:, 2] >= 0) & (np.abs(proj[:, 0]) < np.abs(xf).max() + m) & (np.abs(proj[:, 1]) < np.abs(yf).max() + m))[0]


def assert_exact(proj, W, H, radius):
    f = np.float32
    xf32, yf32 = OW.pix_to_ndc(W - 1 - np.arange(W), W, H), OW.pix_to_ndc(H - 1 - np.arange(H), H, W)           # fp32, as splat_pix_to_ndc
    assert xf32.dtype == f and np.array_equal(xf32.astype(np.float64), pix_ndc64(W, H)) and np.array_equal(yf32.astype(np.float64), pix_ndc64(H, W))
    p = proj[near(proj, W, H, radius)]
    dx, dy = xf32[None, :, None] - p[:, 0], yf32[:, None, None] - p[:, 1]
    d2 = dx * dx + dy * dy
    assert d2.dtype == f
    d2_64 = (xf32.astype(np.float64)[None, :, None] - p[:, 0].astype(np.float64)) ** 2 + (yf32.astype(np.float64)[:, None, None] - p[:, 1].astype(np.float64)) ** 2
    assert np.array_equal(d2.astype(np.float64), d2_64), "d2 is not exact in fp32"
    assert np.array_equal((dx * dx).astype(np.float64), (xf32.astype(np.float64)[None, :, None] - p[:, 0].astype(np.float64)) ** 2), "dx^2 rounds: FMA contraction would differ"
    r2 = f(radius) * f(radius)
    assert float(r2) == float(radius) ** 2 and not (d2 == r2).any()


@pytest.mark.parametrize("kind,key", GRID, ids=_id)
def test_grid_cases_are_exact_in_fp32(kind, key):
    c = case_of(kind, key)
    assert c.W & (c.W - 1) == 0 and c.H & (c.H - 1) == 0 and max(c.W, c.H) // min(c.W, c.H) in (1, 2, 4) and c.g == 4 * max(c.W, c.H)
    assert float(c.radius) * 2 * c.g == 2 * c.k + 1
    fin = np.isfinite(c.proj[:, :2]).all(1) & (np.abs(c.proj[:, :2]) < 1e3).all(1)
    assert np.array_equal(c.proj[fin, :2] * c.g, np.round(c.proj[fin, :2] * c.g))
    assert_exact(c.proj, c.W, c.H, c.radius)
    assert not reference(kind, key, 1).amb.any()


def test_the_second_grid_pass_case_is_exact_in_fp32():
    c = wrap_case()
    proj = project64(lift64(c.depth, c.idx[-300:], c.W0, c.H0, c.f, c.f), c.X).astype(np.float32)
    assert np.array_equal(proj[:, :2] * 128, np.round(proj[:, :2] * 128)) and (np.abs(proj[:, :2]) <= 1).all()
    assert_exact(proj, c.W, c.H, c.radius)
    far = project64(lift64(c.depth, c.idx[:-300], c.W0, c.H0, c.f, c.f), c.X)
    assert (np.abs(far[:, :2]).max(1) >= 1.25).all() and float(c.radius) + 2 * 2 / 32 < 0.25


def topk_pairs(c, ref, K):
    """ids at slots K - 1 and K (the last kept, the first cut off) of every pixel with more than K covering points"""
    xf, yf = pix_ndc64(c.W, c.H), pix_ndc64(c.H, c.W)
    p = c.proj.astype(np.float64)
    ids = near(c.proj, c.W, c.H, c.radius)
    ids = ids[np.lexsort((ids, p[ids, 2]))]
    r2 = float(c.radius) ** 2
    out = []
    for row, col in zip(*np.nonzero(ref.count > K)):
        hit = ids[(xf[col] - p[ids, 0]) ** 2 + (yf[row] - p[ids, 1]) ** 2 < r2]
        assert len(hit) == ref.count[row, col]
        out.append((hit[K - 1], hit[K]))
    return np.array(out)


@pytest.mark.parametrize("K", K_EDGES)
def test_k_boundary_case_has_the_pixels_and_rejects_one_point_more_or_fewer(K):
    c, ref = case_of("kb", "random"), reference("kb", "random", K)
    assert (ref.count < K).any() and (ref.count == K).any() and (ref.count > K).any() and ref.count.max() > 32 and (ref.count == 0).any()
    pairs = topk_pairs(c, ref, K)
    assert (c.rgb[pairs[:, 0]] != c.rgb[pairs[:, 1]]).any(1).all(), "slot K - 1 and the point cut off share a colour"
    assert (c.proj[pairs[:, 0], 2] <= c.proj[pairs[:, 1], 2]).all()
    for other in (K + 1, K - 1):
        wrong = ref_render(c.proj, c.rgb, c.W, c.H, c.radius, other)
        ratio = mismatch((wrong.image, ref.idx_sum, ref.covered), ref, K)[2]              # the image alone must give it away
        assert ratio > 1.0, (K, other, ratio)
        assert not passes(as_out(wrong), ref, K)


@pytest.mark.parametrize("z,K", [("equal", 8), ("equal", 17), ("two", 8), ("two", 17)])
def test_tie_cases_reject_the_reversed_tie_rule_and_back_to_front(z, K):
    c, ref = case_of("kb", z), reference("kb", z, K)
    assert len(np.unique(c.proj[near(c.proj, c.W, c.H, c.radius), 2])) == (1 if z == "equal" else 2)
    pairs = topk_pairs(c, ref, K)
    tied = c.proj[pairs[:, 0], 2] == c.proj[pairs[:, 1], 2]
    assert tied.sum() > 100 and (pairs[tied, 0] < pairs[tied, 1]).all(), "slot K - 1 ties with the point cut off; the smaller id stays"
    rev = ref_render(c.proj, c.rgb, c.W, c.H, c.radius, K, tie_rev=True)
    cov, ids, ratio = mismatch(as_out(rev), ref, K)
    assert cov == 0 and ids > 100 and ratio > 1.0
    b2f = ref_render(c.proj, c.rgb, c.W, c.H, c.radius, K, back_to_front=True)
    cov, ids, ratio = mismatch(as_out(b2f), ref, K)
    assert cov == 0 and ids == 0 and ratio > 1.0


@pytest.mark.parametrize("L", CHUNK_LENGTHS)
def test_chunk_cases_put_the_nearest_points_in_the_last_chunk(L):
    K = 8
    c, ref = case_of("chunk", L), reference("chunk", L, K)
    assert len(c.lst) == L and sorted(c.lst.tolist()) == list(range(L)) and c.S in c.lst[L - c.last:]
    in_last = np.isin(ref.first, c.lst[L - c.last:])
    assert ((ref.first == c.S) & (ref.count == 1)).any() and ((ref.first == c.S) & (ref.count > 1)).any() and in_last.sum() >= 4
    assert (ref.count > K).any() and (ref.count == 0).any()


def render_from_lists(c, offs, lst, K, draw_behind=False):
    """the reference restricted, tile by tile, to the points the tile's list names"""
    TW, TH = tiles_of(c.W, c.H)
    validate_lists(offs, lst, c.n, TW * TH)
    image, idx_sum, covered = np.zeros((c.H, c.W, 3)), np.zeros((c.H, c.W), np.int64), np.zeros((c.H, c.W), np.uint8)
    for t, seg in enumerate(segments(offs, lst)):
        proj = c.proj.copy()
        off = np.ones(c.n, bool)
        off[seg] = False
        proj[off, 0] = np.nan
        r = ref_render(proj, c.rgb, c.W, c.H, c.radius, K, band=c.band, draw_behind=draw_behind)
        rows, cols = slice(16 * (t // TW), 16 * (t // TW) + 16), slice(16 * (t % TW), 16 * (t % TW) + 16)
        image[rows, cols], idx_sum[rows, cols], covered[rows, cols] = r.image[rows, cols], r.idx_sum[rows, cols], r.covered[rows, cols]
    return image, idx_sum, covered


@pytest.mark.parametrize("kind,key,K", SMALL, ids=_id)
def test_hand_built_lists_are_sufficient_and_the_fp32_oracle_stays_inside_the_bounds(kind, key, K):
    c, ref = case_of(kind, key), reference(kind, key, K)
    assert ref.amb.mean() <= AMBIGUOUS_CAP
    print(f"{kind} {key}: ambiguous {int(ref.amb.sum())} of {ref.amb.size}, band / r2 = {c.b:.2e}, image bound {image_bound(K, c.b):.3g}")
    offs, lst = lists_of(kind, key)
    cov, ids, ratio = mismatch(render_from_lists(c, offs, lst, K), ref, K)
    assert cov == 0 and ids == 0 and ratio < 1e-6                        # fp64 sums over another number of candidates
    with np.errstate(all="ignore"):
        image, idx, _ = OW.splat(c.proj[:, :3], c.rgb, c.H, c.W, c.radius, K)
    out = (image, idx.sum(-1), (idx[..., 0] >= 0).astype(np.uint8))
    cov, ids, ratio = mismatch(out, ref, K, c.b)
    print(f"oracle fp32: |err| / bound = {ratio:.3f}")
    assert passes(out, ref, K, c.b), (cov, ids, ratio)


@pytest.mark.parametrize("name", list(PARTIAL))
def test_a_drawn_point_behind_the_camera_is_rejected(name):
    K = 5
    c, ref = case_of("partial", name), reference("partial", name, K)
    behind = c.rejected[c.proj[c.rejected, 2] < 0]
    assert len(behind) == 4 and np.isfinite(c.proj[behind, :2]).all()
    offs, lst = lists_of("partial", name)
    assert all(np.isin(c.rejected, s).all() for s in segments(offs, lst))
    wrong = render_from_lists(c, offs, lst, K, draw_behind=True)
    cov, ids, ratio = mismatch(wrong, ref, K)
    assert ids > 0 and ratio > 1.0 and not passes(wrong, ref, K)


def test_a_list_truncated_at_256_is_rejected():
    K = 8
    for L in (257, 513):
        c, ref = case_of("chunk", L), reference("chunk", L, K)
        offs, lst = lists_of("chunk", L)
        cut = 256 * ((L - 1) // 256)
        wrong = render_from_lists(c, np.array([0, cut], np.int32), lst, K)
        cov, ids, ratio = mismatch(wrong, ref, K)
        assert cov > 0 and ids > 0 and ratio > 1.0


def as_bin(pairs):
    """[tiles, n] bool -> counts, offs, list as the two bin passes would leave them"""
    counts = pairs.sum(1).astype(np.int32)
    offs = np.zeros(len(counts) + 1, np.int32)
    offs[1:] = np.cumsum(counts)
    lst = np.concatenate([np.nonzero(row)[0] for row in pairs] + [np.full(8, -1)]).astype(np.int32)
    return counts, offs, lst


BINS = [("bin", (W, H, e)) for W, H in BIN_SIZES for e in (False, True)] + [("partial", k) for k in PARTIAL] + [("random", k) for k in RANDOM]


@pytest.mark.parametrize("kind,key", BINS, ids=_id)
def test_bin_properties_accept_the_fp64_tile_set_and_the_fp32_tile_box(kind, key):
    c = bin_case(*key) if kind == "bin" else case_of(kind, key)
    cover = cover64(c.proj, c.W, c.H, c.radius)
    if kind == "bin" and key[2]:
        assert cover.all(0).any()
    counts, offs, lst = as_bin(cover)
    assert check_bin(c.proj, c.W, c.H, c.radius, counts, counts, offs, lst, cover, guard=-1) == cover.sum()
    box = tile_box_f32(c.proj, c.radius, c.W, c.H)
    counts, offs, lst = as_bin(box)
    total = check_bin(c.proj, c.W, c.H, c.radius, counts, counts, offs, lst, cover, guard=-1)
    print(f"{kind} {key}: {int(cover.sum())} covering pairs, the fp32 box lists {total}")
    # a bin that loses one tile of a disc over the border, one that lists a point twice, one whose fill pass disagrees with its count pass
    t, p = np.nonzero(cover)
    dropped = box.copy()
    dropped[t[0], p[0]] = False
    for bad in (as_bin(dropped), (counts, offs, np.where(np.arange(len(lst)) == 1, lst[0], lst)) if counts[0] > 1 else None):
        if bad is not None:
            with pytest.raises(AssertionError):
                check_bin(c.proj, c.W, c.H, c.radius, bad[0], bad[0], bad[1], bad[2], cover, guard=-1)
    with pytest.raises(AssertionError):
        check_bin(c.proj, c.W, c.H, c.radius, counts, counts + (np.arange(len(counts)) == 0), offs, lst, cover, guard=-1)


@pytest.mark.parametrize("name", list(PARTIAL))
def test_border_cases_hang_over_every_edge_and_a_missing_border_tile_is_rejected(name):
    c, ref = case_of("partial", name), reference("partial", name, 5)
    xf, yf = pix_ndc64(c.W, c.H), pix_ndc64(c.H, c.W)
    ex, ey = np.abs(xf).max() + abs(xf[0] - xf[1]) / 2, np.abs(yf).max() + abs(yf[0] - yf[1]) / 2            # the image's edges
    x, y = c.proj[:, 0].astype(np.float64), c.proj[:, 1].astype(np.float64)
    reaches = ref.cover.any(0)
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            if sx or sy:
                outside = (x * sx > ex if sx else np.abs(x) < ex) & (y * sy > ey if sy else np.abs(y) < ey) & (c.proj[:, 2] > 0)
                assert (outside & reaches).any(), ("no disc hangs into the image from", sx, sy)
    off = ((np.abs(x) > ex) | (np.abs(y) > ey)) & (np.abs(x) < ex + float(c.radius)) & (np.abs(y) < ey + float(c.radius)) & (c.proj[:, 2] > 0)
    assert (off & ~reaches).any(), "no disc off-screen by less than a radius that covers nothing"
    # the bin that forgets the tile of a disc hanging in from outside
    TW, TH = tiles_of(c.W, c.H)
    p = np.nonzero(reaches & ((np.abs(x) > ex) | (np.abs(y) > ey)))[0][0]
    t = np.nonzero(ref.cover[:, p])[0][0]
    assert t % TW in (0, TW - 1) or t // TW in (0, TH - 1)
    dropped = ref.cover.copy()
    dropped[t, p] = False
    counts, offs, lst = as_bin(dropped)
    with pytest.raises(AssertionError):
        check_bin(c.proj, c.W, c.H, c.radius, counts, counts, offs, lst, ref.cover, guard=-1)


def test_rim_case_needs_the_margins_of_the_tile_box():
    """discs that reach the next tile by a few ulps: the fp32 box with its margins lists every needed tile, without them it loses some -- and on every
    other bin case the margins make no difference to the superset property, which is why this case exists"""
    c = rim_case()
    cover = cover64(c.proj, c.W, c.H, c.radius)
    assert (cover.sum(0) >= 2).sum() > 200, "few discs reach a second tile"
    counts, offs, lst = as_bin(tile_box_f32(c.proj, c.radius, c.W, c.H))
    check_bin(c.proj, c.W, c.H, c.radius, counts, counts, offs, lst, cover, guard=-1)
    bare = tile_box_f32(c.proj, c.radius, c.W, c.H, margin=0)
    lost = int((cover & ~bare).sum())
    print(f"rim case: {int(cover.sum())} needed pairs, {lost} lost without the margins")
    assert lost > 0
    counts, offs, lst = as_bin(bare)
    with pytest.raises(AssertionError):
        check_bin(c.proj, c.W, c.H, c.radius, counts, counts, offs, lst, cover, guard=-1)
    for kind, key in BINS:
        o = bin_case(*key) if kind == "bin" else case_of(kind, key)
        assert not (cover64(o.proj, o.W, o.H, o.radius) & ~tile_box_f32(o.proj, o.radius, o.W, o.H, margin=0)).any(), (kind, key)
