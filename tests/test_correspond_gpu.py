"""GPU: the correspondence outputs of the point-cloud warp -- ffn_splat_ids (which points ffn_splat_render composites at a pixel) and ffn_splat_correspond (where
every source pixel went, and whether it shows there) -- through the C ABI and through warp3d.point_cloud_warp(return_correspondence=True), on the five geometries
of tests/test_warp3d_gpu.py and on an object with a depth step.  The fp64 restatement, the ambiguity rules and the bound of the map are tests/correspond_cases.py
(held to the caps on their own, without a device, by tests/test_correspond_cpu.py).  Every comparison is made on the projected points the library itself
recorded (test_splat_gpu.Recorder), so the two sides differ in the arithmetic under test only.

Tolerance of the invariants (identity / translation at constant depth, u = 2^-24, S = max(W, H)).  A target pixel is x = W - 1 - u(x_ndc), x_ndc = X' / (z' tan):
the lift rounds three times (4u |X|), q = X - c + t twice, the product with R = I once, the scale and + c once each -- each an absolute error of at most u times a
coordinate no larger than the cloud's, i.e. at most u S / 2 in pixels -- the quotient by z' tan carries the same for z' plus two roundings of its own and the
roundings of f and tan (fp32 fields): about 20 roundings of a value <= S / 2, 10 u S.  The map adds correspond_cases.map_bound <= 8 u S inside the image.
Held to 32 u S (1.2e-4 pixel at S = 64)."""
import functools
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

import correspond_cases as CC
import test_splat_gpu as S

pytestmark = pytest.mark.gpu

RENDER_CALLS = ["ffn_splat_lift", "ffn_splat_project", "ffn_splat_bin", "ffn_splat_bin", "ffn_splat_render"]


class NamedRecorder(S.Recorder):
    """test_splat_gpu.Recorder, which also keeps the order of the entries called"""

    def __init__(self, torch, lib):
        super().__init__(torch, lib)
        self.names = []

    def __getattr__(self, name):
        call = super().__getattr__(name)

        def logged(*a):
            self.names.append(name)
            return call(*a)
        return logged


def recorded(fn):
    """fn(warp3d) with the library recorded -> (result, project operands, render operands, names of the entries in call order)"""
    torch, L, lib, _ = S._dev()
    from freefine_amd import warp3d
    rec = NamedRecorder(torch, lib)
    real = warp3d.L.load
    warp3d.L.load = lambda: rec
    try:
        result = fn(warp3d)
    finally:
        warp3d.L.load = real
    return result, rec.calls["ffn_splat_project"], rec.calls["ffn_splat_render"], rec.names


def run_ids(gpu, proj, offs, lst, radius, K, W, H):
    """ffn_splat_ids into a sentinel-filled, guarded buffer -> ids int32 [H, W, K]"""
    torch, L, lib, stream = S._dev()
    S.validate_lists(offs, lst, len(proj), np.prod(S.tiles_of(W, H)))
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (proj, offs, lst)]
    _, ids, ok = S.guarded(torch, gpu, (H, W, K), torch.int32, S.SENT_I, 16 * (W + 16) * K)
    L.check(lib.ffn_splat_ids(stream, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), float(radius), K, W, H, ids.data_ptr()), "splat_ids")
    torch.cuda.synchronize()
    assert ok(), "the sentinel outside H x W x K was overwritten"
    return ids.cpu().numpy()


def run_correspond(gpu, proj, idx, W, H, ids, K, want_visible=True):
    """ffn_splat_correspond into sentinel-filled, guarded buffers -> (map f32 [H, W, 2], visible u8 [H, W] or None)"""
    torch, L, lib, stream = S._dev()
    idx = np.ascontiguousarray(idx, np.int32)
    assert idx.min() >= 0 and idx.max() < W * H and len(idx) == len(proj)
    p, i = torch.from_numpy(np.ascontiguousarray(proj)).to(gpu), torch.from_numpy(idx).to(gpu)
    _, cmap, ok0 = S.guarded(torch, gpu, (H, W, 2), torch.float32, S.SENT_F, 64)
    _, vis, ok1 = S.guarded(torch, gpu, (H, W), torch.uint8, S.SENT_B, 64)
    ids_d = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(gpu) if want_visible else None
    L.check(lib.ffn_splat_correspond(stream, p.data_ptr(), i.data_ptr(), len(idx), W, H, ids_d.data_ptr() if want_visible else None, K, cmap.data_ptr(),
                                     vis.data_ptr() if want_visible else None), "splat_correspond")
    torch.cuda.synchronize()
    assert ok0() and ok1()
    if not want_visible:
        assert (vis == S.SENT_B).all()
    return cmap.cpu().numpy(), vis.cpu().numpy() if want_visible else None


def _run(gpu, img, depth, mask, f, r, K, tf, pixel_translation=False):
    """the Python entry with the correspondence outputs, recorded; then ids and render from the library on the recorded points and the bin's own lists"""
    h, w = depth.shape
    (out, ref_mask, cov, corr, visible), pr, rd, names = recorded(
        lambda W3: W3.point_cloud_warp(img, depth, tf, f, f, mask, True, r, K, device=gpu, return_covered=True, pixel_translation=pixel_translation,
                                       return_correspondence=True))
    assert names == RENDER_CALLS + ["ffn_splat_ids", "ffn_splat_correspond"]
    keep = np.nonzero(mask.reshape(-1) > 0)[0]
    assert pr.n == len(keep) and (rd.K, rd.W, rd.H) == (K, w, h)
    counts_a, counts_b, offs, lst = S.run_bin(gpu, pr.proj, r, w, h)
    image, idx_sum, covered = S.render(gpu, pr.proj, rd.rgb, offs, lst, r, K, w, h)
    ids = run_ids(gpu, pr.proj, offs, lst, r, K, w, h)
    band = S.rim_band(w, h, r)
    ref, amb = CC.ref_ids(pr.proj, w, h, r, K, band)
    return NS(h=h, w=w, K=K, r=r, keep=keep, out=out, ref_mask=ref_mask, cov=cov, corr=corr, visible=visible, pr=pr, rd=rd, offs=offs, lst=lst, idx_sum=idx_sum,
              covered=covered, ids=ids, ref_ids=ref, amb=amb, img=img, depth=depth, mask=mask, f=f, tf=tf)


@functools.lru_cache(maxsize=None)
def device_case(gpu, i):
    """geometry i, computed once and shared (read-only) by the tests below"""
    return _run(gpu, *CC.geometry(i))


@functools.lru_cache(maxsize=None)
def device_step_case(gpu):
    return _run(gpu, *CC.step_case())


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the ids
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5))
def test_ids_are_what_render_composites(gpu, i):
    """exactly, on every pixel: the ids add up to ffn_splat_render's idx_sum (-1 per empty slot) and slot 0 is filled where render says covered -- both kernels
    run one selection routine on the same points and lists.  Shuffled lists (the bin fills them through atomics) give the same bits."""
    c = device_case(gpu, i)
    assert c.ids.dtype == np.int32 and c.ids.shape == (c.h, c.w, c.K)
    assert np.array_equal(c.ids.astype(np.int64).sum(-1), c.idx_sum.astype(np.int64))
    assert np.array_equal(c.ids[..., 0] >= 0, c.covered > 0) and c.covered.any() and not c.covered.all()
    assert ((c.ids >= -1) & (c.ids < c.pr.n)).all()
    filled = c.ids >= 0
    assert (filled[..., :-1] >= filled[..., 1:]).all(), "an empty slot before a filled one"
    rng = np.random.default_rng(i)
    o2, l2 = S.pack_lists([rng.permutation(s) for s in S.segments(c.offs, c.lst)])
    assert np.array_equal(run_ids(gpu, c.pr.proj, o2, l2, c.r, c.K, c.w, c.h), c.ids)


@pytest.mark.parametrize("i", range(5))
def test_ids_against_the_oracle(gpu, i):
    """the numpy oracle's `idx` of the same projected points, and the fp64 restatement, outside the pixels the restatement calls ambiguous"""
    from oracle import warp3d as OW
    c = device_case(gpu, i)
    print(f"CORRESPOND ids {c.h}x{c.w} K = {c.K}: ambiguous {int(c.amb.sum())} of {c.amb.size} = {c.amb.mean():.4%}")
    assert c.amb.mean() <= S.AMBIGUOUS_CAP
    _, idx_o, _ = OW.splat(c.pr.proj[:, :3], c.rd.rgb, c.h, c.w, c.r, c.K)
    sure = ~c.amb
    assert np.array_equal(c.ids[sure], idx_o[sure])
    assert np.array_equal(c.ids[sure], c.ref_ids[sure])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3: the map
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5))
def test_map_against_fp64(gpu, i):
    """object pixels: the fp64 map of the recorded projection within correspond_cases.map_bound; every other pixel: its own coordinates, exactly.  The entry
    without the visibility output (visible = NULL, ids = NULL) writes the same bits and touches no pixel `idx` does not name."""
    c = device_case(gpu, i)
    assert c.corr.dtype == np.float32 and c.corr.shape == (c.h, c.w, 2)
    want = CC.map64(c.pr.proj, c.w, c.h)
    assert np.isfinite(want).all()
    got = c.corr.reshape(-1, 2)[c.keep].astype(np.float64)
    ratio = float((np.abs(got - want) / CC.map_bound(want, c.w, c.h)).max())
    print(f"CORRESPOND map {c.h}x{c.w}: |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    obj = c.mask > 0
    assert np.array_equal(c.corr[~obj], CC.identity_map(c.h, c.w)[~obj])
    alone, none = run_correspond(gpu, c.pr.proj, c.keep, c.w, c.h, None, c.K, want_visible=False)
    assert none is None and np.array_equal(alone[obj], c.corr[obj]) and (alone[~obj] == S.SENT_F).all()
    both, vis = run_correspond(gpu, c.pr.proj, c.keep, c.w, c.h, c.ids, c.K)
    assert np.array_equal(both, alone) and np.array_equal(vis[obj] * 255, c.visible[obj]) and (vis[~obj] == S.SENT_B).all()
    assert (c.visible[~obj] == 0).all() and set(np.unique(c.visible)) <= {0, 255}


@pytest.mark.parametrize("h,w", [(64, 64), (40, 72), (72, 40)])
def test_map_invariants(gpu, h, w):
    """at f = min(H, W) / (2 tan 30 deg): identity -> (i - 1/2, j - 1/2) (the half-pixel offset between the lift and the pixel centres);
    a pixel translation of (7, 3) at constant depth -> (i + 6.5, j + 2.5); non-object pixels: identity; a cloud pushed behind the camera: NaN on the object,
    identity elsewhere, nothing visible"""
    from freefine_amd import warp3d
    import test_warp3d_gpu as T3
    img, depth, mask, f = T3._case(h, w, 3)
    r, K = 1.5 * 2.0 / min(h, w), 5
    obj = mask > 0
    ident = CC.identity_map(h, w)
    tol = 32 * S.U * max(h, w)
    _, _, corr, vis = warp3d.point_cloud_warp(img, depth, CC.IDENT, f, f, mask, True, r, K, device=gpu, return_correspondence=True)
    err = np.abs(corr - (ident - 0.5))[obj].max()
    print(f"CORRESPOND identity {h}x{w}: worst |err| = {err:.2e} (tolerance {tol:.2e})")
    assert err <= tol and np.array_equal(corr[~obj], ident[~obj])
    assert (vis[obj] == 255).all() and (vis[~obj] == 0).all(), "four points cover a pixel under the identity: each of them is among its K = 5"
    flat = np.full((h, w), 2.0, np.float32)
    _, _, corr, vis = warp3d.point_cloud_warp(img, flat, [7, 3, 0, 0, 0, 0, 1, 1, 1], f, f, mask, True, r, K, device=gpu, pixel_translation=True,
                                              return_correspondence=True)
    err = np.abs(corr - (ident + np.float32([6.5, 2.5])))[obj].max()
    print(f"CORRESPOND translation {h}x{w}: worst |err| = {err:.2e} (tolerance {tol:.2e})")
    assert err <= tol and np.array_equal(corr[~obj], ident[~obj]) and (vis[obj] == 255).all()
    # tz = -2 f pixels = twice the mean depth towards the camera: z' = z - 2 mean(z) < 0 for depths in [2, 3)
    out, _, cov, corr, vis = warp3d.point_cloud_warp(img, depth, [0, 0, -2 * f, 0, 0, 0, 1, 1, 1], f, f, mask, True, r, K, device=gpu, pixel_translation=True,
                                                     return_covered=True, return_correspondence=True)
    assert np.isnan(corr[obj]).all() and np.array_equal(corr[~obj], ident[~obj]) and (vis == 0).all() and (cov == 0).all() and (out == 0).all()
    # an empty mask: the identity everywhere, nothing visible
    e = warp3d.point_cloud_warp(img, depth, CC.IDENT, f, f, np.zeros_like(mask), True, r, K, device=gpu, return_correspondence=True)
    assert np.array_equal(e[2], ident) and (e[3] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4: visibility
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_visibility_on_a_depth_step(gpu):
    """the near half, rotated 40 degrees about y, hides part of the far half: `visible` is the fp64 restatement's outside the ambiguous points"""
    c = device_step_case(gpu)
    vis64, amb = CC.visible64(c.pr.proj, c.ref_ids, c.amb, c.w, c.h)
    print(f"CORRESPOND visible {c.h}x{c.w}: ambiguous pixels {c.amb.mean():.4%}, ambiguous points {int(amb.sum())} of {amb.size} = {amb.mean():.4%}; "
          f"visible {int(vis64.sum())}, hidden {int((~vis64).sum())}")
    assert c.amb.mean() <= S.AMBIGUOUS_CAP and amb.mean() <= S.AMBIGUOUS_CAP
    got = c.visible.reshape(-1)[c.keep]
    assert set(np.unique(got)) == {0, 255}
    sure = ~amb
    assert (vis64 & sure).any() and (~vis64 & sure).any()
    assert np.array_equal(got[sure] > 0, vis64[sure])
    assert (c.visible[c.mask == 0] == 0).all()
    # a visible point is one of the ids of the pixel it lands on, by the kernel's own outputs
    xy = c.corr.reshape(-1, 2)[c.keep]
    r_, c_ = CC.nearest_pixel(xy)
    v = np.nonzero(got > 0)[0]
    assert (c.ids[r_[v].astype(int), c_[v].astype(int)] == v[:, None]).any(-1).all()


def test_identity_makes_every_landed_point_visible(gpu):
    from freefine_amd import warp3d
    img, depth, mask, f, r, K, _ = CC.step_case()
    h, w = depth.shape
    _, _, corr, vis = warp3d.point_cloud_warp(img, depth, CC.IDENT, f, f, mask, True, r, K, device=gpu, return_correspondence=True)
    obj = mask > 0
    r_, c_ = CC.nearest_pixel(corr.reshape(-1, 2))
    inside = ((r_ >= 0) & (r_ < h) & (c_ >= 0) & (c_ < w)).reshape(h, w)
    assert inside[obj].all() and (vis[obj & inside] == 255).all() and (vis[~obj] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5: orientation, end to end through the metric
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def carried(H, W, corr, vis_obj):
    """two source pixels may round to one target pixel, which can carry one row only: the first of them in row-major order is the one whose row it carries
    -> bool [H, W], the visible object pixels whose row is in the edited image"""
    r_, c_ = CC.nearest_pixel(corr.reshape(-1, 2))
    src = np.nonzero(vis_obj.reshape(-1))[0]
    _, first = np.unique(r_[src].astype(np.int64) * W + c_[src].astype(np.int64), return_index=True)
    out = np.zeros(H * W, bool)
    out[src[first]] = True
    return out.reshape(H, W)


class MovedFeatures:
    """stands in for HipSDFeaturizer.pair at grid (H, W): random unit rows for the source; for the edited image rows that are zero except at the nearest pixel
    of corr of every visible object pixel, which carry that pixel's source row (`carried`: one row per target pixel)"""

    def __init__(self, H, W, corr, owners, gpu):
        import torch
        src = torch.randn(H * W, 32, generator=torch.Generator().manual_seed(9))
        src = src / src.norm(dim=1, keepdim=True)
        tgt = torch.zeros_like(src)
        r_, c_ = CC.nearest_pixel(corr.reshape(-1, 2))
        q = np.nonzero(owners.reshape(-1))[0]
        tgt[torch.from_numpy(r_[q].astype(np.int64) * W + c_[q].astype(np.int64))] = src[torch.from_numpy(q)]
        self.src, self.tgt, self.hw = src[None].contiguous().to(gpu), tgt[None].contiguous().to(gpu), (H, W)

    def pair(self, src, edited, prompt, **kw):
        return self.src, self.tgt, self.hw


def test_orientation_through_the_metric(gpu, tmp_path):
    """64 x 64, 15 degrees about z plus a translation of (5, -4) pixels.  The map goes to disk through save_correspondence, is found by the path rule of
    calculate_md and read by mean_distance; every keypoint's match (the pixel its feature really moved to) lies within sqrt(1/2) of the map's target -- the
    rounding of a target to a pixel.  (Keypoints are sampled among the visible pixels whose row the edited image carries: with every visible pixel, two of 30
    keypoints shared a target pixel, which holds one row, and the other matched 22.7 pixels away -- the stub's collision, not the map's error.)  x and y, or rows and columns, swapped anywhere in the chain move the targets by pixels.  The metric is handed a neutral
    edit_param: with a translation in x / y or a rotation about z in it, the reference's rule takes the 2-D branches and never opens the file."""
    from freefine_amd import geobench, metrics as FM, warp3d
    import test_warp3d_gpu as T3
    H = W = 64
    img, depth, mask, f = T3._case(H, W, 11)
    tf = [5, -4, 0, 0, 0, 15, 1, 1, 1]
    out, _, corr, visible = warp3d.point_cloud_warp(img, depth, tf, f, f, mask, True, 1.5 * 2.0 / W, 5, device=gpu, pixel_translation=True,
                                                    return_correspondence=True)
    root = str(tmp_path / "Geo-Bench-3D")
    path, _ = warp3d.save_correspondence(root, "0001", "0", "0", corr, visible)
    gen = os.path.join(str(tmp_path), geobench.VARIANTS["3d_rgb"]["gen_subdir"], "0001", "0", "0.png")
    assert FM.correspondence_path(gen) == path and os.path.exists(path)
    vis_obj = (mask > 0) & (visible > 0)
    owners = carried(H, W, corr, vis_obj)
    assert 0.5 * vis_obj.sum() < owners.sum() <= vis_obj.sum()
    kps = FM.default_keypoints(owners.astype(np.float64), 30)            # the default sampler over the visible pixels whose feature is in the edited image
    assert len(kps) >= 20
    feat = MovedFeatures(H, W, corr, owners, gpu)
    neutral = [0, 0, 0, 0, 0, 0, 1, 1, 1]
    d = FM.mean_distance(feat, img, out, mask, neutral, "x", kps, FM.correspondence_path(gen))
    print(f"CORRESPOND orientation: {len(d)} keypoints, worst distance {max(d):.4f}")
    assert len(d) == len(kps) and max(d) <= math.sqrt(0.5) + 1e-3
    # the same with x and y swapped on disk: the targets are elsewhere
    np.save(os.path.join(str(tmp_path), "swapped.npy"), corr[..., ::-1])
    bad = FM.mean_distance(feat, img, out, mask, neutral, "x", kps, os.path.join(str(tmp_path), "swapped.npy"))
    assert max(bad) > 4.0 and float(np.mean(bad)) > 2.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 6: repeatability and the default path
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_repeatable_and_the_default_path_is_unchanged(gpu):
    """two runs: bit-identical ids (the bin runs again: its lists come in another order), corr, visible.  return_correspondence = False issues exactly the five
    calls it issued before, returns the same bits as a second call and as the first outputs of the call that asks for the map, and holds against the oracle's
    splat of the same points outside the ambiguous pixels as tests/test_warp3d_gpu.py holds it."""
    from oracle import warp3d as OW
    i = 1
    c = device_case(gpu, i)
    again = _run(gpu, *CC.geometry(i))
    for a, b in ((c.ids, again.ids), (c.corr, again.corr), (c.visible, again.visible), (c.pr.proj, again.pr.proj)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    img, depth, mask, f, r, K, tf = CC.geometry(i)
    res, pr, rd, names = recorded(lambda W3: W3.point_cloud_warp(img, depth, tf, f, f, mask, True, r, K, device=gpu))
    assert names == RENDER_CALLS and len(res) == 2
    res3, _, _, names3 = recorded(lambda W3: W3.point_cloud_warp(img, depth, tf, f, f, mask, True, r, K, device=gpu, return_covered=True))
    assert names3 == RENDER_CALLS and len(res3) == 3
    assert np.array_equal(res[0], res3[0]) and np.array_equal(res[1], res3[1])
    assert np.array_equal(res3[0], c.out) and np.array_equal(res3[1], c.ref_mask) and np.array_equal(res3[2], c.cov)
    assert np.array_equal(pr.proj.view(np.uint8), c.pr.proj.view(np.uint8))
    image_o, idx_o, _ = OW.splat(pr.proj[:, :3], rd.rgb, c.h, c.w, r, K)
    sure = ~c.amb
    assert np.array_equal(res3[2][sure], ((idx_o[..., 0] >= 0) * 255)[sure]) and (res3[1] == 255).all()
    assert np.abs(res3[0].astype(int) - image_o.astype(np.uint8).astype(int)).max(-1)[sure].max() <= 1
    # coarse_edit_3d: today's pair, or the pair followed by the map of the same warp
    from freefine_amd import warp3d
    bg = np.random.default_rng(2).integers(0, 256, img.shape, dtype=np.uint8)
    two = warp3d.coarse_edit_3d(img, mask, depth, [6, -3, 2, 10, 25, -15, 1, 1, 1], bg, focal_length=f, device=gpu)
    four = warp3d.coarse_edit_3d(img, mask, depth, [6, -3, 2, 10, 25, -15, 1, 1, 1], bg, focal_length=f, device=gpu, return_correspondence=True)
    assert len(two) == 2 and len(four) == 4 and np.array_equal(two[0], four[0]) and np.array_equal(two[1], four[1])
    assert four[2].shape == (c.h, c.w, 2) and four[2].dtype == np.float32 and four[3].shape == (c.h, c.w) and four[3].dtype == np.uint8
    landed = four[3] > 0
    r_, c_ = CC.nearest_pixel(four[2].reshape(-1, 2))
    assert landed.any() and (four[1][r_.reshape(c.h, c.w)[landed].astype(int), c_.reshape(c.h, c.w)[landed].astype(int)] == 255).all(), \
        "a visible point lands on a pixel of the target mask"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the drivers: geobench.run(variant="3d_rgb", save_correspondence=True) and geobench.prepare_3d, with the real depth network and warp
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class NoEdit:
    """stands in for the pipeline: the "edit" hands the coarse input back, and checks that the maps never reach it as inputs"""
    EDIT_KEYS = {"draw_mask", "use_auto_draw", "reduce_inp_artifacts", "cons_area"}

    def __init__(self):
        self.seen = 0

    def FreeFine_generation(self, ori_img, ori_mask, coarse_input, target_mask, text, gs, eta, **kw):
        assert not {"correspondence", "correspondence_visible"} & set(kw) and self.EDIT_KEYS <= set(kw)
        self.seen += 1
        return coarse_input

    def FreeFine_generation_batch(self, inputs, gs, eta, **kw):
        assert all(not {"correspondence", "correspondence_visible"} & set(i) for i in inputs)
        self.seen += len(inputs)
        return [i["coarse_input"] for i in inputs]


def test_drivers_write_the_map_where_the_metric_looks(gpu, tmp_path):
    """three cases of a synthetic GeoBenchMeta tree through geobench.run (a batch of two, then one): every case's map lies at the path calculate_md derives
    from its gen_img_path, is the map of THAT case's warp (coarse_edit_3d on the same inputs gives the same bits), and the visibility image lies beside it;
    without the flag neither tree appears.  prepare_3d writes the same maps, and coarse image and target mask of the same warp."""
    import torch
    from PIL import Image
    from freefine_amd import depth as FDp, geobench, metrics as FM
    dcfg = FDp.depth_config("tiny")
    dmodel = FDp.HipDepthAnything(dcfg, FDp.synthetic_state(dcfg, seed=3), dtype=torch.float32, device=gpu)
    size = 96
    root = str(tmp_path / "meta")
    geobench.make_synthetic_dataset(root, n_images=1, edits_per_image=3, size=size, seed=8, with_3d=True)
    model = NoEdit()
    res = geobench.run(model, root, batch=2, dsize=(size, size), verbose=False, variant="3d_rgb", depth_model=dmodel, save_correspondence=True)
    assert len(res) == 3 and model.seen == 3
    d3 = os.path.join(root, "Geo-Bench-3D")
    for r in res:
        assert "correspondence" not in r and "correspondence_visible" not in r
        path = FM.correspondence_path(r["gen_img_path"])
        assert path == os.path.join(d3, "correspondence", r["da_n"], r["ins_id"], r["edit_ins"] + ".npy") and os.path.exists(path)
        corr = np.load(path)
        vis = np.array(Image.open(os.path.join(d3, "correspondence_visible", r["da_n"], r["ins_id"], r["edit_ins"] + ".png")))
        want = geobench.finish_case_3d_rgb(geobench.read_case_3d_rgb(r, root, (size, size)), dmodel, correspondence=True)
        assert corr.shape == (size, size, 2) and np.array_equal(corr, want["correspondence"], equal_nan=True)
        assert np.array_equal(vis, want["correspondence_visible"]) and vis.any()
        assert np.array_equal(np.array(Image.open(r["gen_img_path"])), want["coarse_input"])
        obj = (want["ori_mask"] if want["ori_mask"].ndim == 2 else want["ori_mask"][:, :, 0]) > 0
        assert np.array_equal(corr[~obj], CC.identity_map(size, size)[~obj]) and not np.array_equal(corr[obj], CC.identity_map(size, size)[obj])
        assert FM.transform_coordinates([0, 0, 0, 0, 20, 0, 1, 1, 1], (size, size), obj, path).shape == (size, size, 2)
    root2 = str(tmp_path / "meta2")
    geobench.make_synthetic_dataset(root2, n_images=1, edits_per_image=3, size=size, seed=8, with_3d=True)
    res2 = geobench.run(NoEdit(), root2, batch=2, dsize=(size, size), verbose=False, variant="3d_rgb", depth_model=dmodel)
    assert len(res2) == 3 and not os.path.exists(os.path.join(root2, "Geo-Bench-3D", "correspondence"))
    assert not os.path.exists(os.path.join(root2, "Geo-Bench-3D", "correspondence_visible"))
    done = geobench.prepare_3d(root2, dmodel, dsize=(size, size), verbose=False)
    assert len(done) == 3
    for r, p in zip(res, done):
        assert np.array_equal(np.load(p["correspondence_path"]), np.load(FM.correspondence_path(r["gen_img_path"])), equal_nan=True)
        assert np.array_equal(np.array(Image.open(p["coarse_input_path"])), np.array(Image.open(r["gen_img_path"])))
        mesh = np.array(Image.open(p["target_mask_path"]))
        assert mesh.shape == (size, size) and set(np.unique(mesh)) == {0, 255}
