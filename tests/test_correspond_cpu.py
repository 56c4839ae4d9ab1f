"""CPU: the host side of the correspondence maps of the 3-D coarse edit -- the ABI entries ffn_splat_ids / ffn_splat_correspond (declared, bound, refusals
before any launch), warp3d.save_correspondence -> metrics.transform_coordinates, the path rule of metrics.calculate_md, the new refusals and filters of
metrics.mean_distance, geobench.prepare_3d on a synthetic GeoBenchMeta tree -- and the fp64 restatement of tests/correspond_cases.py on its own: it stays under
the ambiguity caps on every case of tests/test_correspond_gpu.py, agrees with the numpy oracle outside the ambiguous pixels, and the fp32 arithmetic of the map
stays inside the derived bound.  The kernels themselves: tests/test_correspond_gpu.py."""
import os
import re

import numpy as np
import pytest

import correspond_cases as CC
import test_splat_gpu as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ffn_splat_ids", "ffn_splat_correspond")
EINVAL = -22


def test_entries_are_declared_bound_and_exported():
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    declared = set(re.findall(r"\b(ffn_[a-z0-9_]+)\s*\(", header))
    for name in ENTRIES:
        assert name in declared and name in _lib.SYMBOLS, name
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfreefine_hip.so not built")
    lib = _lib.load()
    assert lib.ffn_version() >= 10
    for name in ENTRIES:
        assert hasattr(lib, name)


def test_bad_arguments_are_refused_before_any_launch():
    """no GPU needed: validation comes first.  Null required pointers, n < 0, W / H <= 0, K outside the 1 .. 32 of ffn_splat_render, a non-positive radius, a
    visibility output without the ids it is read from; and what is allowed: visible = NULL with ids = NULL, n = 0 (a no-op, nothing launched)."""
    from freefine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfreefine_hip.so not built")
    lib = _lib.load()
    p = 0x10000                                                   # never dereferenced

    def ids(proj=p, offs=p, lst=p, radius=0.1, K=5, W=8, H=8, out=p):
        return lib.ffn_splat_ids(None, proj, offs, lst, radius, K, W, H, out)

    def corr(proj=p, idx=p, n=4, W=8, H=8, ids_=p, K=5, out=p, vis=p):
        return lib.ffn_splat_correspond(None, proj, idx, n, W, H, ids_, K, out, vis)

    for kw in (dict(proj=None), dict(offs=None), dict(lst=None), dict(out=None)):
        assert ids(**kw) == EINVAL and lib.ffn_last_error().startswith(b"splat_ids: null operand"), kw
    for K in (0, -1, 33):
        assert ids(K=K) == EINVAL and f"K={K} ".encode() in lib.ffn_last_error()
    for kw in (dict(W=0), dict(H=0), dict(W=-8), dict(H=-1), dict(radius=0.0), dict(radius=-0.1)):
        assert ids(**kw) == EINVAL and b"bad shape / radius" in lib.ffn_last_error(), kw
    for kw in (dict(proj=None), dict(idx=None), dict(out=None)):
        assert corr(**kw) == EINVAL and lib.ffn_last_error().startswith(b"splat_correspond: null operand"), kw
    assert corr(ids_=None) == EINVAL and b"needs the ids" in lib.ffn_last_error()
    for kw in (dict(n=-1), dict(W=0), dict(H=0), dict(W=-8), dict(H=-1), dict(W=1 << 16, H=1 << 15)):
        assert corr(**kw) == EINVAL and b"bad shape" in lib.ffn_last_error(), kw
    for K in (0, -1, 33):
        assert corr(K=K) == EINVAL and f"K={K} ".encode() in lib.ffn_last_error()
        assert corr(K=K, ids_=None, vis=None) == EINVAL
    # n = 0 launches nothing (these pointers could not be read), with and without the visibility output
    assert corr(n=0) == 0 and corr(n=0, ids_=None, vis=None) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the fp64 restatement on its own
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5))
def test_ids_restatement_stays_under_the_cap_and_agrees_with_the_oracle(i):
    """on the oracle's own fp32 projection of every geometry: ambiguous pixels <= test_splat_gpu.AMBIGUOUS_CAP; outside them the ids are the oracle splat's;
    their sum and first slot are idx_sum and covered of test_splat_gpu.ref_render (what the device test compares the kernel's with)"""
    from oracle import warp3d as OW
    img, depth, mask, f, r, K, tf = CC.geometry(i)
    h, w = depth.shape
    proj, keep = CC.oracle_proj(depth, mask, f, tf)
    band = S.rim_band(w, h, r)
    ids, amb = CC.ref_ids(proj, w, h, r, K, band)
    print(f"CORRESPOND ids {h}x{w} K = {K}: ambiguous {int(amb.sum())} of {amb.size} = {amb.mean():.4%}")
    assert amb.mean() <= S.AMBIGUOUS_CAP
    _, idx_o, _ = OW.splat(proj[:, :3], np.zeros((len(proj), 3), np.float32), h, w, r, K)
    assert np.array_equal(ids[~amb], idx_o[~amb]) and (ids >= 0).any() and (ids < 0).any()
    ref = S.ref_render(proj, np.zeros((len(proj), 3)), w, h, r, K, band=band)
    assert np.array_equal(ids.sum(-1), ref.idx_sum) and np.array_equal(ids[..., 0] >= 0, ref.covered > 0)
    # compositing order: depths ascend along the slots, ids ascend where depths tie
    z = np.where(ids >= 0, proj[np.maximum(ids, 0), 2].astype(np.float64), np.inf)
    assert (z[..., 1:] >= z[..., :-1]).all()
    tie = (z[..., 1:] == z[..., :-1]) & (ids[..., 1:] >= 0)
    assert (np.diff(ids, axis=-1)[tie] > 0).all()


@pytest.mark.parametrize("i", range(5))
def test_map_arithmetic_stays_inside_the_bound(i):
    """the kernel's formula in numpy fp32 against fp64, on the oracle's projection and on the same points pushed far outside the image"""
    img, depth, mask, f, r, K, tf = CC.geometry(i)
    h, w = depth.shape
    proj, _ = CC.oracle_proj(depth, mask, f, tf)
    far = proj.copy()
    far[:, :2] *= np.float32(37.3)
    worst = 0.0
    for pr in (proj, far):
        want = CC.map64(pr, w, h)
        err = np.abs(CC.map_f32(pr, w, h).astype(np.float64) - want)
        worst = max(worst, float((err / CC.map_bound(want, w, h)).max()))
    print(f"CORRESPOND map {h}x{w}: |err| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_map_of_points_on_pixel_centres_and_of_rejected_points():
    """a point drawn exactly on a pixel centre maps to that pixel's integer coordinates (square and non-square NDC ranges, fp64 exactly and the fp32
    arithmetic within the bound); the points no stage may draw have no target"""
    for W, H in ((32, 32), (40, 72), (72, 40)):
        xf, yf = S.pix_ndc64(W, H), S.pix_ndc64(H, W)
        cols, rows = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
        proj = np.stack([xf[cols.ravel()], yf[rows.ravel()], np.full(W * H, 1.5), np.zeros(W * H)], 1)
        want = np.stack([cols.ravel(), rows.ravel()], 1).astype(np.float64)
        assert np.abs(CC.map64(proj, W, H) - want).max() <= 1e-11
        p32 = proj.astype(np.float32)                             # the centres themselves round: compare with fp64 of the fp32 points
        w32 = CC.map64(p32, W, H)
        assert (np.abs(CC.map_f32(p32, W, H) - w32) <= CC.map_bound(w32, W, H)).all()
        assert np.abs(w32 - want).max() <= 4 * S.U * max(W, H)
        rej = S.rejected_points(W, H)
        assert np.isnan(CC.map64(rej, W, H)).all() and np.isnan(CC.map_f32(rej, W, H)).all()


def test_visibility_restatement_on_the_depth_step():
    """the near half hides part of the far half: both values occur, ambiguous points and pixels stay under the cap; under the identity transform every point
    whose target is inside the image is visible"""
    img, depth, mask, f, r, K, tf = CC.step_case()
    h, w = depth.shape
    band = S.rim_band(w, h, r)
    proj, keep = CC.oracle_proj(depth, mask, f, tf)
    ids, amb_pix = CC.ref_ids(proj, w, h, r, K, band)
    vis, amb = CC.visible64(proj, ids, amb_pix, w, h)
    print(f"CORRESPOND visible {h}x{w}: ambiguous pixels {amb_pix.mean():.4%}, ambiguous points {int(amb.sum())} of {amb.size} = {amb.mean():.4%}; "
          f"visible {int(vis.sum())}, hidden {int((~vis).sum())}")
    assert amb_pix.mean() <= S.AMBIGUOUS_CAP and amb.mean() <= S.AMBIGUOUS_CAP
    assert (vis & ~amb).sum() > 50 and (~vis & ~amb).sum() > 50
    # the far half (depth 3) loses points behind the near half: a hidden far point whose nearest pixel shows a near point first
    near = depth.reshape(-1)[keep] == 2.0
    r_, c_ = CC.nearest_pixel(CC.map64(proj, w, h))
    inside = (r_ >= 0) & (r_ < h) & (c_ >= 0) & (c_ < w)
    hidden_far = np.nonzero(inside & ~near & ~vis & ~amb)[0]
    first = ids[r_[hidden_far].astype(int), c_[hidden_far].astype(int), 0]
    assert near[first].sum() > 10, "no far point is hidden by a near one"
    # identity: the targets sit half-way between two pixels (x + 1/2 is an integer up to rounding), but no pixel is covered by more than four points, so
    # with K = 5 every covering point is listed and the point is visible whichever neighbour is taken
    proj0, _ = CC.oracle_proj(depth, mask, f, CC.IDENT)
    ids0, _ = CC.ref_ids(proj0, w, h, r, K, band)
    r0, c0 = CC.nearest_pixel(CC.map64(proj0, w, h))
    assert ((r0 >= 0) & (r0 < h) & (c0 >= 0) & (c0 < w)).all() and (ids0 >= 0).sum(-1).max() == 4 and K == 5


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# files and the metric
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_save_correspondence_round_trip_and_the_path_rule(tmp_path):
    """(x, y) on disk -- the reference's order -- and (row, col) out of transform_coordinates; the path calculate_md derives from a 3d_rgb result path is the
    path written; the visibility image lies beside it"""
    from PIL import Image
    from freefine_amd import geobench, metrics as FM, warp3d
    H, W = 6, 9
    rng = np.random.default_rng(3)
    corr = rng.uniform(-2, 12, (H, W, 2)).astype(np.float32)
    corr[2, 3] = np.nan
    visible = (rng.random((H, W)) < 0.5).astype(np.uint8) * 255
    root = str(tmp_path / "Geo-Bench-3D")
    path, vis_path = warp3d.save_correspondence(root, "0007", 2, "1", corr, visible)
    assert path == os.path.join(root, "correspondence", "0007", "2", "1.npy") and vis_path == os.path.join(root, "correspondence_visible", "0007", "2", "1.png")
    on_disk = np.load(path)
    assert on_disk.dtype == np.float32 and on_disk.shape == (H, W, 2) and np.array_equal(on_disk, corr, equal_nan=True)
    assert np.array_equal(np.array(Image.open(vis_path)), visible)
    got = FM.transform_coordinates([0, 0, 0, 0, 30, 0, 1, 1, 1], (H, W), np.ones((H, W)), path)
    assert got.shape == (H, W, 2) and np.array_equal(got[..., 0], corr[..., 1], equal_nan=True) and np.array_equal(got[..., 1], corr[..., 0], equal_nan=True)
    gen = os.path.join(str(tmp_path), geobench.VARIANTS["3d_rgb"]["gen_subdir"], "0007", "2", "1.png")
    assert gen.split("/")[-4] == "Gen_results_FreeFine_depth_rgb" and FM.correspondence_path(gen) == path
    assert warp3d.save_correspondence(root, "0007", 2, "2", corr) == (os.path.join(root, "correspondence", "0007", "2", "2.npy"), None)
    assert not os.path.exists(os.path.join(root, "correspondence_visible", "0007", "2", "2.png"))
    with pytest.raises(ValueError):
        warp3d.save_correspondence(root, "0007", 2, "3", corr[..., 0])
    with pytest.raises(ValueError):
        warp3d.save_correspondence(root, "0007", 2, "3", corr, visible[:-1])


class OneHot:
    """stands in for HipSDFeaturizer.pair: the source feature of pixel q is the q-th unit vector; the edited image carries source pixel q's feature at
    pixel `where[q]` (flat), so the arg-max below finds exactly that pixel"""

    def __init__(self, H, W, where):
        self.H, self.W, self.asked = H, W, 0
        self.src = np.eye(H * W, dtype=np.float32)[None]
        self.tgt = np.zeros((1, H * W, H * W), np.float32)
        for q, t in enumerate(where):
            self.tgt[0, t, q] = 1.0

    def pair(self, src, edited, prompt, **kw):
        self.asked += 1
        return self.src, self.tgt, (self.H, self.W)


class HostMatch:
    """ops.dift_match as a numpy arg-max (features at image resolution: no upsampling); remembers the keypoints it was asked for"""

    def __init__(self):
        self.kps = []

    def __call__(self, rows_s, rows_t, hw, HW, kps):
        import torch
        assert tuple(hw) == tuple(HW)
        kps = np.asarray(kps).reshape(-1, 2)
        self.kps.append(kps.copy())
        flat = kps[:, 0] * HW[1] + kps[:, 1]
        best = np.argmax(rows_s[0][flat] @ rows_t[0].T, -1)
        rc = np.stack([best // HW[1], best % HW[1]], 1).astype(np.int32)
        return torch.from_numpy(rc), torch.ones(len(kps))


def _md_case(tmp_path, H=10, W=12):
    """a map that sends pixel (row, col) to (row + 1, col + 2); the features really moved that way"""
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    corr = np.stack([cols + 2.0, rows + 1.0], -1).astype(np.float32)                # (x, y)
    where = (np.clip(rows + 1, 0, H - 1) * W + np.clip(cols + 2, 0, W - 1)).ravel()
    img = np.zeros((H, W, 3), np.uint8)
    mask = np.zeros((H, W), np.uint8)
    mask[2:7, 2:8] = 255
    return corr, where, img, mask


def test_mean_distance_refuses_a_map_of_another_size(tmp_path, monkeypatch):
    from freefine_amd import metrics as FM, ops
    monkeypatch.setattr(ops, "dift_match", HostMatch())
    corr, where, img, mask = _md_case(tmp_path)
    H, W = mask.shape
    tf = [0, 0, 0, 0, 30, 0, 1, 1, 1]
    kps = [[3, 3], [4, 5]]
    for shape in ((W, H, 2), (H, W + 1, 2), (H - 1, W, 2)):
        np.save(tmp_path / "bad.npy", np.zeros(shape, np.float32))
        with pytest.raises(ValueError) as e:
            FM.mean_distance(OneHot(H, W, where), img, img, mask, tf, "x", kps, str(tmp_path / "bad.npy"))
        assert f"{shape[0]} x {shape[1]}" in str(e.value) and f"{H} x {W}" in str(e.value)
    np.save(tmp_path / "bad.npy", np.zeros((H, W, 3), np.float32))
    with pytest.raises(ValueError):
        FM.transform_coordinates(tf, (H, W), mask, str(tmp_path / "bad.npy"))
    np.save(tmp_path / "good.npy", corr)
    assert FM.mean_distance(OneHot(H, W, where), img, img, mask, tf, "x", kps, str(tmp_path / "good.npy")) == [0.0, 0.0]
    # (x, y) swapped on disk: the metric reports it
    np.save(tmp_path / "swapped.npy", corr[..., ::-1])
    assert FM.mean_distance(OneHot(H, W, where), img, img, mask, tf, "x", kps, str(tmp_path / "swapped.npy")) != [0.0, 0.0]


def test_non_finite_targets_and_hidden_keypoints_are_dropped(tmp_path, monkeypatch):
    """keypoints whose target is NaN / inf leave (after the max_points cut: the cut is the reference's), hidden keypoints leave BEFORE it; calculate_md reads the
    visibility image only when asked to and only where it exists"""
    from PIL import Image
    from freefine_amd import metrics as FM, ops, warp3d
    match = HostMatch()
    monkeypatch.setattr(ops, "dift_match", match)
    corr, where, img, mask = _md_case(tmp_path)
    H, W = mask.shape
    tf = [0, 0, 0, 0, 30, 0, 1, 1, 1]
    corr[3, 3] = np.nan
    corr[4, 5, 0] = np.inf
    root = str(tmp_path / "Geo-Bench-3D")
    visible = np.full((H, W), 255, np.uint8)
    visible[2, 2:8] = 0                                            # the first row of the object is hidden
    path, vis_path = warp3d.save_correspondence(root, "a", "0", "0", corr, visible)
    kps = [[3, 3], [2, 4], [4, 5], [5, 6], [6, 7]]
    feat = OneHot(H, W, where)
    assert FM.mean_distance(feat, img, img, mask, tf, "x", kps, path) == [0.0, 0.0, 0.0]
    assert match.kps[-1].tolist() == [[2, 4], [5, 6], [6, 7]]
    assert FM.mean_distance(feat, img, img, mask, tf, "x", kps, path, visible=visible) == [0.0, 0.0]
    assert match.kps[-1].tolist() == [[5, 6], [6, 7]]
    # the order of the two filters and the cut: max_points = 2 keeps [3, 3], [2, 4] (one of them finite) without the image, [3, 3], [4, 5] (none) with it
    assert FM.mean_distance(feat, img, img, mask, tf, "x", kps, path, max_points=2) == [0.0] and match.kps[-1].tolist() == [[2, 4]]
    asked = feat.asked
    assert FM.mean_distance(feat, img, img, mask, tf, "x", kps, path, max_points=2, visible=visible) == [] and feat.asked == asked
    with pytest.raises(ValueError):
        FM.mean_distance(feat, img, img, mask, tf, "x", kps, path, visible=visible[:-1])
    # calculate_md: a featurizer is accepted as it is only if it is a HipSDFeaturizer
    from freefine_amd import dift

    class Feat(dift.HipSDFeaturizer, OneHot):
        def __init__(self, *a):
            OneHot.__init__(self, *a)

        pair = OneHot.pair
    gen = os.path.join(str(tmp_path), "Geo-Bench-3D", "Gen_results_FreeFine_depth_rgb", "a", "0", "0.png")
    os.makedirs(os.path.dirname(gen))
    Image.fromarray(img).save(gen)
    Image.fromarray(img).save(tmp_path / "src.png")
    Image.fromarray(mask).save(tmp_path / "mask.png")
    sample = dict(ori_img_path=str(tmp_path / "src.png"), gen=gen, ori_mask_path=str(tmp_path / "mask.png"), edit_param=tf, obj_label="x")
    data = {"a": {"instances": {"0": {"0": sample}}}}
    obj = np.argwhere(mask > 0)
    finite = [k.tolist() for k in obj if np.isfinite(corr[k[0], k[1]]).all()]
    assert FM.calculate_md(data, "gen", Feat(H, W, where)) == 0.0 and match.kps[-1].tolist() == finite
    assert FM.calculate_md(data, "gen", Feat(H, W, where), visible_only=True) == 0.0
    assert match.kps[-1].tolist() == [k for k in finite if k[0] != 2]
    os.remove(vis_path)                                            # no image: every keypoint stays
    assert FM.calculate_md(data, "gen", Feat(H, W, where), visible_only=True) == 0.0 and match.kps[-1].tolist() == finite


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# step 2 of the 3-D run
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_prepare_3d_writes_the_three_trees_skips_existing_files_and_shards(tmp_path, monkeypatch):
    from PIL import Image
    from freefine_amd import geobench, warp3d
    root = str(tmp_path / "meta")
    size = 32
    data = geobench.make_synthetic_dataset(root, n_images=3, edits_per_image=2, size=size, seed=5, with_3d=True)
    calls = []

    def fake_edit(ori_img, ori_mask, depth, transforms, background, focal_length=550.0, return_correspondence=False, **kw):
        calls.append((tuple(transforms), focal_length))
        assert return_correspondence and ori_mask.ndim == 2 and depth.shape == ori_mask.shape
        tgt = np.roll((ori_mask > 0).astype(np.uint8) * 255, 1, axis=1)
        corr = CC.identity_map(*ori_mask.shape) + np.float32(transforms[0])
        return np.where(tgt[..., None] > 0, ori_img, background), tgt, corr, (ori_mask > 0).astype(np.uint8) * 255

    monkeypatch.setattr(warp3d, "coarse_edit_3d", fake_edit)
    monkeypatch.setattr(geobench, "monocular_depth", lambda img, model, **kw: np.full(img.shape[:2], 2.0, np.float32))
    keys = [f"{da}/{ins}/{e}" for da, v in data.items() for ins, edits in v["instances"].items() for e in edits]
    assert len(keys) == 6
    d3 = os.path.join(root, "Geo-Bench-3D")
    trees = [("coarse3d_depth_anything_rgb", ".png"), ("mesh_mask", ".png"), ("correspondence", ".npy"), ("correspondence_visible", ".png")]
    # two ranks split the cases between them
    a = geobench.prepare_3d(root, object(), rank=0, world=2, dsize=(size, size), verbose=False)
    assert sorted(x["key"] for x in a) == sorted(keys[0::2]) and len(calls) == 3
    for k in keys:
        for tree, ext in trees:
            assert os.path.exists(os.path.join(d3, tree, k + ext)) == (k in keys[0::2]), (k, tree)
    b = geobench.prepare_3d(root, object(), rank=1, world=2, dsize=(size, size), verbose=False)
    assert sorted(x["key"] for x in b) == sorted(keys[1::2]) and len(calls) == 6
    k = keys[0]
    da, ins, e = k.split("/")
    ep = data[da]["instances"][ins][e]["edit_param"]
    corr = np.load(os.path.join(d3, "correspondence", k + ".npy"))
    assert corr.shape == (size, size, 2) and corr.dtype == np.float32 and np.array_equal(corr, CC.identity_map(size, size) + np.float32(ep[0] * size / 512.0))
    mesh = np.array(Image.open(os.path.join(d3, "mesh_mask", k + ".png")))
    assert mesh.shape == (size, size) and set(np.unique(mesh)) == {0, 255}
    assert np.array(Image.open(os.path.join(d3, "coarse3d_depth_anything_rgb", k + ".png"))).shape == (size, size, 3)
    assert a[0]["correspondence_path"] == os.path.join(d3, "correspondence", k + ".npy")
    # everything exists: nothing is rendered again; one file gone: that case alone; check_exist off: all of them
    assert geobench.prepare_3d(root, object(), dsize=(size, size), verbose=False) == [] and len(calls) == 6
    os.remove(os.path.join(d3, "mesh_mask", keys[3] + ".png"))
    again = geobench.prepare_3d(root, object(), dsize=(size, size), verbose=False)
    assert [x["key"] for x in again] == [keys[3]] and len(calls) == 7
    assert len(geobench.prepare_3d(root, object(), dsize=(size, size), check_exist=False, verbose=False)) == 6 and len(calls) == 13
    # the reference's step name imports the same function
    from evaluation.FreeFine.get_3d_transform_correspondence import prepare_3d
    assert prepare_3d is geobench.prepare_3d


def test_finish_case_3d_rgb_keeps_todays_keys_unless_asked(monkeypatch):
    from freefine_amd import geobench, warp3d
    H = W = 32
    rng = np.random.default_rng(0)
    mask = np.zeros((H, W), np.uint8)
    mask[8:20, 8:20] = 255
    raw = dict(_raw_3d_rgb=True, _resized=True, ori_img=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), ori_mask=mask,
               bg=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), edit_param=[4.0, 0, 0, 0, 10.0, 0, 1, 1, 1], obj_label="a cup", dsize=(W, H))
    seen = []

    def fake_edit(ori_img, ori_mask, depth, transforms, background, focal_length=550.0, **kw):
        seen.append(kw)
        out = (background, (ori_mask > 0).astype(np.uint8) * 255)
        return out + (CC.identity_map(H, W), out[1]) if kw.get("return_correspondence") else out

    monkeypatch.setattr(warp3d, "coarse_edit_3d", fake_edit)
    monkeypatch.setattr(geobench, "monocular_depth", lambda img, model, **kw: np.full(img.shape[:2], 2.0, np.float32))
    today = {"ori_img", "ori_mask", "coarse_input", "target_mask", "guidance_text", "draw_mask", "use_auto_draw", "reduce_inp_artifacts", "cons_area"}
    off = geobench.finish_case_3d_rgb(dict(raw), object())
    assert set(off) == today and seen[-1] == {}, "the default call passes no new keyword"
    on = geobench.finish_case_3d_rgb(dict(raw), object(), correspondence=True)
    assert set(on) == today | {"correspondence", "correspondence_visible"} and on["correspondence"].shape == (H, W, 2)
    with pytest.raises(ValueError):
        geobench.run(None, "/nonexistent", variant="3d_depth", save_correspondence=True)
