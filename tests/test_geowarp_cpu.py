"""CPU: the GeoDiffuser warp (step 2 of the reference's GeoBench-3D preparation).  The numpy restatement tests/geowarp_ref.py is held to the reference's own
coordinates, pose and faces (tests/golden/g18_geodiffuser_coords.npz, written by tools/gen_golden.py run_g18) and to invariants; it stays inside the caps
the GPU tests rely on (ambiguous pixels <= 1 %, pixels on the one-level rule <= 2 %); the new C ABI, the drivers' `warp` argument and the scripts' --warp exist
and refuse what they must -- none of which holds before the feature."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

import geowarp_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g18_geodiffuser_coords.npz")
CASES = list(GR.CASES)
AMBIGUOUS_CAP, ONE_LEVEL_CAP = 0.01, 0.02


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLD))


@functools.lru_cache(maxsize=None)
def staged(name):
    """what the GPU tests compare the rasterisers with, computed once: the restatement (fp64 and fp32) on the GOLDEN fp32 coordinates"""
    img, mask, depth, bg, edit = GR.case_inputs(name)
    t32 = golden()[name + "/tcoords"]
    obj = GR.object_mask(GR.normalise_depth(depth), mask)
    feats = np.concatenate([img / 255.0, mask[..., None].astype(np.float64)], -1)
    ids, comp, amb = GR.splat(t32, feats, return_ambiguous=True)
    ids32, comp32 = GR.splat(t32, feats, dt=np.float32)
    cover, mesh_amb = GR.mesh_cover(t32, obj, return_ambiguous=True)
    scale = np.array([1.0, 1.0, 1.0, 255.0])                    # the mask travels as 0 / 255
    e_comp = float((np.abs(comp32 - comp) / scale)[~amb].max())
    return dict(img=img, mask=mask, depth=depth, bg=bg, edit=edit, t32=t32, obj=obj, feats=feats, ids=ids, comp=comp, amb=amb, ids32=ids32, comp32=comp32,
                cover=cover, cover32=GR.mesh_cover(t32, obj, dt=np.float32), mesh_amb=mesh_amb, scale=scale, e_comp=e_comp)


def u8_bounds(comp, tol):
    """the uint8 image of every value within tol of comp: (lowest, highest) -- the rounding through fp16 and the truncation are monotone"""
    out_scale = np.array([255.0, 255.0, 255.0, 1.0])
    return GR.to_half_u8(np.maximum(comp - tol, 0.0), out_scale), GR.to_half_u8(comp + tol, out_scale)


# ---- the restatement against the reference's own code ---------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_coordinates_pose_and_faces(name):
    g = golden()
    img, mask, depth, bg, edit = GR.case_inputs(name)
    dn = GR.normalise_depth(depth)
    obj = GR.object_mask(dn, mask)
    assert np.array_equal(GR.normalise_depth(depth, np.float32), g[name + "/depth_n"])
    assert np.array_equal(GR.faces(obj), g[name + "/faces"]) and len(g[name + "/faces"]) > 0
    spur = np.argwhere(obj)[0]                                    # the first object pixel in row-major order is the spur: in no triangle
    assert not obj[spur[0] + 1, spur[1]] and 0 not in g[name + "/faces"]
    pose = GR.compose_pose(dn, obj, edit)
    assert np.abs(pose - g[name + "/pose"]).max() <= 16 * GR.U32 * max(1.0, np.abs(pose).max())
    t, clamped = GR.project(dn, pose)
    ref = g[name + "/tcoords"]
    free = ~clamped & (ref[..., 2] > 1e-3)
    e_ref, e_rel = float(g[name + "/e_ref"]), float(g[name + "/e_rel"])
    assert np.isclose(np.abs(ref - t)[free].max(), e_ref, rtol=1e-6) and e_rel <= 2.0 ** -10      # single precision with Z down to the clamp, no worse
    assert (ref[..., 2][clamped] == np.float32(1e-3)).all() and clamped.any() == (name == "combined")
    t32, _ = GR.project(GR.normalise_depth(depth, np.float32), GR.compose_pose(GR.normalise_depth(depth, np.float32), obj, edit, dt=np.float32), dt=np.float32)
    assert np.abs(t32 - t)[free].max() <= GR.MARGIN * e_ref      # the restatement's own float32 run is as near as the reference's


def test_cases_cover_what_they_are_for():
    frames = {}
    for name in CASES:
        t = golden()[name + "/tcoords"]
        obj = staged(name)["obj"]
        frames[name] = (np.abs(t[..., :2]).max(-1) <= 1)[obj].mean()
    assert frames["identity"] == 1.0 and 0.3 < frames["shift_out"] < 0.95                       # part of the object leaves the frame
    assert sorted({GR.CASES[n][0] for n in CASES}) == [40, 48, 64]
    full = {n: int(((staged(n)["ids"] >= 0).sum(-1) == GR.KPP).sum()) for n in CASES}
    assert full["shrink"] > 100 and full["identity"] == 0                                        # more than K candidates: the truncation is exercised
    t = golden()["fold_ry35/tcoords"]
    obj = staged("fold_ry35")["obj"]
    f = GR.faces(obj)
    v = t.reshape(-1, 3)[obj.reshape(-1)]
    area = GR.edge(v[f[:, 0], 0], v[f[:, 0], 1], v[f[:, 1], 0], v[f[:, 1], 1], v[f[:, 2], 0], v[f[:, 2], 1])
    assert (area > 0).any() and (area < 0).any()                                                 # the mesh folds: faces of both orientations


# ---- invariants of the restatement ----------------------------------------------------------------------------------------
def test_identity_maps_every_pixel_to_itself():
    r = GR.coarse_edit(*GR.case_inputs("identity")[:3], [0, 0, 0, 0, 0, 0, 1, 1, 1], GR.case_inputs("identity")[3])
    S = r["tcoords"].shape[0]
    ii, jj = np.mgrid[0:S, 0:S]
    assert np.abs(r["correspondence"] - np.stack([jj, ii], -1)).max() < 1e-9
    assert np.array_equal(r["tcoords"][..., 2], r["depth_n"])


def test_constant_depth_translation_is_a_shift():
    S, n = 40, 3
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    mask = np.zeros((S, S), np.uint8)
    mask[10:25, 8:20] = 255
    depth = np.full((S, S), 0.5, np.float32)                      # the reference's constant-depth case: kept at 0.5
    # the map counts pixels as 2 / (S - 1) of the normalised frame, the rasteriser as 2 / S: n of the rasteriser's pixels are n (S - 1) / S of the map's
    tx = n * (S - 1) / S * 0.5 / GR.FOCAL * 512
    a = GR.coarse_edit(img, mask, depth, [0, 0, 0, 0, 0, 0, 1, 1, 1], img)
    b = GR.coarse_edit(img, mask, depth, [tx, 0, 0, 0, 0, 0, 1, 1, 1], img)
    assert np.abs(b["correspondence"] - a["correspondence"] - [n * (S - 1) / S, 0]).max() < 1e-9
    assert np.allclose(b["composite"][:, 2 * n:-n], a["composite"][:, n:-2 * n], atol=1e-9)
    sure = ~(b["mesh_ambiguous"][:, n:] | a["mesh_ambiguous"][:, :-n])      # on this regular grid pixel centres fall on triangle edges: undecided
    assert np.array_equal(b["mesh_projected"][:, n:][sure], a["mesh_projected"][:, :-n][sure]) and a["mesh_projected"][:, :-n][sure].sum() > 50


def test_nearer_points_win():
    S = 8
    t = np.zeros((S, S, 3))
    t[..., :2], t[..., 2] = 50.0, 1.0                             # everything out of frame ...
    cen = GR.pixel_centres(S, np.float64)
    t[0, 0], t[0, 1] = (cen[3], cen[2], 0.7), (cen[3], cen[2], 0.4)      # ... but two points on the centre of pixel (row 2, col 3)
    feats = np.zeros((S, S, 2))
    feats[0, 0], feats[0, 1] = (1.0, 0.0), (0.0, 1.0)
    a = 1 - np.sqrt(1e-3)                                         # d2 = 0 is clamped at 1e-3
    ids, out = GR.splat(t, feats, K=4)
    assert ids[2, 3].tolist() == [1, 0, -1, -1] and np.allclose(out[2, 3], [(1 - a) * a, a])
    t[0, 0, 2], t[0, 1, 2] = 0.4, 0.4                             # equal z: the lower id first
    assert GR.splat(t, feats, K=4)[0][2, 3].tolist() == [0, 1, -1, -1]
    t[0, 1, 2] = -0.1                                             # behind the camera: dropped
    assert GR.splat(t, feats, K=4)[0][2, 3].tolist() == [0, -1, -1, -1]
    assert (GR.splat(t, feats, K=1)[0] >= 0).sum() == 5           # radius 1.3 pixels: the centre pixel and its four neighbours


@pytest.mark.parametrize("name", CASES)
def test_masks_are_consistent_and_the_restatement_stays_inside_the_caps(name):
    img, mask, depth, bg, edit = GR.case_inputs(name)
    r = GR.coarse_edit(img, mask, depth, edit, bg)
    assert not (r["md_mask"] & r["target_mask"]).any()
    assert ((r["md_mask"] | r["target_mask"]) | ~r["mesh_projected"]).all()
    assert np.array_equal(r["coarse"][~r["target_mask"]], bg[~r["target_mask"]])
    assert r["ambiguous"].mean() <= AMBIGUOUS_CAP and r["mesh_ambiguous"].mean() <= AMBIGUOUS_CAP
    s = staged(name)                                              # the same on the golden coordinates, which the GPU tests use
    assert s["amb"].mean() <= AMBIGUOUS_CAP and s["mesh_amb"].mean() <= AMBIGUOUS_CAP
    assert np.array_equal(s["ids32"][~s["amb"]], s["ids"][~s["amb"]])
    assert np.array_equal(s["cover32"][~s["mesh_amb"]], s["cover"][~s["mesh_amb"]])
    lo, hi = u8_bounds(s["comp"], GR.MARGIN * s["e_comp"] * s["scale"])
    assert (hi.astype(int) - lo).max() <= 1
    assert ((lo != hi).any(-1) & ~s["amb"]).mean() <= ONE_LEVEL_CAP
    assert s["e_comp"] <= 64 * GR.U32                             # a single-precision error, not a disagreement


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NEW = ("ffn_geo_project", "ffn_splat_composite", "ffn_mesh_cover")


def test_new_symbols_are_declared_bound_and_versioned():
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    declared = set(re.findall(r"\b(ffn_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert lib.ffn_version() >= 13
    assert "unpinned" in header[header.index("ffn_splat_composite"):]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from freefine_amd import _lib
    lib = _lib.load()
    p = 4096                                                      # any non-null address: nothing is launched, so nothing is read
    pose = (ctypes.c_float * 12)()
    E = -22
    assert lib.ffn_geo_project(None, p, pose, 550.0, 40, 48, p, p) == E and b"square" in lib.ffn_last_error()
    assert lib.ffn_geo_project(None, None, pose, 550.0, 40, 40, p, p) == E
    assert lib.ffn_geo_project(None, p, None, 550.0, 40, 40, p, p) == E
    assert lib.ffn_geo_project(None, p, pose, 0.0, 40, 40, p, p) == E
    ok = dict(radius=0.05, tau=1.0, K=15, C=4, H=40, W=40)
    for bad in (dict(W=48), dict(K=0), dict(K=33), dict(C=0), dict(C=9), dict(radius=0.0), dict(tau=0.0), dict(tau=-1.0)):
        a = dict(ok, **bad)
        assert lib.ffn_splat_composite(None, p, p, p, p, a["radius"], a["tau"], a["K"], a["C"], a["H"], a["W"], 1, p) == E, bad
    assert lib.ffn_splat_composite(None, p, None, p, p, 0.05, 1.0, 15, 4, 40, 40, 1, p) == E
    assert lib.ffn_mesh_cover(None, p, p, 40, 48, p) == E and b"square" in lib.ffn_last_error()
    assert lib.ffn_mesh_cover(None, p, None, 40, 40, p) == E and lib.ffn_mesh_cover(None, p, p, 40, 40, None) == E


def test_host_refuses_non_square_images():
    from freefine_amd import warp3d
    img = np.zeros((40, 48, 3), np.uint8)
    with pytest.raises(ValueError, match="square"):
        warp3d.geodiffuser_coarse_edit(img, np.zeros((40, 48), np.uint8), np.ones((40, 48), np.float32), [0] * 6 + [1] * 3, img, device="cpu")


def test_pose_is_the_reference_pose():
    from freefine_amd import warp3d
    for name in CASES:
        s = staged(name)
        dn = golden()[name + "/depth_n"]
        centre = GR.lift(dn, GR.FOCAL, np.float32)[s["obj"]].mean(0, dtype=np.float32)
        pose = warp3d.geodiffuser_pose(s["edit"], centre).numpy()
        assert np.abs(pose - golden()[name + "/pose"]).max() <= 4 * GR.U32, name


# ---- the drivers ----------------------------------------------------------------------------------------------------------
def test_prepare_3d_geodiffuser_writes_the_four_trees_under_the_reference_names(tmp_path, monkeypatch):
    from PIL import Image
    from freefine_amd import geobench, warp3d
    root = str(tmp_path / "meta")
    size = 32
    data = geobench.make_synthetic_dataset(root, n_images=2, edits_per_image=2, size=size, seed=5, with_3d=True)
    calls = []

    def fake(img, mask, depth, edit_param, background, focal_length=550, **kw):
        calls.append((tuple(edit_param), focal_length, img.shape, mask.shape, float(depth.max())))
        assert mask.ndim == 2 and set(np.unique(mask)) <= {0, 255}
        t = np.roll(mask > 0, 1, axis=1)
        mesh = t | np.roll(t, 1, axis=0)
        ii, jj = np.mgrid[0:size, 0:size].astype(np.float32)
        return np.where(t[..., None], img, background), t, mesh, mesh & ~t, np.stack([jj, ii], -1) + np.float32(edit_param[0])

    monkeypatch.setattr(warp3d, "geodiffuser_coarse_edit", fake)
    monkeypatch.setattr(geobench, "monocular_depth", lambda img, model, translate_factor=None, **kw: np.full(img.shape[:2], 2.0 + translate_factor, np.float32))
    d3 = os.path.join(root, "Geo-Bench-3D")
    before = {dp: sorted(fs) for dp, _, fs in os.walk(os.path.join(d3, "coarse3d_depth_anything"))}
    done = geobench.prepare_3d(root, object(), dsize=(size, size), verbose=False, warp="geodiffuser")
    keys = [f"{da}/{ins}/{e}" for da, v in data.items() for ins, edits in v["instances"].items() for e in edits]
    assert [d["key"] for d in done] == keys and len(calls) == 4
    assert all(c[1] == 550 * size / 512 and c[2] == (size, size, 3) and c[4] == 2.0 for c in calls)      # translate_factor = 0.0, focal scaled with the side
    da, ins, e = keys[0].split("/")
    assert calls[0][0] == tuple(float(v) for v in data[da]["instances"][ins][e]["edit_param"])             # untouched: / 512 happens in the warp
    for k in keys:
        for tree, ext in (("coarse3d_depth_anything_blended", ".png"), ("mesh_mask", ".png"), ("md_mask", ".png"), ("correspondence", ".npy")):
            assert os.path.exists(os.path.join(d3, tree, k + ext)), (tree, k)
        assert not os.path.exists(os.path.join(d3, "coarse3d_depth_anything_rgb", k + ".png"))
        assert not os.path.exists(os.path.join(d3, "correspondence_visible", k + ".png"))
    assert before == {dp: sorted(fs) for dp, _, fs in os.walk(os.path.join(d3, "coarse3d_depth_anything"))}, "the dataset's own folder is never written"
    md = np.array(Image.open(done[0]["md_mask_path"]))
    mesh = np.array(Image.open(done[0]["target_mask_path"]))
    assert md.shape == (size, size) and set(np.unique(md)) == {0, 255} and not (md & mesh).any()
    corr = np.load(done[0]["correspondence_path"])
    assert corr.shape == (size, size, 2) and corr.dtype == np.float32
    assert geobench.prepare_3d(root, object(), dsize=(size, size), verbose=False, warp="geodiffuser") == [] and len(calls) == 4
    with pytest.raises(ValueError):
        geobench.prepare_3d(root, object(), dsize=(size, size), verbose=False, warp="softsplat")
    with pytest.raises(ValueError):
        geobench.run(None, root, variant="3d_depth", warp="geodiffuser")
    # the draw mask of the edit is md_mask; the edit's other inputs keep today's form
    case = geobench.CaseList(data, os.path.join(d3, "x"), check_exist=False)[0]
    got = geobench.finish_case_3d_geo(geobench.read_case_3d_rgb(case, root, (size, size), prep=None), object())
    assert set(got) == {"ori_img", "ori_mask", "coarse_input", "target_mask", "guidance_text", "draw_mask", "use_auto_draw", "reduce_inp_artifacts", "cons_area"}
    assert np.array_equal(got["draw_mask"] * 255, md) and got["target_mask"].dtype == np.uint8 and set(np.unique(got["target_mask"])) == {0, 255}
    with pytest.raises(ValueError, match="square"):
        geobench.finish_case_3d_geo(geobench.read_case_3d_rgb(case, root, (size, size + 16), prep=None), object())
    with pytest.raises(ValueError):
        geobench.finish_case_3d_geo(geobench.read_case_3d_rgb(case, root, (size, size)), object())       # already resized another way


def test_scripts_take_warp():
    sys.path.insert(0, ROOT)
    from evaluation.FreeFine import get_3d_transform_correspondence as step2
    assert step2.build_parser().parse_args(["--base-dir", "x"]).warp == "p3d"
    assert step2.build_parser().parse_args(["--base-dir", "x", "--warp", "geodiffuser"]).warp == "geodiffuser"
    with pytest.raises(SystemExit):
        step2.build_parser().parse_args(["--base-dir", "x", "--warp", "softsplat"])
    from evaluation.FreeFine import freefine_batch_infer_2d as infer
    a = infer.build_parser().parse_args(["--base-dir", "x", "--variant", "3d_rgb", "--warp", "geodiffuser"])
    assert a.warp == "geodiffuser" and infer.build_parser().parse_args(["--base-dir", "x"]).warp == "p3d"
