"""GPU: the GeoDiffuser warp on the HIP kernels of csrc/geowarp.h against tests/geowarp_ref.py (held to the reference's code by tests/test_geowarp_cpu.py).

Tolerances are measured on the CPU, never from the device: e_ref = max |reference fp32 - fp64 restatement| of the coordinates (stored in the golden file) and
e_comp = max |fp32 restatement - fp64 restatement| of the composites on the same inputs (test_geowarp_cpu.staged); the device is gated at geowarp_ref.MARGIN = 4
times each -- two single-precision evaluations of one formula in different orders.  A pixel the restatement marks ambiguous (a candidate within eps of the
radius, two of the K + 1 nearest within eps in z, a barycentric coordinate within eps of 0) is left out: at most 1 % per case, asserted on the CPU."""
import os

import numpy as np
import pytest

import geowarp_ref as GR
from test_geowarp_cpu import AMBIGUOUS_CAP, CASES, ONE_LEVEL_CAP, golden, staged, u8_bounds

pytestmark = pytest.mark.gpu


def dev(a, gpu, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a)).to(gpu)
    return (t if dtype is None else t.to(dtype)).contiguous()


def check_coordinates(name, t_dev, pose=None):
    """(a): the device's t_coords against the fp64 restatement at MARGIN * e_ref (absolute, and over max(1, |value|)); clamped points only for being clamped.
    pose: the fp64 restatement's own (None), or the float32 pose the device was given, evaluated in fp64"""
    g = golden()
    img, mask, depth, bg, edit = GR.case_inputs(name)
    dn = GR.normalise_depth(depth)
    obj = GR.object_mask(dn, mask)
    P = GR.compose_pose(dn, obj, edit) if pose is None else np.asarray(pose, np.float64)
    t, _ = GR.project(dn, P)
    z_raw = (GR.lift(dn, GR.FOCAL, np.float64) @ P[:3, :3].T + P[:3, 3])[..., 2]
    e_ref, e_rel = float(g[name + "/e_ref"]), float(g[name + "/e_rel"])
    band = 1e-5                                                    # |Z - 1e-3| below this: either side of the clamp is right
    clamped, free = z_raw < 1e-3 - band, z_raw > 1e-3 + band
    assert (clamped | free).mean() >= 0.99
    assert (t_dev[..., 2][clamped] == np.float32(1e-3)).all()
    err = np.abs(t_dev.astype(np.float64) - t)
    print(f"[geo_project] {name}: max err {err[free].max():.3e} (gate {GR.MARGIN * e_ref:.3e}), relative {(err / np.maximum(1, np.abs(t)))[free].max():.3e} "
          f"(gate {GR.MARGIN * e_rel:.3e}), clamped {int(clamped.sum())}")
    assert err[free].max() <= GR.MARGIN * e_ref
    assert (err / np.maximum(1.0, np.abs(t)))[free].max() <= GR.MARGIN * e_rel


@pytest.mark.parametrize("name", CASES)
def test_geo_project_matches_the_reference_coordinates(gpu, name):
    from freefine_amd import ops
    g = golden()
    S = GR.CASES[name][0]
    tcoords, proj = ops.geo_project(dev(g[name + "/depth_n"], gpu), g[name + "/pose"], GR.FOCAL)
    t, p = tcoords.cpu().numpy(), proj.cpu().numpy()
    assert t.shape == (S, S, 3) and p.shape == (S * S, 4)
    assert np.array_equal(p[:, 0], -t[..., 0].reshape(-1)) and np.array_equal(p[:, 1], -t[..., 1].reshape(-1))
    assert np.array_equal(p[:, 2], t[..., 2].reshape(-1)) and not p[:, 3].any()
    check_coordinates(name, t)


def check_rasterisers(name, s, ids, raw, half, cover):
    """(b), (c): ids, composites before and after the fp16 rounding, and the mesh cover, against the restatement `s` on the same coordinates"""
    sure = ~s["amb"]
    assert s["amb"].mean() <= AMBIGUOUS_CAP and s["mesh_amb"].mean() <= AMBIGUOUS_CAP
    want = s["ids"]
    assert np.array_equal(ids[sure], want[sure]), f"{int((ids != want).any(-1)[sure].sum())} decided pixels select other points"
    tol = GR.MARGIN * s["e_comp"] * s["scale"]
    err = np.abs(raw.astype(np.float64) - s["comp"])[sure]
    print(f"[splat_composite] {name}: ambiguous {s['amb'].mean():.4f}, composite err {(err / s['scale']).max():.3e} (gate {GR.MARGIN * s['e_comp']:.3e}); "
          f"mesh ambiguous {s['mesh_amb'].mean():.4f}")
    assert (err <= tol).all()
    lo, hi = u8_bounds(s["comp"], tol)
    out_scale = np.array([255.0, 255.0, 255.0, 1.0], np.float16)
    assert np.array_equal(half.astype(np.float16).astype(np.float32), half), "the rounded result holds fp16 values"
    u8 = (half.astype(np.float16) * out_scale).astype(np.uint8)
    assert ((lo != hi).any(-1) & sure).mean() <= ONE_LEVEL_CAP
    assert ((u8 >= lo) & (u8 <= hi))[sure].all()                  # equal where the truncation is decided, within one level elsewhere
    assert np.array_equal(cover[~s["mesh_amb"]] > 0, s["cover"][~s["mesh_amb"]])
    assert set(np.unique(cover)) <= {0, 1}


@pytest.mark.parametrize("name", CASES)
def test_splat_composite_and_mesh_cover_match_the_restatement(gpu, name):
    import torch
    from freefine_amd import ops
    s = staged(name)
    S = GR.CASES[name][0]
    t32 = dev(s["t32"], gpu)
    proj = torch.cat([-t32[..., :2], t32[..., 2:], torch.zeros_like(t32[..., :1])], -1).reshape(S * S, 4).contiguous()
    feat = dev(s["feats"].reshape(S * S, 4), gpu, torch.float32)
    r = GR.RADIUS / S * 2.0
    offs, lst = ops.splat_tile_lists(proj, r, S)
    ids = ops.splat_ids(proj, offs, lst, r, GR.KPP, S).cpu().numpy()
    raw = ops.splat_composite(proj, feat, offs, lst, r, GR.TAU, GR.KPP, S, round_half=False).cpu().numpy()
    half = ops.splat_composite(proj, feat, offs, lst, r, GR.TAU, GR.KPP, S, round_half=True).cpu().numpy()
    cover = ops.mesh_cover(t32, dev(s["obj"].astype(np.uint8), gpu)).cpu().numpy()
    check_rasterisers(name, s, ids, raw, half, cover)
    assert np.array_equal(raw.astype(np.float16).astype(np.float32), half)      # one rounding of the same sums


def test_tau_and_channel_count(gpu):
    """tau != 1 takes the pow path; C = 1 and C = 8 channels, K = 5 (the 8-slot instantiation) and K = 20 (the 32-slot one)"""
    import torch
    from freefine_amd import ops
    s = staged("shrink")
    S = GR.CASES["shrink"][0]
    t32 = dev(s["t32"], gpu)
    proj = torch.cat([-t32[..., :2], t32[..., 2:], torch.zeros_like(t32[..., :1])], -1).reshape(S * S, 4).contiguous()
    rng = np.random.default_rng(3)
    r = GR.RADIUS / S * 2.0
    offs, lst = ops.splat_tile_lists(proj, r, S)
    for C, K, tau in ((1, 5, 0.5), (8, 20, 2.0)):
        feats = rng.random((S, S, C))
        ids, comp, amb = GR.splat(s["t32"], feats, tau=tau, K=K, return_ambiguous=True)
        _, comp32 = GR.splat(s["t32"], feats, tau=tau, K=K, dt=np.float32)
        e = np.abs(comp32 - comp)[~amb].max()
        got = ops.splat_composite(proj, dev(feats.reshape(S * S, C), gpu, torch.float32), offs, lst, r, tau, K, S, round_half=False).cpu().numpy()
        assert np.array_equal(ops.splat_ids(proj, offs, lst, r, K, S).cpu().numpy()[~amb], ids[~amb])
        assert amb.mean() <= AMBIGUOUS_CAP and np.abs(got - comp)[~amb].max() <= GR.MARGIN * e, (C, K, tau)


@pytest.mark.parametrize("name", CASES)
def test_geodiffuser_coarse_edit_end_to_end(gpu, name):
    """(d): the host entry point.  Its pose and coordinates against the reference's (golden) and the fp64 restatement; its images and masks against the
    restatement run on the coordinates the device produced (the rasterisers see those, not the restatement's)."""
    from freefine_amd import warp3d
    img, mask, depth, bg, edit = GR.case_inputs(name)
    S = depth.shape[0]
    coarse, tmask, mesh, md, corr, st = warp3d.geodiffuser_coarse_edit(img, mask, depth, edit, bg, device=gpu, return_stages=True)
    g = golden()
    assert np.array_equal(st["depth_n"].cpu().numpy(), g[name + "/depth_n"])
    assert np.abs(st["pose"].numpy() - g[name + "/pose"]).max() <= 4 * GR.U32 * max(1.0, np.abs(g[name + "/pose"]).max())
    t_dev = st["tcoords"].cpu().numpy()
    check_coordinates(name, t_dev, st["pose"].numpy())              # the centre is a device reduction: the pose may differ from the golden one in the last bit
    assert corr.dtype == np.float32 and np.array_equal(corr, ((t_dev[..., :2] + np.float32(1.0)) / np.float32(2.0) * np.float32(S - 1)))
    obj = GR.object_mask(GR.normalise_depth(depth), mask)
    feats = np.concatenate([img / 255.0, mask[..., None].astype(np.float64)], -1)
    ids, comp, amb = GR.splat(t_dev, feats, return_ambiguous=True)
    cover, mesh_amb = GR.mesh_cover(t_dev, obj, return_ambiguous=True)
    assert amb.mean() <= AMBIGUOUS_CAP and mesh_amb.mean() <= AMBIGUOUS_CAP
    s = staged(name)
    lo, hi = u8_bounds(comp, GR.MARGIN * s["e_comp"] * s["scale"])
    sure = ~amb
    decided = sure & (lo == hi).all(-1)
    assert (sure & ~decided).mean() <= ONE_LEVEL_CAP
    t_lo, t_hi = lo[..., 3] / 255.0 > 0.5, hi[..., 3] / 255.0 > 0.5
    assert np.array_equal(tmask[decided], t_lo[decided]) and ((tmask == t_lo) | (tmask == t_hi))[sure].all()
    inside = decided & tmask
    assert np.array_equal(coarse[inside], lo[..., :3][inside]) and np.array_equal(coarse[~tmask], bg[~tmask])
    near = sure & tmask & ~decided
    assert (np.abs(coarse[near].astype(int) - lo[..., :3][near]) <= 1).all()
    assert np.array_equal(mesh[~mesh_amb], cover[~mesh_amb]) and np.array_equal(md, mesh & ~tmask)
    assert not (md & tmask).any() and tmask.any() and mesh.any()


def test_prepare_3d_geodiffuser_with_a_depth_network(gpu, tmp_path):
    """the synthetic GeoBenchMeta tree through geobench.prepare_3d(warp="geodiffuser") with a tiny seeded depth network: the four trees under the reference's
    names, the files are those of finish_case_3d_geo on the same case, and Mean Distance finds the map where it looks"""
    import torch
    from PIL import Image
    from freefine_amd import depth as FDp, geobench, metrics as FM
    dcfg = FDp.depth_config("tiny")
    dmodel = FDp.HipDepthAnything(dcfg, FDp.synthetic_state(dcfg, seed=3), dtype=torch.float32, device=gpu)
    size = 96
    root = str(tmp_path / "meta")
    data = geobench.make_synthetic_dataset(root, n_images=1, edits_per_image=2, size=size, seed=8, with_3d=True)
    done = geobench.prepare_3d(root, dmodel, dsize=(size, size), verbose=False, warp="geodiffuser")
    assert len(done) == 2
    d3 = os.path.join(root, "Geo-Bench-3D")
    cl = geobench.CaseList(data, os.path.join(d3, "unused"), check_exist=False)
    for d, case in zip(done, [cl[0], cl[1]]):
        want = geobench.finish_case_3d_geo(geobench.read_case_3d_rgb(case, root, (size, size), prep=None), dmodel, correspondence=True)
        assert np.array_equal(np.array(Image.open(d["coarse_input_path"])), want["coarse_input"])
        assert np.array_equal(np.array(Image.open(d["target_mask_path"])), want["target_mask"])
        assert np.array_equal(np.array(Image.open(d["md_mask_path"])), want["md_mask"]) and np.array_equal(want["draw_mask"] * 255, want["md_mask"])
        corr = np.load(d["correspondence_path"])
        assert corr.shape == (size, size, 2) and np.array_equal(corr, want["correspondence"]) and np.isfinite(corr).all()
        gen = os.path.join(d3, "Gen_results_FreeFine_depth_rgb", d["key"] + ".png")
        assert FM.correspondence_path(gen) == d["correspondence_path"]
        obj = (want["ori_mask"] if want["ori_mask"].ndim == 2 else want["ori_mask"][:, :, 0]) > 0
        assert FM.transform_coordinates(case["edit_param"], (size, size), obj, d["correspondence_path"]).shape == (size, size, 2)
        for tree in ("coarse3d_depth_anything_blended", "mesh_mask", "md_mask"):
            assert os.path.dirname(d["coarse_input_path"]).replace("coarse3d_depth_anything_blended", tree) == os.path.join(d3, tree, os.path.dirname(d["key"]))
    assert not os.path.exists(os.path.join(d3, "coarse3d_depth_anything_rgb")) and not os.path.exists(os.path.join(d3, "correspondence_visible"))
