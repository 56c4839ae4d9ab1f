"""The point-cloud warp of the 3-D coarse edit on the HIP kernels of csrc/splat.h: depth-lifted object pixels -> rigid
transform about the cloud's centre -> FoV-perspective projection -> disc splat with the K nearest points per pixel, alpha-composited.
Restates IntegratedP3DTransRasterBlendingFull (/root/reference/src/utils/geo_utils.py:427-528; helpers :343-425), whose renderer is
pytorch3d's PointsRasterizer + AlphaCompositor.  PARITY UNPINNED: pytorch3d is not in the build image, so the result is checked against
oracle/warp3d.py (a numpy restatement of the same published semantics) and against domain invariants, not against the reference's output.

Host side (plumbing): index list of the masked pixels, the centre / extents of the cloud (three reductions over [n, 3]), the 3 x 3 rotation,
the exclusive scan of the tile counts.  Device side: lift, transform + project, tile binning, top-K splat + compositing, and -- on request --
the correspondence map of the warp (where every source pixel went; Mean Distance reads it for 3-D edits) with the visibility of every point."""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream(dev=None):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device(device):
    """None -> the CURRENT device (rank r of a sharded run works on cuda:LOCAL_RANK; "cuda:0" was the default until round 4)"""
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def euler_xyz_matrix(rx, ry, rz):
    """pytorch3d's euler_angles_to_matrix(convention="XYZ") of angles given in degrees (get_transformation, geo_utils.py:365-368)"""
    a, b, c = (torch.deg2rad(torch.tensor(float(v), dtype=torch.float32)) for v in (rx, ry, rz))
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    Rx = torch.stack([one, zero, zero, zero, torch.cos(a), -torch.sin(a), zero, torch.sin(a), torch.cos(a)]).reshape(3, 3)
    Ry = torch.stack([torch.cos(b), zero, torch.sin(b), zero, one, zero, -torch.sin(b), zero, torch.cos(b)]).reshape(3, 3)
    Rz = torch.stack([torch.cos(c), -torch.sin(c), zero, torch.sin(c), torch.cos(c), zero, zero, zero, one]).reshape(3, 3)
    return Rx @ Ry @ Rz


def point_cloud_warp(img, depth, transforms, focal_length_x, focal_length_y, mask, object_only=True, splatting_radius=0.1,
                     splatting_points_per_pixel=5, device=None, fov_deg=60.0, return_covered=False, pixel_translation=False,
                     return_correspondence=False):
    """img uint8 [H, W, 3], depth float [H, W], mask [H, W] (> 0 = object), transforms = [tx, ty, tz (relative to the cloud's extent),
    rx, ry, rz (degrees), sx, sy, sz] -> (rendered uint8 [H, W, 3], mask uint8 [H, W] by the reference's own test `sum of the K ids != -30`
    -- 255 everywhere unless K = 30, geo_utils.py:517) and, with return_covered, the pixels any point reached (x 255).
    pixel_translation (extension, off = the reference's semantics): tx, ty, tz are IMAGE PIXELS -- the cloud moves by t * mean depth / focal
    length, i.e. by t pixels to the right / down at its mean depth (tz: away from the camera) -- instead of fractions of the cloud's extent.
    return_correspondence (off: exactly the calls above): the result is followed by `corr`, float32 [H, W, 2] with last axis (x, y) -- the
    continuous pixel of the RENDERED image every source pixel went to (the on-disk order of the reference's correspondence files,
    evaluation/FreeFine/get_3d_transform_correspondence.py:21-54, which metrics.transform_coordinates reverses to (row, col)); pixels outside the
    object hold their own coordinates, points the renderer does not draw (behind the camera) NaN -- and by `visible`, uint8 [H, W] x 255: the
    source pixel's point is among the K points composited at the pixel nearest to its target, i.e. it shows in the rendered image (0 for
    self-occluded points, points that leave the image, and every pixel outside the object).
    The half-pixel offset: the reference lifts pixel i at i - W/2 while the rasterizer samples pixel centres, so the
    identity transform maps pixel (i, j) to (i - 0.5, j - 0.5), not to itself.  It is kept: the rendered image carries the same offset, and the
    map must agree with the image it describes."""
    lib = L.load()
    dev = _device(device)
    H, W = depth.shape
    K = int(splatting_points_per_pixel)
    d = torch.as_tensor(np.ascontiguousarray(depth), dtype=torch.float32).to(dev).contiguous()
    m = torch.as_tensor(np.ascontiguousarray(mask)).to(dev).reshape(-1)
    keep = (m > 0) if object_only else torch.ones_like(m, dtype=torch.bool)
    idx = torch.nonzero(keep).flatten().to(torch.int32).contiguous()
    n = int(idx.numel())
    assert K * max(n, 1) < 2 ** 31, "the id sum of a pixel's K points is kept in int32 (the reference sums in int64): K * n must stay below 2^31"
    image = torch.zeros(H, W, 3, dtype=torch.float32, device=dev)
    idx_sum = torch.full((H, W), -K, dtype=torch.int32, device=dev)
    covered = torch.zeros(H, W, dtype=torch.uint8, device=dev)
    if return_correspondence:                                              # identity outside the object; the kernel writes the object's pixels
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
        corr = torch.stack([xs, ys], -1).contiguous()
        visible = torch.zeros(H, W, dtype=torch.uint8, device=dev)
    if n > 0:
        rgb = torch.as_tensor(np.ascontiguousarray(img)).to(dev).reshape(-1, 3).float().index_select(0, idx.long()).contiguous()
        pts = torch.empty(n, 4, dtype=torch.float32, device=dev)
        L.check(lib.ffn_splat_lift(_stream(dev), _p(d), _p(idx), _p(pts), n, W, H, float(focal_length_x), float(focal_length_y)), "splat_lift")
        xyz = pts[:, :3]
        # centre and extents (translation invariant: centred or not) in ONE host round trip
        c_h, ext = torch.cat([xyz.mean(0), xyz.max(0).values - xyz.min(0).values]).cpu().split(3)
        x = L.SplatXform()
        for a in range(3):
            x.center[a] = float(c_h[a])
            t = float(transforms[a])
            if pixel_translation:                                          # world +x / +y point left / up after the flip of geo_utils.py:455
                x.translate[a] = (-1.0 if a < 2 else 1.0) * t * float(c_h[2]) / float((focal_length_x, focal_length_y, focal_length_x)[a])
            else:
                x.translate[a] = 0.0 if t == 0 else float(ext[a]) * t      # refine_transforms (geo_utils.py:399-413)
            x.scale[a] = float(transforms[6 + a])
        R = euler_xyz_matrix(*transforms[3:6])
        for a in range(9):
            x.rotate[a] = float(R.reshape(-1)[a])
        x.tan_half_fov = math.tan(math.radians(fov_deg) / 2)
        proj = torch.empty(n, 4, dtype=torch.float32, device=dev)
        L.check(lib.ffn_splat_project(_stream(dev), _p(pts), _p(proj), n, C.byref(x)), "splat_project")
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        counts = torch.zeros(tiles, dtype=torch.int32, device=dev)
        r = float(splatting_radius)
        L.check(lib.ffn_splat_bin(_stream(dev), 0, _p(proj), n, r, W, H, _p(counts), None, None), "splat_bin(count)")
        offs = torch.zeros(tiles + 1, dtype=torch.int32, device=dev)
        offs[1:] = torch.cumsum(counts, 0)
        total = int(offs[-1].item())
        lst = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        counts.zero_()
        L.check(lib.ffn_splat_bin(_stream(dev), 1, _p(proj), n, r, W, H, _p(counts), _p(offs), _p(lst)), "splat_bin(fill)")
        L.check(lib.ffn_splat_render(_stream(dev), _p(proj), _p(rgb), _p(offs), _p(lst), r, K, W, H, _p(image), _p(idx_sum), _p(covered)), "splat_render")
        if return_correspondence:
            ids = torch.empty(H, W, K, dtype=torch.int32, device=dev)
            L.check(lib.ffn_splat_ids(_stream(dev), _p(proj), _p(offs), _p(lst), r, K, W, H, _p(ids)), "splat_ids")
            L.check(lib.ffn_splat_correspond(_stream(dev), _p(proj), _p(idx), n, W, H, _p(ids), K, _p(corr), _p(visible)), "splat_correspond")
    out = image.cpu().numpy().astype(np.uint8)                              # `.astype(np.uint8)` of the float image (geo_utils.py:516)
    ref_mask = ((idx_sum != -30).to(torch.uint8) * 255).cpu().numpy()
    res = (out, ref_mask, (covered * 255).cpu().numpy()) if return_covered else (out, ref_mask)
    if return_correspondence:
        res += (corr.cpu().numpy(), (visible * 255).cpu().numpy())
    return res


def coarse_edit_3d(ori_img, ori_mask, depth, transforms, background, focal_length=550.0, splatting_radius=None, points_per_pixel=5,
                   device=None, pixel_translation=True, return_correspondence=False):
    """A coarse 3-D edit built from the RGB image and a transform instead of being read from disk (freefine_batch_infer_3d_depth.py:121 reads
    `coarse3d_depth_anything/...png`, rendered by the GeoDiffuser warp of get_3d_transform_correspondence.py:217-251: geodiffuser_coarse_edit
    below): the object's pixels, lifted through `depth`, moved by `transforms` (translation in image pixels by default -- this
    module's own convention, an extension; see geobench.load_case_3d_rgb) and splatted over `background` (the inpainted scene).  NOT a
    restatement of the dataset's generator.  Returns (coarse uint8 [H, W, 3], target_mask uint8 {0, 255}), followed with return_correspondence by
    point_cloud_warp's `corr` and `visible` (the map of THIS warp, half-pixel offset included: it describes `coarse`).
    Default radius: 1.5 pixels in NDC units (holes between neighbouring source pixels close under moderate rotations / scalings)."""
    H, W = ori_mask.shape[:2]
    m2 = ori_mask if ori_mask.ndim == 2 else ori_mask[:, :, 0]
    r = splatting_radius if splatting_radius is not None else 1.5 * 2.0 / min(H, W)
    img, _, cov, *extra = point_cloud_warp(ori_img, depth, transforms, focal_length, focal_length, m2, True, r, points_per_pixel, device, return_covered=True,
                                           pixel_translation=pixel_translation, return_correspondence=return_correspondence)
    tgt = cov > 0
    coarse = np.where(tgt[:, :, None], img, background).astype(np.uint8)
    return (coarse, tgt.astype(np.uint8) * 255, *extra)


def geodiffuser_pose(edit_param, centre, length=512):
    """The pose the reference's step 2 applies to every point (float32 torch on the host, op for op): P = T(t) Sx Sy Sz Rx Ry Rz with t = edit_param[0:3] /
    length (get_transformed_mask, evaluation/GeoDiffuser/GeoDiffuser/utils/ui_utils2.py:709-735, called at evaluation/FreeFine/
    get_3d_transform_correspondence.py:233-251), moved to the object's centre: T(-c)^-1 P T(-c) (warp_utils.py:427-437).  -> float32 [4, 4]"""
    e = [float(v) for v in edit_param]
    P = torch.eye(4).float()
    tr = torch.eye(4)
    for a in range(3):
        tr[a, 3] += e[a] / length
    P = P @ tr.type_as(P)
    for a in range(3):
        if e[6 + a] != 1.0:
            s = torch.eye(4).type_as(P)
            s[a, a] = e[6 + a]
            P = P @ s
    for a in range(3):
        if e[3 + a] != 0.0:
            r = np.radians(e[3 + a])
            c, s = np.cos(r), np.sin(r)
            R = [[[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]],
                 [[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]],
                 [[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]][a]
            P = P @ torch.tensor(R, dtype=torch.float64).type_as(P)
    back = torch.eye(4).float()
    back[:3, 3] += -torch.as_tensor(centre, dtype=torch.float32).cpu()
    return (back.inverse() @ P @ back).float()


def geodiffuser_coarse_edit(img_u8, mask, depth, edit_param, background, focal_length=550, radius=1.3, tau=1.0, points_per_pixel=15, device=None,
                            return_stages=False):
    """Step 2 of the reference's GeoBench-3D preparation on the HIP kernels of csrc/geowarp.h: the GeoDiffuser warp that renders the dataset's
    coarse3d_depth_anything_blended/, mesh_mask/, md_mask/ and correspondence/ (evaluation/FreeFine/get_3d_transform_correspondence.py:207-289 ->
    get_transformed_mask / project_image_latest, evaluation/GeoDiffuser/GeoDiffuser/utils/ui_utils2.py:685-743, 504-593; get_transform_coordinates,
    vis_utils.py:404-479; forward_splatting_pytorch3d_warp and the SynSin splat, warp_utils.py:407-492, 28-176; the mask mesh, :235-399).
    img_u8 uint8 [S, S, 3], mask [S, S] (> 0 = object; splatted as 0 / 255 like the reference's mask image), depth float [S, S] as the depth network
    gives it (normalised here), edit_param = [tx, ty, tz (pixels of a 512 image: / 512), rx, ry, rz (degrees), sx, sy, sz], background uint8 [S, S, 3].
    EVERY pixel is lifted and moved (not only the object's); the mask is one more splatted feature.  Square images only (ValueError otherwise).
    -> (coarse uint8 [S, S, 3] = where(target_mask, splat * 255 -> uint8, background); target_mask bool [S, S] = warped mask > 0.5, what the script saves as
    mesh_mask; mesh_projected bool [S, S], the projected mask mesh; md_mask = mesh_projected outside target_mask; correspondence float32 [S, S, 2], last
    axis (x, y), the reference's denormalize_coordinates of t_coords in its on-disk order).  return_stages: followed by a dict of the device's intermediates.
    PINNED to the reference's code: pose, t_coords and the mesh's triangles.  NOT pinned: the point and mesh rasterisers (pytorch3d is absent; they
    restate its published kernels and are held to tests/geowarp_ref.py).  Out of scope: the GeoDiffuser diffusion edit, the softsplat / cupy path."""
    from . import ops
    dev = _device(device)
    depth = np.asarray(depth)
    if depth.ndim != 2 or depth.shape[0] != depth.shape[1]:
        raise ValueError(f"geodiffuser_coarse_edit: square images only (the reference takes sqrt(N) for the side); depth is {depth.shape}")
    S = depth.shape[0]
    m2 = np.asarray(mask)
    m2 = m2 if m2.ndim == 2 else m2[:, :, 0]
    if np.asarray(img_u8).shape != (S, S, 3) or m2.shape != (S, S) or np.asarray(background).shape != (S, S, 3):
        raise ValueError(f"geodiffuser_coarse_edit: image {np.asarray(img_u8).shape}, mask {m2.shape}, background {np.asarray(background).shape} for a depth of {depth.shape}")
    K = int(points_per_pixel)
    f = float(focal_length)
    with torch.cuda.device(dev):
        d = torch.as_tensor(np.ascontiguousarray(depth), dtype=torch.float32).to(dev)
        if float(d.sum()) == 0.5 * d.numel():                              # the constant-depth case (vis_utils.py:410-411)
            d = torch.full_like(d, 0.5)
        else:
            d = d / (d.max() + 1e-8)
            d[d > 0.95] = 1.0
        d = d.contiguous()
        m = torch.as_tensor(np.ascontiguousarray(m2)).to(dev) > 0
        obj = (m & (d < 0.95))
        if not bool(obj.any()):
            raise ValueError("geodiffuser_coarse_edit: no pixel of the mask is nearer than 0.95 of the depth range: the object has no centre")
        # pixel2cam (warp_utils.py:738-747) for the centre only; the kernel lifts every pixel again
        ar = torch.arange(S, dtype=torch.float32, device=dev)
        c = S / 2.0
        lin = ar * (1.0 / f) + (-c / f)
        cam = torch.stack([lin[None, :] * d, lin[:, None] * d, d], 0)
        centre = cam[:, obj].mean(-1)
        pose = geodiffuser_pose(edit_param, centre)
        tcoords, proj = ops.geo_project(d, pose[:3], f)
        r = float(radius) / float(S) * 2.0
        img = torch.as_tensor(np.ascontiguousarray(img_u8)).to(dev)
        feat = torch.cat([img.reshape(-1, 3).float() / 255.0, m.reshape(-1, 1).float() * 255.0], 1).contiguous()
        offs, lst = ops.splat_tile_lists(proj, r, S)
        out = ops.splat_composite(proj, feat, offs, lst, r, tau, K, S, round_half=True)
        cover = ops.mesh_cover(tcoords, obj.to(torch.uint8).contiguous())
        # `(image_warped...numpy() * 255.0).astype("uint8")`, ui_utils2.py:541: a float16 array times a Python scalar stays float16, so the product is
        # rounded to fp16 once more before it is truncated (`out` holds fp16 values: .half() is exact)
        p_image = (out[..., :3].half() * 255.0).to(torch.uint8)
        tmask = out[..., 3].to(torch.uint8).double() / 255.0 > 0.5         # :553-556
        bg = torch.as_tensor(np.ascontiguousarray(background)).to(dev)
        coarse = torch.where(tmask[..., None], p_image, bg)
        corr = (tcoords[..., :2] + 1.0) / 2.0 * (S - 1)
        mesh = cover > 0
        res = (coarse.cpu().numpy(), tmask.cpu().numpy(), mesh.cpu().numpy(), (mesh & ~tmask).cpu().numpy(), corr.cpu().numpy())
        if return_stages:
            res += (dict(depth_n=d, obj=obj, pose=pose, tcoords=tcoords, proj=proj, offs=offs, list=lst, composite=out, feat=feat, radius=r),)
    return res


def save_geodiffuser_case(root, da_n, ins_id, edit_ins, coarse, target_mask, md_mask, corr):
    """One case of the reference's step 2 under the reference's names (get_3d_transform_correspondence.py:194-203, 253-288): <root>/
    coarse3d_depth_anything_blended/<da>/<ins>/<edit>.png, mesh_mask/...png, md_mask/...png, correspondence/...npy.  Never the dataset's own
    coarse3d_depth_anything/.  -> the four paths"""
    from PIL import Image
    sub = os.path.join(str(da_n), str(ins_id))
    paths = []
    for tree, arr in (("coarse3d_depth_anything_blended", np.asarray(coarse, np.uint8)), ("mesh_mask", (np.asarray(target_mask) > 0).astype(np.uint8) * 255),
                      ("md_mask", (np.asarray(md_mask) > 0).astype(np.uint8) * 255)):
        os.makedirs(os.path.join(root, tree, sub), exist_ok=True)
        paths.append(os.path.join(root, tree, sub, f"{edit_ins}.png"))
        Image.fromarray(arr).save(paths[-1])
    paths.append(save_correspondence(root, da_n, ins_id, edit_ins, corr)[0])
    return paths


def save_correspondence(root, da_n, ins_id, edit_ins, corr, visible=None):
    """The correspondence map of one case where Mean Distance looks for it: <root>/correspondence/<da_n>/<ins_id>/<edit_ins>.npy, float32 [H, W, 2]
    with last axis (x, y) (the reference's save_correspondence and layout, evaluation/FreeFine/get_3d_transform_correspondence.py:21-54, 197, 282-288;
    read at evaluation/metrics/MD/mean_distance.py:108, 122), and, when `visible` is given, <root>/correspondence_visible/<da_n>/<ins_id>/<edit_ins>.png
    (an extension: metrics.calculate_md(visible_only=True) reads it).  -> (path of the map, path of the image or None)"""
    corr = np.asarray(corr, np.float32)
    if corr.ndim != 3 or corr.shape[2] != 2:
        raise ValueError(f"a correspondence map is [H, W, 2]; got shape {corr.shape}")
    sub = os.path.join(str(da_n), str(ins_id))
    os.makedirs(os.path.join(root, "correspondence", sub), exist_ok=True)
    path = os.path.join(root, "correspondence", sub, f"{edit_ins}.npy")
    np.save(path, corr)
    vis_path = None
    if visible is not None:
        from PIL import Image
        visible = np.asarray(visible)
        if visible.shape != corr.shape[:2]:
            raise ValueError(f"the visibility image {visible.shape} and the map {corr.shape[:2]} differ in size")
        os.makedirs(os.path.join(root, "correspondence_visible", sub), exist_ok=True)
        vis_path = os.path.join(root, "correspondence_visible", sub, f"{edit_ins}.png")
        Image.fromarray((visible > 0).astype(np.uint8) * 255).save(vis_path)
    return path, vis_path
