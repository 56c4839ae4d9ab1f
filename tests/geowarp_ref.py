"""The GeoDiffuser warp of the reference's GeoBench-3D step 2, restated in numpy, brute force (every pixel against every point / triangle):
evaluation/FreeFine/get_3d_transform_correspondence.py:207-289 -> evaluation/GeoDiffuser/GeoDiffuser/utils/ui_utils2.py:685-743 (pose), :504-593 (outputs);
vis_utils.py:404-479 (depth normalisation, object mask); warp_utils.py:407-492, 599-645, 738-747 (coordinates), :28-176 (z-buffer splat), :235-298,
304-399 (mask mesh).  `dt` is the arithmetic every stage runs in: np.float64 (the yardstick) or np.float32 (the size of single-precision error).

What is pinned: coordinates, pose and faces are held to the reference's own code by tests/golden/g18_geodiffuser_coords.npz (tools/gen_golden.py run_g18).
What is not: pytorch3d's rasterize_points / rasterize_meshes are absent, so `splat` and `mesh_cover` restate their published semantics (K nearest by z
among d2 < r2, ties by point id; barycentric coordinates all > 0, |area| <= 1e-8 skipped) and rest on invariants (tests/test_geowarp_cpu.py)."""
import numpy as np

U32 = 2.0 ** -23          # float32 spacing in [1, 2): the magnitude of in-frame NDC coordinates
MARGIN = 4.0              # every measured single-precision error is gated at MARGIN times itself
FOCAL, RADIUS, TAU, KPP = 550.0, 1.3, 1.0, 15       # get_3d_transform_correspondence.py:244-251


# ---- the recorded cases (tools/gen_golden.py run_g18 runs the reference on exactly these) ---------------------------------
#        name        S   edit_param = tx ty tz (pixels of a 512 image) rx ry rz (degrees) sx sy sz
CASES = {
    "identity": (64, [0, 0, 0, 0, 0, 0, 1, 1, 1]),
    "shift_out": (48, [7, -2, 0, 0, 0, 0, 1, 1, 1]),           # 7 / 512 camera units at depth ~0.45 and f = 550: ~17 pixels, part of the object leaves
    "fold_ry35": (40, [0, 0, 0, 0, 35, 0, 1, 1, 1]),
    "shrink": (48, [0, 0, 0, 0, 0, 0, 0.5, 0.5, 0.5]),
    "combined": (40, [1, 1, -215, 3, -4, 15, 0.6, 0.5, 1.0]),    # tz pulls the object's nearest points through the camera: Z at the 1e-3 clamp
}


def case_inputs(name):
    """-> (img uint8 [S, S, 3], mask uint8 {0, 255} [S, S], depth float32 [S, S], background uint8 [S, S, 3], edit_param).  The mask: a blob with a
    hole and a one-pixel spur (which carries no triangle).  The depth: a dome over the object in front of a sloping background that passes 0.95 of the
    maximum, plus seeded noise so that points drawn at one pixel do not share z."""
    S, edit = CASES[name]
    rng = np.random.default_rng(1800 + S + len(name))
    ii, jj = np.mgrid[0:S, 0:S].astype(np.float64)
    cy, cx, rad = 0.5 * S - 1.5, 0.5 * S + 1.0, 0.3 * S
    blob = (ii - cy) ** 2 / 1.3 + (jj - cx) ** 2 < rad ** 2
    blob &= ~((ii - cy - 2) ** 2 + (jj - cx + 3) ** 2 < (0.08 * S) ** 2)          # the hole
    mask = blob.copy()
    top = int(np.argwhere(blob[:, int(cx)])[0, 0])
    mask[top - 2, int(cx)] = True                                                   # the spur: one pixel, detached by one row
    dome = 0.55 - 0.15 * np.clip(1 - ((ii - cy) ** 2 + (jj - cx) ** 2) / rad ** 2, 0, 1)
    back = 0.75 + 0.27 * jj / (S - 1)
    depth = np.where(blob, dome, back) + rng.uniform(-0.01, 0.01, (S, S))
    depth[top - 2, int(cx)] = 0.5
    depth = (depth * 7.3).astype(np.float32)                                        # metres, say: the reference normalises by the maximum
    img = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    bg = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    return img, mask.astype(np.uint8) * 255, depth, bg, [float(v) for v in edit]


# ---- coordinates ----------------------------------------------------------------------------------------------------------
def normalise_depth(depth, dt=np.float64):
    """vis_utils.py:410-423"""
    d = np.asarray(depth).astype(dt)
    if d.sum() == 0.5 * d.size:
        return np.full_like(d, 0.5)
    d = d / (d.max() + dt(1e-8))
    d[d > 0.95] = 1.0
    return d


def object_mask(depth_n, mask):
    """vis_utils.py:423-430: the object's points are the mask's pixels nearer than 0.95"""
    return (np.asarray(mask) > 0) & (depth_n < 0.95)


def rot(deg, axis, dt):
    r = np.radians(deg)
    c, s = np.cos(r), np.sin(r)
    m = np.eye(4)
    a, b = [(1, 2), (0, 2), (0, 1)][axis]
    m[a, a], m[b, b] = c, c
    m[a, b], m[b, a] = (-s, s) if axis != 1 else (s, -s)
    return m.astype(dt)


def translate(v, dt):
    m = np.eye(4, dtype=dt)
    m[:3, 3] = np.asarray(v, dt)
    return m


def edit_matrix(edit_param, dt=np.float64, length=512):
    """ui_utils2.py:709-735 with the script's translation / 512: T(t) Sx Sy Sz Rx Ry Rz"""
    e = [float(v) for v in edit_param]
    m = translate([e[0] / length, e[1] / length, e[2] / length], dt)
    for a in range(3):
        if e[6 + a] != 1.0:
            s = np.eye(4, dtype=dt)
            s[a, a] = e[6 + a]
            m = m @ s
    for a in range(3):
        if e[3 + a] != 0.0:
            m = m @ rot(e[3 + a], a, dt)
    return m


def lift(depth_n, focal, dt):
    """pixel2cam with K = (f, f, S/2, S/2) -> [S, S, 3]"""
    S = depth_n.shape[0]
    ii, jj = np.mgrid[0:S, 0:S].astype(dt)
    c, f = dt(S / 2.0), dt(focal)
    return np.stack([(jj / f - c / f) * depth_n, (ii / f - c / f) * depth_n, depth_n], -1).astype(dt)


def compose_pose(depth_n, obj, edit_param, focal=FOCAL, dt=np.float64):
    """warp_utils.py:421-437: T(c) P T(-c), c the mean camera point of the object -> [4, 4]"""
    c = lift(depth_n, focal, dt)[obj].mean(0, dtype=dt)
    return (translate(c, dt) @ edit_matrix(edit_param, dt) @ translate(-c, dt)).astype(dt)


def project(depth_n, pose, focal=FOCAL, dt=np.float64):
    """cam2pixel_vanilla(norm_scale=True, return_z=True) -> t_coords [S, S, 3] = (X_norm, Y_norm, Z) and the clamp's mask"""
    S = depth_n.shape[0]
    cam = lift(depth_n.astype(dt), focal, dt)
    P = np.asarray(pose, dt)
    p = cam @ P[:3, :3].T + P[:3, 3]
    f, c = dt(focal), dt(S / 2.0)
    X, Y = f * p[..., 0] + c * p[..., 2], f * p[..., 1] + c * p[..., 2]
    Z = np.maximum(p[..., 2], dt(1e-3))
    t = np.stack([2 * (X / Z) / dt(S - 1) - 1, 2 * (Y / Z) / dt(S - 1) - 1, Z], -1).astype(dt)
    return t, p[..., 2] <= 1e-3


def denormalise(t_xy, S):
    """get_3d_transform_correspondence.py:55-69"""
    return (np.asarray(t_xy)[..., :2] + 1.0) / 2.0 * (S - 1)


def faces(obj):
    """get_coordinate_array + create_triangles (warp_utils.py:304-362): [F, 3] indices into the object's pixels in row-major order; all (tl, tr, bl)
    triangles first, then all (bl, tr, br)"""
    S = obj.shape[0]
    m = np.full(obj.shape, -1, np.int64)
    m[obj] = np.arange(int(obj.sum()))
    tl, tr, bl, br = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
    f = np.concatenate([np.stack([tl, tr, bl], 0).reshape(3, -1), np.stack([bl, tr, br], 0).reshape(3, -1)], 1)
    return f[:, f.min(0) > -1].T


# ---- the two rasterisers --------------------------------------------------------------------------------------------------
def pixel_centres(S, dt):
    """pytorch3d's NDC pixel centres in the frame of t_coords (x right, y down): pixel col sits at (2 col + 1) / S - 1"""
    return ((2 * np.arange(S).astype(dt) + 1) / dt(S) - 1).astype(dt)


def splat(tcoords, feats, radius_px=RADIUS, tau=TAU, K=KPP, dt=np.float64, return_ambiguous=False):
    """RasterizePointsXYsBlending.forward (warp_utils.py:72-176) before its fp16 rounding: -> ids int [S, S, K] (-1 = empty), out dt [S, S, C],
    and on request the pixels whose selection single precision may change: a candidate with |d2 - r2| <= eps_d, or two of the K + 1 nearest with
    0 < |dz| <= eps_z.  eps_d = MARGIN * 6 r U32: a pixel centre and a point coordinate of magnitude < 2 carry up to 2 U32 between them in dx (and dy),
    so d2 = dx^2 + dy^2 carries 2 (|dx| + |dy|) 2 U32 <= 4 sqrt(2) r U32 < 6 r U32.  eps_z = MARGIN * spacing(z) (z is an input of the selection:
    read, never recomputed)."""
    t = np.asarray(tcoords).astype(dt)
    S = t.shape[0]
    N = S * S
    px, py, pz = t[..., 0].reshape(N), t[..., 1].reshape(N), t[..., 2].reshape(N)
    F = np.asarray(feats).reshape(N, -1).astype(dt)
    r = dt(radius_px) / dt(S) * dt(2.0)
    r2 = r * r
    cen = pixel_centres(S, dt)
    ids = np.full((S, S, K), -1, np.int64)
    out = np.zeros((S, S, F.shape[1]), dt)
    amb = np.zeros((S, S), bool)
    eps_d = MARGIN * 6 * float(r) * U32
    order_all = np.lexsort((np.arange(N), pz))                   # by z, ties by id
    pxs, pys, pzs = px[order_all], py[order_all], pz[order_all]
    front = pzs >= 0
    for row in range(S):
        dy = cen[row] - pys
        for col in range(S):
            dx = cen[col] - pxs
            d2 = dx * dx + dy * dy
            hit = np.nonzero((d2 < r2) & front)[0]               # already in compositing order
            if return_ambiguous:
                near = np.abs(d2.astype(np.float64) - float(r2)) <= eps_d
                zz = pzs[hit[:K + 1]].astype(np.float64)
                dz = np.diff(zz)
                tight = (dz > 0) & (dz <= MARGIN * np.spacing(np.abs(zz[1:]).astype(np.float32)).astype(np.float64))
                amb[row, col] = bool((near & front).any() or tight.any())
            hit = hit[:K]
            ids[row, col, :hit.size] = order_all[hit]
            q = np.clip(d2[hit] / r2, dt(1e-3), dt(1.0))
            a = (1 - np.sqrt(q)) ** dt(tau)
            cum = np.concatenate([[dt(1.0)], np.cumprod(1 - a)[:-1]]).astype(dt)
            out[row, col] = ((cum * a)[:, None] * F[order_all[hit]]).sum(0, dtype=dt)
    return (ids, out, amb) if return_ambiguous else (ids, out)


def edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def mesh_cover(tcoords, obj, dt=np.float64, return_ambiguous=False):
    """splatter_mesh over get_mesh (warp_utils.py:235-298, 364-399): cover[S, S] = the pixel centre is strictly inside a triangle; on request the pixels
    at which some triangle's smallest barycentric coordinate is within eps of 0, i.e. whose decision single precision may change.  eps per triangle:
    an edge function (px - ax)(by - ay) - (py - ay)(bx - ax) of coordinates carrying 2 u each (u = U32 times the largest coordinate magnitude, at
    least 1) carries 2 u L1 with L1 the sum of the four differences' magnitudes; over |area|, times MARGIN."""
    t = np.asarray(tcoords).astype(dt)
    S = t.shape[0]
    v = t.reshape(-1, 3)[obj.reshape(-1)]
    cen = pixel_centres(S, dt)
    PX, PY = np.meshgrid(cen, cen)                               # [row, col]
    cover = np.zeros((S, S), bool)
    amb = np.zeros((S, S), bool)
    for a, b, c in faces(obj):
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = v[a], v[b], v[c]
        if max(az, bz, cz) < 0:
            continue
        area = edge(ax, ay, bx, by, cx, cy)                      # the sign differs from pytorch3d's frame by nothing: both axes flip
        if abs(area) <= 1e-8:
            continue
        ar = edge(cx, cy, ax, ay, bx, by) + dt(1e-8)
        w0, w1, w2 = edge(PX, PY, bx, by, cx, cy) / ar, edge(PX, PY, cx, cy, ax, ay) / ar, edge(PX, PY, ax, ay, bx, by) / ar
        cover |= (w0 > 0) & (w1 > 0) & (w2 > 0)
        if return_ambiguous:
            lo = np.minimum(np.minimum(w0, w1), w2).astype(np.float64)             # > 0 inside; the pixel's decision flips where lo crosses 0
            u = U32 * max(1.0, *(abs(float(q)) for q in (ax, ay, bx, by, cx, cy)))
            ext = float(max(ax, bx, cx) - min(ax, bx, cx) + max(ay, by, cy) - min(ay, by, cy))
            l1 = 2 * ext + np.abs(PX - float(ax)) + np.abs(PY - float(ay))         # bounds the four differences of each of the three edge functions
            amb |= np.abs(lo) <= MARGIN * 2 * u * l1.astype(np.float64) / abs(float(area))
    return (cover, amb) if return_ambiguous else cover


def to_half_u8(x, scale=255.0):
    """`.to(torch.half)` then `.numpy() * 255.0 -> astype(uint8)` (warp_utils.py:176, ui_utils2.py:541, 553-554).  A float16 array times a Python scalar
    stays float16: the product is rounded to fp16 again before the truncation.  Monotone in x."""
    return (np.asarray(x).astype(np.float16) * np.asarray(scale, np.float16)).astype(np.uint8)


def coarse_edit(img, mask, depth, edit_param, background, focal=FOCAL, radius_px=RADIUS, tau=TAU, K=KPP, dt=np.float64):
    """get_transformed_mask -> project_image_latest, and the script's md_mask (get_3d_transform_correspondence.py:233-260).  -> dict"""
    S = depth.shape[0]
    dn = normalise_depth(depth, dt)
    obj = object_mask(dn, mask)
    pose = compose_pose(dn, obj, edit_param, focal, dt)
    t, clamped = project(dn, pose, focal, dt)
    feats = np.concatenate([np.asarray(img).astype(dt) / dt(255.0), np.asarray(mask).astype(dt)[..., None]], -1)
    ids, comp, amb = splat(t, feats, radius_px, tau, K, dt, return_ambiguous=True)
    cover, mesh_amb = mesh_cover(t, obj, dt, return_ambiguous=True)
    p_image = to_half_u8(comp[..., :3])
    tmask = to_half_u8(comp[..., 3], 1.0) / 255.0 > 0.5
    return dict(depth_n=dn, obj=obj, pose=pose, tcoords=t, clamped=clamped, ids=ids, composite=comp, ambiguous=amb, mesh_projected=cover, mesh_ambiguous=mesh_amb,
                target_mask=tmask, coarse=np.where(tmask[..., None], p_image, background).astype(np.uint8), md_mask=cover & ~tmask,
                correspondence=denormalise(t, S))
