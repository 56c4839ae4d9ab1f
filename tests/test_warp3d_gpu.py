"""GPU: the point-cloud warp on the HIP kernels (freefine_amd/warp3d.py -> csrc/splat.h through the C ABI) against the numpy restatement
oracle/warp3d.py of geo_utils.py:427-528 (PARITY UNPINNED: pytorch3d absent -- both restate its published semantics) and against the
domain invariants the CPU tests hold the oracle to.  tests/test_splat_gpu.py holds the five kernels to fp64 one by one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _case(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    depth = (2.0 + rng.random((h, w))).astype(np.float32)
    mask = np.zeros((h, w), np.uint8)
    mask[h // 4:3 * h // 4, w // 5:3 * w // 5] = 255
    return img, depth, mask, 0.5 * min(h, w) / np.tan(np.deg2rad(30.0))


@pytest.mark.parametrize("h,w,K,r_px,tf", [
    (48, 48, 5, 0.8, [0, 0, 0, 0, 0, 0, 1, 1, 1]),
    (64, 64, 5, 2.5, [0.2, -0.1, 0.05, 10, 25, -15, 1.0, 1.0, 1.0]),
    (40, 72, 12, 3.0, [-0.3, 0.2, 0.0, 0, 40, 0, 1.2, 0.8, 1.0]),          # non-square image (the longer side's NDC range grows), K on the 16-slot kernel
    (72, 40, 30, 2.0, [0, 0, -0.2, 5, 0, 60, 1.0, 1.0, 1.0]),             # K = 30: the one value at which the reference's own mask test is meaningful
    (96, 96, 8, 6.0, [0.4, 0.4, 0.3, -20, 10, 5, 0.7, 0.7, 0.7]),         # discs spanning several 16 x 16 tiles
])
def test_point_cloud_warp_matches_the_numpy_restatement(monkeypatch, gpu, h, w, K, r_px, tf):
    """Stage by stage, on the operands point_cloud_warp itself hands to the library (recorded by test_splat_gpu.run_entry).  Host side: the centre, the
    translation, the rotation matrix and the scale in the recorded SplatXform against fp64 within derived bounds (S.hold_host_operands).  Lift: the oracle's fp32 lift
    to within two fp32 evaluations of the same formula.  Project: the oracle's fp32 projection to within twice the derived bound of one evaluation plus
    what the two sides' centres, translations and rotation matrices (host arithmetic: torch here, numpy there) differ by.  Splat: the oracle's fp32
    splat of the SAME projected points, outside the pixels the fp64 reference calls ambiguous (a point within the rounding band of the disc's rim; at
    most 1 %) -- coverage and the reference's mask equal, colours within the uint8 truncation.  Comparing the two end-to-end results instead needed
    allowances (n // 500 pixels of coverage, n // 200 of colour): two fp32 projections also swap points whose depths nearly tie, which no band on the
    rim accounts for."""
    from oracle import warp3d as OW
    import test_splat_gpu as S
    img, depth, mask, f = _case(h, w, h + w + K)
    r = r_px * 2.0 / min(h, w)
    (out, ref_mask, cov), pr, rd = S.run_entry(monkeypatch, gpu, lambda W3: W3.point_cloud_warp(img, depth, tf, f, f, mask, True, r, K, device=gpu, return_covered=True))
    # every stage against fp64 of this test's inputs, the host's centre, translation, rotation and scale included: a wrong one fails here
    S.hold_entry_stages(depth, mask > 0, img, f, pr, rd)
    S.hold_host_operands(depth, mask > 0, f, pr, tf, pixel_translation=False)
    # lift and the colours against the oracle
    pts_o, keep = OW.lift(depth, mask, f, f)
    assert pr.n == len(keep) and np.array_equal(rd.rgb, img.reshape(-1, 3).astype(np.float32)[keep])
    assert (np.abs(pr.pts[:, :3] - pts_o) <= 8 * S.U * np.abs(pts_o)).all() and (pr.pts[:, 3] == 0).all()
    # projection
    proj_o, c_o, t_o, R_o, s_o = OW.project(pts_o, tf)
    bound = proj_difference_bound(S, pr, c_o, t_o, R_o)
    assert np.array_equal(pr.X.s, s_o.astype(np.float64)) and proj_o[:, 2].min() > 0.5
    for a in range(3):
        assert (np.abs(pr.proj[:, a].astype(np.float64) - proj_o[:, a]) <= bound[a]).all(), a
    # splat: fp32 oracle and HIP kernel on the same points, fp64 reference for the ambiguous pixels
    image_o, idx_o, _ = OW.splat(pr.proj[:, :3], rd.rgb, h, w, r, K)
    o_out, o_ref_mask, o_cov = image_o.astype(np.uint8), (idx_o.sum(-1) != -30).astype(np.uint8) * 255, (idx_o[..., 0] >= 0).astype(np.uint8) * 255
    band = S.rim_band(w, h, r)
    ref = S.ref_render(pr.proj, rd.rgb, w, h, r, K, band=band)
    sure = ~ref.amb
    print(f"SPLAT warp {h}x{w}: ambiguous {int(ref.amb.sum())} of {ref.amb.size}")
    assert ref.amb.mean() <= S.AMBIGUOUS_CAP
    assert np.array_equal(cov[sure], o_cov[sure]) and np.array_equal(cov[sure], ref.covered[sure] * 255)
    assert np.array_equal(ref_mask[sure], o_ref_mask[sure]) and np.array_equal(ref_mask[sure], ((ref.idx_sum != -30) * 255)[sure])
    assert np.abs(out.astype(int) - o_out.astype(int)).max(-1)[sure].max() <= 1
    S.hold_uint8(out, ref.image, sure, S.image_bound(K, band / float(np.float32(r)) ** 2))
    assert o_cov.sum() > 0 and (out[cov == 0] == 0).all()


def proj_difference_bound(S, pr, c_o, t_o, R_o):
    """-> bounds of |ndc x|, |ndc y|, |z_view| differences between the recorded fp32 projection and the oracle's: each side is within
    S.project_bound of fp64 on its own operands, and the operands differ by d_in (centre, translation, the lifted points, the rotation matrix against
    |q| <= 3M) before the rotation and by the centre after it.  Those operand differences are capped first: the test holds c, t and R to fp64 within
    derived bounds (S.hold_entry_stages, S.hold_host_operands) before it calls this"""
    X = pr.X
    P = pr.pts[:, :3].astype(np.float64)
    M = max(np.abs(P).max(), np.abs(X.c).max(), np.abs(X.t).max())
    d_c = np.abs(X.c - c_o).max()
    d_in = d_c + np.abs(X.t - np.asarray(t_o, np.float64)).max() + 8 * S.U * M + 9 * M * np.abs(X.R - R_o).max()
    d_v = np.abs(X.s) * np.abs(X.R).sum(0) * d_in + d_c
    v = ((P - X.c + X.t) @ X.R) * X.s + X.c
    z = np.abs(v[:, 2])
    bx, by, bz = S.project_bound(pr.pts, X)
    d_n = [(d_v[a] + np.abs(v[:, a]) / z * d_v[2]) / X.tan / z for a in (0, 1)]
    return 2 * bx + d_n[0], 2 * by + d_n[1], 2 * bz + d_v[2]


def test_point_cloud_warp_invariants_and_repeatability(gpu):
    """identity: every lifted corner covers the four pixel centres around it; translation at constant depth = shift; bit-repeatable (the
    tile lists are filled through atomics in any order, the top-K is ordered by (depth, point id))"""
    from freefine_amd import warp3d
    h = w = 64
    img, depth, mask, f = _case(h, w, 1)
    depth[...] = 2.0
    r = 0.8 * 2 / w
    ident = [0, 0, 0, 0, 0, 0, 1, 1, 1]
    base, _, cov0 = warp3d.point_cloud_warp(img, depth, ident, f, f, mask, True, r, 5, device=gpu, return_covered=True)
    m = mask > 0
    u = m.copy()
    u[:, :-1] |= m[:, 1:]
    u[:-1, :] |= m[1:, :]
    u[:-1, :-1] |= m[1:, 1:]
    assert np.array_equal(cov0 > 0, u)
    ext = np.ptp(np.nonzero(m.any(0))[0])                      # object extent in pixels along x
    out, _, cov = warp3d.point_cloud_warp(img, depth, [-5 / ext, 0, 0, 0, 0, 0, 1, 1, 1], f, f, mask, True, r, 5, device=gpu, return_covered=True)
    assert np.array_equal(cov, np.roll(cov0, 5, axis=1))
    assert np.abs(out.astype(int) - np.roll(base, 5, axis=1).astype(int)).max() <= 1
    # translation given in image pixels (the GeoBench edit_param convention of the 3d_rgb variant): +7 px right, +3 px down at constant depth
    outp, _, covp = warp3d.point_cloud_warp(img, depth, [7, 3, 0, 0, 0, 0, 1, 1, 1], f, f, mask, True, r, 5, device=gpu, return_covered=True, pixel_translation=True)
    assert np.array_equal(covp, np.roll(cov0, (3, 7), axis=(0, 1)))
    assert np.abs(outp.astype(int) - np.roll(base, (3, 7), axis=(0, 1)).astype(int)).max() <= 1
    big = [0.1, 0.1, 0, 15, -30, 20, 1.1, 0.9, 1.0]
    a = warp3d.point_cloud_warp(img, 2.0 + 0 * depth, big, f, f, mask, True, 4.0 * 2 / w, 15, device=gpu)     # constant depth: every depth ties
    b = warp3d.point_cloud_warp(img, 2.0 + 0 * depth, big, f, f, mask, True, 4.0 * 2 / w, 15, device=gpu)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # empty mask: black image, nothing covered
    e = warp3d.point_cloud_warp(img, depth, ident, f, f, np.zeros_like(mask), True, r, 5, device=gpu, return_covered=True)
    assert (e[0] == 0).all() and (e[2] == 0).all()
