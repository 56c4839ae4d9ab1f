"""CPU: the host side of the Mean Distance metric (freefine_amd/metrics.py): the coordinate maps against the REFERENCE's own get_transform_coordinates
(tests/golden/g13_md_coords.npz, recorded by tools/gen_golden.py run_g13: translation and uniform scale), the rotation branch against the documented matrix
formula, the default keypoint sampler, the reference's import path, and the host-side validation of ffn_dift_match (nothing is launched)."""
import os

import numpy as np

from freefine_amd import metrics as FM

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_md_coords.npz"))


def test_transform_coordinates_translation_and_scale_vs_reference():
    mask = G["mask"]
    for name in ("trans_a", "trans_b"):
        got = FM.transform_coordinates(list(G[f"{name}_param"]), mask.shape, mask)
        assert got.dtype == np.float64 and np.array_equal(got, G[f"{name}_coords"]), name
    for name in ("scale_a", "scale_b"):
        got = FM.transform_coordinates(list(G[f"{name}_param"]), mask.shape, mask)
        assert got.shape == G[f"{name}_coords"].shape and np.abs(got - G[f"{name}_coords"]).max() <= 1e-12, name
    # the translation is (row + dy, col + dx)
    got = FM.transform_coordinates([3, -2, 0, 0, 0, 0, 1, 1, 1], (12, 10), mask)
    assert tuple(got[4, 5]) == (4 - 2, 5 + 3)


def test_transform_coordinates_rotation_is_the_documented_matrix_about_the_mask_centre():
    from scipy.ndimage import center_of_mass
    from src.utils.vis_utils import _rotation_matrix_2d
    mask = np.zeros((9, 14))
    mask[1:5, 6:13] = 1.0
    angle = 30.0
    got = FM.transform_coordinates([0, 0, 0, 0, 0, angle, 1, 1, 1], mask.shape, mask)
    M = _rotation_matrix_2d(center_of_mass(mask), angle, 1.0)        # the (row, col) centre of mass goes in as the matrix centre unchanged
    assert got.shape == (9, 14, 2)
    for r, c in ((0, 0), (3, 9), (8, 13), (2, 11)):
        want = M @ np.array([r, c, 1.0])                             # points are (row, col, 1) . M^T
        assert np.abs(got[r, c] - want).max() <= 1e-12
    cr, cc = center_of_mass(mask)                                    # the centre is the fixed point of the map
    fix = M @ np.array([cr, cc, 1.0])
    assert np.abs(fix - np.array([cr, cc])).max() <= 1e-12


def test_transform_coordinates_reads_the_correspondence_file_reversed(tmp_path):
    arr = np.random.default_rng(0).standard_normal((5, 4, 2))
    np.save(tmp_path / "c.npy", arr)
    got = FM.transform_coordinates([0, 0, 0, 0, 0, 0, 1, 1, 1], (5, 4), np.ones((5, 4)), str(tmp_path / "c.npy"))
    assert np.array_equal(got, arr[..., ::-1])


def test_default_keypoint_sampler():
    full = FM.default_keypoints(np.ones((12, 10)), 30)               # 120 pixels, every 4th in row-major order
    assert full.shape == (30, 2) and full[0].tolist() == [0, 0] and full[1].tolist() == [0, 4] and full[3].tolist() == [1, 2]
    flat = full[:, 0] * 10 + full[:, 1]
    assert np.all(np.diff(flat) == 4)
    assert FM.default_keypoints(np.ones((7, 7)), 30).shape[0] <= 30   # 49 pixels: stride 2 -> 25 points
    empty = FM.default_keypoints(np.zeros((12, 10)), 30)
    assert empty.shape == (0, 2)
    m = np.zeros((12, 10))
    m[3, 4], m[3, 5], m[9, 1] = 1.0, 0.5, 0.7                        # >= 0.5 counts
    m[0, 0] = 0.49
    assert FM.default_keypoints(m, 30).tolist() == [[3, 4], [3, 5], [9, 1]]
    # an empty mask: the case contributes nothing and the featurizer is never asked (the reference's `continue`)
    img = np.zeros((12, 10, 3), dtype=np.uint8)
    assert FM.mean_distance(None, img, img, np.zeros((12, 10), dtype=np.uint8), [1, 0, 0, 0, 0, 0, 1, 1, 1], "x",
                            lambda s, g, mk: FM.default_keypoints(mk)) == []


def test_reference_import_path():
    from evaluation.metrics.MD.mean_distance import calculate_md
    assert calculate_md is FM.calculate_md


def test_dift_match_arguments_are_checked_on_the_host():
    """ffn_dift_match refuses, before any launch: channels that are no multiple of 4, a keypoint outside the image, a workspace that is too small; and
    ffn_dift_workspace_bytes covers the low-resolution tables (no GPU needed)."""
    import ctypes
    from freefine_amd import _lib
    lib = _lib.load()
    C, h, w, K = 64, 5, 7, 3
    need = lib.ffn_dift_workspace_bytes(C, h, w, K)
    assert need >= 4 * (h * w * C + K * C + 5 * h * w + K + K * h * w)
    assert lib.ffn_dift_workspace_bytes(6, h, w, K) == -22
    kps = (ctypes.c_int * (2 * K))(0, 0, 39, 55, 3, 4)

    def desc(**kw):
        d = _lib.DiftDesc()
        d.src = d.tgt = d.ws = d.out_rc = d.out_cos = 0x10000          # never dereferenced: validation fails first
        d.kps = ctypes.addressof(kps)
        d.ws_bytes, d.es = need, h * w * C
        d.dtype, d.E, d.C, d.ld, d.h, d.w, d.H, d.W, d.K = _lib.FFN_F32, 2, C, C, h, w, 40, 56, K
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for d, msg in ((desc(C=62, ld=62), b"C % 4"), (desc(H=39), b"keypoint 1"), (desc(ws_bytes=need - 4), b"workspace"), (desc(ld=60), b"ld=60"),
                   (desc(dtype=_lib.FFN_BF16X3), b"dtype"), (desc(K=0), b"bad shape")):
        assert lib.ffn_dift_match(None, ctypes.byref(d)) == -22
        assert msg in lib.ffn_last_error(), lib.ffn_last_error()
