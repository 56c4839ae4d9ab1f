"""CPU: the host side of the DINOv2 feature metrics (FID-DINO, Kernel Distance): the PIL-bilinear coefficient tables against PIL itself, the ToTensor + Normalize
lookup table against the torch expressions, the metric drivers on a fake model, the reference's import paths, the host-side validation of the two preparation
entry points (nothing is launched), and tests/golden/g14_dinov2_cls.npz (the reference's own DinoVisionTransformer, tools/gen_golden.py run_g14) against
oracle/dpt.py."""
import os

import numpy as np
import pytest
import torch

from freefine_amd import metrics as FM
from freefine_amd import ops

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def rng_tensor(seed, shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def resize_numpy(img, oh, ow):
    """ops.pil_bilinear_coeffs applied in integer arithmetic: horizontal pass, then vertical pass; img uint8 [H, W, 3]"""
    def one_axis(a, n_out):                                   # resamples axis 0
        bounds, coef = ops.pil_bilinear_coeffs(a.shape[0], n_out)
        out = np.empty((n_out,) + a.shape[1:], dtype=np.uint8)
        for i, (lo, n) in enumerate(bounds):
            acc = (1 << 21) + np.tensordot(coef[i, :n].astype(np.int64), a[lo:lo + n].astype(np.int64), axes=(0, 0))
            assert acc.max() < 2 ** 31
            out[i] = np.clip(acc >> 22, 0, 255)
        return out
    h = one_axis(np.ascontiguousarray(img.transpose(1, 0, 2)), ow).transpose(1, 0, 2)
    return one_axis(h, oh)


def pil_resize(img, oh, ow):
    from PIL import Image
    return np.array(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))


# (W, H) -> (ow, oh), as the issue lists them (width x height)
RESIZE_CASES = [((512, 512), (224, 224)), ((37, 53), (224, 224)), ((300, 200), (224, 224)), ((640, 480), (224, 224)), ((224, 224), (224, 224)),
                ((100, 1000), (28, 28))]


@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_pil_bilinear_coeffs_reproduce_pil_bit_for_bit(src, dst):
    (W, H), (ow, oh) = src, dst
    rng = np.random.default_rng(W * 1000 + H)
    checker = (((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2) * 255).astype(np.uint8)
    for name, img in (("random", rng.integers(0, 256, (H, W, 3), dtype=np.uint8)), ("all 255", np.full((H, W, 3), 255, np.uint8)),
                      ("checkerboard", np.repeat(checker[..., None], 3, axis=2))):
        assert np.array_equal(resize_numpy(img, oh, ow), pil_resize(img, oh, ow)), (name, src, dst)


def test_coefficient_tables_shape_identity_and_cache():
    b, k = ops.pil_bilinear_coeffs(224, 224)
    assert k.shape == (224, 3) and np.array_equal(b[:, 0], np.arange(224))
    for i in range(224):                                      # the identity: one tap of 2^22 on the pixel itself
        row = np.zeros(224, dtype=np.int64)
        row[b[i, 0]:b[i, 0] + b[i, 1]] = k[i, :b[i, 1]]
        assert row[i] == 1 << 22 and row.sum() == 1 << 22
    b, k = ops.pil_bilinear_coeffs(700, 28)
    assert k.shape == (28, 51) and b.dtype == k.dtype == np.int32
    assert (k >= 0).all() and np.abs(k.sum(axis=1) - (1 << 22)).max() <= 51 // 2 + 1
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 700).all() and (b[:, 1] <= 51).all()
    assert ops.pil_bilinear_coeffs(700, 28)[1] is k


def test_norm_table_equals_the_transform_on_an_image():
    lut = ops.vit_norm_table(MEAN, STD)
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    img = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (37, 41, 3), dtype=np.uint8))
    # ToTensor: HWC uint8 -> CHW float32 / 255; Normalize: in place - mean[:, None, None], / std[:, None, None] with float32 tensors made from float64 arrays
    t = img.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean = torch.as_tensor(np.array(MEAN), dtype=torch.float32)
    std = torch.as_tensor(np.array(STD), dtype=torch.float32)
    t.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))
    got = torch.stack([lut[c][img[..., c].long()] for c in range(3)])
    assert torch.equal(got, t)


class FakeModel:
    """stands for a HipDinoV2: features_u8 returns per-image checksums and records the batches it saw"""

    def __init__(self):
        self.batches = []

    def features_u8(self, images, size=224):
        images = np.asarray(images)
        assert images.dtype == np.uint8 and images.ndim == 4 and images.shape[-1] == 3
        self.batches.append(images.shape)
        f = images.reshape(len(images), -1).astype(np.float64)
        return torch.from_numpy(np.stack([f.sum(1), f[:, 0], f[:, -1], (f * np.arange(f.shape[1])).sum(1) / f.shape[1]], axis=1).astype(np.float32))


def write_images(root, sizes, seed):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    paths = []
    for i, (h, w) in enumerate(sizes):
        p = os.path.join(root, f"img_{i:03d}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        paths.append(p)
    return paths


def test_get_activations_keeps_file_order_across_sizes_and_partial_batches(tmp_path):
    sizes = [(8, 6), (5, 5), (8, 6), (8, 6), (5, 5), (7, 3), (8, 6), (8, 6), (5, 5), (8, 6), (8, 6)]
    files = write_images(str(tmp_path / "a"), sizes, 1)
    model = FakeModel()
    act = FM.get_activations(files, model, batch_size=3)
    assert act.dtype == np.float64 and act.shape == (len(files), 4)
    one = FakeModel()
    from PIL import Image
    for i, p in enumerate(files):
        img = np.array(Image.open(p).convert("RGB"))
        assert np.array_equal(act[i], one.features_u8(img[None]).double().numpy()[0]), i
    # one launch sees one size; 7 images of 8 x 6 in batches of 3 -> 3 + 3 + 1
    assert sorted(model.batches) == sorted([(3, 8, 6, 3), (3, 8, 6, 3), (1, 8, 6, 3), (3, 5, 5, 3), (1, 7, 3, 3)])
    # a caller's reader is used instead of PIL
    act2 = FM.get_activations(["x", "y"], FakeModel(), batch_size=64, reader=lambda p: np.full((4, 4, 3), 7 if p == "x" else 9, np.uint8))
    assert act2[0, 1] == 7 and act2[1, 1] == 9


def make_tree(tmp_path):
    real = write_images(str(tmp_path / "real"), [(6, 6)] * 9 + [(4, 7)] * 4, 2)
    gen = write_images(str(tmp_path / "gen"), [(5, 5)] * 12, 3)
    other = write_images(str(tmp_path / "other"), [(3, 3)] * 12, 4)
    data = {"im0": {"instances": {"0": {}, "1": {}}}}
    for i, (g, o) in enumerate(zip(gen, other)):
        data["im0"]["instances"][str(i % 2)][f"s{i}"] = {"ori_img_path": o, "gen_img_path": g}
    return data, real, gen


def test_parse_data_uses_the_directory_listing(tmp_path):
    data, real, gen = make_tree(tmp_path)
    r, g = FM.parse_data(data, "gen_img_path", str(tmp_path / "real"))
    assert r == [os.path.join(str(tmp_path / "real"), n) for n in os.listdir(str(tmp_path / "real"))] and sorted(r) == sorted(real)
    assert sorted(g) == sorted(gen) and len(g) == 12
    assert not any("other" in p for p in r)                   # the ori_img_paths are collected and then dropped, as in the reference


def test_fid_dino_and_kd_equal_the_existing_functions_on_the_fake_features(tmp_path):
    data, real, gen = make_tree(tmp_path)
    root = str(tmp_path / "real")
    r, g = FM.parse_data(data, "gen_img_path", root)
    fr, fg = FM.get_activations(r, FakeModel()), FM.get_activations(g, FakeModel())
    want = FM.frechet_distance(*FM.feature_statistics(fr), *FM.feature_statistics(fg))
    assert FM.calculate_fid_dino(data, "gen_img_path", root, FakeModel()) == want
    np.random.seed(11)
    want_kd = FM.kernel_distance(fr, fg).mean()
    np.random.seed(11)
    assert FM.calculate_fid_kd(data, "gen_img_path", root, FakeModel()) == want_kd
    assert np.isfinite(want) and np.isfinite(want_kd)


def test_reference_import_paths():
    from evaluation.metrics.FID.fid_dino import calculate_fid_dino
    from evaluation.metrics.FID.fid_kd import calculate_fid_kd
    assert calculate_fid_dino is FM.calculate_fid_dino and calculate_fid_kd is FM.calculate_fid_kd


def test_dinov2_config_and_state_layout():
    from freefine_amd.depth import depth_config
    from freefine_amd.dino import dinov2_config, dinov2_param_shapes
    for name in ("vitb", "tiny", "mini"):
        c, d = dinov2_config(name), depth_config(name)
        assert (c.embed_dim, c.depth, c.num_heads, c.patch, c.img_size, c.mlp_ratio, c.interpolate_offset, c.ln_eps) == \
               (d.embed_dim, d.depth, d.num_heads, d.patch, d.img_size, d.mlp_ratio, d.interpolate_offset, d.ln_eps)
    with pytest.raises(KeyError):
        dinov2_config("vitx")
    sh = dinov2_param_shapes(dinov2_config("vitb"))
    assert sh["pos_embed"] == (1, 1370, 768) and sh["mask_token"] == (1, 768) and sh["blocks.11.ls2.gamma"] == (768,) and not any(k.startswith("pretrained.") for k in sh)


def test_preparation_entry_points_check_their_arguments_on_the_host():
    """ffn_resize_pil_bilinear_u8 / ffn_vit_patch_rows refuse, before any launch: null pointers, sides beyond FFN_IMGPREP_MAX_SIDE, table widths that do not
    belong to the sizes, images that are not whole patches, a row stride below the patch's columns (no GPU needed: nothing is launched)."""
    from freefine_amd import _lib
    lib = _lib.load()
    P = 0x10000                                               # never dereferenced: validation fails first
    lim = _lib.IMGPREP_MAX_SIDE
    assert lim == 4096

    def resize(src=P, dst=P, scratch=P, B=2, H=512, W=512, oh=224, ow=224, tabs=(P, P, P, P), hks=7, vks=7):
        return lib.ffn_resize_pil_bilinear_u8(None, src, dst, scratch, B, H, W, oh, ow, tabs[0], tabs[1], hks, tabs[2], tabs[3], vks)
    for kw, msg in ((dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(scratch=None), b"null"), (dict(tabs=(P, None, P, P)), b"null"),
                    (dict(H=lim + 1, vks=41), b"outside 1 .. 4096"), (dict(W=lim + 1, hks=41), b"outside 1 .. 4096"), (dict(oh=lim + 1), b"outside 1 .. 4096"),
                    (dict(H=0), b"outside"), (dict(B=0), b"B=0"), (dict(hks=5), b"table widths"), (dict(vks=9), b"table widths")):
        assert resize(**kw) == -22, kw
        assert msg in lib.ffn_last_error() and lib.ffn_last_error().startswith(b"resize_pil_bilinear_u8"), lib.ffn_last_error()

    def rows(dtype=_lib.FFN_F32, src=P, lut=P, out=P, B=2, H=224, W=224, patch=14, ldo=592):
        return lib.ffn_vit_patch_rows(None, dtype, src, lut, out, B, H, W, patch, ldo)
    for kw, msg in ((dict(src=None), b"null"), (dict(lut=None), b"null"), (dict(out=None), b"null"), (dict(H=225), b"whole patches"), (dict(W=200), b"whole patches"),
                    (dict(ldo=587), b"ldo=587"), (dict(H=lim + 14), b"bad shape"), (dict(W=lim + 14), b"bad shape"), (dict(dtype=_lib.FFN_BF16X3), b"dtype"),
                    (dict(patch=0), b"whole patches")):
        assert rows(**kw) == -22, kw
        assert msg in lib.ffn_last_error() and lib.ffn_last_error().startswith(b"vit_patch_rows"), lib.ffn_last_error()


# tools/gen_golden.py run_g14 printed a difference of exactly 0 between the oracle and the reference's DinoVisionTransformer on the recording machine (class tokens
# of scale 3).  fp32 matmuls block differently with another thread count, so the bound is a few ulp of that scale after 12 blocks: the 2e-5 that G8 holds
# the same encoder to (tests/test_oracle_golden.py).
G14_ORACLE_TOL = 2e-5
G14_CASES = [("tiny", 224, 224, 2), ("tiny", 518, 518, 1), ("mini", 224, 224, 2), ("mini", 518, 518, 1), ("vitb", 224, 224, 2)]


def g14_inputs(name, H, W, B):
    """(oracle configuration, full state with the `pretrained.` prefix, input) of one G14 case -- shared with tests/test_dino_gpu.py"""
    from oracle import dpt as OD
    cfg = OD.dpt_config(name)
    st = OD.dpt_synthetic_state(cfg, seed=14 + len(name))
    return cfg, st, rng_tensor(140 + H + len(name), (B, 3, H, W))


@pytest.mark.parametrize("name,H,W,B", G14_CASES)
def test_g14_matches_the_oracle(name, H, W, B):
    from oracle import dpt as OD
    gold = np.load(os.path.join(GOLD, "g14_dinov2_cls.npz"))
    cfg, st, x = g14_inputs(name, H, W, B)
    with torch.no_grad():
        cls = OD.vit_features(cfg, st, x, 1)[0][1]
    want = torch.from_numpy(gold[f"{name}_{H}x{W}"])
    assert want.shape == (B, cfg.embed_dim)
    d = (cls - want).abs().max().item()
    print(f"G14 {name} {H}x{W}: oracle vs reference {d:.3e} (|y|max {want.abs().max():.3f})")
    assert d <= G14_ORACLE_TOL
