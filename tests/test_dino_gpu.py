"""GPU: the DINOv2 feature metrics (FID-DINO, Kernel Distance) through the C ABI: the device image preparation (ffn_resize_pil_bilinear_u8 against PIL itself,
ffn_vit_patch_rows against the torch expressions of ToTensor + Normalize, both bit for bit), HipDinoV2 against the reference's own outputs (G14) and the oracle,
the uint8 entry against the host-prepared one, and the metric drivers end to end."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from test_dino_cpu import G14_CASES, MEAN, STD, g14_inputs, pil_resize  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def relerr(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def host_prepare(images, size=224):
    """the reference's transform on the host (fid_score.py:124): PIL Resize((size, size)), ToTensor, Normalize -- uint8 [B, H, W, 3] -> float [B, 3, size, size]"""
    mean = torch.as_tensor(np.array(MEAN), dtype=torch.float32)
    std = torch.as_tensor(np.array(STD), dtype=torch.float32)
    out = []
    for im in images:
        t = torch.from_numpy(pil_resize(im, size, size)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        out.append(t.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1)))
    return torch.stack(out)


def hub_state(st):
    return {k[len("pretrained."):]: v for k, v in st.items() if k.startswith("pretrained.")}


def special_images(H, W):
    checker = (((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2) * 255).astype(np.uint8)
    return np.stack([np.full((H, W, 3), 255, np.uint8), np.repeat(checker[..., None], 3, axis=2)])


@pytest.mark.parametrize("B,H,W,oh,ow", [(3, 512, 512, 224, 224), (2, 37, 53, 28, 42), (1, 224, 224, 224, 224), (2, 700, 90, 28, 42), (1, 1, 1, 14, 14),
                                         (2, 300, 200, 224, 224)])
def test_resize_equals_pil_bit_for_bit(gpu, B, H, W, oh, ow):
    """random images, an all-255 image and a 0 / 255 checkerboard; destination and scratch inside sentinel-filled buffers that must stay untouched outside"""
    from freefine_amd import ops
    rng = np.random.default_rng(H * 1000 + W)
    for imgs in (rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), special_images(H, W)):
        n = len(imgs)
        pad, n_out, n_scr = 1024, n * oh * ow * 3, n * H * ow * 3
        big = torch.full((n_out + 2 * pad,), 0xA5, dtype=torch.uint8, device=gpu)
        scr = torch.full((n_scr + 2 * pad,), 0x5A, dtype=torch.uint8, device=gpu)
        got = ops.resize_pil_bilinear_u8(torch.from_numpy(imgs).to(gpu), oh, ow, out=big[pad:pad + n_out].view(n, oh, ow, 3), scratch=scr[pad:pad + n_scr])
        torch.cuda.synchronize()
        want = torch.from_numpy(np.stack([pil_resize(im, oh, ow) for im in imgs]))
        assert got.shape == want.shape and torch.equal(got.cpu(), want), (H, W, oh, ow, int((got.cpu() != want).sum()))
        assert (big[:pad] == 0xA5).all() and (big[pad + n_out:] == 0xA5).all(), "bytes outside the destination written"
        assert (scr[:pad] == 0x5A).all() and (scr[pad + n_scr:] == 0x5A).all(), "bytes outside the scratch buffer written"


@pytest.mark.parametrize("B,H,W", [(2, 28, 42), (1, 224, 224)])
def test_patch_rows_equal_im2col_of_the_torch_transform(gpu, B, H, W):
    from freefine_amd import ops
    from freefine_amd.dino import HipDinoEncoder
    img = torch.from_numpy(np.random.default_rng(B + H + W).integers(0, 256, (B, H, W, 3), dtype=np.uint8))
    mean = torch.as_tensor(np.array(MEAN), dtype=torch.float32)
    std = torch.as_tensor(np.array(STD), dtype=torch.float32)
    x = img.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255).sub_(mean.view(1, -1, 1, 1)).div_(std.view(1, -1, 1, 1))
    cols = HipDinoEncoder._im2col(x, 14)
    M, K, ldo = cols.shape[0], 588, 592
    lut = ops.vit_norm_table(MEAN, STD).to(gpu)
    for dt in (torch.float32, torch.bfloat16):
        big = torch.full((M + 3, ldo), 7.0, dtype=dt, device=gpu)
        got = ops.vit_patch_rows(img.to(gpu), lut, 14, ldo, dt, out=big[:M])
        torch.cuda.synchronize()
        assert torch.equal(got[:, :K].cpu(), cols.to(dt)), dt
        assert (got[:, K:] == 0).all(), "pad columns must be zero"
        assert (big[M:] == 7.0).all(), "rows past the end written"


@pytest.mark.parametrize("name,H,W,B", G14_CASES)
def test_forward_vs_reference_golden_and_oracle(gpu, name, H, W, B):
    """HipDinoV2.forward against the reference's own class tokens (G14) and the oracle; the tolerances of tests/test_depth_gpu.py, which holds the same encoder
    to the same kind of quantity: tiny / mini fp32 1e-4 of the output scale, bf16 6e-2; ViT-B/14 2e-4 / 8e-2"""
    from oracle import dpt as OD
    from freefine_amd.dino import HipDinoV2, dinov2_config
    gold = torch.from_numpy(np.load(os.path.join(GOLD, "g14_dinov2_cls.npz"))[f"{name}_{H}x{W}"])
    ocfg, st, x = g14_inputs(name, H, W, B)
    with torch.no_grad():
        ref = OD.vit_features(ocfg, st, x, 1)[0][1]
    tols = ((torch.float32, 2e-4), (torch.bfloat16, 8e-2)) if name == "vitb" else ((torch.float32, 1e-4), (torch.bfloat16, 6e-2))
    for dt, tol in tols:
        net = HipDinoV2(dinov2_config(name), hub_state(st), dtype=dt, device=gpu)
        y = net(x)
        eg, eo = relerr(y, gold), relerr(y, ref)
        print(f"HipDinoV2 {name} {H}x{W} B={B} {dt}: class token vs reference {eg:.2e}, vs oracle {eo:.2e} (|y| max {gold.abs().max():.3f})")
        assert y.shape == (B, ocfg.embed_dim) and y.dtype == torch.float32
        assert eg < tol and eo < tol, (name, dt)
        del net


@pytest.mark.parametrize("shape", [(3, 96, 64, 3), (2, 512, 512, 3)])
def test_features_u8_equals_forward_of_the_host_prepared_tensor_bit_for_bit(gpu, shape):
    """the operand rows are identical and so is every shape after them: any difference is a bug in the device preparation"""
    from freefine_amd.dino import HipDinoV2, dinov2_config
    _, st, _ = g14_inputs("tiny", 224, 224, 1)
    imgs = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
    x = host_prepare(imgs)
    for dt in (torch.float32, torch.bfloat16):
        net = HipDinoV2(dinov2_config("tiny"), hub_state(st), dtype=dt, device=gpu)
        want = net(x)
        for src in (imgs, torch.from_numpy(imgs).to(gpu)):                # host array and device tensor
            got = net.features_u8(src)
            assert got.shape == (shape[0], 128) and torch.equal(got, want), (dt, (got - want).abs().max().item())


def write_metric_tree(tmp_path):
    """150 real PNGs (48 x 64 and 96 x 96 alternating) and 140 generated PNGs (64 x 64), seeded random with the top half darkened by a random factor
    -> (GeoBench result tree, image label, real root)"""
    from PIL import Image
    rng = np.random.default_rng(2024)

    def write(root, n, size_of):
        os.makedirs(root)
        for i in range(n):
            h, w = size_of(i)
            im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            im[:h // 2] = (im[:h // 2] * rng.uniform(0.1, 1.0)).astype(np.uint8)
            Image.fromarray(im).save(os.path.join(root, f"{i:04d}.png"))
    real_root, gen_root = str(tmp_path / "real"), str(tmp_path / "gen")
    write(real_root, 150, lambda i: (48, 64) if i % 2 == 0 else (96, 96))
    write(gen_root, 140, lambda i: (64, 64))
    data = {f"im{j}": {"instances": {"0": {f"s{i}": {"ori_img_path": "unused", "gen": os.path.join(gen_root, f"{i:04d}.png")} for i in range(j * 70, j * 70 + 70)}}}
            for j in range(2)}
    return data, "gen", real_root


def oracle_activations(ocfg, st, files):
    """the oracle's class tokens of the PIL-prepared images, float64 [len(files), C]"""
    from PIL import Image
    from oracle import dpt as OD
    x = host_prepare([np.array(Image.open(p).convert("RGB")) for p in files])
    with torch.no_grad():
        return torch.cat([OD.vit_features(ocfg, st, x[i:i + 50], 1)[0][1] for i in range(0, len(x), 50)]).double().numpy()


def test_metric_drivers_end_to_end(gpu, tmp_path):
    """the tree of write_metric_tree, tiny configuration, batch 32: get_activations within 1e-4 (of the output scale) of the oracle's class tokens on the
    PIL-prepared inputs; the two drivers equal the model-free functions on those activations exactly.  With the oracle alone these inputs give a covariance of
    rank 127 of 128, a finite Frechet distance (1.98) without the eps retry raising, and a finite KD (0.029).  The metric values from HIP and from oracle features are printed,
    not gated: nobody has measured how far a 1e-4 feature deviation moves a Frechet distance."""
    from freefine_amd import metrics as FM
    from freefine_amd.dino import HipDinoV2, dinov2_config
    data, label, real_root = write_metric_tree(tmp_path)
    ocfg, st, _ = g14_inputs("tiny", 224, 224, 1)
    net = HipDinoV2(dinov2_config("tiny"), hub_state(st), dtype=torch.float32, device=gpu)
    real, gen = FM.parse_data(data, label, real_root)
    assert len(real) == 150 and len(gen) == 140
    acts, oracle = [], []
    for files in (real, gen):
        a, o = FM.get_activations(files, net, batch_size=32), oracle_activations(ocfg, st, files)
        e = relerr(torch.from_numpy(a), torch.from_numpy(o))
        print(f"get_activations on {len(files)} files vs oracle class tokens: {e:.2e} of the output scale ({np.abs(o).max():.3f})")
        assert a.shape == (len(files), 128) and a.dtype == np.float64 and e < 1e-4
        acts.append(a)
        oracle.append(o)
    want_fid = FM.frechet_distance(*FM.feature_statistics(acts[0]), *FM.feature_statistics(acts[1]))
    got_fid = FM.calculate_fid_dino(data, label, real_root, net, batch_size=32)
    np.random.seed(5)
    want_kd = FM.kernel_distance(acts[0], acts[1]).mean()
    np.random.seed(5)
    got_kd = FM.calculate_fid_kd(data, label, real_root, net, batch_size=32)
    np.random.seed(5)
    o_fid, o_kd = FM.frechet_distance(*FM.feature_statistics(oracle[0]), *FM.feature_statistics(oracle[1])), FM.kernel_distance(oracle[0], oracle[1]).mean()
    print(f"FID-DINO from HIP features {got_fid:.6f}, from oracle features {o_fid:.6f}; KD from HIP features {got_kd:.6e}, from oracle features {o_kd:.6e}")
    assert got_fid == want_fid and got_kd == want_kd
    assert np.isfinite(got_fid) and np.isfinite(got_kd)
