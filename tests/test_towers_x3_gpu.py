"""GPU: the split-bf16 mode of the metric suite's ViT towers (HipDinoV2, HipDino, HipCLIPVision with x3=True): ffn_vit_patch_rows_pair bit for bit against the
fp32 entry + ffn_split_pair and against the host statement of the pair form, the split-bf16 GEMM and attention routes at the towers' ragged sequence lengths
against fp64, the three towers against their fp64 references within 2 x the error of the split-bf16 emulation (tests/test_towers_x3_cpu.py), the uint8 entries
against the host-prepared ones bit for bit, and the metric drivers and evaluation/metrics/main.py --precision x3 end to end.  All weights are seeded random at a
plausible scale (no checkpoints exist offline)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_consistency_gpu import MASK_VALUES, clip_host_prepare, dino_host_prepare, masked_numpy, reference_scores, write_tree
from test_consistency_cpu import dino16_ref, g15_inputs, vision_case
from test_dino_gpu import host_prepare, write_metric_tree
from test_ops_gpu import X3_ATT_TOL, X3_TOL, pair_value, ref_attention, relerr, rnd
from test_text_native_cpu import scale_err
from test_text_native_gpu import make_qkv, tower_bound
from test_towers_x3_cpu import DINO_CASES, clip_case, dino_case, dino_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def parity_line(line):
    """printed, and appended to the file FFN_TOWER_X3_PARITY_OUT names (how profiles/towers_x3_parity.txt is written)"""
    print(line)
    if os.environ.get("FFN_TOWER_X3_PARITY_OUT"):
        with open(os.environ["FFN_TOWER_X3_PARITY_OUT"], "a") as f:
            f.write(line + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# ffn_vit_patch_rows_pair
# ---------------------------------------------------------------------------------------------------------------------
def pair_layout(v, K):
    """fp32 [M, K] -> bf16 [M, 2K] as include/freefine_hip.h defines the pair form: hi = bf16(v), lo = bf16(v - hi); K % 32 == 0: 128-byte blocks
    [hi(32) | lo(32)], otherwise the planes [hi(K) | lo(K)]"""
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    if K % 32 == 0:
        return torch.stack([hi.reshape(-1, K // 32, 32), lo.reshape(-1, K // 32, 32)], dim=2).reshape(-1, 2 * K)
    return torch.cat([hi, lo], dim=1)


def patch_images(B, H, W, seed):
    checker = np.repeat(((((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2) * 255).astype(np.uint8))[None, ..., None], 3, axis=3)
    return [("random", np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)), ("all 0", np.zeros((B, H, W, 3), np.uint8)),
            ("all 255", np.full((B, H, W, 3), 255, np.uint8)), ("checkerboard", np.repeat(checker, B, axis=0))]


@pytest.mark.parametrize("B,H,W,patch,K", [(2, 28, 42, 14, 608),       # blocked; the last block is half real columns (576 .. 587), half padding
                                            (2, 28, 42, 14, 592),       # planes
                                            (1, 32, 48, 16, 768), (1, 64, 32, 32, 3072),
                                            (3, 14, 14, 14, 608)])      # one patch per image
def test_patch_rows_pair_bit_for_bit(gpu, B, H, W, patch, K):
    """equal to (a) ops.split_pair(ops.vit_patch_rows(fp32, ldo = K)) on the device and (b) the host statement of the pair form of the torch-evaluated transform;
    padding columns zero in both halves; nothing outside the output written"""
    from freefine_amd import ops
    from freefine_amd.dino import IMAGENET_MEAN, IMAGENET_STD, HipDinoEncoder
    lut = ops.vit_norm_table(IMAGENET_MEAN, IMAGENET_STD).to(gpu)
    mean, std = (torch.as_tensor(np.array(t), dtype=torch.float32) for t in (IMAGENET_MEAN, IMAGENET_STD))
    M, Kr, pad = B * (H // patch) * (W // patch), 3 * patch * patch, 1024
    for name, imgs in patch_images(B, H, W, B * 1000 + H + W + K):
        img = torch.from_numpy(imgs)
        big = torch.full((M * 2 * K + 2 * pad,), -7.0, dtype=torch.bfloat16, device=gpu)
        got = ops.vit_patch_rows_pair(img.to(gpu), lut, patch, K, out=big[pad:pad + M * 2 * K].view(M, 2 * K))
        torch.cuda.synchronize()
        assert ops.pair_width(got) == K and got.shape == (M, 2 * K) and got.dtype == torch.bfloat16
        assert (big[:pad] == -7.0).all() and (big[pad + M * 2 * K:] == -7.0).all(), (name, "elements outside the output written")
        dev = ops.split_pair(ops.vit_patch_rows(img.to(gpu), lut, patch, K, torch.float32), K)
        assert torch.equal(got.view(torch.int16), dev.view(torch.int16)), (name, "differs from vit_patch_rows + split_pair")
        x = img.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255).sub_(mean.view(1, -1, 1, 1)).div_(std.view(1, -1, 1, 1))
        v = torch.zeros(M, K)
        v[:, :Kr] = HipDinoEncoder._im2col(x, patch)
        assert torch.equal(got.cpu().view(torch.int16), pair_layout(v, K).view(torch.int16)), (name, "differs from the host statement")
        if K > Kr:                                            # the padding columns, located by the layout: zero in both halves
            mark = torch.zeros(M, K)
            mark[:, Kr:] = 1.0
            where = pair_layout(mark, K) != 0                 # hi positions of the padding columns; lo positions are 32 (or K) further
            hi_pos = where.nonzero()
            assert len(hi_pos) == M * (K - Kr)
            g = got.cpu().float()
            off = 32 if K % 32 == 0 else K
            assert (g[hi_pos[:, 0], hi_pos[:, 1]] == 0).all() and (g[hi_pos[:, 0], hi_pos[:, 1] + off] == 0).all(), name


# ---------------------------------------------------------------------------------------------------------------------
# the GEMM shapes the towers add, in split-bf16 arithmetic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(2, 257), (4, 50)])
@pytest.mark.parametrize("C", [768, 128])
def test_tower_gemm_shapes_vs_fp64(gpu, C, B, S):
    """M = B S ragged rows through every GEMM of a tower block and the patch embedding, against fp64 within the project's per-op split-bf16 bound X3_TOL"""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(C + S)
    dt, M = torch.float32, B * S
    x = rnd((B, S, C), dt, gpu, g)
    x64 = x.double().cpu()
    pk = lambda w: ops.pack_linear(w, dt, x3=True)

    def wb(N, K):
        return rnd((N, K), dt, gpu, g, K ** -0.5), rnd((N,), dt, gpu, g)
    xp = ops.split_pair(x, C)                                  # what layernorm(pair=True) hands the GEMMs
    # q | k
    w, b = wb(2 * C, C)
    e = relerr(ops.linear(xp, pk(w), b, K=C), x64 @ w.double().cpu().t() + b.double().cpu())
    assert e < X3_TOL, ("qk", e)
    # V^T: transposed output into a zeroed padded buffer whose padding must stay zero
    w, b = wb(C, C)
    ld = (S + 7) // 8 * 8
    assert ld > S
    vt = torch.zeros(B, C, ld, device=gpu)
    ops.linear(xp, pk(w), b, K=C, rows_per_batch=S, transposed_ld=ld, out=vt)
    torch.cuda.synchronize()
    e = relerr(vt[:, :, :S], (x64 @ w.double().cpu().t() + b.double().cpu()).transpose(1, 2))
    assert e < X3_TOL and (vt[:, :, S:] == 0).all(), ("V^T", e)
    # fc1 with GELU and with quick-GELU into pair rows
    w, b = wb(4 * C, C)
    y = x64 @ w.double().cpu().t() + b.double().cpu()
    for kw, ref in ((dict(gelu=True), F.gelu(y)), (dict(qgelu=True), y * torch.sigmoid(1.702 * y))):
        h = ops.linear(xp, pk(w), b, K=C, out_pair=True, **kw)
        assert ops.pair_width(h) == 4 * C and h.shape == (B, S, 8 * C)
        e = relerr(pair_value(h, 4 * C), ref)
        assert e < X3_TOL, (kw, e)
    # fc2 with the fp32 residual, from the pair rows fc1 wrote
    w2, b2 = wb(C, 4 * C)
    hv = pair_value(h, 4 * C).cpu()                            # the operand the device holds (hi + lo)
    e = relerr(ops.linear(h, pk(w2), b2, K=4 * C, residual=x), hv @ w2.double().cpu().t() + b2.double().cpu() + x64)
    assert e < X3_TOL, ("fc2", e)
    # the patch embedding at patch 14: K = 608 pair rows whose last 20 columns are zero, positional embedding as the residual
    a = rnd((M, 608), dt, gpu, g)
    a[:, 588:] = 0
    w, b = wb(C, 608)
    res = rnd((M, C), dt, gpu, g)
    e = relerr(ops.linear(ops.split_pair(a, 608), pk(w), b, K=608, residual=res), a.double().cpu() @ w.double().cpu().t() + b.double().cpu() + res.double().cpu())
    assert e < X3_TOL, ("patch embedding", e)


# ---------------------------------------------------------------------------------------------------------------------
# the non-causal split-bf16 attention at the towers' sequence lengths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [50, 197, 257])
def test_noncausal_x3_attention_vs_fp64(gpu, S):
    """S = 50 (CLIP ViT-B/32), 197 (ViT-B/16), 257 (ViT-B/14 at 224: a second 256-query workgroup with one query); heads 12 and 2, B in {1, 3}; fp32 output and
    pair rows (decoded)"""
    from freefine_amd import ops
    worst = 0.0
    for heads in (12, 2):
        for B in (1, 3):
            qk, vt, q, k, v = make_qkv(B, S, heads, "x3", gpu, 100 * S + 10 * heads + B)
            C = heads * 64
            for out_pair in (False, True):
                out = ops.attention(qk, qk[..., C:], vt, heads, 0.125, None, Sk=S, C=C, x3=True, out_pair=out_pair)
                torch.cuda.synchronize()
                if out_pair:
                    assert ops.pair_width(out) == C and out.shape == (B, S, 2 * C) and out.dtype == torch.bfloat16
                    out = pair_value(out, C)
                assert out.shape == (B, S, C)
                for b in range(B):
                    e = relerr(out[b], ref_attention(q[b], k[b], v[b], heads, 0.125))
                    worst = max(worst, e)
                    assert e < X3_ATT_TOL, (S, heads, B, b, out_pair, e)
    print(f"non-causal split-bf16 attention S={S}: worst {worst:.2e} (tolerance {X3_ATT_TOL:.1e})")


# ---------------------------------------------------------------------------------------------------------------------
# the towers
# ---------------------------------------------------------------------------------------------------------------------
def build_dino(kind, cfg, st, gpu, **kw):
    from freefine_amd.dino import HipDino, HipDinoV2
    return (HipDinoV2 if kind == "g14" else HipDino)(cfg, st, device=gpu, **kw)


@pytest.mark.parametrize("kind,name,H,W,B", DINO_CASES)
def test_dino_towers_x3_vs_oracle_fp64(gpu, kind, name, H, W, B):
    """HipDinoV2(x3=True) on the G14 cases, HipDino(x3=True) on the G15 cases, against the oracle in fp64; bound = 2 x the error of the split-bf16 emulation of the
    same case (tower_bound of tests/test_text_native_gpu.py)"""
    cfg, st, x, want, errs = dino_case(kind, name, H, W, B)
    net = build_dino(kind, cfg, st, gpu, x3=True)
    assert net.kpe == (608 if cfg.patch == 14 else 768) and build_dino(kind, cfg, st, gpu).kpe == (592 if cfg.patch == 14 else 768)
    out = net(x)
    assert out.shape == (B, cfg.embed_dim) and out.dtype == torch.float32
    e, bound = scale_err(out, want), tower_bound(errs, "x3")
    line = f"{'DINOv2' if kind == 'g14' else 'DINO'} tower {name} {H}x{W} B={B} x3: error {e:.3e} of the output maximum ({want.abs().max():.3f}); bound {bound:.3e} " + \
           "(reference errors: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + ")"
    parity_line(line)
    assert e <= bound, line
    with pytest.raises(ValueError, match="x3"):
        build_dino(kind, cfg, st, gpu, dtype=torch.bfloat16, x3=True)


@pytest.mark.parametrize("name", ["tiny", "vitb32"])
def test_clip_tower_x3_vs_transformers_fp64(gpu, name):
    """HipCLIPVision(x3=True), B = 4, against CLIPVisionModelWithProjection.double(); the same bound"""
    from freefine_amd.clipvision import HipCLIPVision
    cfg, st, x, want, errs = clip_case(name)
    out = HipCLIPVision(cfg, st, dtype=torch.float32, device=gpu, x3=True)(x)
    assert out.shape == want.shape and out.dtype == torch.float32
    e, bound = scale_err(out, want), tower_bound(errs, "x3")
    line = f"CLIP vision tower {name} x3: error {e:.3e} of the output maximum ({want.abs().max():.3f}); bound {bound:.3e} (reference errors: " + \
           ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + ")"
    parity_line(line)
    assert e <= bound, line
    with pytest.raises(ValueError, match="x3"):
        HipCLIPVision(cfg, st, dtype=torch.bfloat16, device=gpu, x3=True)


# ---------------------------------------------------------------------------------------------------------------------
# features_u8 in split-bf16 mode: the pair rows straight from the bytes feed the patch GEMM the bytes ops.linear splits from the host-prepared tensor
# ---------------------------------------------------------------------------------------------------------------------
def test_dinov2_features_u8_x3_equals_forward_bit_for_bit(gpu):
    shape = (3, 96, 64, 3)
    cfg, st, *_ = dino_case("g14", "tiny", 224, 224, 2)
    net = build_dino("g14", cfg, st, gpu, x3=True)
    imgs = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
    want = net(host_prepare(imgs))
    for src in (imgs, torch.from_numpy(imgs).to(gpu)):
        got = net.features_u8(src)
        assert got.shape == (shape[0], 128) and torch.equal(got, want), (got - want).abs().max().item()


@pytest.mark.parametrize("shape", [(3, 64, 96, 3), (2, 64, 100, 3)])
def test_dino_features_u8_x3_equals_forward_bit_for_bit(gpu, shape):
    cfg, st, *_ = dino_case("g15", "tiny16", 224, 224, 2)
    net = build_dino("g15", cfg, st, gpu, x3=True)
    rng = np.random.default_rng(shape[2])
    imgs = rng.integers(0, 256, shape, dtype=np.uint8)
    m1 = MASK_VALUES[rng.integers(0, 7, shape[:3])]
    for keep, src in ((None, imgs), (("gt128", m1, None), masked_numpy(imgs, "gt128", m1, None))):
        want = net(dino_host_prepare(src))
        got = net.features_u8(imgs, keep=keep)
        assert got.shape == (shape[0], 128) and torch.equal(got, want), (keep is not None, (got - want).abs().max().item())


@pytest.mark.parametrize("shape", [(3, 64, 96, 3), (2, 90, 64, 3)])
def test_clip_features_u8_x3_equals_forward_bit_for_bit(gpu, shape):
    from freefine_amd.clipvision import HipCLIPVision
    cfg, st, *_ = vision_case("tiny")
    net = HipCLIPVision(cfg, st, dtype=torch.float32, device=gpu, x3=True)
    rng = np.random.default_rng(shape[1])
    imgs = rng.integers(0, 256, shape, dtype=np.uint8)
    m1, m2 = MASK_VALUES[rng.integers(0, 7, shape[:3])], MASK_VALUES[rng.integers(0, 7, shape[:3])]
    for keep, src in ((None, imgs), (("sum_lt128", m1, m2), masked_numpy(imgs, "sum_lt128", m1, m2))):
        want = net(clip_host_prepare(src))
        got = net.features_u8(imgs, keep=keep)
        assert got.shape == (shape[0], 64) and torch.equal(got, want), (keep is not None, (got - want).abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return write_tree(str(tmp_path_factory.mktemp("consistency_x3")))


@pytest.fixture(scope="module")
def tiny_x3(gpu):
    """the tiny CLIP and DINO ViT-B/16 towers in split-bf16 mode beside their fp64 references on PIL-prepared images"""
    from transformers import CLIPVisionModelWithProjection
    from freefine_amd import clipvision as CV
    from freefine_amd.dino import HipDino
    ccfg, cst, *_ = vision_case("tiny")
    dcfg, dst, _ = g15_inputs("tiny16", 224, 224, 1)
    mod = CLIPVisionModelWithProjection(CV.transformers_vision_config(ccfg)).eval()
    mod.load_state_dict(cst, strict=True)
    mod = mod.double()

    def clip64(im):
        with torch.no_grad():
            return mod(pixel_values=clip_host_prepare([im]).double()).image_embeds[0]

    def dino64(im):
        return dino16_ref(dcfg, dst, dino_host_prepare([im]).double())[0]
    return dict(bgc=(CV.HipCLIPVision(ccfg, cst, dtype=torch.float32, device=gpu, x3=True), clip64),
                subc=(HipDino(dcfg, dst, dtype=torch.float32, device=gpu, x3=True), dino64), states=(cst, dst))


@pytest.mark.parametrize("kind", ["bgc", "subc"])
def test_consistency_drivers_x3(gpu, tree, tiny_x3, kind):
    """the 12-pair tree of tests/test_consistency_gpu.py with the tiny towers in split-bf16 mode: every per-pair cosine within 1e-4 (that file's bound for this
    quantity) of the same arithmetic on fp64-reference features; the driver's mean is the mean of those"""
    from freefine_amd import metrics as FM
    data, label, _ = tree
    net, ref_fn = tiny_x3[kind]
    pairs = FM.consistency_pairs(data, label)
    assert len(pairs) == 12
    ref = reference_scores(pairs, kind, ref_fn)
    assert all(c > 0.05 for c in ref), ref
    got = FM.consistency_scores(pairs, net, kind, batch_size=4)
    for i, (r, s) in enumerate(zip(ref, got)):
        print(f"{kind} x3 pair {i:2d}: reference {r:.7f}  split-bf16 {s:.7f} ({abs(s - r):.1e})")
    assert all(abs(s - r) <= 1e-4 for s, r in zip(got, ref))
    fn = FM.calculate_bgc if kind == "bgc" else FM.calculate_subc
    assert fn(data, label, net, batch_size=4) == sum(got) / len(got)


def test_get_activations_x3_vs_oracle(gpu, tmp_path):
    """the PNG tree of tests/test_dino_gpu.py (real images of two sizes) through get_activations with a tiny HipDinoV2(x3=True): the rows of a subset of both
    sizes within the tower bound (2 x the split-bf16 emulation's error on the same PIL-prepared inputs) of the oracle's fp64 class tokens.  FID-DINO and KD are
    printed beside the fp32 model's, not gated."""
    from PIL import Image
    from oracle import dpt as OD
    from test_dino_cpu import g14_inputs
    from freefine_amd import metrics as FM
    data, label, real_root = write_metric_tree(tmp_path)
    cfg, st, *_ = dino_case("g14", "tiny", 224, 224, 2)
    ocfg, full, _ = g14_inputs("tiny", 224, 224, 2)
    net = build_dino("g14", cfg, st, gpu, x3=True)
    real, gen = FM.parse_data(data, label, real_root)
    acts = [FM.get_activations(files, net, batch_size=32) for files in (real, gen)]
    assert acts[0].shape == (150, 128) and acts[1].shape == (140, 128) and acts[0].dtype == np.float64
    pick = sorted(range(len(real)), key=lambda i: real[i])[:6]                     # 48 x 64 and 96 x 96 alternate
    x = host_prepare([np.array(Image.open(real[i]).convert("RGB")) for i in pick] + [np.array(Image.open(p).convert("RGB")) for p in gen[:4]])
    with torch.no_grad():
        want = OD.vit_features(ocfg, full, x.double(), 1)[0][1]
    bound = 2 * scale_err(dino_ref(cfg, st, x, "x3"), want)
    e = scale_err(torch.from_numpy(np.concatenate([acts[0][pick], acts[1][:4]])), want)
    print(f"get_activations x3 on {len(x)} files of {len(set(Image.open(real[i]).size for i in pick)) + 1} sizes vs oracle fp64 class tokens: {e:.3e} of the output "
          f"maximum ({want.abs().max():.3f}); bound {bound:.3e}")
    assert e <= bound
    f32 = build_dino("g14", cfg, st, gpu)
    for nm, m in (("x3", net), ("f32", f32)):
        np.random.seed(5)
        print(f"FID-DINO {nm} {FM.calculate_fid_dino(data, label, real_root, m, batch_size=32):.6f}  KD {nm} {FM.calculate_fid_kd(data, label, real_root, m, batch_size=32):.6e}")


def test_main_driver_precision_as_a_child_process(gpu, tree, tiny_x3, tmp_path):
    """--precision x3 prints BGC and SUBC (the values of the split-bf16 towers); without the flag the output is --precision f32's, line for line"""
    from freefine_amd import metrics as FM
    data, label, jpath = tree
    cst, dst = tiny_x3["states"]
    cw, dw = str(tmp_path / "clip_tiny.pt"), str(tmp_path / "dino_tiny16.pt")
    torch.save(cst, cw)
    torch.save(dst, dw)
    base = [sys.executable, os.path.join(ROOT, "evaluation", "metrics", "main.py"), "--path", jpath, "--task", "000110000", "--clip_weights", cw, "--dino_weights", dw,
            "--clip_config", "tiny", "--dino_config", "tiny16"]
    outs = {}
    for nm, extra in (("x3", ["--precision", "x3"]), ("f32", ["--precision", "f32"]), ("default", [])):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        print(nm, r.stdout[-1000:], r.stderr[-2000:])
        assert r.returncode == 0, nm
        outs[nm] = r.stdout
    assert outs["default"] == outs["f32"]
    vals = {nm: dict(line.split(": ", 1) for line in o.split("-----Result-----")[1].strip().splitlines()) for nm, o in outs.items()}
    assert list(vals["x3"]) == ["BGC", "SUBC"]
    want = {"BGC": FM.calculate_bgc(data, label, tiny_x3["bgc"][0]), "SUBC": FM.calculate_subc(data, label, tiny_x3["subc"][0])}
    for k in vals["x3"]:
        assert abs(float(vals["x3"][k]) - want[k]) <= 1e-6 and 0.05 < float(vals["x3"][k]) <= 1.0, (k, vals["x3"][k], want[k])
