"""GPU: Background / Subject Consistency through the C ABI: ffn_resize_pil_u8 against PIL itself, bit for bit (any filter, 1 / 3 channels, crop windows, keep
masks), the non-causal attention at the two towers' sequence lengths against fp64, HipDino against the vendored DinoVisionTransformer's recorded class tokens (G15),
HipCLIPVision against transformers' CLIPVisionModelWithProjection.double(), the uint8 entries against the host-prepared ones, and the metric drivers and
evaluation/metrics/main.py end to end.  All weights are seeded random at a plausible scale (no checkpoints exist offline)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_attention_edges_gpu import TOL as ATT_TOL
from test_consistency_cpu import FILTERS, G15_CASES, RESIZE_CASES, dino16_ref, g15_inputs, pil_resize, sample_images, vision_case
from test_ops_gpu import ref_attention, relerr
from test_text_native_cpu import scale_err
from test_text_native_gpu import make_qkv, tower_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

MASK_VALUES = np.array([0, 100, 127, 128, 129, 200, 255], np.uint8)
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


# ---------------------------------------------------------------------------------------------------------------------
# ffn_resize_pil_u8
# ---------------------------------------------------------------------------------------------------------------------
def run_resize(gpu, imgs, oh, ow, filter, crop=None, keep=None):
    """ops.resize_pil_u8 with destination and scratch inside sentinel-filled buffers, which must stay untouched outside; imgs uint8 [B, H, W, C] or [B, H, W]"""
    from freefine_amd import ops
    B, H = imgs.shape[:2]
    C = 1 if imgs.ndim == 3 else imgs.shape[3]
    y0, x0, ch, cw = crop or (0, 0, oh, ow)
    pad, n_out, n_scr = 1024, B * ch * cw * C, B * H * cw * C
    big = torch.full((n_out + 2 * pad,), 0xA5, dtype=torch.uint8, device=gpu)
    scr = torch.full((n_scr + 2 * pad,), 0x5A, dtype=torch.uint8, device=gpu)
    if keep is not None:
        keep = (keep[0],) + tuple(None if m is None else torch.from_numpy(m).to(gpu) for m in keep[1:])
    got = ops.resize_pil_u8(torch.from_numpy(imgs).to(gpu), oh, ow, filter, crop=crop, keep=keep, out=big[pad:pad + n_out].view((B, ch, cw) + imgs.shape[3:]),
                            scratch=scr[pad:pad + n_scr])
    torch.cuda.synchronize()
    assert (big[:pad] == 0xA5).all() and (big[pad + n_out:] == 0xA5).all(), "bytes outside the destination written"
    assert (scr[:pad] == 0x5A).all() and (scr[pad + n_scr:] == 0x5A).all(), "bytes outside the scratch buffer written"
    return got.cpu().numpy()


def pil_batch(imgs, oh, ow, filter, crop=None):
    y0, x0, ch, cw = crop or (0, 0, oh, ow)
    return np.stack([pil_resize(im, oh, ow, filter)[y0:y0 + ch, x0:x0 + cw] for im in imgs])


def batch_of(H, W, C, B, seed):
    """B random images with the 0 / 255 checkerboard as the last one (B = 1: the checkerboard is a batch of its own)"""
    (_, rnd), (_, checker) = sample_images(H, W, C, seed)
    rng = np.random.default_rng(seed + 1)
    if B == 1:
        return [rnd[None], checker[None]]
    return [np.stack([rnd] + [rng.integers(0, 256, rnd.shape, dtype=np.uint8) for _ in range(B - 2)] + [checker])]


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("src,dst,C0", RESIZE_CASES)
def test_resize_pil_u8_equals_pil_bit_for_bit(gpu, src, dst, C0, filter):
    """every CPU shape, both channel counts, B in {1, 3}"""
    (W, H), (ow, oh) = src, dst
    for C in (1, 3):
        for B in (1, 3):
            for imgs in batch_of(H, W, C, B, W * 1000 + H + C):
                got, want = run_resize(gpu, imgs, oh, ow, filter), pil_batch(imgs, oh, ow, filter)
                assert got.shape == want.shape and np.array_equal(got, want), (src, dst, C, B, filter, int((got != want).sum()))


WINDOWS = [((640, 480), (298, 224), (0, 37, 224, 224)),          # CLIP's centre crop of a 4:3 image
           ((640, 480), (298, 224), (111, 5, 1, 51)),             # one row
           ((53, 37), (42, 28), (3, 7, 9, 1)),                    # one column
           ((100, 64), (350, 224), (0, 0, 224, 336)),             # DINO's floor to whole patches
           ((64, 64), (224, 224), (1, 1, 223, 223))]


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("src,dst,crop", WINDOWS)
def test_crop_windows_at_odd_offsets(gpu, src, dst, crop, filter):
    (W, H), (ow, oh) = src, dst
    for C in (3, 1):
        for imgs in batch_of(H, W, C, 3, W + H + C):
            got, want = run_resize(gpu, imgs, oh, ow, filter, crop=crop), pil_batch(imgs, oh, ow, filter, crop)
            assert got.shape == want.shape and np.array_equal(got, want), (src, dst, crop, C, filter)


def masked_numpy(imgs, rule, m1, m2):
    """the reference's statements: background_consistency.py:22-27 (uint8 sum wraps), subject_consistency.py:20-21"""
    if rule == "sum_lt128":
        mask = m1 + m2 if m2 is not None else m1
        assert mask.dtype == np.uint8
        mask_bool = (mask < 128).astype(np.uint8)
    else:
        mask_bool = (m1 > 128).astype(np.uint8)
    return imgs * mask_bool[..., np.newaxis]


@pytest.mark.parametrize("rule,with_m2", [("sum_lt128", True), ("sum_lt128", False), ("gt128", False), ("gt128", True)])
@pytest.mark.parametrize("src,dst,crop,filter", [((640, 480), (298, 224), (0, 37, 224, 224), "bicubic"), ((53, 37), (42, 28), None, "bilinear"),
                                                  ((96, 64), (336, 224), (0, 0, 224, 336), "bilinear"), ((64, 64), (224, 224), (5, 3, 1, 200), "bicubic")])
def test_keep_masks_equal_pil_on_the_numpy_masked_image(gpu, src, dst, crop, filter, rule, with_m2):
    """mask values drawn from {0, 100, 127, 128, 129, 200, 255}: the wrap (200 + 100 = 44, 128 + 128 = 0, 255 + 129 = 128) and both sides of either threshold"""
    (W, H), (ow, oh) = src, dst
    rng = np.random.default_rng(W * H + len(rule))
    for B in (1, 3):
        imgs = rng.integers(1, 256, (B, H, W, 3), dtype=np.uint8)
        m1, m2 = MASK_VALUES[rng.integers(0, 7, (B, H, W))], (MASK_VALUES[rng.integers(0, 7, (B, H, W))] if with_m2 else None)
        m1[:, 0, :7], m1[:, 1, :7] = MASK_VALUES, MASK_VALUES                      # every value against 128 and against 200 in the first two rows
        if with_m2:
            m2[:, 0, :7], m2[:, 1, :7] = 128, 200
        want_img = masked_numpy(imgs, rule, m1, None if rule == "gt128" else m2)
        assert 0.2 < (want_img == 0).all(-1).mean() < 0.8
        got = run_resize(gpu, imgs, oh, ow, filter, crop=crop, keep=(rule, m1, m2))
        want = pil_batch(want_img, oh, ow, filter, crop)
        assert np.array_equal(got, want), (src, dst, crop, filter, rule, with_m2, B, int((got != want).sum()))
        if rule == "sum_lt128" and with_m2:                   # the wrap matters: a sum that does not wrap gives another image
            nowrap = imgs * ((m1.astype(np.int64) + m2) < 128)[..., None].astype(np.uint8)
            assert not np.array_equal(pil_batch(nowrap, oh, ow, filter, crop), want)


def test_the_old_entry_is_unchanged_beside_the_new_one(gpu):
    from freefine_amd import ops
    imgs = np.random.default_rng(5).integers(0, 256, (2, 300, 200, 3), dtype=np.uint8)
    old = ops.resize_pil_bilinear_u8(torch.from_numpy(imgs).to(gpu), 224, 224).cpu().numpy()
    new = run_resize(gpu, imgs, 224, 224, "bilinear")
    want = pil_batch(imgs, 224, 224, "bilinear")
    assert np.array_equal(old, want) and np.array_equal(new, want)


# ---------------------------------------------------------------------------------------------------------------------
# the non-causal attention at the towers' sequence lengths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("S", [50, 197])
def test_noncausal_attention_vs_fp64(gpu, mode, S):
    """S = 50 (CLIP ViT-B/32 at 224) and 197 (ViT-B/16 at 224), heads 12 and 2, B in {1, 3}; bf16 against the bf16-rounded inputs"""
    from freefine_amd import ops
    worst = 0.0
    for heads in (12, 2):
        for B in (1, 3):
            qk, vt, q, k, v = make_qkv(B, S, heads, mode, gpu, 100 * S + 10 * heads + B)
            C = heads * 64
            out = ops.attention(qk, qk[..., C:], vt, heads, 0.125, None, Sk=S, C=C)
            torch.cuda.synchronize()
            assert out.shape == (B, S, C)
            for b in range(B):
                e = relerr(out[b], ref_attention(q[b], k[b], v[b], heads, 0.125))
                worst = max(worst, e)
                assert e < ATT_TOL[mode], (mode, S, heads, B, b, e)
    print(f"non-causal attention S={S} {mode}: worst {worst:.2e} (tolerance {ATT_TOL[mode]:.1e})")


# ---------------------------------------------------------------------------------------------------------------------
# HipDino (DINO ViT-B/16)
# ---------------------------------------------------------------------------------------------------------------------
def normalise(u8, mean, std):
    """ToTensor + Normalize of uint8 [H, W, 3] as torchvision spells them -> float32 [3, H, W]"""
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean, std = torch.as_tensor(np.array(mean), dtype=torch.float32), torch.as_tensor(np.array(std), dtype=torch.float32)
    return t.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))


def dino_host_prepare(imgs, size=224, patch=16):
    """subject_consistency.py:11-15 on the host: Resize(224) of the PIL image (short side, BILINEAR), ToTensor, Normalize; then the rows and columns a stride-16
    convolution would not reach are cut"""
    from freefine_amd import ops
    out = []
    for im in imgs:
        oh, ow = ops.torchvision_resize_size(im.shape[0], im.shape[1], size)
        out.append(normalise(pil_resize(im, oh, ow, "bilinear")[:oh // patch * patch, :ow // patch * patch], *IMAGENET))
    return torch.stack(out)


@pytest.mark.parametrize("name,H,W,B", G15_CASES)
def test_hipdino_vs_g15(gpu, name, H, W, B):
    """tests/test_dino_gpu.py's tolerances for the same encoder: tiny 1e-4 fp32 / 6e-2 bf16 of the output scale, ViT-B 2e-4 / 8e-2"""
    from freefine_amd.dino import HipDino
    gold = torch.from_numpy(np.load(os.path.join(GOLD, "g15_dino16_cls.npz"))[f"{name}_{H}x{W}"])
    cfg, st, x = g15_inputs(name, H, W, B)
    tols = ((torch.float32, 2e-4), (torch.bfloat16, 8e-2)) if name == "vitb16" else ((torch.float32, 1e-4), (torch.bfloat16, 6e-2))
    for dt, tol in tols:
        net = HipDino(cfg, st, dtype=dt, device=gpu)
        y = net(x)
        e = relerr(y, gold)
        print(f"HipDino {name} {H}x{W} B={B} {dt}: class token vs reference {e:.2e} (|y| max {gold.abs().max():.3f})")
        assert y.shape == (B, cfg.embed_dim) and y.dtype == torch.float32 and e < tol, (name, dt, e)
        del net


@pytest.mark.parametrize("shape", [(3, 64, 96, 3), (2, 64, 100, 3), (2, 90, 64, 3)])
def test_hipdino_features_u8_equals_forward_of_the_host_prepared_tensor(gpu, shape):
    """non-square images stay non-square: 96 x 64 -> 336 x 224, 100 x 64 -> 350 x 224 cut to 336, 64 x 90 -> 224 x 315 cut to 304; with and without a keep mask"""
    from freefine_amd.dino import HipDino
    cfg, st, _ = g15_inputs("tiny16", 224, 224, 1)
    rng = np.random.default_rng(shape[2])
    imgs = rng.integers(0, 256, shape, dtype=np.uint8)
    m1 = MASK_VALUES[rng.integers(0, 7, shape[:3])]
    for dt in (torch.float32, torch.bfloat16):
        net = HipDino(cfg, st, dtype=dt, device=gpu)
        for keep, src in ((None, imgs), (("gt128", m1, None), masked_numpy(imgs, "gt128", m1, None))):
            x = dino_host_prepare(src)
            assert x.shape[2] == 224 or x.shape[3] == 224
            want = net(x)
            got = net.features_u8(imgs, keep=keep)
            assert got.shape == (shape[0], 128) and torch.equal(got, want), (dt, keep is not None, (got - want).abs().max().item())
            got = net.features_u8(torch.from_numpy(imgs).to(gpu), keep=None if keep is None else ("gt128", torch.from_numpy(m1).to(gpu), None))
            assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# HipCLIPVision
# ---------------------------------------------------------------------------------------------------------------------
def clip_host_prepare(imgs, size=224):
    """clip/clip.py _transform on the host: Resize(224, BICUBIC), CenterCrop(224), ToTensor, Normalize"""
    from freefine_amd import ops
    from freefine_amd.clipvision import CLIP_MEAN, CLIP_STD
    out = []
    for im in imgs:
        oh, ow = ops.torchvision_resize_size(im.shape[0], im.shape[1], size)
        y0, x0, ch, cw = ops.center_crop_window(oh, ow, size)
        out.append(normalise(pil_resize(im, oh, ow, "bicubic")[y0:y0 + ch, x0:x0 + cw], CLIP_MEAN, CLIP_STD))
    return torch.stack(out)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "vitb32"])
def test_hipclipvision_vs_transformers_fp64(gpu, name, mode):
    """B = 4, against CLIPVisionModelWithProjection.double() on the CPU, bounded by tower_bound (tests/test_text_native_gpu.py): fp32 min(8 x the error of the
    module in fp32 on the CPU, 2e-5), bf16 2 x the error of the emulation.  FFN_CLIP_PARITY_OUT=<file> appends the line (how profiles/clip_vision_parity.txt is
    written)."""
    from freefine_amd.clipvision import HipCLIPVision
    cfg, st, x, want, errs = vision_case(name)
    net = HipCLIPVision(cfg, st, dtype=torch.bfloat16 if mode == "bf16" else torch.float32, device=gpu)
    out = net(x)
    assert out.shape == want.shape and out.dtype == torch.float32
    e, bound = scale_err(out, want), tower_bound(errs, mode)
    line = f"CLIP vision tower {name} {mode}: error {e:.3e} of the output maximum ({want.abs().max():.3f}); bound {bound:.3e} (reference errors: " + \
           ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + ")"
    print(line)
    if os.environ.get("FFN_CLIP_PARITY_OUT"):
        with open(os.environ["FFN_CLIP_PARITY_OUT"], "a") as f:
            f.write(line + "\n")
    assert e <= bound, line


@pytest.mark.parametrize("shape", [(3, 64, 96, 3), (2, 480, 640, 3), (2, 90, 64, 3)])
def test_hipclipvision_features_u8_equals_the_host_prepared_path(gpu, shape):
    from freefine_amd.clipvision import HipCLIPVision
    cfg, st, *_ = vision_case("tiny")
    rng = np.random.default_rng(shape[1])
    imgs = rng.integers(0, 256, shape, dtype=np.uint8)
    m1, m2 = MASK_VALUES[rng.integers(0, 7, shape[:3])], MASK_VALUES[rng.integers(0, 7, shape[:3])]
    for dt in (torch.float32, torch.bfloat16):
        net = HipCLIPVision(cfg, st, dtype=dt, device=gpu)
        for keep, src in ((None, imgs), (("sum_lt128", m1, m2), masked_numpy(imgs, "sum_lt128", m1, m2))):
            want = net(clip_host_prepare(src))
            got = net.features_u8(imgs, keep=keep)
            assert got.shape == (shape[0], 64) and torch.equal(got, want), (dt, keep is not None, (got - want).abs().max().item())
    with pytest.raises(ValueError, match="no positional interpolation"):
        net(torch.zeros(1, 3, 256, 256))


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def write_tree(root):
    """12 pairs: 64 x 64 and 96 x 64 (W x H) PNGs of smooth colour fields, mode-"L" masks (a box of 255; two of them half the size of their image, which PIL
    resizes with BICUBIC to intermediate values at the box edge), generated images = the source blended with another field (more from pair to pair) with the
    target box replaced by the object and the source box by noise -> (result tree, label, json path)"""
    from PIL import Image
    rng = np.random.default_rng(12)
    os.makedirs(root, exist_ok=True)
    data = {"im0": {"instances": {"0": {}, "1": {}}}, "im1": {"instances": {"0": {}}}}
    for i in range(12):
        H, W = (64, 64) if i % 3 else (64, 96)
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([127 + 100 * np.sin(xx / rng.uniform(4, 12) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(4, 12)) for _ in range(3)], axis=-1)
        src = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        (a0, b0), (a1, b1) = rng.integers(4, 20, 2), rng.integers(30, 40, 2)
        m1, m2 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        m1[a0:a0 + 24, b0:b0 + 24] = 255
        m2[a1:a1 + 22, b1:b1 + 22] = 255
        other = np.stack([127 + 100 * np.cos(xx / rng.uniform(3, 9)) * np.sin(yy / rng.uniform(3, 9) + rng.uniform(0, 6)) for _ in range(3)], axis=-1)
        alpha = 0.1 + 0.07 * i                                # the edit also disturbs the rest of the image, more from pair to pair
        gen = np.clip((1 - alpha) * src + alpha * other, 0, 255).astype(np.uint8)
        gen[a1:a1 + 22, b1:b1 + 22] = src[a0:a0 + 22, b0:b0 + 22]
        gen[a0:a0 + 24, b0:b0 + 24] = rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)
        if i in (4, 9):                                       # masks of another size than their image
            m1, m2 = m1[::2, ::2].copy(), m2[::2, ::2].copy()
        paths = {}
        for n, a in (("src", src), ("gen", gen), ("m1", m1), ("m2", m2)):
            paths[n] = os.path.join(root, f"{n}_{i:02d}.png")
            Image.fromarray(a).save(paths[n])
        data["im0" if i < 8 else "im1"]["instances"][str(i % 2) if i < 8 else "0"][f"s{i}"] = {
            "ori_img_path": paths["src"], "gen_img_path": paths["gen"], "ori_mask_path": paths["m1"], "tgt_mask_path": paths["m2"]}
    jpath = os.path.join(root, "results.json")
    with open(jpath, "w") as f:
        json.dump(data, f)
    return data, "gen_img_path", jpath


def reference_scores(pairs, kind, features64):
    """the reference's statements per pair (background_consistency.py:18-36, subject_consistency.py:10-30) with PIL and numpy on the host, features from
    `features64` (uint8 [H, W, 3] masked image -> fp64 [C]); the cosine BEFORE the clamp"""
    from PIL import Image
    import torch.nn.functional as F
    out = []
    for paths in pairs:
        inputs = [Image.open(p) for p in paths]
        if kind == "bgc":
            mask = np.array(inputs[2].resize(inputs[0].size)) + np.array(inputs[3].resize(inputs[0].size))
            ims = [np.array(inputs[i]) * (mask < 128).astype(np.uint8)[..., np.newaxis] for i in range(2)]
        else:
            ims = [np.array(inputs[i]) * (np.array(inputs[i + 2].resize(inputs[i].size)) > 128).astype(np.uint8)[..., np.newaxis] for i in range(2)]
        f = [F.normalize(features64(im)[None], dim=-1, p=2) for im in ims]
        out.append(F.cosine_similarity(f[0], f[1]).item())
    return out


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return write_tree(str(tmp_path_factory.mktemp("consistency")))


@pytest.fixture(scope="module")
def tiny_models(gpu):
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
    return dict(bgc=(CV.HipCLIPVision(ccfg, cst, dtype=torch.float32, device=gpu), clip64), subc=(HipDino(dcfg, dst, dtype=torch.float32, device=gpu), dino64),
                states=(cst, dst))


@pytest.mark.parametrize("kind", ["bgc", "subc"])
def test_drivers_end_to_end(gpu, tree, tiny_models, kind):
    """tiny extractors in fp32: every per-pair cosine within 1e-4 of the same arithmetic on fp64-reference features of PIL-prepared inputs (the reference cosines
    are > 0.05: the clamp is never active and cannot hide a sign error); the driver's mean is the mean of its own per-pair values exactly; batched and
    one-pair-at-a-time values are printed and held to the same 1e-4"""
    from freefine_amd import metrics as FM
    data, label, _ = tree
    net, ref_fn = tiny_models[kind]
    pairs = FM.consistency_pairs(data, label)
    assert len(pairs) == 12
    ref = reference_scores(pairs, kind, ref_fn)
    assert all(c > 0.05 for c in ref), ref
    batched = FM.consistency_scores(pairs, net, kind, batch_size=4)
    single = FM.consistency_scores(pairs, net, kind, batch_size=1)
    for i, (r, b, s) in enumerate(zip(ref, batched, single)):
        print(f"{kind} pair {i:2d}: reference {r:.7f}  batched {b:.7f} ({abs(b - r):.1e})  one at a time {s:.7f} ({abs(s - r):.1e})  {'bit-identical' if b == s else 'differ'}")
    print(f"{kind}: batched and one-at-a-time values bit-identical: {batched == single}")
    assert all(abs(b - r) <= 1e-4 for b, r in zip(batched, ref)) and all(abs(s - r) <= 1e-4 for s, r in zip(single, ref))
    fn = FM.calculate_bgc if kind == "bgc" else FM.calculate_subc
    assert fn(data, label, net, batch_size=4) == sum(batched) / len(batched)
    assert len(set(f"{c:.4f}" for c in ref)) > 6              # the pairs are told apart


def test_main_driver_as_a_child_process(gpu, tree, tiny_models, tmp_path):
    from freefine_amd import metrics as FM
    data, label, jpath = tree
    cst, dst = tiny_models["states"]
    cw, dw = str(tmp_path / "clip_tiny.pt"), str(tmp_path / "dino_tiny16.pt")
    torch.save(cst, cw)
    torch.save(dst, dw)
    main = os.path.join(ROOT, "evaluation", "metrics", "main.py")
    r = subprocess.run([sys.executable, main, "--path", jpath, "--task", "000110000", "--clip_weights", cw, "--dino_weights", dw, "--clip_config", "tiny",
                        "--dino_config", "tiny16"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    vals = dict(line.split(": ", 1) for line in r.stdout.split("-----Result-----")[1].strip().splitlines())
    assert list(vals) == ["BGC", "SUBC"]
    want = {"BGC": FM.calculate_bgc(data, label, tiny_models["bgc"][0]), "SUBC": FM.calculate_subc(data, label, tiny_models["subc"][0])}
    for k in vals:
        assert abs(float(vals[k]) - want[k]) <= 1e-6 and 0.05 < float(vals[k]) <= 1.0, (k, vals[k], want[k])
    r = subprocess.run([sys.executable, main, "--path", jpath, "--task", "100000000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FID: not built" in r.stdout, (r.stdout, r.stderr)
