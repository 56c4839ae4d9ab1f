"""CPU: the host side of Background / Subject Consistency: the PIL resampling tables (bilinear and bicubic) against PIL itself, torchvision's documented size and
crop rules, the ABI of ffn_resize_pil_u8 with every refusal (nothing is launched), a test-local restatement of the CLIP image tower (fp64 sums, and the bf16
arithmetic emulated) against transformers' CLIPVisionModelWithProjection.double(), both state layouts, the DINO ViT-B/16 configuration against
tests/golden/g15_dino16_cls.npz's shapes, the metric arithmetic on a stub extractor, the reference's import paths and the driver's command line."""
import ctypes
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from freefine_amd import metrics as FM
from freefine_amd import ops
from test_text_native_cpu import _mm, _store, scale_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# (W, H) -> (ow, oh), channels: as the issue lists them (width x height)
RESIZE_CASES = [((512, 512), (224, 224), 3), ((53, 37), (42, 28), 3), ((200, 300), (224, 336), 3), ((64, 64), (224, 224), 3), ((640, 480), (298, 224), 3),
                ((1, 1), (5, 7), 3), ((70, 50), (33, 97), 1)]
FILTERS = ("bilinear", "bicubic")


def pil_resize(img, oh, ow, filter):
    """img uint8 [H, W, 3] or [H, W] -> PIL's Image.resize((ow, oh), filter)"""
    from PIL import Image
    return np.array(Image.fromarray(img).resize((ow, oh), {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filter]))


def resize_numpy(img, oh, ow, filter):
    """ops.pil_resample_coeffs applied in int64: horizontal pass, then vertical pass, each clamp((2^21 + sum) >> 22) -- img uint8 [H, W, C] or [H, W]"""
    def one_axis(a, n_out):                                   # resamples axis 0
        bounds, coef = ops.pil_resample_coeffs(a.shape[0], n_out, filter)
        out = np.empty((n_out,) + a.shape[1:], dtype=np.uint8)
        for i, (lo, n) in enumerate(bounds):
            acc = (1 << 21) + np.tensordot(coef[i, :n].astype(np.int64), a[lo:lo + n].astype(np.int64), axes=(0, 0))
            assert np.abs(acc).max() < 2 ** 31               # the kernels' 32-bit sum holds it
            out[i] = np.clip(acc >> 22, 0, 255)
        return out
    swap = (1, 0, 2) if img.ndim == 3 else (1, 0)
    h = one_axis(np.ascontiguousarray(img.transpose(swap)), ow).transpose(swap)
    return one_axis(np.ascontiguousarray(h), oh)


def sample_images(H, W, C, seed):
    """(name, uint8 [H, W, C] or [H, W] for C = 1): a random image and a 0 / 255 checkerboard"""
    checker = (((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2) * 255).astype(np.uint8)
    rnd = np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)
    out = [("random", rnd), ("checkerboard", np.ascontiguousarray(np.repeat(checker[..., None], C, axis=2)))]
    return [(n, a[..., 0].copy() if C == 1 else a) for n, a in out]


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("src,dst,C", RESIZE_CASES)
def test_resample_tables_reproduce_pil_bit_for_bit(src, dst, C, filter):
    (W, H), (ow, oh) = src, dst
    for name, img in sample_images(H, W, C, W * 1000 + H):
        want = pil_resize(img, oh, ow, filter)
        assert np.array_equal(resize_numpy(img, oh, ow, filter), want), (name, src, dst, filter)
    if filter == "bicubic" and src == (64, 64):               # the upscaled checkerboard overshoots: both clamps are exercised
        b, k = ops.pil_resample_coeffs(64, 224, "bicubic")
        assert (k < 0).any()
        row = np.tile(np.array([0, 255], np.int64), 32)
        raw = np.array([((1 << 21) + (k[i, :n].astype(np.int64) * row[lo:lo + n]).sum()) >> 22 for i, (lo, n) in enumerate(b)])
        assert raw.min() < 0 and raw.max() > 255


def test_bilinear_tables_are_todays_and_bicubic_shapes():
    for n_in, n_out in [(512, 224), (37, 28), (224, 224), (700, 28), (1, 7), (64, 224)]:
        b, k = ops.pil_resample_coeffs(n_in, n_out, "bilinear")
        b0, k0 = ops.pil_bilinear_coeffs(n_in, n_out)
        assert np.array_equal(b, b0) and np.array_equal(k, k0) and b.dtype == k.dtype == np.int32
    b, k = ops.pil_resample_coeffs(700, 28, "bicubic")
    assert k.shape == (28, 2 * 50 + 1) and b.dtype == k.dtype == np.int32 and (k < 0).any()
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 700).all() and (b[:, 1] <= k.shape[1]).all()
    assert np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)).max() <= k.shape[1] // 2 + 1
    b, k = ops.pil_resample_coeffs(224, 224, "bicubic")       # an unchanged axis: the filter itself gives the identity
    for i in range(224):
        row = np.zeros(224, dtype=np.int64)
        row[b[i, 0]:b[i, 0] + b[i, 1]] = k[i, :b[i, 1]]
        assert row[i] == 1 << 22 and np.abs(row).sum() == 1 << 22
    assert ops.pil_resample_coeffs(224, 224, "bicubic")[1] is k
    with pytest.raises(ValueError, match="lanczos"):
        ops.pil_resample_coeffs(10, 5, "lanczos")


def test_size_and_crop_rules():
    """torchvision's documented rules at (W x H) 640 x 480, 480 x 640, 225 x 224 and 224 x 224; the expected numbers are worked by hand from the rules"""
    # Resize(224): short side -> 224, long side -> int(224 * long / short): int(224 * 640 / 480) = int(298.67) = 298, int(224 * 225 / 224) = 225
    assert ops.torchvision_resize_size(480, 640, 224) == (224, 298)
    assert ops.torchvision_resize_size(640, 480, 224) == (298, 224)
    assert ops.torchvision_resize_size(224, 225, 224) == (224, 225)
    assert ops.torchvision_resize_size(224, 224, 224) == (224, 224)
    assert ops.torchvision_resize_size(64, 96, 224) == (224, 336) and ops.torchvision_resize_size(37, 53, 224) == (224, 320)
    # CenterCrop(224): top = int(round((h - 224) / 2.0)): round(37.0) = 37, round(0.5) = 0 (Python rounds halves to even)
    assert ops.center_crop_window(224, 298, 224) == (0, 37, 224, 224)
    assert ops.center_crop_window(298, 224, 224) == (37, 0, 224, 224)
    assert ops.center_crop_window(224, 225, 224) == (0, 0, 224, 224)
    assert ops.center_crop_window(224, 227, 224) == (0, 2, 224, 224)      # round(1.5) = 2
    assert ops.center_crop_window(224, 224, 224) == (0, 0, 224, 224)


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_resize_pil_u8_is_declared_bound_exported_and_refuses_on_the_host():
    """ffn_resize_pil_u8 refuses, before any launch: null pointers, sides beyond FFN_IMGPREP_MAX_SIDE, C outside {1, 3}, a window outside the destination, an
    unknown rule, masks with C = 1, a rule without m1, a table width outside 1 .. FFN_IMGPREP_MAX_TAPS (no GPU needed: nothing is launched)"""
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    assert re.search(r"\bint\s+ffn_resize_pil_u8\s*\(", header) and "ffn_resize_pil_u8" in _lib.SYMBOLS
    assert re.search(r"FFN_KEEP_NONE\s*=\s*0\s*,\s*FFN_KEEP_SUM_LT128\s*=\s*1\s*,\s*FFN_KEEP_GT128\s*=\s*2", header)
    assert (_lib.KEEP_NONE, _lib.KEEP_SUM_LT128, _lib.KEEP_GT128) == (0, 1, 2)
    assert re.search(r"#define\s+FFN_IMGPREP_MAX_TAPS\s+\(2 \* 3 \* FFN_IMGPREP_MAX_SIDE \+ 1\)", header) and _lib.IMGPREP_MAX_TAPS == 24577
    # the descriptor's fields, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} ffn_resize_pil_desc;", header).group(1)
    names = [n.strip(" *\n") for line in body.split(";") if line.strip() for n in line.replace("const", "").replace("uint8_t", "").replace("int", "").split(",")]
    assert names == [f[0] for f in _lib.ResizePilDesc._fields_], names
    lib = _lib.load()
    assert hasattr(lib, "ffn_resize_pil_u8") and lib.ffn_version() >= 6
    P, lim, taps = 0x10000, _lib.IMGPREP_MAX_SIDE, _lib.IMGPREP_MAX_TAPS      # P: never dereferenced, validation fails first

    def call(**kw):
        d = _lib.ResizePilDesc()
        base = dict(src=P, dst=P, scratch=P, m1=None, m2=None, hbounds=P, hcoef=P, vbounds=P, vcoef=P, B=2, H=480, W=640, C=3, oh=224, ow=298, hksize=11, vksize=11,
                    y0=0, x0=37, ch=224, cw=224, rule=_lib.KEEP_NONE)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.ffn_resize_pil_u8(None, ctypes.byref(d))
    bad = [(dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(scratch=None), b"null"), (dict(hbounds=None), b"null"), (dict(hcoef=None), b"null"),
           (dict(vbounds=None), b"null"), (dict(vcoef=None), b"null"),
           (dict(H=lim + 1), b"outside 1 .. 4096"), (dict(W=lim + 1), b"outside 1 .. 4096"), (dict(oh=lim + 1), b"outside 1 .. 4096"),
           (dict(ow=lim + 1), b"outside 1 .. 4096"), (dict(H=0), b"outside"), (dict(ow=0), b"outside"), (dict(B=0), b"B=0"), (dict(B=65536), b"B=65536"),
           (dict(C=2), b"C=2"), (dict(C=4), b"C=4"), (dict(C=0), b"C=0"),
           (dict(x0=75), b"window"), (dict(y0=1), b"window"), (dict(x0=-1), b"window"), (dict(y0=-1, ch=10), b"window"), (dict(ch=0), b"window"),
           (dict(cw=0), b"window"), (dict(cw=262), b"window"), (dict(ch=225), b"window"), (dict(x0=2 ** 31 - 1, cw=2), b"window"),
           (dict(rule=3), b"unknown keep rule"), (dict(rule=-1), b"unknown keep rule"),
           (dict(C=1, rule=_lib.KEEP_GT128, m1=P), b"needs C=3"), (dict(C=1, rule=_lib.KEEP_SUM_LT128, m1=P, m2=P), b"needs C=3"),
           (dict(rule=_lib.KEEP_GT128), b"without m1"), (dict(rule=_lib.KEEP_SUM_LT128, m2=P), b"without m1"),
           (dict(hksize=0), b"table widths"), (dict(vksize=0), b"table widths"), (dict(hksize=taps + 1), b"table widths"), (dict(vksize=taps + 1), b"table widths"),
           (dict(vksize=-3), b"table widths")]
    for kw, msg in bad:
        assert call(**kw) == -22, kw
        err = lib.ffn_last_error()
        assert msg in err and err.startswith(b"resize_pil_u8"), (kw, err)
    d = None
    assert lib.ffn_resize_pil_u8(None, d) == -22 and b"null descriptor" in lib.ffn_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the CLIP image tower restated (test-local; fp64 sums everywhere)
# ---------------------------------------------------------------------------------------------------------------------
def vision_ref(cfg, state, x, mode="f64"):
    """CLIPVisionModelWithProjection(x).image_embeds restated from transformers' layout: patch rows W^T + pos, class row, pre_layrnorm, the blocks
    (softmax(q k^T / 8) v per head, quick-gelu MLP), post_layernorm of the class row, projection.  x [B, 3, S, S] -> fp64 [B, P].  mode "f64", or "bf16": the
    device's fast mode emulated -- bf16-rounded operands of every product, every stored activation (and the stored positional / class rows) rounded to bf16, sums
    in fp64 -- like tower_ref of tests/test_text_native_cpu.py."""
    st = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v.double() for k, v in state.items()}
    C, nh, eps, ps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps, cfg.patch_size
    B = x.shape[0]
    keep = lambda t: _store(t, mode)
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (C,), st[p + ".weight"], st[p + ".bias"], eps)
    lin = lambda t, p: _mm(t, st[p + ".weight"], mode) + st[p + ".bias"]
    g = x.shape[2] // ps
    rows = keep(x.double().reshape(B, 3, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * ps * ps))
    pos = st["embeddings.position_embedding.weight"]
    t = keep(_mm(rows, st["embeddings.patch_embedding.weight"].reshape(C, -1), mode) + keep(pos[1:]))
    cls = keep(st["embeddings.class_embedding"] + pos[0])
    h = torch.cat([cls.expand(B, 1, C), t], dim=1)
    S = h.shape[1]
    h = keep(ln(h, "pre_layrnorm"))
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        y = keep(ln(h, p + "layer_norm1"))
        heads = lambda u: u.view(B, S, nh, 64).transpose(1, 2)
        q, k, v = (heads(keep(lin(y, p + "self_attn." + n))) for n in ("q_proj", "k_proj", "v_proj"))
        s = _mm(q, k, mode) * 0.125
        e = torch.exp(s - s.amax(-1, keepdim=True))
        a = _mm(e, v.transpose(-1, -2), mode) / e.sum(-1, keepdim=True)         # the kernels normalise after the second product
        a = keep(a.transpose(1, 2).reshape(B, S, C))
        h = keep(h + lin(a, p + "self_attn.out_proj"))
        y = keep(ln(h, p + "layer_norm2"))
        u = lin(y, p + "mlp.fc1")
        h = keep(h + lin(keep(u * torch.sigmoid(1.702 * u)), p + "mlp.fc2"))
    return keep(_mm(keep(ln(h[:, 0], "post_layernorm")), st["visual_projection.weight"], mode))


@functools.lru_cache(maxsize=None)
def vision_case(name, B=4):
    """(config, seeded state in transformers' layout, normalised input [B, 3, 224, 224], CLIPVisionModelWithProjection.double() image_embeds, the reference
    errors {"f32": the module in fp32 on the CPU, "bf16": the bf16 emulation} against it) -- computed once, shared with tests/test_consistency_gpu.py"""
    from transformers import CLIPVisionModelWithProjection
    from freefine_amd import clipvision as CV
    cfg = CV.clip_vision_config(name)
    st = CV.synthetic_state(cfg, seed=32 + len(name))
    x = torch.from_numpy(np.random.default_rng(320 + len(name)).standard_normal((B, 3, 224, 224)).astype(np.float32))
    mod = CLIPVisionModelWithProjection(CV.transformers_vision_config(cfg)).eval()
    mod.load_state_dict(st, strict=True)
    with torch.no_grad():
        f32 = mod(pixel_values=x).image_embeds
        want = mod.double()(pixel_values=x.double()).image_embeds
        errs = {"f32": scale_err(f32, want), "bf16": scale_err(vision_ref(cfg, st, x, "bf16"), want)}
    return cfg, st, x, want, errs


@pytest.mark.parametrize("name", ["tiny", "vitb32"])
def test_vision_restatement_equals_transformers_fp64(name):
    cfg, st, x, want, errs = vision_case(name)
    got = vision_ref(cfg, st, x)
    e = scale_err(got, want)
    print(f"vision restatement vs CLIPVisionModelWithProjection.double() ({name}): {e:.2e}; fp32 module {errs['f32']:.2e}, emulated bf16 {errs['bf16']:.2e} "
          f"(|y| max {want.abs().max():.3f})")
    assert got.shape == want.shape == (4, cfg.projection_dim) and e <= 1e-12
    assert 0 < errs["f32"] < 1e-5 and errs["f32"] < errs["bf16"] < 1e-1


def test_both_state_layouts_pack_to_identical_tensors():
    from freefine_amd import clipvision as CV
    cfg, st, *_ = vision_case("tiny")
    bare = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in st.items()}
    bare["embeddings.position_ids"] = torch.arange(50)[None]
    oa = CV.to_openai_layout(st, cfg.num_hidden_layers)
    assert oa["visual.proj"].shape == (128, 64) and oa["visual.transformer.resblocks.1.attn.in_proj_weight"].shape == (384, 128) and "visual.conv1.weight" in oa
    packs = [CV.pack_vision_state(cfg, s) for s in (st, bare, oa, {k[len("visual."):]: v for k, v in oa.items()})]
    for p in packs[1:]:
        assert set(p) == set(packs[0]) and all(torch.equal(p[k], packs[0][k]) for k in p)
    a = packs[0]
    C = 128
    assert torch.equal(a["1.qk.w"][:C], st["vision_model.encoder.layers.1.self_attn.q_proj.weight"])
    assert torch.equal(a["1.qk.w"][C:], st["vision_model.encoder.layers.1.self_attn.k_proj.weight"])
    assert torch.equal(a["cls"], st["vision_model.embeddings.class_embedding"] + st["vision_model.embeddings.position_embedding.weight"][0])
    assert a["pe.w"].shape == (128, 3072) and a["pos"].shape == (49, 128) and a["proj.w"].shape == (64, 128)
    broken = dict(st)
    broken.pop("vision_model.encoder.layers.0.mlp.fc2.bias")
    with pytest.raises(ValueError, match="fc2.bias"):
        CV.pack_vision_state(cfg, broken)
    broken = dict(oa)
    broken.pop("visual.ln_post.bias")
    with pytest.raises(ValueError, match="ln_post.bias"):
        CV.pack_vision_state(cfg, broken)
    with pytest.raises(ValueError, match="head dim"):
        CV.clip_vision_config(dict(hidden_size=128, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4))
    with pytest.raises(ValueError, match="hidden_act"):
        CV.clip_vision_config(dict(hidden_size=128, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2, hidden_act="gelu"))
    with pytest.raises(ValueError, match="one of"):
        CV.clip_vision_config("vitl14")


# ---------------------------------------------------------------------------------------------------------------------
# DINO ViT-B/16
# ---------------------------------------------------------------------------------------------------------------------
G15_CASES = [("tiny16", 224, 224, 2), ("tiny16", 224, 288, 1), ("vitb16", 224, 224, 2)]


def g15_inputs(name, H, W, B):
    """(configuration, seeded state in hub layout, input) of one G15 case: the seeds of tools/gen_golden.py g15_inputs -- shared with tests/test_consistency_gpu.py"""
    from freefine_amd import dino as FD
    cfg = FD.dino_config(name)
    x = torch.from_numpy((np.random.default_rng(150 + H + W + len(name)).standard_normal((B, 3, H, W))).astype(np.float32))
    return cfg, FD.synthetic_state(cfg, seed=15 + len(name)), x


def dino16_ref(cfg, st, x):
    """the class tokens of DINO ViT-B/16 from oracle/dpt.py's ViT, which reads patch and grid from its configuration: the hub-layout state under the oracle's
    `pretrained.` prefix with LayerScale gammas of exactly 1 (x * 1 is exact).  In the dtype of x: fp64 inputs give the fp64 reference of the GPU tests."""
    from oracle import dpt as OD
    full = {"pretrained." + k: v for k, v in st.items()}
    for i in range(cfg.depth):
        full[f"pretrained.blocks.{i}.ls1.gamma"] = full[f"pretrained.blocks.{i}.ls2.gamma"] = torch.ones(cfg.embed_dim)
    with torch.no_grad():
        return OD.vit_features(cfg, full, x, 1)[0][1]


# the oracle against the vendored DinoVisionTransformer's recorded class tokens (scale 3): a few fp32 ulp of that scale after 12 blocks, the bound G14 holds
G15_ORACLE_TOL = 2e-5


@pytest.mark.parametrize("name,H,W,B", G15_CASES)
def test_g15_matches_the_oracle_at_patch_16(name, H, W, B):
    gold = torch.from_numpy(np.load(os.path.join(GOLD, "g15_dino16_cls.npz"))[f"{name}_{H}x{W}"])
    cfg, st, x = g15_inputs(name, H, W, B)
    d = (dino16_ref(cfg, st, x) - gold).abs().max().item()
    d64 = (dino16_ref(cfg, st, x.double()) - gold).abs().max().item()
    print(f"G15 {name} {H}x{W}: oracle fp32 vs reference {d:.3e}, oracle fp64 vs reference {d64:.3e} (|y|max {gold.abs().max():.3f})")
    assert d <= G15_ORACLE_TOL and d64 <= G15_ORACLE_TOL


def test_dino16_config_state_layout_and_golden_shapes():
    from freefine_amd import dino as FD
    gold = np.load(os.path.join(GOLD, "g15_dino16_cls.npz"))
    assert sorted(gold.files) == sorted(f"{n}_{H}x{W}" for n, H, W, _ in G15_CASES)
    for name, H, W, B in G15_CASES:
        cfg, st, x = g15_inputs(name, H, W, B)
        assert (cfg.patch, cfg.img_size, cfg.layerscale, cfg.interpolate_offset, cfg.ln_eps) == (16, 224, False, 0.1, 1e-6)
        assert gold[f"{name}_{H}x{W}"].shape == (B, cfg.embed_dim) and np.isfinite(gold[f"{name}_{H}x{W}"]).all()
        assert not any("gamma" in k for k in st) and st["pos_embed"].shape == (1, 197, cfg.embed_dim) and st["patch_embed.proj.weight"].shape[2:] == (16, 16)
        assert set(st) == set(FD.param_shapes(cfg))
    b, t = FD.dino_config("vitb16"), FD.dino_config("tiny16")
    assert (b.embed_dim, b.depth, b.num_heads) == (768, 12, 12) and (t.embed_dim, t.depth, t.num_heads) == (128, 4, 2)
    with pytest.raises(KeyError):
        FD.dino_config("vitb")
    # the DINOv2 layout is what it was: LayerScale present
    assert "blocks.0.ls1.gamma" in FD.dinov2_param_shapes(FD.dinov2_config("tiny"))


# ---------------------------------------------------------------------------------------------------------------------
# the metric arithmetic on a stub extractor
# ---------------------------------------------------------------------------------------------------------------------
def stub_features(images):
    """per image [mean R - 64, mean G - 64, mean B - 64, 8]: cosines of either sign are reachable"""
    f = np.asarray(images, np.float64).reshape(len(images), -1, 3).mean(1) - 64.0
    return torch.from_numpy(np.concatenate([f, np.full((len(f), 1), 8.0)], axis=1).astype(np.float32))


class StubExtractor:
    """stands for HipCLIPVision / HipDino: applies the keep rule in numpy as the header states it, records the batches"""

    def __init__(self):
        self.calls = []

    def features_u8(self, images, keep=None):
        images = np.asarray(images)
        rule, m1, m2 = keep
        assert images.dtype == np.uint8 and images.ndim == 4 and m1.dtype == np.uint8 and m1.shape == images.shape[:3]
        if rule == "sum_lt128":
            kept = ((m1.astype(np.int64) + m2.astype(np.int64)) % 256) < 128
        else:
            assert rule == "gt128" and m2 is None
            kept = m1 > 128
        self.calls.append((rule, images.shape))
        return stub_features(images * kept[..., None].astype(np.uint8))


def reference_pair(kind, src, gen, m1, m2):
    """one pair as the reference spells it (background_consistency.py:20-36, subject_consistency.py:18-30), on the stub's features; masks already image-sized"""
    import torch.nn.functional as F
    if kind == "bgc":
        mask = m1 + m2                                                       # uint8 + uint8: wraps
        mask_bool = (mask < 128).astype(np.uint8)
        ims = [src * mask_bool[..., np.newaxis], gen * mask_bool[..., np.newaxis]]
    else:
        ims = [im * (m > 128).astype(np.uint8)[..., np.newaxis] for im, m in ((src, m1), (gen, m2))]
    f = [F.normalize(stub_features(im[None]), dim=-1, p=2) for im in ims]
    return F.cosine_similarity(f[0], f[1]).item()


def stub_tree():
    """six pairs held in memory (the reader maps names to arrays): mask values that wrap (200 + 100), values exactly 128 (128 + 0 drops, 128 + 128 keeps; GT128
    drops 128 and keeps 129), a pair whose cosine is negative, and two sizes"""
    rng = np.random.default_rng(7)
    files, data = {}, {"im0": {"instances": {"0": {}, "1": {}}}}
    vals = np.array([0, 100, 127, 128, 129, 200, 255], np.uint8)
    for i in range(6):
        H, W = (8, 6) if i % 2 == 0 else (5, 9)
        src = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        gen = src.copy()
        gen[1:4, 1:4] = rng.integers(0, 256, (3, 3, 3), dtype=np.uint8)
        m1, m2 = vals[rng.integers(0, 7, (H, W))], vals[rng.integers(0, 7, (H, W))]
        if i == 0:
            m1[:], m2[:] = 200, 100                         # wraps to 44: everything kept (a non-wrapping sum would drop everything)
            m1[0], m2[0] = 128, 0                           # 128: dropped
            m1[1], m2[1] = 128, 128                         # wraps to 0: kept
        if i == 1:
            m1[:], m2[:] = 129, 129                         # SUBC keeps everything; BGC: 258 -> 2 keeps everything
            m1[0], m2[0] = 128, 128                         # SUBC drops this row
        if i == 2:                                          # opposite images: a negative cosine, clamped to 0
            src[:], gen[:], m1[:], m2[:] = 250, 0, 200, 130      # both > 128 (SUBC keeps all) and 200 + 130 -> 74 < 128 (BGC keeps all)
        for n, a in (("src", src), ("gen", gen), ("m1", m1), ("m2", m2)):
            files[f"{n}{i}"] = a
        data["im0"]["instances"][str(i % 2)][f"s{i}"] = {"ori_img_path": f"src{i}", "gen": f"gen{i}", "ori_mask_path": f"m1{i}", "tgt_mask_path": f"m2{i}"}
    return data, files


@pytest.mark.parametrize("kind", ["bgc", "subc"])
def test_metric_arithmetic_on_a_stub_extractor(kind):
    data, files = stub_tree()
    pairs = FM.consistency_pairs(data, "gen")
    assert len(pairs) == 6 and pairs[0] == ("src0", "gen0", "m10", "m20") and [p[0] for p in pairs] == ["src0", "src2", "src4", "src1", "src3", "src5"]
    model = StubExtractor()
    scores = FM.consistency_scores(pairs, model, kind, batch_size=2, reader=files.__getitem__)
    raw = [reference_pair(kind, *(files[n] for n in p)) for p in pairs]
    want = [max(0.0, c) for c in raw]
    print(kind, "raw cosines", [f"{c:.4f}" for c in raw])
    assert all(abs(a - b) <= 1e-6 for a, b in zip(scores, want)), (scores, want)
    i2 = [p[0] for p in pairs].index("src2")
    assert raw[i2] < -0.5 and scores[i2] == 0.0                                 # the clamp
    # one launch sees one size: 3 pairs of each size in batches of 2 -> 2 + 1, twice (source and generated) per batch
    assert sorted(model.calls) == sorted([(model.calls[0][0], (2, 8, 6, 3))] * 2 + [(model.calls[0][0], (1, 8, 6, 3))] * 2 +
                                         [(model.calls[0][0], (2, 5, 9, 3))] * 2 + [(model.calls[0][0], (1, 5, 9, 3))] * 2)
    fn = FM.calculate_bgc if kind == "bgc" else FM.calculate_subc
    assert fn(data, "gen", StubExtractor(), batch_size=2, reader=files.__getitem__) == sum(scores) / len(scores)
    one = FM.consistency_scores(pairs, StubExtractor(), kind, batch_size=1, reader=files.__getitem__)
    assert one == scores


def test_wrap_and_threshold_values_change_the_result():
    """the uint8 wrap and the two thresholds, each against the pair worked by hand"""
    data, files = stub_tree()
    s0, g0 = files["src0"], files["gen0"]
    got = FM.consistency_scores([("src0", "gen0", "m10", "m20")], StubExtractor(), "bgc", reader=files.__getitem__)[0]
    kept = np.ones(s0.shape[:2], bool)
    kept[0] = False                                           # 128 + 0 = 128 is not < 128; 200 + 100 -> 44 and 128 + 128 -> 0 are
    f = [torch.nn.functional.normalize(stub_features((im * kept[..., None])[None]), dim=-1) for im in (s0, g0)]
    assert abs(got - (f[0] * f[1]).sum().item()) <= 1e-6
    got = FM.consistency_scores([("src1", "gen1", "m11", "m21")], StubExtractor(), "subc", reader=files.__getitem__)[0]
    kept = np.ones(files["src1"].shape[:2], bool)
    kept[0] = False                                           # 128 is not > 128; 129 is
    f = [torch.nn.functional.normalize(stub_features((files[n] * kept[..., None])[None]), dim=-1) for n in ("src1", "gen1")]
    assert abs(got - (f[0] * f[1]).sum().item()) <= 1e-6


def test_refusals_of_the_consistency_drivers():
    data, files = stub_tree()
    files = dict(files)
    files["rgba"] = np.zeros((8, 6, 4), np.uint8)
    files["gray"] = np.zeros((8, 6), np.uint8)
    files["rgbmask"] = np.zeros((8, 6, 3), np.uint8)
    files["m16"] = np.zeros((8, 6), np.uint16)
    files["bigger"] = np.zeros((9, 6, 3), np.uint8)
    files["bigmask"] = np.zeros((9, 6), np.uint8)
    rd = files.__getitem__
    for kind in ("bgc", "subc"):
        with pytest.raises(ValueError, match="RGB images only"):
            FM.consistency_scores([("rgba", "gen0", "m10", "m20")], StubExtractor(), kind, reader=rd)
        with pytest.raises(ValueError, match="RGB images only"):
            FM.consistency_scores([("src0", "gray", "m10", "m20")], StubExtractor(), kind, reader=rd)
        with pytest.raises(ValueError, match='mode-"L" masks only'):
            FM.consistency_scores([("src0", "gen0", "rgbmask", "m20")], StubExtractor(), kind, reader=rd)
        with pytest.raises(ValueError, match='mode-"L" masks only'):
            FM.consistency_scores([("src0", "gen0", "m10", "m16")], StubExtractor(), kind, reader=rd)
    with pytest.raises(ValueError, match="Background Consistency"):
        FM.consistency_scores([("src0", "bigger", "m10", "m20")], StubExtractor(), "bgc", reader=rd)
    # Subject Consistency masks each image with its own mask: a generated image of another size is fine when its mask has that size
    assert len(FM.consistency_scores([("src0", "bigger", "m10", "bigmask")], StubExtractor(), "subc", reader=rd)) == 1


def test_default_reader_checks_pil_modes(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(1)
    paths = {}
    for n, a, mode in (("src", rng.integers(0, 256, (8, 6, 3), dtype=np.uint8), None), ("gen", rng.integers(0, 256, (8, 6, 3), dtype=np.uint8), None),
                       ("m1", np.full((8, 6), 255, np.uint8), None), ("m2", np.full((8, 6), 200, np.uint8), None),
                       ("pal", rng.integers(0, 256, (8, 6, 3), dtype=np.uint8), "P"), ("bit", np.full((8, 6), 255, np.uint8), "1")):
        im = Image.fromarray(a)
        paths[n] = str(tmp_path / f"{n}.png")
        (im.convert(mode) if mode else im).save(paths[n])
    ok = FM.consistency_scores([(paths["src"], paths["gen"], paths["m1"], paths["m2"])], StubExtractor(), "subc")
    assert len(ok) == 1 and ok[0] > 0.05
    with pytest.raises(ValueError, match="RGB images only"):
        FM.consistency_scores([(paths["pal"], paths["gen"], paths["m1"], paths["m2"])], StubExtractor(), "subc")
    with pytest.raises(ValueError, match='mode-"L" masks only'):
        FM.consistency_scores([(paths["src"], paths["gen"], paths["bit"], paths["m2"])], StubExtractor(), "subc")


def test_pil_default_filter_of_an_l_mask_is_bicubic():
    """the premise of metrics._mask_to: Image.resize without a filter on a mode-"L" image is BICUBIC"""
    from PIL import Image
    m = np.random.default_rng(2).integers(0, 256, (50, 70), dtype=np.uint8)
    assert np.array_equal(np.array(Image.fromarray(m).resize((33, 97))), pil_resize(m, 97, 33, "bicubic"))


# ---------------------------------------------------------------------------------------------------------------------
# import paths and the driver's command line
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_import_paths():
    from evaluation.metrics.VBench.background_consistency import calculate_bgc, parse_data
    from evaluation.metrics.VBench.subject_consistency import calculate_subc
    assert calculate_bgc is FM.calculate_bgc and calculate_subc is FM.calculate_subc and parse_data is FM.consistency_pairs


def load_driver():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ffn_metrics_main", os.path.join(ROOT, "evaluation", "metrics", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_filters_and_reports_what_is_not_built(tmp_path, capsys):
    from PIL import Image
    drv = load_driver()
    rng = np.random.default_rng(3)
    for n in ("coarse", "gen"):
        Image.fromarray(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)).save(str(tmp_path / f"{n}.png"))
    Image.fromarray(np.full((8, 8), 255, np.uint8)).save(str(tmp_path / "mask.png"))
    Image.fromarray(np.full((8, 8), 255, np.uint8)).save(str(tmp_path / "mask3d.png"))

    def sample(prompt, rot):
        return {"edit_prompt": prompt, "edit_param": [0, 0, 0, 0, 0, rot, 1, 1], "coarse_input_path": "coarse.png", "gen_img_path": "gen.png", "tgt_mask_path": "mask.png",
                "ori_img_path": "gen.png", "ori_mask_path": "mask.png", "target_mask_0": "mask3d.png", "coarse_input_path_0": "coarse.png"}
    data = {"a": {"instances": {"0": {"c0": sample("move it Slightly left", 0), "c1": sample("rotate it heavily", 30), "c2": sample("move it strongly", 0)}}}}
    path = str(tmp_path / "results.json")
    json.dump(data, open(path, "w"))
    # FID alone: reported as not built, nothing else runs, no error
    res = drv.main(["--path", path, "--task", "100000000"])
    out = capsys.readouterr().out
    assert list(res) == ["FID"] and "not built" in res["FID"] and "FID: not built" in out
    res = drv.main(["--path", path, "--task", "111001000", "--use_relative_path", "--base_dir", str(tmp_path), "--3d"])
    assert list(res) == ["FID", "IRS", "HPS", "WRAP_E"] and all("not built" in res[k] for k in ("FID", "IRS", "HPS")) and isinstance(res["WRAP_E"], float)
    # BGC / SUBC without weights: said so, no failure
    res = drv.main(["--path", path, "--task", "000110000"])
    assert "clip_weights" in res["BGC"] and "dino_weights" in res["SUBC"]
    # the filters
    ns = lambda **kw: type("A", (), dict(dict(level=0, no_rotate=False, three_d=False, use_relative_path=False, base_dir=None, gen_img_key="gen_img_path"), **kw))
    keys = lambda d: sorted(d["a"]["instances"]["0"])
    assert keys(drv.filter_data(json.load(open(path)), ns(level=1))) == ["c0"]
    assert keys(drv.filter_data(json.load(open(path)), ns(level=3))) == ["c1", "c2"]
    assert keys(drv.filter_data(json.load(open(path)), ns(no_rotate=True))) == ["c0", "c2"]
    assert keys(drv.filter_data(json.load(open(path)), ns(level=3, no_rotate=True))) == ["c2"]
    d = drv.filter_data(json.load(open(path)), ns(three_d=True, use_relative_path=True, base_dir="/b"))["a"]["instances"]["0"]["c0"]
    assert d["tgt_mask_path"] == "/b/mask3d.png" and d["gen_img_path"] == "/b/gen.png" and d["target_mask_0"] == "mask3d.png"
    with pytest.raises(SystemExit):
        drv.main(["--path", path, "--task", "1001"])
