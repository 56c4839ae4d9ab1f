"""CPU: the split-bf16 mode of the metric suite's ViT towers (HipDinoV2, HipDino, HipCLIPVision with x3=True) as far as it runs without a device: the ABI of
ffn_vit_patch_rows_pair with every refusal (nothing is launched), a test-local restatement of the DINO / DINOv2 forward (fp64 sums; the split-bf16 and the bf16
arithmetic emulated) against oracle/dpt.py in fp64, the separation of the three arithmetics that gives the GPU bound of tests/test_towers_x3_gpu.py its teeth,
and the attention kernels the towers' ragged sequence lengths run."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_consistency_cpu import dino16_ref, g15_inputs, vision_case, vision_ref
from test_dino_cpu import g14_inputs
from test_text_native_cpu import _mm, _store, attn_desc, kernel_name, scale_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kind, name, H, W, B): the G14 (DINOv2: patch 14, LayerScale) and G15 (DINO: patch 16, none) cases the towers are held to in split-bf16 mode
DINO_CASES = [("g14", "tiny", 224, 224, 2), ("g14", "tiny", 518, 518, 1), ("g14", "mini", 224, 224, 2), ("g15", "tiny16", 224, 224, 2), ("g15", "tiny16", 224, 288, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_patch_rows_pair_is_declared_bound_exported_and_refuses_on_the_host():
    """ffn_vit_patch_rows_pair refuses, before any launch: what ffn_vit_patch_rows refuses (null pointers, sides outside 1 .. FFN_IMGPREP_MAX_SIDE, images that are
    not whole patches, a patch outside 1 .. 256), K below the patch's columns, K that is not a multiple of 8; the old entry still refuses FFN_BF16X3"""
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    assert re.search(r"\bint\s+ffn_vit_patch_rows_pair\s*\(", header) and "ffn_vit_patch_rows_pair" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ffn_vit_patch_rows_pair") and lib.ffn_version() >= 7
    P, lim = 0x10000, _lib.IMGPREP_MAX_SIDE                   # P: never dereferenced, validation fails first

    def rows(src=P, lut=P, out=P, B=2, H=224, W=224, patch=14, K=608):
        return lib.ffn_vit_patch_rows_pair(None, src, lut, out, B, H, W, patch, K)
    bad = [(dict(src=None), b"null"), (dict(lut=None), b"null"), (dict(out=None), b"null"),
           (dict(H=lim + 14), b"bad shape"), (dict(W=lim + 14), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=-14), b"bad shape"), (dict(B=0), b"bad shape"),
           (dict(H=225), b"whole patches"), (dict(W=200), b"whole patches"), (dict(patch=0), b"whole patches"), (dict(patch=257, H=257, W=257, K=198152), b"whole patches"),
           (dict(K=584), b"K=584 below"), (dict(K=0), b"K=0 below"), (dict(patch=16, H=224, W=224, K=760), b"K=760 below"),
           (dict(K=590), b"multiple of 8"), (dict(K=588), b"multiple of 8"), (dict(K=604), b"multiple of 8")]
    for kw, msg in bad:
        assert rows(**kw) == -22, kw
        err = lib.ffn_last_error()
        assert msg in err and err.startswith(b"vit_patch_rows_pair"), (kw, err)
    # the old entry is what it was: no split-bf16 output
    assert lib.ffn_vit_patch_rows(None, _lib.FFN_BF16X3, P, P, P, 2, 224, 224, 14, 592) == -22
    err = lib.ffn_last_error()
    assert b"dtype" in err and err.startswith(b"vit_patch_rows:"), err


# ---------------------------------------------------------------------------------------------------------------------
# the DINO / DINOv2 forward restated (test-local; fp64 sums everywhere)
# ---------------------------------------------------------------------------------------------------------------------
def dino_ref(cfg, state, x, mode="f64"):
    """DinoVisionTransformer(x) -> the final LayerNorm's class token, restated from the hub layout the way the towers run it: im2col rows W_patch^T + bias + pos,
    class row, the blocks (softmax(q k^T / 8) v per head, normalised after the second product as the kernels do; LayerScale folded into proj / fc2 BEFORE the
    operands are split; erf-gelu MLP), final LayerNorm of the class rows.  x [B, 3, H, W] -> fp64 [B, C].  mode "f64", or a device mode emulated like vision_ref
    of tests/test_consistency_cpu.py: "x3" = split-bf16 products of the fp32-rounded operands, fp32 storage; "bf16" = bf16 products and storage (the stored
    positional and class rows included); sums in fp64.  The positional embedding is interpolated by the oracle's own function (in fp32, as the reference and
    the towers do)."""
    import torch.nn.functional as F
    from oracle import dpt as OD
    st = {k: v.double() for k, v in state.items()}
    C, nh, eps, ps = cfg.embed_dim, cfg.num_heads, cfg.ln_eps, cfg.patch
    B, _, H, W = x.shape
    ph, pw = H // ps, W // ps
    keep = lambda t: _store(t, mode)
    ln = lambda t, p: F.layer_norm(t, (C,), st[p + ".weight"], st[p + ".bias"], eps)

    def lin(t, p, gamma=None):
        w, b = st[p + ".weight"], st[p + ".bias"]
        if gamma is not None:                                 # folded at pack time (the towers do it in fp32, before the split)
            w, b = (w * gamma[:, None], b * gamma) if mode == "f64" else ((w.float() * gamma.float()[:, None]).double(), (b.float() * gamma.float()).double())
        return _mm(t, w, mode) + b
    rows = keep(x.double().reshape(B, 3, ph, ps, pw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, ph * pw, 3 * ps * ps))
    pos = OD.interpolate_pos_encoding(cfg, st["pos_embed"], ph * pw, H, W)[0]
    t = keep(_mm(rows, st["patch_embed.proj.weight"].reshape(C, -1), mode) + st["patch_embed.proj.bias"] + keep(pos[1:]))
    cls = keep(st["cls_token"][0] + pos[:1])
    h = torch.cat([cls.expand(B, 1, C), t], dim=1)
    S = h.shape[1]
    scale = (C // nh) ** -0.5
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        y = keep(ln(h, p + "norm1"))
        qkv = keep(lin(y, p + "attn.qkv"))
        heads = lambda u: u.reshape(B, S, nh, C // nh).transpose(1, 2)
        q, k, v = heads(qkv[..., :C]), heads(qkv[..., C:2 * C]), heads(qkv[..., 2 * C:])
        s = _mm(q, k, mode) * scale
        e = torch.exp(s - s.amax(-1, keepdim=True))
        a = _mm(e, v.transpose(-1, -2), mode) / e.sum(-1, keepdim=True)
        a = keep(a.transpose(1, 2).reshape(B, S, C))
        h = keep(h + lin(a, p + "attn.proj", st.get(p + "ls1.gamma")))
        y = keep(ln(h, p + "norm2"))
        u = keep(F.gelu(lin(y, p + "mlp.fc1")))
        h = keep(h + lin(u, p + "mlp.fc2", st.get(p + "ls2.gamma")))
    return keep(ln(h[:, 0], "norm"))


@functools.lru_cache(maxsize=None)
def dino_case(kind, name, H, W, B):
    """(tower configuration, state in hub layout, input, the oracle's class tokens on x.double(), the reference errors {"f32": the oracle in fp32, "x3" / "bf16":
    the emulations} against them) -- computed once, shared with tests/test_towers_x3_gpu.py"""
    from oracle import dpt as OD
    from freefine_amd import dino as FD
    if kind == "g14":
        ocfg, full, x = g14_inputs(name, H, W, B)
        cfg, st = FD.dinov2_config(name), {k[len("pretrained."):]: v for k, v in full.items() if k.startswith("pretrained.")}
        with torch.no_grad():
            f32, want = OD.vit_features(ocfg, full, x, 1)[0][1], OD.vit_features(ocfg, full, x.double(), 1)[0][1]
    else:
        cfg, st, x = g15_inputs(name, H, W, B)
        f32, want = dino16_ref(cfg, st, x), dino16_ref(cfg, st, x.double())
    errs = {"f32": scale_err(f32, want), "x3": scale_err(dino_ref(cfg, st, x, "x3"), want), "bf16": scale_err(dino_ref(cfg, st, x, "bf16"), want)}
    return cfg, st, x, want, errs


@functools.lru_cache(maxsize=None)
def clip_case(name):
    """vision_case of tests/test_consistency_cpu.py with the split-bf16 emulation's error beside the two it records"""
    cfg, st, x, want, errs = vision_case(name)
    return cfg, st, x, want, dict(errs, x3=scale_err(vision_ref(cfg, st, x, "x3"), want))


@pytest.mark.parametrize("kind,name,H,W,B", DINO_CASES)
def test_dino_restatement_equals_the_oracle_fp64_and_the_arithmetics_separate(kind, name, H, W, B):
    """mode f64 equals oracle.dpt.vit_features on x.double() to 1e-10 of the output scale; the split-bf16 emulation sits above the fp32 oracle's error and below a
    hundredth of the bf16 emulation's: the separation the GPU bound (2 x the emulation's error) relies on"""
    cfg, st, x, want, errs = dino_case(kind, name, H, W, B)
    e = scale_err(dino_ref(cfg, st, x), want)
    print(f"DINO restatement vs oracle fp64 ({kind} {name} {H}x{W} B={B}): {e:.2e}; fp32 oracle {errs['f32']:.2e}, emulated split-bf16 {errs['x3']:.2e}, "
          f"emulated bf16 {errs['bf16']:.2e} (|y| max {want.abs().max():.3f})")
    assert want.shape == (B, cfg.embed_dim) and want.dtype == torch.float64 and e <= 1e-10
    assert errs["f32"] < errs["x3"] < errs["bf16"] / 100


@pytest.mark.parametrize("name", ["tiny", "vitb32"])
def test_clip_emulation_separates_the_arithmetics(name):
    *_, errs = clip_case(name)
    print(f"CLIP vision {name}: fp32 module {errs['f32']:.2e}, emulated split-bf16 {errs['x3']:.2e}, emulated bf16 {errs['bf16']:.2e}")
    assert errs["f32"] < errs["x3"] < errs["bf16"] / 100


def test_x3_requires_float32():
    """the refusal needs no device: it comes before anything is uploaded"""
    from freefine_amd.clipvision import HipCLIPVision
    from freefine_amd.dino import HipDino, HipDinoV2
    cfg, st, *_ = dino_case("g14", "tiny", 224, 224, 2)
    with pytest.raises(ValueError, match="x3"):
        HipDinoV2(cfg, st, dtype=torch.bfloat16, device="cpu", x3=True)
    cfg, st, *_ = dino_case("g15", "tiny16", 224, 224, 2)
    with pytest.raises(ValueError, match="x3"):
        HipDino(cfg, st, dtype=torch.bfloat16, device="cpu", x3=True)
    cfg, st, *_ = vision_case("tiny")
    with pytest.raises(ValueError, match="x3"):
        HipCLIPVision(cfg, st, dtype=torch.bfloat16, device="cpu", x3=True)


def test_padded_patch_embedding_lengths():
    """the contraction length of the patch embedding: whole 16-byte chunks as before, whole 32-column blocks in split-bf16 mode (both operands blocked)"""
    pad = lambda K, e: (K + e - 1) // e * e
    assert [pad(3 * p * p, 8) for p in (14, 16, 32)] == [592, 768, 3072] and [pad(3 * p * p, 32) for p in (14, 16, 32)] == [608, 768, 3072]


def test_metric_builders_forward_x3(monkeypatch):
    """_dino_model / _clip_model / _dino16_model pass x3 on only where they build the tower from a state dict; a ready model goes through as it is"""
    from freefine_amd import clipvision, dino
    from freefine_amd import metrics as FM
    seen = []

    class Stub:
        def __init__(self, cfg, state, dtype=None, device="cuda:0", x3=False):
            seen.append((type(self).__name__, getattr(cfg, "name", cfg), dtype, x3))
    for mod, cls in ((dino, "HipDinoV2"), (dino, "HipDino"), (clipvision, "HipCLIPVision")):
        monkeypatch.setattr(mod, cls, type(cls, (Stub,), {}))
    ready = object()
    for fn in (FM._dino_model, FM._clip_model, FM._dino16_model):
        assert fn(ready) is ready and fn(ready, x3=True) is ready
        fn({})
        fn({}, x3=True)
    assert seen == [("HipDinoV2", "vitb", torch.float32, False), ("HipDinoV2", "vitb", torch.float32, True),
                    ("HipCLIPVision", "vitb32", torch.float32, False), ("HipCLIPVision", "vitb32", torch.float32, True),
                    ("HipDino", "vitb16", torch.float32, False), ("HipDino", "vitb16", torch.float32, True)]


def test_driver_takes_precision(tmp_path):
    import json
    from test_consistency_cpu import load_driver
    drv = load_driver()
    path = str(tmp_path / "results.json")
    json.dump({"a": {"instances": {"0": {}}}}, open(path, "w"))
    for extra in ([], ["--precision", "f32"], ["--precision", "x3"]):
        res = drv.main(["--path", path, "--task", "100110000"] + extra)
        assert "not built" in res["FID"] and "clip_weights" in res["BGC"] and "dino_weights" in res["SUBC"]
    with pytest.raises(SystemExit):
        drv.main(["--path", path, "--task", "100000000", "--precision", "bf16"])


# ---------------------------------------------------------------------------------------------------------------------
# the attention kernels of the towers' sequence lengths
# ---------------------------------------------------------------------------------------------------------------------
def test_ragged_sequence_lengths_name_their_split_bf16_attention_kernels():
    """FFN_BF16X3, head dim 64, one plain pass: S = Sk = 50 (CLIP ViT-B/32) runs the short-key kernel, 197 (ViT-B/16) and 257 (ViT-B/14 at 224) the generic
    split-bf16 kernel (Sk % 64 != 0 keeps them off the fast schedules).  Documents the route; nothing is launched."""
    from freefine_amd import _lib
    got = {S: kernel_name(_lib.FFN_BF16X3, attn_desc(S=S, Sk=S, flags=0)) for S in (50, 197, 257)}
    assert got[50].startswith("void xattn_x3_kernel<"), got
    assert got[197] == got[257] == "void attn_x3_kernel<false>(ffn_attn_desc)", got
