"""The pre-LayerNorm transformer block of the project's four towers -- the DINOv2 / DINO encoder (dino.py, which depth.py also runs), the CLIP image tower
(clipvision.py) and the CLIP text encoder (text.py) -- and the plumbing around it that they share.  The towers keep their own configs, state layouts, input
transforms and heads; what a block computes, how its weights are packed and how V^T is buffered is decided here alone.

    y = LN1(x); q | k = Linear(y) (one GEMM); V^T = Linear(y) (transposed-output GEMM); a = softmax(q k^T / sqrt(Dh) (+ causal)) v per head; x += o(a);
    y = LN2(x); x += fc2(act(fc1(y)))                     (the residuals and the activation are GEMM epilogues)

dtype float32 = parity mode (exact-fp32 MFMA), float32 with x3 = split-bf16 (FFN_BF16X3: operands as hi + lo bf16 pairs, three bf16 MFMAs per product term,
fp32 accumulation), bfloat16 = fast mode.  Split-bf16: weights are packed with ops.pack_linear(x3=True); LN1 / LN2 write the pair rows their GEMMs read
(`ffn_layernorm_pair`), attention and fc1 write pair rows for the GEMM behind them; the residual stream and V^T stay fp32.

V^T: ONE buffer per forward (`vt_buffer`), [B, C, ceil8(S)] in the activation type, zero-filled once and handed as `out=` to every layer's V^T GEMM.  The
padding columns (S not a multiple of 8) are multiplied by P = 0 in the attention kernels and must be finite; no GEMM writes them, so zeroing them once holds
for all layers.  The stream orders a layer's attention before the next layer's V^T GEMM, and no tower keeps a V^T.

The post-LayerNorm block with cross-attention to a second sequence (BERT as BLIP runs it: irs.py) is CrossBlock / run_cross_block further down."""
import math
from collections import namedtuple

import torch

from . import ops

Block = namedtuple("Block", "ln1 ln2 qk v o fc1 fc2")       # ln*: (gamma, beta) fp32; the linears: (packed weight, fp32 bias)


def check_mode(dtype, x3):
    assert dtype in (torch.float32, torch.bfloat16)
    if x3 and dtype != torch.float32:
        raise ValueError(f"x3=True (split-bf16) takes dtype=torch.float32: operands are split from fp32 values (dtype={dtype})")


def ceil8(n):
    return (n + 7) // 8 * 8


def pack_block(ln1, ln2, qk, v, o, fc1, fc2, dtype, x3=False):
    """fp32 (weight, bias) pairs on the tower's device -> Block.  Whatever a tower folds into a weight (DINOv2's LayerScale) is folded before this, so in
    split-bf16 mode before the split."""
    norm = lambda p: (p[0].contiguous(), p[1].contiguous())
    lin = lambda p: (ops.pack_linear(p[0].contiguous(), dtype, x3=x3), p[1].contiguous())
    return Block(norm(ln1), norm(ln2), lin(qk), lin(v), lin(o), lin(fc1), lin(fc2))


def vt_buffer(x):
    """the one V^T buffer (module docstring) of a forward whose residual stream is x [B, S, C]"""
    B, S, C = x.shape
    return torch.zeros(B, C, ceil8(S), dtype=x.dtype, device=x.device)


def run_block(b, x, vt, *, heads, eps, act, hidden, x3=False, causal=False, splitk=0):
    """x [B, S, C] (the residual stream) -> the block's output, the same shape.  vt: vt_buffer(x); act: "gelu" / "qgelu", fc1's epilogue;
    hidden: fc2's contraction length; splitk: 0 leaves the K split to the library, 1 forbids it (the text encoder's bit-identity per prompt)."""
    _, S, C = x.shape
    y = ops.layernorm(x, *b.ln1, eps=eps, pair=x3)
    qk = ops.linear(y, *b.qk, K=C, splitk=splitk)                                                     # [B, S, 2C]: q | k
    ops.linear(y, *b.v, K=C, rows_per_batch=S, transposed_ld=vt.shape[-1], splitk=splitk, out=vt)      # V^T [B, C, S']
    a = ops.attention(qk, qk[..., C:], vt, heads, (C // heads) ** -0.5, None, Sk=S, C=C, x3=x3, out_pair=x3, causal=causal)
    x = ops.linear(a, *b.o, K=C, residual=x, splitk=splitk)
    y = ops.layernorm(x, *b.ln2, eps=eps, pair=x3)
    h = ops.linear(y, *b.fc1, K=C, out_pair=x3, splitk=splitk, **{act: True})
    return ops.linear(h, *b.fc2, K=hidden, residual=x, splitk=splitk)


# ---------------------------------------------------------------------------------------------------------------------
# the post-LayerNorm block that also attends to a second sequence (BERT with cross-attention: BLIP's text encoder, irs.py)
# ---------------------------------------------------------------------------------------------------------------------
# lns / lnc / lnm: the LayerNorms behind self-attention, cross-attention and the MLP; cq / co: the cross-attention's query and output projections.  The
# cross-attention's K and V projections read the second sequence only, so they are no part of the block: the tower projects them for all its layers before
# the first block runs (cross_kv).
CrossBlock = namedtuple("CrossBlock", "qk v o lns cq co lnc fc1 fc2 lnm")


def pack_cross_block(qk, v, o, lns, cq, co, lnc, fc1, fc2, lnm, dtype, x3=False):
    """fp32 (weight, bias) pairs on the tower's device -> CrossBlock"""
    norm = lambda p: (p[0].contiguous(), p[1].contiguous())
    lin = lambda p: (ops.pack_linear(p[0].contiguous(), dtype, x3=x3), p[1].contiguous())
    return CrossBlock(lin(qk), lin(v), lin(o), norm(lns), lin(cq), lin(co), norm(lnc), lin(fc1), lin(fc2), norm(lnm))


def cross_kv(e, wk, wv, layers, C):
    """The cross-attention operands of all `layers` blocks from the second sequence e [B, Sk, Ce] (activation type; split-bf16: fp32, or pair rows, which are
    split once here): wk = (the layers' K weights stacked into one packed [layers * C, Ce] weight, the stacked bias), wv = per layer (packed weight, bias) ->
    (ck: per layer a [B, Sk, C] column view of ONE [B, Sk, layers * C] GEMM result, cvt: per layer V^T [B, C, ceil8(Sk)] of one zero-filled buffer -- the padding
    columns are written by no GEMM and stay zero, as in vt_buffer)."""
    B, Sk = e.shape[0], e.shape[1]
    x3 = ops.is_x3(wk[0])
    if x3 and ops.pair_width(e) is None:
        e = ops.split_pair(e)
    Ce = ops.pair_width(e) or e.shape[-1]
    k = ops.linear(e, *wk, K=Ce)
    cvt = torch.zeros(layers, B, C, ceil8(Sk), dtype=k.dtype, device=k.device)
    for i in range(layers):
        ops.linear(e, *wv[i], K=Ce, rows_per_batch=Sk, transposed_ld=cvt.shape[-1], out=cvt[i])
    return [k[..., i * C:(i + 1) * C] for i in range(layers)], [cvt[i] for i in range(layers)]


def run_cross_block(b, x, vt, ck, cvt, *, heads, eps, hidden, kmask=None, x3=False, splitk=0):
    """x [B, S, C] -> the block's output, the same shape:

        x = LN(x + o(attn(q = k = v = x, key mask)));  x = LN(x + co(attn(q = cq(x), k = ck, v = cvt)));  x = LN(x + fc2(gelu(fc1(x))))

    vt: vt_buffer(x); ck [B, Sk, C] (may be a column view) and cvt [B, C, ceil8(Sk)]: cross_kv's; kmask: None, or per row of x one uint8 [>= S] device tensor
    (4-byte aligned; non-zero = the key is attended to), a list of B or of one shared by all rows.  Every residual is its GEMM's epilogue and every LayerNorm
    normalises that sum.  Post-LN: the residual stream IS the next GEMM's operand, so in split-bf16 mode it stays fp32 and ops.linear splits it; attention and
    fc1 still hand pair rows to the GEMM behind them."""
    B, S, C = x.shape
    scale = (C // heads) ** -0.5
    xa = ops.split_pair(x) if x3 else x                                                                # split once for the two GEMMs that read it
    qk = ops.linear(xa, *b.qk, K=C, splitk=splitk)                                                     # [B, S, 2C]: q | k
    ops.linear(xa, *b.v, K=C, rows_per_batch=S, transposed_ld=vt.shape[-1], splitk=splitk, out=vt)     # V^T [B, C, S']
    passes = None if kmask is None else [[ops.AttnEntrySpec(i, i, kmask=kmask[i % len(kmask)]) for i in range(B)]]
    a = ops.attention(qk, qk[..., C:], vt, heads, scale, passes, Sk=S, C=C, x3=x3, out_pair=x3)
    x = ops.layernorm(ops.linear(a, *b.o, K=C, residual=x, splitk=splitk), *b.lns, eps=eps)
    q = ops.linear(x, *b.cq, K=C, splitk=splitk)
    a = ops.attention(q, ck, cvt, heads, scale, None, Sk=ck.shape[1], C=C, x3=x3, out_pair=x3)
    x = ops.layernorm(ops.linear(a, *b.co, K=C, residual=x, splitk=splitk), *b.lnc, eps=eps)
    h = ops.linear(x, *b.fc1, K=C, out_pair=x3, splitk=splitk, gelu=True)
    return ops.layernorm(ops.linear(h, *b.fc2, K=hidden, residual=x, splitk=splitk), *b.lnm, eps=eps)


def im2col(x, ps):
    """[B, 3, H, W] -> [B (H/ps)(W/ps), 3 ps ps]: one row per patch (row-major over the patch grid), columns ordered (channel, ky, kx) like the patch
    embedding's Conv2d(kernel = stride = patch) weight .reshape(C, -1)"""
    B, Cc, H, W = x.shape
    ph, pw = H // ps, W // ps
    return x.reshape(B, Cc, ph, ps, pw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * ph * pw, Cc * ps * ps)


def u8_batch(images, keep, device):
    """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device), keep = None or (rule, m1, m2) as in ops.resize_pil_u8 (masks uint8 [B, H, W],
    host or device) -> the same, contiguous on the device"""
    img = torch.as_tensor(images)
    assert img.dtype == torch.uint8 and img.ndim == 4 and img.shape[-1] == 3
    img = img.to(device).contiguous()
    if keep is not None:
        keep = (keep[0],) + tuple(None if m is None else torch.as_tensor(m).to(device).contiguous() for m in keep[1:])
    return img, keep


def clip_crop_u8(images, keep, size, device):
    """CLIP's geometric transform on the device (clip/clip.py _transform: Resize(size, BICUBIC) of the short side, CenterCrop(size)), after image * keep mask: one
    ffn_resize_pil_u8 with a crop window.  images / keep as u8_batch takes them -> uint8 [B, size, size, 3].  The CLIP image towers and the ImageReward
    score's BLIP tower (irs.py) share it."""
    img, keep = u8_batch(images, keep, device)
    oh, ow = ops.torchvision_resize_size(img.shape[1], img.shape[2], size)
    return ops.resize_pil_u8(img, oh, ow, "bicubic", crop=ops.center_crop_window(oh, ow, size), keep=keep)


def patch_rows_u8(small, lut, patch, K, dtype, x3):
    """resized uint8 images -> the patch GEMM's operand rows: the activation type's, or the pair rows of split-bf16 (straight from the bytes)"""
    if x3:
        return ops.vit_patch_rows_pair(small, lut, patch, K)
    return ops.vit_patch_rows(small, lut, patch, K, dtype)


def embed_patches(a, w, bias, K, pos, cls_row, B):
    """operand rows a [B n, K] (split-bf16: pair rows, or fp32 rows that ops.linear splits), positional embedding pos [n, C] (the GEMM's residual) and the
    class row [1, C], both in the activation type -> tokens [B, 1 + n, C]"""
    n, C = pos.shape
    res = pos.unsqueeze(0).expand(B, -1, -1).reshape(B * n, C).contiguous()
    t = ops.linear(a, w, bias, K=K, residual=res)
    return torch.cat([cls_row.unsqueeze(0).expand(B, -1, -1), t.view(B, n, C)], dim=1).contiguous()


def clip_layer_shapes(cfg, prefix=""):
    """name -> shape of the encoder.layers.N.* parameters of a CLIP tower, in state_dict order"""
    C, I = cfg.hidden_size, cfg.intermediate_size
    sh = {}
    for i in range(cfg.num_hidden_layers):
        p = f"{prefix}encoder.layers.{i}."
        for nm in ("k_proj", "v_proj", "q_proj", "out_proj"):
            sh[p + f"self_attn.{nm}.weight"], sh[p + f"self_attn.{nm}.bias"] = (C, C), (C,)
        sh[p + "layer_norm1.weight"], sh[p + "layer_norm1.bias"] = (C,), (C,)
        sh[p + "mlp.fc1.weight"], sh[p + "mlp.fc1.bias"], sh[p + "mlp.fc2.weight"], sh[p + "mlp.fc2.bias"] = (I, C), (I,), (C, I), (C,)
        sh[p + "layer_norm2.weight"], sh[p + "layer_norm2.bias"] = (C,), (C,)
    return sh


def pack_clip_layers(cfg, f, out):
    """f(name) -> fp32 host tensor of a parameter; adds the layers' host tensors to `out` as "<i>.<field>.{w,b}": q | k rows of one GEMM, V apart (its GEMM
    writes V^T)"""
    for i in range(cfg.num_hidden_layers):
        p, a = f"encoder.layers.{i}.", f"encoder.layers.{i}.self_attn."
        out[f"{i}.ln1.w"], out[f"{i}.ln1.b"] = f(p + "layer_norm1.weight"), f(p + "layer_norm1.bias")
        out[f"{i}.ln2.w"], out[f"{i}.ln2.b"] = f(p + "layer_norm2.weight"), f(p + "layer_norm2.bias")
        out[f"{i}.qk.w"] = torch.cat([f(a + "q_proj.weight"), f(a + "k_proj.weight")], 0).contiguous()
        out[f"{i}.qk.b"] = torch.cat([f(a + "q_proj.bias"), f(a + "k_proj.bias")], 0).contiguous()
        out[f"{i}.v.w"], out[f"{i}.v.b"] = f(a + "v_proj.weight"), f(a + "v_proj.bias")
        out[f"{i}.o.w"], out[f"{i}.o.b"] = f(a + "out_proj.weight"), f(a + "out_proj.bias")
        out[f"{i}.fc1.w"], out[f"{i}.fc1.b"] = f(p + "mlp.fc1.weight"), f(p + "mlp.fc1.bias")
        out[f"{i}.fc2.w"], out[f"{i}.fc2.b"] = f(p + "mlp.fc2.weight"), f(p + "mlp.fc2.bias")
    return out


def clip_blocks(cfg, host, device, dtype, x3):
    """the host tensors of pack_clip_layers, uploaded and packed -> [Block]"""
    pair = lambda k: (host[k + ".w"].to(device), host[k + ".b"].to(device))
    return [pack_block(*(pair(f"{i}.{n}") for n in Block._fields), dtype, x3) for i in range(cfg.num_hidden_layers)]


def draw_state(shapes, seed, fan_in_first=()):
    """name -> shape => seeded random fp32 tensors of a plausible scale, drawn in the order of `shapes`: for tests and benchmarks without a checkpoint.
    fan_in_first: name fragments of the weights whose fan-in is shape[0] (ConvTranspose2d stores [in, out, k, k])"""
    g = torch.Generator().manual_seed(seed)
    st = {}
    for k, shp in shapes.items():
        if "norm" in k and k.endswith(".weight"):
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(".gamma"):
            t = 0.5 + 0.25 * torch.rand(shp, generator=g)
        elif k.endswith(".bias"):
            t = 0.05 * torch.randn(shp, generator=g)
        elif k.endswith(("pos_embed", "cls_token", "mask_token", "class_embedding", "position_embedding.weight")):
            t = 0.2 * torch.randn(shp, generator=g)
        else:
            fan_in = shp[0] if any(s in k for s in fan_in_first) else math.prod(shp[1:])
            t = torch.randn(shp, generator=g) / math.sqrt(fan_in)
        st[k] = t.float()
    return st
