"""The project's own torch restatement of EfficientSAM (freefine_amd/sam.py runs the same network on the device), the G16 cases, and their inputs from seeds.

sam_ref is written from the network's description: a ViT encoder without class token (pre-LayerNorm blocks, global attention, eps 1e-6) with a 1x1 / LayerNorm /
3x3 / LayerNorm neck; SAM's prompt encoder (random-Fourier features of at most six points + one learned row per label); the two-way transformer (token self
attention, token -> image, MLP, image -> token; a final token -> image) with attention projected down by 2 in the cross attentions; two k = s = 2 transposed
convolutions (GroupNorm(1) + GELU after the first, GELU after the second); one hypernetwork MLP per mask token whose output is multiplied with every pixel; an
IoU head; bicubic upsampling; the three multi-mask outputs sorted by predicted IoU.  tests/test_sam_cpu.py pins it (mode "f64") to what the reference's source
computes on the same seeded weights (tests/golden/g16_efficient_sam.npz), and the GPU tests compare the device against it: the reference does not travel.

mode: "f64" -- everything in fp64 except what the reference itself evaluates in fp32 whatever the model's type (the random-Fourier features); "f32" -- torch fp32
on the CPU; "x3" / "bf16" -- the ENCODER in the emulated arithmetic of the device modes (tests/test_text_native_cpu.py: split-bf16 products with fp32 storage /
bf16 products and storage, sums in fp64), the decoder in fp64 on the embedding as the device would hold it (fp32)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from freefine_amd import sam as S
from test_text_native_cpu import _mm, _store

# name -> (configuration, (H, W) of the image, kind of prompt)
G16_CASES = {
    "tiny_48x80_box": ("tiny", (48, 80), "box"),
    "tiny_128x128_points": ("tiny", (128, 128), "points"),
    "tiny_200x136_q2": ("tiny", (200, 136), "q2"),
    "vits_480x640_box": ("vits", (480, 640), "box"),
}


def smooth_image(H, W, seed):
    """a smooth synthetic uint8 image [H, W, 3]: a few low-frequency waves per channel and a bright disc, so that a box has something to hold"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = g.uniform(0.5, 3.0) / H, g.uniform(0.5, 3.0) / W, g.uniform(0, 2 * np.pi)
            img[..., c] += g.uniform(20, 45) * np.sin(2 * np.pi * (fy * y + fx * x) + ph)
    disc = ((y - 0.45 * H) ** 2 / (0.2 * H) ** 2 + (x - 0.55 * W) ** 2 / (0.22 * W) ** 2) < 1.0
    img += 70.0 * disc[..., None]
    return np.clip(np.rint(img + 110.0), 0, 255).astype(np.uint8)


def g16_prompts(hw, kind):
    """(points fp32 [1, Q, P, 2] as (x, y), labels int64 [1, Q, P])"""
    H, W = hw
    if kind == "box":
        pts, lab = [[[0.3 * W, 0.2 * H], [0.8 * W, 0.7 * H]]], [[2, 3]]
    elif kind == "points":
        pts, lab = [[[0.55 * W, 0.45 * H], [0.5 * W, 0.55 * H]]], [[1, 1]]
    else:        # two queries of seven points: the seventh is cut; the second query has an absent point in the middle
        a = [[0.55 * W, 0.45 * H], [0.5 * W, 0.5 * H], [0.6 * W, 0.4 * H], [0.45 * W, 0.42 * H], [0.62 * W, 0.52 * H], [0.5 * W, 0.35 * H], [0.1 * W, 0.9 * H]]
        b = [[0.2 * W, 0.8 * H], [0.25 * W, 0.75 * H], [-1.0, -1.0], [0.15 * W, 0.85 * H], [0.3 * W, 0.7 * H], [0.22 * W, 0.9 * H], [0.9 * W, 0.1 * H]]
        pts, lab = [a, b], [[1] * 7, [1, 1, -1, 1, 1, 1, 1]]
    return torch.tensor([pts], dtype=torch.float32), torch.tensor([lab], dtype=torch.int64)


def g16_inputs(name, seed):
    """(configuration, seeded state, uint8 image [1, H, W, 3], points, labels) of a G16 case; `seed`: the state's, recorded in the golden per configuration"""
    cname, hw, kind = G16_CASES[name]
    cfg = S.sam_config(cname)
    pts, lab = g16_prompts(hw, kind)
    return cfg, S.synthetic_state(cfg, seed), smooth_image(hw[0], hw[1], 160 + hw[0] + hw[1])[None], pts, lab


def _ln(x, w, b, eps):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def _attention(q, k, v, heads, mode):
    """softmax(q k^T / sqrt(d)) v per head over [N, S, C] projections; the emulated modes normalise after the second product, like the kernels"""
    N, Sq, C = q.shape
    d = C // heads
    sp = lambda t: t.reshape(N, t.shape[1], heads, d).transpose(1, 2)
    q, k, v = sp(q), sp(k), sp(v)
    s = _mm(q, k, mode) * d ** -0.5
    e = torch.exp(s - s.amax(-1, keepdim=True))
    a = _mm(e, v.transpose(-1, -2), mode) / e.sum(-1, keepdim=True)
    return a.transpose(1, 2).reshape(N, Sq, C)


def encode_ref(cfg, st, images_u8, mode):
    """uint8 [B, H, W, 3] -> embedding [B, n, D]; st: the state in the computing type"""
    dt = st["image_encoder.pos_embed"].dtype
    mm = "f64" if mode == "f32" else mode                     # (fp32: plain products in the tensors' own type)
    keep = (lambda t: t) if mode in ("f64", "f32") else (lambda t: _store(t, mode))
    e, C, ps, g = "image_encoder.", cfg.embed_dim, cfg.patch, cfg.img_size // cfg.patch
    x = (torch.as_tensor(images_u8).permute(0, 3, 1, 2).float() / 255).to(dt)          # ToTensor rounds byte / 255 to fp32
    B = x.shape[0]
    if x.shape[2] != cfg.img_size or x.shape[3] != cfg.img_size:
        x = F.interpolate(x, (cfg.img_size, cfg.img_size), mode="bilinear")
    mean, std = (torch.tensor(v, dtype=torch.float32).to(dt).view(1, 3, 1, 1) for v in (S.PIXEL_MEAN, S.PIXEL_STD))
    x = keep((x - mean) / std)
    rows = x.reshape(B, 3, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * ps * ps)
    lin = lambda t, p: _mm(t, st[p + ".weight"].reshape(st[p + ".weight"].shape[0], -1), mm) + (st[p + ".bias"] if p + ".bias" in st else 0)
    x = keep(lin(rows, e + "patch_embed.proj") + keep(S.abs_pos(st[e + "pos_embed"], g)))
    for i in range(cfg.depth):
        p = f"{e}blocks.{i}."
        y = keep(_ln(x, st[p + "norm1.weight"], st[p + "norm1.bias"], cfg.ln_eps))
        q, k, v = keep(lin(y, p + "attn.qkv")).split(C, dim=-1)
        x = keep(x + lin(keep(_attention(q, k, v, cfg.num_heads, mm)), p + "attn.proj"))
        y = keep(_ln(x, st[p + "norm2.weight"], st[p + "norm2.bias"], cfg.ln_eps))
        x = keep(x + lin(keep(F.gelu(lin(y, p + "mlp.fc1"))), p + "mlp.fc2"))
    D = cfg.neck
    x = keep(_ln(keep(lin(x, e + "neck.0")), st[e + "neck.1.weight"], st[e + "neck.1.bias"], cfg.ln_eps))
    cols = F.unfold(x.transpose(1, 2).reshape(B, D, g, g), 3, padding=1).transpose(1, 2)              # [B, n, D * 9], columns (channel, ky, kx)
    return keep(_ln(keep(lin(cols, e + "neck.2")), st[e + "neck.3.weight"], st[e + "neck.3.bias"], cfg.ln_eps))


def decode_ref(cfg, st, emb, pts, lab, out_hw):
    """emb [B, n, D] in the computing type, prompts as S.prepare_prompts gives them -> dict(iou [B, Q, 3], low [B, Q, 3, 4g, 4g], full [B, Q, 3, H, W]), sorted
    by predicted IoU descending"""
    dt = emb.dtype
    B, n, D = emb.shape
    N, g, heads = pts.shape[0], cfg.img_size // cfg.patch, cfg.dec_heads
    Q = N // B
    pr, m, t = "prompt_encoder.", "mask_decoder.", "mask_decoder.transformer."
    gauss = st[pr + "pe_layer.positional_encoding_gaussian_matrix"].float()
    # fp32 whatever the model's type: the matrix stays a float32 buffer in the reference, and the coordinates are cast to it
    point_pe = S.fourier_features((pts + 0.5) / cfg.img_size, gauss)
    for k, nm in ((-1, "invalid_points"), (1, "point_embeddings"), (2, "bbox_top_left_embeddings"), (3, "bbox_bottom_right_embeddings")):
        point_pe = point_pe + st[pr + nm + ".weight"][:, None, :] * (lab == k)[:, :, None]
    tokens = torch.cat([torch.cat([st[m + "iou_token.weight"], st[m + "mask_tokens.weight"]], 0).unsqueeze(0).expand(N, -1, -1), point_pe.to(dt)], dim=1)
    key_pe = S.dense_pe(gauss, g)[None]                        # fp32, added to keys of the computing type
    lin = lambda x, p: F.linear(x, st[p + ".weight"], st[p + ".bias"])
    ln = lambda x, p: _ln(x, st[p + ".weight"], st[p + ".bias"], 1e-5)

    def attn(p, q, k, v):
        return lin(_attention(lin(q, p + "q_proj"), lin(k, p + "k_proj"), lin(v, p + "v_proj"), heads, "f64"), p + "out_proj")
    queries, keys = tokens, emb[:, None].expand(B, Q, n, D).reshape(N, n, D)
    for i in range(cfg.dec_depth):
        p = f"{t}layers.{i}."
        if i > 0:
            queries = queries + tokens
        queries = ln(queries + attn(p + "self_attn.", queries, queries, queries), p + "norm1")
        queries = ln(queries + attn(p + "cross_attn_token_to_image.", queries + tokens, keys + key_pe, keys), p + "norm2")
        queries = ln(queries + lin(F.gelu(lin(queries, p + "mlp.layers.0.0")), p + "mlp.fc"), p + "norm3")
        keys = ln(keys + attn(p + "cross_attn_image_to_token.", keys + key_pe, queries + tokens, queries), p + "norm4")
    queries = ln(queries + attn(t + "final_attn_token_to_image.", queries + tokens, keys + key_pe, keys), t + "norm_final_attn")
    u = m + "final_output_upscaling_layers."
    x = F.conv_transpose2d(keys.transpose(1, 2).reshape(N, D, g, g), st[u + "0.0.weight"], st[u + "0.0.bias"], stride=2)
    x = F.gelu(F.group_norm(x, 1, st[u + "0.1.weight"], st[u + "0.1.bias"], 1e-5))
    x = F.gelu(F.conv_transpose2d(x, st[u + "1.0.weight"], st[u + "1.0.bias"], stride=2))

    def mlp(x, p):
        return lin(F.gelu(lin(F.gelu(lin(x, p + "layers.0.0")), p + "layers.1.0")), p + "fc")
    nm = cfg.num_masks + 1
    hyper = torch.stack([mlp(queries[:, 1 + i], m + f"output_hypernetworks_mlps.{i}.") for i in range(nm)], dim=1)
    low = (hyper @ x.flatten(2)).view(N, nm, 4 * g, 4 * g)[:, 1:]
    iou = mlp(queries[:, 0], m + "iou_prediction_head.")[:, 1:]
    full = F.interpolate(low, out_hw, mode="bicubic")
    iou = iou.reshape(B, Q, -1)
    order = torch.argsort(iou, dim=-1, descending=True)
    pick = lambda a: torch.take_along_dim(a.reshape(B, Q, nm - 1, *a.shape[-2:]), order[..., None, None], dim=2)
    return dict(iou=torch.take_along_dim(iou, order, dim=2), low=pick(low), full=pick(full), order=order)


def sam_ref(cfg, state, images_u8, points, labels, mode="f64", out_hw=None):
    """images uint8 [B, H, W, 3], points [B, Q, P, 2], labels [B, Q, P] -> dict(emb [B, n, D], iou, low, full, order) in the computing type (module docstring)"""
    dt = torch.float32 if mode == "f32" else torch.float64
    st = {k: v.detach().to(dt) for k, v in S.check_state(cfg, state).items()}
    hw = tuple(np.asarray(images_u8).shape[1:3])
    with torch.no_grad():
        emb = encode_ref(cfg, st, images_u8, mode)
        pts, lab = S.prepare_prompts(cfg, points, labels, hw)
        if mode in ("x3", "bf16"):
            emb = emb.float().double()
        out = decode_ref(cfg, st, emb, pts, lab, out_hw or hw)
    out["emb"] = emb
    return out
