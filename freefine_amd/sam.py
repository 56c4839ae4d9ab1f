"""Click-to-mask: EfficientSAM (ViT-T / ViT-S image encoder, SAM's prompt encoder and two-way mask decoder) on the project's HIP kernels -- the network the
reference's application turns two clicks into `ori_mask` with (src/demo/utils.py:26, 40-100; source: evaluation/DesignEdit/sam/efficient_sam/).

    encode    uint8 image of any size -> patch rows (ops.sam_patch_rows: ToTensor, bilinear resize to side x side, normalise, im2col in one kernel) -> patch GEMM with
              the interpolated positional embedding as its residual -> `depth` encoder.Blocks (global attention, no class token) -> neck: 1x1 GEMM, LayerNorm over
              channels, 3x3 convolution, LayerNorm -> embedding fp32 [B, (side / patch)^2, neck].  Once per image, in the mode of the model (fp32, split-bf16, bf16).
    predict   per click, always exact fp32: prompt tokens (host: the random-Fourier encoding of at most six points, as the reference casts them to fp32) ->
              two-way transformer (ops.attention at head dims 32 and 16: 11 tokens against the image's positions and back) -> two k = s = 2 transposed convolutions as
              GEMMs + pixel shuffle, GroupNorm(1) + GELU between them -> hypernetwork product (ops.hyper_masks) -> IoU head -> bicubic upsampling to the image size
              (ops.upsample_bicubic, which also thresholds) -> the three masks sorted by predicted IoU.
    segment   both, and the best mask as uint8 255 / 0.
    generate  the masks of everything in the image -- the `mask_pool` of the edit calls: the single-crop path of SamAutomaticMaskGenerator (source:
              evaluation/GeoDiffuser/GeoDiffuser/segment_anything/automatic_mask_generator.py, utils/amg.py).  encode once; a grid of foreground clicks through
              decode_low (predict up to the low-res logits) in batches; per candidate the predicted-IoU filter, then ops.upsample_bicubic_stats -- the bicubic values
              counted at image size, not stored: area, the two counts of the stability score, the box -- the stability filter, ops.box_nms over all survivors, and
              byte masks of the kept ones only.  Pinned to the reference's code: the point grid, the stability score, the boxes, XYWH and the order of the filters
              (tests/golden/g19_amg.npz); restated from its definition: box NMS (torchvision is not installed).

Keys projected from the fixed dense positional encoding (K pe, Q pe of the cross attentions) are computed once at load and enter as GEMM residuals.  torch is
used for layout plumbing only (pixel shuffle, tiling the embedding per query, sorting three numbers per query).

No EfficientSAM checkpoint exists offline: parity is pinned to the reference's SOURCE on seeded weights (tests/golden/g16_efficient_sam.npz); parity with the published
efficient_sam_vits.pt is unmeasured."""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from . import encoder, ops

PIXEL_MEAN, PIXEL_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PRETRAIN_GRID = 14                  # the positional embedding is stored for 224 / 16 patches a side (+ a class position)
_FULL = dict(img_size=1024, patch=16, depth=12, mlp_ratio=4, neck=256, dec_depth=2, dec_heads=8, dec_mlp=2048, attn_down=2, max_points=6, num_masks=3,
             up_dims=(64, 32), iou_hidden=256, ln_eps=1e-6)
_CONFIGS = {
    "vits": dict(_FULL, embed_dim=384, num_heads=6),
    "vitt": dict(_FULL, embed_dim=192, num_heads=3),
    # for tests: 64 tokens, head dim 64 in the encoder, decoder head dims 32 (self) and 16 (cross) as at full size
    "tiny": dict(_FULL, img_size=128, embed_dim=128, num_heads=2, depth=2, neck=64, dec_heads=2, dec_mlp=128, up_dims=(32, 16), iou_hidden=64),
}


def sam_config(name):
    if name not in _CONFIGS:
        raise ValueError(f"unknown EfficientSAM configuration {name!r} (one of {sorted(_CONFIGS)})")
    return SimpleNamespace(name=name, **_CONFIGS[name])


def _attn_shapes(sh, p, D, inner):
    for n in ("q_proj", "k_proj", "v_proj"):
        sh[p + n + ".weight"], sh[p + n + ".bias"] = (inner, D), (inner,)
    sh[p + "out_proj.weight"], sh[p + "out_proj.bias"] = (D, inner), (D,)


def _norm_shapes(sh, p, D):
    sh[p + ".weight"], sh[p + ".bias"] = (D,), (D,)


def _mlp_shapes(sh, p, dims):
    """MLPBlock: layers.<i>.0 for all but the last Linear, which is fc"""
    for i in range(len(dims) - 2):
        sh[p + f"layers.{i}.0.weight"], sh[p + f"layers.{i}.0.bias"] = (dims[i + 1], dims[i]), (dims[i + 1],)
    sh[p + "fc.weight"], sh[p + "fc.bias"] = (dims[-1], dims[-2]), (dims[-1],)


def sam_shapes(cfg):
    """name -> shape of every entry of EfficientSam.state_dict(), in its order"""
    C, D, ps, hid = cfg.embed_dim, cfg.neck, cfg.patch, cfg.embed_dim * cfg.mlp_ratio
    sh, e = {}, "image_encoder."
    sh[e + "pos_embed"] = (1, PRETRAIN_GRID * PRETRAIN_GRID + 1, C)
    sh[e + "patch_embed.proj.weight"], sh[e + "patch_embed.proj.bias"] = (C, 3, ps, ps), (C,)
    for i in range(cfg.depth):
        q = f"{e}blocks.{i}."
        sh.update({q + "norm1.weight": (C,), q + "norm1.bias": (C,), q + "attn.qkv.weight": (3 * C, C), q + "attn.qkv.bias": (3 * C,),
                   q + "attn.proj.weight": (C, C), q + "attn.proj.bias": (C,), q + "norm2.weight": (C,), q + "norm2.bias": (C,),
                   q + "mlp.fc1.weight": (hid, C), q + "mlp.fc1.bias": (hid,), q + "mlp.fc2.weight": (C, hid), q + "mlp.fc2.bias": (C,)})
    sh[e + "neck.0.weight"] = (D, C, 1, 1)
    _norm_shapes(sh, e + "neck.1", D)
    sh[e + "neck.2.weight"] = (D, D, 3, 3)
    _norm_shapes(sh, e + "neck.3", D)
    p = "prompt_encoder."
    sh[p + "pe_layer.positional_encoding_gaussian_matrix"] = (2, D // 2)
    for n in ("invalid_points", "point_embeddings", "bbox_top_left_embeddings", "bbox_bottom_right_embeddings"):
        sh[p + n + ".weight"] = (1, D)
    m, t = "mask_decoder.", "mask_decoder.transformer."
    for i in range(cfg.dec_depth):
        q = f"{t}layers.{i}."
        _attn_shapes(sh, q + "self_attn.", D, D)
        _norm_shapes(sh, q + "norm1", D)
        _attn_shapes(sh, q + "cross_attn_token_to_image.", D, D // cfg.attn_down)
        _norm_shapes(sh, q + "norm2", D)
        _mlp_shapes(sh, q + "mlp.", (D, cfg.dec_mlp, D))
        _norm_shapes(sh, q + "norm3", D)
        _norm_shapes(sh, q + "norm4", D)
        _attn_shapes(sh, q + "cross_attn_image_to_token.", D, D // cfg.attn_down)
    _attn_shapes(sh, t + "final_attn_token_to_image.", D, D // cfg.attn_down)
    _norm_shapes(sh, t + "norm_final_attn", D)
    sh[m + "iou_token.weight"], sh[m + "mask_tokens.weight"] = (1, D), (cfg.num_masks + 1, D)
    u0, u1 = cfg.up_dims
    u = m + "final_output_upscaling_layers."
    sh[u + "0.0.weight"], sh[u + "0.0.bias"] = (D, u0, 2, 2), (u0,)
    _norm_shapes(sh, u + "0.1", u0)
    sh[u + "1.0.weight"], sh[u + "1.0.bias"] = (u0, u1, 2, 2), (u1,)
    for i in range(cfg.num_masks + 1):
        _mlp_shapes(sh, m + f"output_hypernetworks_mlps.{i}.", (D, D, D, u1))
    _mlp_shapes(sh, m + "iou_prediction_head.", (D, cfg.iou_hidden, cfg.iou_hidden, cfg.num_masks + 1))
    return sh


def synthetic_state(cfg, seed=0):
    """seeded random weights of a plausible scale under the checkpoint's key names, for tests, tools and benchmarks (no checkpoint exists offline); the
    random-Fourier matrix keeps the unit scale the reference draws it with"""
    st = encoder.draw_state(sam_shapes(cfg), seed, fan_in_first=("upscaling_layers.0.0.weight", "upscaling_layers.1.0.weight"))
    g = "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"
    st[g] = st[g] * math.sqrt(cfg.neck // 2)
    return st


def check_state(cfg, state):
    """the checkpoint's ["model"] dict or the dict itself -> that dict, after a strict comparison with sam_shapes: a missing, unexpected or misshapen entry is
    refused by name"""
    if isinstance(state.get("model"), dict):
        state = state["model"]
    shapes = sam_shapes(cfg)
    missing = [k for k in shapes if k not in state]
    extra = [k for k in state if k not in shapes]
    if missing or extra:
        raise KeyError(f"EfficientSAM {cfg.name} state: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                       f"unexpected {extra[:4]}{'...' if len(extra) > 4 else ''}")
    for k, shp in shapes.items():
        if tuple(state[k].shape) != tuple(shp):
            raise ValueError(f"EfficientSAM {cfg.name} state: {k} has shape {tuple(state[k].shape)}, expected {tuple(shp)}")
    return state


def abs_pos(pos_embed, grid):
    """pos_embed fp32 [1, 1 + 14 * 14, C] -> [grid * grid, C]: the class position dropped, bicubic interpolation (align_corners=False) where the grid differs"""
    pos = pos_embed[:, 1:]
    C = pos.shape[-1]
    if grid != PRETRAIN_GRID:
        pos = F.interpolate(pos.reshape(1, PRETRAIN_GRID, PRETRAIN_GRID, C).permute(0, 3, 1, 2), size=(grid, grid), mode="bicubic", align_corners=False)
        pos = pos.permute(0, 2, 3, 1)
    return pos.reshape(grid * grid, C)


def fourier_features(coords01, gauss):
    """points in the unit square [..., 2] (x, y) and the fp32 matrix [2, D / 2] -> [..., D] = sin | cos of 2 pi (2 c - 1) G, evaluated in fp32 on the host as the
    reference evaluates it (its matrix stays a float32 buffer whatever the model's type).  The reference computes `coords @ G` with the CPU library's matmul, whose
    rounding of this two-term product is a property of the host, not of the reference: here it is spelled out as fl(cx gx), then cy gy added to it with one rounding --
    what that matmul gave on the host where the golden was recorded.  The reference itself, run on another host, may differ from these values in the last bit of the
    angle, about 1e-7 on the outputs (seen: 7e-8 on an IoU prediction); fixing one order keeps the device model and the tests' restatement on the same values everywhere"""
    c, g = 2 * coords01.to(torch.float32) - 1, gauss.to(torch.float32)
    first = (c[..., 0:1].double() * g[0].double()).float()
    c = 2 * np.pi * (first.double() + c[..., 1:2].double() * g[1].double()).float()
    return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)


def dense_pe(gauss, grid):
    """the positional encoding of the grid's cell centres [grid * grid, D] (row-major), fp32 on the host"""
    one = torch.ones(grid, grid, dtype=torch.float32)
    y, x = (one.cumsum(0) - 0.5) / grid, (one.cumsum(1) - 0.5) / grid
    return fourier_features(torch.stack([x, y], dim=-1), gauss).reshape(grid * grid, -1)


def prepare_prompts(cfg, points, labels, input_hw):
    """points [B, Q, P, 2] (x, y in input pixels; negative = absent), labels [B, Q, P] -> ([B Q, 6, 2] rescaled to the network's side, negative coordinates -1;
    [B Q, 6] labels), P padded with -1 or cut to max_points"""
    pts = torch.as_tensor(np.asarray(points), dtype=torch.float32).clone()
    lab = torch.as_tensor(np.asarray(labels)).to(torch.int64).clone()
    assert pts.ndim == 4 and pts.shape[-1] == 2 and lab.shape == pts.shape[:3], "points [B, Q, P, 2], labels [B, Q, P]"
    H, W = input_hw
    neg = torch.full((), -1.0)
    pts = torch.stack([torch.where(pts[..., 0] >= 0, pts[..., 0] * cfg.img_size / W, neg), torch.where(pts[..., 1] >= 0, pts[..., 1] * cfg.img_size / H, neg)], dim=-1)
    P, n = pts.shape[2], cfg.max_points
    if P > n:
        pts, lab = pts[:, :, :n], lab[:, :, :n]
    elif P < n:
        pts, lab = F.pad(pts, (0, 0, 0, n - P), value=-1.0), F.pad(lab, (0, n - P), value=-1)
    return pts.reshape(-1, n, 2), lab.reshape(-1, n)


def build_point_grid(n_per_side):
    """segment_anything/utils/amg.py build_point_grid: the n x n cell centres of the unit square, float64 [n n, 2] (x, y), x fastest"""
    offset = 1 / (2 * n_per_side)
    side = np.linspace(offset, 1 - offset, n_per_side)
    return np.stack([np.tile(side[None, :], (n_per_side, 1)), np.tile(side[:, None], (1, n_per_side))], axis=-1).reshape(-1, 2)


def box_xyxy_to_xywh(box):
    """amg.py box_xyxy_to_xywh on one box of four numbers: (x1, y1, x2 - x1, y2 - y1) -- with the inclusive extents of a mask the width of a w-pixel box is w - 1"""
    out = np.array(box, copy=True)
    out[2], out[3] = out[2] - out[0], out[3] - out[1]
    return out


_ATTN = ("q_proj", "k_proj", "v_proj", "out_proj")


class HipEfficientSam:
    def __init__(self, cfg, state, dtype=torch.float32, x3=False, device="cuda:0"):
        """cfg: sam_config(...); state: the checkpoint's ["model"] dict or the dict itself (keys checked strictly); dtype / x3: the ENCODER's mode (float32 = exact
        fp32, float32 with x3 = split-bf16, bfloat16 = fast); the decoder always runs exact fp32"""
        encoder.check_mode(dtype, x3)
        state = check_state(cfg, state)
        self.cfg, self.dtype, self.x3, self.device = cfg, dtype, bool(x3), torch.device(device)
        self.grid = cfg.img_size // cfg.patch
        host = {k: v.detach().to(torch.float32).cpu() for k, v in state.items()}
        st = {k: v.to(self.device) for k, v in host.items()}
        self._pack_encoder(st, host)
        self._pack_decoder(st, host)

    # ------------------------------------------------------------------------------------------------------------
    # image encoder
    # ------------------------------------------------------------------------------------------------------------
    def _pack_encoder(self, st, host):
        cfg, e = self.cfg, "image_encoder."
        C, D = cfg.embed_dim, cfg.neck
        self.kpe = 3 * cfg.patch * cfg.patch
        assert C % cfg.num_heads == 0 and C % 8 == 0 and self.kpe % 32 == 0, "channel counts must be whole chunks"
        self.pe = (ops.pack_linear(st[e + "patch_embed.proj.weight"].reshape(C, self.kpe).contiguous(), self.dtype, x3=self.x3), st[e + "patch_embed.proj.bias"].contiguous())
        # the GEMM's residual: activation type (split-bf16: fp32)
        self.pos = abs_pos(host[e + "pos_embed"], self.grid).to(self.device, self.dtype).contiguous()
        self.blocks = []
        for i in range(cfg.depth):
            q = f"{e}blocks.{i}."
            wb = lambda n: (st[q + n + ".weight"], st[q + n + ".bias"])
            wqkv, bqkv = wb("attn.qkv")                       # q | k in one GEMM, V^T from its own (transposed-output) GEMM
            self.blocks.append(encoder.pack_block(wb("norm1"), wb("norm2"), (wqkv[:2 * C], bqkv[:2 * C]), (wqkv[2 * C:], bqkv[2 * C:]), wb("attn.proj"),
                                                  wb("mlp.fc1"), wb("mlp.fc2"), self.dtype, self.x3))
        self.neck0 = ops.pack_linear(st[e + "neck.0.weight"].reshape(D, C).contiguous(), self.dtype, x3=self.x3)
        self.neck1 = (st[e + "neck.1.weight"].contiguous(), st[e + "neck.1.bias"].contiguous())
        self.neck2 = ops.pack_conv3x3(st[e + "neck.2.weight"], self.dtype, x3=self.x3)
        self.neck3 = (st[e + "neck.3.weight"].contiguous(), st[e + "neck.3.bias"].contiguous())

    @torch.no_grad()
    def encode(self, images_u8):
        """uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device; [H, W, 3] = one image) -> the image embedding fp32 [B, grid * grid, neck]"""
        cfg = self.cfg
        img = torch.as_tensor(images_u8)
        img, _ = encoder.u8_batch(img[None] if img.ndim == 3 else img, None, self.device)
        B, g, C, D = img.shape[0], self.grid, cfg.embed_dim, cfg.neck
        a = ops.sam_patch_rows(img, cfg.img_size, cfg.patch, self.kpe, self.dtype, PIXEL_MEAN, PIXEL_STD, pair=self.x3)
        res = self.pos.unsqueeze(0).expand(B, -1, -1).reshape(B * g * g, C).contiguous()
        t = ops.linear(a, *self.pe, K=self.kpe, residual=res).view(B, g * g, C)
        vt = encoder.vt_buffer(t)
        for b in self.blocks:
            t = encoder.run_block(b, t, vt, heads=cfg.num_heads, eps=cfg.ln_eps, act="gelu", hidden=C * cfg.mlp_ratio, x3=self.x3)
        t = ops.layernorm(ops.linear(t, self.neck0, None, K=C), *self.neck1, eps=cfg.ln_eps)
        t = ops.layernorm(ops.conv3x3(t, self.neck2, None, B, g, g, D), *self.neck3, eps=cfg.ln_eps)
        return t if t.dtype == torch.float32 else ops.cast(t, torch.float32)

    # ------------------------------------------------------------------------------------------------------------
    # prompt encoder and mask decoder (exact fp32)
    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _lin(w, b):
        return ops.pack_linear(w.contiguous(), torch.float32), b.contiguous()

    def _pack_attn(self, st, p, self_attn=False):
        """q, k, v, o packed; self attention: q | k rows of one GEMM (both read the same tokens)"""
        a = SimpleNamespace(**{n[0]: self._lin(st[p + n + ".weight"], st[p + n + ".bias"]) for n in _ATTN})
        if self_attn:
            a.qk = self._lin(torch.cat([st[p + "q_proj.weight"], st[p + "k_proj.weight"]], 0), torch.cat([st[p + "q_proj.bias"], st[p + "k_proj.bias"]], 0))
        a.inner = st[p + "q_proj.weight"].shape[0]
        return a

    def _pe_product(self, lin):
        """the fixed dense positional encoding through a projection, WITHOUT its bias: [grid * grid, inner], the residual of that projection's GEMM over the keys"""
        return ops.linear(self.key_pe, lin[0], None, K=self.cfg.neck)

    def _pack_decoder(self, st, host):
        cfg, p, m, t = self.cfg, "prompt_encoder.", "mask_decoder.", "mask_decoder.transformer."
        D = cfg.neck
        assert D % (cfg.dec_heads * cfg.attn_down) == 0 and (D // cfg.attn_down // cfg.dec_heads) % 4 == 0, "decoder head dims must be whole fp32 chunks"
        self.gauss = host[p + "pe_layer.positional_encoding_gaussian_matrix"]
        self.label_rows = {-1: host[p + "invalid_points.weight"], 1: host[p + "point_embeddings.weight"], 2: host[p + "bbox_top_left_embeddings.weight"],
                           3: host[p + "bbox_bottom_right_embeddings.weight"]}
        self.out_tokens = torch.cat([host[m + "iou_token.weight"], host[m + "mask_tokens.weight"]], 0)                # [1 + masks, D], host
        self.key_pe = dense_pe(self.gauss, self.grid).to(self.device).contiguous()
        norm = lambda k: (st[k + ".weight"].contiguous(), st[k + ".bias"].contiguous())
        self.layers = []
        for i in range(cfg.dec_depth):
            q = f"{t}layers.{i}."
            ly = SimpleNamespace(self_attn=self._pack_attn(st, q + "self_attn.", True), t2i=self._pack_attn(st, q + "cross_attn_token_to_image."),
                                 i2t=self._pack_attn(st, q + "cross_attn_image_to_token."), norm1=norm(q + "norm1"), norm2=norm(q + "norm2"), norm3=norm(q + "norm3"),
                                 norm4=norm(q + "norm4"), fc1=self._lin(st[q + "mlp.layers.0.0.weight"], st[q + "mlp.layers.0.0.bias"]),
                                 fc2=self._lin(st[q + "mlp.fc.weight"], st[q + "mlp.fc.bias"]))
            ly.t2i.pe, ly.i2t.pe = self._pe_product(ly.t2i.k), self._pe_product(ly.i2t.q)
            self.layers.append(ly)
        self.final = self._pack_attn(st, t + "final_attn_token_to_image.")
        self.final.pe = self._pe_product(self.final.k)
        self.norm_final = norm(t + "norm_final_attn")
        u = m + "final_output_upscaling_layers."
        self.up0, self.up1 = self._deconv(st, u + "0.0"), self._deconv(st, u + "1.0")
        self.up_norm = norm(u + "0.1")
        mlp = lambda q: [self._lin(st[q + n + ".weight"], st[q + n + ".bias"]) for n in ("layers.0.0", "layers.1.0", "fc")]
        self.hyper = [mlp(m + f"output_hypernetworks_mlps.{i}.") for i in range(cfg.num_masks + 1)]
        self.iou_head = mlp(m + "iou_prediction_head.")

    def _deconv(self, st, name):
        """ConvTranspose2d(kernel = stride = 2) as a GEMM with columns (dy, dx, co), as depth.py packs its own"""
        w, b = st[name + ".weight"], st[name + ".bias"]       # [in, out, 2, 2]
        cin, cout = w.shape[0], w.shape[1]
        return ops.pack_linear(w.permute(2, 3, 1, 0).reshape(4 * cout, cin).contiguous(), torch.float32), b.repeat(4).contiguous(), cin, cout

    @staticmethod
    def _shuffle(y, N, g, cout):
        """GEMM output [N, g * g, (dy, dx, co)] -> NHWC rows [N, (2 g)^2, co]"""
        return y.view(N, g, g, 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(N, 4 * g * g, cout).contiguous()

    def _tokens(self, pts, lab):
        """host: rescaled points [N, 6, 2], labels [N, 6] -> decoder tokens [N, 1 + masks + 6, D] on the device"""
        emb = fourier_features((pts + 0.5) / self.cfg.img_size, self.gauss)
        for k, row in self.label_rows.items():
            emb = emb + row[:, None, :] * (lab == k)[:, :, None]
        return torch.cat([self.out_tokens.unsqueeze(0).expand(pts.shape[0], -1, -1), emb], dim=1).contiguous().to(self.device)

    def _attend(self, a, q, k, vt, Sk, residual):
        """projected q [N, S, inner], k [N, Sk, inner] (views allowed), V^T [N, inner, ld] -> residual + out_proj(attention)"""
        heads = self.cfg.dec_heads
        o = ops.attention(q, k, vt, heads, (a.inner // heads) ** -0.5, None, Sk=Sk, C=a.inner)
        return ops.linear(o, *a.o, K=a.inner, residual=residual)

    def _image_side(self, a, lin, keys, N):
        """a projection of (keys + dense positional encoding): the GEMM over the keys with the precomputed product as its residual"""
        n = keys.shape[1]
        return ops.linear(keys, *lin, K=self.cfg.neck, residual=a.pe.unsqueeze(0).expand(N, -1, -1).reshape(N * n, a.inner).contiguous()).view(N, n, a.inner)

    def _token_to_image(self, a, queries, pe, keys, norm):
        N, T, D = queries.shape
        n = keys.shape[1]
        q = ops.linear(ops.add(queries, pe), *a.q, K=D)
        k = self._image_side(a, a.k, keys, N)
        vt = ops.linear(keys, *a.v, K=D, rows_per_batch=n, transposed_ld=encoder.ceil8(n))
        return ops.layernorm(self._attend(a, q, k, vt, n, queries), *norm)

    def _decode(self, embedding, tokens):
        """embedding fp32 [N, n, D] (tiled per query), tokens [N, T, D] -> (low-res logits [N, masks, 4 g, 4 g], IoU predictions [N, masks])"""
        cfg, g = self.cfg, self.grid
        N, T, D = tokens.shape
        n, T8 = g * g, encoder.ceil8(T)
        queries, keys, pe = tokens, embedding, tokens
        for i, ly in enumerate(self.layers):
            if i > 0:
                queries = ops.add(queries, pe)
            a = ly.self_attn
            qk = ops.linear(queries, *a.qk, K=D)
            vt = ops.linear(queries, *a.v, K=D, rows_per_batch=T, transposed_ld=T8)
            queries = ops.layernorm(self._attend(a, qk, qk[..., D:], vt, T, queries), *ly.norm1)
            queries = self._token_to_image(ly.t2i, queries, pe, keys, ly.norm2)
            h = ops.linear(queries, *ly.fc1, K=D, gelu=True)
            queries = ops.layernorm(ops.linear(h, *ly.fc2, K=cfg.dec_mlp, residual=queries), *ly.norm3)
            a = ly.i2t                                        # the image's positions attend to the tokens
            q = self._image_side(a, a.q, keys, N)
            k = ops.linear(ops.add(queries, pe), *a.k, K=D)
            vt = ops.linear(queries, *a.v, K=D, rows_per_batch=T, transposed_ld=T8)
            keys = ops.layernorm(self._attend(a, q, k, vt, T, keys), *ly.norm4)
        queries = self._token_to_image(self.final, queries, pe, keys, self.norm_final)
        nm = cfg.num_masks + 1
        u0, u1 = cfg.up_dims
        x = self._shuffle(ops.linear(keys, self.up0[0], self.up0[1], K=D), N, g, u0)
        x = ops.gelu(ops.groupnorm(x, *self.up_norm, 1, 1e-5))
        x = self._shuffle(ops.linear(x, self.up1[0], self.up1[1], K=u0, gelu=True), N, 2 * g, u1)
        hyper = torch.empty(N, nm * u1, dtype=torch.float32, device=self.device)
        for i, (l0, l1, fc) in enumerate(self.hyper):
            h = ops.linear(ops.linear(queries[:, 1 + i].contiguous(), *l0, K=D, gelu=True), *l1, K=D, gelu=True)
            ops.linear(h, *fc, K=D, out=hyper[:, i * u1:(i + 1) * u1])
        masks = ops.hyper_masks(x, hyper.view(N, nm, u1)).view(N, nm, 4 * g, 4 * g)
        l0, l1, fc = self.iou_head
        h = ops.linear(ops.linear(queries[:, 0].contiguous(), *l0, K=D, gelu=True), *l1, K=cfg.iou_hidden, gelu=True)
        iou = ops.linear(h, *fc, K=cfg.iou_hidden)
        return masks[:, 1:], iou[:, 1:]                      # multimask output: the first mask token is the single-mask one

    @torch.no_grad()
    def decode_low(self, embedding, points, labels, input_hw):
        """predict up to the network's own outputs: embedding, points [B, Q, P, 2], labels [B, Q, P] and input_hw as predict takes them -> (low-res logits fp32
        [B, Q, 3, 4 g, 4 g], predicted IoU [B, Q, 3]) in the network's output order (NOT sorted).  A query's rows do not depend on the queries beside it."""
        cfg = self.cfg
        pts, lab = prepare_prompts(cfg, points, labels, input_hw)
        B, Q = np.asarray(labels).shape[:2]
        assert embedding.shape[0] == B and embedding.dtype == torch.float32
        nm = cfg.num_masks
        with ops.batch_invariant():                          # a query's masks do not depend on the queries beside it
            emb = embedding if Q == 1 else embedding[:, None].expand(-1, Q, -1, -1).reshape(B * Q, *embedding.shape[1:])
            low, iou = self._decode(emb.contiguous(), self._tokens(pts, lab))
        return low.contiguous().view(B, Q, nm, *low.shape[2:]), iou.reshape(B, Q, nm)

    @torch.no_grad()
    def predict(self, embedding, points, labels, input_hw, output_hw=None, details=False):
        """embedding: encode()'s [B, n, D]; points [B, Q, P, 2] (x, y in pixels of the input_hw = (H, W) image; negative = absent), labels [B, Q, P] (1 point,
        2 box top-left, 3 box bottom-right, -1 absent) -> (mask logits fp32 [B, Q, 3, H', W'] at output_hw (default input_hw) sorted by predicted IoU descending,
        predicted IoU [B, Q, 3]); details: also (low-res logits [B, Q, 3, 4 g, 4 g], uint8 masks [B, Q, 3, H', W'] = 255 (logit >= 0)), sorted the same way, and
        the order itself [B, Q, 3] (indices into the network's three outputs)"""
        low, iou = self.decode_low(embedding, points, labels, input_hw)
        B, Q, nm = iou.shape
        Ho, Wo = output_hw if output_hw is not None else input_hw
        with ops.batch_invariant():
            full, m8 = ops.upsample_bicubic(low.view(B * Q * nm, *low.shape[3:]), Ho, Wo, mask=True)
        order = torch.argsort(iou, dim=-1, descending=True)
        pick = lambda t: torch.take_along_dim(t.view(B, Q, nm, *t.shape[-2:]), order[..., None, None], dim=2)
        out = (pick(full), torch.take_along_dim(iou, order, dim=2))
        return out + (pick(low), pick(m8), order) if details else out

    @torch.no_grad()
    def segment(self, image_u8, points, labels):
        """uint8 [H, W, 3] image, points [P, 2] (x, y), labels [P] -> uint8 [H, W] (numpy): 255 where the best mask's logit is >= 0"""
        img = np.asarray(image_u8)
        assert img.ndim == 3 and img.shape[-1] == 3
        pts, lab = np.asarray(points, dtype=np.float32).reshape(1, 1, -1, 2), np.asarray(labels).reshape(1, 1, -1)
        m8 = self.predict(self.encode(img), pts, lab, img.shape[:2], details=True)[3]
        return m8[0, 0, 0].cpu().numpy()

    @torch.no_grad()
    def generate(self, image_u8, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88, stability_score_thresh=0.95, stability_score_offset=1.0,
                 box_nms_thresh=0.7, point_grid=None):
        """uint8 [H, W, 3] image -> the masks of everything in it: the single-crop path of SamAutomaticMaskGenerator (crop_n_layers = 0, min_mask_region_area = 0;
        segment_anything/automatic_mask_generator.py: generate, _process_crop, _process_batch), in its order:
          1. encode once;
          2. points = build_point_grid(points_per_side) * (W, H), or point_grid [n, 2] in the unit square in its place;
          3. per batch of points_per_batch points, each one foreground click (label 1) of a query of its own: decode_low; the candidates point-major, then the
             network's three outputs; keep predicted IoU > pred_iou_thresh; ops.upsample_bicubic_stats of the survivors at the image's size; stability =
             n_hi / n_lo, the fp32 quotient of the two counts (0 / 0 = NaN fails); keep stability >= stability_score_thresh; boxes from the statistics.  As in
             the reference a threshold <= 0 switches its filter off;
          4. the survivors' low-res logits stay on the device;
          5. ops.box_nms of all survivors by predicted IoU at box_nms_thresh;
          6. the byte masks of the kept ones: ops.upsample_bicubic_stats(mask=True), in chunks.
        -> records in NMS order (best predicted IoU first), each a dict: segmentation uint8 [H, W] 0 / 255 (the project's mask form: SAM returns bool), area (int),
        bbox [x, y, w, h] (box_xyxy_to_xywh of the inclusive extents: w = x_max - x_min), predicted_iou, point_coords [[x, y]], stability_score.
        Where this differs from SAM: a pixel belongs to a mask where its logit is >= 0 (predict's rule, src/demo/utils.py:94 of the reference), SAM's generator takes
        > 0; area and bbox follow the bytes returned.  The filter of boxes near a crop's edge (_process_batch) is the empty filter for a single crop -- a box edge
        near the crop's edge is near the image's edge -- and is not run.  The result does not depend on points_per_batch: decode_low is batch-invariant and every
        later step is per candidate or over all of them."""
        img = np.asarray(image_u8)
        assert img.ndim == 3 and img.shape[-1] == 3 and img.dtype == np.uint8
        H, W = img.shape[:2]
        grid = build_point_grid(points_per_side) if point_grid is None else np.asarray(point_grid, dtype=np.float64).reshape(-1, 2)
        points = grid * np.array([[W, H]], dtype=np.float64)
        emb = self.encode(img)
        nm, step = self.cfg.num_masks, int(points_per_batch)
        assert 1 <= step * nm <= 65535
        lows, ious, stabs, boxes, areas, coords = [], [], [], [], [], []
        for at in range(0, len(points), step):
            p = points[at:at + step]
            low, iou = self.decode_low(emb, p[None, :, None, :], np.ones((1, len(p), 1), dtype=np.int64), (H, W))
            low, iou_h, cand = low.view(len(p) * nm, *low.shape[3:]), iou.reshape(-1).cpu().numpy(), np.repeat(p, nm, axis=0)
            keep = np.flatnonzero(iou_h > np.float32(pred_iou_thresh)) if pred_iou_thresh > 0.0 else np.arange(len(iou_h))
            if len(keep) == 0:
                continue
            low = low[torch.as_tensor(keep, device=low.device)].contiguous()
            st = ops.upsample_bicubic_stats(low, H, W, stability_score_offset).cpu().numpy()
            with np.errstate(divide="ignore", invalid="ignore"):
                stab = st[:, 1].astype(np.float32) / st[:, 2].astype(np.float32)
            stable = np.flatnonzero(stab >= np.float32(stability_score_thresh)) if stability_score_thresh > 0.0 else np.arange(len(stab))
            if len(stable) == 0:
                continue
            lows.append(low[torch.as_tensor(stable, device=low.device)])
            keep = keep[stable]
            ious.append(iou_h[keep]), stabs.append(stab[stable]), boxes.append(st[stable, 3:7]), areas.append(st[stable, 0]), coords.append(cand[keep])
        if not lows:
            return []
        lows, ious, stabs, boxes, areas, coords = torch.cat(lows), np.concatenate(ious), np.concatenate(stabs), np.concatenate(boxes), np.concatenate(areas), np.concatenate(coords)
        dev = lows.device
        kept = ops.box_nms(torch.from_numpy(boxes.astype(np.float32)).to(dev), torch.from_numpy(ious).to(dev), box_nms_thresh)
        lows, kept = lows[kept].contiguous(), kept.cpu().numpy()
        chunk = min(max(1, (64 << 20) // (H * W)), 65535)     # byte masks of at most 64 MiB per launch
        masks = np.concatenate([ops.upsample_bicubic_stats(lows[c:c + chunk], H, W, stability_score_offset, mask=True)[1].cpu().numpy() for c in range(0, len(kept), chunk)])
        return [dict(segmentation=masks[r], area=int(areas[k]), bbox=box_xyxy_to_xywh(boxes[k]).tolist(), predicted_iou=float(ious[k]), point_coords=[coords[k].tolist()],
                     stability_score=float(stabs[k])) for r, k in enumerate(kept)]
