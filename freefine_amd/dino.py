"""The DINOv2 ViT on the HIP kernels: the one encoder of the project (`HipDinoEncoder`), used by the depth network (freefine_amd/depth.py: HipDepthAnything,
the last four blocks' patch tokens) and by the feature extractor of the FID-DINO / Kernel Distance metrics (`HipDinoV2` below: the normalised class token;
/root/reference/evaluation/metrics/FID/fid_dino.py:35, fid_kd.py:34 torch.hub dinov2_vitb14, fid_score.py:93-143 get_activations;
torchhub/facebookresearch_dinov2_main/vision_transformer.py:178-257, 319-324).

Activations are token rows, every Linear and the patch embedding is an `ffn_igemm` call, LayerNorm and attention are the UNet's kernels (`ffn_layernorm`,
`ffn_attn` with head dim 64 and the ragged S = 1 + (H/14)(W/14)).  Folded at pack time: LayerScale into attn.proj / mlp.fc2 (rows scaled by gamma), the patch
embedding into a [C, 3*14*14] GEMM weight over im2col rows of the image.  The rows come either from a float image (torch view plumbing, `_im2col`) or, for the
metrics, straight from decoded uint8 images on the device: `features_u8` = ffn_resize_pil_bilinear_u8 (PIL's antialiased bilinear Resize, bit for bit) ->
ffn_vit_patch_rows (ToTensor + Normalize as a lookup, im2col) -> the same GEMM.  torchvision is absent here: the transform's semantics are torchvision's
documented ones (see ops.py), the resize is pinned to PIL itself.

`HipDino` is the same encoder as DINO v1's ViT-B/16, the extractor of Subject Consistency (evaluation/metrics/VBench/subject_consistency.py:10-35, torch.hub
dino_vitb16): patch 16, 224 x 224 positional grid, no LayerScale.  DINO v1's own source is on neither machine; what IS pinned is the reference's vendored
DinoVisionTransformer configured that way (patch_size=16, init_values=None, interpolate_offset=0.1; tests/golden/g15_dino16_cls.npz, tools/gen_golden.py
run_g15), and the claim that this equals dino_vitb16 rests on the two published sources, not on a recording.

dtype float32 = parity mode (exact-fp32 MFMA), float32 with x3=True = split-bf16 (below), bfloat16 = fast mode.  No graph capture, no class-token-only last block.

Split-bf16 (`HipDinoV2(..., x3=True)`, `HipDino` likewise; the depth network passes no x3 and stays as it is): every GEMM and the attention run FFN_BF16X3 --
operands as hi + lo bf16 pairs, three bf16 MFMAs per product term, fp32 accumulation -- in the blocks as encoder.py describes it (LayerScale is folded
BEFORE the split); the positional embedding and the class row stay fp32 like the residual stream.  The patch embedding's contraction length is
rounded up to a multiple of 32 (608 at patch 14) so that both operands are in the blocked pair form; `features_u8` gets its rows from
`ffn_vit_patch_rows_pair` (pair rows straight from the bytes), `forward` from fp32 rows that ops.linear splits -- the same operand bytes."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import encoder, ops

_ENC = dict(vits=(384, 12, 6), vitb=(768, 12, 12), vitl=(1024, 24, 16), tiny=(128, 4, 2), mini=(192, 5, 3))
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # fid_score.py:122-123


def dinov2_config(name="vitb"):
    """dinov2_vitb14 (hubconf.py: img_size 518, patch 14, LayerScale, mlp ffn, interpolate_offset 0.1) -- the metrics' model -- and the small test sizes
    "tiny" / "mini"; the same numbers as depth.depth_config"""
    enc = {k: _ENC[k] for k in ("vitb", "tiny", "mini")}[name]
    return SimpleNamespace(name=name, embed_dim=enc[0], depth=enc[1], num_heads=enc[2], patch=14, img_size=518, mlp_ratio=4, interpolate_offset=0.1, ln_eps=1e-6)


def dino_config(name="vitb16"):
    """DINO v1 ViT-B/16 as the vendored DinoVisionTransformer spells it -- patch 16, img_size 224 (a 14 x 14 positional grid), no LayerScale (init_values=None),
    interpolate_offset 0.1 -- and the small test size "tiny16" """
    enc = {"vitb16": _ENC["vitb"], "tiny16": _ENC["tiny"]}[name]
    return SimpleNamespace(name=name, embed_dim=enc[0], depth=enc[1], num_heads=enc[2], patch=16, img_size=224, mlp_ratio=4, interpolate_offset=0.1, ln_eps=1e-6,
                           layerscale=False)


def dinov2_param_shapes(cfg, prefix=""):
    """name -> shape of DinoVisionTransformer.state_dict() (hub layout; `prefix` = "pretrained." inside DPT_DINOv2)"""
    C, hid = cfg.embed_dim, cfg.embed_dim * cfg.mlp_ratio
    n = (cfg.img_size // cfg.patch) ** 2
    p = prefix
    sh = {p + "cls_token": (1, 1, C), p + "pos_embed": (1, n + 1, C), p + "mask_token": (1, C),
          p + "patch_embed.proj.weight": (C, 3, cfg.patch, cfg.patch), p + "patch_embed.proj.bias": (C,),
          p + "norm.weight": (C,), p + "norm.bias": (C,)}
    ls = getattr(cfg, "layerscale", True)                      # dino_config: no ls*.gamma
    for i in range(cfg.depth):
        q = f"{p}blocks.{i}."
        sh.update({q + "norm1.weight": (C,), q + "norm1.bias": (C,), q + "attn.qkv.weight": (3 * C, C), q + "attn.qkv.bias": (3 * C,),
                   q + "attn.proj.weight": (C, C), q + "attn.proj.bias": (C,), q + "ls1.gamma": (C,),
                   q + "norm2.weight": (C,), q + "norm2.bias": (C,), q + "mlp.fc1.weight": (hid, C), q + "mlp.fc1.bias": (hid,),
                   q + "mlp.fc2.weight": (C, hid), q + "mlp.fc2.bias": (C,), q + "ls2.gamma": (C,)})
        if not ls:
            del sh[q + "ls1.gamma"], sh[q + "ls2.gamma"]
    return sh


param_shapes = dinov2_param_shapes


def synthetic_state(cfg, seed=0):
    """seeded random weights of a plausible scale in hub layout, for benchmarks without a checkpoint (`tools/bench_dino.py`; there is no network)"""
    return encoder.draw_state(dinov2_param_shapes(cfg), seed)


class HipDinoEncoder:
    """The DINOv2 ViT encoder: weights packed from `<prefix>*` of a state dict, tokens, blocks.  Subclasses add what they read off the tokens."""

    def _init_encoder(self, cfg, dtype, device, x3=False):
        encoder.check_mode(dtype, x3)
        self.cfg, self.dtype, self.device, self.x3 = cfg, dtype, torch.device(device), bool(x3)
        C = cfg.embed_dim
        assert C % cfg.num_heads == 0 and C % 8 == 0, "channel counts must be whole 16-byte chunks"
        self._pos = {}

    def _pack_encoder(self, st, p):
        """st: fp32 tensors on the device; p: the prefix of the ViT's parameters (`pretrained.` inside DPT_DINOv2, empty in hub layout)"""
        cfg = self.cfg
        C = cfg.embed_dim
        e = 32 if self.x3 else 8                              # split-bf16: whole 32-column blocks, so that both operands are in the blocked pair form
        K = 3 * cfg.patch * cfg.patch
        self.kpe = (K + e - 1) // e * e                        # patch-embedding contraction length, padded to whole chunks (patch 14: 592; split-bf16: 608)
        wpe = torch.zeros(C, self.kpe, device=self.device)
        wpe[:, :K] = st[p + "patch_embed.proj.weight"].reshape(C, K)
        self.pe = (ops.pack_linear(wpe, self.dtype, x3=self.x3), st[p + "patch_embed.proj.bias"].contiguous())
        self.pos_embed, self.cls_token = st[p + "pos_embed"], st[p + "cls_token"]
        self.blocks = []
        for i in range(cfg.depth):
            q = f"{p}blocks.{i}."

            def wb(n, gamma=None):                            # LayerScale folded: gamma * (W x + b); no ls*.gamma: no LayerScale
                w, b = st[q + n + ".weight"], st[q + n + ".bias"]
                return (w, b) if gamma is None else (w * gamma[:, None], b * gamma)
            wqkv, bqkv = wb("attn.qkv")                       # q | k in one GEMM, V^T from its own (transposed-output) GEMM
            self.blocks.append(encoder.pack_block(wb("norm1"), wb("norm2"), (wqkv[:2 * C], bqkv[:2 * C]), (wqkv[2 * C:], bqkv[2 * C:]),
                                                  wb("attn.proj", st.get(q + "ls1.gamma")), wb("mlp.fc1"), wb("mlp.fc2", st.get(q + "ls2.gamma")),
                                                  self.dtype, self.x3))
        self.norm = (st[p + "norm.weight"].contiguous(), st[p + "norm.bias"].contiguous())

    # ------------------------------------------------------------------------------------------------------------
    # tokens and blocks
    # ------------------------------------------------------------------------------------------------------------
    def _pos_tokens(self, H, W):
        """(class row = cls_token + pos[0] [1, C], positional embedding of the H/14 x W/14 patches [N, C]) in the activation dtype --
        vision_transformer.py:178-209 (bicubic, antialias off, offset 0.1; evaluated once per input size)"""
        key = (H, W)
        hit = self._pos.get(key)
        if hit is not None:
            return hit
        cfg = self.cfg
        pe = self.pos_embed.float()
        N = pe.shape[1] - 1
        npatch = (H // cfg.patch) * (W // cfg.patch)
        patch_pos = pe[:, 1:]
        if not (npatch == N and H == W):
            dim = pe.shape[-1]
            w0, h0 = H // cfg.patch + cfg.interpolate_offset, W // cfg.patch + cfg.interpolate_offset
            sq = math.sqrt(N)
            patch_pos = F.interpolate(patch_pos.reshape(1, int(sq), int(sq), dim).permute(0, 3, 1, 2), scale_factor=(float(w0) / sq, float(h0) / sq),
                                      mode="bicubic", antialias=False)
            assert int(w0) == patch_pos.shape[-2] and int(h0) == patch_pos.shape[-1]
            patch_pos = patch_pos.permute(0, 2, 3, 1).reshape(1, -1, dim)
        cls_row = (self.cls_token.float()[0] + pe[:, 0]).to(self.dtype).contiguous()
        hit = self._pos[key] = (cls_row, patch_pos[0].to(self.dtype).contiguous())
        return hit

    _im2col = staticmethod(encoder.im2col)

    def _patch_rows(self, x):
        """float image [B, 3, H, W] -> the patch-embedding GEMM's operand rows [B * ph * pw, kpe] in the activation dtype (columns >= 3 * 14 * 14 zero)"""
        B, _, H, W = x.shape
        ps = self.cfg.patch
        cols = self._im2col(x.to(self.device, torch.float32), ps)
        a = torch.zeros(B * (H // ps) * (W // ps), self.kpe, dtype=self.dtype, device=self.device)
        a[:, :cols.shape[1]] = cols.to(self.dtype)
        return a

    def _embed(self, a, B, H, W):
        """patch embedding of given operand rows + class row -> ([B, 1 + ph * pw, C], ph, pw).  Split-bf16: a = pair rows (ops.vit_patch_rows_pair) or fp32
        rows, which ops.linear splits."""
        cls_row, pos = self._pos_tokens(H, W)
        return encoder.embed_patches(a, self.pe[0], self.pe[1], self.kpe, pos, cls_row, B), H // self.cfg.patch, W // self.cfg.patch

    def _tokens(self, x):
        """patch rows from a float image, embedded"""
        B, _, H, W = x.shape
        return self._embed(self._patch_rows(x), B, H, W)

    def _run_blocks(self, t, keep_last=1):
        """all blocks over tokens [B, S, C] -> the outputs of the last `keep_last` blocks (before the final LayerNorm)"""
        cfg = self.cfg
        vt = encoder.vt_buffer(t)
        outs = []
        for i, b in enumerate(self.blocks):
            t = encoder.run_block(b, t, vt, heads=cfg.num_heads, eps=cfg.ln_eps, act="gelu", hidden=cfg.embed_dim * cfg.mlp_ratio, x3=self.x3)
            if i >= cfg.depth - keep_last:
                outs.append(t)
        return outs


class HipDinoV2(HipDinoEncoder):
    """DinoVisionTransformer.forward with the hub's identity head: the final LayerNorm's class token (vision_transformer.py:319-324, 236-257)."""

    def __init__(self, cfg, state, dtype=torch.float32, device="cuda:0", x3=False):
        """state: DinoVisionTransformer.state_dict() in hub layout (no `pretrained.` prefix; mask_token accepted and unused); x3: split-bf16 arithmetic (module
        docstring; needs dtype float32, ValueError otherwise)"""
        self._init_encoder(cfg, dtype, device, x3=x3)
        self._pack_encoder({k: v.detach().to(self.device, torch.float32) for k, v in state.items()}, "")
        self._lut = ops.vit_norm_table(IMAGENET_MEAN, IMAGENET_STD).to(self.device)

    def _cls_u8(self, small):
        """resized uint8 images [B, H, W, 3] -> patch rows -> tokens -> _cls"""
        B, H, W, _ = small.shape
        a = encoder.patch_rows_u8(small, self._lut, self.cfg.patch, self.kpe, self.dtype, self.x3)
        return self._cls(self._embed(a, B, H, W)[0])

    def _cls(self, t):
        """tokens -> blocks -> final LayerNorm on the class rows only (fp32 in split-bf16 mode too) -> fp32 [B, C]"""
        last = self._run_blocks(t, 1)[0]
        return ops.layernorm(last[:, 0].contiguous(), *self.norm, eps=self.cfg.ln_eps).float()

    @torch.no_grad()
    def forward(self, x):
        """x float [B, 3, H, W] (normalised image, H and W multiples of 14) -> fp32 [B, C]: the reference's model(batch) = head(x_norm_clstoken), head = identity"""
        assert x.shape[2] % self.cfg.patch == 0 and x.shape[3] % self.cfg.patch == 0, f"patch embedding: image sides must be multiples of {self.cfg.patch}"
        return self._cls(self._tokens(x)[0])

    __call__ = forward

    @torch.no_grad()
    def features_u8(self, images, size=224):
        """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device) -> fp32 [B, C]: the transform of fid_score.py:124 -- Resize((size, size)) of the
        PIL image, ToTensor, Normalize(imagenet) -- and the network, all on the device: resize -> patch rows -> encoder."""
        img, _ = encoder.u8_batch(images, None, self.device)
        assert size % self.cfg.patch == 0
        return self._cls_u8(ops.resize_pil_bilinear_u8(img, size, size))


class HipDino(HipDinoV2):
    """DINO ViT-B/16 (module docstring): the same class-token extractor at patch 16 without LayerScale; `forward` is HipDinoV2's.  `features_u8` is the transform
    of subject_consistency.py:11-15 on the device -- image * keep mask, Resize(224) (short side to 224, PIL BILINEAR, NO crop: a non-square image stays
    non-square), ToTensor, Normalize(imagenet) -- with the window that floors both sides to multiples of 16: the patch embedding of DINO v1 is a strided
    convolution, which drops a trailing partial patch."""

    @torch.no_grad()
    def features_u8(self, images, keep=None, size=224):
        """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device); keep = None or (rule, m1, m2) as in ops.resize_pil_u8 (uint8 [B, H, W], host or
        device) -> fp32 [B, C]"""
        img, keep = encoder.u8_batch(images, keep, self.device)
        ps = self.cfg.patch
        oh, ow = ops.torchvision_resize_size(img.shape[1], img.shape[2], size)
        H, W = oh // ps * ps, ow // ps * ps
        return self._cls_u8(ops.resize_pil_u8(img, oh, ow, "bilinear", crop=(0, 0, H, W), keep=keep))
