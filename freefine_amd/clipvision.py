"""The CLIP image tower on the HIP kernels: the feature extractor of Background Consistency (the reference's evaluation/metrics/VBench/background_consistency.py:
18-41, `clip.load('ViT-B/32')` -> `clip_model.encode_image`).  The `clip` package is absent here; `transformers.CLIPVisionModelWithProjection(...).image_embeds` is
the same arithmetic and is what the tower is pinned to (tests/test_consistency_cpu.py restates it in fp64, tests/test_consistency_gpu.py holds the device to it).

    rows = im2col(image)  [B 49, 3 32 32];  t = rows W_patch^T + pos[1:]  (no bias; the positional embedding is the GEMM's residual);  x = [class + pos[0] | t]
    x = pre_layrnorm(x)  (transformers' spelling);  per layer: y = LN1(x); q, k, v = Linear(y); a = softmax(q k^T / 8) v per head; x += out_proj(a);
    y = LN2(x); x += fc2(quick_gelu(fc1(y)));  result post_layernorm(x[:, 0]) W_proj^T  -> [B, projection_dim]

built like text.HipCLIPTextEncoder and dino.HipDinoEncoder: every Linear an `ffn_igemm` (q | k in one GEMM, V^T from the transposed-output GEMM, residuals and
quick-gelu in the epilogues), `ffn_layernorm`, non-causal `ffn_attn` at S = 50 with head dim 64.  224 x 224 only: no positional interpolation.

`features_u8` is CLIP's transform on the device, from decoded uint8 images: image * keep mask, Resize(224, BICUBIC) (short side to 224), CenterCrop(224) -- one
ffn_resize_pil_u8 with a crop window, PIL's bicubic bit for bit -- then ToTensor + Normalize(CLIP's mean / std) and the im2col as ffn_vit_patch_rows.

dtype float32 = parity mode (exact-fp32 MFMA), float32 with x3=True = split-bf16, bfloat16 = fast mode.

Split-bf16 (`HipCLIPVision(..., x3=True)`): every GEMM (the 768 -> 512 projection included) and the attention run FFN_BF16X3 -- operands as hi + lo bf16 pairs,
three bf16 MFMAs per product term, fp32 accumulation -- built like text.HipCLIPTextEncoder: weights packed with ops.pack_linear(x3=True), layer_norm1 / 2 and
post_layernorm write the pair rows their GEMMs read (`ffn_layernorm_pair`), attention and fc1 write pair rows for the GEMM behind them; the residual stream
(pre_layrnorm writes it: fp32), the positional embedding, the class row and V^T stay fp32.  `features_u8` gets the patch GEMM's rows from
`ffn_vit_patch_rows_pair` (pair rows straight from the bytes), `forward` from fp32 rows that ops.linear splits -- the same operand bytes."""
from types import SimpleNamespace

import torch

from . import ops

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)      # clip/clip.py _transform

_VISION = dict(vitb32=dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, projection_dim=512),
               tiny=dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, projection_dim=64))
_VISION_FIELDS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "projection_dim", "image_size", "patch_size", "hidden_act",
                  "layer_norm_eps")
_VISION_DEFAULTS = dict(image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=512)      # transformers' CLIPVisionConfig defaults


def clip_vision_config(config="vitb32"):
    """"vitb32" (CLIP ViT-B/32: width 768, 12 layers, 12 heads, MLP 3072, projection 512) / "tiny" (the test size), a CLIPVisionConfig, or a dict of its fields
    -> the fields the tower needs, checked.  Raises ValueError with the reason otherwise."""
    if isinstance(config, SimpleNamespace):
        return config
    if isinstance(config, str):
        if config not in _VISION:
            raise ValueError(f"CLIP vision config {config!r} (one of {sorted(_VISION)})")
        config = _VISION[config]
    get = (lambda k: config.get(k, _VISION_DEFAULTS.get(k))) if isinstance(config, dict) else (lambda k: getattr(config, k, _VISION_DEFAULTS.get(k)))
    cfg = SimpleNamespace(**{k: get(k) for k in _VISION_FIELDS})
    missing = [k for k in _VISION_FIELDS if getattr(cfg, k) is None]
    if missing:
        raise ValueError(f"CLIP vision config: missing {missing}")
    C, nh = cfg.hidden_size, cfg.num_attention_heads
    if C % nh != 0 or C // nh != 64:
        raise ValueError(f"CLIP vision tower: head dim {C / nh:g} (hidden_size {C} / {nh} heads); the tower runs the head-dim-64 attention kernels")
    if cfg.hidden_act != "quick_gelu":
        raise ValueError(f"CLIP vision tower: hidden_act {cfg.hidden_act!r}; CLIP's image tower uses 'quick_gelu'")
    if cfg.image_size % cfg.patch_size != 0 or cfg.intermediate_size % 8 != 0 or cfg.projection_dim % 8 != 0:
        raise ValueError(f"CLIP vision tower: image {cfg.image_size} / patch {cfg.patch_size}, MLP {cfg.intermediate_size}, projection {cfg.projection_dim}: "
                         "whole patches and multiples of 8 only")
    return cfg


def transformers_vision_config(cfg):
    """the CLIPVisionConfig of a checked configuration (tests and tools build the yardstick module from it)"""
    from transformers import CLIPVisionConfig
    return CLIPVisionConfig(**{k: getattr(cfg, k) for k in _VISION_FIELDS})


def vision_param_shapes(cfg, prefix=""):
    """name -> shape of CLIPVisionModelWithProjection.state_dict() (`prefix` = "vision_model." as the module spells it; visual_projection carries none)"""
    C, I, P, ps = cfg.hidden_size, cfg.intermediate_size, cfg.projection_dim, cfg.patch_size
    n = (cfg.image_size // ps) ** 2
    q = prefix
    sh = {q + "embeddings.class_embedding": (C,), q + "embeddings.patch_embedding.weight": (C, 3, ps, ps), q + "embeddings.position_embedding.weight": (n + 1, C),
          q + "pre_layrnorm.weight": (C,), q + "pre_layrnorm.bias": (C,)}
    for i in range(cfg.num_hidden_layers):
        p = f"{q}encoder.layers.{i}."
        for nm in ("k_proj", "v_proj", "q_proj", "out_proj"):
            sh[p + f"self_attn.{nm}.weight"], sh[p + f"self_attn.{nm}.bias"] = (C, C), (C,)
        sh[p + "layer_norm1.weight"], sh[p + "layer_norm1.bias"] = (C,), (C,)
        sh[p + "mlp.fc1.weight"], sh[p + "mlp.fc1.bias"], sh[p + "mlp.fc2.weight"], sh[p + "mlp.fc2.bias"] = (I, C), (I,), (C, I), (C,)
        sh[p + "layer_norm2.weight"], sh[p + "layer_norm2.bias"] = (C,), (C,)
    sh.update({q + "post_layernorm.weight": (C,), q + "post_layernorm.bias": (C,), "visual_projection.weight": (P, C)})
    return sh


def synthetic_state(cfg, seed=0):
    """seeded random weights of a plausible scale in transformers' layout (with the `vision_model.` prefix), drawn the way dino.synthetic_state draws them: for
    tests and benchmarks without a checkpoint (there is no network)"""
    import math
    g = torch.Generator().manual_seed(seed)
    st = {}
    for k, shp in vision_param_shapes(cfg, "vision_model.").items():
        if "norm" in k and k.endswith(".weight"):
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(".bias"):
            t = 0.05 * torch.randn(shp, generator=g)
        elif k.endswith("class_embedding") or k.endswith("position_embedding.weight"):
            t = 0.2 * torch.randn(shp, generator=g)
        else:
            t = torch.randn(shp, generator=g) / math.sqrt(math.prod(shp[1:]))
        st[k] = t.float()
    return st


def to_openai_layout(state, layers):
    """transformers' names -> the OpenAI checkpoint's `visual.*` names: the inverse of _openai_to_transformers, for tests of that mapping (it is the same
    published layout read the other way, no independent evidence)"""
    st = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in state.items()}
    out = {"visual.class_embedding": st["embeddings.class_embedding"], "visual.conv1.weight": st["embeddings.patch_embedding.weight"],
           "visual.positional_embedding": st["embeddings.position_embedding.weight"], "visual.ln_pre.weight": st["pre_layrnorm.weight"],
           "visual.ln_pre.bias": st["pre_layrnorm.bias"], "visual.ln_post.weight": st["post_layernorm.weight"], "visual.ln_post.bias": st["post_layernorm.bias"],
           "visual.proj": st["visual_projection.weight"].t().contiguous()}
    for i in range(layers):
        r, p = f"visual.transformer.resblocks.{i}.", f"encoder.layers.{i}."
        out[r + "attn.in_proj_weight"] = torch.cat([st[p + f"self_attn.{n}.weight"] for n in ("q_proj", "k_proj", "v_proj")], 0)
        out[r + "attn.in_proj_bias"] = torch.cat([st[p + f"self_attn.{n}.bias"] for n in ("q_proj", "k_proj", "v_proj")], 0)
        for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[r + a + ".weight"], out[r + a + ".bias"] = st[p + b + ".weight"], st[p + b + ".bias"]
    return out


def _openai_to_transformers(st, layers):
    """The OpenAI checkpoint's `visual.*` names (clip/model.py VisionTransformer, what the reference's `clip.load` users hold) -> transformers' names.  Written
    from the published layout -- conv1, class_embedding, positional_embedding, ln_pre, transformer.resblocks.N.{ln_1, attn.in_proj_{weight,bias} (q | k | v rows),
    attn.out_proj, ln_2, mlp.c_fc, mlp.c_proj}, ln_post, proj stored [width, projection] (applied as x @ proj) -- and PINNED TO NOTHING: the `clip` package is on
    no machine this project is tested on."""
    st = {(k[len("visual."):] if k.startswith("visual.") else k): v for k, v in st.items()}
    out = {"embeddings.class_embedding": st["class_embedding"], "embeddings.patch_embedding.weight": st["conv1.weight"],
           "embeddings.position_embedding.weight": st["positional_embedding"], "pre_layrnorm.weight": st["ln_pre.weight"], "pre_layrnorm.bias": st["ln_pre.bias"],
           "post_layernorm.weight": st["ln_post.weight"], "post_layernorm.bias": st["ln_post.bias"], "visual_projection.weight": st["proj"].t()}
    for i in range(layers):
        r, p = f"transformer.resblocks.{i}.", f"encoder.layers.{i}."
        C = st[r + "attn.in_proj_weight"].shape[1]
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            out[p + f"self_attn.{n}.weight"] = st[r + "attn.in_proj_weight"][j * C:(j + 1) * C]
            out[p + f"self_attn.{n}.bias"] = st[r + "attn.in_proj_bias"][j * C:(j + 1) * C]
        for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[p + b + ".weight"], out[p + b + ".bias"] = st[r + a + ".weight"], st[r + a + ".bias"]
    return out


def pack_vision_state(cfg, state):
    """CLIPVisionModelWithProjection.state_dict() (names with or without `vision_model.`; `position_ids` ignored), or the OpenAI checkpoint's `visual.*` names
    (see _openai_to_transformers) -> the fp32 host tensors the tower uploads: q | k rows of one GEMM, V apart (its GEMM writes V^T), the patch embedding as a
    [C, 3 p p] GEMM weight, the class row = class_embedding + pos[0].  Missing or mis-shaped parameters raise ValueError."""
    if any(k in state for k in ("visual.conv1.weight", "conv1.weight")):
        try:
            st = _openai_to_transformers(state, cfg.num_hidden_layers)
        except KeyError as e:
            raise ValueError(f"CLIP vision state (OpenAI layout): missing parameter {e.args[0]!r}") from None
    else:
        st = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in state.items()}
    C, ps = cfg.hidden_size, cfg.patch_size
    want = vision_param_shapes(cfg)
    bad = [k for k, s in want.items() if k not in st or tuple(st[k].shape) != s]
    if bad:
        raise ValueError(f"CLIP vision state: missing or mis-shaped parameters {bad[:4]}{' ...' if len(bad) > 4 else ''}")
    f = lambda k: st[k].detach().float().cpu().contiguous()
    pos = f("embeddings.position_embedding.weight")
    out = {"pe.w": f("embeddings.patch_embedding.weight").reshape(C, 3 * ps * ps).contiguous(), "cls": (f("embeddings.class_embedding") + pos[0]).contiguous(),
           "pos": pos[1:].contiguous(), "pre.w": f("pre_layrnorm.weight"), "pre.b": f("pre_layrnorm.bias"), "post.w": f("post_layernorm.weight"),
           "post.b": f("post_layernorm.bias"), "proj.w": f("visual_projection.weight")}
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


def im2col(x, ps):
    """[B, 3, H, W] -> [B (H/ps)(W/ps), 3 ps ps]: one row per patch, columns (channel, ky, kx) like patch_embedding.weight.reshape(C, -1)"""
    B, Cc, H, W = x.shape
    ph, pw = H // ps, W // ps
    return x.reshape(B, Cc, ph, ps, pw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * ph * pw, Cc * ps * ps)


class HipCLIPVision:
    """CLIPVisionModelWithProjection(pixel_values).image_embeds = clip's encode_image on the HIP kernels (module docstring).  forward: float [B, 3, 224, 224]
    (normalised) -> fp32 [B, projection_dim]; features_u8: decoded uint8 images of any one size -> the same, the transform on the device."""

    def __init__(self, config, state, dtype=torch.float32, device="cuda:0", x3=False):
        assert dtype in (torch.float32, torch.bfloat16)
        if x3 and dtype != torch.float32:
            raise ValueError(f"x3=True (split-bf16) takes dtype=torch.float32: operands are split from fp32 values (dtype={dtype})")
        self.config = clip_vision_config(config)
        self.dtype, self.device, self.x3 = dtype, torch.device(device), bool(x3)
        self.host = pack_vision_state(self.config, state)
        cfg, dev = self.config, self.device
        up = lambda k: self.host[k].to(dev)
        lin = lambda k: (ops.pack_linear(up(k + ".w"), dtype, x3=self.x3), up(k + ".b"))
        self.kpe = 3 * cfg.patch_size ** 2                       # 3072 at patch 32: whole 16-byte chunks
        if self.x3 and (self.kpe % 32 or cfg.hidden_size % 32 or cfg.intermediate_size % 32):
            raise ValueError(f"HipCLIPVision x3: contraction lengths {self.kpe}, {cfg.hidden_size}, {cfg.intermediate_size} must be multiples of 32 (blocked pair rows)")
        self.pe, self.proj = ops.pack_linear(up("pe.w"), dtype, x3=self.x3), ops.pack_linear(up("proj.w"), dtype, x3=self.x3)
        self.cls, self.pos = up("cls").to(dtype)[None].contiguous(), up("pos").to(dtype).contiguous()
        self.pre, self.post = (up("pre.w"), up("pre.b")), (up("post.w"), up("post.b"))
        self.blocks = [SimpleNamespace(ln1=(up(f"{i}.ln1.w"), up(f"{i}.ln1.b")), ln2=(up(f"{i}.ln2.w"), up(f"{i}.ln2.b")), qk=lin(f"{i}.qk"), v=lin(f"{i}.v"),
                                       o=lin(f"{i}.o"), fc1=lin(f"{i}.fc1"), fc2=lin(f"{i}.fc2")) for i in range(cfg.num_hidden_layers)]
        self._lut = ops.vit_norm_table(CLIP_MEAN, CLIP_STD).to(dev)

    @classmethod
    def from_torch(cls, module, dtype=torch.float32, device="cuda:0", x3=False):
        """from a transformers CLIPVisionModelWithProjection (its config and state_dict)"""
        return cls(module.config, module.state_dict(), dtype=dtype, device=device, x3=x3)

    def _tower(self, a, B):
        """operand rows of the patch embedding [B n, 3 p p] in the activation dtype (split-bf16: pair rows, or fp32 rows that ops.linear splits) -> fp32
        [B, projection_dim]"""
        cfg, x3 = self.config, self.x3
        C, nh, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
        n = self.pos.shape[0]
        S = n + 1
        res = self.pos.unsqueeze(0).expand(B, -1, -1).reshape(B * n, C).contiguous()
        t = ops.linear(a, self.pe, None, K=self.kpe, residual=res)
        x = torch.cat([self.cls.unsqueeze(0).expand(B, -1, -1), t.view(B, n, C)], dim=1).contiguous()
        x = ops.layernorm(x, *self.pre, eps=eps)
        ld = (S + 7) // 8 * 8
        vt = torch.zeros(B, C, ld, dtype=self.dtype, device=self.device)      # V^T of every layer: padding columns zeroed once, no GEMM writes them
        for b in self.blocks:
            y = ops.layernorm(x, *b.ln1, eps=eps, pair=x3)
            qk = ops.linear(y, b.qk[0], b.qk[1], K=C)                                               # [B, S, 2C]: q | k
            ops.linear(y, b.v[0], b.v[1], K=C, rows_per_batch=S, transposed_ld=ld, out=vt)
            att = ops.attention(qk, qk[..., C:], vt, nh, 0.125, None, Sk=S, C=C, x3=x3, out_pair=x3)
            x = ops.linear(att, b.o[0], b.o[1], K=C, residual=x)
            y = ops.layernorm(x, *b.ln2, eps=eps, pair=x3)
            h = ops.linear(y, b.fc1[0], b.fc1[1], K=C, qgelu=True, out_pair=x3)
            x = ops.linear(h, b.fc2[0], b.fc2[1], K=cfg.intermediate_size, residual=x)
        pooled = ops.layernorm(x[:, 0].contiguous(), *self.post, eps=eps, pair=x3)                  # the class rows only
        return ops.linear(pooled, self.proj, None, K=C).float()

    @torch.no_grad()
    def forward(self, x):
        """x float [B, 3, image_size, image_size] (normalised image) -> fp32 [B, projection_dim]"""
        cfg = self.config
        if tuple(x.shape[1:]) != (3, cfg.image_size, cfg.image_size):
            raise ValueError(f"HipCLIPVision: input {tuple(x.shape)}; the tower takes [B, 3, {cfg.image_size}, {cfg.image_size}] (no positional interpolation)")
        a = im2col(x.to(self.device, torch.float32), cfg.patch_size).to(self.dtype).contiguous()
        return self._tower(a, x.shape[0])

    __call__ = forward

    @torch.no_grad()
    def features_u8(self, images, keep=None):
        """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device); keep = None or (rule, m1, m2) as in ops.resize_pil_u8 (uint8 [B, H, W], host or
        device) -> fp32 [B, projection_dim]: CLIP's transform (clip/clip.py _transform: Resize(n, BICUBIC), CenterCrop(n), ToTensor, Normalize) and the tower"""
        cfg = self.config
        img = torch.as_tensor(images)
        assert img.dtype == torch.uint8 and img.ndim == 4 and img.shape[-1] == 3
        img = img.to(self.device).contiguous()
        if keep is not None:
            keep = (keep[0],) + tuple(None if m is None else torch.as_tensor(m).to(self.device).contiguous() for m in keep[1:])
        size = cfg.image_size
        oh, ow = ops.torchvision_resize_size(img.shape[1], img.shape[2], size)
        small = ops.resize_pil_u8(img, oh, ow, "bicubic", crop=ops.center_crop_window(oh, ow, size), keep=keep)
        if self.x3:
            a = ops.vit_patch_rows_pair(small, self._lut, cfg.patch_size, self.kpe)
        else:
            a = ops.vit_patch_rows(small, self._lut, cfg.patch_size, self.kpe, self.dtype)
        return self._tower(a, img.shape[0])
