"""The CLIP image tower on the HIP kernels: the feature extractor of Background Consistency (the reference's evaluation/metrics/VBench/background_consistency.py:
18-41, `clip.load('ViT-B/32')` -> `clip_model.encode_image`).  The `clip` package is absent here; `transformers.CLIPVisionModelWithProjection(...).image_embeds` is
the same arithmetic and is what the tower is pinned to (tests/test_consistency_cpu.py restates it in fp64, tests/test_consistency_gpu.py holds the device to it).

    rows = im2col(image)  [B 49, 3 32 32];  t = rows W_patch^T + pos[1:]  (no bias; the positional embedding is the GEMM's residual);  x = [class + pos[0] | t]
    x = pre_layrnorm(x)  (transformers' spelling);  per layer: y = LN1(x); q, k, v = Linear(y); a = softmax(q k^T / 8) v per head; x += out_proj(a);
    y = LN2(x); x += fc2(quick_gelu(fc1(y)));  result post_layernorm(x[:, 0]) W_proj^T  -> [B, projection_dim]

The layers are encoder.py's block (every Linear an `ffn_igemm`: q | k in one GEMM, V^T from the transposed-output GEMM, residuals and quick-gelu in the
epilogues; `ffn_layernorm`; non-causal `ffn_attn` at S = 50 with head dim 64).  224 x 224 only: no positional interpolation.

`features_u8` is CLIP's transform on the device, from decoded uint8 images: image * keep mask, Resize(224, BICUBIC) (short side to 224), CenterCrop(224) -- one
ffn_resize_pil_u8 with a crop window, PIL's bicubic bit for bit -- then ToTensor + Normalize(CLIP's mean / std) and the im2col as ffn_vit_patch_rows.

dtype float32 = parity mode (exact-fp32 MFMA), float32 with x3=True = split-bf16, bfloat16 = fast mode.

hps.py's OpenCLIP ViT-H/14 image tower is this class under another configuration check (`_config`), so what differs between the two is read from the
configuration here: the MLP activation (`_ACT`), the head dim, and the patch embedding's contraction length, zero-padded to whole chunks where 3 p p is none
(patch 14; nothing at patch 32).  `_pool` is the class rows' norm, which that tower replaces by one launch.

Split-bf16 (`HipCLIPVision(..., x3=True)`): every GEMM (the 768 -> 512 projection included) and the attention run FFN_BF16X3 -- operands as hi + lo bf16 pairs,
three bf16 MFMAs per product term, fp32 accumulation -- in the layers as encoder.py describes it; post_layernorm too writes the pair rows its GEMM reads; the
residual stream (pre_layrnorm writes it: fp32), the positional embedding and the class row stay fp32.  `features_u8` gets the patch GEMM's rows from
`ffn_vit_patch_rows_pair` (pair rows straight from the bytes), `forward` from fp32 rows that ops.linear splits -- the same operand bytes."""
from types import SimpleNamespace

import torch

from . import encoder, ops

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
    sh.update(encoder.clip_layer_shapes(cfg, q))
    sh.update({q + "post_layernorm.weight": (C,), q + "post_layernorm.bias": (C,), "visual_projection.weight": (P, C)})
    return sh


def synthetic_state(cfg, seed=0):
    """seeded random weights of a plausible scale in transformers' layout (with the `vision_model.` prefix), drawn the way dino.synthetic_state draws them: for
    tests and benchmarks without a checkpoint (there is no network)"""
    return encoder.draw_state(vision_param_shapes(cfg, "vision_model."), seed)


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
    return encoder.pack_clip_layers(cfg, f, out)


im2col = encoder.im2col


class HipCLIPVision:
    """CLIPVisionModelWithProjection(pixel_values).image_embeds = clip's encode_image on the HIP kernels (module docstring).  forward: float [B, 3, 224, 224]
    (normalised) -> fp32 [B, projection_dim]; features_u8: decoded uint8 images of any one size -> the same, the transform on the device."""

    _config = staticmethod(clip_vision_config)      # the checked configuration of this tower (hps.py's ViT-H/14 tower has its own)
    _ACT = {"quick_gelu": "qgelu", "gelu": "gelu"}    # hidden_act -> fc1's GEMM epilogue

    def __init__(self, config, state, dtype=torch.float32, device="cuda:0", x3=False):
        encoder.check_mode(dtype, x3)
        self.config = self._config(config)
        self.dtype, self.device, self.x3 = dtype, torch.device(device), bool(x3)
        self.host = pack_vision_state(self.config, state)
        cfg, dev = self.config, self.device
        up = lambda k: self.host[k].to(dev)
        K, e = 3 * cfg.patch_size ** 2, 32 if self.x3 else 8     # split-bf16: whole 32-column blocks, so that both operands are in the blocked pair form
        self.kpe = (K + e - 1) // e * e                          # 3072 at patch 32: whole chunks as it is; patch 14: 588 -> 592, split-bf16 608 (zero columns, as dino.py)
        if self.x3 and (cfg.hidden_size % 32 or cfg.intermediate_size % 32):
            raise ValueError(f"{type(self).__name__} x3: contraction lengths {cfg.hidden_size}, {cfg.intermediate_size} must be multiples of 32 (blocked pair rows)")
        wpe = up("pe.w")
        if self.kpe != K:
            wpe = torch.nn.functional.pad(wpe, (0, self.kpe - K))
        self.pe, self.proj = ops.pack_linear(wpe, dtype, x3=self.x3), ops.pack_linear(up("proj.w"), dtype, x3=self.x3)
        self.cls, self.pos = up("cls").to(dtype)[None].contiguous(), up("pos").to(dtype).contiguous()
        self.pre, self.post = (up("pre.w"), up("pre.b")), (up("post.w"), up("post.b"))
        self.blocks = encoder.clip_blocks(cfg, self.host, dev, dtype, self.x3)
        self._lut = ops.vit_norm_table(CLIP_MEAN, CLIP_STD).to(dev)

    @classmethod
    def from_torch(cls, module, dtype=torch.float32, device="cuda:0", x3=False):
        """from a transformers CLIPVisionModelWithProjection (its config and state_dict)"""
        return cls(module.config, module.state_dict(), dtype=dtype, device=device, x3=x3)

    def _tower(self, a, B):
        """operand rows of the patch embedding [B n, 3 p p] in the activation dtype (split-bf16: pair rows, or fp32 rows that ops.linear splits) -> fp32
        [B, projection_dim]"""
        cfg, x3 = self.config, self.x3
        C, eps = cfg.hidden_size, cfg.layer_norm_eps
        x = encoder.embed_patches(a, self.pe, None, self.kpe, self.pos, self.cls, B)
        x = ops.layernorm(x, *self.pre, eps=eps)
        vt = encoder.vt_buffer(x)
        for b in self.blocks:
            x = encoder.run_block(b, x, vt, heads=cfg.num_attention_heads, eps=eps, act=self._ACT[cfg.hidden_act], hidden=cfg.intermediate_size, x3=x3)
        return ops.linear(self._pool(x), self.proj, None, K=C).float()

    def _pool(self, x):
        """post_layernorm of the class rows only (split-bf16: as the pair rows the projection reads)"""
        return ops.layernorm(x[:, 0].contiguous(), *self.post, eps=self.config.layer_norm_eps, pair=self.x3)

    @torch.no_grad()
    def forward(self, x):
        """x float [B, 3, image_size, image_size] (normalised image) -> fp32 [B, projection_dim]"""
        cfg = self.config
        if tuple(x.shape[1:]) != (3, cfg.image_size, cfg.image_size):
            raise ValueError(f"{type(self).__name__}: input {tuple(x.shape)}; the tower takes [B, 3, {cfg.image_size}, {cfg.image_size}] (no positional interpolation)")
        a = im2col(x.to(self.device, torch.float32), cfg.patch_size).to(self.dtype)
        if self.kpe != a.shape[1]:
            a = torch.nn.functional.pad(a, (0, self.kpe - a.shape[1]))
        a = a.contiguous()
        return self._tower(a, x.shape[0])

    __call__ = forward

    @torch.no_grad()
    def features_u8(self, images, keep=None):
        """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device); keep = None or (rule, m1, m2) as in ops.resize_pil_u8 (uint8 [B, H, W], host or
        device) -> fp32 [B, projection_dim]: CLIP's transform (clip/clip.py _transform: Resize(n, BICUBIC), CenterCrop(n), ToTensor, Normalize) and the tower"""
        cfg = self.config
        small = encoder.clip_crop_u8(images, keep, cfg.image_size, self.device)
        a = encoder.patch_rows_u8(small, self._lut, cfg.patch_size, self.kpe, self.dtype, self.x3)
        return self._tower(a, small.shape[0])
