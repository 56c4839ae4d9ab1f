"""The ImageReward score (the reference's evaluation/metrics/image_reward.py: ImageReward-v1.0 = BLIP's ViT-L/16 image tower, BLIP's cross-attending BERT and a
five-layer reward head) on the HIP kernels: the reward of a generated image given its caption.

    image : Resize(224, BICUBIC) on the short side, CenterCrop(224), ToTensor, Normalize(CLIP's mean / std)      -> HipBlipVision -> image_embeds [B, 197, 1024]
    text  : BertTokenizer(bert-base-uncased) + BLIP's two added specials, padded / truncated to 35              -> ids, attention_mask
            HipBlipText: x = LN(word[id] + pos[s]); 12 post-LN layers of  x = LN(x + O_s(attn(x, x, x; key mask)));  x = LN(x + O_c(attn(x, image_embeds)));
            x = LN(x + W2 gelu(W1 x))                                                                            -> x[:, 0]  [B, 768]
    reward: 768 -> 1024 -> 128 -> 64 -> 16 -> 1, five Linears with nothing but dropout between them (`ffn_affine_chain`, layer by layer), then
            (r - 0.16717362830052426) / 1.0333394966054072

Neither `ImageReward` nor BLIP's own code exists where this project is tested.  transformers' BlipVisionModel (last_hidden_state: post_layernorm over ALL tokens)
and BlipTextModel (a port of BLIP's med.py BERT: built with is_decoder=True so that every layer has its `crossattention`, called with is_decoder=False and
encoder_hidden_states, which is the bidirectional, key-padding-masked encoder ImageReward calls) are the same arithmetic and are what the towers are pinned to
(tests/irs_ref.py restates them in fp64, tests/test_irs_gpu.py holds the device to them).

What is NOT pinned -- written from the published source, with nothing offline to check it against:
  * the preprocessing: ImageReward's _transform (Resize(224, BICUBIC), CenterCrop(224), RGB, ToTensor, Normalize with CLIP's mean / std);
  * the tokenizer: bert-base-uncased's vocabulary plus BLIP's `[DEC]` (bos) and `[ENC]` (additional special) = 30524 ids, max_length 35; the ids go in as
    the tokenizer returns them (score() does not replace [CLS] by [ENC]);
  * the checkpoint's names (`blip.visual_encoder.*` in timm's layout, `blip.text_encoder.*` in BERT's, `mlp.layers.{0, 2, 4, 6, 7}.*`) and the two constants of
    the final standardisation;
  * parity with the published ImageReward.pt: no weights exist offline.

HipBlipVision is dino.py's encoder (HipDinoEncoder: timm's layout, LayerScale absent) at patch 16 on the fixed 224 grid; its final `norm` runs over all 197
tokens.  HipBlipText's layers are encoder.py's CrossBlock.  The cross-attention's K and V^T read the image tokens only: they are projected for all layers
before the first layer runs (encoder.cross_kv: the twelve K projections as ONE GEMM).  The key mask is one uint8 buffer per prompt (`kmask` of ffn_attn).

Modes: dtype float32 = parity mode (exact-fp32 MFMA), float32 with x3=True = split-bf16, bfloat16 = fast mode.  The head always runs in fp32.  The reference
evaluates in fp32."""
import os
from types import SimpleNamespace

import torch

from . import dino, encoder, ops, text
from .clipvision import CLIP_MEAN, CLIP_STD

REWARD_MEAN, REWARD_STD = 0.16717362830052426, 1.0333394966054072
MAX_LENGTH = 35
HEAD_LAYERS = (0, 2, 4, 6, 7)          # the Linears of ImageReward's nn.Sequential `mlp.layers` (dropouts between them)

# ---------------------------------------------------------------------------------------------------------------------
# the image tower
# ---------------------------------------------------------------------------------------------------------------------
_VISION = dict(vitl16=dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16),
               tiny16=dict(hidden_size=192, intermediate_size=768, num_hidden_layers=2, num_attention_heads=3))      # tiny16's width = the tiny text tower's encoder width
_VISION_FIELDS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size", "hidden_act", "layer_norm_eps")
_VISION_DEFAULTS = dict(image_size=224, patch_size=16, hidden_act="gelu", layer_norm_eps=1e-6)      # BLIP's ViT: timm's LayerNorm eps


def _fields(config, fields, defaults, what):
    get = (lambda k: config.get(k, defaults.get(k))) if isinstance(config, dict) else (lambda k: getattr(config, k, defaults.get(k)))
    cfg = {k: get(k) for k in fields}
    missing = [k for k in fields if cfg[k] is None]
    if missing:
        raise ValueError(f"{what}: missing {missing}")
    return SimpleNamespace(**cfg)


def blip_vision_config(config="vitl16"):
    """"vitl16" (BLIP's ViT-L/16: width 1024, 24 blocks, 16 heads of 64, MLP 4096, LayerNorm eps 1e-6) / "tiny16" (the test size: width 192, 3 heads, 2 blocks), a
    BlipVisionConfig or a dict of its fields -> the configuration HipDinoEncoder runs (embed_dim, depth, num_heads, patch, img_size, mlp_ratio, ln_eps; no
    LayerScale), checked.  Raises ValueError with the reason otherwise."""
    if isinstance(config, SimpleNamespace) and hasattr(config, "embed_dim"):
        return config
    name = config if isinstance(config, str) else "custom"
    if isinstance(config, str):
        if config not in _VISION:
            raise ValueError(f"BLIP vision config {config!r} (one of {sorted(_VISION)})")
        config = _VISION[config]
    c = _fields(config, _VISION_FIELDS, _VISION_DEFAULTS, "BLIP vision config")
    C, nh = c.hidden_size, c.num_attention_heads
    if C % nh != 0 or C // nh != 64:
        raise ValueError(f"BLIP vision tower: head dim {C / nh:g} (hidden_size {C} / {nh} heads); the tower runs the head-dim-64 attention kernels")
    if c.hidden_act != "gelu":
        raise ValueError(f"BLIP vision tower: hidden_act {c.hidden_act!r}; BLIP's ViT uses 'gelu'")
    if c.image_size % c.patch_size != 0 or c.intermediate_size % C != 0:
        raise ValueError(f"BLIP vision tower: image {c.image_size} / patch {c.patch_size}, MLP {c.intermediate_size} / width {C}: whole patches and a whole MLP ratio only")
    return SimpleNamespace(name=name, embed_dim=C, depth=c.num_hidden_layers, num_heads=nh, patch=c.patch_size, img_size=c.image_size,
                           mlp_ratio=c.intermediate_size // C, interpolate_offset=0.1, ln_eps=c.layer_norm_eps, layerscale=False)


def transformers_vision_config(cfg):
    """the BlipVisionConfig of a checked configuration (tests and tools build the yardstick module from it)"""
    from transformers import BlipVisionConfig
    return BlipVisionConfig(hidden_size=cfg.embed_dim, intermediate_size=cfg.embed_dim * cfg.mlp_ratio, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads,
                            image_size=cfg.img_size, patch_size=cfg.patch, hidden_act="gelu", layer_norm_eps=cfg.ln_eps)


def vision_param_shapes(cfg, prefix=""):
    """name -> shape of BLIP's VisionTransformer.state_dict() (timm's layout)"""
    sh = dino.dinov2_param_shapes(cfg, prefix)
    del sh[prefix + "mask_token"]
    return sh


_VIS_TOP = (("embeddings.class_embedding", "cls_token"), ("embeddings.position_embedding", "pos_embed"), ("embeddings.patch_embedding.weight", "patch_embed.proj.weight"),
            ("embeddings.patch_embedding.bias", "patch_embed.proj.bias"), ("post_layernorm.weight", "norm.weight"), ("post_layernorm.bias", "norm.bias"))
_VIS_LAYER = (("layer_norm1", "norm1"), ("self_attn.qkv", "attn.qkv"), ("self_attn.projection", "attn.proj"), ("layer_norm2", "norm2"), ("mlp.fc1", "mlp.fc1"),
              ("mlp.fc2", "mlp.fc2"))


def _vision_names(depth):
    """(transformers' BlipVisionModel name, timm's name) of every parameter"""
    names = list(_VIS_TOP)
    for i in range(depth):
        names += [(f"encoder.layers.{i}.{a}.{p}", f"blocks.{i}.{b}.{p}") for a, b in _VIS_LAYER for p in ("weight", "bias")]
    return names


def to_transformers_vision_layout(state, depth):
    """timm's names -> BlipVisionModel's (the same tensors: both keep cls_token [1, 1, C], pos_embed [1, 197, C] and the fused qkv)"""
    return {a: state[b] for a, b in _vision_names(depth)}


def pack_vision_state(cfg, state):
    """BLIP's timm layout (cls_token, pos_embed, patch_embed.proj.*, blocks.N.{norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2}.*, norm.*) or transformers'
    BlipVisionModel layout (names with or without `vision_model.`) -> fp32 host tensors under timm's names.  Missing or mis-shaped parameters raise ValueError."""
    st = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in state.items()}
    if "embeddings.class_embedding" in st:
        st = {b: st[a] for a, b in _vision_names(cfg.depth) if a in st}
    want = vision_param_shapes(cfg)
    bad = [k for k, s in want.items() if k not in st or tuple(st[k].shape) != s]
    if bad:
        raise ValueError(f"BLIP vision state: missing or mis-shaped parameters {bad[:4]}{' ...' if len(bad) > 4 else ''}")
    return {k: st[k].detach().float().cpu().contiguous() for k in want}


class HipBlipVision(dino.HipDinoEncoder):
    """BLIP's VisionTransformer = transformers' BlipVisionModel(pixel_values).last_hidden_state on the HIP kernels: dino.py's encoder at patch 16 on the fixed
    224 x 224 grid (no LayerScale, no positional interpolation), the final `norm` over ALL tokens.  forward: float [B, 3, 224, 224] (normalised) -> [B, 197, C] in
    the activation type; features_u8: decoded uint8 images of any one size -> the same, CLIP's transform on the device (encoder.clip_crop_u8, as
    HipCLIPVision.features_u8)."""

    def __init__(self, config, state, dtype=torch.float32, device="cuda:0", x3=False):
        encoder.check_mode(dtype, x3)
        self.config = blip_vision_config(config)
        host = pack_vision_state(self.config, state)
        self._init_encoder(self.config, dtype, device, x3=x3)
        self._pack_encoder({k: v.to(self.device) for k, v in host.items()}, "")
        self._lut = ops.vit_norm_table(CLIP_MEAN, CLIP_STD).to(self.device)

    @classmethod
    def from_torch(cls, module, dtype=torch.float32, device="cuda:0", x3=False):
        """from a transformers BlipVisionModel (its config and state_dict)"""
        return cls(module.config, module.state_dict(), dtype=dtype, device=device, x3=x3)

    def _embeds(self, t, pair=False):
        """tokens -> blocks -> `norm` of every token (pair: as the pair rows a split-bf16 GEMM reads, for the text tower's K / V projections)"""
        return ops.layernorm(self._run_blocks(t, 1)[0], *self.norm, eps=self.cfg.ln_eps, pair=pair)

    @torch.no_grad()
    def forward(self, x, pair=False):
        """x float [B, 3, 224, 224] (normalised image) -> image_embeds [B, 197, C] in the activation type"""
        n = self.cfg.img_size
        if x.ndim != 4 or tuple(x.shape[1:]) != (3, n, n):
            raise ValueError(f"HipBlipVision: input {tuple(x.shape)}; the tower takes [B, 3, {n}, {n}] (a fixed grid: no positional interpolation)")
        return self._embeds(self._tokens(x)[0], pair)

    __call__ = forward

    @torch.no_grad()
    def features_u8(self, images, pair=False):
        """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device) -> image_embeds [B, 197, C]: ImageReward's transform and the tower"""
        small = encoder.clip_crop_u8(images, None, self.cfg.img_size, self.device)
        B, H, W, _ = small.shape
        a = encoder.patch_rows_u8(small, self._lut, self.cfg.patch, self.kpe, self.dtype, self.x3)
        return self._embeds(self._embed(a, B, H, W)[0], pair)


# ---------------------------------------------------------------------------------------------------------------------
# the text tower
# ---------------------------------------------------------------------------------------------------------------------
_TEXT = dict(med=dict(vocab_size=30524, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, max_position_embeddings=512,
                      encoder_hidden_size=1024),                                             # BLIP's med_config.json with ViT-L's width
             tiny=dict(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=40,
                       encoder_hidden_size=192))                                             # the test size; 300 >= text.ByteTokenizer's 259 ids
_TEXT_FIELDS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings", "encoder_hidden_size",
                "hidden_act", "layer_norm_eps")
_TEXT_DEFAULTS = dict(hidden_act="gelu", layer_norm_eps=1e-12)


def blip_text_config(config="med"):
    """"med" (BLIP's BERT: hidden 768, 12 layers, 12 heads of 64, MLP 3072, erf-gelu, LayerNorm eps 1e-12, vocabulary 30524, cross-attending to width 1024) /
    "tiny" (the test size), a BlipTextConfig or a dict of its fields -> the fields the tower needs, checked.  Raises ValueError with the reason otherwise."""
    if isinstance(config, SimpleNamespace):
        return config
    if isinstance(config, str):
        if config not in _TEXT:
            raise ValueError(f"BLIP text config {config!r} (one of {sorted(_TEXT)})")
        config = _TEXT[config]
    cfg = _fields(config, _TEXT_FIELDS, _TEXT_DEFAULTS, "BLIP text config")
    C, nh = cfg.hidden_size, cfg.num_attention_heads
    if C % nh != 0 or C // nh != 64:
        raise ValueError(f"BLIP text tower: head dim {C / nh:g} (hidden_size {C} / {nh} heads); the tower runs the head-dim-64 attention kernels")
    if cfg.hidden_act != "gelu":
        raise ValueError(f"BLIP text tower: hidden_act {cfg.hidden_act!r}; BERT's MLP uses 'gelu'")
    if cfg.intermediate_size % 8 != 0 or cfg.encoder_hidden_size % 8 != 0:
        raise ValueError(f"BLIP text tower: MLP {cfg.intermediate_size}, encoder width {cfg.encoder_hidden_size}: multiples of 8 only")
    return cfg


def transformers_text_config(cfg):
    """the BlipTextConfig of a checked configuration: is_decoder=True gives every layer its `crossattention` (the module is then CALLED with is_decoder=False)"""
    from transformers import BlipTextConfig
    return BlipTextConfig(**{k: getattr(cfg, k) for k in _TEXT_FIELDS}, is_decoder=True, pad_token_id=0, bos_token_id=None, eos_token_id=None, sep_token_id=None,
                          hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def text_param_shapes(cfg, prefix=""):
    """name -> shape of BlipTextModel(add_pooling_layer=False).state_dict() = BLIP's BertModel"""
    C, I, E, q = cfg.hidden_size, cfg.intermediate_size, cfg.encoder_hidden_size, prefix
    sh = {q + "embeddings.word_embeddings.weight": (cfg.vocab_size, C), q + "embeddings.position_embeddings.weight": (cfg.max_position_embeddings, C),
          q + "embeddings.LayerNorm.weight": (C,), q + "embeddings.LayerNorm.bias": (C,)}
    for i in range(cfg.num_hidden_layers):
        p = f"{q}encoder.layer.{i}."
        for att, kin in (("attention", C), ("crossattention", E)):
            for n, k in (("query", C), ("key", kin), ("value", kin)):
                sh[p + f"{att}.self.{n}.weight"], sh[p + f"{att}.self.{n}.bias"] = (C, k), (C,)
            sh[p + f"{att}.output.dense.weight"], sh[p + f"{att}.output.dense.bias"] = (C, C), (C,)
            sh[p + f"{att}.output.LayerNorm.weight"], sh[p + f"{att}.output.LayerNorm.bias"] = (C,), (C,)
        sh[p + "intermediate.dense.weight"], sh[p + "intermediate.dense.bias"] = (I, C), (I,)
        sh[p + "output.dense.weight"], sh[p + "output.dense.bias"] = (C, I), (C,)
        sh[p + "output.LayerNorm.weight"], sh[p + "output.LayerNorm.bias"] = (C,), (C,)
    return sh


def pack_text_state(cfg, state):
    """BlipTextModel / BLIP BertModel parameters (persistent `position_ids` buffers and a pooler ignored) -> fp32 host tensors under the same names.  Missing or
    mis-shaped parameters raise ValueError."""
    want = text_param_shapes(cfg)
    bad = [k for k, s in want.items() if k not in state or tuple(state[k].shape) != s]
    if bad:
        raise ValueError(f"BLIP text state: missing or mis-shaped parameters {bad[:4]}{' ...' if len(bad) > 4 else ''}")
    return {k: state[k].detach().float().cpu().contiguous() for k in want}


class HipBlipText:
    """BLIP's cross-attending BERT = transformers' BlipTextModel(ids, attention_mask, encoder_hidden_states=image_embeds, is_decoder=False).last_hidden_state[:, 0]
    on the HIP kernels (module docstring).  The embedding is `ffn_embed_tokens_ln`, the layers are encoder.run_cross_block."""

    def __init__(self, config, state, dtype=torch.float32, device="cuda:0", x3=False):
        encoder.check_mode(dtype, x3)
        self.config = cfg = blip_text_config(config)
        self.dtype, self.device, self.x3 = dtype, torch.device(device), bool(x3)
        if self.x3 and (cfg.hidden_size % 32 or cfg.intermediate_size % 32 or cfg.encoder_hidden_size % 32):
            raise ValueError(f"HipBlipText x3: contraction lengths {cfg.hidden_size}, {cfg.intermediate_size}, {cfg.encoder_hidden_size} must be multiples of 32 "
                             "(blocked pair rows)")
        host = pack_text_state(cfg, state)
        up = lambda k: host[k].to(self.device)
        wb = lambda k: (up(k + ".weight"), up(k + ".bias"))
        self.tok, self.pos, self.lne = up("embeddings.word_embeddings.weight"), up("embeddings.position_embeddings.weight"), wb("embeddings.LayerNorm")
        self.blocks, wk, bk, self.wv = [], [], [], []
        for i in range(cfg.num_hidden_layers):
            p, a, c = f"encoder.layer.{i}.", f"encoder.layer.{i}.attention.", f"encoder.layer.{i}.crossattention."
            qk = (torch.cat([up(a + "self.query.weight"), up(a + "self.key.weight")], 0), torch.cat([up(a + "self.query.bias"), up(a + "self.key.bias")], 0))
            self.blocks.append(encoder.pack_cross_block(qk, wb(a + "self.value"), wb(a + "output.dense"), wb(a + "output.LayerNorm"), wb(c + "self.query"),
                                                        wb(c + "output.dense"), wb(c + "output.LayerNorm"), wb(p + "intermediate.dense"), wb(p + "output.dense"),
                                                        wb(p + "output.LayerNorm"), dtype, self.x3))
            wk.append(up(c + "self.key.weight")), bk.append(up(c + "self.key.bias"))
            self.wv.append((ops.pack_linear(up(c + "self.value.weight"), dtype, x3=self.x3), up(c + "self.value.bias")))
        self.wk = (ops.pack_linear(torch.cat(wk, 0).contiguous(), dtype, x3=self.x3), torch.cat(bk, 0).contiguous())      # the layers' cross K projections: ONE GEMM

    @classmethod
    def from_torch(cls, module, dtype=torch.float32, device="cuda:0", x3=False):
        """from a transformers BlipTextModel built with is_decoder=True (its config and state_dict)"""
        return cls(module.config, module.state_dict(), dtype=dtype, device=device, x3=x3)

    def _stream(self, ids, mask, image_embeds):
        """the checks of forward, then every layer -> the last layer's output [B, S, C] in the activation type"""
        cfg, name = self.config, type(self).__name__
        ids, mask = torch.as_tensor(ids).cpu(), torch.as_tensor(mask).cpu()
        if ids.ndim == 1:
            ids, mask = ids[None], mask[None]
        N, S = ids.shape
        B = image_embeds.shape[0]
        Ce = ops.pair_width(image_embeds) or image_embeds.shape[-1]
        if tuple(mask.shape) != (N, S):
            raise ValueError(f"{name}: ids {tuple(ids.shape)} and mask {tuple(mask.shape)} differ")
        if N not in (1, B):
            raise ValueError(f"{name}: {N} prompts for {B} images (one, or one each)")
        if S > cfg.max_position_embeddings:
            raise ValueError(f"{name}: {S} positions requested (at most {cfg.max_position_embeddings})")
        if int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab_size:
            raise ValueError(f"{name}: token ids outside [0, {cfg.vocab_size})")
        live = mask != 0
        if not bool(live.any(-1).all()):
            raise ValueError(f"{name}: a prompt without a live token (attention_mask all zero)")
        if image_embeds.ndim != 3 or Ce != cfg.encoder_hidden_size or not image_embeds.is_cuda:
            raise ValueError(f"{name}: image_embeds {tuple(image_embeds.shape)}; the cross-attention reads device rows of {cfg.encoder_hidden_size} values")
        km = torch.zeros(N, (S + 3) // 4 * 4, dtype=torch.uint8)          # rows 4 bytes apart in whole words: the attention kernels read a mask in 32-bit words
        km[:, :S] = live.to(torch.uint8)
        km = km.to(self.device)
        idd = ids.to(torch.int32).expand(B, S).contiguous().to(self.device)
        x = ops.embed_tokens_ln(idd, self.tok, self.pos, *self.lne, self.dtype, eps=cfg.layer_norm_eps)
        vt = encoder.vt_buffer(x)
        ck, cvt = encoder.cross_kv(image_embeds, self.wk, self.wv, cfg.num_hidden_layers, cfg.hidden_size)
        for i, b in enumerate(self.blocks):
            x = encoder.run_cross_block(b, x, vt, ck[i], cvt[i], heads=cfg.num_attention_heads, eps=cfg.layer_norm_eps, hidden=cfg.intermediate_size,
                                        kmask=[km[n] for n in range(N)], x3=self.x3)
        return x

    @torch.no_grad()
    def forward(self, ids, mask, image_embeds):
        """ids, mask int [N, S] on the host (N = 1: one prompt for all images, or N = B; S <= max_position_embeddings; ids range-checked here; mask: non-zero =
        a live token, at least one per prompt), image_embeds [B, Sk, encoder_hidden_size] on the device in the activation type (split-bf16: fp32 or pair rows)
        -> fp32 [B, hidden_size]: row 0 of the last layer"""
        return self._stream(ids, mask, image_embeds)[:, 0].float().contiguous()

    __call__ = forward


# ---------------------------------------------------------------------------------------------------------------------
# the checkpoint, the score
# ---------------------------------------------------------------------------------------------------------------------
def head_param_shapes(hidden=768, prefix="mlp."):
    """name -> shape of ImageReward's reward head"""
    dims = (hidden, 1024, 128, 64, 16, 1)
    sh = {}
    for i, n in enumerate(HEAD_LAYERS):
        sh[f"{prefix}layers.{n}.weight"], sh[f"{prefix}layers.{n}.bias"] = (dims[i + 1], dims[i]), (dims[i + 1],)
    return sh


def synthetic_state(vision_config="vitl16", text_config="med", seed=0):
    """seeded random weights of a plausible scale in ImageReward's layout (blip.visual_encoder.*, blip.text_encoder.*, mlp.layers.*), drawn by
    encoder.draw_state: for tests and benchmarks without a checkpoint (there is no network).  BERT spells its norms `LayerNorm`: they are drawn as norms."""
    vcfg, tcfg = blip_vision_config(vision_config), blip_text_config(text_config)
    sh = vision_param_shapes(vcfg, "blip.visual_encoder.")
    sh.update(text_param_shapes(tcfg, "blip.text_encoder."))
    sh.update(head_param_shapes(tcfg.hidden_size))
    return draw_state(sh, seed)


def draw_state(shapes, seed):
    """encoder.draw_state for names that spell a norm `LayerNorm` (BERT's): its weights are drawn around 1 like every other norm's"""
    low = encoder.draw_state({k.replace("LayerNorm", "layer_norm"): v for k, v in shapes.items()}, seed)
    return {k: low[k.replace("LayerNorm", "layer_norm")] for k in shapes}


def split_state(state):
    """an ImageReward checkpoint's state_dict (blip.visual_encoder.*, blip.text_encoder.*, mlp.layers.{0, 2, 4, 6, 7}.*; everything else ignored), or a dict that
    already holds {"vision", "text", "head"} -> (the image tower's state, the text tower's state, the head's [(W, b)] in order)"""
    if all(k in state for k in ("vision", "text", "head")):
        vis, txt, head = state["vision"], state["text"], state["head"]
    else:
        cut = lambda p: {k[len(p):]: v for k, v in state.items() if k.startswith(p)}
        vis, txt, head = cut("blip.visual_encoder."), cut("blip.text_encoder."), cut("mlp.")
    if isinstance(head, dict):
        try:
            head = [(head[f"layers.{n}.weight"], head[f"layers.{n}.bias"]) for n in HEAD_LAYERS]
        except KeyError as e:
            raise ValueError(f"ImageReward state: missing parameter 'mlp.{e.args[0]}'") from None
    return vis, txt, list(head)


class HipImageReward:
    """ImageReward.score on the HIP towers.  vision: a HipBlipVision; text: a HipBlipText whose encoder width is the image tower's; head: the five (W, b) of
    `mlp.layers`; tokenizer: callable(prompts, padding="max_length", truncation=True, max_length=35, return_tensors="pt") with .input_ids and (optionally)
    .attention_mask -- load_tokenizer's BertTokenizer, or text.ByteTokenizer in tests (mask = ids != 0)."""

    def __init__(self, vision, text, head, tokenizer):
        if vision.cfg.embed_dim != text.config.encoder_hidden_size:
            raise ValueError(f"HipImageReward: image tokens of {vision.cfg.embed_dim} values, cross-attention reading {text.config.encoder_hidden_size}")
        if (vision.dtype, vision.x3) != (text.dtype, text.x3):
            raise ValueError("HipImageReward: the two towers run different modes")
        self.vision, self.text, self.tokenizer, self.device = vision, text, tokenizer, vision.device
        params, self.dims = ops.affine_chain_params([(torch.as_tensor(w), torch.as_tensor(b)) for w, b in head])
        if self.dims[0] != text.config.hidden_size or self.dims[-1] != 1 or len(self.dims) - 1 > ops.L.CHAIN_MAXL or max(self.dims) > ops.L.CHAIN_MAXW:
            raise ValueError(f"HipImageReward: head widths {self.dims} (from {text.config.hidden_size} to 1, at most {ops.L.CHAIN_MAXL} layers of {ops.L.CHAIN_MAXW})")
        self.params = params.to(self.device)

    @classmethod
    def from_state(cls, state, tokenizer, vision_config="vitl16", text_config="med", dtype=torch.float32, device="cuda:0", x3=False):
        """from one state dict holding the towers and the head (split_state) and the towers' configurations"""
        vis, txt, head = split_state(state)
        return cls(HipBlipVision(vision_config, vis, dtype=dtype, device=device, x3=x3), HipBlipText(text_config, txt, dtype=dtype, device=device, x3=x3), head, tokenizer)

    def tokens(self, prompts):
        """prompts (a str or a list) -> (ids, mask) int64 [N, 35] on the host"""
        tok = self.tokenizer([prompts] if isinstance(prompts, str) else list(prompts), padding="max_length", truncation=True, max_length=MAX_LENGTH, return_tensors="pt")
        ids = tok.input_ids
        mask = getattr(tok, "attention_mask", None)
        return ids, (ids != 0).long() if mask is None else mask

    @torch.no_grad()
    def score_u8(self, images_u8, prompt):
        """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device), prompt: one str for all of them, or B of them -> fp32 [B] on the device:
        each image's reward given its prompt"""
        ids, mask = self.tokens(prompt)
        B = len(images_u8)
        if ids.shape[0] not in (1, B):
            raise ValueError(f"HipImageReward: {ids.shape[0]} prompts for {B} images (one, or one each)")
        x = self.text._stream(ids, mask, self.vision.features_u8(images_u8, pair=self.vision.x3))
        _, S, C = x.shape
        if x.dtype == torch.float32:                      # row 0 of every sequence, read in place
            r = ops.affine_chain(x, self.params, self.dims, REWARD_MEAN, REWARD_STD, ldx=S * C, B=B)
        else:
            r = ops.affine_chain(x[:, 0].float().contiguous(), self.params, self.dims, REWARD_MEAN, REWARD_STD)
        return r.view(B)


def load_tokenizer(path):
    """"bytes" -> text.ByteTokenizer (tests; mask = ids != 0); a folder with vocab.txt -> transformers.BertTokenizer from that local file, lower-casing, with
    BLIP's two added specials ([DEC] as bos, [ENC] as an additional special: BLIP's init_tokenizer), which pads with id 0"""
    if path == "bytes":
        return text.ByteTokenizer()
    vocab = os.path.join(path, "vocab.txt")
    if not os.path.isfile(vocab):
        raise ValueError(f"--irs_tokenizer: {vocab} not found (a folder with bert-base-uncased's vocab.txt)")
    from transformers import BertTokenizer
    tok = BertTokenizer(vocab, do_lower_case=True)
    tok.add_special_tokens({"bos_token": "[DEC]"})
    tok.add_special_tokens({"additional_special_tokens": ["[ENC]"]})
    return tok
