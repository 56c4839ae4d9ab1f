"""The Human Preference Score (the reference's evaluation/metrics/human_preference_score.py: HPSv2 = OpenCLIP ViT-H/14 with the `HPS_v2.1_compressed.pt`
weights) on the HIP kernels: the score of a generated image is the cosine between the tower's embedding of the image and of the image's caption.

    image: Resize(224, BICUBIC) on the short side, CenterCrop(224), ToTensor, Normalize(CLIP's mean / std)  -> HipOpenCLIPVision -> [B, 1024]
    text:  CLIP's BPE tokens, padded / truncated to 77                                                          -> text.HipCLIPTextWithProjection -> [1, 1024]
    score_i = <f_i, t> / (max(|f_i|, 1e-12) max(|t|, 1e-12))                                                    (`ffn_cosine_rows`: F.normalize's rule)

Neither `hpsv2` nor `open_clip` exists where this project is tested.  transformers' CLIPVisionModelWithProjection / CLIPTextModelWithProjection with a ViT-H/14
configuration are the same arithmetic and are what the towers are pinned to (tests/test_hps_cpu.py restates them in fp64, tests/test_hps_gpu.py holds the device
to them) -- the substitution clipvision.py made for `clip.load('ViT-B/32')`.  What is NOT pinned: the checkpoint's names (read from open_clip's published layout:
clipvision._openai_to_transformers for `visual.*`, text._openclip_text_to_transformers for the rest) and hpsv2's vendored copy of open_clip's transform,
which could not be read here: the preprocessing is open_clip's validation transform as published (image_transform(is_train=False): Resize(size, BICUBIC),
CenterCrop(size), convert to RGB, ToTensor, Normalize) -- exactly what HipCLIPVision.features_u8 does for CLIP ViT-B/32.  The reference evaluates the towers
under fp16 autocast; these run fp32 (or split-bf16 / bf16 on request), so scores agree with the reference's to fp16's accuracy at best.  No HPSv2 weights exist
offline: parity against the published checkpoint is unmeasured.

HipOpenCLIPVision is HipCLIPVision (clipvision.py: same packing, same `_tower`, same `features_u8`) under a configuration check of its own: head dim 64 or 80,
erf-gelu or quick-gelu, any patch size.  At patch 14 the patch embedding's contraction length 3 * 14 * 14 = 588 is zero-padded to whole chunks as dino.py does:
592, or 608 in split-bf16.

Modes: dtype float32 = parity mode (exact-fp32 MFMA), float32 with x3=True = split-bf16, bfloat16 = fast mode.  AT HEAD DIM 80 THE SPLIT-BF16 MODE'S ATTENTION
IS THE EXACT fp32 KERNEL: the library's attention plan routes FFN_BF16X3 with 80-wide heads to `attn_kernel` in fp32 (there is no split-bf16 kernel for that
width) and ops.attention keeps `out_pair` off, so the out projection splits the fp32 rows itself.  Every GEMM of the mode still runs split-bf16."""
from types import SimpleNamespace

import torch

from . import ops, text
from .clipvision import _VISION_DEFAULTS, _VISION_FIELDS, HipCLIPVision

_OPENCLIP_VISION = dict(vith14=dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, projection_dim=1024, patch_size=14,
                                    image_size=224, hidden_act="gelu", layer_norm_eps=1e-5),
                        tiny14=dict(hidden_size=160, intermediate_size=640, num_hidden_layers=2, num_attention_heads=2, projection_dim=64, patch_size=14,
                                    image_size=56, hidden_act="gelu", layer_norm_eps=1e-5))


def openclip_vision_config(config="vith14"):
    """"vith14" (OpenCLIP ViT-H/14: width 1280, 32 layers, 16 heads of 80, MLP 5120, patch 14, image 224, projection 1024, erf-gelu) / "tiny14" (the test size:
    width 160, 2 heads of 80, 2 layers, MLP 640, image 56 = 17 tokens, projection 64), a CLIPVisionConfig, or a dict of its fields -> the fields the tower needs,
    checked.  Raises ValueError with the reason otherwise."""
    if isinstance(config, SimpleNamespace):
        return config
    if isinstance(config, str):
        if config not in _OPENCLIP_VISION:
            raise ValueError(f"OpenCLIP vision config {config!r} (one of {sorted(_OPENCLIP_VISION)})")
        config = _OPENCLIP_VISION[config]
    get = (lambda k: config.get(k, _VISION_DEFAULTS.get(k))) if isinstance(config, dict) else (lambda k: getattr(config, k, _VISION_DEFAULTS.get(k)))
    cfg = SimpleNamespace(**{k: get(k) for k in _VISION_FIELDS})
    missing = [k for k in _VISION_FIELDS if getattr(cfg, k) is None]
    if missing:
        raise ValueError(f"OpenCLIP vision config: missing {missing}")
    C, nh = cfg.hidden_size, cfg.num_attention_heads
    if C % nh != 0 or C // nh not in (64, 80):
        raise ValueError(f"OpenCLIP vision tower: head dim {C / nh:g} (hidden_size {C} / {nh} heads); the tower runs the attention kernels at head dim 64 or 80")
    if cfg.hidden_act not in ("gelu", "quick_gelu"):
        raise ValueError(f"OpenCLIP vision tower: hidden_act {cfg.hidden_act!r}; the GEMM epilogues carry 'gelu' and 'quick_gelu'")
    if cfg.image_size % cfg.patch_size != 0 or cfg.intermediate_size % 8 != 0 or cfg.projection_dim % 8 != 0:
        raise ValueError(f"OpenCLIP vision tower: image {cfg.image_size} / patch {cfg.patch_size}, MLP {cfg.intermediate_size}, projection {cfg.projection_dim}: "
                         "whole patches and multiples of 8 only")
    return cfg


class HipOpenCLIPVision(HipCLIPVision):
    """CLIPVisionModelWithProjection(pixel_values).image_embeds at an OpenCLIP configuration (module docstring) = open_clip's encode_image (unnormalised) on the
    HIP kernels.  forward: float [B, 3, image_size, image_size] (normalised) -> fp32 [B, projection_dim]; features_u8: decoded uint8 images of any one size ->
    the same, open_clip's validation transform on the device.  Everything but the configuration check and the pooled norm's entry is HipCLIPVision's."""
    _config = staticmethod(openclip_vision_config)

    def _pool(self, x):
        """post_layernorm of the class rows, gathered by the norm itself (`ffn_pool_layernorm`: ffn_layernorm's bits on x[:, 0], without the copy of the rows)"""
        return ops.pool_layernorm(x, None, *self.post, eps=self.config.layer_norm_eps, pair=self.x3)


def split_openclip_state(state):
    """a whole open_clip CLIP state dict -> (the `visual.*` entries, the rest).  The text tower's `transformer.resblocks.*` sit at the top level beside
    `visual.transformer.resblocks.*`: each tower must see its own only."""
    vis = {k: v for k, v in state.items() if k.startswith("visual.")}
    return vis, {k: v for k, v in state.items() if not k.startswith("visual.")}


def split_state(state):
    """`HPS_v2.1_compressed.pt`'s state_dict in open_clip's layout, or transformers' CLIPModel layout (vision_model.* / visual_projection.weight, text_model.* /
    text_projection.weight) -> (the image tower's state, the text tower's state)"""
    if any(k.startswith("visual.") for k in state):
        return split_openclip_state(state)
    vis = {k: v for k, v in state.items() if k.startswith(("vision_model.", "visual_projection."))}
    txt = {k: v for k, v in state.items() if k.startswith(("text_model.", "text_projection."))}
    return vis, txt


class HipHPSv2:
    """The score of human_preference_score.py:score on the HIP towers.  vision: a HipOpenCLIPVision; text: a text.HipCLIPTextWithProjection of the same
    projection width; tokenizer: callable(prompts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids, CLIP's BPE tokenizer
    (transformers.CLIPTokenizer) or text.ByteTokenizer in tests."""

    def __init__(self, vision, text, tokenizer):
        if vision.config.projection_dim != text.config.projection_dim:
            raise ValueError(f"HipHPSv2: image embeddings of {vision.config.projection_dim} and text embeddings of {text.config.projection_dim} values")
        self.vision, self.text, self.tokenizer = vision, text, tokenizer
        self.device = vision.device

    @classmethod
    def from_state(cls, state, tokenizer, vision_config="vith14", text_config="vith14", dtype=torch.float32, device="cuda:0", x3=False):
        """from one state dict holding both towers (split_state) and their configurations"""
        vis, txt = split_state(state)
        return cls(HipOpenCLIPVision(vision_config, vis, dtype=dtype, device=device, x3=x3),
                   text.HipCLIPTextWithProjection(text_config, txt, dtype=dtype, device=device, x3=x3), tokenizer)

    def text_features(self, prompts):
        """prompts (a str or a list) -> fp32 [N, projection_dim]"""
        ids = self.tokenizer([prompts] if isinstance(prompts, str) else list(prompts), padding="max_length", max_length=77, truncation=True,
                             return_tensors="pt").input_ids
        return self.text(ids)

    @torch.no_grad()
    def score_u8(self, images_u8, prompt):
        """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device), prompt: one str for all of them, or B of them -> fp32 [B] on the device:
        the cosine between each image's embedding and its prompt's"""
        f = self.vision.features_u8(images_u8).contiguous()
        t = self.text_features(prompt).contiguous()
        if t.shape[0] not in (1, f.shape[0]):
            raise ValueError(f"HipHPSv2: {t.shape[0]} prompts for {f.shape[0]} images (one, or one each)")
        return ops.cosine_rows(f, t)


def load_tokenizer(path):
    """"bytes" -> text.ByteTokenizer (tests); a folder with vocab.json and merges.txt -> transformers.CLIPTokenizer from those local files (CLIP's BPE, the
    tokenizer open_clip's get_tokenizer('ViT-H-14') implements; pad token id 0 as open_clip pads)"""
    if path == "bytes":
        return text.ByteTokenizer()
    import os
    from transformers import CLIPTokenizer
    vocab, merges = os.path.join(path, "vocab.json"), os.path.join(path, "merges.txt")
    for p in (vocab, merges):
        if not os.path.isfile(p):
            raise ValueError(f"--hps_tokenizer: {p} not found (a folder with vocab.json and merges.txt)")
    return CLIPTokenizer(vocab, merges, pad_token="!")          # "!" is id 0 of CLIP's vocabulary: open_clip pads with zeros
