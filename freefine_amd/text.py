"""Text conditioning for the hot path.

The reference tokenises with CLIP and calls `self.text_encoder(ids)[0]` (/root/reference/src/demo/model.py:536-567, 842-848).
No CLIP weights exist in this environment, so synthetic runs use a deterministic byte-level stand-in with the same
interface pair (tokenizer(prompts, padding=..., max_length=77, return_tensors="pt").input_ids ; text_encoder(ids)[0]
-> [N,77,D]).  A real HF tokenizer/text-encoder pair can be plugged into FreeFinePipeline unchanged.

HipCLIPTextEncoder (below) is the same interface on the project's own kernels: transformers' CLIPTextModel arithmetic without a library GEMM; its layers are
encoder.py's block.  HipCLIPTextWithProjection adds pooling and the projection (CLIPTextModelWithProjection = open_clip's encode_text): the text half of
the Human Preference Score (hps.py).
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import encoder, ops


class ByteTokenizer:
    model_max_length = 77

    def __call__(self, prompts, padding="max_length", max_length=77, return_tensors="pt", **kw):
        if isinstance(prompts, str):
            prompts = [prompts]
        ids = np.zeros((len(prompts), max_length), dtype=np.int64)
        for i, p in enumerate(prompts):
            b = list(p.encode("utf-8"))[: max_length - 2]
            ids[i, 0] = 257                      # BOS
            ids[i, 1:1 + len(b)] = np.asarray(b, dtype=np.int64) + 1
            ids[i, 1 + len(b)] = 258             # EOS, then 0-padding
        return SimpleNamespace(input_ids=torch.from_numpy(ids))


class SyntheticTextEncoder:
    """ids [N,77] -> ([N,77,D],): seeded token table + position table, unit-RMS rows.  Host side, fp32, deterministic."""

    def __init__(self, dim, seed=1234, device="cpu"):
        rng = np.random.default_rng(seed)
        self.table = torch.from_numpy(rng.standard_normal((259, dim)).astype(np.float32))
        self.pos = torch.from_numpy((0.3 * rng.standard_normal((77, dim))).astype(np.float32))
        self.device = torch.device(device)
        self.dim = dim

    def to(self, device):
        self.device = torch.device(device)
        return self

    def __call__(self, input_ids):
        ids = input_ids.cpu()
        e = self.table[ids] + self.pos[None, : ids.shape[1]]
        e = e / e.pow(2).mean(dim=-1, keepdim=True).sqrt()
        return (e.to(self.device),)


def make_text_embed(tokenizer, text_encoder):
    """callable(list[str]) -> [N,77,D], the form the oracle consumes."""
    def f(prompts):
        return text_encoder(tokenizer(prompts, padding="max_length", max_length=77, return_tensors="pt").input_ids)[0]
    return f


def clip_shaped_text_encoder(dim, seed=1234, layers=None):
    """A REAL-SIZE text encoder for synthetic runs (bench.py): transformers' CLIPTextModel built from a config of the checkpoint's shape --
    SD-2.1's OpenCLIP ViT-H text tower (width 1024, 23 layers = the penultimate-layer output the checkpoint ships, 16 heads, MLP 4096, gelu),
    SD-1.x's CLIP ViT-L (768, 12 layers, 12 heads, 3072, quick_gelu) -- with seeded random weights (no checkpoints exist offline), so that the
    text side of an edit costs what it costs with a checkpoint.  torch module: FreeFinePipeline moves it to its device on first use."""
    from transformers import CLIPTextConfig, CLIPTextModel
    if dim == 1024:
        cfg = CLIPTextConfig(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=layers or 23, num_attention_heads=16,
                             max_position_embeddings=77, hidden_act="gelu", projection_dim=1024)
    else:
        cfg = CLIPTextConfig(vocab_size=49408, hidden_size=dim, intermediate_size=4 * dim, num_hidden_layers=layers or 12,
                             num_attention_heads=max(1, dim // 64), max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=dim)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    enc = CLIPTextModel(cfg).eval()
    torch.random.set_rng_state(state)
    for q in enc.parameters():
        q.requires_grad_(False)
    return enc


# ---------------------------------------------------------------------------------------------------------------------
# the CLIP text tower on the project's own kernels
# ---------------------------------------------------------------------------------------------------------------------
_TEXT_DEFAULTS = dict(hidden_act="quick_gelu", layer_norm_eps=1e-5, max_position_embeddings=77)      # transformers' CLIPTextConfig defaults
_TEXT_FIELDS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings", "hidden_act",
                "layer_norm_eps")
TEXT_MAX_POSITIONS = 96            # the causal attention kernel holds a sequence's keys in six 16-key fragments


def text_config(config):
    """a CLIPTextConfig, or the dict of a checkpoint's text_encoder/config.json -> the fields the tower needs, checked: head dim 64 (the causal attention kernel's),
    quick_gelu (CLIP ViT-L, SD-1.x) or erf-gelu (OpenCLIP ViT-H, SD-2.1) MLP.  Raises ValueError with the reason otherwise."""
    get = (lambda k: config.get(k, _TEXT_DEFAULTS.get(k))) if isinstance(config, dict) else (lambda k: getattr(config, k, _TEXT_DEFAULTS.get(k)))
    cfg = SimpleNamespace(**{k: get(k) for k in _TEXT_FIELDS})
    missing = [k for k in _TEXT_FIELDS if getattr(cfg, k) is None]
    if missing:
        raise ValueError(f"text encoder config: missing {missing}")
    C, nh = cfg.hidden_size, cfg.num_attention_heads
    if C % nh != 0 or C // nh != 64:
        raise ValueError(f"text encoder: head dim {C / nh:g} (hidden_size {C} / {nh} heads); the causal attention kernel is built for head dim 64")
    if cfg.hidden_act not in ("quick_gelu", "gelu"):
        raise ValueError(f"text encoder: hidden_act {cfg.hidden_act!r}; the GEMM epilogues carry 'quick_gelu' and 'gelu'")
    if cfg.intermediate_size % 8 != 0:
        raise ValueError(f"text encoder: intermediate_size {cfg.intermediate_size} must be a multiple of 8")
    return cfg


def pack_text_state(cfg, state):
    """CLIPTextModel parameters (names with or without the hub files' `text_model.` prefix; `text_projection` and `position_ids` ignored) -> the fp32 host tensors
    the tower uploads, the layers in the packing of encoder.py: q | k rows of one GEMM, V apart (its GEMM writes V^T).  Missing or mis-shaped parameters raise
    ValueError."""
    st = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state.items()}
    C = cfg.hidden_size
    want = {"embeddings.token_embedding.weight": (cfg.vocab_size, C), "embeddings.position_embedding.weight": (cfg.max_position_embeddings, C),
            "final_layer_norm.weight": (C,), "final_layer_norm.bias": (C,)}
    want.update(encoder.clip_layer_shapes(cfg))
    bad = [k for k, s in want.items() if k not in st or tuple(st[k].shape) != s]
    if bad:
        raise ValueError(f"text encoder state: missing or mis-shaped parameters {bad[:4]}{' ...' if len(bad) > 4 else ''}")
    f = lambda k: st[k].detach().float().cpu().contiguous()
    out = {"tok": f("embeddings.token_embedding.weight"), "pos": f("embeddings.position_embedding.weight"),
           "lnf.w": f("final_layer_norm.weight"), "lnf.b": f("final_layer_norm.bias")}
    return encoder.pack_clip_layers(cfg, f, out)


class NativeTextSpec:
    """what FreeFinePipeline.components reads from <path>/text_encoder for native_text=True: the checked config and the host state, no executor yet (the
    pipeline's mode and device are from_pretrained's business) -- so the loading path runs without a GPU"""

    def __init__(self, path):
        from .weights import load_safetensors_dir
        cfg, self.state = load_safetensors_dir(path, "text_encoder")
        self.config = text_config(cfg)

    def build(self, dtype=torch.float32, device="cuda:0", x3=False):
        return HipCLIPTextEncoder(self.config, self.state, dtype=dtype, device=device, x3=x3)


class HipCLIPTextEncoder:
    """transformers' CLIPTextModel (`self.text_encoder(ids)[0]`, /root/reference/src/demo/model.py:536-567, 842-848) on the HIP kernels: the layers are
    encoder.py's block (every Linear an `ffn_igemm`: q | k in one GEMM, V^T from a transposed-output GEMM, residuals and the MLP activation in the epilogues;
    LayerNorm `ffn_layernorm`) with the causal self attention (`ffn_attn` with FFN_ATT_CAUSAL), the token + position lookup is `ffn_embed_tokens`.

        x = tok[ids] + pos;  per layer: y = LN1(x); q, k, v = Linear(y); a = softmax(q k^T / 8 + causal) v per head; x += out_proj(a);
        y = LN2(x); x += fc2(act(fc1(y)));  result final_layer_norm(x)                         (no padding mask: the reference passes none)

    dtype float32 = parity mode (exact-fp32 MFMA), float32 with x3 = split-bf16, bfloat16 = fast mode.  The result is fp32 [N, S, C] on the device.

    BIT-IDENTICAL PER PROMPT.  Tile choice and the bf16 tuner key on M, so prompts run in groups of GROUP rows (the last group zero-padded; rows are independent
    in every op) with split-K off: a prompt's embedding does not depend on what is encoded beside it, and FreeFinePipeline._encode_text can hand all missing
    prompts over in one call.  M = 77 * GROUP = 308 keeps the 192- and 256-row tiles eligible."""
    GROUP = 4

    def __init__(self, config, state, dtype=torch.float32, device="cuda:0", x3=False):
        encoder.check_mode(dtype, x3)
        self.config = config if isinstance(config, SimpleNamespace) else text_config(config)
        self.dtype, self.device, self.x3 = dtype, torch.device(device), bool(x3)
        self.host = pack_text_state(self.config, state)
        up = lambda k: self.host[k].to(self.device)
        self.tok, self.pos, self.lnf = up("tok"), up("pos"), (up("lnf.w"), up("lnf.b"))
        self.blocks = encoder.clip_blocks(self.config, self.host, self.device, dtype, self.x3)

    @classmethod
    def from_torch(cls, module, dtype=torch.float32, device="cuda:0", x3=False):
        """from a transformers CLIPTextModel (its config and state_dict)"""
        return cls(module.config, module.state_dict(), dtype=dtype, device=device, x3=x3)

    @classmethod
    def from_folder(cls, path, dtype=torch.float32, device="cuda:0", x3=False):
        """from <path>/text_encoder/{config.json, *.safetensors} of a HF-layout Stable-Diffusion folder; no transformers model class is built"""
        return NativeTextSpec(path).build(dtype=dtype, device=device, x3=x3)

    def to(self, *a, **k):
        return self

    def _stream(self, ids):
        """ids int32 [GROUP, S] on the device -> the residual stream behind the last layer [GROUP, S, C] in the activation type (before final_layer_norm)"""
        cfg = self.config
        eps, act = cfg.layer_norm_eps, {"quick_gelu": "qgelu", "gelu": "gelu"}[cfg.hidden_act]
        x = ops.embed_tokens(ids, self.tok, self.pos, self.dtype)
        vt = encoder.vt_buffer(x)
        for b in self.blocks:
            x = encoder.run_block(b, x, vt, heads=cfg.num_attention_heads, eps=eps, act=act, hidden=cfg.intermediate_size, x3=self.x3, causal=True, splitk=1)
        return x

    def _group(self, ids):
        """ids int32 [GROUP, S] on the device -> final_layer_norm output [GROUP, S, C] in the activation type"""
        return ops.layernorm(self._stream(ids), *self.lnf, eps=self.config.layer_norm_eps)

    def _run_groups(self, input_ids, attention_mask, kw):
        """the checks of __call__, then _group over the prompts in groups of GROUP (the last one zero-padded) -> (its outputs cut to the real rows, N, S)"""
        name = type(self).__name__
        if attention_mask is not None:
            raise ValueError(f"{name} takes no attention_mask (the reference passes none: padding tokens attend like any other)")
        if kw:
            raise ValueError(f"{name}: unsupported arguments {sorted(kw)}")
        ids = torch.as_tensor(input_ids)
        if ids.ndim == 1:
            ids = ids[None]
        N, S = ids.shape
        cfg = self.config
        if S > TEXT_MAX_POSITIONS or S > cfg.max_position_embeddings:
            raise ValueError(f"{name}: {S} positions requested (at most {min(TEXT_MAX_POSITIONS, cfg.max_position_embeddings)})")
        if not ids.is_cuda:
            if N and (int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab_size):
                raise ValueError(f"{name}: token ids outside [0, {cfg.vocab_size})")
        ids = ids.to(self.device, torch.int32)
        P, outs = self.GROUP, []
        for g0 in range(0, N, P):
            grp = ids[g0:g0 + P]
            n = grp.shape[0]
            if n < P:
                grp = torch.cat([grp, torch.zeros(P - n, S, dtype=torch.int32, device=self.device)])
            outs.append(self._group(grp.contiguous())[:n])
        return outs, N, S

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, **kw):
        """input_ids [N, S] (S <= 96 and <= max_position_embeddings) -> (last_hidden_state fp32 [N, S, C] on the device,).  Host ids are range-checked before upload;
        device ids are taken as checked by whoever uploaded them (no synchronisation: the call is capturable; the lookup kernel reads no row outside the table)."""
        outs, N, S = self._run_groups(input_ids, attention_mask, kw)
        out = torch.cat(outs) if outs else torch.empty(0, S, self.config.hidden_size, device=self.device)
        return (out.float(),)


# ---------------------------------------------------------------------------------------------------------------------
# the text tower that pools and projects (CLIPTextModelWithProjection = open_clip's encode_text)
# ---------------------------------------------------------------------------------------------------------------------
_TEXT_H14 = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, max_position_embeddings=77,
                 hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=1024)               # OpenCLIP ViT-H/14's text tower
_TEXT_TINY = dict(vocab_size=259, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
                  hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=64)                # the test size; 259 = ByteTokenizer's ids


def text_projection_config(config="vith14"):
    """"vith14" (OpenCLIP ViT-H/14's text tower: width 1024, 24 layers, 16 heads, MLP 4096, gelu, projection 1024) / "tiny" (the test size, ByteTokenizer's
    vocabulary), a CLIPTextConfig or a dict of its fields -> text_config's checked fields plus projection_dim.  Raises ValueError with the reason otherwise."""
    if isinstance(config, SimpleNamespace):
        return config
    if isinstance(config, str):
        if config not in ("vith14", "tiny"):
            raise ValueError(f"text tower config {config!r} (one of ['tiny', 'vith14'])")
        config = _TEXT_H14 if config == "vith14" else _TEXT_TINY
    cfg = text_config(config)
    cfg.projection_dim = config.get("projection_dim") if isinstance(config, dict) else getattr(config, "projection_dim", None)
    if not isinstance(cfg.projection_dim, int) or cfg.projection_dim <= 0 or cfg.projection_dim % 8 != 0:
        raise ValueError(f"text tower: projection_dim {cfg.projection_dim!r} must be a positive multiple of 8")
    return cfg


def transformers_text_config(cfg, **kw):
    """the CLIPTextConfig of a checked configuration (tests and tools build the yardstick module from it)"""
    from transformers import CLIPTextConfig
    return CLIPTextConfig(**{k: getattr(cfg, k) for k in _TEXT_FIELDS + ("projection_dim",)}, **kw)


def text_param_shapes(cfg, prefix=""):
    """name -> shape of CLIPTextModelWithProjection.state_dict() (`prefix` = "text_model." as the module spells it; text_projection carries none)"""
    C, q = cfg.hidden_size, prefix
    sh = {q + "embeddings.token_embedding.weight": (cfg.vocab_size, C), q + "embeddings.position_embedding.weight": (cfg.max_position_embeddings, C)}
    sh.update(encoder.clip_layer_shapes(cfg, q))
    sh.update({q + "final_layer_norm.weight": (C,), q + "final_layer_norm.bias": (C,), "text_projection.weight": (cfg.projection_dim, C)})
    return sh


def synthetic_text_state(cfg, seed=0):
    """seeded random weights of a plausible scale in transformers' layout (with the `text_model.` prefix): for tests and benchmarks without a checkpoint"""
    return encoder.draw_state(text_param_shapes(cfg, "text_model."), seed)


_RESBLOCK = (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2"))


def to_openclip_text_layout(state, layers):
    """transformers' names -> open_clip's text names: the inverse of _openclip_text_to_transformers, for tests of that mapping (the same published layout read
    the other way, no independent evidence)"""
    st = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state.items()}
    out = {"positional_embedding": st["embeddings.position_embedding.weight"], "token_embedding.weight": st["embeddings.token_embedding.weight"],
           "ln_final.weight": st["final_layer_norm.weight"], "ln_final.bias": st["final_layer_norm.bias"],
           "text_projection": st["text_projection.weight"].t().contiguous()}
    for i in range(layers):
        r, p = f"transformer.resblocks.{i}.", f"encoder.layers.{i}."
        out[r + "attn.in_proj_weight"] = torch.cat([st[p + f"self_attn.{n}.weight"] for n in ("q_proj", "k_proj", "v_proj")], 0)
        out[r + "attn.in_proj_bias"] = torch.cat([st[p + f"self_attn.{n}.bias"] for n in ("q_proj", "k_proj", "v_proj")], 0)
        for a, b in _RESBLOCK:
            out[r + a + ".weight"], out[r + a + ".bias"] = st[p + b + ".weight"], st[p + b + ".bias"]
    return out


def _openclip_text_to_transformers(st, layers):
    """open_clip's text names (open_clip/model.py CLIP: the text tower's parameters sit at the top level of the checkpoint, beside `visual.*`) -> transformers'
    names.  Written from the published layout -- positional_embedding, token_embedding.weight, transformer.resblocks.N.{ln_1, attn.in_proj_{weight,bias}
    (q | k | v rows), attn.out_proj, ln_2, mlp.c_fc, mlp.c_proj}, ln_final, text_projection stored [width, projection] (applied as x @ text_projection) -- and
    PINNED TO NOTHING: the `open_clip` package is on no machine this project is tested on.  `visual.*`, `attn_mask` and `logit_scale` are ignored."""
    out = {"embeddings.position_embedding.weight": st["positional_embedding"], "embeddings.token_embedding.weight": st["token_embedding.weight"],
           "final_layer_norm.weight": st["ln_final.weight"], "final_layer_norm.bias": st["ln_final.bias"], "text_projection.weight": st["text_projection"].t()}
    for i in range(layers):
        r, p = f"transformer.resblocks.{i}.", f"encoder.layers.{i}."
        C = st[r + "attn.in_proj_weight"].shape[1]
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            out[p + f"self_attn.{n}.weight"] = st[r + "attn.in_proj_weight"][j * C:(j + 1) * C]
            out[p + f"self_attn.{n}.bias"] = st[r + "attn.in_proj_bias"][j * C:(j + 1) * C]
        for a, b in _RESBLOCK:
            out[p + b + ".weight"], out[p + b + ".bias"] = st[r + a + ".weight"], st[r + a + ".bias"]
    return out


def pack_text_projection_state(cfg, state):
    """CLIPTextModelWithProjection.state_dict() (names with or without `text_model.`), or open_clip's names (see _openclip_text_to_transformers) -> pack_text_state's
    host tensors plus "proj.w" [projection, width].  Missing or mis-shaped parameters raise ValueError naming them."""
    if "token_embedding.weight" in state or "positional_embedding" in state:
        try:
            state = _openclip_text_to_transformers(state, cfg.num_hidden_layers)
        except KeyError as e:
            raise ValueError(f"text encoder state (open_clip layout): missing parameter {e.args[0]!r}") from None
    out = pack_text_state(cfg, state)
    w = state.get("text_projection.weight")
    if w is None or tuple(w.shape) != (cfg.projection_dim, cfg.hidden_size):
        raise ValueError(f"text encoder state: missing or mis-shaped parameters ['text_projection.weight'] (wanted {(cfg.projection_dim, cfg.hidden_size)})")
    out["proj.w"] = w.detach().float().cpu().contiguous()
    return out


class HipCLIPTextWithProjection(HipCLIPTextEncoder):
    """transformers' CLIPTextModelWithProjection(ids).text_embeds = open_clip's encode_text on the HIP kernels: HipCLIPTextEncoder's embedding and blocks, then

        row = x[n, first position of max(ids[n])];  result final_layer_norm(row) W_proj^T  (no bias)  -> fp32 [N, projection_dim]

    POOLING is open_clip's rule (text_global_pool 'argmax': the end-of-text token has the largest id of CLIP's vocabulary); transformers uses the same rule when
    eos_token_id == 2 (its legacy configs) and "first position of eos_token_id" otherwise -- the same row whenever end-of-text is the largest id present.  The
    norm runs on the pooled row alone (`ffn_pool_layernorm`: LayerNorm is per row, so this is final_layer_norm(x)[n, pos] bit for bit), the projection is an
    `ffn_igemm` over the GROUP rows with split-K off: like the encoder's, a prompt's embedding does not depend on what is encoded beside it."""

    def __init__(self, config, state, dtype=torch.float32, device="cuda:0", x3=False):
        encoder.check_mode(dtype, x3)
        self.config = text_projection_config(config)
        self.dtype, self.device, self.x3 = dtype, torch.device(device), bool(x3)
        self.host = pack_text_projection_state(self.config, state)
        up = lambda k: self.host[k].to(self.device)
        self.tok, self.pos, self.lnf = up("tok"), up("pos"), (up("lnf.w"), up("lnf.b"))
        self.blocks = encoder.clip_blocks(self.config, self.host, self.device, dtype, self.x3)
        self.proj = ops.pack_linear(up("proj.w"), dtype, x3=self.x3)

    @classmethod
    def from_folder(cls, path, dtype=torch.float32, device="cuda:0", x3=False):
        raise NotImplementedError("HipCLIPTextWithProjection is built from a config and a state dict")

    def _group(self, ids):
        """ids int32 [GROUP, S] on the device -> text_embeds [GROUP, projection_dim] in the GEMM's output type"""
        cfg = self.config
        pooled = ops.pool_layernorm(self._stream(ids), ids, *self.lnf, eps=cfg.layer_norm_eps, pair=self.x3)
        return ops.linear(pooled, self.proj, None, K=cfg.hidden_size, splitk=1)

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, **kw):
        """input_ids [N, S] (S <= 96 and <= max_position_embeddings; checked like HipCLIPTextEncoder's) -> text_embeds fp32 [N, projection_dim] on the device"""
        outs, N, S = self._run_groups(input_ids, attention_mask, kw)
        out = torch.cat(outs) if outs else torch.empty(0, self.config.projection_dim, device=self.device)
        return out.float()
