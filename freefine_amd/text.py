"""Text conditioning for the hot path.

The reference tokenises with CLIP and calls `self.text_encoder(ids)[0]` (/root/reference/src/demo/model.py:536-567, 842-848).
No CLIP weights exist in this environment, so synthetic runs use a deterministic byte-level stand-in with the same
interface pair (tokenizer(prompts, padding=..., max_length=77, return_tensors="pt").input_ids ; text_encoder(ids)[0]
-> [N,77,D]).  A real HF tokenizer/text-encoder pair can be plugged into FreeFinePipeline unchanged.

HipCLIPTextEncoder (below) is the same interface on the project's own kernels: transformers' CLIPTextModel arithmetic without a library GEMM; its layers are
encoder.py's block.
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

    def _group(self, ids):
        """ids int32 [GROUP, S] on the device -> final_layer_norm output [GROUP, S, C] in the activation type"""
        cfg = self.config
        eps, act = cfg.layer_norm_eps, {"quick_gelu": "qgelu", "gelu": "gelu"}[cfg.hidden_act]
        x = ops.embed_tokens(ids, self.tok, self.pos, self.dtype)
        vt = encoder.vt_buffer(x)
        for b in self.blocks:
            x = encoder.run_block(b, x, vt, heads=cfg.num_attention_heads, eps=eps, act=act, hidden=cfg.intermediate_size, x3=self.x3, causal=True, splitk=1)
        return ops.layernorm(x, *self.lnf, eps=eps)

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, **kw):
        """input_ids [N, S] (S <= 96 and <= max_position_embeddings) -> (last_hidden_state fp32 [N, S, C] on the device,).  Host ids are range-checked before upload;
        device ids are taken as checked by whoever uploaded them (no synchronisation: the call is capturable; the lookup kernel reads no row outside the table)."""
        if attention_mask is not None:
            raise ValueError("HipCLIPTextEncoder takes no attention_mask (the reference passes none: padding tokens attend like any other)")
        if kw:
            raise ValueError(f"HipCLIPTextEncoder: unsupported arguments {sorted(kw)}")
        ids = torch.as_tensor(input_ids)
        if ids.ndim == 1:
            ids = ids[None]
        N, S = ids.shape
        cfg = self.config
        if S > TEXT_MAX_POSITIONS or S > cfg.max_position_embeddings:
            raise ValueError(f"HipCLIPTextEncoder: {S} positions requested (at most {min(TEXT_MAX_POSITIONS, cfg.max_position_embeddings)})")
        if not ids.is_cuda:
            if N and (int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab_size):
                raise ValueError(f"HipCLIPTextEncoder: token ids outside [0, {cfg.vocab_size})")
        ids = ids.to(self.device, torch.int32)
        P, outs = self.GROUP, []
        for g0 in range(0, N, P):
            grp = ids[g0:g0 + P]
            n = grp.shape[0]
            if n < P:
                grp = torch.cat([grp, torch.zeros(P - n, S, dtype=torch.int32, device=self.device)])
            outs.append(self._group(grp.contiguous())[:n])
        out = torch.cat(outs) if outs else torch.empty(0, S, cfg.hidden_size, device=self.device)
        return (out.float(),)
