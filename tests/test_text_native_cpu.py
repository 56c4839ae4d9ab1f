"""CPU: the native CLIP text tower (freefine_amd.text.HipCLIPTextEncoder) as far as it runs without a device -- the ABI additions it needs, an fp64
restatement of the tower's arithmetic checked against transformers' CLIPTextModel.double() (the class the reference calls,
/root/reference/src/demo/model.py:536-567), the same restatement in emulated split-bf16 and bf16 arithmetic (tests/test_text_native_gpu.py derives its
bounds from them), loading from a checkpoint folder, and every refusal."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PROMPTS = ["a photo of a cup", "", "a very long prompt " + "with many more words than the seventy seven positions of the text tower can hold " * 6]


# ---------------------------------------------------------------------------------------------------------------------
# the tower restated (test-local; fp64 sums everywhere)
# ---------------------------------------------------------------------------------------------------------------------
def _bf16(x):
    return x.float().to(torch.bfloat16).double()


def _split(x):
    """fp32 value -> (hi, lo) as the FFN_BF16X3 kernels carry it"""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    return hi.double(), (x - hi).to(torch.bfloat16).double()


def _mm(a, w, mode):
    """a @ w^T over the last axes in the product arithmetic of `mode`: f64 exact; x3 = hi.hi + hi.lo + lo.hi of the fp32-rounded operands; bf16 = bf16-rounded operands"""
    wt = w.transpose(-1, -2)
    if mode == "f64":
        return a @ wt
    if mode == "bf16":
        return _bf16(a) @ _bf16(wt)
    ah, al = _split(a)
    wh, wl = _split(wt)
    return al @ wh + ah @ wl + ah @ wh


def _store(x, mode):
    """what an activation keeps between two ops: fp64 / fp32 (split-bf16 mode stores fp32) / bf16"""
    return x if mode == "f64" else (x.float().double() if mode == "x3" else _bf16(x))


def unprefixed(state):
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state.items()}


def tower_ref(cfg, state, ids, mode="f64"):
    """CLIPTextModel(ids)[0] restated: x = tok[ids] + pos; per layer y = LN1(x); q, k, v = Linear(y); a = softmax(q k^T 64^-0.5 + causal) v per head; x += out_proj(a);
    y = LN2(x); x += fc2(act(fc1(y))); final_layer_norm(x).  ids [N, S] int64 -> [N, S, C] fp64.  mode: "f64", or the emulated arithmetic of a device mode
    ("x3": split-bf16 products, fp32 storage; "bf16": bf16 products and storage; sums in fp64 in both)."""
    st = {k: v.double() for k, v in unprefixed(state).items()}
    C, nh, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    N, S = ids.shape
    ln = lambda x, p: torch.nn.functional.layer_norm(x, (C,), st[p + ".weight"], st[p + ".bias"], eps)
    lin = lambda x, p: _mm(x, st[p + ".weight"], mode) + st[p + ".bias"]
    act = (lambda x: x * torch.sigmoid(1.702 * x)) if cfg.hidden_act == "quick_gelu" else torch.nn.functional.gelu
    keep = lambda x: _store(x, mode)
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    x = keep(st["embeddings.token_embedding.weight"][ids] + st["embeddings.position_embedding.weight"][:S])
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        y = keep(ln(x, p + "layer_norm1"))
        heads = lambda t: t.view(N, S, nh, 64).transpose(1, 2)
        q, k, v = (heads(keep(lin(y, p + "self_attn." + n))) for n in ("q_proj", "k_proj", "v_proj"))
        s = (_mm(q, k, mode) * 0.125).masked_fill(~causal, float("-inf"))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        a = _mm(e, v.transpose(-1, -2), mode) / e.sum(-1, keepdim=True)         # the kernels normalise after the second product
        a = keep(a.transpose(1, 2).reshape(N, S, C))
        x = keep(x + lin(a, p + "self_attn.out_proj"))
        y = keep(ln(x, p + "layer_norm2"))
        h = keep(act(lin(y, p + "mlp.fc1")))
        x = keep(x + lin(h, p + "mlp.fc2"))
    return keep(ln(x, "final_layer_norm"))


def scale_err(a, b):
    """max |a - b| over the output maximum of b"""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def clip_tokens(prompts, vocab=49408, S=77):
    """deterministic stand-in for the CLIP tokenizer at a real vocabulary (no tokenizer files exist offline): BOS, one id per character, EOS, EOS padding;
    truncated to S positions like padding='max_length', truncation=True"""
    ids = torch.full((len(prompts), S), vocab - 1, dtype=torch.int64)
    for i, p in enumerate(prompts):
        body = [(ord(c) * 7919 + 13 * j) % (vocab - 2) for j, c in enumerate(p)][: S - 2]
        ids[i, 0] = vocab - 2
        ids[i, 1:1 + len(body)] = torch.tensor(body, dtype=torch.int64)
    return ids


# ---------------------------------------------------------------------------------------------------------------------
def test_abi_additions_are_declared_bound_and_exported():
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    assert re.search(r"\bFFN_ATT_CAUSAL\s*=\s*8\b", header) and _lib.ATT_CAUSAL == 8
    assert re.search(r"\bFFN_IG_OUT_QGELU\s*=\s*1\s*<<\s*8\b", header) and _lib.IG_OUT_QGELU == 256
    assert re.search(r"\bint\s+ffn_embed_tokens\s*\(", header) and "ffn_embed_tokens" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ffn_embed_tokens") and lib.ffn_version() >= 2
    # validation runs before any launch: no device needed
    assert lib.ffn_embed_tokens(None, 0, None, None, None, None, 77, 77, 64, 100) == -22 and b"embed_tokens" in lib.ffn_last_error()
    d = _lib.IgemmDesc()
    d.A = d.W = d.out = 0x10000
    d.M, d.N, d.K, d.Kpad, d.lda, d.ldo, d.rows_per_batch, d.alpha, d.splitk = 308, 256, 64, 64, 64, 256, 308, 1.0, 1
    d.flags = _lib.IG_OUT_QGELU | _lib.IG_OUT_GELU
    assert lib.ffn_igemm(None, 0, ctypes.byref(d)) == -22 and b"exclusive" in lib.ffn_last_error()
    d.flags = _lib.IG_OUT_QGELU | _lib.IG_OUT_TRANSPOSED
    assert lib.ffn_igemm(None, 0, ctypes.byref(d)) == -22 and b"transposed" in lib.ffn_last_error()


def attn_desc(S=77, Sk=77, D=64, heads=12, Bo=3, npass=1, kv_pair=0, flags=8, kmask=0, wq=0, w_slope=0.0):
    from freefine_amd import _lib
    d = _lib.AttnDesc()
    d.Bo, d.S, d.Sk, d.heads, d.D, d.npass, d.kv_pair, d.scale = Bo, S, Sk, heads, D, npass, kv_pair, 0.125
    d.ldq = d.ldk = d.ldo = heads * D
    d.ldvt = (Sk + 7) // 8 * 8
    for p in range(npass):
        for b in range(Bo):
            e = d.e[p * _lib.ATT_MAXB + b]
            e.q_row = e.kv_row = b
            e.w_const, e.w_slope, e.flags, e.kmask, e.wq = 1.0, w_slope, flags, kmask, wq
    return d


def kernel_name(dtype, d):
    from freefine_amd import _lib
    buf = ctypes.create_string_buffer(160)
    rc = _lib.load().ffn_attn_kernel_name(dtype, ctypes.byref(d), buf, 160)
    return buf.value.decode() if rc == 0 else rc


def test_causal_plan_names_its_kernel_and_refuses_everything_else():
    from freefine_amd import _lib
    lib = _lib.load()
    want = {_lib.FFN_F32: "void attn_causal_kernel<float, false>(ffn_attn_desc)", _lib.FFN_BF16: "void attn_causal_kernel<bf16, false>(ffn_attn_desc)",
            _lib.FFN_BF16X3: "void attn_causal_kernel<float, true>(ffn_attn_desc)"}
    for dtype, name in want.items():
        for S in (1, 16, 33, 77, 96):
            assert kernel_name(dtype, attn_desc(S=S, Sk=S)) == name
        bad = [attn_desc(S=64, Sk=77), attn_desc(S=128, Sk=128), attn_desc(kmask=0x10000), attn_desc(npass=2), attn_desc(kv_pair=1), attn_desc(D=40),
               attn_desc(wq=0x10000), attn_desc(w_slope=0.5)]
        mixed = attn_desc()
        mixed.e[1].flags = 0                           # an active entry without the flag beside flagged ones
        for d in bad + [mixed]:
            assert kernel_name(dtype, d) == -22 and b"FFN_ATT_CAUSAL" in lib.ffn_last_error(), lib.ffn_last_error()
        # without the flag the plan is what it was (names the existing tests pin)
        plain = kernel_name(dtype, attn_desc(flags=0))
        assert plain == {_lib.FFN_F32: "void attn_kernel<float, 64, 2, 64, 1, true>(ffn_attn_desc)", _lib.FFN_BF16: "void xattn_kernel<5>(ffn_attn_desc, int, int)",
                         _lib.FFN_BF16X3: "void xattn_x3_kernel<5, 4>(ffn_attn_desc, int, int)"}[dtype], plain


@pytest.mark.parametrize("dim,layers", [(1024, 2), (768, 2)])
def test_restatement_equals_cliptextmodel_fp64(dim, layers):
    from freefine_amd.text import clip_shaped_text_encoder, text_config
    enc = clip_shaped_text_encoder(dim, layers=layers).double()
    cfg = text_config(enc.config)
    assert cfg.hidden_act == ("gelu" if dim == 1024 else "quick_gelu") and cfg.hidden_size // cfg.num_attention_heads == 64
    ids = clip_tokens(PROMPTS)
    with torch.no_grad():
        want = enc(ids)[0]
    got = tower_ref(cfg, enc.state_dict(), ids)
    e = scale_err(got, want)
    print(f"restatement vs CLIPTextModel.double() ({dim}/{layers}): {e:.2e}")
    assert e <= 1e-12
    # the emulated device arithmetics are the same tower, off by what their number formats cost
    ex, eb = scale_err(tower_ref(cfg, enc.state_dict(), ids, "x3"), want), scale_err(tower_ref(cfg, enc.state_dict(), ids, "bf16"), want)
    print(f"  emulated split-bf16 {ex:.2e}, bf16 {eb:.2e}")
    assert 0 < ex < 1e-4 and ex < eb < 5e-2


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    import make_synthetic_checkpoint as msc
    out = {}
    for name, kw in (("quick", dict(text_heads=1)), ("gelu", dict(text_heads=1, text_act="gelu")), ("d32", dict())):
        p = str(tmp_path_factory.mktemp(name))
        msc.write(p, "tiny", "tiny", **kw)
        out[name] = p
    return out


def test_synthetic_checkpoint_defaults_are_unchanged(folders, tmp_path):
    """text_heads / text_act default to today's folder: width // 32 heads, the config's default activation"""
    import json
    cfg = json.load(open(os.path.join(folders["d32"], "text_encoder", "config.json")))
    assert cfg["num_attention_heads"] == cfg["hidden_size"] // 32 and cfg["hidden_act"] == "quick_gelu"
    q = json.load(open(os.path.join(folders["quick"], "text_encoder", "config.json")))
    g = json.load(open(os.path.join(folders["gelu"], "text_encoder", "config.json")))
    assert q["num_attention_heads"] == g["num_attention_heads"] == 1 and q["hidden_act"] == "quick_gelu" and g["hidden_act"] == "gelu"
    assert {k: v for k, v in q.items() if k != "num_attention_heads"} == {k: v for k, v in cfg.items() if k != "num_attention_heads"}


def test_from_folder_packs_the_same_with_and_without_prefix(folders):
    from transformers import CLIPTextModel
    from freefine_amd.text import HipCLIPTextEncoder, pack_text_state, text_config
    from freefine_amd.weights import load_safetensors_dir
    for name in ("quick", "gelu"):
        enc = HipCLIPTextEncoder.from_folder(folders[name], device="cpu")
        assert enc.config.hidden_size == 64 and enc.config.intermediate_size == 128 and enc.config.hidden_act == ("quick_gelu" if name == "quick" else "gelu")
        assert enc.to("cpu") is enc
        cfgd, st = load_safetensors_dir(folders[name], "text_encoder")
        bare = unprefixed(st)
        pref = {"text_model." + k: v for k, v in bare.items()}
        pref["text_projection.weight"] = torch.zeros(4, 64)
        pref["text_model.embeddings.position_ids"] = torch.arange(77)[None]
        a, b = pack_text_state(text_config(cfgd), bare), pack_text_state(text_config(cfgd), pref)
        assert set(a) == set(b) == set(enc.host) and all(torch.equal(a[k], b[k]) and torch.equal(a[k], enc.host[k]) for k in a)
        C = 64
        wq, wk = bare["encoder.layers.1.self_attn.q_proj.weight"], bare["encoder.layers.1.self_attn.k_proj.weight"]
        assert torch.equal(a["1.qk.w"][:C], wq) and torch.equal(a["1.qk.w"][C:], wk) and a["1.fc1.w"].shape == (128, 64)
        # the folder's weights are the module's: from_torch sees the same tensors, and the restatement on them equals the module in fp64
        mod = CLIPTextModel.from_pretrained(os.path.join(folders[name], "text_encoder")).eval()
        t = HipCLIPTextEncoder.from_torch(mod, device="cpu")
        assert all(torch.equal(t.host[k], enc.host[k]) for k in enc.host)
        ids = clip_tokens(PROMPTS, vocab=enc.config.vocab_size)
        with torch.no_grad():
            want = mod.double()(ids)[0]
        assert scale_err(tower_ref(enc.config, bare, ids), want) <= 1e-12
        broken = dict(bare)
        broken.pop("encoder.layers.0.mlp.fc2.bias")
        with pytest.raises(ValueError, match="fc2.bias"):
            pack_text_state(text_config(cfgd), broken)


def test_refusals(folders):
    from freefine_amd.text import HipCLIPTextEncoder, text_config
    with pytest.raises(ValueError, match="head dim 32"):
        HipCLIPTextEncoder.from_folder(folders["d32"], device="cpu")
    base = dict(vocab_size=100, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2)
    assert text_config(base).hidden_act == "quick_gelu" and text_config(base).layer_norm_eps == 1e-5
    with pytest.raises(ValueError, match="hidden_act 'relu'"):
        text_config(dict(base, hidden_act="relu"))
    with pytest.raises(ValueError, match="head dim"):
        text_config(dict(base, num_attention_heads=3))
    with pytest.raises(ValueError, match="missing"):
        text_config({k: v for k, v in base.items() if k != "vocab_size"})
    enc = HipCLIPTextEncoder.from_folder(folders["quick"], device="cpu")
    ids = torch.zeros(2, 77, dtype=torch.int64)
    with pytest.raises(ValueError, match="attention_mask"):
        enc(ids, attention_mask=torch.ones(2, 77))
    with pytest.raises(ValueError, match="positions"):
        enc(torch.zeros(1, 97, dtype=torch.int64))
    with pytest.raises(ValueError, match="positions"):
        enc(torch.zeros(1, 80, dtype=torch.int64))          # beyond the checkpoint's 77 position embeddings
    with pytest.raises(ValueError, match="token ids"):
        enc(torch.full((1, 77), enc.config.vocab_size, dtype=torch.int64))
    with pytest.raises(ValueError, match="token ids"):
        enc(torch.full((1, 77), -1, dtype=torch.int64))


def test_pipeline_components_take_the_native_switch(folders):
    """FreeFinePipeline.components(native_text=True) builds no transformers model (the executor is built in from_state's mode, on the device); default unchanged"""
    from freefine_amd.pipeline import FreeFinePipeline
    from freefine_amd.text import NativeTextSpec
    *_, enc, _, _ = FreeFinePipeline.components(folders["quick"], native_text=True)
    assert isinstance(enc, NativeTextSpec) and enc.config.hidden_size == 64
    *_, enc, _, _ = FreeFinePipeline.components(folders["quick"])
    assert isinstance(enc, torch.nn.Module)
    with pytest.raises(ValueError, match="head dim 32"):
        FreeFinePipeline.components(folders["d32"], native_text=True)
