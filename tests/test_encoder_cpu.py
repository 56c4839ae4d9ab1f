"""CPU: the launch sequence of the four transformer towers that run on encoder.run_block -- HipDinoV2, HipDino, HipDepthAnything.features, HipCLIPVision and
HipCLIPTextEncoder.  ops.linear / layernorm / attention / embed_tokens are replaced by recorders that return zero tensors of the shapes (and pair marks) the real
wrappers return, so the towers' forwards run on the CPU device without the library; what is asserted is each tower's contract with the block: per block the eight
calls in order with their operands, flags and the one V^T buffer, and nothing but the tower's own calls around them."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from freefine_amd import clipvision, depth, dino, encoder, ops, text

ACTS = ("silu", "gelu", "relu", "qgelu", "geglu")
_REAL = {n: inspect.signature(getattr(ops, n)) for n in ("linear", "layernorm", "attention", "embed_tokens")}


class Recorder:
    """stand-ins for the four ops; .calls = [SimpleNamespace(op, <every argument of the real signature, defaults applied>, ret)]"""

    def __init__(self, monkeypatch):
        self.calls = []
        for n in _REAL:
            monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: self._call(_n, a, k))

    def _call(self, name, a, k):
        b = _REAL[name].bind(*a, **k)
        b.apply_defaults()
        c = SimpleNamespace(op=name, **b.arguments)
        c.ret = getattr(self, "_" + name)(c)
        self.calls.append(c)
        return c.ret

    @staticmethod
    def _pair(shape, C):
        return ops._mark_pair(torch.zeros(*shape, 2 * C, dtype=torch.bfloat16), C)

    def _layernorm(self, c):
        return self._pair(c.x.shape[:-1], c.x.shape[-1]) if c.pair else torch.zeros_like(c.x)

    def _linear(self, c):
        x3, N = ops.is_x3(c.w), c.w.shape[0]
        odt = torch.float32 if x3 else c.x.dtype
        if c.transposed_ld is not None:
            M = c.x.numel() // c.x.shape[-1]
            return c.out if c.out is not None else torch.zeros(M // (c.rows_per_batch or M), N, c.transposed_ld, dtype=odt)
        if c.out_pair:
            assert x3 and c.out is None
            return self._pair(c.x.shape[:-1], N)
        return c.out if c.out is not None else torch.zeros(*c.x.shape[:-1], N, dtype=odt)

    def _attention(self, c):
        Bq, S, _ = c.q.shape
        if c.out_pair and c.x3 and c.q.dtype == torch.float32:
            return self._pair((Bq, S), c.C)
        return torch.zeros(Bq, S, c.C, dtype=c.q.dtype)

    def _embed_tokens(self, c):
        return torch.zeros(*c.ids.shape, c.table.shape[1], dtype=c.dtype)


def same(a, b):
    """the same tensor: storage, shape and strides"""
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype


def check_blocks(calls, blocks, x, *, S, C, heads, eps, act, hidden, x3, causal, splitk):
    """calls: the 8 * len(blocks) recorded calls of one forward's blocks; x: the tensor the first block reads.  Returns the last block's output."""
    assert len(calls) == 8 * len(blocks)
    B, ld, vt = x.shape[0], (S + 7) // 8 * 8, None
    pair = lambda t: ops.pair_width(t) if x3 else None
    for i, b in enumerate(blocks):
        ln1, qk, v, att, o, ln2, fc1, fc2 = calls[8 * i:8 * i + 8]
        assert [c.op for c in calls[8 * i:8 * i + 8]] == ["layernorm", "linear", "linear", "attention", "linear", "layernorm", "linear", "linear"], i
        for c, w in ((qk, b.qk), (v, b.v), (o, b.o), (fc1, b.fc1), (fc2, b.fc2)):
            assert c.w is w[0] and c.bias is w[1] and c.splitk == splitk and c.rowbias is None and c.alpha == 1.0 and not c.out_f32 and c.kv64_from is None
            assert [a for a in ACTS if getattr(c, a)] == ([act] if c is fc1 else []), (i, c.w.shape)
            assert c.out_pair == (x3 and c is fc1) and (c.residual is None) == (c is not o and c is not fc2) and (c.transposed_ld is None) == (c is not v)
            assert (c.out is None) == (c is not v) and ops.is_x3(c.w) == x3
        for c, w, src in ((ln1, b.ln1, x), (ln2, b.ln2, o.ret)):
            assert c.x is src and c.gamma is w[0] and c.beta is w[1] and c.eps == eps and c.pair == x3 and c.out is None and tuple(c.x.shape) == (B, S, C)
            assert pair(c.ret) == (C if x3 else None) and c.x.dtype == x.dtype
        assert qk.x is ln1.ret and qk.K == C and tuple(qk.ret.shape) == (B, S, 2 * C)
        assert v.x is ln1.ret and v.K == C and v.rows_per_batch == S and v.transposed_ld == ld
        assert tuple(v.out.shape) == (B, C, ld) and v.out.dtype == x.dtype and v.out.is_contiguous()
        vt = vt if vt is not None else v.out
        assert v.out is vt, "every block of one forward writes V^T into the same buffer"
        assert att.q is qk.ret and same(att.k, qk.ret[..., C:]) and att.vt is vt and att.heads == heads and att.scale == 0.125 and att.passes is None
        assert att.Sk == S and att.C == C and att.x3 == x3 and att.out_pair == x3 and att.causal == causal and att.out is None and not att.kv_images
        assert att.w_dev is None and att.Bo is None and pair(att.ret) == (C if x3 else None)
        assert o.x is att.ret and o.K == C and o.residual is x
        assert fc1.x is ln2.ret and fc1.K == C and pair(fc1.ret) == (hidden if x3 else None) and fc1.ret.shape[-1] == (2 * hidden if x3 else hidden)
        assert fc2.x is fc1.ret and fc2.K == hidden and fc2.residual is o.ret and tuple(fc2.ret.shape) == (B, S, C)
        x = fc2.ret
    return x


MODES = [pytest.param(False, id="f32"), pytest.param(True, id="x3")]


def _image(B, H, W, seed=0):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("x3", MODES)
@pytest.mark.parametrize("kind,H,W", [("dinov2", 56, 42), ("dino", 48, 32)])
def test_dino_towers_run_the_shared_block(monkeypatch, kind, H, W, x3):
    """HipDinoV2 "tiny" at 56 x 42 (S = 13, V^T rows of 16) and HipDino "tiny16" at 48 x 32 (S = 7, rows of 8): patch GEMM, the blocks, the class rows' norm"""
    cfg = dino.dinov2_config("tiny") if kind == "dinov2" else dino.dino_config("tiny16")
    net = (dino.HipDinoV2 if kind == "dinov2" else dino.HipDino)(cfg, dino.synthetic_state(cfg, 1), dtype=torch.float32, device="cpu", x3=x3)
    rec = Recorder(monkeypatch)
    out = net(_image(2, H, W))
    C, S, n = cfg.embed_dim, 1 + (H // cfg.patch) * (W // cfg.patch), len(net.blocks)
    assert len(rec.calls) == 2 + 8 * n == 34 and (S, (S + 7) // 8 * 8) == ((13, 16) if kind == "dinov2" else (7, 8))
    pe, norm = rec.calls[0], rec.calls[-1]
    assert pe.op == "linear" and pe.w is net.pe[0] and pe.bias is net.pe[1] and pe.K == net.kpe == ((608 if x3 else 592) if cfg.patch == 14 else 768)
    assert tuple(pe.x.shape) == (2 * (S - 1), net.kpe) and tuple(pe.residual.shape) == (2 * (S - 1), C) and pe.splitk == 0 and not any(getattr(pe, a) for a in ACTS)
    x = rec.calls[1].x
    assert tuple(x.shape) == (2, S, C) and x.dtype == torch.float32
    check_blocks(rec.calls[1:-1], net.blocks, x, S=S, C=C, heads=cfg.num_heads, eps=1e-6, act="gelu", hidden=4 * C, x3=x3, causal=False, splitk=0)
    assert norm.op == "layernorm" and tuple(norm.x.shape) == (2, C) and norm.gamma is net.norm[0] and norm.eps == 1e-6
    assert not norm.pair and tuple(out.shape) == (2, C) and out.dtype == torch.float32


def test_depth_features_run_the_shared_block(monkeypatch):
    """HipDepthAnything "tiny" .features at 56 x 42: the encoder's calls, then the final LayerNorm over each of the last four blocks' tokens"""
    cfg = depth.depth_config("tiny")
    net = depth.HipDepthAnything(cfg, depth.synthetic_state(cfg, 1), dtype=torch.float32, device="cpu")
    rec = Recorder(monkeypatch)
    feats, ph, pw = net.features(_image(1, 56, 42))
    C, S = cfg.embed_dim, 13
    assert (ph, pw) == (4, 3) and len(rec.calls) == 1 + 8 * 4 + 4 and rec.calls[0].op == "linear" and rec.calls[0].w is net.pe[0]
    check_blocks(rec.calls[1:33], net.blocks, rec.calls[1].x, S=S, C=C, heads=cfg.num_heads, eps=1e-6, act="gelu", hidden=4 * C, x3=False, causal=False, splitk=0)
    kept = [rec.calls[8 * i + 8].ret for i in range(4)]                       # fc2's output of each block
    for c, t, f in zip(rec.calls[33:], kept, feats):
        assert c.op == "layernorm" and c.x is t and c.gamma is net.norm[0] and c.eps == 1e-6 and not c.pair and tuple(f.shape) == (1, S - 1, C)
    assert len({t.data_ptr() for t in kept}) == 4 and all(t.data_ptr() != rec.calls[3].out.data_ptr() for t in kept)      # token tensors, never the V^T buffer


@pytest.mark.parametrize("x3", MODES)
def test_clip_vision_runs_the_shared_block(monkeypatch, x3):
    """HipCLIPVision "tiny": S = 50, V^T rows of 56; patch GEMM without bias, pre_layrnorm, the layers, post_layernorm on the class rows, the projection"""
    cfg = clipvision.clip_vision_config("tiny")
    net = clipvision.HipCLIPVision(cfg, clipvision.synthetic_state(cfg, 1), dtype=torch.float32, device="cpu", x3=x3)
    rec = Recorder(monkeypatch)
    out = net(_image(2, 224, 224))
    C, S = cfg.hidden_size, 50
    assert len(rec.calls) == 4 + 8 * 2 == 20
    pe, pre, post, proj = rec.calls[0], rec.calls[1], rec.calls[-2], rec.calls[-1]
    assert pe.op == "linear" and pe.w is net.pe and pe.bias is None and pe.K == 3072 and tuple(pe.residual.shape) == (2 * 49, C) and pe.splitk == 0
    assert pre.op == "layernorm" and pre.gamma is net.pre[0] and pre.eps == cfg.layer_norm_eps and not pre.pair and tuple(pre.x.shape) == (2, S, C)
    check_blocks(rec.calls[2:-2], net.blocks, pre.ret, S=S, C=C, heads=cfg.num_attention_heads, eps=cfg.layer_norm_eps, act="qgelu", hidden=cfg.intermediate_size,
                 x3=x3, causal=False, splitk=0)
    assert rec.calls[4].transposed_ld == 56
    assert post.op == "layernorm" and post.gamma is net.post[0] and post.eps == cfg.layer_norm_eps and post.pair == x3 and tuple(post.x.shape) == (2, C)
    assert proj.op == "linear" and proj.x is post.ret and proj.w is net.proj and proj.bias is None and proj.K == C and proj.splitk == 0
    assert not any(getattr(c, a) for c in (pe, proj) for a in ACTS) and tuple(out.shape) == (2, cfg.projection_dim)


@pytest.mark.parametrize("x3", MODES)
@pytest.mark.parametrize("hidden_act,act", [("quick_gelu", "qgelu"), ("gelu", "gelu")])
def test_clip_text_runs_the_shared_block(monkeypatch, hidden_act, act, x3):
    """HipCLIPTextEncoder, one layer of width 128 with two heads, on 5 prompts of 77 ids (a full group of 4 and a padded one): per group the lookup, the layer
    (causal, unsplit GEMMs, the config's eps), final_layer_norm"""
    cfg = text.text_config(dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, hidden_act=hidden_act,
                                layer_norm_eps=1e-4))
    shapes = {"embeddings.token_embedding.weight": (64, 128), "embeddings.position_embedding.weight": (77, 128), "final_layer_norm.weight": (128,),
              "final_layer_norm.bias": (128,), **encoder.clip_layer_shapes(cfg)}
    enc = text.HipCLIPTextEncoder(cfg, encoder.draw_state(shapes, 1), dtype=torch.float32, device="cpu", x3=x3)
    rec = Recorder(monkeypatch)
    out, = enc(torch.randint(0, 64, (5, 77), generator=torch.Generator().manual_seed(0)))
    assert len(rec.calls) == 2 * 10 and tuple(out.shape) == (5, 77, 128)
    for g in (rec.calls[:10], rec.calls[10:]):
        emb, lnf = g[0], g[-1]
        assert emb.op == "embed_tokens" and tuple(emb.ids.shape) == (4, 77) and emb.table is enc.tok and emb.pos is enc.pos and emb.dtype == torch.float32
        last = check_blocks(g[1:-1], enc.blocks, emb.ret, S=77, C=128, heads=2, eps=1e-4, act=act, hidden=256, x3=x3, causal=True, splitk=1)
        assert g[3].transposed_ld == 80
        assert lnf.op == "layernorm" and lnf.x is last and lnf.gamma is enc.lnf[0] and lnf.eps == 1e-4 and not lnf.pair
    assert rec.calls[3].out is not rec.calls[13].out                          # a buffer per forward


def test_split_bf16_takes_float32_in_every_tower():
    """x3=True with dtype bfloat16 is a ValueError in all four (the text encoder included)"""
    dc, vc = dino.dinov2_config("tiny"), clipvision.clip_vision_config("tiny")
    tc = text.text_config(dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2))
    for build in (lambda: dino.HipDinoV2(dc, {}, dtype=torch.bfloat16, device="cpu", x3=True),
                  lambda: dino.HipDino(dino.dino_config("tiny16"), {}, dtype=torch.bfloat16, device="cpu", x3=True),
                  lambda: clipvision.HipCLIPVision(vc, {}, dtype=torch.bfloat16, device="cpu", x3=True),
                  lambda: text.HipCLIPTextEncoder(tc, {}, dtype=torch.bfloat16, device="cpu", x3=True)):
        with pytest.raises(ValueError, match="x3=True .split-bf16. takes dtype=torch.float32"):
            build()
