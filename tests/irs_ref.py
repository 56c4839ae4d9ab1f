"""The ImageReward score restated in plain torch, fp64 sums everywhere: BLIP's ViT (timm layout), BLIP's cross-attending BERT (BlipTextModel's names), the reward
head and the score.  mode "f64", or a device mode's arithmetic emulated as tests/test_text_native_cpu.py does it: "x3" = split-bf16 products of the fp32-rounded
operands, fp32 storage; "bf16" = bf16 products and storage.  tests/test_irs_cpu.py checks the f64 mode against transformers' BlipVisionModel / BlipTextModel;
tests/test_irs_gpu.py holds the device to those modules and takes its x3 / bf16 reference errors from the emulations."""
import torch
import torch.nn.functional as F

from test_text_native_cpu import _mm, _store

REWARD_MEAN, REWARD_STD = 0.16717362830052426, 1.0333394966054072


def _attend(q, k, v, nh, mode, live=None):
    """q [B, S, C], k / v [B, Sk, C] -> softmax(q k^T / sqrt(D) over the live keys) v per head [B, S, C]; normalised after the second product as the kernels do.
    live: None or bool [B, Sk]"""
    B, S, C = q.shape
    D = C // nh
    heads = lambda u: u.reshape(B, u.shape[1], nh, D).transpose(1, 2)
    q, k, v = heads(q), heads(k), heads(v)
    s = _mm(q, k, mode) * D ** -0.5
    if live is not None:
        s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    a = _mm(e, v.transpose(-1, -2), mode) / e.sum(-1, keepdim=True)
    return a.transpose(1, 2).reshape(B, S, C)


def vision_ref(cfg, state, x, mode="f64"):
    """BLIP's VisionTransformer(x) = BlipVisionModel(x).last_hidden_state: x [B, 3, 224, 224] -> fp64 [B, 197, C].  state: timm's layout; cfg: irs.blip_vision_config's"""
    st = {k: v.double() for k, v in state.items()}
    C, nh, eps, ps = cfg.embed_dim, cfg.num_heads, cfg.ln_eps, cfg.patch
    B, _, H, W = x.shape
    ph, pw = H // ps, W // ps
    keep = lambda t: _store(t, mode)
    ln = lambda t, p: F.layer_norm(t, (C,), st[p + ".weight"], st[p + ".bias"], eps)
    lin = lambda t, p: _mm(t, st[p + ".weight"], mode) + st[p + ".bias"]
    rows = keep(x.double().reshape(B, 3, ph, ps, pw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, ph * pw, 3 * ps * ps))
    pos = st["pos_embed"][0]
    t = keep(_mm(rows, st["patch_embed.proj.weight"].reshape(C, -1), mode) + st["patch_embed.proj.bias"] + keep(pos[1:]))
    h = torch.cat([keep(st["cls_token"][0] + pos[:1]).expand(B, 1, C), t], dim=1)
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        qkv = keep(lin(keep(ln(h, p + "norm1")), p + "attn.qkv"))
        a = keep(_attend(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], nh, mode))
        h = keep(h + lin(a, p + "attn.proj"))
        u = keep(F.gelu(lin(keep(ln(h, p + "norm2")), p + "mlp.fc1")))
        h = keep(h + lin(u, p + "mlp.fc2"))
    return keep(ln(h, "norm"))


def text_ref(cfg, state, ids, mask, embeds, mode="f64"):
    """BlipTextModel(ids, attention_mask=mask, encoder_hidden_states=embeds, is_decoder=False).last_hidden_state: ids, mask [B, S], embeds [B, Sk, Ce] ->
    fp64 [B, S, C] (the score reads row 0).  Post-LN: every GEMM's residual sum is stored, then normalised."""
    st = {k: v.double() for k, v in state.items()}
    C, nh, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    B, S = ids.shape
    keep = lambda t: _store(t, mode)
    ln = lambda t, p: F.layer_norm(t, (C,), st[p + ".weight"], st[p + ".bias"], eps)
    lin = lambda t, p: _mm(t, st[p + ".weight"], mode) + st[p + ".bias"]
    live = mask != 0
    e = keep(embeds.double())
    x = keep(ln(st["embeddings.word_embeddings.weight"][ids] + st["embeddings.position_embeddings.weight"][:S], "embeddings.LayerNorm"))
    for i in range(cfg.num_hidden_layers):
        p, a, c = f"encoder.layer.{i}.", f"encoder.layer.{i}.attention.", f"encoder.layer.{i}.crossattention."
        q, k, v = (keep(lin(x, a + "self." + n)) for n in ("query", "key", "value"))
        o = keep(_attend(q, k, v, nh, mode, live))
        x = keep(ln(keep(x + lin(o, a + "output.dense")), a + "output.LayerNorm"))
        q, k, v = keep(lin(x, c + "self.query")), keep(lin(e, c + "self.key")), keep(lin(e, c + "self.value"))
        o = keep(_attend(q, k, v, nh, mode))
        x = keep(ln(keep(x + lin(o, c + "output.dense")), c + "output.LayerNorm"))
        h = keep(F.gelu(lin(x, p + "intermediate.dense")))
        x = keep(ln(keep(x + lin(h, p + "output.dense")), p + "output.LayerNorm"))
    return x


def head_ref(head, x):
    """the five Linears one after the other (fp64), then the standardisation: x [B, hidden] -> [B]"""
    a = x.double()
    for w, b in head:
        a = a @ w.double().t() + b.double()
    return (a[:, 0] - REWARD_MEAN) / REWARD_STD


def chain_tol(layers, x, delta=0.0, scale=1.0):
    """per row of x [B, k_0]: a bound on |ffn_affine_chain - fp64| for fp32 inputs carrying an error of at most `delta` each.  The chain is affine, so an error
    vector entering layer l reaches the output through the exact product P_l = W_L ... W_l: |dr| <= sum_j |P_l[:, j]| max|error_j|.  Entering layer 1: delta.
    Made by layer l itself: every output is a lane's ceil(K / 64) sequential fused multiply-adds, six tree additions and the bias, so at most
    (ceil(K / 64) + 8) 2^-24 (|W_l| |a_{l-1}| + |b_l|).  Then one subtraction and one division."""
    u = 2.0 ** -24
    ws = [(w.double(), b.double()) for w, b in layers]
    tails = [None] * (len(ws) + 1)                      # tails[l]: sum over inputs j of |product of layers l.. [:, j]|, per output
    prod = torch.eye(ws[-1][0].shape[0], dtype=torch.float64)
    tails[len(ws)] = prod.abs().sum(1)
    for l in range(len(ws) - 1, -1, -1):
        prod = prod @ ws[l][0]
        tails[l] = prod.abs().sum(1)
    a = x.double()
    tol = delta * tails[0].max() * torch.ones(a.shape[0], dtype=torch.float64)
    for l, (w, b) in enumerate(ws):
        mag = a.abs() @ w.abs().t() + b.abs()
        tol = tol + (-(-w.shape[1] // 64) + 8) * u * mag.max(1).values * tails[l + 1].max()
        a = a @ w.t() + b
    return tol / abs(scale) + 4 * u * (a.abs().max(1).values + 1) / abs(scale)


def score_ref(vcfg, vst, tcfg, tst, head, x, ids, mask, mode="f64"):
    """normalised images x [B, 3, 224, 224], ids / mask [N, S] with N = 1 or B -> (fp64 rewards [B], the text tower's row 0 [B, hidden])"""
    e = vision_ref(vcfg, vst, x, mode)
    B = x.shape[0]
    row = text_ref(tcfg, tst, ids.expand(B, -1), mask.expand(B, -1), e, mode)[:, 0]
    return head_ref(head, row), row
