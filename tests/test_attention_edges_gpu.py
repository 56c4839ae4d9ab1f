"""Every attention kernel of the ffn_attn plan at the edges of its online softmax and its masks, against ONE fp64 statement of the pass
table (ref_passes) evaluated on the GPU.

The other attention tests draw q and k from N(0, 1): logits of about N(0, 1), so the deferred re-referencing of the running maximum (taken
only when a later score beats the reference by more than 2^6 in log2 units, ~4.2 nats) is almost never exercised.  Here the logits are
PLANTED: within each head a unit vector u is removed from every q and k, then q_i += beta_i u and k_j += c_j u, so query i sees key j at
exactly scale * beta_i * c_j nats above its N(0, 1) background -- which queries jump, by how much and at which key is chosen.

Every case asserts the exact set of kernels it launched (ops.profile_begin / profile_end, spelled like rocprofv3's kernel trace), and the
reference rounds the operands the way that kernel rounds them (bf16 q pre-multiplied by scale * log2 e where the kernel does it; split-bf16
hi / lo operands without the lo * lo product), so the gates stay those of test_ops_gpu.py with keys planted up to 25 nats above the
background (no logit reaches 31 nats): fp32 2e-5, split-bf16 X3_ATT_TOL, bf16 1.5e-2."""
import math

import pytest
import torch

from test_ops_gpu import X3_ATT_TOL, _production_masks, ref_attention, relerr

pytestmark = pytest.mark.gpu

HEAD_RULE, UNIFORM_SEL1, UNIFORM_SEL0 = 1, 2, 4      # FFN_ATT_* (include/freefine_hip.h)
LOG2E = 1.44269504088896340736
TOL = {"f32": 2e-5, "bf16": 1.5e-2, "bf16p": 1.5e-2, "x3": X3_ATT_TOL, "x3p": X3_ATT_TOL}

# kernel names as ffn_attn_kernel_name spells them (test_abi_cpu.py::test_attention_kernel_choice_table), D = 64
F32_K = "void attn_kernel<float, 64, 2, 64, 1, true>(ffn_attn_desc)"
PRESPLIT = "attn_presplit_kernel"


def bf16_k(m):
    return f"void attn_kernel<bf16, 64, 2, 64, 2, {'true' if m else 'false'}>(ffn_attn_desc)"


def tk(name, m):
    return f"void {name}<{'true' if m else 'false'}>(ffn_attn_desc)"


def xk(name, *tpl):
    return f"void {name}<{', '.join(str(t) for t in tpl)}>(ffn_attn_desc, int, int)"


# the nine kernel kinds of the plan, both instantiations where a kind has two: each is the expectation of some case of this module
KINDS = ["attn_kernel<float", "attn_kernel<bf16", "attn_pp_kernel<true>", "attn_pp_kernel<false>", "xattn_kernel<", "xattn_mp_kernel<",
         "xattn_x3_kernel<", "attn_x3_kernel<true>", "attn_x3_kernel<false>", "attn_x3p_kernel<true>", "attn_x3p_kernel<false>",
         "attn_x3w_kernel<true>", "attn_x3w_kernel<false>"]


def operand_kind(names):
    """how the kernel that ran rounds its operands (see ref_passes)"""
    (k,) = [n for n in names if n != PRESPLIT]
    if "attn_x3p_kernel" in k or "attn_x3w_kernel" in k:
        return "x3p"
    if "x3_kernel" in k:                                   # attn_x3_kernel, xattn_x3_kernel: q split as it is, scale applied to the scores
        return "x3"
    if "attn_pp_kernel" in k or "attn_kernel<bf16" in k:   # q * scale * log2 e rounded to bf16 in the fragment load
        return "bf16p"
    if "xattn" in k:
        return "bf16"
    return "f32"


def _split(x):
    """fp32 x -> (hi, lo) in fp64: hi = RNE bf16(x), lo = RNE bf16(x - hi) (x3_split8, attention_x3.h)"""
    hi = x.to(torch.bfloat16).float()
    return hi.double(), (x - hi).to(torch.bfloat16).double()


def ref_passes(q, k, v, heads, scale, passes, w_dev=None, kind="f32", head_rows=None):
    """out[b] = sum_p w_p(b) wq_p[q] softmax_k(scale <Q[q_row], K[kv_row]> | mask) V[kv_row] in fp64 on q's device, the pass table of
    include/freefine_hip.h as attention.h reads it: weight w_const + w_slope * w_dev, per-query weight wq, allowed(q, k) = (kmask[k] != 0) ==
    (qsel[q] != 0) (qsel absent: 1) on the heads the tiled-head rule masks (parity of (hr_row or b) * heads + head), UNIFORM_SEL1 / SEL0: the
    sel = 1 / sel = 0 queries of a masked head get a uniform softmax over all keys; skipped entries contribute nothing (rows without any
    entry are zeros).
    q [Bq,S,C], k / v [Bk,Sk,C] as the kernel got them.  kind = the operand rounding of the kernel (operand_kind):
      f32: exact (fp64 scale); bf16: bf16 operands; bf16p: and q * fp32(scale * log2 e) rounded to bf16 (the fp32 product);
      x3: split-bf16 products (q, k, v each hi + lo, the lo * lo term dropped), scale applied to the scores;
      x3p: the same on q pre-multiplied in fp32 by fp32(scale * log2 e).
    head_rows: the row the tiled-head rule uses for each output row, stated by the test (default: the entry's hr_row, else the output row)."""
    S, C = q.shape[1], q.shape[2]
    D = C // heads
    c32 = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).item()
    post = c32                                            # scores -> log2 units
    if kind in ("f32", "bf16", "bf16p"):
        qa, ka, qb, kb = q.double(), k.double(), None, None
        if kind == "f32":
            post = scale * LOG2E
        if kind == "bf16p":
            qa, post = (q.float() * c32).to(torch.bfloat16).double(), 1.0
        vv = v.double()
    else:
        qh, ql = _split(q.float() * c32 if kind == "x3p" else q.float())
        kh, kl = _split(k.float())
        qa, ka, qb, kb = qh, kh + kl, ql, kh
        post = 1.0 if kind == "x3p" else c32
        vh, vl = _split(v.float())
        vv = vh + vl
    wd = 0.0 if w_dev is None else float(w_dev.item())
    out = torch.zeros(len(passes[0]), S, C, dtype=torch.float64, device=q.device)
    for rows in passes:
        for b, sp in enumerate(rows):
            if sp is None or (sp.w_const == 0.0 and sp.w_slope == 0.0):
                continue
            w = sp.w_const + sp.w_slope * wd
            wq = 1.0 if sp.wq is None else sp.wq.double()[:, None]
            hb = head_rows[b] if head_rows is not None else (b if sp.hr_row is None else sp.hr_row)
            for h in range(heads):
                sl = slice(h * D, (h + 1) * D)
                t = qa[sp.q_row, :, sl] @ ka[sp.kv_row, :, sl].t()
                if qb is not None:
                    t += qb[sp.q_row, :, sl] @ kb[sp.kv_row, :, sl].t()
                t *= post
                if sp.kmask is not None and (not (sp.flags & HEAD_RULE) or (hb * heads + h) % 2 == 0):
                    sel = torch.ones(S, dtype=torch.bool, device=q.device) if sp.qsel is None else sp.qsel != 0
                    allowed = (sp.kmask != 0)[None, :] == sel[:, None]
                    uni = (sel & bool(sp.flags & UNIFORM_SEL1)) | (~sel & bool(sp.flags & UNIFORM_SEL0))
                    allowed[uni] = True
                    t[uni] = 0.0
                    assert bool(allowed.any(dim=1).all()), "a query without allowed keys and without its uniform flag: outside the contract"
                    t = t.masked_fill(~allowed, -math.inf)
                p = torch.exp2(t - t.amax(dim=1, keepdim=True))
                out[b, :, sl] += (w * wq) * ((p / p.sum(dim=1, keepdim=True)) @ vv[sp.kv_row, :, sl])
    return out


def check(out, ref, tol, what=""):
    """per output row: max |out - ref| / max |ref| < tol; rows no pass contributes to must be exact zeros"""
    worst = 0.0
    for b in range(ref.shape[0]):
        if not bool(ref[b].any()):
            assert not bool(out[b].any()), (what, b, "row without active entries is not zero")
            continue
        worst = max(worst, relerr(out[b], ref[b]))
    assert worst < tol, (what, worst)
    return worst


def run_profiled(q, k, vt, heads, scale, passes, **kw):
    """ops.attention with its launches recorded -> (out, {kernel name: dict(calls, ...)})"""
    from freefine_amd import ops
    ops.profile_begin()
    try:
        out = ops.attention(q, k, vt, heads, scale, passes, **kw)
    finally:
        prof = ops.profile_end()
    return out, prof


def run(q, k, vt, heads, scale, passes, **kw):
    """ops.attention with its launches recorded -> (out, set of kernel names)"""
    out, prof = run_profiled(q, k, vt, heads, scale, passes, **kw)
    return out, set(prof)


def test_reference_reproduces_the_hand_written_statements(gpu):
    """ref_passes against the statements test_attention_uniform_and_wq and test_attention_tca_edit (test_ops_gpu.py) write by hand: uniform
    flag, per-query weights, skipped entries, a row remap, a second pass, key mask + query selector under the tiled-head rule, device-scalar
    blend.  (Pure fp64, nothing launched.)"""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(22)
    B, S, Sk, heads, D = 3, 100, 77, 8, 40
    C = heads * D
    q, k, v = (torch.randn(B, n, C, generator=g, dtype=torch.float64) for n in (S, Sk, Sk))
    km = torch.zeros(Sk, dtype=torch.uint8)
    wq = torch.rand(S, generator=g)
    p0 = [ops.AttnEntrySpec(0, 0, 1.0, 0.0, kmask=km, flags=UNIFORM_SEL1), ops.AttnEntrySpec(1, 1), ops.AttnEntrySpec(2, 2, wq=wq)]
    p1 = [None, None, ops.AttnEntrySpec(0, 1, 0.5)]
    scale = D ** -0.5
    got = ref_passes(q, k, v, heads, scale, [p0, p1]).cpu()
    want = [v[0].mean(dim=0, keepdim=True).expand(S, C), ref_attention(q[1], k[1], v[1], heads, scale),
            wq.double()[:, None] * ref_attention(q[2], k[2], v[2], heads, scale) + 0.5 * ref_attention(q[0], k[1], v[1], heads, scale)]
    for b in range(B):
        assert (got[b] - want[b]).abs().max().item() < 1e-12, b

    B, S, heads, D = 4, 136, 2, 160
    C = heads * D
    q, k, v = (torch.randn(B, S, C, generator=g, dtype=torch.float64) for _ in range(3))
    src, tgt = (torch.rand(S, generator=g) > 0.6).to(torch.uint8), (torch.rand(S, generator=g) > 0.5).to(torch.uint8)
    cg, scale, ref_rows = 0.35, D ** -0.5, [1, 1, 3, 3]
    p_ref = [ops.AttnEntrySpec(b, ref_rows[b], 0.0, 1.0, kmask=src, qsel=tgt, flags=HEAD_RULE) for b in range(B)]
    p_self = [ops.AttnEntrySpec(b, b, 1.0, -1.0) for b in range(B)]
    got = ref_passes(q, k, v, heads, scale, [p_ref, p_self], w_dev=torch.tensor([cg], dtype=torch.float64)).cpu()
    for b in range(B):
        allowed = torch.ones(heads, S, S, dtype=torch.bool)
        for h in range(heads):
            if (b * heads + h) % 2 == 0:
                allowed[h] = (src[None, :] != 0) == (tgt[:, None] != 0)
        want = cg * ref_attention(q[b], k[ref_rows[b]], v[ref_rows[b]], heads, scale, allowed) + (1 - cg) * ref_attention(q[b], k[b], v[b], heads, scale)
        assert (got[b] - want).abs().max().item() < 1e-12, b


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. planted logits: exact control of where a query's running maximum jumps
# ---------------------------------------------------------------------------------------------------------------------------------------
S_SP, H_SP, D_SP = 256, 2, 64
BETA = 8.0            # scale * BETA = 1 at D = 64: a key planted with c sits c nats above the background for the queries with beta = BETA


def _planted(g, Bq, Bk, Sk):
    q = torch.randn(Bq, S_SP, H_SP, D_SP, generator=g)
    k = torch.randn(Bk, Sk, H_SP, D_SP, generator=g)
    v = torch.randn(Bk, Sk, H_SP, D_SP, generator=g)
    u = torch.randn(H_SP, D_SP, generator=g)
    u /= u.norm(dim=-1, keepdim=True)
    q -= (q * u).sum(-1, keepdim=True) * u
    k -= (k * u).sum(-1, keepdim=True) * u
    return q, k, v, u


def _case(name, Sk, dev):
    """-> q, k, v [B, n, C] fp32 (CPU), passes, w_dev.  Logits stay below ~30 nats."""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(sum(map(ord, name)) + Sk)
    nt, allq = Sk // 64, torch.arange(S_SP)
    w_dev = None
    if name == "two_pass":
        q, k, v, u = _planted(g, 2, 4, Sk)
    else:
        q, k, v, u = _planted(g, 2, 2, Sk)
    beta = torch.full((2, S_SP), BETA)

    def key(row, j, c):
        k[row, j] += c * u
    plain = [[ops.AttnEntrySpec(0, 0), ops.AttnEntrySpec(1, 1)]]
    passes = plain
    if name == "mid_jump":                       # one jump of ~9-12 nats in the second 32-key unit of a middle tile
        key(0, 64 * (nt // 2) + 37, 11.0)
        key(1, 64 * max(nt // 2 - 1, 0) + 52, 9.0)
    elif name == "consecutive":                  # jumps in five consecutive units, each 5 nats (7.2 in log2 units) above the last
        u0 = Sk // 32 // 2 - 2
        for r in range(2):
            for j in range(5):
                key(r, 32 * (u0 + j) + (7 * j + 11 * r) % 32, 5.0 * (j + 1))
    elif name == "partial":                      # row 0: only the second 32-query block of each wave; row 1: a few lanes
        beta[0, allq % 64 < 32] = 0.0
        beta[1, allq % 7 != 3] = 0.0
        key(0, 64 * (nt // 2) + 40, 10.0)
        key(1, 64 * (nt // 2) + 8, 10.0)
    elif name == "edges":                        # jumps in the first unit and in the last tile; row 1 masked (two keys off) on every head
        for r in range(2):
            key(r, 1, 10.0)
            key(r, Sk - 3, 16.0)
        km = torch.ones(Sk, dtype=torch.uint8)
        km[[10, Sk - 20]] = 0
        passes = [[ops.AttnEntrySpec(0, 0), ops.AttnEntrySpec(1, 1, kmask=km.to(dev))]]
    elif name == "masked_prefix":                # sel = 1 queries: nothing allowed before key P, the first allowed key at P, then a jump;
        P = Sk * 11 // 16 + 5                    # sel = 0 queries: only the prefix, with a jump of their own in it
        km = torch.ones(Sk, dtype=torch.uint8)
        km[:P] = 0
        qs = (torch.rand(S_SP, generator=g) > 0.5).to(torch.uint8)
        for r in range(2):
            key(r, P, 3.0)
            key(r, P + 150, 14.0)
            key(r, 100, 10.0)
        km, qs = km.to(dev), qs.to(dev)
        passes = [[ops.AttnEntrySpec(0, 0, kmask=km, qsel=qs, flags=HEAD_RULE), ops.AttnEntrySpec(1, 1, kmask=km, qsel=qs)]]
    elif name == "two_pass":                     # row 0: a jump in pass 2 only; row 1: jumps in both passes at different keys; blend + wq;
                                                 # row 2: no active entry (skipped in pass 1, zero weight in pass 2): zeros
        key(1, 64 * (nt // 2) + 45, 12.0)
        key(2, min(200, Sk - 1), 9.0)
        key(3, max(Sk - 224, 0) + 33, 13.0)
        w_dev = torch.tensor([0.35], device=dev)
        wq, wq2 = torch.rand(S_SP, generator=g).to(dev), torch.rand(S_SP, generator=g).to(dev)
        passes = [[ops.AttnEntrySpec(0, 0, 1.0, -1.0), ops.AttnEntrySpec(1, 2, 1.0, -1.0, wq=wq2), None],
                  [ops.AttnEntrySpec(0, 1, 0.0, 1.0, wq=wq), ops.AttnEntrySpec(1, 3, 0.0, 1.0, wq=wq), ops.AttnEntrySpec(0, 0, 0.0, 0.0)]]
    elif name == "dominant_first":               # the first key (row 1: the first key of tile 1) ~20 nats above all others: every later
                                                 # probability ~2^-29 of it (small, not underflowing) and no later re-reference
        key(0, 0, 22.0)
        key(1, 64, 21.0)
    elif name == "masked_max":                   # a masked key carries the row's largest raw score (25 nats): what is observable is its zero
        km = torch.ones(Sk, dtype=torch.uint8)   # weight; the heads the tiled-head rule leaves unmasked do see it
        j = 64 * 5 + 10
        km[j] = 0
        for r in range(2):
            key(r, j, 25.0)
            key(r, 64 * 9 + 40, 8.0)
        km = km.to(dev)
        passes = [[ops.AttnEntrySpec(0, 0, kmask=km, flags=HEAD_RULE), ops.AttnEntrySpec(1, 1, kmask=km, flags=HEAD_RULE)]]
    else:
        raise ValueError(name)
    q += beta[:, :, None, None] * u
    C = H_SP * D_SP
    return q.reshape(-1, S_SP, C), k.reshape(-1, Sk, C), v.reshape(-1, Sk, C), passes, w_dev


def _masked(passes):
    return any(sp is not None and sp.kmask is not None for rows in passes for sp in rows)


def _expected(mode, Sk, masked, npass, multi, S=S_SP):
    """the kernel(s) the plan runs for the D = 64 launches of this module"""
    need = -(-Sk // 16)
    nkf = 2 if need <= 2 else (5 if need <= 5 else 6)
    short = not masked and Sk <= 96
    if mode == "f32":
        return {F32_K}
    if mode == "bf16":
        if short:
            return {xk("xattn_mp_kernel", nkf) if multi else xk("xattn_kernel", nkf)}
        return {tk("attn_pp_kernel", masked)} if Sk % 64 == 0 else {bf16_k(masked)}
    if short:
        return {xk("xattn_x3_kernel", nkf, 8 if (npass >= 2 or S >= 4096) else 4)}
    if Sk % 64:
        return {tk("attn_x3_kernel", masked)}
    return {PRESPLIT, tk("attn_x3w_kernel", masked)} if mode == "x3" else {tk("attn_x3p_kernel", masked)}


# (case, Sk, masked, npass, multi): Sk = 1024 = 16 tiles; 64 = one tile (unmasked: the short-key kernels); 1000 = ragged (attn_kernel<bf16>, attn_x3_kernel)
SPIKE_CASES = [("mid_jump", 1024, False, 1, False), ("consecutive", 1024, False, 1, False), ("partial", 1024, False, 1, False),
               ("edges", 1024, True, 1, False), ("masked_prefix", 1024, True, 1, False), ("two_pass", 1024, False, 2, True),
               ("dominant_first", 1024, False, 1, False), ("masked_max", 1024, True, 1, False),
               ("edges", 64, True, 1, False), ("mid_jump", 64, False, 1, False), ("two_pass", 64, False, 2, True),
               ("mid_jump", 1000, False, 1, False), ("masked_prefix", 1000, True, 1, False)]
# modes: f32, bf16, x3 (split-bf16, pre-split K / V^T where the plan takes them), x3-inkernel (ops._ATTN_PRESPLIT off: attn_x3p_kernel) where it differs
SPIKE_PARAMS = [pytest.param(c, Sk, m, id=f"{c}-Sk{Sk}-{m}") for c, Sk, masked, _, _ in SPIKE_CASES
                for m in ("f32", "bf16", "x3", "x3-inkernel") if m != "x3-inkernel" or (Sk % 64 == 0 and (masked or Sk > 96))]
SPIKE_META = {(c, Sk): (masked, npass, multi) for c, Sk, masked, npass, multi in SPIKE_CASES}


@pytest.mark.parametrize("case,Sk,mode", SPIKE_PARAMS)
def test_planted_logits(gpu, monkeypatch, case, Sk, mode):
    """softmax-range cases through every kernel that takes their shape, against ref_passes on the kernel's operand rounding"""
    from freefine_amd import ops
    masked, npass, multi = SPIKE_META[(case, Sk)]
    q, k, v, passes, w_dev = _case(case, Sk, gpu)
    assert _masked(passes) == masked and len(passes) == npass
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    q, k, v = q.to(gpu, dt), k.to(gpu, dt), v.to(gpu, dt)
    vt = ops.transpose(v, ld_dst=(Sk + 7) // 8 * 8)
    if mode == "x3-inkernel":
        monkeypatch.setattr(ops, "_ATTN_PRESPLIT", False)
    scale = D_SP ** -0.5
    out, names = run(q, k, vt, H_SP, scale, passes, Sk=Sk, w_dev=w_dev, x3=mode.startswith("x3"))
    assert names == _expected(mode, Sk, masked, npass, multi), names
    kind = operand_kind(names)
    ref = ref_passes(q, k, v, H_SP, scale, passes, w_dev, kind)
    e = check(out, ref, TOL[kind], (case, Sk, mode))
    print(f"planted {case} Sk={Sk} {mode} ({kind}): {e:.2e}")


def test_planted_logits_reach_the_rescale_branch(gpu):
    """the data of every case does what its comment says: on some head of some active entry an ALLOWED key beats the running maximum of
    the allowed keys before it (32-key units, after the query's first unit that holds an allowed key) by more than the 2^6 threshold in
    log2 units -- the kernels' re-referencing branch; and no logit reaches 31 nats"""
    for case, Sk, _, _, _ in SPIKE_CASES:
        q, k, _, passes, _ = _case(case, Sk, gpu)
        q, k = q.to(gpu).double(), k.to(gpu).double()
        jumps, top, n = 0, 0.0, Sk // 32 * 32
        for rows in passes:
            for b, sp in enumerate(rows):
                if sp is None or (sp.w_const == 0.0 and sp.w_slope == 0.0):
                    continue
                hb = b if sp.hr_row is None else sp.hr_row
                for h in range(H_SP):
                    sl = slice(h * D_SP, (h + 1) * D_SP)
                    t = (q[sp.q_row, :, sl] @ k[sp.kv_row, :, sl].t()) * D_SP ** -0.5 * LOG2E
                    top = max(top, t.max().item() / LOG2E)
                    if sp.kmask is not None and (not (sp.flags & HEAD_RULE) or (hb * H_SP + h) % 2 == 0):
                        sel = torch.ones(S_SP, dtype=torch.bool, device=gpu) if sp.qsel is None else sp.qsel != 0
                        t = t.masked_fill((sp.kmask != 0)[None, :] != sel[:, None], -math.inf)
                    um = t[:, :n].reshape(S_SP, -1, 32).amax(dim=2)
                    prev = torch.cummax(um, dim=1).values[:, :-1]
                    jumps += int(((um[:, 1:] > prev + 6.0) & torch.isfinite(prev)).sum().item())
        assert top < 31.0, (case, Sk, top)
        assert jumps > 0, (case, Sk)


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. masks at production shapes on the split-bf16 kernels; the uniform-softmax fall-back
# ---------------------------------------------------------------------------------------------------------------------------------------
def _masks(S, kind, g):
    """(source mask, target selector): _production_masks, or allowed keys only in the last tile / only in the second 32-key half of
    each tile (attn_x3w_kernel's unit boundary) for the sel = 1 queries (the sel = 0 queries: the complement)"""
    if kind in ("rect", "rand"):
        return _production_masks(S, kind, g)
    src = torch.zeros(S, dtype=torch.uint8)
    if kind == "lasttile":
        src[-64:] = 1
    else:
        src[(torch.arange(S) % 64) >= 32] = 1
    return src, (torch.rand(S, generator=g) > 0.5).to(torch.uint8)


def _tca_tables(B, src, tgt, hook, dev, ref_rows=(1, 1, 3, 3)):
    from freefine_amd import ops
    if hook == "edit":
        kmask, qsel = src.to(dev), tgt.to(dev)
        p_ref = [ops.AttnEntrySpec(b, ref_rows[b], 0.0, 1.0, kmask=kmask, qsel=qsel, flags=HEAD_RULE) for b in range(B)]
    else:                                        # keys allowed OUTSIDE the hole, no query-side blend
        kmask = (1 - src).to(dev)
        p_ref = [ops.AttnEntrySpec(b, ref_rows[b], 0.0, 1.0, kmask=kmask, flags=HEAD_RULE) for b in range(B)]
    return [p_ref, [ops.AttnEntrySpec(b, b, 1.0, -1.0) for b in range(B)]]


TCA_PARAMS = ([(4096, 5, h, m, True) for h in ("edit", "bggen") for m in ("rect", "rand")] +
              [(1024, 10, h, m, True) for h in ("edit", "bggen") for m in ("rect", "rand")] +
              [(9216, 5, "edit", "rect", True)] +
              [(4096, 5, h, m, False) for h in ("edit", "bggen") for m in ("rect", "rand")] +
              [(4096, 5, "edit", "lasttile", True), (4096, 5, "edit", "secondhalf", True)])


def _tca_kernels(presplit):
    return {PRESPLIT, tk("attn_x3w_kernel", True)} if presplit else {tk("attn_x3p_kernel", True)}


@pytest.mark.parametrize("S,heads,hook,kind,presplit", TCA_PARAMS)
def test_x3_tca_masks_at_production_shapes(gpu, monkeypatch, S, heads, hook, kind, presplit):
    """the TCA pass tables of the guided loop (reference-row K / V, key mask, query selector, tiled-head rule, device-scalar blend) with
    GeoBench-like rectangle masks (whole tiles on the kernels' 'unseen' path), random masks and two tile-aligned ones, through
    attn_x3w_kernel (pre-split K / V^T) and attn_x3p_kernel (in-kernel split), against fp64"""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(S + heads + len(kind))
    B, D = 4, 64
    C = heads * D
    q, k, v = (torch.randn(B, S, C, generator=g).to(gpu) for _ in range(3))
    vt = ops.transpose(v)
    src, tgt = _masks(S, kind, g)
    passes = _tca_tables(B, src, tgt, hook, gpu)
    cg = torch.tensor([0.35], dtype=torch.float32, device=gpu)
    monkeypatch.setattr(ops, "_ATTN_PRESPLIT", presplit)
    out, names = run(q, k, vt, heads, D ** -0.5, passes, w_dev=cg, x3=True)
    assert names == _tca_kernels(presplit), names
    ref = ref_passes(q, k, v, heads, D ** -0.5, passes, cg, "x3p")
    e = check(out, ref, X3_ATT_TOL, (S, heads, hook, kind, presplit))
    print(f"x3 TCA {hook} {kind} S={S} h={heads} {'attn_x3w' if presplit else 'attn_x3p'}: {e:.2e}")


UNIFORM_KERNELS = {"f32": {F32_K}, "bf16": {bf16_k(True)}, "x3": {tk("attn_x3_kernel", True)}}


@pytest.mark.parametrize("mode", list(UNIFORM_KERNELS))
def test_uniform_flags_fall_back(gpu, mode):
    """the two-pass TCA table with UNIFORM_SEL1 (rows 0, 1: no key has mask != 0) and UNIFORM_SEL0 (rows 2, 3: every key has it) at d = 64,
    S = 1024, h = 10: the flags move the launch off the ping-pong kernels onto attn_kernel / attn_x3_kernel"""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(1010)
    B, S, heads, D = 4, 1024, 10, 64
    C = heads * D
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    q, k, v = (torch.randn(B, S, C, generator=g).to(gpu, dt) for _ in range(3))
    vt = ops.transpose(v)
    qsel = (torch.rand(S, generator=g) > 0.5).to(torch.uint8).to(gpu)
    none_, all_ = torch.zeros(S, dtype=torch.uint8, device=gpu), torch.ones(S, dtype=torch.uint8, device=gpu)
    ref_rows = [1, 1, 3, 3]
    p_ref = [ops.AttnEntrySpec(b, ref_rows[b], 0.0, 1.0, kmask=none_ if b < 2 else all_, qsel=qsel,
                               flags=HEAD_RULE | (UNIFORM_SEL1 if b < 2 else UNIFORM_SEL0)) for b in range(B)]
    passes = [p_ref, [ops.AttnEntrySpec(b, b, 1.0, -1.0) for b in range(B)]]
    cg = torch.tensor([0.35], dtype=torch.float32, device=gpu)
    out, names = run(q, k, vt, heads, D ** -0.5, passes, w_dev=cg, x3=mode == "x3")
    assert names == UNIFORM_KERNELS[mode], names
    kind = operand_kind(names)
    e = check(out, ref_passes(q, k, v, heads, D ** -0.5, passes, cg, kind), TOL[kind], mode)
    print(f"uniform-flag TCA {mode}: {e:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. the row split of a batched self-attention call and the tiled-head rule across its launches
# ---------------------------------------------------------------------------------------------------------------------------------------
ROWSPLIT_KERNELS = {"x3": {PRESPLIT, tk("attn_x3w_kernel", True)}, "bf16": {tk("attn_pp_kernel", True)}}


@pytest.mark.parametrize("mode", list(ROWSPLIT_KERNELS))
def test_image_batched_rows_across_row_splits(gpu, monkeypatch, mode):
    """8 images x 3 rows at S = 1024 / h = 5 (TCA tables with per-image masks): with an odd head count and an odd number of rows per image the
    parity of row * heads + head that the tiled-head rule tests differs between an entry's logical row (pinned by AttnEntrySpec.shifted), its
    absolute output row (entries left unpinned, images 3 and 7: ops._set_entries pins b0 + b) and its row inside a launch.  The head-rule rows
    are stated here, not read back from the entries.  Launches cut by ops.attn_row_split's own choice and into 5- and 7-row chunks that start
    at odd rows in the middle of images: each against fp64, and all bit-identical (every output row is computed by independent workgroups)."""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(624)
    K, Bp, S, heads, D = 8, 3, 1024, 5, 64
    C = heads * D
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    q, k, v = (torch.randn(K * Bp, S, C, generator=g).to(gpu, dt) for _ in range(3))
    vt = ops.transpose(v)
    ref_rows = [1, 1, 2]
    p_ref, p_self, head_rows = [], [], []
    for i in range(K):
        src, tgt = _production_masks(S, "rect" if i % 2 else "rand", g)
        if i % 3 == 2:
            src = 1 - src
        sg, tg = src.to(gpu), tgt.to(gpu)
        for b in range(Bp):
            r = ops.AttnEntrySpec(b, ref_rows[b], 0.0, 1.0, kmask=sg, qsel=tg, flags=HEAD_RULE)
            s_ = ops.AttnEntrySpec(b, b, 1.0, -1.0)
            if i % 4 == 3:                       # unpinned: the rule follows the absolute output row
                p_ref.append(ops.AttnEntrySpec(i * Bp + b, i * Bp + ref_rows[b], 0.0, 1.0, kmask=sg, qsel=tg, flags=HEAD_RULE))
                p_self.append(ops.AttnEntrySpec(i * Bp + b, i * Bp + b, 1.0, -1.0))
                head_rows.append(i * Bp + b)
            else:
                p_ref.append(r.shifted(i * Bp, b))
                p_self.append(s_.shifted(i * Bp, b))
                head_rows.append(b)
    passes = [p_ref, p_self]
    cg = torch.tensor([0.6], dtype=torch.float32, device=gpu)
    kind = "x3p" if mode == "x3" else "bf16p"
    ref = ref_passes(q, k, v, heads, D ** -0.5, passes, cg, kind, head_rows=head_rows)
    # the rows matter: the rule on the absolute output rows instead gives a result far outside the gate
    wrong = ref_passes(q, k, v, heads, D ** -0.5, passes, cg, kind, head_rows=list(range(K * Bp)))
    assert relerr(wrong, ref) > 20 * TOL[kind]
    launches, outs = {}, {}
    own = ops.attn_row_split
    for chunk in (None, 5, 7):
        if chunk is not None:
            monkeypatch.setattr(ops, "attn_row_split", lambda Bo, wg, maxb, cus, n=chunk: n)
        try:
            outs[chunk], prof = run_profiled(q, k, vt, heads, D ** -0.5, passes, w_dev=cg, x3=mode == "x3")
        finally:
            monkeypatch.setattr(ops, "attn_row_split", own)
        assert set(prof) == ROWSPLIT_KERNELS[mode], prof
        launches[chunk] = sum(d["calls"] for n, d in prof.items() if n != PRESPLIT)
        e = check(outs[chunk], ref, TOL[kind], (mode, chunk))
        print(f"image-batched TCA rows {mode}, chunk {chunk}: {e:.2e}, {launches[chunk]} launches")
    assert launches[5] == 5 and launches[7] == 4, launches
    assert torch.equal(outs[5], outs[None]) and torch.equal(outs[7], outs[None])


# ---------------------------------------------------------------------------------------------------------------------------------------
# F. the pass table itself, through each of the five multi-pass kernels at the smallest shape it takes
# ---------------------------------------------------------------------------------------------------------------------------------------
# (mode, S, Sk, out_pair): S = 40 / Sk = 72 leaves attn_kernel and attn_x3_kernel a ragged query block and a ragged last key tile; S = 128 / Sk = 64 is
# the smallest launch of the ping-pong kernels (one query block, one key tile)
TABLE_PARAMS = ([("f32", 40, 72, False), ("bf16", 40, 72, False), ("x3", 40, 72, False), ("x3", 40, 72, True), ("bf16", 128, 64, False)] +
                [(m, 128, 64, pair) for m in ("x3", "x3-inkernel") for pair in (False, True)])


def _table_kernels(mode, Sk):
    if Sk % 64:
        return {"f32": {F32_K}, "bf16": {bf16_k(True)}, "x3": {tk("attn_x3_kernel", True)}}[mode]
    return {"bf16": {tk("attn_pp_kernel", True)}, "x3": {PRESPLIT, tk("attn_x3w_kernel", True)}, "x3-inkernel": {tk("attn_x3p_kernel", True)}}[mode]


@pytest.mark.parametrize("mode,S,Sk,out_pair", TABLE_PARAMS)
def test_pass_table_at_smallest_shapes(gpu, monkeypatch, mode, S, Sk, out_pair):
    """one two-pass table of three output rows that takes a kernel through every branch of the pass-table helpers (attention.h), against ref_passes:
    row 0: a masked entry whose tiled-head rule is pinned to row 1 (hr_row: not the output row), blended through w_dev with its own plain attention;
    row 1: a self-referencing row (both passes q = kv = 1): on the heads the rule leaves unmasked its second pass is folded into the first;
    row 2: no active entry (skipped in pass 1, zero weight in pass 2): exact zeros, also in the pair form of the split-bf16 kernels.
    Three heads, not two: with an even head count the parity of row * heads + head does not depend on the row, and the pin could not be told from
    the output row (the reference evaluated on the output rows instead must miss the gate)."""
    from freefine_amd import ops
    from test_ops_gpu import pair_value
    g = torch.Generator().manual_seed(S + Sk)
    heads, D, B = 3, 64, 3
    C = heads * D
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    q, k, v = (torch.randn(B, n, C, generator=g).to(gpu, dt) for n in (S, Sk, Sk))
    vt = ops.transpose(v, ld_dst=(Sk + 7) // 8 * 8)
    km = (torch.rand(Sk, generator=g) > 0.5).to(torch.uint8).to(gpu)
    qs = (torch.rand(S, generator=g) > 0.5).to(torch.uint8).to(gpu)
    p0 = [ops.AttnEntrySpec(0, 1, 0.0, 1.0, kmask=km, qsel=qs, flags=HEAD_RULE, hr_row=1),
          ops.AttnEntrySpec(1, 1, 0.0, 1.0, kmask=km, qsel=qs, flags=HEAD_RULE), None]
    p1 = [ops.AttnEntrySpec(0, 0, 1.0, -1.0), ops.AttnEntrySpec(1, 1, 1.0, -1.0), ops.AttnEntrySpec(2, 2, 0.0, 0.0)]
    passes = [p0, p1]
    cg = torch.tensor([0.35], dtype=torch.float32, device=gpu)
    if mode == "x3-inkernel":
        monkeypatch.setattr(ops, "_ATTN_PRESPLIT", False)
    out, names = run(q, k, vt, heads, D ** -0.5, passes, Sk=Sk, w_dev=cg, x3=mode.startswith("x3"), out_pair=out_pair)
    assert names == _table_kernels(mode, Sk), names
    if out_pair:
        assert out.dtype == torch.bfloat16 and out.shape == (B, S, 2 * C)
        out = pair_value(out, C)
    kind = operand_kind(names)
    ref = ref_passes(q, k, v, heads, D ** -0.5, passes, cg, kind)
    wrong = ref_passes(q, k, v, heads, D ** -0.5, passes, cg, kind, head_rows=[0, 1, 2])
    assert relerr(wrong[0], ref[0]) > 20 * TOL[kind]
    e = check(out, ref, TOL[kind], (mode, S, Sk, out_pair))
    print(f"pass table {mode} S={S} Sk={Sk} pair={out_pair} ({kind}): {e:.2e}")


def test_every_kernel_kind_is_expected():
    """the cases of this module expect, together, every kernel kind of the plan (from the tables the tests assert against)"""
    names = set()
    for c, Sk, masked, npass, multi in SPIKE_CASES:
        for m in ("f32", "bf16", "x3", "x3-inkernel"):
            names |= _expected(m, Sk, masked, npass, multi)
    for *_, presplit in TCA_PARAMS:
        names |= _tca_kernels(presplit)
    for v in list(UNIFORM_KERNELS.values()) + list(ROWSPLIT_KERNELS.values()):
        names |= v
    for kind in KINDS:
        assert any(kind in n for n in names), kind
