"""GPU: the ImageReward score on the project's kernels -- the two entries it adds (ffn_embed_tokens_ln bit for bit against ffn_layernorm of ffn_embed_tokens,
ffn_affine_chain against fp64), the attention kernels at the shapes of a key-padding-masked 35-token self-attention and of a cross-attention to 197 image tokens,
both towers against transformers' BlipVisionModel / BlipTextModel in fp64 (bounds by tower_bound's rule from reference runs of the same weights and inputs),
padding independence, the score and the drivers.  All weights are drawn (no ImageReward checkpoint exists offline); full WIDTH at 2 layers: no test runs the
24 / 12-layer depth."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import irs_ref
from test_attention_edges_gpu import TOL as ATT_TOL
from test_irs_cpu import CAPTIONS, LIVE, TEXT_CASES, VISION_CASES, host_rewards, score_case, smooth_images, text_case, text_errs, tiny_state, vision_case, vision_errs
from test_ops_gpu import pair_value, ref_attention, relerr
from test_text_native_cpu import scale_err
from test_text_native_gpu import tower_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["f32", "x3", "bf16"]


def mode_dtype(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# ffn_embed_tokens_ln
# ---------------------------------------------------------------------------------------------------------------------
def embed_inputs(N, S, C, V, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (N, S), generator=g, dtype=torch.int32)
    ids.view(-1)[0], ids.view(-1)[-1] = V - 1, 0
    table, pos = torch.randn(V, C, generator=g), 0.3 * torch.randn(40, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return ids, table, pos, gamma, beta, [t.to(gpu) for t in (ids, table, pos, gamma, beta)]


@pytest.mark.parametrize("C", [128, 768])
def test_embed_tokens_ln_equals_the_two_step_form(gpu, C):
    """S in {1, 35} x N in {1, 3}, ids holding 0 and V - 1: the fp32 output is torch.equal to layernorm(embed_tokens(..., float32)); the bf16 output lies within
    one bf16 ulp of the fp64 value (plus the fp32 norm's own 2e-5 of the scale); sentinel rows around the output survive"""
    from freefine_amd import ops
    V, eps = 50, 1e-12
    for S in (1, 35):
        for N in (1, 3):
            ids, table, pos, gamma, beta, dev = embed_inputs(N, S, C, V, gpu, seed=C + 10 * S + N)
            want = ops.layernorm(ops.embed_tokens(dev[0], dev[1], dev[2], torch.float32), dev[3], dev[4], eps=eps)
            big = torch.full((N + 2, S, C), 512.0, device=gpu)
            got = ops.embed_tokens_ln(*dev, torch.float32, eps=eps, out=big[1:N + 1])
            assert torch.equal(got, want), (C, S, N, (got - want).abs().max().item())
            assert bool((big[0] == 512).all()) and bool((big[-1] == 512).all())
            ref = torch.nn.functional.layer_norm(table.double()[ids.long()] + pos.double()[:S], (C,), gamma.double(), beta.double(), eps)
            assert relerr(got, ref) < 2e-5
            low = ops.embed_tokens_ln(*dev, torch.bfloat16, eps=eps)
            assert low.dtype == torch.bfloat16 and low.shape == (N, S, C)
            ulp = torch.exp2(torch.frexp(ref.abs())[1].double() - 8)
            over = ((low.double().cpu() - ref).abs() - ulp - 2e-5 * ref.abs().max()).max().item()
            assert over <= 0, (C, S, N, over)


def test_embed_tokens_ln_constant_row_gives_beta(gpu):
    """a row whose sum is the same value everywhere (0.25 + 0.25: every partial sum exact) has variance 0; at eps = 1e-12 the result is beta, bit for bit"""
    from freefine_amd import ops
    for C in (128, 768):
        g = torch.Generator().manual_seed(C)
        table, pos = torch.full((7, C), 0.25, device=gpu), torch.full((40, C), 0.25, device=gpu)
        gamma, beta = (1 + torch.randn(C, generator=g)).to(gpu), torch.randn(C, generator=g).to(gpu)
        ids = torch.randint(0, 7, (3, 35), generator=g, dtype=torch.int32).to(gpu)
        out = ops.embed_tokens_ln(ids, table, pos, gamma, beta, torch.float32, eps=1e-12)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, beta.expand(3, 35, C))
        low = ops.embed_tokens_ln(ids, table, pos, gamma, beta, torch.bfloat16, eps=1e-12)
        assert torch.equal(low, beta.to(torch.bfloat16).expand(3, 35, C))


def test_embed_tokens_ln_refuses_bad_descriptors(gpu):
    from freefine_amd import _lib
    lib = _lib.load()
    N, S, C, V = 2, 35, 128, 50
    ids = torch.zeros(N * S + 8, dtype=torch.int32, device=gpu)
    table, pos = torch.randn(V, 2048, device=gpu), torch.randn(40, 2048, device=gpu)
    gamma, beta = torch.ones(2048, device=gpu), torch.zeros(2048, device=gpu)
    out = torch.full((N * S, 2048), 512.0, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    base = dict(stream=s, dtype=0, ids=ids.data_ptr(), table=table.data_ptr(), pos=pos.data_ptr(), out=out.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                M=N * S, S=S, C=C, V=V, eps=1e-12)
    call = lambda **kw: lib.ffn_embed_tokens_ln(*{**base, **kw}.values())
    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(512.0)
    bad = [dict(ids=None), dict(table=None), dict(pos=None), dict(out=None), dict(gamma=None), dict(beta=None), dict(table=table.data_ptr() + 4),
           dict(out=out.data_ptr() + 8), dict(ids=ids.data_ptr() + 2), dict(M=0), dict(S=0), dict(V=0), dict(C=0), dict(C=130), dict(C=1540), dict(dtype=1, C=132),
           dict(dtype=2), dict(dtype=3)]
    for kw in bad:
        assert call(**kw) == -22 and b"embed_tokens_ln" in lib.ffn_last_error(), (kw, lib.ffn_last_error())
    torch.cuda.synchronize()
    assert bool((out == 512).all()), "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------------
# ffn_affine_chain
# ---------------------------------------------------------------------------------------------------------------------
def chain_layers(dims, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, k, generator=g) / k ** 0.5, 0.1 * torch.randn(n, generator=g)) for k, n in zip(dims[:-1], dims[1:])]


@pytest.mark.parametrize("dims", [(768, 1024, 128, 64, 16, 1), (8, 1), (1024, 1024), (5, 3, 1)])
def test_affine_chain_vs_fp64(gpu, dims):
    """B in {1, 3, 33}, rows ldx = dims[0] + 5 apart: within irs_ref.chain_tol of the fp64 chain; rows 0 and 2 are equal and give equal bits, and a row's bits
    do not depend on B"""
    from freefine_amd import ops
    layers = chain_layers(dims, seed=len(dims) + dims[0])
    params, got_dims = ops.affine_chain_params(layers)
    assert got_dims == list(dims)
    params = params.to(gpu)
    ldx = dims[0] + 5
    x = torch.randn(33, ldx, generator=torch.Generator().manual_seed(dims[0]))
    x[2] = x[0]
    xd = x.to(gpu)
    a = x[:, :dims[0]].double()
    for w, b in layers:
        a = a @ w.double().t() + b.double()
    want = (a - 0.3) / 1.7
    tol = irs_ref.chain_tol(layers, x[:, :dims[0]], 0.0, 1.7)
    first = None
    for B in (1, 3, 33):
        out = ops.affine_chain(xd, params, dims, 0.3, 1.7, ldx=ldx, B=B)
        assert out.shape == (B, dims[-1]) and out.dtype == torch.float32
        err = (out.double().cpu() - want[:B]).abs().max(1).values
        print(f"affine_chain {dims} B={B}: max error {err.max():.2e} (tolerance {tol[:B].max():.2e})")
        assert bool((err <= tol[:B]).all()), (dims, B, err.max().item(), tol.max().item())
        first = out if first is None else first
        assert torch.equal(out[:1], first[:1]) and (B < 3 or torch.equal(out[2], out[0]))
        assert torch.equal(ops.affine_chain(xd, params, dims, 0.3, 1.7, ldx=ldx, B=B), out), "two runs are bit-equal"
    dense = ops.affine_chain(xd[:, :dims[0]].contiguous(), params, dims, 0.3, 1.7)
    assert torch.equal(dense, out)


def test_affine_chain_refuses_bad_descriptors(gpu):
    import ctypes
    from freefine_amd import _lib
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    x, params = torch.randn(4, 2048, device=gpu), torch.randn(1025 * 1026 + 64, device=gpu)
    out = torch.full((4, 1025), 512.0, device=gpu)
    dims = lambda *d: (ctypes.c_int * len(d))(*d)
    call = lambda d, L, B=4, ldx=2048, xp=x.data_ptr(), pp=params.data_ptr(), op=out.data_ptr(), scale=1.0: lib.ffn_affine_chain(s, xp, pp, op, B, ldx, d, L, 0.0, scale)
    assert call(dims(8, 3, 1), 2) == 0
    torch.cuda.synchronize()
    out.fill_(512.0)
    bad = [call(dims(1025, 1), 1), call(dims(8, 1025, 1), 2), call(dims(8, 0), 1), call(dims(*([4] * 10)), 9), call(dims(8), 0), call(dims(8, 1), 1, B=0),
           call(dims(8, 1), 1, ldx=7), call(dims(8, 1), 1, xp=0), call(dims(8, 1), 1, pp=0), call(dims(8, 1), 1, op=0), call(dims(8, 1), 1, xp=x.data_ptr() + 2),
           call(dims(8, 1), 1, scale=0.0), lib.ffn_affine_chain(s, x.data_ptr(), params.data_ptr(), out.data_ptr(), 4, 2048, None, 1, 0.0, 1.0)]
    assert bad == [-22] * len(bad) and b"affine_chain" in lib.ffn_last_error(), bad
    torch.cuda.synchronize()
    assert bool((out == 512).all()), "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------------
# the attention kernels at the text tower's shapes: existing kernels, shapes no other test covers
# ---------------------------------------------------------------------------------------------------------------------
def attn_out(out, C, mode):
    return pair_value(out, C) if mode == "x3" else out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("heads", [2, 12])
def test_key_masked_self_attention_at_35_tokens(gpu, heads, mode):
    """S = Sk = 35, head dim 64, q | k in one buffer, V^T padded to 40 with zeros; one row per mask with 1, 2, 9, 34 and 35 live keys (one uint8 buffer each, 36
    bytes apart); the masked keys' K and V rows hold +-1e4: a kernel that let one through would be off by orders of magnitude"""
    from freefine_amd import ops
    S, live = 35, (1, 2, 9, 34, 35)
    B, C, dt = len(live), heads * 64, mode_dtype(mode)
    g = torch.Generator().manual_seed(100 * heads + len(mode))
    qk, v = torch.randn(B, S, 2 * C, generator=g), torch.randn(B, S, C, generator=g)
    km = torch.zeros(B, 36, dtype=torch.uint8)
    for b, n in enumerate(live):
        km[b, :n] = 1 + b                                   # any non-zero byte marks a live key
        qk[b, n:, C:] = 1e4 * torch.sign(qk[b, n:, C:])
        v[b, n:] = -1e4 * torch.sign(v[b, n:])
    qk, v = qk.to(dt), v.to(dt)
    vt = torch.zeros(B, C, 40, dtype=dt)
    vt[:, :, :S] = v.transpose(1, 2)
    qkd, kmd = qk.to(gpu), km.to(gpu)
    passes = [[ops.AttnEntrySpec(b, b, kmask=kmd[b]) for b in range(B)]]
    out = ops.attention(qkd, qkd[..., C:], vt.to(gpu), heads, 0.125, passes, Sk=S, C=C, x3=mode == "x3", out_pair=mode == "x3")
    worst = 0.0
    for b, n in enumerate(live):
        allowed = (torch.arange(S) < n)[None, None].expand(heads, S, S)
        e = relerr(attn_out(out[b], C, mode), ref_attention(qk[b, :, :C].double(), qk[b, :, C:].double(), v[b].double(), heads, 0.125, allowed))
        worst = max(worst, e)
        assert e < ATT_TOL[mode], (mode, heads, n, e)
    print(f"masked self-attention S=35 {mode} heads={heads}: worst {worst:.2e} (tolerance {ATT_TOL[mode]:.1e})")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Sk", [10, 197])
def test_cross_attention_to_another_sequence(gpu, Sk, mode):
    """S = 35 queries, Sk in {10, 197} keys (ldvt 16 / 200, padding zero), heads in {2, 12}, 3 rows; K is a column view of a three-layer-wide buffer as
    encoder.cross_kv hands it over"""
    from freefine_amd import ops
    S, B, dt = 35, 3, mode_dtype(mode)
    ld = (Sk + 7) // 8 * 8
    assert ld == {10: 16, 197: 200}[Sk]
    worst = 0.0
    for heads in (2, 12):
        C = heads * 64
        g = torch.Generator().manual_seed(Sk + heads)
        q, kw, v = (torch.randn(B, S, C, generator=g).to(dt), torch.randn(B, Sk, 3 * C, generator=g).to(dt), torch.randn(B, Sk, C, generator=g).to(dt))
        vt = torch.zeros(B, C, ld, dtype=dt)
        vt[:, :, :Sk] = v.transpose(1, 2)
        kd = kw.to(gpu)[..., C:2 * C]
        out = ops.attention(q.to(gpu), kd, vt.to(gpu), heads, 0.125, None, Sk=Sk, C=C, x3=mode == "x3", out_pair=mode == "x3")
        for b in range(B):
            e = relerr(attn_out(out[b], C, mode), ref_attention(q[b].double(), kw[b, :, C:2 * C].double(), v[b].double(), heads, 0.125))
            worst = max(worst, e)
            assert e < ATT_TOL[mode], (mode, Sk, heads, b, e)
    print(f"cross-attention S=35 Sk={Sk} {mode}: worst {worst:.2e} (tolerance {ATT_TOL[mode]:.1e})")


# ---------------------------------------------------------------------------------------------------------------------
# the towers against transformers in fp64
# ---------------------------------------------------------------------------------------------------------------------
def report(line):
    print(line)
    if os.environ.get("FFN_IRS_PARITY_OUT"):            # (how profiles/irs_parity.txt is written)
        with open(os.environ["FFN_IRS_PARITY_OUT"], "a") as f:
            f.write(line + "\n")


# measured on the MI355X: profiles/irs_parity.txt
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VISION_CASES))
def test_blip_vision_vs_transformers_fp64(gpu, name, mode):
    """tiny16 and ViT-L/16 cut to 2 blocks at full width, B = 2, all 197 tokens against BlipVisionModel.double() on the CPU under tower_bound's rule"""
    from freefine_amd.irs import HipBlipVision
    cfg, st, x, want, _ = vision_case(name)
    errs = vision_errs(name)
    net = HipBlipVision(cfg, st, dtype=mode_dtype(mode), device=gpu, x3=mode == "x3")
    out = net(x)
    assert out.shape == want.shape and out.dtype == mode_dtype(mode) and out.is_cuda
    e, bound = scale_err(out, want), tower_bound(errs, mode)
    line = f"BLIP vision tower {name} {mode}: error {e:.3e} of the output maximum ({want.abs().max():.3f}); bound {bound:.3e} (reference errors: " + \
           ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + ")"
    report(line)
    assert e <= bound, line
    if mode == "x3":                                      # the pair rows the text tower's K / V projections read: the same values to hi + lo's 16 bits
        assert scale_err(pair_value(net(x, pair=True), cfg.embed_dim), out) < 2.0 ** -16


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TEXT_CASES))
def test_blip_text_vs_transformers_fp64(gpu, name, mode):
    """tiny and BLIP's BERT cut to 2 layers at full width (768 / 12 heads / encoder width 1024), three prompts of 3, 11 and 35 live tokens over 197 image tokens,
    row 0 against BlipTextModel.double() on the CPU under tower_bound's rule; one prompt for all images = that prompt repeated"""
    from freefine_amd.irs import HipBlipText
    cfg, st, ids, mask, embeds, want, _ = text_case(name)
    errs = text_errs(name)
    net = HipBlipText(cfg, st, dtype=mode_dtype(mode), device=gpu, x3=mode == "x3")
    ed = embeds.to(gpu, mode_dtype(mode))
    out = net(ids, mask, ed)
    assert out.shape == want.shape and out.dtype == torch.float32 and out.is_cuda
    e, bound = scale_err(out, want), tower_bound(errs, mode)
    line = f"BLIP text tower {name} {mode}: error {e:.3e} of the output maximum ({want.abs().max():.3f}); bound {bound:.3e} (reference errors: " + \
           ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + ")"
    report(line)
    assert e <= bound, line
    one = net(ids[1:2], mask[1:2], ed)
    assert torch.equal(one, net(ids[1:2].expand(3, -1), mask[1:2].expand(3, -1), ed)) and torch.equal(one[1], out[1])


@pytest.mark.parametrize("mode", MODES)
def test_padded_ids_do_not_reach_the_reward(gpu, mode):
    """other ids at the padded positions under the same mask: row 0 of the tower, and the reward behind it, keep their bits"""
    from freefine_amd import irs, ops
    cfg, st, ids, mask, embeds, _, _ = text_case("tiny")
    net = irs.HipBlipText(cfg, st, dtype=mode_dtype(mode), device=gpu, x3=mode == "x3")
    ed = embeds.to(gpu, mode_dtype(mode))
    other = torch.where(mask != 0, ids, torch.randint(1, cfg.vocab_size, ids.shape, generator=torch.Generator().manual_seed(5)))
    assert not torch.equal(other, ids) and torch.equal(other[2], ids[2])          # the 35-token prompt has no padding
    a, b = net(ids, mask, ed), net(other, mask, ed)
    assert torch.equal(a, b), (mode, (a - b).abs().max().item())
    params, dims = ops.affine_chain_params(chain_layers((cfg.hidden_size, 1024, 128, 64, 16, 1), seed=2))
    ra, rb = (ops.affine_chain(t, params.to(gpu), dims, irs.REWARD_MEAN, irs.REWARD_STD) for t in (a, b))
    assert torch.equal(ra, rb)
    live = ids.clone()
    live[0, 1] = 7 if ids[0, 1] != 7 else 8
    assert not torch.equal(net(live, mask, ed)[0], a[0]), "a live id does"


# ---------------------------------------------------------------------------------------------------------------------
# the score and the drivers
# ---------------------------------------------------------------------------------------------------------------------
_TINY = {}


def tiny_model(gpu):
    """HipImageReward of the tiny towers with the byte tokenizer in fp32 -- built once"""
    if not _TINY:
        from freefine_amd import irs, text
        _TINY["m"] = irs.HipImageReward.from_state(tiny_state()[0], text.ByteTokenizer(), "tiny16", "tiny", device=gpu)
    return _TINY["m"]


def test_score_vs_fp64_restatement(gpu):
    model = tiny_model(gpu)
    imgs, want, tols = score_case()
    got = []
    for cap in CAPTIONS:
        s = model.score_u8(imgs, cap)
        assert s.shape == (3,) and s.dtype == torch.float32 and s.is_cuda
        got.append(s.double().cpu())
    err = (torch.stack(got) - want).abs()
    print(f"ImageReward score, tiny towers: max error {err.max():.2e} (tolerance {tols.max():.2e}); rewards {want.min():.4f} .. {want.max():.4f}")
    assert bool((err <= tols).all()), (err.max().item(), tols.max().item())
    # different images and prompts give different rewards: the cross-attention and the text path are in the test
    assert (want.max(1).values - want.min(1).values).min() > 10 * tols.max() and (want.max(0).values - want.min(0).values).min() > 10 * tols.max()
    # one prompt each = the diagonal of the rows above
    each = model.score_u8(imgs, CAPTIONS)
    assert torch.equal(each.cpu(), torch.stack([model.score_u8(imgs, c)[i] for i, c in enumerate(CAPTIONS)]).cpu())
    with pytest.raises(ValueError, match="prompts"):
        model.score_u8(imgs, CAPTIONS[:2])


@pytest.mark.parametrize("mode", ["x3", "bf16"])
def test_score_in_the_other_modes_is_the_same_score(gpu, mode):
    """split-bf16 and bf16 towers (the head stays fp32) against the fp64 rewards.  Tolerance: tower_bound's rule for these modes on the two towers together --
    2 x the error of the emulated arithmetic on the text tower's row 0 -- carried through the head by irs_ref.chain_tol"""
    from test_consistency_gpu import clip_host_prepare
    from freefine_amd import irs, text
    imgs, want, _ = score_case()
    st, vcfg, tcfg = tiny_state()
    vst, tst, head = irs.split_state(st)
    model = irs.HipImageReward.from_state(st, text.ByteTokenizer(), "tiny16", "tiny", dtype=mode_dtype(mode), device=gpu, x3=mode == "x3")
    ids = text.ByteTokenizer()([CAPTIONS[0]], max_length=35).input_ids
    x = clip_host_prepare(imgs, size=224)
    _, row = irs_ref.score_ref(vcfg, vst, tcfg, tst, head, x, ids, (ids != 0).long())
    _, emu = irs_ref.score_ref(vcfg, vst, tcfg, tst, head, x, ids, (ids != 0).long(), mode)
    tol = irs_ref.chain_tol(head, row, 2 * (emu - row).abs().max().item(), irs_ref.REWARD_STD)
    err = (model.score_u8(imgs, CAPTIONS[0]).double().cpu() - want[0]).abs()
    print(f"ImageReward score, tiny towers, {mode}: max error {err.max():.2e} (tolerance {tol.max():.2e})")
    assert bool((err <= tol).all())


def write_tree(root):
    """5 PNGs of two sizes under two image entries with captions of their own"""
    from PIL import Image
    a, b = smooth_images(3, 64, 64, seed=11), smooth_images(2, 64, 96, seed=12)
    data = {"imgA": {"4v_caption": CAPTIONS[0], "instances": {"0": {"c0": {}, "c1": {}}, "1": {"c0": {}}}},
            "imgB": {"4v_caption": CAPTIONS[1], "instances": {"0": {"c0": {}, "c1": {}}}}}
    arrays = {"imgA": [a[0], b[0], a[1]], "imgB": [b[1], a[2]]}
    for key, image in data.items():
        samples = [s for inst in image["instances"].values() for s in inst.values()]
        for i, (s, arr) in enumerate(zip(samples, arrays[key])):
            s["gen_img_path"] = os.path.join(root, f"{key}_{i}.png")
            Image.fromarray(arr).save(s["gen_img_path"])
    return data, arrays


def test_calculate_irs_and_the_driver_end_to_end(gpu, tmp_path):
    from freefine_amd import metrics as FM
    model = tiny_model(gpu)
    data, arrays = write_tree(str(tmp_path))
    got = FM.calculate_irs(data, "gen_img_path", model)
    total, tol = 0.0, 0.0
    for key, image in data.items():
        for arr in arrays[key]:
            w, t = host_rewards(arr[None], [image["4v_caption"]])
            total, tol = total + w.item(), max(tol, t.item())
    want = total / 5
    print(f"calculate_irs: {got:.8f} vs host fp64 {want:.8f} (tolerance {tol:.2e})")
    assert abs(got - want) <= tol
    # the command-line driver, a process of its own
    path, weights = str(tmp_path / "results.json"), str(tmp_path / "irs_tiny.pt")
    json.dump(data, open(path, "w"))
    torch.save(tiny_state()[0], weights)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "evaluation", "metrics", "main.py"), "--path", path, "--task", "010000000", "--irs_config", "tiny",
                          "--irs_tokenizer", "bytes", "--irs_weights", weights], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("IRS: ")]
    assert len(lines) == 1 and float(lines[0][5:]) == got, (lines, got)
