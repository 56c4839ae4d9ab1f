"""GPU: the CLIP text tower on the project's kernels -- the causal attention kernel, the quick_gelu epilogue (and erf-GELU in split-bf16), the token
embedding lookup, each against fp64 at the per-op tolerances of tests/test_ops_gpu.py / tests/test_attention_edges_gpu.py; then the whole
HipCLIPTextEncoder against transformers' CLIPTextModel.double() on the CPU (the class the reference calls, /root/reference/src/demo/model.py:536-567) at both
Stable-Diffusion shapes and full depth, with bounds computed inside the test from reference runs of the same weights and prompts; bit-identity per
prompt; graph capture; the pipeline switch.  All weights are seeded random at the checkpoints' shapes (no checkpoints exist offline)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from test_attention_edges_gpu import TOL as ATT_TOL
from test_ops_gpu import X3_ATT_TOL, X3_TOL, pair_value, ref_attention, relerr, tol
from test_text_native_cpu import PROMPTS, clip_tokens, scale_err, tower_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["f32", "x3", "bf16"]
assert ATT_TOL["f32"] == 2e-5 and ATT_TOL["bf16"] == 1.5e-2 and ATT_TOL["x3"] == X3_ATT_TOL


def mode_dtype(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def make_qkv(B, S, heads, mode, gpu, seed, ldvt=None):
    """q | k in one [B, S, 2C] buffer like the tower's fused projection, V^T [B, C, ldvt] with zeroed padding, and the fp64 values of what the device holds"""
    g = torch.Generator().manual_seed(seed)
    C, dt = heads * 64, mode_dtype(mode)
    qk = torch.randn(B, S, 2 * C, generator=g).to(dt)
    v = torch.randn(B, S, C, generator=g).to(dt)
    ldvt = ldvt or (S + 7) // 8 * 8
    vt = torch.zeros(B, C, ldvt, dtype=dt)
    vt[:, :, :S] = v.transpose(1, 2)
    return qk.to(gpu), vt.to(gpu), qk[..., :C].double(), qk[..., C:].double(), v.double()


def causal_ref(q, k, v, heads):
    S = q.shape[0]
    allowed = torch.ones(S, S, dtype=torch.bool).tril()[None].expand(heads, S, S)
    return ref_attention(q, k, v, heads, 0.125, allowed)


def run_causal(qk, vt, heads, mode, out_pair=False):
    from freefine_amd import ops
    C = heads * 64
    return ops.attention(qk, qk[..., C:], vt, heads, 0.125, None, Sk=qk.shape[1], C=C, x3=mode == "x3", out_pair=out_pair, causal=True)


@pytest.mark.parametrize("S", [1, 16, 33, 77, 96])
@pytest.mark.parametrize("mode", MODES)
def test_causal_attention_vs_fp64(gpu, mode, S):
    """every mode x sequence length x heads in {1, 12, 16} x rows in {1, 3, 17} (17 rows: two launches over row ranges); bf16 against the bf16-rounded inputs"""
    worst = 0.0
    for heads in (1, 12, 16):
        for B in (1, 3, 17):
            qk, vt, q, k, v = make_qkv(B, S, heads, mode, gpu, 1000 * S + 10 * heads + B)
            out = run_causal(qk, vt, heads, mode)
            assert out.shape == (B, S, heads * 64) and out.dtype == mode_dtype(mode)
            pair = run_causal(qk, vt, heads, mode, out_pair=True) if mode == "x3" else None
            for b in range(B):
                ref = causal_ref(q[b], k[b], v[b], heads)
                e = relerr(out[b], ref)
                worst = max(worst, e)
                assert e < ATT_TOL[mode], (mode, S, heads, B, b, e)
                if pair is not None:      # the pair rows carry the same values to 16-17 bits
                    assert relerr(pair_value(pair[b], heads * 64), ref) < ATT_TOL[mode], (S, heads, B, b)
    print(f"causal attention {mode} S={S}: worst {worst:.2e} (tolerance {ATT_TOL[mode]:.1e})")


@pytest.mark.parametrize("mode", MODES)
def test_causality_and_padding(gpu, mode):
    heads, B, S = 12, 3, 77
    C = heads * 64
    qk, vt, q, k, v = make_qkv(B, S, heads, mode, gpu, 7)
    out = run_causal(qk, vt, heads, mode)
    # row 0 sees key 0 only: it IS V[0]
    assert relerr(out[:, 0], v[:, 0]) < ATT_TOL[mode]
    # K and V at positions > q0 do not reach output rows <= q0, bit for bit
    for q0 in (0, 15, 16, 40, 75):
        qk2, vt2 = qk.clone(), vt.clone()
        qk2[:, q0 + 1:, C:] = 37.0
        vt2[:, :, q0 + 1:] = -1e3
        out2 = run_causal(qk2, vt2, heads, mode)
        assert torch.equal(out2[:, :q0 + 1], out[:, :q0 + 1]), (mode, q0)
        assert not torch.equal(out2[:, q0 + 1:], out[:, q0 + 1:])
    # V^T padding columns (ldvt 80 for 77 keys) never reach the result
    vt3 = vt.clone()
    vt3[:, :, S:] = 1e4
    assert torch.equal(run_causal(qk, vt3, heads, mode), out)
    # a wider V^T row (ldvt 96: the last key-fragment pair lies inside the row) as well
    qk4, vt4, *_ = make_qkv(B, S, heads, mode, gpu, 7, ldvt=96)
    vt4[:, :, S:] = 1e4
    assert torch.equal(run_causal(qk4, vt4, heads, mode), out)


def test_unacceptable_causal_descriptors_launch_nothing(gpu):
    from freefine_amd import _lib, ops
    lib = _lib.load()
    heads, S = 12, 77
    C = heads * 64
    big = torch.zeros(2, 128, 2 * C, device=gpu)
    vt = torch.zeros(2, C, 128, device=gpu)
    out = torch.full((2 * 128, C), 5.0, device=gpu)
    km = torch.ones(128, dtype=torch.uint8, device=gpu)

    def desc(S=S, Sk=S, npass=1, kv_pair=0, kmask=None, flags=_lib.ATT_CAUSAL):
        d = _lib.AttnDesc()
        d.q, d.k, d.vt, d.out = big.data_ptr(), big.data_ptr() + C * 4, vt.data_ptr(), out.data_ptr()
        d.Bo, d.S, d.Sk, d.heads, d.D, d.npass, d.kv_pair, d.scale = 2, S, Sk, heads, 64, npass, kv_pair, 0.125
        d.ldq = d.ldk = 2 * C
        d.ldo, d.ldvt = C, 128
        for p in range(npass):
            for b in range(2):
                e = d.e[p * _lib.ATT_MAXB + b]
                e.q_row = e.kv_row = b
                e.w_const, e.flags, e.kmask = 1.0, flags, (0 if kmask is None else kmask.data_ptr())
        return d
    stream = torch.cuda.current_stream().cuda_stream
    for dtype in (_lib.FFN_F32, _lib.FFN_BF16, _lib.FFN_BF16X3):
        for d in (desc(S=64, Sk=77), desc(S=128, Sk=128), desc(kmask=km), desc(npass=2), desc(kv_pair=1)):
            assert lib.ffn_attn(stream, dtype, ctypes.byref(d)) == -22
            assert b"FFN_ATT_CAUSAL" in lib.ffn_last_error()
    torch.cuda.synchronize()
    assert (out == 5.0).all()                           # nothing was launched
    assert lib.ffn_attn(stream, _lib.FFN_F32, ctypes.byref(desc())) == 0
    torch.cuda.synchronize()
    assert (out[:2 * S] == 0.0).all() and (out[2 * S:] == 5.0).all()        # (zero operands -> zero rows; nothing beyond the 2 x S output rows is touched)
    # a descriptor without the flag plans what it planned before the flag existed
    buf = ctypes.create_string_buffer(160)
    for dtype, want in ((_lib.FFN_F32, b"attn_kernel<float, 64, 2, 64, 1, true>"), (_lib.FFN_BF16, b"xattn_kernel<5>"), (_lib.FFN_BF16X3, b"xattn_x3_kernel<5, 4>")):
        assert lib.ffn_attn_kernel_name(dtype, ctypes.byref(desc(flags=0)), buf, 160) == 0 and want in buf.value, buf.value
    with pytest.raises(_lib.FreeFineHipError, match="FFN_ATT_CAUSAL"):
        ops.attention(big[:, :64], big[:, :77, C:], vt, heads, 0.125, None, Sk=77, C=C, causal=True)


@pytest.mark.parametrize("N,K", [(3072, 768), (4096, 1024)])
@pytest.mark.parametrize("M", [77, 77 * 24])
def test_qgelu_and_x3_gelu_epilogues(gpu, M, N, K):
    from freefine_amd import ops
    g = torch.Generator().manual_seed(M + N)
    x32 = torch.randn(M, K, generator=g)
    w32 = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g)
    quick = lambda y: y * torch.sigmoid(1.702 * y)
    for mode in MODES:
        dt = mode_dtype(mode)
        x, w = x32.to(dt), w32.to(dt)
        y = x.double() @ w.double().t() + b.double()
        wp = ops.pack_linear(w.to(gpu), dt, x3=mode == "x3")
        bound = X3_TOL if mode == "x3" else tol(dt)
        out = ops.linear(x.to(gpu), wp, b.to(gpu), K=K, qgelu=True, splitk=1)
        e = relerr(out, quick(y))
        print(f"qgelu {mode} M={M} N={N} K={K}: {e:.2e} (tolerance {bound:.1e})")
        assert e < bound
        if mode == "x3":
            e = relerr(ops.linear(x.to(gpu), wp, b.to(gpu), K=K, gelu=True, splitk=1), torch.nn.functional.gelu(y))
            print(f"gelu  x3 M={M} N={N} K={K}: {e:.2e}")
            assert e < X3_TOL
            for kw in (dict(qgelu=True), dict(gelu=True)):          # the pair rows fc2 reads
                p = ops.linear(x.to(gpu), wp, b.to(gpu), K=K, out_pair=True, splitk=1, **kw)
                assert relerr(pair_value(p, N), quick(y) if "qgelu" in kw else torch.nn.functional.gelu(y)) < X3_TOL


def test_embed_tokens_is_exact(gpu):
    from freefine_amd import ops
    g = torch.Generator().manual_seed(11)
    V, S, C, N = 49408, 77, 768, 5
    table, pos = torch.randn(V, C, generator=g), torch.randn(S, C, generator=g) * 0.3
    ids = torch.randint(0, V, (N, S), generator=g)
    ids[0, :3] = torch.tensor([0, V - 1, V - 2])
    want = table[ids] + pos
    idd, td, pd = ids.to(gpu, torch.int32), table.to(gpu), pos.to(gpu)
    assert torch.equal(ops.embed_tokens(idd, td, pd, torch.float32).cpu(), want)
    assert torch.equal(ops.embed_tokens(idd, td, pd, torch.bfloat16).cpu(), want.to(torch.bfloat16))
    short = ops.embed_tokens(idd[:, :33].contiguous(), td, pd, torch.float32)
    assert torch.equal(short.cpu(), want[:, :33])


# ---------------------------------------------------------------------------------------------------------------------
# the whole tower
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}


def tower_case(dim):
    """per shape, once: the transformers module (full depth, seeded), token ids, its fp64 output, and the reference errors the bounds are made of"""
    if dim not in _REF:
        from freefine_amd.text import clip_shaped_text_encoder, text_config
        enc = clip_shaped_text_encoder(dim)
        cfg = text_config(enc.config)
        ids = clip_tokens(PROMPTS)
        state = {k: v.detach().clone() for k, v in enc.state_dict().items()}
        with torch.no_grad():
            got32 = enc(ids)[0].double()
            want = enc.double()(ids)[0]
            enc.float()
        errs = {"f32": scale_err(got32, want), "x3": scale_err(tower_ref(cfg, state, ids, "x3"), want), "bf16": scale_err(tower_ref(cfg, state, ids, "bf16"), want)}
        _REF[dim] = dict(cfg=cfg, state=state, ids=ids, want=want, errs=errs, native={})
    return _REF[dim]


def native(dim, mode, gpu):
    from freefine_amd.text import HipCLIPTextEncoder
    c = tower_case(dim)
    if mode not in c["native"]:
        c["native"][mode] = HipCLIPTextEncoder(c["cfg"], c["state"], dtype=mode_dtype(mode), device=gpu, x3=mode == "x3")
    return c["native"][mode]


def tower_bound(errs, mode):
    """f32: 8 x the error of CLIPTextModel in fp32 on the CPU against fp64 (what the depth network, same kernels and depth, shows against its fp32-derived
    references), never above the per-op 2e-5; x3 / bf16: 2 x the error of the CPU emulation of that arithmetic (which sums in fp64 where the kernels sum in
    fp32 in 16- or 32-key / 32- or 64-element steps).  The bf16 emulation keeps EVERY activation in bf16 between two ops, the residual stream included, because
    that is what the project's fast mode stores (bf16 [B, S, C] tensors, fp32 only inside a kernel); an emulation with an fp32 residual stream would show about a
    third of that error and is not the arithmetic this mode runs."""
    return min(8 * errs["f32"], 2e-5) if mode == "f32" else 2 * errs[mode]


# measured on the MI355X (profiles/text_encoder_parity.txt), error over the output maximum against CLIPTextModel.double() | the bound = factor x reference error:
#   1024 / 23 layers / gelu:        f32 2.12e-6 | 8 x 7.21e-7 = 5.77e-6    x3 1.32e-5 | 2 x 1.39e-5 = 2.77e-5    bf16 2.21e-2 | 2 x 2.27e-2 = 4.54e-2
#   768 / 12 layers / quick_gelu:   f32 1.97e-6 | 8 x 7.08e-7 = 5.67e-6    x3 1.42e-5 | 2 x 1.46e-5 = 2.91e-5    bf16 1.48e-2 | 2 x 1.73e-2 = 3.46e-2
# (the reference errors differ from run to run of the CPU library only in their last digits; the prompts here are longer than a typical caption, which is why the
# emulations' errors sit above the figures of a short-prompt probe)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dim", [1024, 768])
def test_encoder_vs_cliptextmodel_fp64(gpu, dim, mode):
    c = tower_case(dim)
    out = native(dim, mode, gpu)(c["ids"])[0]
    assert out.shape == c["want"].shape and out.dtype == torch.float32 and out.is_cuda
    e, bound = scale_err(out, c["want"]), tower_bound(c["errs"], mode)
    line = f"text tower {dim} {mode}: error {e:.3e} of the output maximum; bound {bound:.3e} (reference errors: " + \
           ", ".join(f"{k} {v:.3e}" for k, v in c["errs"].items()) + ")"
    print(line)
    if os.environ.get("FFN_TEXT_PARITY_OUT"):            # (how profiles/text_encoder_parity.txt is written)
        with open(os.environ["FFN_TEXT_PARITY_OUT"], "a") as f:
            f.write(line + "\n")
    assert e <= bound, line


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dim", [1024, 768])
def test_encoder_is_bit_identical_whatever_is_beside_a_prompt(gpu, dim, mode):
    c = tower_case(dim)
    enc, ids = native(dim, mode, gpu), c["ids"]
    together = enc(ids)[0]
    for j in range(3):
        assert torch.equal(enc(ids[j:j + 1])[0][0], together[j]), (dim, mode, j)
    others = clip_tokens([f"filler prompt number {i}" for i in range(21)])
    for at in ((0, 1, 2), (3, 4, 5), (2, 11, 23)):
        batch = torch.empty(24, 77, dtype=torch.int64)
        rest = [i for i in range(24) if i not in at]
        batch[rest] = others
        batch[list(at)] = ids
        got = enc(batch)[0]
        assert got.shape[0] == 24
        for j, pos in enumerate(at):
            assert torch.equal(got[pos], together[j]), (dim, mode, at, j)


@pytest.mark.parametrize("mode", MODES)
def test_encoder_call_is_capturable(gpu, mode):
    c = tower_case(768)
    enc = native(768, mode, gpu)
    ids = c["ids"].to(gpu)
    eager = enc(ids)[0].clone()                          # warm: every GEMM shape tuned before capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = enc(ids)[0]
    cap.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager)


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline switch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [None, "gelu"])
def test_pipeline_native_text(gpu, tmp_path, act):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_checkpoint as M
    from transformers import CLIPTextModel
    from golden_cases import edit_cases, mask_inputs, synth_images
    from test_pipeline_gpu import TOL, _hook_edit
    from freefine_amd.pipeline import FreeFinePipeline
    from freefine_amd.text import HipCLIPTextEncoder
    d = str(tmp_path / "sd_tiny")
    M.write(d, "tiny", "tiny", "fp32", seed=5, text_heads=1, text_act=act)
    a = _hook_edit(FreeFinePipeline.from_pretrained(d, torch_dtype=torch.float32, device=gpu, native_text=True).to(gpu))
    b = _hook_edit(FreeFinePipeline.from_pretrained(d, torch_dtype=torch.float32, device=gpu).to(gpu))
    assert isinstance(a.text_encoder, HipCLIPTextEncoder) and isinstance(b.text_encoder, torch.nn.Module)
    assert a.share().text_encoder is a.text_encoder
    prompts = ["a photo of a cup", "", "a red chair beside a window"]
    ea, eb = a._encode_text(prompts), b._encode_text(prompts)
    assert a.text_encoder_calls == 1 and b.text_encoder_calls == 3
    # the bound of the tower test, from this folder's weights: CLIPTextModel fp32 on the CPU against fp64
    mod = CLIPTextModel.from_pretrained(os.path.join(d, "text_encoder")).eval()
    ids = a.tokenizer(prompts, padding="max_length", max_length=77, return_tensors="pt").input_ids
    with torch.no_grad():
        got32 = mod(ids)[0].double()
        want = mod.double()(ids)[0]
    bound = tower_bound({"f32": scale_err(got32, want)}, "f32")
    e_ref, e_tr = scale_err(ea, want), scale_err(ea, eb)
    print(f"pipeline text ({act or 'quick_gelu'}): native vs fp64 {e_ref:.2e}, native vs transformers path {e_tr:.2e}, bound {bound:.2e}")
    assert e_ref <= bound and e_tr <= bound
    ori_img, coarse, _ = synth_images()
    ori, tgt, *_ = mask_inputs()
    kw = dict(edit_cases()[0][2])
    kw.pop("guidance_text")
    gs, eta = kw.pop("guidance_scale"), kw.pop("eta")
    kw.update(seed=42, return_intermediates=True, verbose=False)
    ia = a.FreeFine_generation(ori_img, ori, coarse, tgt, "a photo of a cup", gs, eta, **kw)
    ib = b.FreeFine_generation(ori_img, ori, coarse, tgt, "a photo of a cup", gs, eta, **kw)
    assert len(a.last_intermediates) == len(b.last_intermediates) > 0
    worst = max((x.float() - y.float()).abs().max().item() for x, y in zip(a.last_intermediates, b.last_intermediates))
    print(f"  edit with the native encoder vs the transformers encoder: latent L-inf {worst:.2e}")
    assert worst <= TOL and np.isfinite(ia.astype(float)).all() and np.abs(ia.astype(int) - ib.astype(int)).max() <= 1
