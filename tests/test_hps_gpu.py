"""GPU: the Human Preference Score on the project's kernels -- the two entries it adds (ffn_pool_layernorm bit for bit against ffn_layernorm on the gathered rows,
ffn_cosine_rows against fp64), the generic attention kernels at the 80-wide heads of ViT-H/14, both towers against transformers' CLIP*ModelWithProjection in fp64
(bounds by tower_bound's rule from reference runs of the same weights and inputs), the device transform of the patch-14 tower, the score and the drivers.  All
weights are seeded random (no HPSv2 checkpoint exists offline), full ViT-H WIDTH at 4 layers: no test runs the 32-layer depth."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_attention_edges_gpu import TOL as ATT_TOL
from test_consistency_gpu import clip_host_prepare
from test_hps_cpu import TEXT_CASES, VISION_CASES, hps_text_ref, hps_vision_ref, run_text_module, run_vision_module, text_case, text_errs, vision_case, vision_errs
from test_ops_gpu import pair_value, ref_attention, relerr
from test_text_native_cpu import scale_err
from test_text_native_gpu import tower_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["f32", "x3", "bf16"]


def mode_dtype(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# ffn_pool_layernorm
# ---------------------------------------------------------------------------------------------------------------------
def id_cases(N, S, g):
    """name -> (ids int32 [N, S] or None, the position the entry must select per row)"""
    base = torch.randint(0, 1000, (N, S), generator=g, dtype=torch.int32)
    first, last, rep = base.clone(), base.clone(), base.clone()
    first[:, 0], last[:, S - 1] = 5000, 5000
    at = torch.zeros(N, dtype=torch.long)
    if S >= 3:                                                 # the maximum at two or three positions: the first wins
        at = torch.randint(0, S - 2, (N,), generator=g)
        for n in range(N):
            rep[n, at[n]] = rep[n, at[n] + 2] = rep[n, S - 1] = 7000
    else:
        rep[:] = 7000
    return {"none": (None, torch.zeros(N, dtype=torch.long)), "first": (first, torch.zeros(N, dtype=torch.long)),
            "last": (last, torch.full((N,), S - 1, dtype=torch.long)), "repeated": (rep, at), "equal": (torch.full((N, S), 42, dtype=torch.int32), torch.zeros(N, dtype=torch.long))}


@pytest.mark.parametrize("kind", ["f32", "bf16", "pair"])
def test_pool_layernorm_equals_layernorm_of_the_gathered_row(gpu, kind):
    """N in {1, 5} x S in {1, 17, 77} x C in {160, 1024, 1280} x the five id cases: torch.equal against ops.layernorm(x[arange, pos]); the output lies in the middle
    of a larger buffer whose sentinel rows survive"""
    from freefine_amd import ops
    dt, pair = (torch.bfloat16 if kind == "bf16" else torch.float32), kind == "pair"
    g = torch.Generator().manual_seed(len(kind))
    for N in (1, 5):
        for S in (1, 17, 77):
            for C in (160, 1024, 1280):
                x = (torch.randn(N, S, C, generator=g) * 3 + torch.randn(N, S, 1, generator=g)).to(dt).to(gpu)
                gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(gpu), (0.1 * torch.randn(C, generator=g)).to(gpu)
                for name, (ids, pos) in id_cases(N, S, g).items():
                    want = ops.layernorm(x[torch.arange(N, device=gpu), pos.to(gpu)].contiguous(), gamma, beta, eps=1e-5, pair=pair)
                    big = torch.full((N + 2, want.shape[1]), 512.0, dtype=want.dtype, device=gpu)
                    got = ops.pool_layernorm(x, None if ids is None else ids.to(gpu), gamma, beta, eps=1e-5, out=big[1:N + 1], pair=pair)
                    assert got.data_ptr() == big[1].data_ptr() and torch.equal(got, want), (kind, N, S, C, name)
                    assert bool((big[0] == 512).all()) and bool((big[-1] == 512).all()), (kind, N, S, C, name)
                    if pair:
                        assert ops.pair_width(got) == C
    # the values are LayerNorm's (not only equal to the other entry's)
    ref = torch.nn.functional.layer_norm(x[:, 0].double().cpu(), (C,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
    got = ops.pool_layernorm(x, None, gamma, beta, eps=1e-5, pair=pair)
    assert relerr(pair_value(got, C) if pair else got, ref) < (1.5e-2 if kind == "bf16" else 2e-5)


def test_pool_layernorm_refuses_bad_descriptors(gpu):
    from freefine_amd import _lib
    lib = _lib.load()
    N, S, C = 2, 17, 160
    x = torch.randn(N, 128, C, device=gpu)                      # room for every S tried below
    ids = torch.zeros(N, 128, dtype=torch.int32, device=gpu)
    gamma, beta = torch.ones(2048, device=gpu), torch.zeros(2048, device=gpu)
    out = torch.full((N, 4096), 512.0, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    base = dict(stream=s, dtype=0, x=x.data_ptr(), ids=ids.data_ptr(), y=out.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), N=N, S=S, C=C, eps=1e-5, pair=0)
    call = lambda **kw: lib.ffn_pool_layernorm(*{**base, **kw}.values())
    assert call() == 0 and call(ids=None) == 0
    out.fill_(512.0)
    bad = [dict(x=None), dict(y=None), dict(gamma=None), dict(beta=None), dict(x=x.data_ptr() + 4), dict(y=out.data_ptr() + 8), dict(ids=ids.data_ptr() + 2),
           dict(S=97), dict(S=0), dict(N=0), dict(C=162), dict(C=1540), dict(dtype=1, C=164), dict(dtype=1, pair=1), dict(dtype=2), dict(pair=2)]
    for kw in bad:
        assert call(**kw) == -22 and b"pool_layernorm" in lib.ffn_last_error(), (kw, lib.ffn_last_error())
    torch.cuda.synchronize()
    assert bool((out == 512).all()), "a refused call launches nothing"
    assert call(S=97, ids=None) == 0            # without ids the sequence length is only a stride
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# ffn_cosine_rows
# ---------------------------------------------------------------------------------------------------------------------
def cosine_tol(P):
    """each of the three fp32 sums makes at most P / 64 sequential plus 6 tree roundings of terms with sum |a_i b_i| <= |a| |b|; square roots and the divide add
    further roundings"""
    return 3 * (P / 64 + 8) * 2.0 ** -24


def cosine_ref(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a * b).sum(-1) / (a.norm(dim=-1).clamp_min(1e-12) * b.norm(dim=-1).clamp_min(1e-12))


@pytest.mark.parametrize("P", [4, 64, 1024])
def test_cosine_rows_vs_fp64(gpu, P):
    from freefine_amd import ops
    g = torch.Generator().manual_seed(P)
    for B in (1, 3, 65):
        for Bt in sorted({1, B}):
            a, b = (torch.randn(B, P, generator=g) * 3).to(gpu), torch.randn(Bt, P, generator=g).to(gpu)
            out = ops.cosine_rows(a, b)
            err = (out.double().cpu() - cosine_ref(a, b)).abs().max().item()
            print(f"cosine_rows B={B} Bt={Bt} P={P}: max error {err:.2e} (tolerance {cosine_tol(P):.2e})")
            assert out.shape == (B,) and out.dtype == torch.float32 and err <= cosine_tol(P), (B, Bt, P, err)
            assert torch.equal(ops.cosine_rows(a, b), out), "two runs are bit-equal"


def test_cosine_rows_edges(gpu):
    from freefine_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(3, 64, generator=g).to(gpu), torch.randn(3, 64, generator=g).to(gpu)
    a[1] = 0
    out = ops.cosine_rows(a, b)
    assert out[1].item() == 0.0 and out[0].item() != 0.0
    assert ops.cosine_rows(a, torch.zeros(1, 64, device=gpu)).abs().max().item() == 0.0
    assert abs(ops.cosine_rows(b, b) - 1).max().item() <= cosine_tol(64)
    sent = torch.full((5,), 512.0, device=gpu)
    ops.cosine_rows(a, b, out=sent[1:4])
    assert sent[0].item() == sent[4].item() == 512.0 and torch.equal(sent[1:4], out)
    with pytest.raises(_lib.FreeFineHipError, match="P %"):
        ops.cosine_rows(torch.randn(2, 6, device=gpu), torch.randn(2, 6, device=gpu))
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    o = torch.full((3,), 512.0, device=gpu)
    for args in ((0, b.data_ptr(), o.data_ptr(), 3, 64, 3), (a.data_ptr(), 0, o.data_ptr(), 3, 64, 3), (a.data_ptr(), b.data_ptr(), 0, 3, 64, 3),
                 (a.data_ptr() + 4, b.data_ptr(), o.data_ptr(), 2, 64, 2), (a.data_ptr(), b.data_ptr(), o.data_ptr(), 3, 64, 2), (a.data_ptr(), b.data_ptr(), o.data_ptr(), 0, 64, 1)):
        assert lib.ffn_cosine_rows(s, *args) == -22 and b"cosine_rows" in lib.ffn_last_error(), args
    torch.cuda.synchronize()
    assert bool((o == 512).all())


# ---------------------------------------------------------------------------------------------------------------------
# the generic attention kernels at head dim 80 (ViT-H/14's image tower): existing kernels, shapes no other test covers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [17, 257])
def test_noncausal_attention_at_head_dim_80(gpu, S, mode):
    """heads in {2, 16} x rows in {1, 3}; q | k in one buffer like the tower's fused projection, V^T padded to ceil8(S) with zeros; bf16 against the bf16-rounded
    inputs; x3 under the fp32 tolerance because at 80-wide heads it runs the exact kernel"""
    from freefine_amd import ops
    tol = ATT_TOL["bf16"] if mode == "bf16" else ATT_TOL["f32"]
    worst = 0.0
    for heads in (2, 16):
        for B in (1, 3):
            g = torch.Generator().manual_seed(1000 * S + 10 * heads + B)
            C, dt = heads * 80, mode_dtype(mode)
            qk, v = torch.randn(B, S, 2 * C, generator=g).to(dt), torch.randn(B, S, C, generator=g).to(dt)
            ld = (S + 7) // 8 * 8
            vt = torch.zeros(B, C, ld, dtype=dt)
            vt[:, :, :S] = v.transpose(1, 2)
            qkd = qk.to(gpu)
            out = ops.attention(qkd, qkd[..., C:], vt.to(gpu), heads, 80 ** -0.5, None, Sk=S, C=C, x3=mode == "x3", out_pair=mode == "x3")
            assert out.shape == (B, S, C) and out.dtype == dt and ops.pair_width(out) is None
            for b in range(B):
                e = relerr(out[b], ref_attention(qk[b, :, :C].double(), qk[b, :, C:].double(), v[b].double(), heads, 80 ** -0.5))
                worst = max(worst, e)
                assert e < tol, (mode, S, heads, B, b, e)
    print(f"attention D=80 {mode} S={S}: worst {worst:.2e} (tolerance {tol:.1e})")


# ---------------------------------------------------------------------------------------------------------------------
# the towers against transformers in fp64
# ---------------------------------------------------------------------------------------------------------------------
def report(line):
    print(line)
    if os.environ.get("FFN_HPS_PARITY_OUT"):            # (how profiles/hps_parity.txt is written)
        with open(os.environ["FFN_HPS_PARITY_OUT"], "a") as f:
            f.write(line + "\n")


# measured on the MI355X: profiles/hps_parity.txt
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VISION_CASES))
def test_openclip_vision_vs_transformers_fp64(gpu, name, mode):
    """tiny14 at B = 4 and ViT-H/14 cut to 4 layers at full width, B = 2, against CLIPVisionModelWithProjection.double() on the CPU under tower_bound's rule"""
    from freefine_amd.hps import HipOpenCLIPVision
    cfg, st, x, want, _ = vision_case(name)
    errs = vision_errs(name)
    net = HipOpenCLIPVision(cfg, st, dtype=mode_dtype(mode), device=gpu, x3=mode == "x3")
    assert net.kpe == (608 if mode == "x3" else 592)
    out = net(x)
    assert out.shape == want.shape and out.dtype == torch.float32
    e, bound = scale_err(out, want), tower_bound(errs, mode)
    line = f"OpenCLIP vision tower {name} {mode}: error {e:.3e} of the output maximum ({want.abs().max():.3f}); bound {bound:.3e} (reference errors: " + \
           ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + ")"
    report(line)
    assert e <= bound, line


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TEXT_CASES))
def test_text_with_projection_vs_transformers_fp64(gpu, name, mode):
    """width 128 / 2 layers / projection 64 and ViT-H/14's text width (1024, 16 heads, MLP 4096, vocabulary 49408) cut to 4 layers, on the three PROMPTS (a short
    one, the empty one, a truncated one), against CLIPTextModelWithProjection.double() on the CPU under tower_bound's rule"""
    from freefine_amd.text import HipCLIPTextWithProjection
    cfg, st, ids, want, _ = text_case(name)
    errs = text_errs(name)
    net = HipCLIPTextWithProjection(cfg, st, dtype=mode_dtype(mode), device=gpu, x3=mode == "x3")
    out = net(ids)
    assert out.shape == want.shape and out.dtype == torch.float32 and out.is_cuda
    e, bound = scale_err(out, want), tower_bound(errs, mode)
    line = f"OpenCLIP text tower {name} {mode}: error {e:.3e} of the output maximum ({want.abs().max():.3f}); bound {bound:.3e} (reference errors: " + \
           ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + ")"
    report(line)
    assert e <= bound, line
    # a prompt's embedding does not depend on what is encoded beside it
    for j in range(3):
        assert torch.equal(net(ids[j:j + 1])[0], out[j]), (name, mode, j)
    assert torch.equal(net(torch.cat([ids, ids.flip(0)]))[3:], out.flip(0))


@pytest.mark.parametrize("shape", [(3, 64, 96, 3), (2, 90, 64, 3)])
def test_features_u8_of_the_patch14_tower(gpu, shape):
    """host and device input; f32 and bf16: torch.equal against forward of the PIL-prepared tensor; x3 (pair rows straight from the bytes): within that mode's
    tower bound of forward"""
    from freefine_amd.hps import HipOpenCLIPVision
    cfg, st, *_ = vision_case("tiny14")
    imgs = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
    x = clip_host_prepare(imgs, size=cfg.image_size)
    assert tuple(x.shape) == (shape[0], 3, 56, 56)
    for mode in MODES:
        net = HipOpenCLIPVision(cfg, st, dtype=mode_dtype(mode), device=gpu, x3=mode == "x3")
        want = net(x)
        for src in (imgs, torch.from_numpy(imgs).to(gpu)):
            got = net.features_u8(src)
            assert got.shape == (shape[0], 64) and got.dtype == torch.float32
            if mode == "x3":
                assert scale_err(got, want) <= tower_bound(vision_errs("tiny14"), "x3"), (mode, scale_err(got, want))
            else:
                assert torch.equal(got, want), (mode, (got - want).abs().max().item())
    with pytest.raises(ValueError, match="no positional interpolation"):
        net(torch.zeros(1, 3, 224, 224))


# ---------------------------------------------------------------------------------------------------------------------
# the score and the drivers
# ---------------------------------------------------------------------------------------------------------------------
CAPTIONS = ["a photo of a cup", "two dogs on a beach at sunset", ""]


def smooth_images(n, H, W, seed):
    """smooth colour fields with some noise, every one different"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(n):
        f = rng.uniform(0.02, 0.3, (3, 2))
        ph = rng.uniform(0, 6.28, (3, 2))
        im = np.stack([127 + 90 * np.sin(f[c, 0] * yy + ph[c, 0]) * np.cos(f[c, 1] * xx + ph[c, 1]) for c in range(3)], -1) + rng.normal(0, 12, (H, W, 3))
        out.append(np.clip(im, 0, 255).astype(np.uint8))
    return np.stack(out)


_TINY = {}


def tiny_model(gpu):
    """(HipHPSv2 of the tiny towers with the byte tokenizer in fp32, vision config and state, text config and state) -- built once"""
    if not _TINY:
        from freefine_amd import clipvision as CV
        from freefine_amd import hps
        from freefine_amd import text as FT
        vcfg, tcfg = hps.openclip_vision_config("tiny14"), FT.text_projection_config("tiny")
        vst, tst = CV.synthetic_state(vcfg, seed=5), FT.synthetic_text_state(tcfg, seed=6)
        _TINY["m"] = (hps.HipHPSv2.from_state(dict(vst, **tst), FT.ByteTokenizer(), "tiny14", "tiny", device=gpu), vcfg, vst, tcfg, tst)
    return _TINY["m"]


def host_scores(imgs, prompts, vcfg, vst, tcfg, tst):
    """(fp64 cosines of the restated towers, the tolerance of each).  Tolerance: a tower error of delta (max-norm, in units of the output maximum) moves the
    normalised feature by at most delta max|F| sqrt(P) / |f|_2 and the cosine by at most that, to first order -- summed over both towers with delta =
    tower_bound's fp32 bound from the CPU modules' fp32 errors on these very inputs -- plus the cosine kernel's own tolerance"""
    from freefine_amd import text as FT
    x = clip_host_prepare(imgs, size=vcfg.image_size)
    ids = FT.ByteTokenizer()(list(prompts)).input_ids
    fv, ft = hps_vision_ref(vcfg, vst, x), hps_text_ref(tcfg, tst, ids)
    wv, ev = run_vision_module(vcfg, vst, x)
    wt, et = run_text_module(tcfg, tst, ids)
    assert scale_err(fv, wv) <= 1e-12 and scale_err(ft, wt) <= 1e-12
    P = fv.shape[1]
    bv, bt = tower_bound({"f32": ev}, "f32"), tower_bound({"f32": et}, "f32")
    tol = bv * fv.abs().max() * P ** 0.5 / fv.norm(dim=-1) + bt * ft.abs().max() * P ** 0.5 / ft.norm(dim=-1) + cosine_tol(P)
    return torch.nn.functional.cosine_similarity(fv, ft.expand_as(fv) if ft.shape[0] == 1 else ft), tol


def test_score_vs_fp64_restatement(gpu):
    model, vcfg, vst, tcfg, tst = tiny_model(gpu)
    imgs = smooth_images(6, 64, 96, seed=3)
    got, want, tols = [], [], []
    for cap in CAPTIONS:
        s = model.score_u8(imgs, cap)
        assert s.shape == (6,) and s.dtype == torch.float32 and s.is_cuda
        w, t = host_scores(imgs, [cap], vcfg, vst, tcfg, tst)
        got.append(s.double().cpu()), want.append(w), tols.append(t)
    got, want, tols = torch.stack(got), torch.stack(want), torch.stack(tols)
    err = (got - want).abs()
    print(f"HPS score, tiny towers: max error {err.max():.2e} (tolerance {tols.max():.2e}); scores {want.min():.4f} .. {want.max():.4f}")
    assert bool((err <= tols).all()), (err.max().item(), tols.max().item())
    # different images and prompts give different scores
    assert (want.max(1).values - want.min(1).values).min() > 10 * tols.max() and (want.max(0).values - want.min(0).values).min() > 10 * tols.max()
    # one prompt each = the diagonal of the rows above
    each = model.score_u8(imgs[:3], CAPTIONS)
    assert torch.equal(each.cpu(), torch.stack([model.score_u8(imgs[:3], c)[i] for i, c in enumerate(CAPTIONS)]).cpu())
    with pytest.raises(ValueError, match="prompts"):
        model.score_u8(imgs[:3], CAPTIONS[:2])


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


def test_calculate_hps_and_the_driver_end_to_end(gpu, tmp_path):
    from freefine_amd import metrics as FM
    model, vcfg, vst, tcfg, tst = tiny_model(gpu)
    data, arrays = write_tree(str(tmp_path))
    got = FM.calculate_hps(data, "gen_img_path", model)
    total, tol = 0.0, 0.0
    for key, image in data.items():
        for arr in arrays[key]:
            w, t = host_scores(arr[None], [image["4v_caption"]], vcfg, vst, tcfg, tst)
            total, tol = total + w.item(), max(tol, t.item())
    want = total / 5
    print(f"calculate_hps: {got:.8f} vs host fp64 {want:.8f} (tolerance {tol:.2e})")
    assert abs(got - want) <= tol
    # the command-line driver, a process of its own
    path, weights = str(tmp_path / "results.json"), str(tmp_path / "hps_tiny.pt")
    json.dump(data, open(path, "w"))
    torch.save(dict(vst, **tst), weights)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "evaluation", "metrics", "main.py"), "--path", path, "--task", "001000000", "--hps_config", "tiny",
                          "--hps_tokenizer", "bytes", "--hps_weights", weights], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("HPS: ")]
    assert len(lines) == 1 and float(lines[0][5:]) == got, (lines, got)
