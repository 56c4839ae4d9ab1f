"""GPU: click-to-mask (freefine_amd/sam.py) -- the three kernels around the network against torch on the CPU / fp64, ops.attention at the decoder's head dims and
sequence lengths against an fp64 softmax, the encoder in every mode and the whole path against tests/sam_ref.py (pinned to the reference's source by
tests/test_sam_cpu.py) and the G16 golden.  Weights and inputs are regenerated from the seeds the golden records.

Bounds.  Patch rows: the no-resize rows are (byte / 255 - mean) / std bit for bit; resized rows 2e-6 absolute (a four-term fp32 blend of values <= 1, <= 4 roundings
~ 2.4e-7, divided by std >= 0.224).  Hyper masks: 1e-6 of the maximum (a C <= 32 long fp32 dot product).  Bicubic: 1e-5 of the input maximum (16 taps, sum |w| <=
1.5625, fp32 sums).  Attention: the per-op fp32 bound 2e-5 of the output maximum.  Network outputs: tower_bound of tests/test_text_native_gpu.py (fp32: 8 x the
error of the fp32 restatement on the CPU, capped at 2e-5; x3 / bf16: 2 x the error of the emulated arithmetic) with the errors of tests/sam_ref.py on the same
case (vits: recorded in the golden by tools/gen_golden.py::run_g16, where the fp32 error is that of the reference's own fp32 model); IoU predictions 1e-4."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sam_ref as SR
from test_ops_gpu import pair_value, ref_attention, relerr
from test_sam_cpu import g16
from test_text_native_cpu import scale_err
from test_text_native_gpu import mode_dtype, tower_bound

pytestmark = pytest.mark.gpu
SIDE, PATCH, K = 128, 16, 768
RESIZE_CASES = [(48, 80), (7, 5), (200, 136), (128, 128)]


def random_images(B, H, W, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8))


def host_rows(img):
    """torch on the CPU: ToTensor, F.interpolate(bilinear), normalise, im2col"""
    from freefine_amd import encoder, sam
    x = img.permute(0, 3, 1, 2).float() / 255
    if tuple(x.shape[2:]) != (SIDE, SIDE):
        x = F.interpolate(x, (SIDE, SIDE), mode="bilinear")
    x = (x - torch.tensor(sam.PIXEL_MEAN).view(1, 3, 1, 1)) / torch.tensor(sam.PIXEL_STD).view(1, 3, 1, 1)
    return encoder.im2col(x, PATCH)


def device_rows(img, gpu, dtype=torch.float32, pair=False, ldo=K):
    from freefine_amd import ops, sam
    return ops.sam_patch_rows(img.to(gpu), SIDE, PATCH, ldo, dtype, sam.PIXEL_MEAN, sam.PIXEL_STD, pair=pair)


@pytest.mark.parametrize("H,W", RESIZE_CASES)
def test_patch_rows_equal_the_torch_transform(gpu, H, W):
    img = random_images(3, H, W, 7 * H + W)
    img[0, :2] = 255                                           # saturated and zero bytes at a border
    img[0, -1] = 0
    want = host_rows(img)
    got = device_rows(img, gpu)
    assert got.shape == want.shape == (3 * 64, K) and got.dtype == torch.float32
    e = (got.cpu() - want).abs().max().item()
    print(f"patch rows {H}x{W} -> {SIDE}: max abs deviation {e:.2e}")
    if (H, W) == (SIDE, SIDE):
        assert torch.equal(got.cpu(), want)
    else:
        assert e <= 2e-6
    # a batch row does not depend on the images beside it
    for b in range(3):
        assert torch.equal(device_rows(img[b:b + 1], gpu), got[b * 64:(b + 1) * 64])
    # bf16 rows are the rounded fp32 rows; the pair rows carry hi + lo of the fp32 value
    assert torch.equal(device_rows(img, gpu, torch.bfloat16), got.to(torch.bfloat16))
    pair = device_rows(img, gpu, pair=True)
    assert pair.shape == (3 * 64, 2 * K) and pair.dtype == torch.bfloat16
    rec, g64 = pair_value(pair, K).cpu(), got.double().cpu()
    assert ((rec - g64).abs() <= 2.0 ** -16 * g64.abs()).all()
    # columns past a patch's 3 * 16 * 16 are zero
    wide = device_rows(img[:1], gpu, ldo=K + 8)
    assert torch.equal(wide[:, :K], got[:64]) and (wide[:, K:] == 0).all()


@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("hw", [32 * 32, 33 * 31])
def test_hyper_masks_vs_fp64(gpu, C, hw):
    from freefine_amd import ops
    g = torch.Generator().manual_seed(100 * C + hw)
    up, hy = torch.randn(2, hw, C, generator=g), torch.randn(2, 4, C, generator=g)
    got = ops.hyper_masks(up.to(gpu), hy.to(gpu))
    want = hy.double() @ up.double().transpose(1, 2)
    assert got.shape == (2, 4, hw)
    e = scale_err(got, want)
    print(f"hyper masks C={C} hw={hw}: {e:.2e} of the maximum")
    assert e <= 1e-6


@pytest.mark.parametrize("h,H,W", [(32, 48, 80), (32, 32, 32), (32, 17, 100), (64, 37, 53)])
def test_upsample_bicubic_equals_torch(gpu, h, H, W):
    from freefine_amd import ops
    g = torch.Generator().manual_seed(h + H + W)
    x = torch.randn(3, h, h, generator=g)
    x[1, 4:20, 8:24] = 0.0                                     # exact zeros: the threshold includes them
    x[2] = -0.37                                               # a constant field
    got, mask = ops.upsample_bicubic(x.to(gpu), H, W, mask=True)
    want = F.interpolate(x[:, None], (H, W), mode="bicubic")[:, 0]
    assert got.shape == (3, H, W) and mask.shape == (3, H, W) and mask.dtype == torch.uint8
    e = (got.cpu() - want).abs().max().item() / x.abs().max().item()
    print(f"bicubic {h}x{h} -> {H}x{W}: {e:.2e} of the input maximum")
    assert e <= 1e-5
    if (H, W) == (h, h):
        assert torch.equal(got.cpu(), x)
    assert torch.equal(mask, ((got >= 0) * 255).to(torch.uint8))
    assert mask[1].any() and not mask[2].any()
    assert torch.equal(ops.upsample_bicubic(x.to(gpu), H, W), got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_eltwise_gelu_vs_fp64(gpu, dtype):
    """FFN_ELT_GELU through ops.gelu, on more elements than one pass of the capped grid holds (4096 workgroups x 256 threads x 4) and on a 4-element tensor.
    Bound per element: the rounding of the result (fp32: 2^-22 |y| covers the product's roundings; bf16: 2^-8 |y| is the round to nearest of an 8-bit significand, half an ulp at the bottom of a binade) plus
    |x| times the error of the normal CDF -- erff's few ulp in fp32, and in bf16 the Abramowitz-Stegun 7.1.26 form (1.5e-7) with an approximate reciprocal and
    exponential (1 ulp each) and fp32 roundings: half of (1.5e-7 + 1e-7 + 7e-8 + 6e-8) + 3e-8 = 2.2e-7, taken as 4e-7."""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(5)
    n = 4096 * 256 * 4 + 4 * 1001
    x = (torch.randn(n, generator=g) * 3).to(dtype)
    x[:8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 6.0, -6.0, 12.0, -12.0]).to(dtype)
    for t in (x, x[:4].clone()):
        got = ops.gelu(t.to(gpu))
        assert got.shape == t.shape and got.dtype == dtype
        want = F.gelu(t.double())
        err = (got.double().cpu() - want).abs()
        bound = 2.0 ** (-22 if dtype == torch.float32 else -8) * want.abs() + 4e-7 * t.double().abs()
        print(f"gelu {dtype} n={t.numel()}: worst error over its bound {(err / bound.clamp_min(1e-30)).max().item():.2f}, max abs error {err.max().item():.2e}")
        assert (err <= bound).all()


@pytest.mark.parametrize("D,S,Sk,heads", [(32, 11, 11, 2), (16, 11, 64, 2), (16, 64, 11, 2), (16, 11, 4096, 8), (16, 4096, 11, 8)])
def test_decoder_attention_shapes_vs_fp64(gpu, D, S, Sk, heads):
    from freefine_amd import encoder, ops
    g = torch.Generator().manual_seed(D + S + Sk)
    B, C = 2, heads * D
    q, k, v = torch.randn(B, S, C, generator=g), torch.randn(B, Sk, C, generator=g), torch.randn(B, Sk, C, generator=g)
    vt = torch.full((B, C, encoder.ceil8(Sk)), 1e4)            # the padding columns are multiplied by P = 0: finite, and not zero here
    vt[:, :, :Sk] = v.transpose(1, 2)
    out = ops.attention(q.to(gpu), k.to(gpu), vt.to(gpu), heads, D ** -0.5, None, Sk=Sk, C=C)
    assert out.shape == (B, S, C) and out.dtype == torch.float32
    e = max(relerr(out[b], ref_attention(q[b].double(), k[b].double(), v[b].double(), heads, D ** -0.5)) for b in range(B))
    print(f"attention D={D} S={S} Sk={Sk} heads={heads}: {e:.2e} of the output maximum")
    assert e <= 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------------
_MODELS, _REFS = {}, {}


def model(cname, mode, gpu):
    from freefine_amd import sam
    if (cname, mode) not in _MODELS:
        cfg = sam.sam_config(cname)
        _MODELS[cname, mode] = sam.HipEfficientSam(cfg, sam.synthetic_state(cfg, int(g16()["seed_" + cname])), dtype=mode_dtype(mode), x3=mode == "x3", device=gpu)
    return _MODELS[cname, mode]


def tiny_ref(name, mode):
    """sam_ref on a tiny G16 case, computed once per (case, mode)"""
    if (name, mode) not in _REFS:
        cfg, state, img, pts, lab = SR.g16_inputs(name, int(g16()["seed_tiny"]))
        _REFS[name, mode] = SR.sam_ref(cfg, state, img, pts, lab, mode)
    return _REFS[name, mode]


def encoder_batch(B):
    """(images uint8 [B, 48, 80, 3], their fp64 embeddings, the restatement's error per mode)"""
    if ("enc", B) not in _REFS:
        cfg, state, _, pts, lab = SR.g16_inputs("tiny_48x80_box", int(g16()["seed_tiny"]))
        img = np.stack([SR.smooth_image(48, 80, 900 + b) for b in range(B)])
        emb = {m: SR.sam_ref(cfg, state, img, pts.expand(B, -1, -1, -1), lab.expand(B, -1, -1), m)["emb"] for m in ("f64", "f32", "x3", "bf16")}
        _REFS["enc", B] = (img, emb["f64"], {m: scale_err(emb[m], emb["f64"]) for m in ("f32", "x3", "bf16")})
    return _REFS["enc", B]


@pytest.mark.parametrize("mode", ["f32", "x3", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
def test_encoder_vs_the_restatement(gpu, B, mode):
    img, want, errs = encoder_batch(B)
    got = model("tiny", mode, gpu).encode(img)
    assert got.shape == want.shape == (B, 64, 64) and got.dtype == torch.float32 and got.is_cuda
    e, bound = scale_err(got, want), tower_bound(errs, mode)
    line = f"SAM tiny encoder {mode} B={B}: error {e:.3e} of the output maximum; bound {bound:.3e} (restatement errors: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + ")"
    print(line)
    assert e <= bound, line


@pytest.mark.parametrize("name", [n for n, c in SR.G16_CASES.items() if c[0] == "tiny"])
def test_tiny_cases_end_to_end(gpu, name):
    G = g16()
    cfg, state, img, pts, lab = SR.g16_inputs(name, int(G["seed_tiny"]))
    ref, ref32 = tiny_ref(name, "f64"), tiny_ref(name, "f32")
    net = model("tiny", "f32", gpu)
    H, W = img.shape[1:3]
    emb = net.encode(img)
    full, iou, low, m8, order = net.predict(emb, pts, lab, (H, W), details=True)
    Q = pts.shape[1]
    assert full.shape == (1, Q, 3, H, W) and iou.shape == (1, Q, 3) and low.shape == (1, Q, 3, 32, 32) and m8.dtype == torch.uint8
    e_iou = (iou.double().cpu() - torch.as_tensor(G[name + "/iou"])).abs().max().item()
    assert e_iou <= 1e-4 and torch.equal(order.cpu(), torch.as_tensor(G[name + "/order"])), (e_iou, order, G[name + "/order"])
    report = [f"SAM tiny {name} f32: IoU deviation {e_iou:.2e} (bound 1e-4)"]
    for key, got, want in (("emb", emb, torch.as_tensor(G[name + "/emb"])), ("low", low, torch.as_tensor(G[name + "/low"])), ("full", full, ref["full"])):
        err32 = scale_err(ref32[key], ref[key])
        e, bound = scale_err(got, want), tower_bound({"f32": err32}, "f32")
        report.append(f"{key} {e:.3e} of the maximum, bound {bound:.3e} (fp32 restatement {err32:.3e})")
        assert e <= bound, report
    # the thresholded mask: the golden's sign wherever the golden's logit is further from zero than the bound
    best = torch.as_tensor(G[name + "/full_best"])
    margin = tower_bound({"f32": scale_err(ref32["full"], ref["full"])}, "f32") * ref["full"].abs().max().item()
    near = best.abs() <= margin
    assert near.double().mean().item() <= 0.02
    assert torch.equal(m8[0, 0, 0].cpu()[~near], ((best >= 0) * 255).to(torch.uint8)[~near])
    assert torch.equal(m8, ((full >= 0) * 255).to(torch.uint8))
    report.append(f"mask: {int(near.sum())} of {near.numel()} pixels inside the margin, {100.0 * (best >= 0).double().mean().item():.1f} % inside the mask")
    print("; ".join(report))
    # every query's rows are what a call with that query alone gives
    for q in range(Q):
        one = net.predict(emb, pts[:, q:q + 1], lab[:, q:q + 1], (H, W), details=True)
        for a, b in zip(one[:4], (full, iou, low, m8)):
            assert torch.equal(a[:, 0], b[:, q]), (name, q)


def test_a_kept_embedding_serves_several_prompts_bit_for_bit(gpu):
    from src.demo import utils as U
    _, _, img, _, _ = SR.g16_inputs("tiny_200x136_q2", int(g16()["seed_tiny"]))
    net = model("tiny", "f32", gpu)
    image, (H, W) = img[0], img.shape[1:3]
    emb = net.encode(image)
    box = np.array([[[[0.3 * W, 0.2 * H], [0.8 * W, 0.7 * H]]]], dtype=np.float32)
    point = np.array([[[[0.2 * W, 0.8 * H]]]], dtype=np.float32)
    m_box = net.predict(emb, box, np.array([[[2, 3]]]), (H, W), details=True)[3][0, 0, 0]
    m_point = net.predict(emb, point, np.array([[[1]]]), (H, W), details=True)[3][0, 0, 0]
    assert np.array_equal(m_box.cpu().numpy(), U.segment_with_box(net, image, (0.8 * W, 0.2 * H), (0.3 * W, 0.7 * H)))       # (clicked top-right, then bottom-left)
    assert np.array_equal(m_point.cpu().numpy(), net.segment(image, point[0, 0], [1]))
    assert not torch.equal(m_box, m_point)


@pytest.mark.parametrize("mode", ["f32", "x3"])
def test_vits_case_vs_the_reference_golden(gpu, mode):
    """the one full-size run: ViT-S at 1024 x 1024 from a 480 x 640 image, one box"""
    G, name = g16(), "vits_480x640_box"
    cfg, state, img, pts, lab = SR.g16_inputs(name, int(G["seed_vits"]))
    net = model("vits", mode, gpu)
    emb = net.encode(img)
    assert emb.shape == (1, 4096, 256)
    full, iou, low, m8, order = net.predict(emb, pts, lab, img.shape[1:3], details=True)
    assert full.shape == (1, 1, 3, 480, 640) and low.shape == (1, 1, 3, 256, 256)
    errs = {"f32": G[name + "/errs_f32"], "x3": G[name + "/errs_x3"]}
    e_iou = (iou.double().cpu() - torch.as_tensor(G[name + "/iou"])).abs().max().item()
    report = [f"SAM vits {mode}: IoU deviation {e_iou:.2e} (bound 1e-4)"]
    assert e_iou <= 1e-4, report
    assert torch.equal(order.cpu(), torch.as_tensor(G[name + "/order"])), (order, G[name + "/order"])        # the reference's sorted_ids
    for i, (key, got) in enumerate((("emb", emb[:, ::8, ::8]), ("low", low[:, :, 0, ::4, ::4]))):
        e, bound = scale_err(got, torch.as_tensor(G[f"{name}/{key}"])), tower_bound({m: float(v[i]) for m, v in errs.items()}, mode)
        report.append(f"{key} {e:.3e} of the maximum, bound {bound:.3e} (recorded reference errors: f32 {errs['f32'][i]:.3e}, x3 {errs['x3'][i]:.3e})")
        assert e <= bound, report
    assert torch.equal(m8, ((full >= 0) * 255).to(torch.uint8))
    print("; ".join(report))
