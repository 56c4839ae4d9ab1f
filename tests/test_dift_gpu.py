"""GPU: the Mean Distance metric's DIFT path on the project's kernels -- the correspondence search (ops.dift_match / ffn_dift_match) against torch's own
F.interpolate(mode='bilinear') + CosineSimilarity(dim=1) + argmax on .double() CPU tensors (the reference's arithmetic, mean_distance.py:144-159), the tie rule,
HipUNet.features against forward hooks on the oracle UNet, HipSDFeaturizer against a torch restatement over the oracle VAE / UNet, and calculate_md end to end.

Tolerance of the cosine check: 4 x the largest deviation, over all keypoints and pixels, of torch's FP32 brute force from its fp64 one on the same inputs, computed
here on the CPU -- the reference's own fp32 arithmetic is the yardstick, the factor 4 covers a different summation order.  bf16 rows: both sides start from the
same bf16-rounded values (the ensemble mean is taken in fp32 / fp64 of those), so the same bound holds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# (C, h, w, H, W, K)
SHAPES = {
    "r1.75_K1": (32, 4, 4, 7, 9, 1),                  # ratio < 2, non-integer
    "r7.5_K7": (96, 6, 4, 45, 30, 7),                 # ratio 7.5, non-square
    "r8_K33": (64, 5, 7, 40, 56, 33),                 # more keypoints than one launch carries (32)
    "r1_K5": (64, 8, 8, 8, 8, 5),                     # ratio 1, all weights 0 / 1
    "sdC_K30": (1280, 32, 32, 128, 128, 30),          # the workload's C and low-resolution size
    "sdratio_K30": (64, 32, 32, 512, 512, 30),        # the workload's ratio
}
TAIL = dict(tail_C36=(36, 5, 7, 40, 56, 6))                # C % 8 == 4: the last 16-byte chunk of a bf16 row is half a chunk; C % 64 != 0: idle lanes
RANDOM = dict(random=(32, 4, 4, 7, 9, 9))                 # the fully random case: no two pixels share a clamped source coordinate at this ratio
ROLL = 2                                              # cells the target features are rolled by, in both directions


def make_rows(C, h, w, E, dtype, seed, rolled=True):
    """source / target rows [E, hw, C] (CPU, `dtype`): the target's ensemble mean is the source's rolled by ROLL cells plus 0.3 x noise (decisive maxima), or
    unrelated (rolled=False); every ensemble member deviates from the mean"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(h, w, C, generator=g) + 0.5
    tgt = (torch.roll(base, (ROLL, ROLL), (0, 1)) + 0.3 * torch.randn(h, w, C, generator=g)) if rolled else torch.randn(h, w, C, generator=g) + 0.5
    dev = 0.2 * torch.randn(2, E, h * w, C, generator=g)
    dev -= dev.mean(1, keepdim=True)
    return (base.reshape(1, h * w, C) + dev[0]).to(dtype), (tgt.reshape(1, h * w, C) + dev[1]).to(dtype)


def make_kps(h, w, H, W, K, seed, interior):
    """the two corners first; the rest random -- with `interior` among the pixels whose match (ROLL cells further) lies where bilinear source coordinates are
    not clamped, so that no two pixels of the edited image carry the same feature vector there (a clamped border band repeats its rows / columns exactly)"""
    rng = np.random.default_rng(seed)
    ry, rx = H / h, W / w
    kps = [(0, 0), (H - 1, W - 1)]
    lo_r, hi_r, lo_c, hi_c = (int(np.ceil(ry / 2)), int(H - (ROLL + 0.6) * ry), int(np.ceil(rx / 2)), int(W - (ROLL + 0.6) * rx)) if interior else (0, H, 0, W)
    while len(kps) < K:
        kps.append((int(rng.integers(lo_r, hi_r)), int(rng.integers(lo_c, hi_c))))
    return kps[:K]


def brute(rows_s, rows_t, h, w, H, W, kps, dt):
    """the reference's arithmetic in precision dt: ensemble mean, F.interpolate, CosineSimilarity per keypoint -> cosine maps [K, H, W]"""
    C = rows_s.shape[-1]
    fs = rows_s.to(dt).mean(0).reshape(1, h, w, C).permute(0, 3, 1, 2)
    ft = rows_t.to(dt).mean(0).reshape(1, h, w, C).permute(0, 3, 1, 2)
    Fs, Ft = F.interpolate(fs, (H, W), mode="bilinear"), F.interpolate(ft, (H, W), mode="bilinear")
    cos = torch.nn.CosineSimilarity(dim=1)
    return torch.stack([cos(Fs[0, :, r, c].view(1, C, 1, 1), Ft)[0] for r, c in kps])


_REF = {}


def reference(name, E, dtype, rolled=True):
    """computed once per (shape, E, dtype) and shared by the row-stride variants; never modified"""
    key = (name, E, dtype, rolled)
    if key not in _REF:
        if len(_REF) >= 2:                              # the cases arrive grouped by key: keep memory flat
            _REF.clear()
        C, h, w, H, W, K = {**SHAPES, **RANDOM, **TAIL}[name]
        rs, rt = make_rows(C, h, w, E, dtype, seed=len(name) + 7 * E, rolled=rolled)
        kps = make_kps(h, w, H, W, K, seed=3, interior=rolled)
        torch.set_num_threads(max(8, min(16, torch.get_num_threads())))
        c64 = brute(rs, rt, h, w, H, W, kps, torch.float64)
        c32 = brute(rs, rt, h, w, H, W, kps, torch.float32)
        tol = 4.0 * (c32.double() - c64).abs().max().item()
        top2 = c64.flatten(1).topk(2).values
        _REF[key] = dict(rs=rs, rt=rt, kps=kps, c64=c64, tol=tol, max64=top2[:, 0], gap=top2[:, 0] - top2[:, 1], arg64=c64.flatten(1).argmax(1))
    return _REF[key]


def strided(rows, ld, gpu):
    """the rows as the left columns of a wider buffer (row stride ld), like an up block's output inside a concatenation buffer"""
    E, n, C = rows.shape
    buf = torch.full((E, n, ld), float("nan"), dtype=rows.dtype, device=gpu)      # the padding must never be read
    buf[..., :C] = rows.to(gpu)
    return buf[..., :C]


def check_match(ref, name, E, dtype, pad, gpu):
    from freefine_amd import ops
    C, h, w, H, W, K = {**SHAPES, **RANDOM, **TAIL}[name]
    rs, rt = strided(ref["rs"], C + pad, gpu), strided(ref["rt"], C + pad, gpu)
    rc, cs = ops.dift_match(rs, rt, (h, w), (H, W), ref["kps"])
    rc2, cs2 = ops.dift_match(rs, rt, (h, w), (H, W), ref["kps"])
    assert rc.dtype == torch.int32 and tuple(rc.shape) == (K, 2) and cs.dtype == torch.float32 and tuple(cs.shape) == (K,)
    assert torch.equal(rc, rc2) and torch.equal(cs.view(torch.int32), cs2.view(torch.int32)), "two runs must agree bit for bit"
    rc, cs = rc.cpu().long(), cs.cpu().double()
    flat = rc[:, 0] * W + rc[:, 1]
    tol, c64 = ref["tol"], ref["c64"]
    at = c64.flatten(1).gather(1, flat[:, None])[:, 0]                            # fp64 cosine at the returned position
    err = (cs - at).abs().max().item()
    decisive = ref["gap"] > 2 * tol
    n_under = int((~decisive).sum())
    print(f"dift_match {name} E={E} {str(dtype)[6:]} ld=C+{pad}: |cos - cos64| {err:.2e} (tol {tol:.2e} = 4 x fp32 brute force), min top-two gap {ref['gap'].min().item():.2e}, "
          f"{n_under}/{K} keypoints under 2 x tol, positions equal {int((flat == ref['arg64']).sum())}/{K}")
    assert (rc[:, 0] >= 0).all() and (rc[:, 0] < H).all() and (rc[:, 1] >= 0).all() and (rc[:, 1] < W).all()
    assert err <= tol
    assert (at >= ref["max64"] - tol).all()
    assert n_under <= 0.1 * K, "the inputs must be decisive: this cap keeps the position check from hiding a failure"
    assert torch.equal(flat[decisive], ref["arg64"][decisive])


@pytest.mark.parametrize("pad", [0, 32])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(SHAPES))
def test_match_vs_fp64_brute_force(gpu, name, dtype, E, pad):
    check_match(reference(name, E, dtype), name, E, dtype, pad, gpu)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_match_channels_not_a_multiple_of_the_chunk(gpu, dtype, pad):
    """C = 36: bf16 rows end in an 8-byte half chunk (C % 8 == 4) and most lanes of a wave have no channel; row strides 36 is not allowed for bf16 (ld % 8),
    so bf16 runs at ld = 40 and 48, fp32 at 36 and 44"""
    pad += 4 if dtype == torch.bfloat16 else 0
    check_match(reference("tail_C36", 3, dtype), "tail_C36", 3, dtype, pad, gpu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_match_unrelated_features(gpu, dtype):
    """fully random target features (no planted match).  At the ratio-1.75 shape no two pixels share a clamped source coordinate, so ties arise only by rounding."""
    check_match(reference("random", 3, dtype, rolled=False), "random", 3, dtype, 0, gpu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E", [1, 3])
def test_tie_rule_and_degenerate_vectors(gpu, dtype, E):
    """ratio 1 (all weights 0 / 1).  (a) two bit-identical target vectors equal to the query at flat indices p1 < p2, an all-zero vector below both: the match
    is p1 (numpy's argmax rule), never the zero vector.  (b) every target vector points away from the query (negative cosines) except one all-zero vector:
    numpy's argmax then IS the zero vector, and its cosine must be exactly 0, not NaN (eps-clamped denominator).  Every case runs twice, bit-identical."""
    from freefine_amd import ops
    C, h, w = 64, 8, 8
    g = torch.Generator().manual_seed(5)
    src = (torch.randn(1, h * w, C, generator=g) + 0.5).to(dtype).repeat(E, 1, 1)
    kp, p0, p1, p2 = (3, 5), 2, 19, 44
    q = src[0, kp[0] * w + kp[1]]
    tgt = (torch.randn(1, h * w, C, generator=g) + 0.5).to(dtype).repeat(E, 1, 1)
    tgt[:, p1], tgt[:, p2], tgt[:, p0] = q, q, 0
    rc, cs = ops.dift_match(src.to(gpu), tgt.to(gpu), (h, w), (h, w), [kp, (0, 0)])
    rc2, cs2 = ops.dift_match(src.to(gpu), tgt.to(gpu), (h, w), (h, w), [kp, (0, 0)])
    assert torch.equal(rc, rc2) and torch.equal(cs.view(torch.int32), cs2.view(torch.int32))
    assert rc[0].tolist() == [p1 // w, p1 % w], rc.tolist()
    assert abs(cs[0].item() - 1.0) <= 1e-6 and not torch.isnan(cs).any()      # 64-term fp32 sums in two orders, a sqrt, a product, a division: < 16 x 2^-24
    assert rc[1].tolist() != [p0 // w, p0 % w]
    # (b)
    amp = torch.rand(h * w, 1, generator=g) + 0.5
    away = (-amp * q.float()[None] + 0.05 * torch.randn(h * w, C, generator=g)).to(dtype)[None].repeat(E, 1, 1)
    away[:, p1] = 0
    c64 = brute(src, away, h, w, h, w, [kp], torch.float64)[0].flatten()
    assert c64.argmax().item() == p1 and c64[p1].item() == 0.0 and (c64[torch.arange(h * w) != p1] < 0).all()
    rc, cs = ops.dift_match(src.to(gpu), away.to(gpu), (h, w), (h, w), [kp])
    rc2, cs2 = ops.dift_match(src.to(gpu), away.to(gpu), (h, w), (h, w), [kp])
    assert torch.equal(rc, rc2) and torch.equal(cs.view(torch.int32), cs2.view(torch.int32))
    assert rc[0].tolist() == [p1 // w, p1 % w] and cs[0].item() == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# HipUNet.features
# ---------------------------------------------------------------------------------------------------------------------------------------------
MODES = [("f32", torch.float32, False, 1e-4), ("bf16", torch.bfloat16, False, 6e-2), ("x3", torch.float32, True, 1e-4)]      # the bounds of tests/test_unet_gpu.py


def hooked(onet, idx, *args):
    """the oracle's forward and the output of its up_blocks[idx] (NCHW)"""
    got = {}
    hd = onet.up_blocks[idx].register_forward_hook(lambda m, a, out: got.__setitem__("ft", out.detach()))
    try:
        eps = onet(*args)
    finally:
        hd.remove()
    return eps, got["ft"]


def rows_to_nchw(rows, hw):
    return rows.float().reshape(rows.shape[0], hw[0], hw[1], -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("name", ["tiny", "tiny-conv"])
@pytest.mark.parametrize("mode,dtype,x3,tol", MODES)
def test_unet_features_vs_oracle(gpu, name, mode, dtype, x3, tol):
    from golden_cases import rng_tensor
    from test_unet_gpu import build, relerr
    onet, hnet = build(name, dtype, gpu, x3=x3)
    D = onet.cfg.cross_attention_dim
    x, enc = rng_tensor(1, (2, 4, 16, 16)), rng_tensor(2, (2, 77, D))
    n = len(onet.up_blocks)
    graph = mode == "f32" and name == "tiny"               # one configuration also checks that a captured forward is undisturbed
    hnet.use_graph = graph
    assert relerr(hnet(x.to(gpu), 481, enc.to(gpu)), onet(x, torch.tensor(481), enc)) < tol
    for idx in sorted({0, 1, n - 1}):
        ref_eps, ref = hooked(onet, idx, x, torch.tensor(261), enc)
        rows, hw = hnet.features(x.to(gpu), 261, enc.to(gpu), idx)
        assert rows.dtype == dtype and tuple(rows.shape) == (2, hw[0] * hw[1], ref.shape[1]) and tuple(hw) == tuple(ref.shape[2:]) and rows.stride(2) == 1
        err = relerr(rows_to_nchw(rows, hw), ref)
        print(f"features {name} {mode} up_blocks[{idx}] {tuple(ref.shape)} row stride {rows.stride(1)}: {err:.2e}")
        assert err < tol
    # forward on the same executor is undisturbed (graph mode: the captured forward is found again, nothing was captured for features)
    assert relerr(hnet(x.to(gpu), 481, enc.to(gpu)), onet(x, torch.tensor(481), enc)) < tol
    assert relerr(hnet(x.to(gpu), 21, enc.to(gpu)), onet(x, torch.tensor(21), enc)) < tol
    assert len(hnet._graphs) == (1 if graph else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# featurizer and metric
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipes(gpu):
    from test_pipeline_gpu import make_pipe
    cache = {}

    def get(mode):
        if mode not in cache:
            _, dtype, x3, _ = next(m for m in MODES if m[0] == mode)
            cache[mode] = make_pipe(gpu, "tiny", "edit", dtype, x3=x3)       # (an edit controller is registered: features() must run plain attention all the same)
        return cache[mode]
    return get


@pytest.mark.parametrize("mode,dtype,x3,tol", MODES)
def test_featurizer_vs_torch_restatement(gpu, pipes, mode, dtype, x3, tol):
    """dift_sd.py's SDFeaturizer.forward restated over the oracle VAE / UNet with explicit noise and the posterior mean: 128^2 image, E = 2, t = 261, up block 1"""
    from freefine_amd.dift import HipSDFeaturizer
    from freefine_amd.text import ByteTokenizer, SyntheticTextEncoder, make_text_embed
    from golden_cases import rng_tensor, synth_images
    from oracle import sd_unet, sd_vae
    from test_unet_gpu import relerr
    pipe = pipes(mode)
    feat = HipSDFeaturizer(pipe)
    img, img2, _ = synth_images()
    E, t = 2, 261
    noise, noise2 = rng_tensor(31, (E, 4, 16, 16)), rng_tensor(32, (E, 4, 16, 16))
    ocfg = sd_unet.unet_config("tiny")
    onet, ovae = sd_unet.init_unet(ocfg, seed=0), sd_vae.init_vae(sd_vae.vae_config("tiny"), seed=1)
    text = make_text_embed(ByteTokenizer(), SyntheticTextEncoder(ocfg.cross_attention_dim))(["a cup"])
    z = ovae.encode_mean((torch.from_numpy(img).float() / 127.5 - 1).permute(2, 0, 1)[None]) * 0.18215
    abar = pipe.scheduler.alphas_cumprod[t]
    zt = abar ** 0.5 * z.repeat(E, 1, 1, 1) + (1 - abar) ** 0.5 * noise
    _, ft = hooked(onet, 1, zt, torch.tensor(t), text.repeat(E, 1, 1))
    ref = ft.mean(0, keepdim=True)
    got = feat.forward_nchw(img, "a cup", t=t, up_ft_index=1, ensemble_size=E, noise=noise)
    assert tuple(got.shape) == tuple(ref.shape)
    err = relerr(got, ref)
    print(f"featurizer {mode}: mean feature map {tuple(ref.shape)} vs the torch restatement {err:.2e}")
    assert err < tol
    # tensor input in [-1, 1], [3, H, W]: the same latent path
    got_t = feat.forward_nchw((torch.from_numpy(img).float() / 127.5 - 1).permute(2, 0, 1), "a cup", t=t, up_ft_index=1, ensemble_size=E, noise=noise)
    assert relerr(got_t, ref) < tol
    # pair() = two forward() calls, bit for bit
    rs, re_, hw = feat.pair(img, img2, "a cup", t=t, up_ft_index=1, ensemble_size=E, noise=noise, noise_edited=noise2)
    fs, hw1 = feat.forward(img, "a cup", t=t, up_ft_index=1, ensemble_size=E, noise=noise)
    fe, hw2 = feat.forward(img2, "a cup", t=t, up_ft_index=1, ensemble_size=E, noise=noise2)
    assert tuple(hw) == tuple(hw1) == tuple(hw2)
    assert torch.equal(rs, fs) and torch.equal(re_, fe)
    # noise drawn from a CPU generator is reproducible
    a, _ = feat.forward(img, "a cup", ensemble_size=E, generator=torch.Generator().manual_seed(9))
    b, _ = feat.forward(img, "a cup", ensemble_size=E, generator=torch.Generator().manual_seed(9))
    assert torch.equal(a, b)


@pytest.mark.parametrize("mode,dtype,x3,tol", MODES)
def test_pair_equals_forward_across_the_groupnorm_threshold(gpu, pipes, mode, dtype, x3, tol):
    """E = 24 at 16x16 latents: forward() runs 24 rows, which the library's GroupNorm rule (ffn_gn_fused: 16x16 positions up to 32 rows) gives the one-launch
    fused kernel, pair() runs 48, which it would give statistics + apply.  features() pins the form to that of one row, so the two must still agree bit for
    bit -- as must the rows of a 6-row batch with the first rows of the 48 (GEMM tiles of other heights)."""
    from freefine_amd import _lib
    from freefine_amd.dift import HipSDFeaturizer
    from golden_cases import rng_tensor, synth_images
    lib = _lib.load()
    assert lib.ffn_gn_fused(24, 256, 32, 32) == 1 and lib.ffn_gn_fused(48, 256, 32, 32) == 0, "the case must cross the library's threshold"
    feat = HipSDFeaturizer(pipes(mode))
    img, img2, _ = synth_images()
    E = 24
    noise, noise2 = rng_tensor(61, (E, 4, 16, 16)), rng_tensor(62, (E, 4, 16, 16))
    for idx in (1, 3):
        rs, re_, hw = feat.pair(img, img2, "a cup", up_ft_index=idx, ensemble_size=E, noise=noise, noise_edited=noise2)
        rs, re_ = rs.clone(), re_.clone()
        fs, _ = feat.forward(img, "a cup", up_ft_index=idx, ensemble_size=E, noise=noise)
        assert torch.equal(rs, fs), (mode, idx)
        fe, _ = feat.forward(img2, "a cup", up_ft_index=idx, ensemble_size=E, noise=noise2)
        assert torch.equal(re_, fe), (mode, idx)
        f6, _ = feat.forward(img, "a cup", up_ft_index=idx, ensemble_size=6, noise=noise[:6])
        assert torch.equal(rs[:6], f6), (mode, idx)


class ShiftedFeatures:
    """stands in for HipSDFeaturizer.pair: full-resolution random features; the edited image's are the source's moved by (dy rows, dx columns)"""

    def __init__(self, H, W, C, dx, dy, gpu):
        f = torch.randn(H, W, C, generator=torch.Generator().manual_seed(7))
        self.src = f.reshape(1, H * W, C).to(gpu)
        self.tgt = torch.roll(f, (dy, dx), (0, 1)).reshape(1, H * W, C).to(gpu)
        self.hw = (H, W)

    def pair(self, src, edited, prompt, **kw):
        return self.src, self.tgt, self.hw


def test_mean_distance_follows_a_real_shift(gpu):
    """the direction convention of the metric through mean_distance + ops.dift_match, without a network: features that really moved by dy = -2 rows and dx = +3
    columns (|dx| != |dy|) give distance 0 at every keypoint when edit_param says (dx, dy) = (3, -2), and |(dx - dy, dy - dx)| when it says them swapped"""
    from freefine_amd import metrics as FM
    H, W, dx, dy = 24, 20, 3, -2
    feat = ShiftedFeatures(H, W, 32, dx, dy, gpu)
    img = np.zeros((H, W, 3), dtype=np.uint8)
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[4:20, 3:15] = 255                                           # the moved points stay inside the frame (the roll wraps)
    kps = FM.default_keypoints(mask / 255.0, 30)
    assert len(kps) > 20
    right = FM.mean_distance(feat, img, img, mask, [dx, dy, 0, 0, 0, 0, 1, 1, 1], "x", kps)
    assert len(right) == len(kps) and all(d == 0.0 for d in right), right
    swapped = FM.mean_distance(feat, img, img, mask, [dy, dx, 0, 0, 0, 0, 1, 1, 1], "x", kps)
    assert all(abs(d - float(np.hypot(dx - dy, dy - dx))) <= 1e-6 for d in swapped), swapped


@pytest.mark.parametrize("mode", ["f32", "x3"])
def test_calculate_md_end_to_end(gpu, pipes, tmp_path, mode):
    """each sample's "generated" image is its source image and both get the same explicit noise, so the two feature maps are bit-identical rows of one batch and
    every keypoint matches itself: MD = |(dx, dy)| of the pure translation the edit_param claims.  A self-match says nothing about the DIRECTION of the shift:
    test_mean_distance_follows_a_real_shift checks that.  (The mask stays clear of the image border: within half a
    feature cell of it bilinear source coordinates are clamped and neighbouring pixels carry identical features.)"""
    from PIL import Image
    from freefine_amd import metrics as FM
    from golden_cases import rect_mask, rng_tensor
    pipe = pipes(mode)
    E = 2
    noise = rng_tensor(41, (E, 4, 16, 16))
    shifts = [(5, 12), (-12, 5)]                                      # (dx, dy): both of length 13, |dx| != |dy|
    data, data_kp = {}, {}
    for i, (dx, dy) in enumerate(shifts):
        img = np.random.default_rng(50 + i).integers(0, 256, (128, 128, 3), dtype=np.uint8)
        mask = rect_mask(128, 128, 40 + 8 * i, 92, 30, 84 - 8 * i, 255)
        Image.fromarray(img).save(tmp_path / f"img{i}.png")
        Image.fromarray(mask).save(tmp_path / f"mask{i}.png")
        sample = dict(ori_img_path=str(tmp_path / f"img{i}.png"), gen=str(tmp_path / f"img{i}.png"), ori_mask_path=str(tmp_path / f"mask{i}.png"),
                      edit_param=[dx, dy, 0, 0, 0, 0, 1, 1, 1], obj_label="a cup")
        data[str(i)] = {"instances": {"0": {"0": sample}}}
        data_kp[str(i)] = {"instances": {"0": {"0": dict(sample, keypoints=FM.default_keypoints(mask / 255.0, 30).tolist())}}}
    md = FM.calculate_md(data, "gen", pipe, ensemble_size=E, noise=noise)
    md_kp = FM.calculate_md(data_kp, "gen", pipe, ensemble_size=E, noise=noise)
    md_fn = FM.calculate_md(data, "gen", pipe, keypoints=lambda s, g, m: [[64, 64], [50, 40]], ensemble_size=E, noise=noise)
    print(f"calculate_md {mode}: {md!r} (per-sample keypoints {md_kp!r}, callable {md_fn!r}); expected 13.0")
    assert abs(md - 13.0) <= 1e-6 and md_kp == md and abs(md_fn - 13.0) <= 1e-6
