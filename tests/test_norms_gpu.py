"""GroupNorm, LayerNorm and row softmax (csrc/norms.h) per slice against fp64 on every route, plus the second grid-stride pass of the elementwise kernels.

Inputs.  Every (batch row, group) slice of a GroupNorm input (every row of a LayerNorm input) has statistics of its own: std = 2^U(-3, 3) and
mean = std * U(-8, 8) (LayerNorm: U(-16, 16)), so that statistics taken from the neighbouring row or group move the output by far more than any bound below
(tests/test_norms_ref_cpu.py shows that on every input used here).  The fp32 cases repeat with mean = r * std for r in {0, 4, 16}.  One slice of every
GroupNorm input is all zeros and one is the constant 2.0.  bf16 inputs are rounded first and the reference is computed from the rounded values.

Reference: F.group_norm / F.layer_norm / torch.softmax in fp64 on the CPU.

Bounds, per slice, S = max |ref| over the slice (derived, not measured):
  fp32   |out - ref| <  1e-5 * S                       the project's fp32 norm tolerance
  bf16   |out - ref| <= 2^-8 |ref| + 2^-16 S           half a bf16 ulp of the true value + room for the fp32 arithmetic before the rounding
  pair   |out - ref| <= 2^-17 |ref| + 1e-5 S           lo is the bf16 of a residual of at most 2^-9 |v|
  f8     |out - ref| <= 2^-4 |ref| + 2^-9 + 2e-2       the formula of test_fp8_groupnorm_and_every_configuration (values scaled by F8_ACT_SCALE)
The constant slice is held to its own bound instead (its sums are exact, mean = 2, var = 0, rstd = 1 / sqrt(eps)): every output finite and within 4 fp32 ulps
of |2 rstd gamma_c| -- the product that cancels in x * sc + (beta - mean * sc) -- from act(beta_c), plus the rounding of the output format.  The zero slice
must give beta_c bit for bit in fp32 (0 * sc + (beta - 0 * sc) is exact); with SiLU every pixel must give the same bits and lie within 4 fp32 ulps of the
fp64 SiLU(beta_c): the device's expf and the host's are different functions, so no host value is the bit pattern to expect.

Routes (ffn_gn_fused decides; every case asserts the route it was chosen for): the one-launch gn_fused_kernel, and gn_partial + gn_finalize + gn_apply.
HW = 25601 gives nchunk = 200 chunks of 129 pixels (chunk 198 partly filled, chunk 199 empty: p0 > HW); the clamp of nchunk at 256 needs HW >= 32768, hence
(1, 32769, 64) (256 chunks of 129 pixels: chunk 254 holds 3 pixels, chunk 255 none).  (1, 2048, 12) with G = 2 is there for the 4-wide pair apply (C % 8 != 0)
and is the shape of the bf16 refusal.

Measured on an MI355X, worst |err| / bound over all slices of all cases of a route (the assertion is < 1 for fp32, <= 1 otherwise):
  route          fp32: general  r = 0   r = 4   r = 16    bf16     pair
  fused                0.040    0.038   0.045   0.037     0.989    0.418
  three-launch         0.056    0.048   0.072   0.144     0.990    0.425
  f8 0.939; route flip (fused vs three-launch) fp32 0.056, bf16 0.989 of one ulp + 2 * 2^-16 S, pair 0.831
  LayerNorm fp32 0.270, bf16 0.988, pair 0.402; softmax fp32 0.008, bf16 0.895
bf16 sits at 0.99 by construction: half an ulp is 2^-8 |ref| at the bottom of a binade.  Before the statistics summed x - pivot (norms.h), r = 16 stood at 3.28
on the three-launch route ((33, 256, 64)) and 1.16 on the fused one ((3, 50, 64) with SiLU): E[x^2] - mean^2 from fp32 sums.  All figures are from the kernels
as they stand now.

Mean / std ratios 64 and 256 are run and printed, not asserted; |err| / S, beside torch's fp32 GroupNorm on the CPU on the same input:
  (2, 1024, 320), fused          r = 64: 1.1e-7 (torch 2.7e-6)    r = 256: 1.3e-7 (torch 1.1e-5)
  (2, 1025, 1280), three-launch  r = 64: 1.2e-6 (torch 2.7e-6)    r = 256: 3.9e-6 (torch 1.2e-5)

Two edits of norms.h and what they would do to this suite (read off the code, never run on a device):
  * `b = pix / HW` -> `0` in gn_apply_kernel: rows b > 0 get row 0's scale / shift, which test_norms_ref_cpu.py shows every bound rejects: every three-launch
    case with B > 1 fails in f32 and bf16 ((33, 256, 64), (2, 4096, 320), (2, 1025, 1280), (2, 25601, 64), (2, 2048, 32), the second-grid-pass shapes,
    batch-invariant (5, 4096, 64) against fp64, the row-chunk case) and (1, 2048, 12) in pair, the only shape whose pair output that kernel writes.
  * `min(cch - cbase, 256)` -> `256` in gn_partial_kernel: with cch < 256 one row of threads covers every pixel (ppi = 1 as computed from 256), so threads
    tid < cch still produce correct statistics, while threads tid >= cch read past their pixel's row and store past the chunk's [C][2] block of `partial`: over
    the neighbouring chunks' statistics -- a race their owners may lose -- past the LDS block, and for the last chunk of the last row past the workspace.  So
    nothing here fails deterministically: a three-launch case with C / EPC < 256 and more than one chunk ((2, 4096, 320), (2, 25601, 64), (1, 32769, 64),
    (33, 256, 64), ...) fails only when a stray store lands after the owner's, which is likely with hundreds of chunks but not certain.  What is certain is the
    stores out of bounds, which is why such an edit must not be run on a shared device.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import pair_value

pytestmark = pytest.mark.gpu

EPS = 1e-5
F8_ACT_SCALE = 16.0            # ops.F8_ACT_SCALE (asserted in the f8 test); a constant here so that the CPU reference test needs no device library

# (B, HW, C), G
FUSED_CASES = [((3, 64, 1280), 32), ((2, 1024, 320), 32), ((3, 50, 64), 32), ((2, 256, 16), 8), ((32, 256, 64), 32)]
THREE_CASES = [((33, 256, 64), 32), ((2, 4096, 320), 32), ((2, 1025, 1280), 32), ((1, 1100, 1216), 32), ((2, 25601, 64), 32), ((2, 2048, 32), 8),
               ((1, 32769, 64), 32), ((1, 2048, 12), 2)]
WRAP_F32 = ((3, 4096, 384), 32)           # 3 * 4096 * 384 / 4 = 1 179 648 work items of gn_apply_kernel<float> (> 4096 blocks x 256 threads)
WRAP_BF16 = ((3, 4096, 768), 32)          # 3 * 4096 * 768 / 8 = 1 179 648 of gn_apply_kernel<bf16> and gn_apply_pair8_kernel
WRAP_F8 = ((3, 4096, 1280), 32, 1408)     # 3 * 4096 * 1408 / 16 = 1 081 344 of gn_apply_f8_kernel (counted over Cp; 1280 / 16 = 80 would stay below)
F8_CASES = [((2, 1025, 320), 32, 384), ((3, 64, 64), 32, 128)]
PAIR_RAW_CASES = [c for c in THREE_CASES if c[0][0] > 1]
INVARIANT_CASES = [((48, 256, 320), 32), ((5, 4096, 64), 32)]
CHUNK_CASE = ((5, 2048, 64), 32)          # 512 KiB per fp32 row; three-launch at any number of rows (HW > 1024)
RATIOS = (0, 4, 16)
RATIOS_PRINTED = (64, 256)
RATIO_CASES = [((2, 1024, 320), 32), ((2, 1025, 1280), 32)]      # one per route; the second has the longest per-thread fp32 sums (129 pixels)

LN_M = (1, 5, 300)
LN_C = {"f32": (8, 200, 512, 516, 1536), "bf16": (8, 200, 1024, 1032, 3072)}      # small / ragged, cch 128 | 129 (MAXCH 2 | 6), the largest accepted
LN_C_REFUSED = {"f32": 1540, "bf16": 3080}
LN_PAIR_C = (200, 512)                    # planes, blocked
SM_N = (1, 63, 256, 257, 1000, 4096)
SM_SCALES = (1.0, 0.0884)

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "pair": torch.float32}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# inputs and the fp64 reference (CPU tensors; shared with tests/test_norms_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def zero_slice(B, G):
    return B - 1, 0


def const_slice(B, G):
    return 0, G - 1


def gn_ref(x, gamma, beta, G, eps=EPS):
    """fp64 GroupNorm of x [B, HW, C] (before the activation)"""
    return F.group_norm(x.double().transpose(1, 2), G, gamma.double(), beta.double(), eps).transpose(1, 2).contiguous()


def gn_case(B, HW, C, G, mode="f32", ratio=None):
    """-> x [B, HW, C] (bf16 for mode 'bf16', else fp32), gamma, beta (fp32), fp64 reference of GroupNorm(x).  Read-only: the tensors are shared."""
    return _gn_case(B, HW, C, G, "bf16" if mode == "bf16" else "f32", ratio)


@functools.lru_cache(maxsize=3)
def _gn_case(B, HW, C, G, dtype, ratio):
    g = torch.Generator().manual_seed(B * 1000003 + HW * 1009 + C * 7 + G)
    cg = C // G
    std = torch.exp2(torch.rand(B, G, generator=g) * 6 - 3)
    u = torch.rand(B, G, generator=g) * 16 - 8
    mean = std * (u if ratio is None else float(ratio))
    x = torch.randn(B, HW, G, cg, generator=g) * std[:, None, :, None] + mean[:, None, :, None]
    zb, zg = zero_slice(B, G)
    cb, cgi = const_slice(B, G)
    x[zb, :, zg] = 0.0
    x[cb, :, cgi] = 2.0
    x = x.reshape(B, HW, C).to(DT[dtype])
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return x, gamma, beta, gn_ref(x, gamma, beta, G)


def ln_case(M, C, dtype="f32"):
    g = torch.Generator().manual_seed(M * 100003 + C)
    std = torch.exp2(torch.rand(M, 1, generator=g) * 6 - 3)
    mean = std * (torch.rand(M, 1, generator=g) * 32 - 16)
    x = (torch.randn(M, C, generator=g) * std + mean).to(DT[dtype])
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return x, gamma, beta, F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), EPS)


def sm_case(N, scale, dtype="f32"):
    """five rows of scores (before the scale): random of standard deviation 3, all equal, one dominant, spanning +-90 after scaling, random again"""
    g = torch.Generator().manual_seed(N)
    s32 = torch.tensor(scale, dtype=torch.float32).item()              # the kernel's scale is a float
    x = torch.randn(5, N, generator=g) * 3
    x[1] = 1.25
    x[2, N // 2] += 60.0
    x[3] = (torch.linspace(-90.0, 90.0, N) if N > 1 else torch.tensor([90.0]))[torch.randperm(N, generator=g)]
    x = (x / s32).to(DT[dtype])
    return x, s32, torch.softmax(x.double() * s32, -1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _slices(t, G):
    B, HW, C = t.shape
    return t.reshape(B, HW, G, C // G)


def gn_worst(mode, out, ref, G, skip=(), against=None):
    """[B, G]: per slice, the largest |out - ref| / bound of `mode` ('f32' must stay < 1, 'bf16' and 'pair' <= 1).  `skip`: slices reported as 0.
    `against`: measure out - against instead (the bound is still taken from ref)."""
    ref = ref.double()
    a = _slices(ref.abs(), G)
    S = a.amax(dim=(1, 3), keepdim=True)
    err = _slices((out.double() - (ref if against is None else against.double())).abs(), G)
    if mode == "f32":
        bound = 1e-5 * S
    elif mode == "bf16":
        bound = 2.0 ** -8 * a + 2.0 ** -16 * S
    elif mode == "pair":
        bound = 2.0 ** -17 * a + 1e-5 * S
    else:
        raise ValueError(mode)
    q = (err / bound).amax(dim=(1, 3))
    for b, g in skip:
        q[b, g] = 0.0
    return q


def bf16_agreement(a, b, ref, G, skip=()):
    """[B, G]: per slice, the largest |a - b| / (one bf16 ulp of the larger of the two + 2 * 2^-16 S) for two bf16 results of the same operation.  Each is the
    rounding of an fp32 value within 2^-16 S of ref, so each is within half an ulp of its own value, and the two values are within 2 * 2^-16 S of each other:
    two correct results can be a whole ulp apart, which the bound against ref (half an ulp) does not allow for."""
    a, b = a.double(), b.double()
    S = _slices(ref.double().abs(), G).amax(dim=(1, 3), keepdim=True)
    big = torch.maximum(a.abs(), b.abs())
    ulp = torch.where(big > 0, torch.exp2(torch.floor(torch.log2(big.clamp_min(1e-300))) - 7), torch.zeros_like(big))
    q = (_slices((a - b).abs(), G) / (_slices(ulp, G) + 2.0 ** -15 * S)).amax(dim=(1, 3))
    for bb, g in skip:
        q[bb, g] = 0.0
    return q


def row_worst(mode, out, ref):
    """the same per row of [M, C] -> [M]"""
    return gn_worst(mode, out[:, None, :], ref[:, None, :], 1)[:, 0]


def passes(mode, q):
    return bool((q < 1).all()) if mode == "f32" else bool((q <= 1).all())      # a NaN fails either


def f8_worst(y8, ref, C, qs=F8_ACT_SCALE):
    """largest |dequantised - ref * qs| / (2^-4 |ref * qs| + 2^-9 + 2e-2): e4m3 has 3 mantissa bits and a subnormal step of 2^-9; bf16 input"""
    r = ref.double() * qs
    deq = y8.view(torch.float8_e4m3fn).float()[..., :C].double()
    return ((deq - r.clamp(-448, 448)).abs() / (r.abs() * 2.0 ** -4 + 2.0 ** -9 + 2e-2)).max()


def act(ref, silu):
    return F.silu(ref) if silu else ref


def ulp32(v):
    """the fp32 ulp of |v| (double tensor)"""
    return torch.exp2(torch.floor(torch.log2(v.abs())) - 23)


def check_special_slices(mode, silu, out, values, gamma, beta, G, zero=True):
    """out: what the kernel wrote ([B, HW, C] fp32 / bf16; for 'pair' pass None), values: the same as doubles."""
    B, HW, C = values.shape
    cg = C // G
    zb, zg = zero_slice(B, G)
    cb, cgi = const_slice(B, G)
    if mode == "f32" and zero:
        sl = _slices(out, G)[zb, :, zg]                                                    # [HW, cg]
        bz = beta[zg * cg:(zg + 1) * cg]
        if not silu:
            assert torch.equal(sl, bz.expand(HW, cg)), "zero slice: not beta bit for bit"
        else:
            assert torch.equal(sl, sl[:1].expand(HW, cg)), "zero slice: pixels differ"
            want = F.silu(bz.double())
            assert ((sl[0].double() - want).abs() <= 4 * ulp32(want)).all(), "zero slice: not SiLU(beta)"
    sl = _slices(values, G)[cb, :, cgi]
    assert torch.isfinite(sl).all(), "constant slice: not finite"
    gc, bc = gamma[cgi * cg:(cgi + 1) * cg].double(), beta[cgi * cg:(cgi + 1) * cg].double()
    rstd = torch.tensor(1.0 / math.sqrt(torch.tensor(EPS, dtype=torch.float32).item()), dtype=torch.float32).double()
    a = act(bc, silu)
    tol = 4 * ulp32(2 * rstd * gc)
    if mode == "bf16":
        tol = tol + (2.0 ** -8 + 2.0 ** -16) * a.abs()
    elif mode == "pair":
        tol = tol + (2.0 ** -17 + 1e-5) * a.abs()
    worst = ((sl - a).abs() / tol).max().item()
    assert worst <= 1, f"constant slice: {worst:.2f} of 4 ulps of |2 rstd gamma| (+ the output rounding) from act(beta)"


def values_of(mode, out, C):
    out = out.cpu()
    return pair_value(out, C) if mode == "pair" else out.double()


def check_gn(mode, silu, out, case, G, tag, zero=True):
    """per-slice bound (the constant slice apart) + the two special slices; -> worst fraction of the bound"""
    x, gamma, beta, ref = case
    B, HW, C = x.shape
    out = out.cpu()
    vals = values_of(mode, out, C)
    q = gn_worst(mode, vals, act(ref, silu), G, skip=[const_slice(B, G)])
    print(f"NORMS {tag} {tuple(x.shape)} G={G} {mode} silu={int(silu)}: worst {q.max().item():.3f} of the bound")
    assert passes(mode, q), (tag, mode, silu, q.max().item(), divmod(int(q.argmax()), G))
    check_special_slices(mode, silu, None if mode == "pair" else out, vals, gamma, beta, G, zero)
    return q.max().item()


def _gn(gpu, mode, case, G, silu, **kw):
    from freefine_amd import ops
    x, gamma, beta, _ = case
    out = ops.groupnorm(x.to(gpu), gamma.to(gpu), beta.to(gpu), G, EPS, silu=silu, pair=(mode == "pair"), **kw)
    if mode == "pair":
        assert ops.pair_width(out) == x.shape[-1] and out.dtype == torch.bfloat16 and tuple(out.shape) == (*x.shape[:-1], 2 * x.shape[-1])
    return out


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _modes(shape, G):
    return ("f32", "pair") if shape[-1] % 8 else ("f32", "bf16", "pair")      # bf16 on the three-launch route needs C % 8 == 0 (refused: see below)


GN_PARAMS = [pytest.param(shape, G, fused, mode, id=f"{'fused' if fused else 'three'}-{'x'.join(map(str, shape))}-g{G}-{mode}")
             for cases, fused in ((FUSED_CASES, True), (THREE_CASES, False)) for shape, G in cases for mode in _modes(shape, G)]


@pytest.mark.parametrize("shape,G,fused,mode", GN_PARAMS)
def test_groupnorm_per_slice(gpu, shape, G, fused, mode):
    from freefine_amd import _lib as L
    B, HW, C = shape
    assert bool(L.load().ffn_gn_fused(B, HW, C, G)) == fused, "the route rule moved: choose a shape that is on this route again"
    for ratio in (None,) + (RATIOS if mode == "f32" else ()):
        if shape == (32, 256, 64):       # rows 0..31 of the 33-row input (test_groupnorm_route_flip_agrees); its zero slice is in row 32
            x, gamma, beta, ref = gn_case(33, HW, C, G, mode, ratio)
            case = (x[:32], gamma, beta, ref[:32])
        else:
            case = gn_case(B, HW, C, G, mode, ratio)
        for silu in (False, True):
            check_gn(mode, silu, _gn(gpu, mode, case, G, silu), case, G, f"ratio={ratio}", zero=shape != (32, 256, 64))


@pytest.mark.parametrize("mode", ["f32", "bf16", "pair"])
def test_groupnorm_route_flip_agrees(gpu, mode):
    """B = 32 takes the fused kernel, B = 33 the three launches: rows 0..31 of the same input must agree within the bound (bf16: within one ulp, see
    bf16_agreement)"""
    from freefine_amd import _lib as L
    lib = L.load()
    assert lib.ffn_gn_fused(32, 256, 64, 32) and not lib.ffn_gn_fused(33, 256, 64, 32)
    case = gn_case(33, 256, 64, 32, mode)
    x, gamma, beta, ref = case
    for silu in (False, True):
        o33 = values_of(mode, _gn(gpu, mode, case, 32, silu), 64)[:32]
        o32 = values_of(mode, _gn(gpu, mode, (x[:32], gamma, beta, ref[:32]), 32, silu), 64)
        if mode == "bf16":
            q = bf16_agreement(o32, o33, act(ref[:32], silu), 32, skip=[const_slice(32, 32)])
        else:
            q = gn_worst(mode, o32, act(ref[:32], silu), 32, skip=[const_slice(32, 32)], against=o33)
        print(f"NORMS route flip {mode} silu={int(silu)}: fused vs three-launch {q.max().item():.3f} of the bound")
        assert passes(mode, q), (mode, silu, q.max().item())


@pytest.mark.parametrize("shape,G", RATIO_CASES, ids=["fused", "three"])
def test_groupnorm_large_offsets_are_reported(gpu, shape, G):
    """mean / std of 64 and 256: printed beside torch's own fp32 error, not asserted (nobody has derived a bound for E[x^2] - mean^2 there)"""
    for ratio in RATIOS_PRINTED:
        case = gn_case(*shape, G, "f32", ratio)
        x, gamma, beta, ref = case
        skip = [const_slice(shape[0], G)]
        q = gn_worst("f32", _gn(gpu, "f32", case, G, False).cpu(), ref, G, skip=skip)
        t = gn_worst("f32", F.group_norm(x.transpose(1, 2), G, gamma, beta, EPS).transpose(1, 2), ref, G, skip=skip)
        print(f"NORMS ratio={ratio} {shape} (not asserted): kernel {q.max().item() * 1e-5:.2e} of S, torch fp32 on the CPU {t.max().item() * 1e-5:.2e}")
        assert torch.isfinite(q).all()


@pytest.mark.parametrize("shape,G", PAIR_RAW_CASES + [WRAP_BF16], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"g{v}")
def test_groupnorm_pair_raw_against_fp64(gpu, shape, G):
    """ffn_groupnorm_pair_raw: both outputs against fp64 (its bit-for-bit test compares them with kernels that share the statistics pass)"""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    B, HW, C = shape
    assert C % 8 == 0 and not L.load().ffn_gn_fused(B, HW, C, G), "this shape no longer reaches gn_apply_pair8_kernel<., RAW>"
    case = gn_case(B, HW, C, G, "pair")
    x, gamma, beta, ref = case
    xd, gd, bd = x.to(gpu), gamma.to(gpu), beta.to(gpu)
    for silu in (False, True):
        y, yr = ops.groupnorm_pair_raw(xd, gd, bd, G, EPS, silu=silu)
        assert ops.pair_width(y) == C and ops.pair_width(yr) == C and tuple(y.shape) == tuple(yr.shape) == (B, HW, 2 * C)
        check_gn("pair", silu, y, case, G, "pair_raw")
        q = gn_worst("pair", pair_value(yr.cpu(), C), x, G, skip=[zero_slice(B, G)])
        assert passes("pair", q), ("raw", silu, q.max().item())
        zb, zg = zero_slice(B, G)
        assert (_slices(pair_value(yr.cpu(), C), G)[zb, :, zg] == 0).all()


@pytest.mark.parametrize("shape,G,Cp", F8_CASES + [WRAP_F8], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_groupnorm_f8_per_element(gpu, shape, G, Cp):
    # no route to assert: ffn_groupnorm_f8 never asks ffn_gn_fused, it always runs gn_partial + gn_finalize + gn_apply_f8
    from freefine_amd import ops
    assert ops.F8_ACT_SCALE == F8_ACT_SCALE
    B, HW, C = shape
    x, gamma, beta, ref = gn_case(B, HW, C, G, "bf16")
    xd, gd, bd = x.to(gpu), gamma.to(gpu), beta.to(gpu)
    for silu in (False, True):
        y8 = ops.groupnorm_f8(xd, gd, bd, G, EPS, Cp, silu=silu).cpu()
        assert y8.shape == (B, HW, Cp) and y8.dtype == torch.uint8 and (y8[..., C:] == 0).all()
        w = f8_worst(y8, act(ref, silu), C).item()
        print(f"NORMS f8 {shape} Cp={Cp} silu={int(silu)}: worst {w:.3f} of the bound")
        assert w <= 1, (silu, w)


@pytest.mark.parametrize("case,mode", [(WRAP_F32, "f32"), (WRAP_BF16, "bf16"), (WRAP_BF16, "pair")], ids=["3x4096x384-f32", "3x4096x768-bf16", "3x4096x768-pair"])
def test_groupnorm_apply_second_grid_pass(gpu, case, mode):
    """more than 4096 x 256 work items: the grid-stride loop of the apply kernel runs a second time for the last rows"""
    from freefine_amd import _lib as L
    (B, HW, C), G = case
    assert B * HW * C // (4 if mode == "f32" else 8) > 4096 * 256
    assert not L.load().ffn_gn_fused(B, HW, C, G)
    case = gn_case(B, HW, C, G, mode)
    for silu in (False, True):
        check_gn(mode, silu, _gn(gpu, mode, case, G, silu), case, G, "wrap")


@pytest.mark.parametrize("mode", ["f32", "bf16", "pair"])
@pytest.mark.parametrize("shape,G", INVARIANT_CASES, ids=["48x256x320-fused-in-chunks", "5x4096x64-three"])
def test_groupnorm_batch_invariant(gpu, shape, G, mode):
    """under ops.batch_invariant() the result for B rows is, bit for bit, the per-row results concatenated"""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    B, HW, C = shape
    if B == 48:
        assert lib.ffn_gn_fused(1, HW, C, G) and not lib.ffn_gn_fused(B, HW, C, G) and lib.ffn_gn_fused(24, HW, C, G)
    else:
        assert not lib.ffn_gn_fused(1, HW, C, G) and not lib.ffn_gn_fused(B, HW, C, G)
    case = gn_case(B, HW, C, G, mode)
    x, gamma, beta, ref = case
    with ops.batch_invariant():
        full = _gn(gpu, mode, case, G, True)
        rows = torch.cat([_gn(gpu, mode, (x[b:b + 1], gamma, beta, None), G, True) for b in range(B)])
    assert torch.equal(_bits(full), _bits(rows))
    check_gn(mode, True, full, case, G, "batch_invariant")


def test_groupnorm_refusals_write_nothing(gpu):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    stream = torch.cuda.current_stream().cuda_stream

    def operands(B, HW, C, dtype, width=None):
        x = torch.randn(B, HW, C, generator=g).to(dtype).to(gpu)
        out = torch.full((B, HW, width or C), -7.0, dtype=torch.bfloat16 if width else dtype, device=gpu)
        return x, torch.randn(C, generator=g).to(gpu), torch.randn(C, generator=g).to(gpu), out

    # C / G odd (either route would read channel pairs across a group's edge)
    for dtype in (torch.float32, torch.bfloat16):
        x, ga, be, out = operands(1, 64, 96, dtype)
        with pytest.raises(L.FreeFineHipError):
            ops.groupnorm(x, ga, be, 32, EPS, out=out)
        torch.cuda.synchronize()
        assert (out == -7.0).all()
    # three-launch route, bf16, C not a multiple of 8 (16-byte loads)
    assert not lib.ffn_gn_fused(1, 2048, 12, 2)
    x, ga, be, out = operands(1, 2048, 12, torch.bfloat16)
    with pytest.raises(L.FreeFineHipError):
        ops.groupnorm(x, ga, be, 2, EPS, out=out)
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    # pair output from bf16 input: the wrapper refuses, and so does the library on either route
    for (B, HW, C) in [(2, 64, 64), (1, 2048, 64)]:
        x, ga, be, out = operands(B, HW, C, torch.bfloat16, width=2 * C)
        with pytest.raises((AssertionError, L.FreeFineHipError)):
            ops.groupnorm(x, ga, be, 32, EPS, pair=True)
        ws = ops.gn_workspace(B, HW, C, gpu)
        rc = lib.ffn_groupnorm(stream, L.FFN_BF16, x.data_ptr(), out.data_ptr(), ga.data_ptr(), be.data_ptr(), B, HW, C, 32, EPS, L.NORM_OUT_PAIR,
                               ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and (out == -7.0).all()
    # ffn_gn_stats: C not a multiple of G
    x, ga, be, _ = operands(1, 2048, 64, torch.float32)
    ws = ops.gn_workspace(1, 2048, 64, gpu)
    for w in ws:
        w.fill_(-7.0)
    rc = lib.ffn_gn_stats(stream, L.FFN_F32, x.data_ptr(), ga.data_ptr(), be.data_ptr(), 1, 2048, 64, 3, EPS, ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and all((w == -7.0).all() for w in ws)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,C", [(m, c) for m in ("f32", "bf16") for c in LN_C[m]])
def test_layernorm_per_row(gpu, mode, C):
    from freefine_amd import ops
    for M in LN_M:
        x, gamma, beta, ref = ln_case(M, C, mode)
        out = ops.layernorm(x.to(gpu), gamma.to(gpu), beta.to(gpu), EPS).cpu()
        q = row_worst(mode, out, ref)
        print(f"NORMS layernorm {mode} M={M} C={C}: worst {q.max().item():.3f} of the bound")
        assert passes(mode, q), (M, C, q.max().item(), int(q.argmax()))


@pytest.mark.parametrize("C", LN_PAIR_C)
def test_layernorm_pair_per_row(gpu, C):
    from freefine_amd import ops
    for M in LN_M:
        x, gamma, beta, ref = ln_case(M, C, "pair")
        xd, gd, bd = x.to(gpu), gamma.to(gpu), beta.to(gpu)
        p = ops.layernorm(xd, gd, bd, EPS, pair=True)
        assert ops.pair_width(p) == C and tuple(p.shape) == (M, 2 * C)
        assert torch.equal(_bits(p), _bits(ops.split_pair(ops.layernorm(xd, gd, bd, EPS), C)))
        q = row_worst("pair", pair_value(p.cpu(), C), ref)
        print(f"NORMS layernorm pair M={M} C={C}: worst {q.max().item():.3f} of the bound")
        assert passes("pair", q), (M, C, q.max().item())


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_layernorm_refuses_one_step_past_its_largest_row(gpu, mode):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    C = LN_C_REFUSED[mode]
    x, gamma, beta, _ = ln_case(5, C, mode)
    out = torch.full((5, C), -7.0, dtype=DT[mode], device=gpu)
    with pytest.raises(L.FreeFineHipError):
        ops.layernorm(x.to(gpu), gamma.to(gpu), beta.to(gpu), EPS, out=out)
    if mode == "f32":
        with pytest.raises(L.FreeFineHipError):
            ops.layernorm(x.to(gpu), gamma.to(gpu), beta.to(gpu), EPS, pair=True)
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# row softmax
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def sm_tolerance(mode, ref):
    t = 2e-5 * ref.amax(-1, keepdim=True).expand_as(ref)
    return t if mode == "f32" else t + 2.0 ** -8 * ref


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("N", SM_N)
def test_softmax_rows_per_row(gpu, mode, N):
    from freefine_amd import ops
    for scale in SM_SCALES:
        x, s32, ref = sm_case(N, scale, mode)
        out = ops.softmax_rows(x.to(gpu), s32).cpu().double()
        assert not torch.isnan(out).any()
        tol = sm_tolerance(mode, ref)
        q = ((out - ref).abs() / tol).amax(-1)
        print(f"NORMS softmax {mode} N={N} scale={scale}: worst {q.max().item():.3f} of the bound")
        assert (q <= 1).all(), (N, scale, q)
        assert ((out.sum(-1) - 1).abs() <= tol.sum(-1)).all(), (N, scale, out.sum(-1))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# elementwise.h: every grid_for kernel once above 4096 blocks x 256 threads (the second pass of its grid-stride loop), compared as its own test compares it
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_elementwise_second_grid_pass(gpu):
    from freefine_amd import ops
    from test_ops_gpu import relerr
    LIMIT = 4096 * 256
    g = torch.Generator().manual_seed(21)

    def rn(*shape, dtype=torch.float32):
        return torch.randn(*shape, generator=g).to(dtype).to(gpu)

    # cast: one element per work item
    a = rn(LIMIT + 4096)
    assert torch.equal(ops.cast(a, torch.bfloat16), a.to(torch.bfloat16))
    assert torch.equal(ops.cast(a.to(torch.bfloat16), torch.float32), a.to(torch.bfloat16).float())
    # concat: one 16-byte chunk per work item; 4100 rows x (512 + 512) / 4
    a, b = rn(4100, 512), rn(4100, 512)
    assert 4100 * 1024 // 4 > LIMIT and torch.equal(ops.concat(a, b), torch.cat([a, b], -1))
    # add / relu: four elements per work item
    a, b = rn(4 * LIMIT + 1024), rn(4 * LIMIT + 1024)
    assert torch.equal(ops.relu(a), torch.relu(a))
    assert relerr(ops.add(a, b), a.double() + b.double()) < 1e-6
    assert (ops.add(a, b)[-1024:] == (a + b)[-1024:]).all()
    # split_pair: 4 columns per work item when C % 8 != 0 (C = 1028: planes), 8 otherwise (C = 2048: blocked)
    for C in (1028, 2048):
        x = rn(4100, C)
        assert 4100 * C // (4 if C % 8 else 8) > LIMIT
        p = ops.split_pair(x, C)
        if C % 32 == 0:
            blk = p.view(4100, C // 32, 2, 32)
            hi, lo = blk[:, :, 0].reshape(4100, C).float(), blk[:, :, 1].reshape(4100, C).float()
        else:
            hi, lo = p[:, :C].float(), p[:, C:].float()
        assert torch.equal(hi, x.to(torch.bfloat16).float()) and torch.equal(lo, (x - hi).to(torch.bfloat16).float())
    # image_to_nhwc: one output element per work item (364 * 364 * 8)
    img = torch.randint(0, 256, (1, 364, 364, 3), generator=g, dtype=torch.uint8).to(gpu)
    x = ops.image_to_nhwc(img, 8, torch.float32)
    assert x.numel() > LIMIT and relerr(x[..., :3], img.reshape(1, -1, 3).float() / 127.5 - 1) < 1e-6 and (x[..., 3:] == 0).all()
    assert (x[0, -64:, :3] - (img.reshape(1, -1, 3)[0, -64:].float() / 127.5 - 1)).abs().max() < 1e-6
    # nhwc_to_nchw_f32: one element per work item (5 x 4 x 230 x 230)
    e = rn(5, 230 * 230, 4)
    assert e.numel() > LIMIT and torch.equal(ops.nhwc_to_nchw_f32(e, 4, 230, 230), e.permute(0, 2, 1).reshape(5, 4, 230, 230))
    # pack_nchw: one output element per work item (4 rows x 192 x 192 x 8)
    lat = rn(2, 4, 192, 192)
    p = ops.pack_nchw(lat, [0, 1, 0, 1], 8, torch.float32)
    ref = torch.cat([lat, lat]).permute(0, 2, 3, 1).reshape(4, 192 * 192, 4)
    assert p.numel() > LIMIT and torch.equal(p[..., :4], ref) and (p[..., 4:] == 0).all()
    # cfg_masked / ddim_inv_step: one element per work item (2 x 4 x 364 x 364)
    eu, ec, x = rn(2, 4, 364, 364), rn(2, 4, 364, 364), rn(2, 4, 364, 364)
    mask = (torch.rand(364, 364, generator=g) > 0.5).float().to(gpu)
    assert eu.numel() > LIMIT
    for m, ref in ((mask.reshape(-1), eu + 7.5 * (ec - eu) * mask), (None, eu + 7.5 * (ec - eu))):
        out = ops.cfg_masked(eu, ec, m, 7.5)
        assert relerr(out, ref) < 1e-6 and (out[1, 3] - ref[1, 3]).abs().max() <= 1e-6 * ref[1, 3].abs().max()
    xn, p0 = ops.ddim_inv_step(eu, x, 0.3, 0.95, 0.9, 0.43, want_pred_x0=True)
    rp0 = (x - 0.3 * eu) / 0.95
    assert relerr(p0, rp0) < 1e-6 and relerr(xn, 0.9 * rp0 + 0.43 * eu) < 1e-6
    assert relerr(p0[1, 3], rp0[1, 3]) < 1e-6 and relerr(xn[1, 3], (0.9 * rp0 + 0.43 * eu)[1, 3]) < 1e-6
    # resize_bilinear: four channels per work item (2 x 365 x 365 x 16 / 4), align_corners = True; 183 -> 365 makes the source step exactly 1 / 2, so the
    # fp32 source coordinates carry no rounding that grows with the size and the tolerance of the small shapes holds
    t = rn(2, 183 * 183, 16)
    ref = F.interpolate(t.double().view(2, 183, 183, 16).permute(0, 3, 1, 2), size=(365, 365), mode="bilinear", align_corners=True)
    ref = ref.permute(0, 2, 3, 1).reshape(2, 365 * 365, 16)
    assert ref.numel() // 4 > LIMIT
    for relu in (False, True):
        out, r = ops.resize_bilinear(t, 2, 183, 183, 365, 365, relu=relu), (F.relu(ref) if relu else ref)
        assert relerr(out, r) < 1e-6 and relerr(out[1, -365 * 16:], r[1, -365 * 16:]) < 1e-6
