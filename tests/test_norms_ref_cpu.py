"""The bounds of tests/test_norms_gpu.py, checked without a device: on every input that module uses, torch's own fp32 GroupNorm / LayerNorm / softmax on
the CPU (rounded to the output format) stays inside the bound against the fp64 reference, and an output computed with the statistics of the neighbouring
batch row, or of the neighbouring group, is rejected in every slice it touches.  So a kernel that passes the device tests is no worse than torch's fp32
kernels by more than the bound, and one that mixes up rows or groups cannot pass."""
import pytest
import torch
import torch.nn.functional as F

from test_norms_gpu import (CHUNK_CASE, EPS, F8_ACT_SCALE, F8_CASES, FUSED_CASES, INVARIANT_CASES, LN_C, LN_M, LN_PAIR_C, RATIOS, SM_N, SM_SCALES, THREE_CASES,
                            WRAP_BF16, WRAP_F32, WRAP_F8, _slices, act, check_special_slices, const_slice, f8_worst, gn_case, gn_worst, ln_case, passes,
                            row_worst, sm_case, sm_tolerance, zero_slice)

SMALL = FUSED_CASES + THREE_CASES + [CHUNK_CASE]                         # these repeat with the mean / std ratios, as the device tests do
LARGE = INVARIANT_CASES + [WRAP_F32, WRAP_BF16]
F8 = F8_CASES + [WRAP_F8]


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else f"g{v}"


def to_format(mode, v):
    """fp32 values as the output format of `mode` holds them, as doubles"""
    if mode == "bf16":
        return v.to(torch.bfloat16).double()
    if mode == "pair":
        hi = v.to(torch.bfloat16).float()
        return hi.double() + (v - hi).to(torch.bfloat16).double()
    return v.double()


def torch_f32(x, gamma, beta, G, silu):
    y = F.group_norm(x.float().transpose(1, 2), G, gamma, beta, EPS).transpose(1, 2)
    return F.silu(y) if silu else y


def with_statistics_of(x, gamma, beta, G, shift_rows, shift_groups):
    """fp64 GroupNorm of x in which slice (b, g) is normalised with the mean and variance of slice (b - shift_rows, g - shift_groups)"""
    xs = _slices(x.double(), G)
    mean = xs.mean(dim=(1, 3), keepdim=True)
    var = xs.var(dim=(1, 3), unbiased=False, keepdim=True)
    mean, var = mean.roll((shift_rows, shift_groups), (0, 2)), var.roll((shift_rows, shift_groups), (0, 2))
    y = ((xs - mean) / torch.sqrt(var + EPS)).reshape(x.shape)
    return y * gamma.double() + beta.double()


@pytest.mark.parametrize("shape,G", SMALL + LARGE, ids=_id)
def test_groupnorm_bounds_hold_for_torch_fp32_and_reject_wrong_statistics(shape, G):
    B, HW, C = shape
    special = [const_slice(B, G)]
    for mode in ("f32", "bf16", "pair"):
        if mode == "bf16" and C % 8:
            continue
        for ratio in (None,) + (RATIOS if mode == "f32" and (shape, G) in SMALL else ()):
            x, gamma, beta, ref = gn_case(B, HW, C, G, mode, ratio)
            for silu in (False, True):
                y = torch_f32(x, gamma, beta, G, silu)
                if mode == "bf16":
                    y = y.to(torch.bfloat16)
                vals = to_format(mode, y)
                q = gn_worst(mode, vals, act(ref, silu), G, skip=special)
                assert passes(mode, q), (mode, ratio, silu, q.max().item())
                check_special_slices(mode, silu, None, vals, gamma, beta, G, zero=False)      # the bit checks of the zero slice are the device's
        # statistics of the neighbouring batch row / group: every slice but the two special ones must be rejected
        x, gamma, beta, ref = gn_case(B, HW, C, G, mode)
        keep = torch.ones(B, G, dtype=torch.bool)
        keep[const_slice(B, G)] = keep[zero_slice(B, G)] = False
        for rows, groups in ((1, 0), (0, 1)):
            if rows and B == 1:
                continue                                                    # no neighbouring row
            wrong = with_statistics_of(x, gamma, beta, G, rows, groups).float()
            q = gn_worst(mode, to_format(mode, wrong.to(torch.bfloat16) if mode == "bf16" else wrong), ref, G)
            assert (q[keep] > 1).all(), (mode, "rows" if rows else "groups", q[keep].min().item())


@pytest.mark.parametrize("shape,G,Cp", F8, ids=_id)
def test_groupnorm_f8_bound_holds_for_torch_fp32(shape, G, Cp):
    B, HW, C = shape
    x, gamma, beta, ref = gn_case(B, HW, C, G, "bf16")
    for silu in (False, True):
        y = torch_f32(x, gamma, beta, G, silu) * F8_ACT_SCALE
        y8 = torch.zeros(B, HW, Cp)
        y8[..., :C] = y.clamp(-448, 448)
        assert f8_worst(y8.to(torch.float8_e4m3fn).view(torch.uint8), act(ref, silu), C) <= 1
    for rows, groups in ((1, 0), (0, 1)):
        wrong = with_statistics_of(x, gamma, beta, G, rows, groups).float() * F8_ACT_SCALE
        assert f8_worst(wrong.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8), ref, C) > 1


@pytest.mark.parametrize("mode,C", [(m, c) for m in ("f32", "bf16") for c in LN_C[m]] + [("pair", c) for c in LN_PAIR_C])
def test_layernorm_bounds_hold_for_torch_fp32_and_reject_wrong_statistics(mode, C):
    for M in LN_M:
        x, gamma, beta, ref = ln_case(M, C, mode)
        y = F.layer_norm(x.float(), (C,), gamma, beta, EPS)
        q = row_worst(mode, to_format(mode, y.to(torch.bfloat16) if mode == "bf16" else y), ref)
        assert passes(mode, q), (mode, M, C, q.max().item())
        if M > 1:       # the statistics of the neighbouring row
            xd = x.double()
            mean, var = xd.mean(-1, keepdim=True).roll(1, 0), xd.var(-1, unbiased=False, keepdim=True).roll(1, 0)
            wrong = ((xd - mean) / torch.sqrt(var + EPS) * gamma.double() + beta.double()).float()
            q = row_worst(mode, to_format(mode, wrong.to(torch.bfloat16) if mode == "bf16" else wrong), ref)
            assert (q > 1).all(), (mode, M, C, q.min().item())


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("N", SM_N)
def test_softmax_bounds_hold_for_torch_fp32(mode, N):
    for scale in SM_SCALES:
        x, s32, ref = sm_case(N, scale, mode)
        y = torch.softmax(x.float() * s32, -1)
        out = (y.to(torch.bfloat16) if mode == "bf16" else y).double()
        tol = sm_tolerance(mode, ref)
        assert ((out - ref).abs() <= tol).all() and ((out.sum(-1) - 1).abs() <= tol.sum(-1)).all(), (N, scale)
        if N > 1:       # the neighbouring row's maximum and sum
            z = x.double() * s32
            m = z.amax(-1, keepdim=True)
            wrong = torch.exp(z - m.roll(1, 0)) / torch.exp(z - m).sum(-1, keepdim=True).roll(1, 0)
            assert not ((wrong - ref).abs() <= tol).all(-1)[:4].any(), (N, scale)       # rows 0-3 differ from their neighbours
