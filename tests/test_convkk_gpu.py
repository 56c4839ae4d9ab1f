"""GPU: ffn_conv2d (csrc/convkk.h), the KH x KW implicit GEMM on the exact-fp32 MFMA, through the C ABI.

The gate is derived, not measured: an fp32 fma chain of length K deviates from the exact sum by at most gamma (|x| * |w| + |b|) elementwise, gamma = (K + 2) 2^-24
(K roundings of the chain, one of the bias addition, one to spare for the second-order terms; the order of the chain does not enter the bound).  The right-hand
side is computed in fp64 here, per output element, and the result is held to fp64 F.conv2d of the same fp32 values.  Every case is the smallest at which its
failure mode exists.  Inputs live in column views of wider buffers: the columns outside the input view hold NaN (reading them shows), everything outside the
output view -- the other columns, the rows past M -- holds a sentinel that must come back bit for bit."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
SENTINEL = -777.25

# name: (B, H, W, Cin, N, (KH, KW), stride, (pad_h, pad_w))
CASES = {
    "stem_3x3_s2": (2, 13, 11, 4, 32, (3, 3), 2, (0, 0)),
    "1x7_on_5x5": (1, 5, 5, 20, 12, (1, 7), 1, (0, 3)),                  # the kernel is longer than the image
    "7x1_on_5x5": (1, 5, 5, 20, 12, (7, 1), 1, (3, 0)),
    "1x7_on_3x9": (1, 3, 9, 20, 12, (1, 7), 1, (0, 3)),
    "7x1_on_3x9": (1, 3, 9, 20, 12, (7, 1), 1, (3, 0)),
    "5x5_p2": (1, 6, 7, 48, 64, (5, 5), 1, (2, 2)),
    "1x3_on_1x1": (1, 1, 1, 12, 20, (1, 3), 1, (0, 1)),                  # tiny images: every neighbour is padding
    "3x1_on_1x1": (1, 1, 1, 12, 20, (3, 1), 1, (1, 0)),
    "3x3_on_1x1": (1, 1, 1, 12, 20, (3, 3), 1, (1, 1)),
    "1x3_on_2x2": (1, 2, 2, 12, 20, (1, 3), 1, (0, 1)),
    "3x1_on_2x2": (1, 2, 2, 12, 20, (3, 1), 1, (1, 0)),
    "3x3_on_2x2": (1, 2, 2, 12, 20, (3, 3), 1, (1, 1)),
    "s2_17_to_8": (1, 17, 17, 8, 16, (3, 3), 2, (0, 0)),
    "s2_8_to_3": (1, 8, 8, 8, 16, (3, 3), 2, (0, 0)),                    # the last row and column are never read
    "s2_6_to_2": (1, 6, 6, 8, 16, (3, 3), 2, (0, 0)),
    "1x1_straddle": (3, 35, 35, 288, 64, (1, 1), 1, (0, 0)),            # M = 3675: no tile multiple, tiles straddle images
    "1x1_long_k": (1, 8, 8, 2048, 320, (1, 1), 1, (0, 0)),
    "3x3_long_k": (1, 8, 8, 448, 384, (3, 3), 1, (1, 1)),
    "mixed6_7x1": (2, 17, 17, 160, 160, (7, 1), 1, (3, 0)),
}
_REF = {}


def case_data(name):
    """fp32 inputs (seeded) and the fp64 reference of one case, computed once: (x NCHW, w, b, conv64 without bias, |x| * |w|)"""
    if name not in _REF:
        B, H, W, Cin, N, (kh, kw), stride, pad = CASES[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(N, Cin, kh, kw, generator=g) / (Cin * kh * kw) ** 0.5
        b = torch.randn(N, generator=g)
        y = F.conv2d(x.double(), w.double(), None, stride, pad)
        a = F.conv2d(x.double().abs(), w.double().abs(), None, stride, pad)
        _REF[name] = (x, w, b, y, a)
    return _REF[name]


def run(lib, gpu, name, relu, bias, view, kpad_extra=0):
    """-> (out NCHW fp32 on the host, the whole output buffer, its untouched twin, (M, N, column offset))"""
    from freefine_amd import _lib
    B, H, W, Cin, N, (kh, kw), stride, pad = CASES[name]
    x, w, b, _, _ = case_data(name)
    Ho, Wo = (H + 2 * pad[0] - kh) // stride + 1, (W + 2 * pad[1] - kw) // stride + 1
    M, K = B * Ho * Wo, kh * kw * Cin
    xoff, ldx, ooff, ldo, extra = (4, Cin + 12, 8, N + 12, 5) if view else (0, Cin, 0, N, 0)
    xbuf = torch.full((B * H * W, ldx), float("nan"))
    xbuf[:, xoff:xoff + Cin] = x.permute(0, 2, 3, 1).reshape(-1, Cin)
    wbuf = torch.full((N, K + kpad_extra), float("nan"))
    wbuf[:, :K] = w.permute(0, 2, 3, 1).reshape(N, K)
    obuf = torch.full((M + extra, ldo), SENTINEL)
    xd, wd, bd, od = xbuf.to(gpu), wbuf.to(gpu), b.to(gpu), obuf.to(gpu)
    d = _lib.Conv2dDesc()
    d.x, d.w, d.bias, d.out = xd.data_ptr() + 4 * xoff, wd.data_ptr(), (bd.data_ptr() if bias else None), od.data_ptr() + 4 * ooff
    d.B, d.Hin, d.Win, d.Cin, d.N, d.KH, d.KW, d.stride, d.pad_h, d.pad_w = B, H, W, Cin, N, kh, kw, stride, pad[0], pad[1]
    d.ldx, d.ldo, d.Kpad, d.flags = ldx, ldo, K + kpad_extra, (_lib.CONV_RELU if relu else 0)
    rc = lib.ffn_conv2d(torch.cuda.current_stream().cuda_stream, _lib.FFN_F32, ctypes.byref(d))
    assert rc == 0, lib.ffn_last_error()
    torch.cuda.synchronize()
    full = od.cpu()
    out = full[:M, ooff:ooff + N].reshape(B, Ho, Wo, N).permute(0, 3, 1, 2)
    return out, full, obuf, (M, N, ooff)


def check(name, out, relu, bias):
    _, _, b, y, a = case_data(name)
    B, H, W, Cin, N, (kh, kw), stride, pad = CASES[name]
    gamma = (kh * kw * Cin + 2) * 2.0 ** -24
    want, bound = y, gamma * a
    if bias:
        want, bound = y + b.double().view(1, -1, 1, 1), gamma * (a + b.double().abs().view(1, -1, 1, 1))
    if relu:
        want = want.clamp_min(0)          # 1-Lipschitz: the bound carries over
    err = (out.double() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name} relu={relu} bias={bias}: max |err| {err.max().item():.3e}, max err / bound {worst:.3f}")
    assert torch.isfinite(out).all() and (err <= bound).all(), (name, relu, bias, err.max().item(), worst)


@pytest.mark.parametrize("name", list(CASES))
def test_conv2d_within_the_fma_chain_bound_in_column_views(gpu, name):
    from freefine_amd import _lib
    lib = _lib.load()
    for relu, bias in ((True, True), (False, False), (True, False), (False, True)):
        out, full, before, (M, N, off) = run(lib, gpu, name, relu, bias, view=True)
        check(name, out, relu, bias)
        keep = torch.ones_like(full, dtype=torch.bool)
        keep[:M, off:off + N] = False
        assert torch.equal(full[keep].view(torch.int32), before[keep].view(torch.int32)), f"{name}: bytes outside the output view changed"
    out, _, _, _ = run(lib, gpu, name, True, True, view=False)
    check(name, out, True, True)


@pytest.mark.parametrize("name", ["stem_3x3_s2", "1x1_straddle", "3x3_long_k", "mixed6_7x1"])
def test_conv2d_is_deterministic_and_ignores_the_weight_padding(gpu, name):
    from freefine_amd import _lib
    lib = _lib.load()
    a = run(lib, gpu, name, True, True, view=True)[0]
    b = run(lib, gpu, name, True, True, view=True)[0]
    c = run(lib, gpu, name, True, True, view=True, kpad_extra=8)[0]          # NaN columns K .. Kpad - 1: never read
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_conv2d_refusals_launch_nothing(gpu):
    """every refusal of the header: FFN_EINVAL (FFN_ENOSYS for another dtype) with a message, and the output buffer untouched"""
    from freefine_amd import _lib
    lib = _lib.load()
    x, w, b = torch.zeros(64, 16, device=gpu), torch.zeros(16, 9 * 8 + 8, device=gpu), torch.zeros(16, device=gpu)
    o = torch.full((64, 24), SENTINEL, device=gpu)

    def desc(**kw):
        d = _lib.Conv2dDesc()
        d.x, d.w, d.bias, d.out = x.data_ptr(), w.data_ptr(), b.data_ptr(), o.data_ptr()
        d.B, d.Hin, d.Win, d.Cin, d.N, d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.ldx, d.ldo, d.Kpad, d.flags = 1, 8, 8, 8, 16, 3, 3, 1, 1, 1, 16, 24, 72, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    s = torch.cuda.current_stream().cuda_stream
    assert lib.ffn_conv2d(s, _lib.FFN_F32, ctypes.byref(desc())) == 0
    torch.cuda.synchronize()
    assert (o[:, :16] == 0).all() and (o[:, 16:] == SENTINEL).all()
    o.fill_(SENTINEL)
    bad = [dict(Cin=6, Kpad=56), dict(N=18), dict(KH=2), dict(KW=9), dict(KH=0), dict(stride=3), dict(stride=0), dict(pad_h=-1), dict(pad_w=-1), dict(ldx=4), dict(ldo=12),
           dict(ldx=18), dict(ldo=26), dict(Kpad=68), dict(Kpad=74), dict(x=x.data_ptr() + 4), dict(w=w.data_ptr() + 8), dict(bias=b.data_ptr() + 4),
           dict(out=o.data_ptr() + 4), dict(x=None), dict(w=None), dict(out=None), dict(B=0), dict(Hin=0), dict(flags=2), dict(KH=7, pad_h=0, Hin=4), dict(Cin=0, Kpad=0)]
    for kw in bad:
        assert lib.ffn_conv2d(s, _lib.FFN_F32, ctypes.byref(desc(**kw))) == -22, kw
        assert lib.ffn_last_error().startswith(b"conv2d: "), (kw, lib.ffn_last_error())
    assert lib.ffn_conv2d(s, _lib.FFN_F32, None) == -22
    for dtype in (_lib.FFN_BF16, _lib.FFN_BF16X3, _lib.FFN_FP8, 9):
        assert lib.ffn_conv2d(s, dtype, ctypes.byref(desc())) == -38 and b"conv2d" in lib.ffn_last_error()
    torch.cuda.synchronize()
    assert (o == SENTINEL).all()
