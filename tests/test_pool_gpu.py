"""GPU: ffn_pool2d, ffn_mean_hw and ffn_fid_prep (csrc/convkk.h) through the C ABI.

Max pooling only selects: it is bit-equal to torch's fp32 result on the CPU.  The in-image average sums at most k^2 values and divides once: within
(k^2 + 1) 2^-24 times the window mean of |x| of fp64.  The global mean likewise within (HW + 1) 2^-24 mean |x|.  The image preparation is held to its fp64
restatement with four times the deviation of torch's own fp32 result from it (only the order of the blend may differ), measured in the same test.
Inputs and outputs are column views of wider buffers: NaN outside the input view, a sentinel outside the output view that must come back bit for bit."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
# (H, W, k, stride, pad): 3 / 1 / 1 where every neighbour of a 1 x 1 image is padding, up to the 35 x 35 of Mixed_5; 3 / 2 / 0 where the last row and column are (7) and are not (8) read
GEOMS = [(1, 1, 3, 1, 1), (2, 2, 3, 1, 1), (3, 5, 3, 1, 1), (35, 35, 3, 1, 1), (7, 7, 3, 2, 0), (8, 8, 3, 2, 0), (35, 35, 3, 2, 0), (3, 5, 3, 2, 0)]


def pooled(lib, gpu, op, x, k, stride, pad):
    """x NCHW fp32 (host) -> (y NCHW, bytes outside the output view unchanged)"""
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ldx, xoff, ldy, yoff, extra = C + 8, 4, C + 12, 8, 3
    xb = torch.full((B * H * W, ldx), float("nan"))
    xb[:, xoff:xoff + C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    yb = torch.full((B * Ho * Wo + extra, ldy), SENTINEL)
    xd, yd = xb.to(gpu), yb.to(gpu)
    rc = lib.ffn_pool2d(torch.cuda.current_stream().cuda_stream, op, xd.data_ptr() + 4 * xoff, yd.data_ptr() + 4 * yoff, B, H, W, C, ldx, ldy, k, stride, pad)
    assert rc == 0, lib.ffn_last_error()
    torch.cuda.synchronize()
    full = yd.cpu()
    keep = torch.ones_like(full, dtype=torch.bool)
    keep[:B * Ho * Wo, yoff:yoff + C] = False
    return full[:B * Ho * Wo, yoff:yoff + C].reshape(B, Ho, Wo, C).permute(0, 3, 1, 2), torch.equal(full[keep].view(torch.int32), yb[keep].view(torch.int32))


@pytest.mark.parametrize("C", [20, 288])
def test_pool2d_max_is_bit_equal_and_the_valid_average_within_its_bound(gpu, C):
    from freefine_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(C)
    for H, W, k, stride, pad in GEOMS:
        x = torch.randn(3, C, H, W, generator=g)
        y, clean = pooled(lib, gpu, _lib.POOL_MAX, x, k, stride, pad)
        assert clean and torch.equal(y.view(torch.int32), F.max_pool2d(x, k, stride, pad).contiguous().view(torch.int32)), (H, W, stride)
        y, clean = pooled(lib, gpu, _lib.POOL_AVG_VALID, x, k, stride, pad)
        want = F.avg_pool2d(x.double(), k, stride, pad, count_include_pad=False)
        bound = (k * k + 1) * 2.0 ** -24 * F.avg_pool2d(x.double().abs(), k, stride, pad, count_include_pad=False)
        err = (y.double() - want).abs()
        print(f"avg_valid C={C} {H}x{W} s{stride} p{pad}: max err / bound {(err / bound).max().item():.3f}")
        assert clean and (err <= bound).all(), (H, W, stride, err.max().item())


def test_pool2d_refusals(gpu):
    from freefine_amd import _lib
    lib = _lib.load()
    x, y = torch.zeros(64, 8, device=gpu), torch.full((64, 8), SENTINEL, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(op=0, B=1, H=8, W=8, C=8, ldx=8, ldy=8, k=3, stride=1, pad=1)

    def call(xp=None, yp=None, **kw):
        a = dict(ok, **kw)
        return lib.ffn_pool2d(s, a["op"], x.data_ptr() if xp is None else xp, y.data_ptr() if yp is None else yp, a["B"], a["H"], a["W"], a["C"], a["ldx"], a["ldy"], a["k"],
                              a["stride"], a["pad"])
    for kw in (dict(op=2), dict(C=6), dict(C=0), dict(ldx=4), dict(ldy=4), dict(ldx=10), dict(k=0), dict(k=9), dict(stride=0), dict(stride=4), dict(pad=2), dict(pad=-1),
               dict(B=0), dict(H=2, W=2, pad=0), dict(xp=x.data_ptr() + 4), dict(yp=y.data_ptr() + 8), dict(xp=0)):
        assert call(**kw) == -22 and lib.ffn_last_error().startswith(b"pool2d: "), (kw, lib.ffn_last_error())
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    assert lib.ffn_mean_hw(s, x.data_ptr(), y.data_ptr(), 1, 8, 6, 8) == -22 and lib.ffn_last_error().startswith(b"mean_hw: ")
    assert lib.ffn_mean_hw(s, x.data_ptr(), y.data_ptr(), 1, 0, 8, 8) == -22 and lib.ffn_mean_hw(s, x.data_ptr(), y.data_ptr(), 1, 8, 8, 4) == -22
    assert lib.ffn_fid_prep(s, None, x.data_ptr(), y.data_ptr(), 1, 8, 8) == -22 and lib.ffn_last_error().startswith(b"fid_prep: ")
    assert lib.ffn_fid_prep(s, x.data_ptr(), x.data_ptr(), y.data_ptr(), 1, 0, 8) == -22 and lib.ffn_fid_prep(s, x.data_ptr(), x.data_ptr(), y.data_ptr(), 1, 8, 5000) == -22


@pytest.mark.parametrize("HW,C", [(1, 20), (4, 20), (15, 288), (64, 2048), (1225, 20)])
def test_mean_hw_within_its_bound_and_deterministic(gpu, HW, C):
    from freefine_amd import _lib
    lib = _lib.load()
    B, ldx, off = 3, C + 8, 4
    x = torch.randn(B, HW, C, generator=torch.Generator().manual_seed(HW * C))
    xb = torch.full((B * HW, ldx), float("nan"))
    xb[:, off:off + C] = x.reshape(-1, C)
    xd = xb.to(gpu)
    outs = []
    for _ in range(2):
        yd = torch.full((B + 1, C), SENTINEL, device=gpu)
        assert lib.ffn_mean_hw(torch.cuda.current_stream().cuda_stream, xd.data_ptr() + 4 * off, yd.data_ptr(), B, HW, C, ldx) == 0, lib.ffn_last_error()
        torch.cuda.synchronize()
        outs.append(yd.cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) and (outs[0][B] == SENTINEL).all()
    err = (outs[0][:B].double() - x.double().mean(1)).abs()
    bound = (HW + 1) * 2.0 ** -24 * x.double().abs().mean(1)
    print(f"mean_hw HW={HW} C={C}: max err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("side", [299, 75])
def test_fid_prep_against_the_fp64_restatement(gpu, side):
    """lut -> bilinear (align_corners=False) -> 2 v - 1 from 224 x 224 bytes.  Gate: four times the deviation of torch's fp32 CPU result from the fp64 restatement."""
    from freefine_amd import _lib, ops
    import inception_ref as IR
    lib = _lib.load()
    img = torch.randint(0, 256, (2, 224, 224, 3), generator=torch.Generator().manual_seed(side), dtype=torch.uint8)
    lut = ops.vit_norm_table(IR.IMAGENET_MEAN, IR.IMAGENET_STD)
    v32 = torch.stack([lut[c][img[..., c].long()] for c in range(3)], 1)      # [B, 3, 224, 224]: the looked-up image
    t64, t32 = IR.resize_input(v32.double(), side), IR.resize_input(v32, side)
    out = torch.full((2, side, side, 4), SENTINEL, device=gpu)
    assert lib.ffn_fid_prep(torch.cuda.current_stream().cuda_stream, img.to(gpu).data_ptr(), lut.to(gpu).data_ptr(), out.data_ptr(), 2, 224, side) == 0, lib.ffn_last_error()
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[..., 3] == 0).all()
    got = got[..., :3].permute(0, 3, 1, 2)
    e_ref, err = (t32.double() - t64).abs().max().item(), (got.double() - t64).abs().max().item()
    same = (got == t32).float().mean().item()
    print(f"fid_prep 224 -> {side}: torch fp32 vs fp64 {e_ref:.3e}, device vs fp64 {err:.3e}, gate {IR.MARGIN * e_ref:.3e}; bit-equal to torch fp32 in {100 * same:.2f}% of the values")
    assert e_ref > 0 and err <= IR.MARGIN * e_ref
