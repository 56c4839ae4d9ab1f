"""The reference, the cases and the preconditions of tests/test_conv_geometry_gpu.py, checked without a device: the two fp64 statements of the convolution
(F.conv2d behind interpolate / pad, and the gather loop written from the ABI's definition) are equal on every case; Hout, Wout are ops.conv3x3's own
formula; the integer operands of every case and seed are integers, survive every encoding a mode applies to them (bf16, hi / lo split, e4m3 with its
power-of-two scales, the four-tap sums of the sub-pixel weights) unchanged, and give |ref| <= 256 under every epilogue, so that torch.equal is the right
assertion on the GPU; and the table reaches every kernel form in every class the eligibility rules admit it to."""
import inspect

import pytest
import torch

import conv_geometry_cases as G
from conv_geometry_cases import CASES, N4_CASES, UP2X_CASES, case_id

GEOS = sorted({(c.cls, c.B, c.H, c.W, c.stride, c.pad, c.up) for c in CASES})


def is_int(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_the_two_statements_of_the_reference_are_equal(c):
    o = G.case_operands(c)
    ho, wo = G.out_size(c.H, c.W, c.stride, c.pad, c.up)
    a = G.conv_ref(o["x"], o["w"], o["bias"], c.B, c.H, c.W, c.stride, c.pad, c.up)
    b = G.gather_ref(o["x"], o["w"], o["bias"], c.B, c.H, c.W, c.stride, c.pad, c.up, ho, wo)
    assert a.shape == b.shape == (c.B, ho * wo, c.Cout) and a.dtype == torch.float64
    assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,W,Cin,Cout", UP2X_CASES)
def test_the_two_statements_are_equal_on_the_subpixel_cases(B, H, W, Cin, Cout):
    o = G.integer_operands(B, H, W, Cin, Cout, 4 * H * W, G.seed_of(70, B, H, W, Cin, Cout))
    a = G.conv_ref(o["x"], o["w"], o["bias"], B, H, W, 1, 1, True)
    assert torch.equal(a, G.gather_ref(o["x"], o["w"], o["bias"], B, H, W, 1, 1, True, 2 * H, 2 * W))
    assert is_int(a) and a.abs().max() <= 256
    # the four-tap sums of the sub-pixel weights are integers of magnitude <= 4: exact in bf16, lo plane 0
    from freefine_amd import ops
    w4 = ops.pack_conv3x3_up2x(o["w"], torch.bfloat16)
    assert is_int(w4.float()) and w4.float().abs().max() <= 4
    x4 = ops.pack_conv3x3_up2x(o["w"], torch.float32, x3=True).float().reshape(4 * Cout, 4, Cin // 32, 2, 32)
    assert is_int(x4) and (x4[..., 1, :] == 0).all()


@pytest.mark.parametrize("B,H,W,Cin", N4_CASES)
def test_the_two_statements_are_equal_on_the_four_channel_cases(B, H, W, Cin):
    o = G.integer_operands(B, H, W, Cin, 4, H * W, G.seed_of(71, B, H, W, Cin))
    a = G.conv_ref(o["x"], o["w"], o["bias"], B, H, W, 1, 1, False)
    assert torch.equal(a, G.gather_ref(o["x"], o["w"], o["bias"], B, H, W, 1, 1, False, H, W))
    assert is_int(a) and a.abs().max() <= 256 and Cin % 16 == 0


def test_out_size_is_the_formula_of_ops_conv3x3():
    from freefine_amd import ops
    src = inspect.getsource(ops.conv3x3)
    assert "Hout = (He + 2 * pad - 3) // stride + 1" in src and "Wout = (We + 2 * pad - 3) // stride + 1" in src and "(Hin * 2, Win * 2) if upsample else (Hin, Win)" in src
    for cls, B, H, W, stride, pad, up in GEOS:
        He, We = (H * 2, W * 2) if up else (H, W)
        ho, wo = G.out_size(H, W, stride, pad, up)
        if pad:
            assert (ho, wo) == ((He + 2 * pad - 3) // stride + 1, (We + 2 * pad - 3) // stride + 1)
        else:          # right / bottom-only padding: the formula on the image with one more row and column; what vae.py passes on even sizes
            assert (ho, wo) == ((He + 1 + 2 * 0 - 3) // stride + 1, (We + 1 + 2 * 0 - 3) // stride + 1) and stride == 2
            if H % 2 == 0 and W % 2 == 0:
                assert (ho, wo) == (H // 2, W // 2)
        # and the shape F.conv2d itself gives
        assert G.conv_ref(torch.zeros(1, H * W, 1), torch.zeros(1, 1, 3, 3), None, 1, H, W, stride, pad, up).shape[1] == ho * wo
    assert G.out_size(13, 11, 2, 1, False) == (7, 6) and G.out_size(37, 37, 2, 1, False) == (19, 19) and G.out_size(7, 5, 1, 1, True) == (14, 10)
    assert G.out_size(13, 11, 2, 0, False) == G.out_size(12, 10, 2, 0, False) == (6, 5) and G.out_size(9, 11, 1, 1, True) == (18, 22)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_exactness_preconditions(c):
    """conditions, not measurements: if one fails, the densities or the seed of the case change, not the bound"""
    from freefine_amd import ops
    o = G.case_operands(c)
    for k, t in o.items():
        assert t.dtype == torch.float32 and is_int(t), k
    assert o["x"].abs().max() == 1 and o["w"].abs().max() == 1 and max(o[k].abs().max() for k in ("bias", "rb", "res")) <= 4
    assert 0.45 < (o["x"] != 0).float().mean() < 0.55 and 0.2 < (o["w"] != 0).float().mean() < 0.3
    for v in c.variants:
        ref = G.case_ref(c, o, v)
        assert is_int(ref) and ref.abs().max() <= 256, (v, ref.abs().max().item())
        assert torch.equal(ref.to(torch.bfloat16).double(), ref)
    # any partial sum, in any order: at most 9 Cin products of magnitude 1 (fp8: 16 x 256 = 2^12 each, before alpha = 2^-12) plus the epilogue's 12 -- below 2^24
    assert (9 * ((c.Cin + 127) // 128 * 128) + 12) * 4096 < 2 ** 24
    for k in ("x", "w", "res"):          # bf16 and the hi / lo split
        assert torch.equal(o[k].to(torch.bfloat16).float(), o[k])
        hi, lo = ops.split_hi_lo(o[k])
        assert torch.equal(hi.float(), o[k]) and (lo == 0).all()
    if "f8" in c.modes:
        wp = ops.pack_conv3x3_f8(o["w"])
        cp, alpha = wp._ffn_f8
        assert cp % 128 == 0 and alpha == 2.0 ** -12          # weights x 2^8 (max |w| = 1 lands at 256), activations x 2^4
        wdq = wp.view(torch.float8_e4m3fn).float().reshape(c.Cout, 3, 3, cp)[..., :c.Cin].permute(0, 3, 1, 2) * (alpha * ops.F8_ACT_SCALE)
        assert torch.equal(wdq, o["w"])
        x8 = (o["x"] * ops.F8_ACT_SCALE).to(torch.float8_e4m3fn)
        assert torch.equal(x8.float() / ops.F8_ACT_SCALE, o["x"])
    if c.splitk > 1:
        assert c.cls in G.SPLIT_CLASSES and all(G.pp_k_tiles(c, m) % c.splitk == 0 and G.pp_k_tiles(c, m) // c.splitk >= 2 for m in c.modes)


def test_border_classes():
    assert G.border_class(0, 100, 5, 4) == (0, 0, 0, "corner, first row of an image")
    assert G.border_class(2, 100, 5, 4) == (0, 0, 2, "edge, first row of an image")
    assert G.border_class(5, 100, 5, 4) == (0, 1, 1, "interior")
    assert G.border_class(4, 100, 5, 4) == (0, 1, 0, "edge")
    assert G.border_class(20 + 19, 100, 5, 4) == (1, 4, 3, "corner, last row of an image")
    assert G.border_class(3, 100, 1, 1) == (3, 0, 0, "corner, first row of an image, last row of an image")
    assert G.border_class(100, 100, 5, 4)[3] == "pixel behind M"


def _reach(pred, cls, mode, tiles, split):
    return {t for t in tiles for c in CASES for v in c.variants if c.cls == cls and mode in c.modes and (c.splitk > 1) == split and pred(c, mode, v, *t)}


def test_the_table_reaches_every_kernel_form_in_every_class():
    wide = {(256, 320), (256, 256), (192, 320), (192, 256)}
    for cls in G.GEOMETRIES:
        mine = [c for c in CASES if c.cls == cls]
        assert len({(c.B, c.H, c.W) for c in mine}) == len(G.GEOMETRIES[cls][0])
        assert all(c.B * G.rows(c) >= 256 for c in mine)
        # recomputing loader: fp32, bf16 with Cin % 64 != 0, split-bf16 planes and blocks; streaming loader: bf16 with whole 64-channel chunks
        assert any("f32" in c.modes for c in mine) and any("bf16" in c.modes and c.Cin % 64 for c in mine) and any("bf16" in c.modes and c.Cin % 64 == 0 for c in mine)
        assert any("x3" in c.modes and c.Cin % 32 for c in mine) and any("x3" in c.modes and c.Cin % 32 == 0 for c in mine)
        assert _reach(G.pp_eligible, cls, "bf16", G.PP_CFGS.values(), False) == wide
        assert _reach(G.pp_eligible, cls, "f8", G.PP_CFGS.values(), False) == wide
        assert _reach(G.pp_eligible, cls, "x3", G.PP_CFGS.values(), False) == wide | {(256, 128)}
        for mode in ("bf16", "x3", "f8"):
            assert bool(_reach(G.pp_eligible, cls, mode, G.PP_CFGS.values(), True)) == (cls in G.SPLIT_CLASSES)
        assert _reach(G.halo_eligible, cls, "bf16", G.HALO_CFGS.values(), False) == (set(G.HALO_CFGS.values()) if cls == "E" else set())
    # the refusals the GPU half must see: row bias on the ping-pong tiles below 128 rows per image; the halo of a 256-wide row piece (3 x 258 slots > 512)
    for c in CASES:
        if c.cls == "D":
            assert not any(G.pp_eligible(c, m, "rb+res", *t) for m in c.modes for t in G.PP_CFGS.values())
        if c.cls == "E" and c.W in (256, 512):
            assert not G.halo_eligible(c, "bf16", "plain", 256, 128) and not G.halo_eligible(c, "bf16", "plain", 256, 256) and G.halo_eligible(c, "bf16", "plain", 128, 128)
    e = [c for c in CASES if c.cls == "E"]
    assert {c.W for c in e} == {1, 2, 4, 8, 64, 128, 256, 512}
    assert any(c.H * c.W == 128 for c in e) and any(c.H * c.W == 256 and G.halo_eligible(c, "bf16", "plain", 256, 128) for c in e)
