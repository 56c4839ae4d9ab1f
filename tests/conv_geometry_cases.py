"""The cases, the operands and the fp64 reference of tests/test_conv_geometry_gpu.py; tests/test_conv_geometry_ref_cpu.py checks all of it without a device.

Geometry classes (the smallest shapes that still reach the kernels; B is chosen so that M = B * Hout * Wout passes a 256-row tile with a ragged tail):
  A  odd / non-square, stride 1, pad 1: 13x11 (143 rows per image: tiles span two and three images, seams anywhere) and 12x12 (144);
  B  stride 2: 13x11 -> 7x6, 37x37 -> 19x19 (the depth network's), and pad = 0 with Hout, Wout given (the VAE encoder's right / bottom-only padding) 13x11, 12x10 -> 6x5;
  C  fused nearest-2x upsample: 7x5 -> 14x10, 9x11 -> 18x22;
  D  degenerate images, every pixel a border pixel, a tile spans dozens of images: 1x37, 37x1, 2x2, 3x3, 1x1;
  E  halo tiles at W other than 16 / 32: W in {1, 2, 4, 8, 64, 128, 256, 512}, H * W a multiple of (or equal to) the tile height;
  F  conv3x3_up2x (conv = 2, the four sub-pixel classes) at odd low-resolution sizes 9x11, 13x15;
  G  conv3x3_n4: 1x1, 1x9, 9x1, 3x3.
Operands of the exact pass are small integers: x, w in {-1, 0, 1} (half / a quarter non-zero), bias, row bias and residual in {-4 .. 4}.  Every product and
every partial sum, in any order, under any K split and any hi / lo split (lo = 0), is an integer far below 2^24; e4m3 holds +-16 = x * F8_ACT_SCALE and the
power-of-two scaled weights exactly; |ref| <= 256 makes the bf16 output exact.  So a correct kernel is torch.equal to the fp64 reference in every mode."""
import collections

import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "cls B H W stride pad up Cin Cout modes variants splitk")

VARIANTS = {"plain": (False, False, False), "rb+res": (True, True, False), "rb+res+relu": (True, True, True)}          # name -> (row bias, residual, relu)

# (Cin, Cout, modes).  Cin: 64 = one chunk per tap (streaming loader, halo, ping-pong); 128 = the tap changes every second K tile; 8 and 24 = a K stage of the
# recomputing loader spans several taps; 32 and 96 = split-bf16 blocks (96: 27 stages, an odd count); 40 (and 24) = split-bf16 planes.
# Cout: 320 / 256 / 128 = the tile widths of ping-pong and halo (128: the split-bf16 256x128 tile); 72 = ragged N
CH_FULL = [(64, 320, ("bf16", "x3", "f8")), (128, 256, ("bf16", "x3", "f8")), (64, 128, ("bf16", "x3")), (8, 72, ("f32", "bf16", "x3")), (24, 72, ("f32", "bf16", "x3")),
           (32, 72, ("x3",)), (96, 72, ("x3",)), (40, 72, ("x3",))]
CH_CORE = [(64, 320, ("bf16", "x3", "f8")), (128, 256, ("bf16",)), (24, 72, ("f32", "bf16")), (96, 72, ("x3",)), (40, 72, ("x3",))]
CH_HALO = [(64, 320, ("bf16",)), (128, 256, ("bf16",))]
CH_SPLIT = (128, 320, ("bf16", "x3", "f8"))          # K tiles of the ping-pong kernel: 18 (bf16), 36 (split-bf16), 9 (fp8): three slices of whole tiles, >= 2 each
SPLITK = 3

# class -> ([(B, H, W, stride, pad, upsample)], variants, channel sets of the first geometry, of the others)
GEOMETRIES = {
    "A": ([(5, 13, 11, 1, 1, False), (5, 12, 12, 1, 1, False)], ("plain", "rb+res", "rb+res+relu"), CH_FULL, CH_CORE),
    "B": ([(7, 13, 11, 2, 1, False), (1, 37, 37, 2, 1, False), (10, 13, 11, 2, 0, False), (9, 12, 10, 2, 0, False)], ("plain", "rb+res"), CH_FULL, CH_CORE),
    "C": ([(3, 7, 5, 1, 1, True), (2, 9, 11, 1, 1, True)], ("plain", "rb+res"), CH_FULL, CH_CORE),
    "D": ([(8, 1, 37, 1, 1, False), (8, 37, 1, 1, 1, False), (75, 2, 2, 1, 1, False), (33, 3, 3, 1, 1, False), (300, 1, 1, 1, 1, False)], ("plain", "rb+res"), CH_FULL, CH_CORE),
    "E": ([(2, 32, 8, 1, 1, False), (3, 128, 1, 1, 1, False), (3, 64, 2, 1, 1, False), (2, 64, 4, 1, 1, False), (2, 4, 64, 1, 1, False), (1, 8, 64, 1, 1, False),
           (2, 2, 64, 1, 1, False), (2, 2, 128, 1, 1, False), (2, 1, 256, 1, 1, False), (1, 1, 512, 1, 1, False)], ("plain", "rb+res"), CH_FULL, CH_HALO),
}
SPLIT_CLASSES = "AB"


def _cases():
    out = []
    for cls, (geos, variants, first, rest) in GEOMETRIES.items():
        for i, g in enumerate(geos):
            for cin, cout, modes in (first if i == 0 else rest):
                out.append(Case(cls, *g, cin, cout, modes, variants, 1))
            if cls in SPLIT_CLASSES:
                out.append(Case(cls, *g, *CH_SPLIT, ("rb+res",) if i else ("rb+res", "rb+res+relu"), SPLITK))
    return out


CASES = _cases()
# class F: (B, H, W, Cin, Cout).  198 and 195 low-resolution pixels reach the 192-row tiles only, 390 the 256-row ones (and leave a ragged tail on both)
UP2X_CASES = [(2, 9, 11, 64, 256), (2, 9, 11, 128, 320), (1, 13, 15, 128, 256), (2, 13, 15, 64, 320), (2, 13, 15, 128, 256)]
N4_CASES = [(300, 1, 1, 16), (30, 1, 9, 32), (30, 9, 1, 48), (3, 3, 3, 64), (29, 3, 3, 16)]                    # class G: (B, H, W, Cin); 64 pixels per workgroup


def case_id(c):
    return f"{c.cls}-{c.B}x{c.H}x{c.W}-s{c.stride}p{c.pad}{'-up' if c.up else ''}-{c.Cin}-{c.Cout}" + (f"-splitk{c.splitk}" if c.splitk > 1 else "")


def out_size(H, W, stride, pad, up):
    """Hout, Wout.  pad >= 1: ops.conv3x3's own formula, (He + 2 pad - 3) // stride + 1 on the (upsampled) input.  pad = 0 is never called that way: it is
    the VAE encoder's F.pad(x, (0, 1, 0, 1)) -> conv(stride 2, padding 0), i.e. the same formula on the image with one more row and column, handed to
    ops.conv3x3 as Hout, Wout (vae.py passes H // 2, W // 2 on even sizes: the same numbers); the kernel's bounds check supplies the zero row and column."""
    He, We = (2 * H, 2 * W) if up else (H, W)
    if pad == 0:
        return (He + 1 - 3) // stride + 1, (We + 1 - 3) // stride + 1
    return (He + 2 * pad - 3) // stride + 1, (We + 2 * pad - 3) // stride + 1


def rows(c):
    ho, wo = out_size(c.H, c.W, c.stride, c.pad, c.up)
    return ho * wo


def seed_of(*key):
    s = 12345
    for k in key:
        s = (s * 1000003 + int(k) * 7919 + 11) % (2 ** 31 - 1)
    return s


def _ternary(shape, g, zeros_of_8):
    """{-1, 0, 1}: `zeros_of_8` of 8 equally likely draws are 0, the others split evenly between -1 and 1"""
    r = torch.randint(0, 8, shape, generator=g)
    nz = 8 - zeros_of_8
    return torch.where(r < zeros_of_8, 0, torch.where(r < zeros_of_8 + nz // 2, 1, -1)).float()


def integer_operands(B, H, W, Cin, Cout, out_rows, seed):
    """-> dict of fp32 CPU tensors holding integers: x [B, H*W, Cin], w [Cout, Cin, 3, 3], bias [Cout], rb [B, Cout], res [B, out_rows, Cout]"""
    g = torch.Generator().manual_seed(seed)
    small = lambda *shape: torch.randint(-4, 5, shape, generator=g).float()
    return dict(x=_ternary((B, H * W, Cin), g, 4), w=_ternary((Cout, Cin, 3, 3), g, 6), bias=small(Cout), rb=small(B, Cout), res=small(B, out_rows, Cout))


def case_operands(c):
    return integer_operands(c.B, c.H, c.W, c.Cin, c.Cout, rows(c), seed_of(ord(c.cls), c.B, c.H, c.W, c.stride, c.pad, c.up, c.Cin, c.Cout, c.splitk))


def epilogue(y, o, variant):
    """the plain epilogue of ffn_igemm (include/freefine_hip.h): act(acc + bias + row bias) + residual; y [B, rows, Cout] fp64 = acc + bias"""
    rb, res, relu = VARIANTS[variant]
    if rb:
        y = y + o["rb"].double()[:, None]
    if relu:
        y = y.clamp_min(0.0)
    if res:
        y = y + o["res"].double()
    return y


def conv_ref(x, w, bias, B, H, W, stride, pad, up):
    """statement 1: F.conv2d in fp64 behind F.interpolate(nearest) for upsample and F.pad(0, 1, 0, 1) for pad = 0 -> [B, Hout*Wout, Cout]"""
    xin = x.double().reshape(B, H, W, -1).permute(0, 3, 1, 2)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if pad == 0:
        xin = F.pad(xin, (0, 1, 0, 1))
    y = F.conv2d(xin, w.double(), None if bias is None else bias.double(), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).reshape(B, -1, w.shape[0])


def gather_ref(x, w, bias, B, H, W, stride, pad, up, Hout, Wout):
    """statement 2, from the ABI's definition of conv = 1 (include/freefine_hip.h): output pixel (yo, xo) sums over the taps (ky, kx) whose position
    yy = yo * stride - pad + ky, xx = xo * stride - pad + kx lies inside [0, Hin << upsample) x [0, Win << upsample) the input pixel (yy >> upsample,
    xx >> upsample) times w[:, :, ky, kx]"""
    u = 1 if up else 0
    xi, wd = x.double().reshape(B, H, W, -1), w.double()
    y = torch.zeros(B, Hout, Wout, w.shape[0], dtype=torch.float64)
    for yo in range(Hout):
        for xo in range(Wout):
            for ky in range(3):
                for kx in range(3):
                    yy, xx = yo * stride - pad + ky, xo * stride - pad + kx
                    if 0 <= yy < (H << u) and 0 <= xx < (W << u):
                        y[:, yo, xo] += xi[:, yy >> u, xx >> u] @ wd[:, :, ky, kx].t()
    if bias is not None:
        y = y + bias.double()
    return y.reshape(B, Hout * Wout, -1)


def case_ref(c, o, variant, x=None, w=None):
    """fp64 reference of a case ([B, rows, Cout]); x / w: the values the kernel is really given where they are not o's (dequantised fp8, bf16-rounded)"""
    return epilogue(conv_ref(o["x"] if x is None else x, o["w"] if w is None else w, o["bias"], c.B, c.H, c.W, c.stride, c.pad, c.up), o, variant)


def border_class(m, M, Hout, Wout):
    """where output row m lies: (image, yo, xo, class)"""
    if m >= M:
        return (m // (Hout * Wout), None, None, "pixel behind M")
    img, rem = divmod(m, Hout * Wout)
    yo, xo = divmod(rem, Wout)
    ey, ex = yo in (0, Hout - 1), xo in (0, Wout - 1)
    kind = "corner" if ey and ex else ("edge" if ey or ex else "interior")
    if yo == 0:
        kind += ", first row of an image"
    if yo == Hout - 1:
        kind += ", last row of an image"
    return (img, yo, xo, kind)


# ---------------------------------------------------------------------------------------------------------------------
# which kernel a forced configuration must run: csrc/capi_igemm.hip restated (pp_ok, halo_bytes_for, the tile list kCfg,
# candidates_for's extra conditions on halo and split-K candidates) for the descriptors ops.conv3x3 builds from these cases
# ---------------------------------------------------------------------------------------------------------------------
HALO_CFGS = {9: (128, 320), 10: (256, 128), 11: (256, 256), 12: (128, 128)}
PP_CFGS = {13: (256, 320), 14: (256, 256), 15: (192, 320), 16: (192, 256), 17: (256, 128)}


def halo_eligible(c, mode, variant, bm, bn):
    """halo_bytes_for(d, bm) > 0 and candidates_for keeps the configuration: bf16, 3x3 / stride 1 / pad 1 / no upsample, whole 64-channel chunks, M a whole
    number of tiles, a tile = whole image rows (W <= bm, bm % W == 0, H * W % bm == 0) or a piece of one row (W % bm == 0), its (rows + 2) x (width + 2)
    halo pixels within 4 x 16 wave instructions of 8 slots, two halo buffers + the weight ring within 160 KiB of LDS, no forced K split, and not a tile
    twice as wide as N"""
    if mode != "bf16" or c.stride != 1 or c.up or c.pad != 1 or c.Cin % 64 or (c.B * c.H * c.W) % bm or c.splitk > 1:
        return False
    if c.W <= bm:
        if bm % c.W or (c.H * c.W) % bm:
            return False
        tw, tr = c.W, bm // c.W
    else:
        if c.W % bm:
            return False
        tw, tr = bm, 1
    nq = ((tr + 2) * (tw + 2) + 7) // 8
    return nq <= 64 and 2 * nq * 1024 + 2 * bn * 128 <= 160 * 1024 and not bn >= 2 * c.Cout


def pp_k_tiles(c, mode):
    """K tiles of the ping-pong kernel: 64 bf16 elements; split-bf16: 32 real elements; fp8: 128 e4m3 values of the channels padded to a multiple of 128"""
    if mode == "x3":
        return 9 * c.Cin // 32
    return 9 * ((c.Cin + 127) // 128 * 128 // 128) if mode == "f8" else 9 * c.Cin // 64


def pp_eligible(c, mode, variant, bm, bn):
    """pp_ok(d, bm, bn, splitk) for the case's own splitk (1, or SPLITK: then also what candidates_for asks of a split candidate)"""
    rb, res, relu = VARIANTS[variant]
    M, N, x3, f8 = c.B * rows(c), c.Cout, mode == "x3", mode == "f8"
    if mode == "f32":
        return False
    if bn == 128 and (bm != 256 or not x3 or c.splitk > 1 or N % 256 == 0 or N % 320 == 0):
        return False
    if not f8 and c.Cin % (32 if x3 else 64):
        return False
    nkt = pp_k_tiles(c, mode)
    if nkt < 2 or N % bn or M < bm:
        return False
    if c.splitk > 1:
        tiles = (M + bm - 1) // bm * (N // bn)
        return nkt % c.splitk == 0 and nkt // c.splitk >= 2 and tiles < 160 and c.splitk <= (384 + tiles - 1) // tiles
    if relu and (res or x3 or f8):          # the activation is applied by the plain bf16 epilogue, whose accumulators start at the bias -- not beside a residual
        return False
    return not (rb and rows(c) < 128)          # a wave's rows may straddle two images, not three
