"""The yardstick of the FID feature extractor (freefine_amd/inception.py): pytorch-fid's InceptionV3([3]) -- torchvision's Inception-v3 with the four
patched FID blocks, resize_input and normalize_input on, the 2048-d pool3 features -- restated with torch's own functions (F.conv2d, F.batch_norm,
F.max_pool2d, F.avg_pool2d, F.interpolate) on the CPU, in whatever dtype the state dict and the input have: fp64 is the reference, fp32 the
single-precision yardstick the GPU tests take their margin from.  BatchNorm is NOT folded here.

A block reads its widths from its weights, so the same functions run the full network, the `tiny` configuration (every width divided by 8 and rounded up to a
multiple of 4) and torchvision's base widths (tests/golden/g20_fid_blocks.npz: tools/gen_golden.py run_g20 runs the reference's four patched classes on
states made by `seeded_state` below, which pins each block's pool and concatenation order to the reference's text).

State dicts are in pytorch-fid's layout: <layer>.conv.weight [Cout, Cin, KH, KW], <layer>.bn.{weight, bias, running_mean, running_var} [Cout]."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MARGIN = 4.0      # a GPU result may deviate from fp64 by this many times what torch's own fp32 does: only the order of the sums differs


def width(c, config):
    if config == "full":
        return c
    assert config == "tiny"
    return -(-(-(-c // 8)) // 4) * 4


# ---------------------------------------------------------------------------------------------------------------------------------------------
# layer tables: {layer: (Cout, Cin, KH, KW)}
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _add(S, name, cin, cout, k):
    kh, kw = k if isinstance(k, tuple) else (k, k)
    S[name] = (cout, cin, kh, kw)


def shapes_a(S, p, cin, c1, c5r, c5, c3r, c3, pf):
    _add(S, p + "branch1x1", cin, c1, 1)
    _add(S, p + "branch5x5_1", cin, c5r, 1)
    _add(S, p + "branch5x5_2", c5r, c5, 5)
    _add(S, p + "branch3x3dbl_1", cin, c3r, 1)
    _add(S, p + "branch3x3dbl_2", c3r, c3, 3)
    _add(S, p + "branch3x3dbl_3", c3, c3, 3)
    _add(S, p + "branch_pool", cin, pf, 1)
    return c1 + c5 + c3 + pf


def shapes_b(S, p, cin, c3, cr, cd):
    _add(S, p + "branch3x3", cin, c3, 3)
    _add(S, p + "branch3x3dbl_1", cin, cr, 1)
    _add(S, p + "branch3x3dbl_2", cr, cd, 3)
    _add(S, p + "branch3x3dbl_3", cd, cd, 3)
    return c3 + cd + cin


def shapes_c(S, p, cin, c7, co):
    _add(S, p + "branch1x1", cin, co, 1)
    _add(S, p + "branch7x7_1", cin, c7, 1)
    _add(S, p + "branch7x7_2", c7, c7, (1, 7))
    _add(S, p + "branch7x7_3", c7, co, (7, 1))
    _add(S, p + "branch7x7dbl_1", cin, c7, 1)
    _add(S, p + "branch7x7dbl_2", c7, c7, (7, 1))
    _add(S, p + "branch7x7dbl_3", c7, c7, (1, 7))
    _add(S, p + "branch7x7dbl_4", c7, c7, (7, 1))
    _add(S, p + "branch7x7dbl_5", c7, co, (1, 7))
    _add(S, p + "branch_pool", cin, co, 1)
    return 4 * co


def shapes_d(S, p, cin, cr, c3):
    _add(S, p + "branch3x3_1", cin, cr, 1)
    _add(S, p + "branch3x3_2", cr, c3, 3)
    _add(S, p + "branch7x7x3_1", cin, cr, 1)
    _add(S, p + "branch7x7x3_2", cr, cr, (1, 7))
    _add(S, p + "branch7x7x3_3", cr, cr, (7, 1))
    _add(S, p + "branch7x7x3_4", cr, cr, 3)
    return c3 + cr + cin


def shapes_e(S, p, cin, c1, c3, cd, cp):
    _add(S, p + "branch1x1", cin, c1, 1)
    _add(S, p + "branch3x3_1", cin, c3, 1)
    _add(S, p + "branch3x3_2a", c3, c3, (1, 3))
    _add(S, p + "branch3x3_2b", c3, c3, (3, 1))
    _add(S, p + "branch3x3dbl_1", cin, cd, 1)
    _add(S, p + "branch3x3dbl_2", cd, c3, 3)
    _add(S, p + "branch3x3dbl_3a", c3, c3, (1, 3))
    _add(S, p + "branch3x3dbl_3b", c3, c3, (3, 1))
    _add(S, p + "branch_pool", cin, cp, 1)
    return c1 + 4 * c3 + cp


def block_shapes(kind, cin, arg=None):
    """one block at torchvision's base widths, names without a prefix: what FIDInceptionA(cin, arg), FIDInceptionC(cin, arg), FIDInceptionE_1/2(cin) hold"""
    S = {}
    if kind == "A":
        shapes_a(S, "", cin, 64, 48, 64, 64, 96, arg)
    elif kind == "C":
        shapes_c(S, "", cin, arg, 192)
    else:
        assert kind in ("E1", "E2")
        shapes_e(S, "", cin, 320, 384, 448, 192)
    return S


def network_shapes(config):
    w = lambda c: width(c, config)
    S = {}
    _add(S, "Conv2d_1a_3x3", 3, w(32), 3)
    _add(S, "Conv2d_2a_3x3", w(32), w(32), 3)
    _add(S, "Conv2d_2b_3x3", w(32), w(64), 3)
    _add(S, "Conv2d_3b_1x1", w(64), w(80), 1)
    _add(S, "Conv2d_4a_3x3", w(80), w(192), 3)
    c = w(192)
    for name, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
        c = shapes_a(S, name + ".", c, w(64), w(48), w(64), w(64), w(96), w(pf))
    c = shapes_b(S, "Mixed_6a.", c, w(384), w(64), w(96))
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        c = shapes_c(S, name + ".", c, w(c7), w(192))
    c = shapes_d(S, "Mixed_7a.", c, w(192), w(320))
    for name in ("Mixed_7b", "Mixed_7c"):
        c = shapes_e(S, name + ".", c, w(320), w(384), w(448), w(192))
    return S


def seeded_state(shapes, seed, dtype=torch.float64):
    """He-scaled convolutions (std sqrt(2 / fan_in): a ReLU layer keeps the second moment of its input), BatchNorm with gamma in [0.9, 1.1], beta and
    running_mean in [-0.1, 0.1], running_var in [0.5, 1.5]: activations stay O(1) through the 94 layers.  Drawn in fp64 from one seeded generator in the
    table's order, then cast."""
    g = torch.Generator().manual_seed(seed)
    st = {}
    for name, (cout, cin, kh, kw) in shapes.items():
        st[name + ".conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g, dtype=torch.float64) * (2.0 / (cin * kh * kw)) ** 0.5
        u = torch.rand(4, cout, generator=g, dtype=torch.float64)
        st[name + ".bn.weight"] = 0.9 + 0.2 * u[0]
        st[name + ".bn.bias"] = -0.1 + 0.2 * u[1]
        st[name + ".bn.running_mean"] = -0.1 + 0.2 * u[2]
        st[name + ".bn.running_var"] = 0.5 + u[3]
    return {k: v.to(dtype) for k, v in st.items()}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------------------------------------
def basic_conv(st, name, x, stride=1, padding=0):
    """BasicConv2d: convolution without bias, BatchNorm (eval, eps 1e-3), ReLU"""
    y = F.conv2d(x, st[name + ".conv.weight"], None, stride, padding)
    y = F.batch_norm(y, st[name + ".bn.running_mean"], st[name + ".bn.running_var"], st[name + ".bn.weight"], st[name + ".bn.bias"], False, 0.0, BN_EPS)
    return F.relu(y)


def _avg(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


def _max(x):
    return F.max_pool2d(x, kernel_size=3, stride=1, padding=1)


def block_a(st, p, x):
    b1 = basic_conv(st, p + "branch1x1", x)
    b5 = basic_conv(st, p + "branch5x5_2", basic_conv(st, p + "branch5x5_1", x), padding=2)
    b3 = basic_conv(st, p + "branch3x3dbl_1", x)
    b3 = basic_conv(st, p + "branch3x3dbl_3", basic_conv(st, p + "branch3x3dbl_2", b3, padding=1), padding=1)
    bp = basic_conv(st, p + "branch_pool", _avg(x))
    return torch.cat([b1, b5, b3, bp], 1)


def block_b(st, p, x):
    b3 = basic_conv(st, p + "branch3x3", x, stride=2)
    bd = basic_conv(st, p + "branch3x3dbl_2", basic_conv(st, p + "branch3x3dbl_1", x), padding=1)
    bd = basic_conv(st, p + "branch3x3dbl_3", bd, stride=2)
    return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def block_c(st, p, x):
    b1 = basic_conv(st, p + "branch1x1", x)
    b7 = basic_conv(st, p + "branch7x7_1", x)
    b7 = basic_conv(st, p + "branch7x7_2", b7, padding=(0, 3))
    b7 = basic_conv(st, p + "branch7x7_3", b7, padding=(3, 0))
    bd = basic_conv(st, p + "branch7x7dbl_1", x)
    bd = basic_conv(st, p + "branch7x7dbl_2", bd, padding=(3, 0))
    bd = basic_conv(st, p + "branch7x7dbl_3", bd, padding=(0, 3))
    bd = basic_conv(st, p + "branch7x7dbl_4", bd, padding=(3, 0))
    bd = basic_conv(st, p + "branch7x7dbl_5", bd, padding=(0, 3))
    bp = basic_conv(st, p + "branch_pool", _avg(x))
    return torch.cat([b1, b7, bd, bp], 1)


def block_d(st, p, x):
    b3 = basic_conv(st, p + "branch3x3_2", basic_conv(st, p + "branch3x3_1", x), stride=2)
    b7 = basic_conv(st, p + "branch7x7x3_1", x)
    b7 = basic_conv(st, p + "branch7x7x3_2", b7, padding=(0, 3))
    b7 = basic_conv(st, p + "branch7x7x3_3", b7, padding=(3, 0))
    b7 = basic_conv(st, p + "branch7x7x3_4", b7, stride=2)
    return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def block_e(st, p, x, pool):
    b1 = basic_conv(st, p + "branch1x1", x)
    b3 = basic_conv(st, p + "branch3x3_1", x)
    b3 = torch.cat([basic_conv(st, p + "branch3x3_2a", b3, padding=(0, 1)), basic_conv(st, p + "branch3x3_2b", b3, padding=(1, 0))], 1)
    bd = basic_conv(st, p + "branch3x3dbl_2", basic_conv(st, p + "branch3x3dbl_1", x), padding=1)
    bd = torch.cat([basic_conv(st, p + "branch3x3dbl_3a", bd, padding=(0, 1)), basic_conv(st, p + "branch3x3dbl_3b", bd, padding=(1, 0))], 1)
    bp = basic_conv(st, p + "branch_pool", pool(x))
    return torch.cat([b1, b3, bd, bp], 1)


def fid_block(kind, st, x):
    """the four patched blocks by the name tools/gen_golden.py run_g20 gives them: average pooling over the in-image taps in A, C and E1, MAX pooling in E2"""
    if kind == "A":
        return block_a(st, "", x)
    if kind == "C":
        return block_c(st, "", x)
    return block_e(st, "", x, _avg if kind == "E1" else _max)


def prepare(images_u8, dtype):
    """uint8 [B, H, W, 3] -> [B, 3, H, W]: ToTensor and Normalize(imagenet) (fid_score.py:124, after its Resize)"""
    x = torch.as_tensor(images_u8).permute(0, 3, 1, 2).to(dtype) / 255
    mean, std = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (IMAGENET_MEAN, IMAGENET_STD))
    return (x - mean) / std


def resize_input(x, side):
    """inception.py:151-158: bilinear to side x side (299 in the full network), then 2 x - 1"""
    return 2 * F.interpolate(x, size=(side, side), mode="bilinear", align_corners=False) - 1


def forward(st, x, side=299):
    """x [B, 3, H, W] (as `prepare` gives it) -> the outputs of pytorch-fid's four blocks, NCHW: after the first max pool (64 channels in the full network), after
    the second (192), after Mixed_6e (768), and the pooled features [B, 2048, 1, 1]"""
    x = resize_input(x, side)
    x = basic_conv(st, "Conv2d_1a_3x3", x, stride=2)
    x = basic_conv(st, "Conv2d_2a_3x3", x)
    x = basic_conv(st, "Conv2d_2b_3x3", x, padding=1)
    b0 = x = F.max_pool2d(x, kernel_size=3, stride=2)
    x = basic_conv(st, "Conv2d_3b_1x1", x)
    x = basic_conv(st, "Conv2d_4a_3x3", x)
    b1 = x = F.max_pool2d(x, kernel_size=3, stride=2)
    for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = block_a(st, name + ".", x)
    x = block_b(st, "Mixed_6a.", x)
    for name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = block_c(st, name + ".", x)
    b2 = x
    x = block_d(st, "Mixed_7a.", x)
    x = block_e(st, "Mixed_7b.", x, _avg)
    x = block_e(st, "Mixed_7c.", x, _max)
    return [b0, b1, b2, F.adaptive_avg_pool2d(x, 1)]


def features(st, images_u8, side=299, dtype=torch.float64):
    """uint8 [B, 224, 224, 3] (already resized) -> [B, C] pool3 features in `dtype`"""
    st = {k: v.to(dtype) for k, v in st.items()}
    return forward(st, prepare(images_u8, dtype), side)[3].flatten(1)


def pil_resize(image_u8, side=224):
    """torchvision's Resize((side, side)) of a PIL image: PIL's bilinear (antialiased) resize"""
    import numpy as np
    from PIL import Image
    return np.asarray(Image.fromarray(image_u8).resize((side, side), Image.BILINEAR))
