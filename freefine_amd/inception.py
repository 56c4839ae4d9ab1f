"""The feature extractor of FID on the project's kernels: pytorch-fid's InceptionV3([3]) -- torchvision's Inception-v3 with the four patched FID blocks
(use_fid_inception), resize_input and normalize_input on, the 2048-d pool3 features (reference: evaluation/metrics/FID/fid.py, fid_score.py and
evaluation/DiffusionHandles/Lama/saicinpainting/evaluation/losses/fid/inception.py).

Every convolution is ffn_conv2d (csrc/convkk.h: an implicit GEMM on the exact-fp32 MFMA for any KH x KW in {1, 3, 5, 7}, stride 1 / 2, independent paddings),
every pool ffn_pool2d, the last AdaptiveAvgPool2d(1) ffn_mean_hw.  Activations are NHWC fp32; each branch of a Mixed block writes straight into its columns of
the block's concatenated output, so there is no concatenation pass.  BatchNorm (eval, eps 1e-3) is folded into weight and bias on the host in fp64 and
rounded to fp32 once; the ReLU is the convolution's epilogue.  The stem reads 4-channel pixels whose fourth channel is zero (ffn_fid_prep writes them).

torchvision is not installed anywhere this is built, and no published checkpoint is available offline: the network is written from its published topology and
held to the torch restatement tests/inception_ref.py (whose four FID blocks are pinned to the reference's classes by tests/golden/g20_fid_blocks.npz).  Parity
with the published pt_inception-2015-12-05 checkpoint and with torchvision's own classes is unmeasured.

`tiny`: the same topology, every width divided by 8 and rounded up to a multiple of 4, any input side from 75 on (the test sizes)."""
import torch

from . import ops

BN_EPS = 1e-3
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # fid_score.py:122-123
CONFIGS = ("full", "tiny")
MIN_SIDE = 75             # the smallest input side at which every stage keeps a pixel


def width(c, config):
    if config not in CONFIGS:
        raise ValueError(f"unknown Inception configuration {config!r} (one of {CONFIGS})")
    return c if config == "full" else -(-(-(-c // 8)) // 4) * 4


class Conv:
    """one BasicConv2d: name, channels, kernel (h, w), stride, padding (h, w)"""

    def __init__(self, name, cin, cout, k=1, stride=1, pad=0):
        self.name, self.cin, self.cout, self.stride = name, cin, cout, stride
        self.k = k if isinstance(k, tuple) else (k, k)
        self.pad = pad if isinstance(pad, tuple) else (pad, pad)


def layer_table(config):
    """-> (stem, blocks): stem = the five stem convolutions; blocks = [(kind, name, cin, cout, {branch: Conv})] for Mixed_5b .. Mixed_7c, kind one of
    "A", "B", "C", "D", "E1", "E2" (E1 pools with the in-image average, E2 with the maximum)."""
    w = lambda c: width(c, config)
    stem = [Conv("Conv2d_1a_3x3", 3, w(32), 3, stride=2), Conv("Conv2d_2a_3x3", w(32), w(32), 3), Conv("Conv2d_2b_3x3", w(32), w(64), 3, pad=1),
            Conv("Conv2d_3b_1x1", w(64), w(80), 1), Conv("Conv2d_4a_3x3", w(80), w(192), 3)]
    blocks = []

    def block(kind, name, cin, convs, passthrough=0):
        L = {c.name: c for c in convs}
        for c in convs:
            c.name = f"{name}.{c.name}"
        outs = {"A": ("branch1x1", "branch5x5_2", "branch3x3dbl_3", "branch_pool"), "B": ("branch3x3", "branch3x3dbl_3"),
                "C": ("branch1x1", "branch7x7_3", "branch7x7dbl_5", "branch_pool"), "D": ("branch3x3_2", "branch7x7x3_4"),
                "E": ("branch1x1", "branch3x3_2a", "branch3x3_2b", "branch3x3dbl_3a", "branch3x3dbl_3b", "branch_pool")}[kind[0]]
        cout = sum(L[o].cout for o in outs) + passthrough
        blocks.append((kind, name, cin, cout, L))
        return cout

    def A(name, cin, pf):
        return block("A", name, cin, [Conv("branch1x1", cin, w(64)), Conv("branch5x5_1", cin, w(48)), Conv("branch5x5_2", w(48), w(64), 5, pad=2),
                                      Conv("branch3x3dbl_1", cin, w(64)), Conv("branch3x3dbl_2", w(64), w(96), 3, pad=1),
                                      Conv("branch3x3dbl_3", w(96), w(96), 3, pad=1), Conv("branch_pool", cin, w(pf))])

    def C(name, cin, c7):
        c7 = w(c7)
        return block("C", name, cin, [Conv("branch1x1", cin, w(192)), Conv("branch7x7_1", cin, c7), Conv("branch7x7_2", c7, c7, (1, 7), pad=(0, 3)),
                                      Conv("branch7x7_3", c7, w(192), (7, 1), pad=(3, 0)), Conv("branch7x7dbl_1", cin, c7),
                                      Conv("branch7x7dbl_2", c7, c7, (7, 1), pad=(3, 0)), Conv("branch7x7dbl_3", c7, c7, (1, 7), pad=(0, 3)),
                                      Conv("branch7x7dbl_4", c7, c7, (7, 1), pad=(3, 0)), Conv("branch7x7dbl_5", c7, w(192), (1, 7), pad=(0, 3)),
                                      Conv("branch_pool", cin, w(192))])

    def E(kind, name, cin):
        return block(kind, name, cin, [Conv("branch1x1", cin, w(320)), Conv("branch3x3_1", cin, w(384)), Conv("branch3x3_2a", w(384), w(384), (1, 3), pad=(0, 1)),
                                       Conv("branch3x3_2b", w(384), w(384), (3, 1), pad=(1, 0)), Conv("branch3x3dbl_1", cin, w(448)),
                                       Conv("branch3x3dbl_2", w(448), w(384), 3, pad=1), Conv("branch3x3dbl_3a", w(384), w(384), (1, 3), pad=(0, 1)),
                                       Conv("branch3x3dbl_3b", w(384), w(384), (3, 1), pad=(1, 0)), Conv("branch_pool", cin, w(192))])

    c = w(192)
    c = A("Mixed_5b", c, 32)
    c = A("Mixed_5c", c, 64)
    c = A("Mixed_5d", c, 64)
    c = block("B", "Mixed_6a", c, [Conv("branch3x3", c, w(384), 3, stride=2), Conv("branch3x3dbl_1", c, w(64)), Conv("branch3x3dbl_2", w(64), w(96), 3, pad=1),
                                   Conv("branch3x3dbl_3", w(96), w(96), 3, stride=2)], passthrough=c)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        c = C(name, c, c7)
    c = block("D", "Mixed_7a", c, [Conv("branch3x3_1", c, w(192)), Conv("branch3x3_2", w(192), w(320), 3, stride=2), Conv("branch7x7x3_1", c, w(192)),
                                   Conv("branch7x7x3_2", w(192), w(192), (1, 7), pad=(0, 3)), Conv("branch7x7x3_3", w(192), w(192), (7, 1), pad=(3, 0)),
                                   Conv("branch7x7x3_4", w(192), w(192), 3, stride=2)], passthrough=c)
    c = E("E1", "Mixed_7b", c)
    c = E("E2", "Mixed_7c", c)
    return stem, blocks


def all_convs(config):
    stem, blocks = layer_table(config)
    return stem + [c for b in blocks for c in b[4].values()]


def fold_batchnorm64(state, conv):
    """-> (weight fp64 [Cout, Cin, KH, KW], bias fp64 [Cout]): conv -> BatchNorm(eval, eps 1e-3) as one affine map, in fp64.  A missing key raises KeyError, a
    wrong shape ValueError, both naming the key."""
    p = conv.name
    want = {f"{p}.conv.weight": (conv.cout, conv.cin) + conv.k}
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        want[f"{p}.bn.{leaf}"] = (conv.cout,)
    t = {}
    for key, shape in want.items():
        if key not in state:
            raise KeyError(key)
        if tuple(state[key].shape) != shape:
            raise ValueError(f"{key}: shape {tuple(state[key].shape)}, expected {shape}")
        t[key] = state[key].detach().to("cpu", torch.float64)
    scale = t[f"{p}.bn.weight"] / torch.sqrt(t[f"{p}.bn.running_var"] + BN_EPS)
    return t[f"{p}.conv.weight"] * scale.view(-1, 1, 1, 1), t[f"{p}.bn.bias"] - t[f"{p}.bn.running_mean"] * scale


def fold_batchnorm(state, conv):
    """-> (weight fp32 [Cout, KH KW Cin4] with columns (ky, kx, ci), bias fp32 [Cout]): fold_batchnorm64 rounded to fp32 once and laid out for ffn_conv2d.
    Cin4 = Cin rounded up to 4 (the stem's 3 image channels; the added column is zero)."""
    wt, bias = fold_batchnorm64(state, conv)
    cin4 = -(-conv.cin // 4) * 4
    packed = torch.zeros(conv.cout, conv.k[0], conv.k[1], cin4, dtype=torch.float64)
    packed[..., :conv.cin] = wt.permute(0, 2, 3, 1)
    return packed.reshape(conv.cout, -1).to(torch.float32).contiguous(), bias.to(torch.float32).contiguous()


def pack_state(config, state):
    """{layer: (weight, bias)} on the host for every convolution of the configuration (fold_batchnorm).  Entries the network does not have (fc.*,
    AuxLogits.*, num_batches_tracked) are ignored."""
    return {c.name: fold_batchnorm(state, c) for c in all_convs(config)}


def synthetic_state(config, seed=0):
    """a seeded fp32 state dict in pytorch-fid's layout for timing and smoke runs: He-scaled convolutions, BatchNorm near the identity"""
    g = torch.Generator().manual_seed(seed)
    st = {}
    for c in all_convs(config):
        st[f"{c.name}.conv.weight"] = torch.randn(c.cout, c.cin, *c.k, generator=g) * (2.0 / (c.cin * c.k[0] * c.k[1])) ** 0.5
        u = torch.rand(4, c.cout, generator=g)
        st[f"{c.name}.bn.weight"], st[f"{c.name}.bn.bias"] = 0.9 + 0.2 * u[0], -0.1 + 0.2 * u[1]
        st[f"{c.name}.bn.running_mean"], st[f"{c.name}.bn.running_var"] = -0.1 + 0.2 * u[2], 0.5 + u[3]
    return st


class HipFIDInception:
    """HipFIDInception(config, state, device): `state` in pytorch-fid's layout (Conv2d_1a_3x3.conv.weight, ....bn.{weight, bias, running_mean, running_var},
    Mixed_5b.branch1x1.conv.weight, ...); fc.* and num_batches_tracked entries are ignored.  fp32 only: a full-size image is 11.5 GFLOP, a whole GeoBench
    run a few seconds of fp32 MFMA work."""

    def __init__(self, config, state, device=None, side=None):
        if config not in CONFIGS:
            raise ValueError(f"unknown Inception configuration {config!r} (one of {CONFIGS})")
        self.config = config
        self.device = torch.device("cuda:0" if device is None else device)
        self.side = 299 if side is None else int(side)
        if config == "full" and self.side != 299:
            raise ValueError("the full network resizes its input to 299 x 299")
        if self.side < MIN_SIDE:
            raise ValueError(f"side {self.side} below {MIN_SIDE}: a stage would lose its last pixel")
        self.stem, self.blocks = layer_table(config)
        self.dim = self.blocks[-1][3]
        self._w = {name: (wt.to(self.device), b.to(self.device)) for name, (wt, b) in pack_state(config, state).items()}
        self._lut = ops.vit_norm_table(IMAGENET_MEAN, IMAGENET_STD).to(self.device)

    @classmethod
    def from_state(cls, state, config="full", device=None, side=None):
        return cls(config, state, device, side)

    # ---- layers ----
    def _conv(self, c, x, out=None):
        wt, b = self._w[c.name]
        return ops.conv2d_kk(x, wt, b, c.k[0], c.k[1], c.stride, c.pad, relu=True, out=out)

    def _block(self, kind, cin, cout, L, x):
        B, H, W, _ = x.shape
        assert x.shape[3] == cin
        down = kind in ("B", "D")
        Ho, Wo = (ops.conv_out_size(H, 3, 2, 0), ops.conv_out_size(W, 3, 2, 0)) if down else (H, W)
        out = torch.empty(B, Ho, Wo, cout, dtype=torch.float32, device=x.device)
        col = [0]

        def cols(n):
            v = out[..., col[0]:col[0] + n]
            col[0] += n
            return v

        def chain(names, src=x):
            for n in names[:-1]:
                src = self._conv(L[n], src)
            self._conv(L[names[-1]], src, out=cols(L[names[-1]].cout))

        if kind == "A":
            chain(["branch1x1"])
            chain(["branch5x5_1", "branch5x5_2"])
            chain(["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"])
            chain(["branch_pool"], ops.pool2d(x, "avg_valid", 3, 1, 1))
        elif kind == "B":
            chain(["branch3x3"])
            chain(["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"])
            ops.pool2d(x, "max", 3, 2, 0, out=cols(cin))
        elif kind == "C":
            chain(["branch1x1"])
            chain(["branch7x7_1", "branch7x7_2", "branch7x7_3"])
            chain(["branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"])
            chain(["branch_pool"], ops.pool2d(x, "avg_valid", 3, 1, 1))
        elif kind == "D":
            chain(["branch3x3_1", "branch3x3_2"])
            chain(["branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"])
            ops.pool2d(x, "max", 3, 2, 0, out=cols(cin))
        else:
            chain(["branch1x1"])
            t = self._conv(L["branch3x3_1"], x)
            chain(["branch3x3_2a"], t)
            chain(["branch3x3_2b"], t)
            t = self._conv(L["branch3x3dbl_2"], self._conv(L["branch3x3dbl_1"], x))
            chain(["branch3x3dbl_3a"], t)
            chain(["branch3x3dbl_3b"], t)
            chain(["branch_pool"], ops.pool2d(x, "avg_valid" if kind == "E1" else "max", 3, 1, 1))
        assert col[0] == cout
        return out

    @torch.no_grad()
    def forward(self, x, blocks=False):
        """x fp32 [B, side, side, 4] NHWC on the device (as ops.fid_prep writes it) -> pool3 features fp32 [B, dim]; blocks=True: the outputs of pytorch-fid's four
        blocks instead, NHWC (after each of the two max pools, after Mixed_6e, and the features as [B, 1, 1, dim])"""
        s = self.stem
        x = self._conv(s[2], self._conv(s[1], self._conv(s[0], x)))
        b0 = x = ops.pool2d(x, "max", 3, 2, 0)
        x = self._conv(s[4], self._conv(s[3], x))
        b1 = x = ops.pool2d(x, "max", 3, 2, 0)
        b2 = None
        for kind, name, cin, cout, L in self.blocks:
            x = self._block(kind, cin, cout, L, x)
            if name == "Mixed_6e":
                b2 = x
        f = ops.mean_hw(x)
        return [b0, b1, b2, f.view(f.shape[0], 1, 1, -1)] if blocks else f

    @torch.no_grad()
    def features_224(self, small, blocks=False):
        """uint8 [B, S, S, 3] on the device, already resized (S = 224 in the metric) -> features: ToTensor + Normalize as a lookup, the bilinear resize to
        side x side, 2 v - 1 (ffn_fid_prep), then the network"""
        return self.forward(ops.fid_prep(small, self._lut, self.side), blocks)

    @torch.no_grad()
    def features_u8(self, images, size=224):
        """images uint8 [B, H, W, 3] of ONE size (numpy or torch, host or device) -> fp32 [B, dim]: the transform of fid_score.py:124 -- Resize((224, 224)) of the PIL
        image (PIL's antialiased bilinear, bit for bit), ToTensor, Normalize(imagenet) -- and pytorch-fid's own resize and rescale, all on the device.  Yes, the
        reference normalises twice; so does this."""
        from . import encoder
        img, _ = encoder.u8_batch(images, None, self.device)
        return self.features_224(ops.resize_pil_bilinear_u8(img, size, size))

