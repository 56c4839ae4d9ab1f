"""DepthAnything (DINOv2 ViT encoder + DPT head) on the HIP kernels: the depth network of the 3D coarse-edit front end
(/root/reference/depth_anything/dpt.py:143-172 DPT_DINOv2.forward, :22-137 DPTHead, blocks.py:38-153,
torchhub/facebookresearch_dinov2_main/vision_transformer.py:178-317).

The encoder half (weights, tokens, blocks) is dino.py's HipDinoEncoder, shared with the metrics' feature extractor HipDinoV2, and its blocks are encoder.py's; this
module adds the DPT head.

Same design as unet.py / vae.py: activations are token / NHWC rows, every Linear, 1x1 conv, 3x3 conv, patch embedding and
transposed conv is an `ffn_igemm` call, LayerNorm and attention are the UNet's kernels (`ffn_layernorm`, `ffn_attn` with head
dim 64 and the ragged S = 1 + (H/14)(W/14)); what the UNet did not need is in the C ABI as `FFN_IG_OUT_GELU` / `FFN_IG_OUT_RELU`
epilogues, `ffn_eltwise` (the activation in front of a ResidualConvUnit, the fusion blocks' skip add) and `ffn_resize_bilinear`
(align_corners = True).  Folded at pack time: LayerScale into attn.proj / mlp.fc2 (rows scaled by gamma), the patch embedding
into a [C, 3*14*14] GEMM weight over an im2col view of the image, ConvTranspose2d(k = s) into a GEMM with k*k*C_out columns followed by
a pixel shuffle (tensor plumbing).  torch is used for layout plumbing only (im2col view, concatenating the class token, the pixel
shuffle, the one-off bicubic interpolation of the positional embedding per input size).

dtype float32 = parity mode (exact-fp32 MFMA), bfloat16 = fast mode.
"""
from types import SimpleNamespace

import torch

from . import ops
from . import encoder
from .dino import _ENC, HipDinoEncoder, dinov2_param_shapes


def depth_config(name="vitl"):
    """encoder = dinov2_{vits,vitb,vitl}14 (hubconf.py: img_size 518, patch 14, LayerScale, mlp ffn, interpolate_offset 0.1); DPT head sizes of
    the released Depth-Anything checkpoints (dpt.py:144: the vitl head)"""
    enc = _ENC[name]
    head = dict(vits=(64, (48, 96, 192, 384)), vitb=(128, (96, 192, 384, 768)), vitl=(256, (256, 512, 1024, 1024)),
                tiny=(32, (16, 32, 64, 64)), mini=(48, (24, 48, 96, 96)))[name]
    return SimpleNamespace(name=name, embed_dim=enc[0], depth=enc[1], num_heads=enc[2], patch=14, img_size=518, mlp_ratio=4,
                           features=head[0], out_channels=head[1], interpolate_offset=0.1, ln_eps=1e-6)


def depth_param_shapes(cfg):
    """name -> shape of DPT_DINOv2(encoder, features, out_channels, use_bn=False, use_clstoken=False).state_dict() (dpt.py:143-153)"""
    C = cfg.embed_dim
    sh = dinov2_param_shapes(cfg, "pretrained.")
    oc, f = cfg.out_channels, cfg.features
    h = "depth_head."
    for i in range(4):
        sh[h + f"projects.{i}.weight"], sh[h + f"projects.{i}.bias"] = (oc[i], C, 1, 1), (oc[i],)
        sh[h + f"scratch.layer{i + 1}_rn.weight"] = (f, oc[i], 3, 3)
    sh[h + "resize_layers.0.weight"], sh[h + "resize_layers.0.bias"] = (oc[0], oc[0], 4, 4), (oc[0],)
    sh[h + "resize_layers.1.weight"], sh[h + "resize_layers.1.bias"] = (oc[1], oc[1], 2, 2), (oc[1],)
    sh[h + "resize_layers.3.weight"], sh[h + "resize_layers.3.bias"] = (oc[3], oc[3], 3, 3), (oc[3],)
    for i in range(1, 5):
        r = h + f"scratch.refinenet{i}."
        sh[r + "out_conv.weight"], sh[r + "out_conv.bias"] = (f, f, 1, 1), (f,)
        for u in ("resConfUnit1", "resConfUnit2"):
            for c in ("conv1", "conv2"):
                sh[r + f"{u}.{c}.weight"], sh[r + f"{u}.{c}.bias"] = (f, f, 3, 3), (f,)
    sh[h + "scratch.output_conv1.weight"], sh[h + "scratch.output_conv1.bias"] = (f // 2, f, 3, 3), (f // 2,)
    sh[h + "scratch.output_conv2.0.weight"], sh[h + "scratch.output_conv2.0.bias"] = (32, f // 2, 3, 3), (32,)
    sh[h + "scratch.output_conv2.2.weight"], sh[h + "scratch.output_conv2.2.bias"] = (1, 32, 1, 1), (1,)
    return sh


def synthetic_state(cfg, seed=0):
    """seeded random weights of a plausible scale for benchmarks without a checkpoint (`tools/bench_depth.py`; there is no network)"""
    return encoder.draw_state(depth_param_shapes(cfg), seed, fan_in_first=("resize_layers.0", "resize_layers.1"))


class HipDepthAnything(HipDinoEncoder):
    def __init__(self, cfg, state, dtype=torch.bfloat16, device="cuda:0"):
        """state: DPT_DINOv2.state_dict() (`pretrained.*`, `depth_head.*`; use_bn = False, use_clstoken = False)"""
        self._init_encoder(cfg, dtype, device)
        assert cfg.features % 16 == 0 and all(c % 8 == 0 for c in cfg.out_channels), \
            "channel counts must be whole 16-byte chunks (features / 2 feeds a 3x3 conv)"
        self._pack({k: v.detach().to(self.device, torch.float32) for k, v in state.items()})

    # ------------------------------------------------------------------------------------------------------------
    # weights (the encoder's: dino.py HipDinoEncoder._pack_encoder)
    # ------------------------------------------------------------------------------------------------------------
    def _lin(self, w, b, n_pad=None):
        """a 1x1 convolution / Linear of the head as a GEMM: [N, K(, 1, 1)] -> (packed weight, fp32 bias), N zero-padded to n_pad rows"""
        w = w.reshape(w.shape[0], -1)
        if n_pad and n_pad > w.shape[0]:
            w = torch.cat([w, torch.zeros(n_pad - w.shape[0], w.shape[1], device=w.device)], 0)
            b = torch.cat([b, torch.zeros(n_pad - b.shape[0], device=b.device)], 0)
        return ops.pack_linear(w.contiguous(), self.dtype), b.float().contiguous()

    def _conv(self, st, name, bias=True):
        w = st[name + ".weight"]
        return ops.pack_conv3x3(w, self.dtype), (st[name + ".bias"].contiguous() if bias else None), w.shape[1]

    def _deconv(self, st, name, k):
        """ConvTranspose2d(kernel = stride = k): out[4y+dy, 4x+dx, co] = sum_ci in[y, x, ci] w[ci, co, dy, dx] + b[co] -> GEMM columns (dy, dx, co)"""
        w, b = st[name + ".weight"], st[name + ".bias"]       # [in, out, k, k]
        cin, cout = w.shape[0], w.shape[1]
        wg = w.permute(2, 3, 1, 0).reshape(k * k * cout, cin).contiguous()
        return ops.pack_linear(wg, self.dtype), b.repeat(k * k).contiguous(), cin, cout, k

    def _pack(self, st):
        cfg = self.cfg
        self._pack_encoder(st, "pretrained.")
        h = "depth_head."
        self.projects = [self._lin(st[h + f"projects.{i}.weight"], st[h + f"projects.{i}.bias"]) for i in range(4)]
        self.up0 = self._deconv(st, h + "resize_layers.0", 4)
        self.up1 = self._deconv(st, h + "resize_layers.1", 2)
        self.down3 = self._conv(st, h + "resize_layers.3")
        self.rn = [self._conv(st, h + f"scratch.layer{i + 1}_rn", bias=False) for i in range(4)]
        self.refine = []
        for i in range(1, 5):
            r, q = SimpleNamespace(), h + f"scratch.refinenet{i}."
            r.u1 = (self._conv(st, q + "resConfUnit1.conv1"), self._conv(st, q + "resConfUnit1.conv2"))
            r.u2 = (self._conv(st, q + "resConfUnit2.conv1"), self._conv(st, q + "resConfUnit2.conv2"))
            r.out = self._lin(st[q + "out_conv.weight"], st[q + "out_conv.bias"])
            self.refine.append(r)
        self.oc1 = self._conv(st, h + "scratch.output_conv1")
        self.oc2 = self._conv(st, h + "scratch.output_conv2.0")
        self.oc3 = self._lin(st[h + "scratch.output_conv2.2.weight"], st[h + "scratch.output_conv2.2.bias"], n_pad=4)

    # ------------------------------------------------------------------------------------------------------------
    # encoder (tokens and blocks: dino.py HipDinoEncoder)
    # ------------------------------------------------------------------------------------------------------------
    def features(self, x):
        """get_intermediate_layers(x, 4, return_class_token=True, norm=True): patch tokens [B, N, C] of the last four blocks"""
        cfg = self.cfg
        t, ph, pw = self._tokens(x)
        outs = [ops.layernorm(o, *self.norm, eps=cfg.ln_eps)[:, 1:].contiguous() for o in self._run_blocks(t, 4)]
        return outs, ph, pw

    # ------------------------------------------------------------------------------------------------------------
    # DPT head (NHWC rows)
    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _pixel_shuffle(y, B, H, W, k, cout):
        """GEMM output [B, H*W, (dy, dx, co)] of a ConvTranspose2d(kernel = stride = k) -> NHWC rows [B, (H k)(W k), co]"""
        return y.view(B, H, W, k, k, cout).permute(0, 1, 3, 2, 4, 5).reshape(B, H * k * W * k, cout).contiguous()

    def _up(self, x, B, H, W, dc):
        w, b, cin, cout, k = dc
        y = ops.linear(x, w, b, K=cin)                                               # [B, H*W, k*k*cout]
        return self._pixel_shuffle(y, B, H, W, k, cout), H * k, W * k

    def _rcu(self, u, x, B, H, W, extra=None):
        """ResidualConvUnit (blocks.py:68-83): conv2(relu(conv1(relu(x)))) + x (+ extra: the fusion block's other input)"""
        C = x.shape[-1]
        y = ops.conv3x3(ops.relu(x), u[0][0], u[0][1], B, H, W, C, relu=True)
        return ops.conv3x3(y, u[1][0], u[1][1], B, H, W, C, residual=x if extra is None else ops.add(x, extra))

    def _fusion(self, r, xs, B, H, W, size):
        """FeatureFusionBlock (blocks.py:128-153), xs = [path (, skip level)], resized to `size` (align_corners = True), out_conv"""
        out = xs[0]
        if len(xs) == 2:
            out = self._rcu(r.u1, xs[1], B, H, W, extra=out)
        out = self._rcu(r.u2, out, B, H, W)
        out = ops.resize_bilinear(out, B, H, W, size[0], size[1])
        return ops.linear(out, r.out[0], r.out[1], K=out.shape[-1])

    def head(self, feats, ph, pw):
        cfg = self.cfg
        B = feats[0].shape[0]
        C = cfg.embed_dim
        lv = []
        for i, x in enumerate(feats):
            x = ops.linear(x, self.projects[i][0], self.projects[i][1], K=C)
            if i == 0:
                x, h, w = self._up(x, B, ph, pw, self.up0)
            elif i == 1:
                x, h, w = self._up(x, B, ph, pw, self.up1)
            elif i == 2:
                h, w = ph, pw
            else:
                x = ops.conv3x3(x, self.down3[0], self.down3[1], B, ph, pw, x.shape[-1], stride=2)
                h, w = (ph - 1) // 2 + 1, (pw - 1) // 2 + 1
            lv.append((ops.conv3x3(x, self.rn[i][0], None, B, h, w, x.shape[-1]), h, w))
        (l1, h1, w1), (l2, h2, w2), (l3, h3, w3), (l4, h4, w4) = lv
        p4 = self._fusion(self.refine[3], [l4], B, h4, w4, (h3, w3))
        p3 = self._fusion(self.refine[2], [p4, l3], B, h3, w3, (h2, w2))
        p2 = self._fusion(self.refine[1], [p3, l2], B, h2, w2, (h1, w1))
        p1 = self._fusion(self.refine[0], [p2, l1], B, h1, w1, (2 * h1, 2 * w1))
        H1, W1 = 2 * h1, 2 * w1
        out = ops.conv3x3(p1, self.oc1[0], self.oc1[1], B, H1, W1, cfg.features)
        Ho, Wo = ph * 14, pw * 14
        out = ops.resize_bilinear(out, B, H1, W1, Ho, Wo)
        out = ops.conv3x3(out, self.oc2[0], self.oc2[1], B, Ho, Wo, cfg.features // 2, relu=True)
        out = ops.linear(out, self.oc3[0], self.oc3[1], K=32, relu=True, out_f32=True)       # [B, Ho*Wo, 4]: channel 0 is the depth
        return out, Ho, Wo

    @torch.no_grad()
    def forward(self, x):
        """x [B, 3, H, W] (normalised image, H and W multiples of 14) -> depth [B, H, W] fp32 (DPT_DINOv2.forward, dpt.py:155-167)"""
        B, _, H, W = x.shape
        assert H % 14 == 0 and W % 14 == 0, "DINOv2 patch embedding: image sides must be multiples of 14"
        feats, ph, pw = self.features(x)
        d, Ho, Wo = self.head(feats, ph, pw)
        if (Ho, Wo) != (H, W):                                 # (never with sides that are multiples of 14; kept for the reference's call shape)
            d = ops.resize_bilinear(d, B, Ho, Wo, H, W, relu=True)
        return d[..., 0].reshape(B, H, W).float()              # the final F.relu is the last GEMM's epilogue

    __call__ = forward
