"""Typed wrappers over the C ABI for torch device tensors (device memory + current stream only; no torch math).

Activations are [B, HW, C] channel-contiguous tensors of dtype float32 ("parity mode") or bfloat16 ("fast mode").
"""
import ctypes as CT
import math

import os
import threading

import torch

from . import _lib as L


def _dt(t):
    if t.dtype == torch.float32:
        return L.FFN_F32
    if t.dtype == torch.bfloat16:
        return L.FFN_BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def epc(dtype):
    return 4 if dtype == torch.float32 else 8


def kstage(dtype):
    return 8 * epc(dtype)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------
# optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg)
# ---------------------------------------------------------------------------------------------------------------
_PROF = None


def profile_begin():
    global _PROF
    _PROF = []


def profile_end():
    """-> {kernel name: dict(calls, total_ms, flops, bytes)}; kernel names spelled like rocprofv3's kernel trace."""
    global _PROF
    rec, _PROF = _PROF, None
    torch.cuda.synchronize()
    out = {}
    for name, flops, nbytes, s, e in rec:
        d = out.setdefault(name, dict(calls=0, total_ms=0.0, flops=0.0, bytes=0.0))
        d["calls"] += 1
        d["total_ms"] += s.elapsed_time(e)
        d["flops"] += flops
        d["bytes"] += nbytes
    return out


def _timed(name, flops, nbytes, fn):
    if _PROF is None:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = fn()
    e.record()
    _PROF.append((name, flops, nbytes, s, e))
    return rc


def _tname(t):
    return "float" if t.dtype == torch.float32 else "bf16"


def _igemm_name(lib, dcode, d):
    buf = CT.create_string_buffer(160)
    lib.ffn_igemm_kernel_name(dcode, CT.byref(d), buf, 160)
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------------------------
# weight packing (host side, once at load time)
# ---------------------------------------------------------------------------------------------------------------
_ATTN_PRESPLIT = True      # not an option: tests clear it to run attn_x3p_kernel (which serves K / V^T of 2 GiB and more and layouts the image path refuses) at small shapes


def _mark_x3(t, order=1):
    t._ffn_x3 = order         # linear() / conv3x3() recognise a split-bf16 weight by this tag and run the FFN_BF16X3 path
    return t                  # (1 = planes [hi | lo | hi] over the whole K / tap, 2 = blocked: 128-byte blocks [hi(32) | lo(32)] per 32 elements of K)


def is_x3(w):
    return bool(getattr(w, "_ffn_x3", 0))


def split_hi_lo(w):
    """fp32 -> (hi, lo) bf16 with hi = bf16(w) (RNE), lo = bf16(w - hi): the operand form of the FFN_BF16X3 GEMMs"""
    w = w.float()
    hi = w.to(torch.bfloat16)
    return hi, (w - hi.float()).to(torch.bfloat16)


def pack_linear(w, dtype, x3=False):
    """[N, K] -> [N, Kpad] zero padded, contiguous, dtype.  x3 (split-bf16, include/freefine_hip.h FFN_BF16X3): K % 32 == 0 -> the BLOCKED pair
    form of every row, bf16 [N, 2K] = 128-byte blocks [W_hi(32) | W_lo(32)] (layout 2: what the ping-pong tile's split-bf16 core streams);
    otherwise the planes bf16 [N, 3K] = [W_hi | W_lo | W_hi] (layout 1), the virtual contraction run against the activation's [A_hi | A_hi | A_lo]."""
    n, k = w.shape
    if x3:
        assert k % 8 == 0, f"split-bf16 weights need K % 8 == 0 (K={k})"
        hi, lo = split_hi_lo(w)
        if k % 32 == 0:
            return _mark_x3(torch.stack([hi.reshape(n, k // 32, 32), lo.reshape(n, k // 32, 32)], dim=2).reshape(n, 2 * k).contiguous(), 2)
        return _mark_x3(torch.cat([hi, lo, hi], dim=1).contiguous(), 1)
    ks = kstage(dtype)
    kpad = (k + ks - 1) // ks * ks
    out = torch.zeros(n, kpad, dtype=dtype, device=w.device)
    out[:, :k] = w.to(dtype)
    return out


def pack_conv3x3(w, dtype, cin_pad=None, x3=False):
    """[Cout, Cin, 3, 3] -> [Cout, Kpad], k = (ky*3+kx)*Cin_p + ci  (x3: per tap the blocked pair form of its Cin_p columns, Cin_p % 32 == 0;
    else k' = ((ky*3+kx)*3 + seg)*Cin_p + ci, seg = hi, lo, hi)."""
    cout, cin = w.shape[:2]
    cp = cin_pad or cin
    w2 = torch.zeros(cout, 3, 3, cp, dtype=torch.float32, device=w.device)
    w2[..., :cin] = w.permute(0, 2, 3, 1).float()
    if x3:
        assert cp % 8 == 0, f"split-bf16 conv weights need Cin % 8 == 0 (Cin={cp})"
        hi, lo = split_hi_lo(w2.reshape(cout, 9, cp))
        if cp % 32 == 0:
            return _mark_x3(torch.stack([hi.reshape(cout, 9, cp // 32, 32), lo.reshape(cout, 9, cp // 32, 32)], dim=3).reshape(cout, 18 * cp).contiguous(), 2)
        return _mark_x3(torch.cat([hi, lo, hi], dim=2).reshape(cout, 27 * cp).contiguous(), 1)
    return pack_linear(w2.reshape(cout, 9 * cp), dtype)


def pack_conv3x3_n4(w):
    """[4, Cin, 3, 3] -> fp32 [4, 9 * Cin] in (ky, kx, ci) order: the weights of ffn_conv3x3_n4 (the UNet's conv_out on the vector ALU)"""
    assert w.shape[0] == 4 and w.shape[2:] == (3, 3)
    return w.float().permute(0, 2, 3, 1).reshape(4, -1).contiguous()


def conv3x3_n4_eligible(cout, cin):
    return cout == 4 and cin % 16 == 0 and cin <= 448


def conv3x3_n4(x, w4, bias, B, H, W, Cin):
    """3x3 / stride 1 / pad 1 convolution with four output channels as a direct fp32 convolution (ffn_conv3x3_n4): x [B, H*W, Cin] fp32 or
    bf16, w4 from pack_conv3x3_n4; returns fp32 [B, H*W, 4]"""
    lib = L.load()
    assert x.is_contiguous() and x.shape[-1] == Cin and x.dtype in (torch.float32, torch.bfloat16)
    out = torch.empty(B, H * W, 4, dtype=torch.float32, device=x.device)
    L.check(_timed("conv3x3_n4_kernel", 2.0 * B * H * W * 4 * 9 * Cin, x.element_size() * x.numel() + 16.0 * B * H * W,
                   lambda: lib.ffn_conv3x3_n4(_stream(), _dt(x), x.data_ptr(), w4.data_ptr(), _p(bias), out.data_ptr(), B, H, W, Cin)), "ffn_conv3x3_n4")
    return out


def up2x_eligible(cin, cout, rows):
    """does the sub-pixel form of `nearest-2x upsample -> 3x3 conv` apply?  (bf16 ping-pong tiles: whole 64-channel chunks, N a tile multiple,
    at least one 192-row tile of LOW-resolution pixels)"""
    return cin % 64 == 0 and (cout % 256 == 0 or cout % 320 == 0) and rows >= 192


def pack_conv3x3_up2x(w, dtype, x3=False):
    """[Cout, Cin, 3, 3] of a 3x3 conv that follows a nearest-2x upsample -> [4 Cout, 4 Cin] weights of its four sub-pixel classes.
    Output pixel (2y + a, 2x + b) sees the upsampled rows 2y + a - 1 .. 2y + a + 1 = low-resolution rows {y - 1, y, y} (a = 0) or {y, y, y + 1}
    (a = 1): a 2x2 window starting at (y + a - 1, x + b - 1) whose taps are sums of the 3x3 taps that coincide -- 4/9 of the multiplies.
    Rows [c Cout, (c + 1) Cout) hold class c = 2a + b, k = (dy*2 + dx) Cin + ci.  The sums are taken in fp32 and rounded once.
    x3 (split-bf16 mode, Cin % 32 == 0): the blocked pair form of pack_conv3x3 over the four taps."""
    assert dtype == torch.bfloat16 or x3
    cout, cin = w.shape[:2]
    wf = w.float()
    groups = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}           # parity -> 3x3 tap indices feeding window position 0 / 1
    out = torch.empty(4, cout, 2, 2, cin, dtype=torch.float32, device=w.device)
    for a in (0, 1):
        for b in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    acc = torch.zeros(cout, cin, dtype=torch.float32, device=w.device)
                    for ky in groups[a][dy]:
                        for kx in groups[b][dx]:
                            acc += wf[:, :, ky, kx]
                    out[2 * a + b, :, dy, dx] = acc
    if x3:
        assert cin % 32 == 0
        hi, lo = split_hi_lo(out.reshape(4 * cout, 4, cin))
        return _mark_x3(torch.stack([hi.reshape(4 * cout, 4, cin // 32, 32), lo.reshape(4 * cout, 4, cin // 32, 32)], dim=3).reshape(4 * cout, 8 * cin).contiguous(), 2)
    return pack_linear(out.reshape(4 * cout, 4 * cin), dtype)


def conv3x3_up2x(x, w4, bias, B, Hin, Win, Cin, *, out=None):
    """nearest-2x upsample followed by the 3x3 conv (pad 1) packed by pack_conv3x3_up2x, evaluated at LOW resolution: four 2x2 convolutions
    (conv = 2 of ffn_igemm, one per output-pixel parity class) into one [B, Hin*Win, 4 Cout] buffer + a pixel shuffle (layout plumbing).
    x: [B, Hin*Win, Cin] bf16 (split-bf16 weights: fp32, or its pair rows); returns [B, 4*Hin*Win, Cout] (written into `out`, which may be a
    column view of a wider buffer)."""
    lib = L.load()
    cout = w4.shape[0] // 4
    x3 = is_x3(w4)
    # the ping-pong kernel addresses its operands through 31-bit buffer resources: batches whose [B, HW, 4 Cout] result (or input) would pass
    # 1 GiB go in slices of whole images (the VAE decoder at 256 x 256 x 512 channels)
    per_img = Hin * Win * max(4 * cout * (4 if x3 else 2), Cin * (4 if x3 else 2))
    nb = max(1, ((1 << 30) - 1) // per_img)
    if B > nb:
        if out is None:
            out = torch.empty(B, 4 * Hin * Win, cout, dtype=torch.float32 if x3 else x.dtype, device=x.device)
        for b0 in range(0, B, nb):
            b1 = min(B, b0 + nb)
            conv3x3_up2x(x[b0:b1], w4, bias, b1 - b0, Hin, Win, Cin, out=out[b0:b1])
        return out
    if x3:                                          # split-bf16 mode: fp32 activations as pair rows, fp32 result
        xa = x if pair_width(x) is not None else split_pair(x, Cin)
        assert pair_width(xa) == Cin
        odt, dcode = torch.float32, L.FFN_BF16X3
    else:
        assert x.dtype == torch.bfloat16 and x.is_contiguous()
        xa, odt, dcode = x, x.dtype, L.FFN_BF16
    assert w4.shape[1] >= (8 if x3 else 4) * Cin
    y = torch.empty(B, Hin * Win, 4 * cout, dtype=odt, device=x.device)
    for c in range(4):
        a, b = c >> 1, c & 1
        d = L.IgemmDesc()
        d.A, d.W = xa.data_ptr(), w4.data_ptr() + c * cout * w4.stride(0) * w4.element_size()
        d.bias, d.rowbias, d.residual = _p(bias), None, None
        d.M, d.N, d.K, d.Kpad = B * Hin * Win, cout, 4 * Cin, w4.stride(0)
        d.lda, d.a_lo, d.x3 = (2 * Cin, 32, 2) if x3 else (Cin, 0, 0)
        d.rows_per_batch, d.ldrb = Hin * Win, 0
        d.out, d.ldo, d.ldr = y.data_ptr() + c * cout * y.element_size(), 4 * cout, 0
        d.Hin, d.Win, d.Cin, d.Hout, d.Wout = Hin, Win, Cin, Hin, Win
        d.stride, d.pad, d.upsample = 1, 2 * (1 - a) + (1 - b), 0
        d.flags, d.alpha, d.conv = 0, 1.0, 2
        d.splitk, d.ws, d.ws_bytes = 0, _workspace(x.device).data_ptr(), WS_BYTES
        if _PROF is None:
            L.check(lib.ffn_igemm(_stream(), dcode, CT.byref(d)), "ffn_igemm(conv 2x2)")
        else:
            L.check(_timed(_igemm_name(lib, dcode, d), 2.0 * d.M * cout * 4 * Cin, y.element_size() * (x.numel() + cout * 4 * Cin + d.M * cout),
                           lambda: lib.ffn_igemm(_stream(), dcode, CT.byref(d))), "ffn_igemm(conv 2x2)")
    if out is None:
        out = torch.empty(B, 4 * Hin * Win, cout, dtype=odt, device=x.device)
    # pixel shuffle: class (a, b) of low-resolution pixel (y, x) is output pixel (2y + a, 2x + b)
    out.view(B, Hin, 2, Win, 2, cout).copy_(y.view(B, Hin, Win, 2, 2, cout).permute(0, 1, 3, 2, 4, 5))
    return out


F8_ACT_SCALE = 16.0         # power-of-two scale of fp8 activations: SiLU(GroupNorm(x)) * 16 saturates at 28, far above its range


def pack_conv3x3_f8(w, cin_pad=None):
    """[Cout, Cin, 3, 3] -> e4m3 bytes [Cout, 9 * Cp] (uint8 storage), k = (ky*3+kx)*Cp + ci, Cp = Cin padded to a multiple of 128 (whole
    K tiles of the fp8 ping-pong conv), scaled by a per-tensor power of two so that max |w| lands in [224, 448).  The tensor carries
    `_ffn_f8 = (Cp, alpha)`, alpha = 1 / (weight scale * F8_ACT_SCALE) = what the GEMM epilogue multiplies by (FFN_FP8, freefine_hip.h)."""
    cout, cin = w.shape[:2]
    cp = cin_pad or (cin + 127) // 128 * 128
    w2 = torch.zeros(cout, 3, 3, cp, dtype=torch.float32, device=w.device)
    w2[..., :cin] = w.permute(0, 2, 3, 1).float()
    amax = float(w2.abs().max())
    k = math.floor(math.log2(448.0 / amax)) if amax > 0 else 0
    ws = 2.0 ** k
    q = (w2 * ws).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).reshape(cout, 9 * cp).contiguous().view(torch.uint8)
    q._ffn_f8 = (cp, 1.0 / (ws * F8_ACT_SCALE))
    return q


def is_f8(w):
    return getattr(w, "_ffn_f8", None) is not None


def groupnorm_f8(x, gamma, beta, G, eps, Cp, silu=False, ws=None):
    """bf16 x [B, HW, C] -> e4m3 bytes [B, HW, Cp] = act(GroupNorm(x)) * F8_ACT_SCALE, channels >= C zero: the A operand of an fp8 conv"""
    lib = L.load()
    B, HW, Cc = x.shape
    assert x.dtype == torch.bfloat16
    out = torch.empty(B, HW, Cp, dtype=torch.uint8, device=x.device)
    out._ffn_f8_act = Cc
    partial, scale, shift = ws if ws is not None else gn_workspace(B, HW, Cc, x.device)
    call = lambda: lib.ffn_groupnorm_f8(_stream(), x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), B, HW, Cc, Cp, G, eps,
                                        L.NORM_SILU if silu else 0, F8_ACT_SCALE, partial.data_ptr(), scale.data_ptr(), shift.data_ptr())
    L.check(_timed("gn_partial+gn_finalize+gn_apply_f8", 0.0, x.numel() * 2.0 + out.numel(), call), "ffn_groupnorm_f8")
    return out


def pack_geglu(w, b, dtype, x3=False):
    """GEGLU proj [2F, K] (+bias [2F]): interleave 16-row blocks hidden/gate so one lane holds both halves."""
    f2, k = w.shape
    f = f2 // 2
    assert f % 16 == 0
    idx = torch.arange(f, device=w.device).reshape(f // 16, 16)
    order = torch.stack([idx, idx + f], dim=1).reshape(-1)  # [h0..h15, g0..g15, h16.., ...]
    wp = pack_linear(w[order], dtype, x3)
    bp = None if b is None else b[order].float().contiguous()
    return wp, bp


def _mark_pair(t, C):
    t._ffn_pair = C            # bf16 [..., 2C]: the pair form of rows of C fp32 values (C % 32 == 0: 128-byte blocks [hi(32) | lo(32)]; else planes): the A operand of an FFN_BF16X3 GEMM
    return t


def pair_width(x):
    """C if x is a split-bf16 pair tensor [..., 2C], else None"""
    return getattr(x, "_ffn_pair", None)


def split_pair(x, K=None):
    """fp32 [..., ld] (first K columns) -> bf16 PAIR rows [..., 2K] (ffn_split_pair; layout: include/freefine_hip.h FFN_BF16X3): the A operand of an FFN_BF16X3 GEMM"""
    lib = L.load()
    assert x.dtype == torch.float32 and x.stride(-1) == 1
    K = K if K is not None else x.shape[-1]
    rows = x.numel() // x.shape[-1]
    ld = x.stride(-2) if x.ndim > 1 else x.shape[-1]
    out = torch.empty(*x.shape[:-1], 2 * K, dtype=torch.bfloat16, device=x.device)
    L.check(_timed("split_pair_kernel", 0.0, 8.0 * rows * K, lambda: lib.ffn_split_pair(_stream(), x.data_ptr(), out.data_ptr(), rows, K, ld)),
            "ffn_split_pair")
    return _mark_pair(out, K)


# ---------------------------------------------------------------------------------------------------------------
# igemm
# ---------------------------------------------------------------------------------------------------------------
_WS = {}
WS_BYTES = 96 << 20


def _workspace(device):
    """fp32 scratch for split-K partial slabs, one per (device, stream): reuse is ordered by the stream"""
    key = (device, torch.cuda.current_stream().cuda_stream)     # one buffer per stream: launches on different streams may overlap
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.empty(WS_BYTES // 4, dtype=torch.float32, device=device)
    return ws

_TLS = threading.local()      # batch_invariant is per host thread: executors of a shared pipeline run on threads of their own


def _invariant():
    return getattr(_TLS, "batch_invariant", False)


class batch_invariant:
    """Within this context (per host thread) the launch choices that this module or the library would take from the NUMBER OF ROWS are pinned, so that a
    row's result does not depend on what is computed beside it (HipUNet.features):
      * ffn_igemm launches of linear / conv3x3 that leave the K split to the library run unsplit (splitk = 1): the library chooses a split from how many
        tiles M x N fills the device with; unsplit, every output element is one K-ordered accumulation;
      * GroupNorm takes the form the library would choose for ONE row (ffn_gn_fused(1, ...)): where that is the one-launch fused kernel, the batch goes in
        chunks of rows small enough to keep it; where it is statistics + apply, any batch takes it anyway.  groupnorm_pair_raw decides the same way.
    What is NOT pinned: the tile of an unsplit GEMM (rule table in fp32, first-use timing in bf16), which follows M.  HipUNet.features documents what was
    measured about it."""

    def __enter__(self):
        self.prev, _TLS.batch_invariant = _invariant(), True

    def __exit__(self, *exc):
        _TLS.batch_invariant = self.prev


def linear(x, w, bias=None, *, K=None, out=None, residual=None, rowbias=None, rows_per_batch=None, silu=False,
           geglu=False, out_f32=False, transposed_ld=None, alpha=1.0, splitk=0, out_pair=False, gelu=False, relu=False, kv64_from=None, qgelu=False):
    """out = x @ w[:, :K]^T (+bias ...).  x: [..., K] rows (M = prod of leading dims).  x, w, out and residual may be column views of wider buffers
    (contiguous columns, rows one row stride apart: lda, Kpad, ldo, ldr of the descriptor are their row strides).
    kv64_from (split-bf16 only): the projection writes the attention kernels' pre-split K / V^T images itself (FFN_IG_OUT_KV64): row-major output --
    columns >= kv64_from of every row as [hi(64) | lo(64)] blocks per head in the bytes of their fp32 values; transposed output (any value, use 0) --
    every run of 64 positions of a row as one such block.  The caller hands such buffers to ops.attention(kv_images=True)."""
    lib = L.load()
    K = K if K is not None else x.shape[-1]
    M = x.numel() // x.shape[-1]
    N = w.shape[0]
    d = L.IgemmDesc()
    x3 = is_x3(w)
    if x3 and pair_width(x) is not None:            # the producer (norm / GEGLU / attention) already wrote the [hi | lo] pair rows
        K = pair_width(x)
        M = x.numel() // x.shape[-1]
        xa = x
    else:
        xa = split_pair(x, K) if x3 else x          # split-bf16: fp32 activations -> [hi | lo] bf16 rows; results / residual stay fp32
    dcode = L.FFN_BF16X3 if x3 else _dt(x)
    d.A, d.W = xa.data_ptr(), w.data_ptr()
    d.bias, d.rowbias, d.residual = _p(bias), _p(rowbias), _p(residual)
    d.M, d.N, d.K, d.Kpad = M, N, K, w.stride(0)    # Kpad = row stride of W (an activation view can serve as W)
    d.lda = xa.stride(-2) if xa.ndim > 1 else xa.shape[-1]
    d.x3 = int(w._ffn_x3) if x3 else 0
    d.a_lo = (32 if d.x3 == 2 else K) if x3 else 0          # blocked pair rows (K % 32 == 0) / planes
    odt = torch.float32 if x3 else x.dtype          # element type of out / residual
    d.rows_per_batch = rows_per_batch or M
    d.ldrb = rowbias.stride(0) if rowbias is not None else 0
    flags = 0
    n_out = N
    if silu:
        flags |= L.IG_OUT_SILU
    if gelu:
        flags |= L.IG_OUT_GELU
    if relu:
        flags |= L.IG_OUT_RELU
    if qgelu:                                       # x * sigmoid(1.702 x): CLIP ViT-L's MLP
        flags |= L.IG_OUT_QGELU
    if geglu:
        flags |= L.IG_GEGLU
        n_out = N // 2
    if out_f32:
        flags |= L.IG_OUT_F32
    if transposed_ld is not None:
        flags |= L.IG_OUT_TRANSPOSED
        nb = M // d.rows_per_batch
        if out is None:
            # columns past the rows of a batch are padding the attention kernels may multiply by P = 0: they must be finite, so a
            # padded buffer is zero-filled; without padding (every UNet level: S % 8 == 0) the GEMM writes every element
            alloc = torch.zeros if transposed_ld > d.rows_per_batch else torch.empty
            out = alloc(nb, N, transposed_ld, dtype=odt, device=x.device)
        d.ldo = transposed_ld
    elif out_pair:                                  # split-bf16 only: the result in the pair form the next GEMM reads
        assert x3 and out is None                   # (a residual is added in fp32 before the split)
        flags |= L.IG_OUT_PAIR
        out = _mark_pair(torch.empty(*x.shape[:-1], 2 * n_out, dtype=torch.bfloat16, device=x.device), n_out)
        d.ldo = 2 * n_out
    else:
        if out is None:
            out = torch.empty(*x.shape[:-1], n_out, dtype=torch.float32 if out_f32 else odt, device=x.device)
        d.ldo = out.stride(-2) if out.ndim > 1 else n_out          # a column view of a wider buffer (cat_dst) keeps the buffer's row stride
    assert xa.stride(-1) == 1 and out.stride(-1) == 1 and (residual is None or residual.stride(-1) == 1), "linear: x, out and residual need contiguous columns"
    d.ldr = (residual.stride(-2) if residual.ndim > 1 else residual.shape[-1]) if residual is not None else 0      # (a column view keeps its buffer's row stride)
    d.out = out.data_ptr()
    if kv64_from is not None:
        assert x3 and residual is None and rowbias is None and not (silu or gelu or relu or qgelu or geglu or out_pair)
        flags |= L.IG_OUT_KV64
        d.kv64_from = int(kv64_from)
        splitk = 1
    d.flags, d.alpha, d.conv = flags, alpha, 0
    if splitk == 0 and _invariant():
        splitk = 1
    d.splitk, d.ws, d.ws_bytes = splitk, _workspace(x.device).data_ptr(), WS_BYTES
    if _PROF is None:
        L.check(lib.ffn_igemm(_stream(), dcode, CT.byref(d)), "ffn_igemm")
    else:
        esz = x.element_size()
        L.check(_timed(_igemm_name(lib, dcode, d), 2.0 * M * N * K, esz * (M * K + N * K + M * n_out),
                       lambda: lib.ffn_igemm(_stream(), dcode, CT.byref(d))), "ffn_igemm")
    return out


def conv3x3(x, w, bias, B, Hin, Win, Cin, *, stride=1, pad=1, upsample=False, out=None, residual=None, rowbias=None,
            rowbias_ld=None, out_f32=False, Hout=None, Wout=None, splitk=0, relu=False):
    """x: [B, Hin*Win, Cin] NHWC; w: packed [Cout, Kpad]; returns [B, Hout*Wout, Cout]."""
    lib = L.load()
    He, We = (Hin * 2, Win * 2) if upsample else (Hin, Win)
    if Hout is None:
        Hout = (He + 2 * pad - 3) // stride + 1
        Wout = (We + 2 * pad - 3) // stride + 1
    N = w.shape[0]
    d = L.IgemmDesc()
    x3 = is_x3(w)
    f8 = is_f8(w)
    if f8:                                          # fp8 convolution: x is the e4m3 tensor groupnorm_f8 wrote, [B, HW, Cp]
        assert x.dtype == torch.uint8 and x.shape[-1] == w._ffn_f8[0] and out_f32 is False
        Cin = x.shape[-1]
        xa = x
    elif x3 and pair_width(x) is not None:
        assert pair_width(x) == Cin
        xa = x
    else:
        xa = split_pair(x, Cin) if x3 else x        # split-bf16: every pixel becomes [hi(Cin) | lo(Cin)]
    dcode = L.FFN_FP8 if f8 else (L.FFN_BF16X3 if x3 else _dt(x))
    odt = torch.float32 if x3 else (torch.bfloat16 if f8 else x.dtype)
    d.A, d.W = xa.data_ptr(), w.data_ptr()
    d.bias, d.rowbias, d.residual = _p(bias), _p(rowbias), _p(residual)
    d.M, d.N, d.K, d.Kpad = B * Hout * Wout, N, 9 * Cin, w.shape[1]
    d.lda = 2 * Cin if x3 else Cin
    d.x3 = int(w._ffn_x3) if x3 else 0
    d.a_lo = (32 if d.x3 == 2 else Cin) if x3 else 0
    d.rows_per_batch = Hout * Wout
    d.ldrb = (rowbias_ld or rowbias.stride(0)) if rowbias is not None else 0
    if out is None:
        out = torch.empty(B, Hout * Wout, N, dtype=torch.float32 if out_f32 else odt, device=x.device)
    # the conv gather reads pixels of Cin elements from a dense NHWC tensor (no pixel stride in the ABI outside split-bf16): a strided x is refused;
    # out and residual may be column views of wider buffers, which keep their buffers' row strides
    assert xa.is_contiguous(), "conv3x3: x must be contiguous (a column view of a wider buffer has no pixel stride the kernels could follow)"
    assert out.stride(-1) == 1 and (residual is None or residual.stride(-1) == 1), "conv3x3: out and residual need contiguous columns"
    d.out, d.ldo = out.data_ptr(), out.stride(-2)
    d.ldr = residual.stride(-2) if residual is not None else 0
    d.Hin, d.Win, d.Cin, d.Hout, d.Wout = Hin, Win, Cin, Hout, Wout
    d.stride, d.pad, d.upsample = stride, pad, 1 if upsample else 0
    d.flags, d.alpha, d.conv = (L.IG_OUT_F32 if out_f32 else 0) | (L.IG_OUT_RELU if relu else 0), (w._ffn_f8[1] if f8 else 1.0), 1
    if splitk == 0 and _invariant():
        splitk = 1
    d.splitk, d.ws, d.ws_bytes = splitk, _workspace(x.device).data_ptr(), WS_BYTES
    if _PROF is None:
        L.check(lib.ffn_igemm(_stream(), dcode, CT.byref(d)), "ffn_igemm(conv)")
    else:
        esz = x.element_size()
        k_real = 9 * getattr(x, "_ffn_f8_act", Cin)       # fp8: the padded channels are zeros, not work
        L.check(_timed(_igemm_name(lib, dcode, d), 2.0 * d.M * N * k_real, esz * (x.numel() + N * d.K + d.M * N),
                       lambda: lib.ffn_igemm(_stream(), dcode, CT.byref(d))), "ffn_igemm(conv)")
    return out


# ---------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------
class AttnEntrySpec:
    """One (pass, output-row) term of ffn_attn (see include/freefine_hip.h)."""
    __slots__ = ("q_row", "kv_row", "w_const", "w_slope", "wq", "kmask", "qsel", "flags", "hr_row")

    def __init__(self, q_row, kv_row, w_const=1.0, w_slope=0.0, wq=None, kmask=None, qsel=None, flags=0, hr_row=None):
        self.q_row, self.kv_row, self.w_const, self.w_slope = q_row, kv_row, w_const, w_slope
        self.wq, self.kmask, self.qsel, self.flags, self.hr_row = wq, kmask, qsel, flags, hr_row

    def remap(self, row_map, logical_row):
        """the same term for a row-deduplicated batch: Q / KV rows through logical->physical, head rule pinned to the logical row"""
        return AttnEntrySpec(row_map[self.q_row], row_map[self.kv_row], self.w_const, self.w_slope, self.wq, self.kmask, self.qsel,
                             self.flags, logical_row if self.hr_row is None else self.hr_row)

    def pinned(self, logical_row):
        """the same term with the tiled-head rule pinned to `logical_row` (unless it already is pinned)"""
        return self if self.hr_row is not None else AttnEntrySpec(self.q_row, self.kv_row, self.w_const, self.w_slope, self.wq, self.kmask, self.qsel,
                                                                  self.flags, logical_row)

    def renumber(self, ren, kv_ren=None):
        """the same term inside a launch that holds only a SUBSET of the physical rows (`ren`: physical row -> row of that launch;
        `kv_ren`: the same for the K / V row where the launch's K / V tensors are not row-aligned with its Q tensor)"""
        kv_ren = ren if kv_ren is None else kv_ren
        if self.q_row not in ren or self.kv_row not in kv_ren:
            raise ValueError(f"attention term (q row {self.q_row}, kv row {self.kv_row}) reaches outside the rows of this phase {sorted(ren)} / {sorted(kv_ren)}")
        return AttnEntrySpec(ren[self.q_row], kv_ren[self.kv_row], self.w_const, self.w_slope, self.wq, self.kmask, self.qsel, self.flags, self.hr_row)

    def shifted(self, base, logical_row, kv_base=None):
        """the same term inside an image-batched launch: this image's physical rows start at `base` (its K / V rows at `kv_base`
        where they differ: cross attention of the composition hook, whose text batch has more rows than the latent batch); the
        tiled-head rule (attention.py:859 vs 761) keeps using the row index the image would have had in its own batch"""
        return AttnEntrySpec(self.q_row + base, self.kv_row + (base if kv_base is None else kv_base), self.w_const, self.w_slope, self.wq,
                             self.kmask, self.qsel, self.flags, logical_row if self.hr_row is None else self.hr_row)


def _set_entries(d, passes, b0, nb, ptr=_p):
    """the (pass, row) entries of descriptor d from rows b0 .. b0 + nb of `passes` (ptr: tensor -> address)"""
    for p, rows in enumerate(passes):
        for b in range(nb):
            sp = rows[b0 + b]
            e = d.e[p * L.ATT_MAXB + b]
            if sp is None:
                e.w_const = e.w_slope = 0.0
                continue
            e.q_row, e.kv_row, e.w_const, e.w_slope = sp.q_row, sp.kv_row, sp.w_const, sp.w_slope
            e.wq, e.kmask, e.qsel, e.flags = ptr(sp.wq), ptr(sp.kmask), ptr(sp.qsel), sp.flags
            # the tiled-head rule defaults to the OUTPUT row index, which a row-range launch shifts by b0: pin it
            hr = sp.hr_row if sp.hr_row is not None else (b0 + b if b0 else None)
            e.hr_row = 0 if hr is None else hr + 1


def _takes_kv_images(lib, d):
    """whether the library runs split-bf16 descriptor d on pre-split K / V^T images (kv_pair = 1): it names a kernel instead of refusing"""
    probe = L.AttnDesc.from_buffer_copy(d)
    probe.kv_pair = 1
    return lib.ffn_attn_kernel_name(L.FFN_BF16X3, CT.byref(probe), CT.create_string_buffer(160), 160) == 0


def kv_images_ok(Dh, S, Sk, passes=None, nbytes=0):
    """split-bf16 self attention whose K / V^T projections may write the attention kernel's pre-split images themselves (linear(kv64_from=...),
    attention(kv_images=True)): the library takes the plan's launches on the images (asked with probe descriptors: the kernel choice depends on the
    shapes and on which entries are active, masked or flagged), and the buffers are within the kernels' 32-bit byte offsets (nbytes = the larger of
    the K and V^T buffers)"""
    if not (_ATTN_PRESPLIT and nbytes < 2 ** 31 - 65536):
        return False
    lib = L.load()
    passes = passes or [[AttnEntrySpec(0, 0)]]
    Bo = len(passes[0])
    for b0 in range(0, Bo, L.ATT_MAXB):
        nb = min(L.ATT_MAXB, Bo - b0)
        d = L.AttnDesc()
        d.Bo, d.S, d.Sk, d.heads, d.D, d.npass = nb, S, Sk, 1, Dh, len(passes)
        d.ldq = d.ldk = d.ldo = Dh
        d.ldvt = Sk
        d.w_dev = 1                          # (a blend scalar is assumed present: the stricter answer for the short-key kernels)
        _set_entries(d, passes, b0, nb, lambda t: 0 if t is None else 1)
        if not _takes_kv_images(lib, d):
            return False
    return True


_CUS = {}


def attn_row_split(Bo, wg_per_row, maxb, cus):
    """output rows per launch of a self-attention call on the one-workgroup-per-CU kernels (attn_x3w / attn_x3p / attn_pp: a (row, head, 256-query block)
    workgroup each, `cus` of them resident at a time): the uniform chunk n <= maxb that minimises the number of resident ROUNDS
    sum_i ceil(n_i * wg_per_row / cus) over the call's launches (launches of one stream do not overlap: every launch pays its own partly filled last
    round); ties go to the larger chunk (fewer launches).  72 rows: S = 4096, 5 heads (80 workgroups per row) 16 + 16 + 16 + 16 + 8 = 23 rounds (as
    before); S = 1024, 10 heads (40 per row) 6 x 12 = 12 rounds instead of 14; S = 256, 20 heads (20 per row) 6 x 12 = 6 rounds instead of 9."""
    best_n, best = min(maxb, Bo), None
    for n in range(min(maxb, Bo), 0, -1):
        full, rest = divmod(Bo, n)
        rounds = full * -(-n * wg_per_row // cus) + (-(-rest * wg_per_row // cus) if rest else 0)
        if best is None or rounds < best:
            best_n, best = n, rounds
    return best_n


def attention(q, k, vt, heads, scale, passes=None, *, Sk=None, out=None, w_dev=None, Bo=None, C=None, x3=False, out_pair=False, kv_images=False, causal=False):
    """q: [Bq,S,C]; k: [Bk,Sk,C]; vt: [Bk,C,ldvt] (V transposed).  passes: list (per pass) of lists (per output
    row) of AttnEntrySpec or None (= skipped).  passes=None -> plain attention, row b uses its own K/V.
    More than FFN_ATT_MAXB output rows are issued as several launches over row ranges (entries name absolute Q/KV rows).
    kv_images (split-bf16 self attention): k / vt already ARE the pre-split images (written by their projections with kv64_from: fp32-typed tensors of
    the shapes above whose bytes hold [hi(64) | lo(64)] blocks); the launches run with kv_pair = 1 and no ffn_attn_presplit pass.
    causal: every term carries FFN_ATT_CAUSAL (key k allowed for query q iff k <= q; S == Sk <= 96, head dim 64, one pass of plain terms)."""
    lib = L.load()
    Bq, S, _ = q.shape
    Cq = C if C is not None else q.shape[2]          # q / k may be column views of a wider [B,S,ld] buffer
    Sk = Sk if Sk is not None else k.shape[1]
    Dh = Cq // heads
    if passes is None:
        passes = [[AttnEntrySpec(b, b) for b in range(Bq)]]
    if causal:
        passes = [[None if sp is None else AttnEntrySpec(sp.q_row, sp.kv_row, sp.w_const, sp.w_slope, sp.wq, sp.kmask, sp.qsel, sp.flags | L.ATT_CAUSAL, sp.hr_row)
                   for sp in rows] for rows in passes]
    Bo = Bo if Bo is not None else len(passes[0])
    out_pair = bool(out_pair and x3 and q.dtype == torch.float32 and Dh <= 64 and out is None and Cq % 8 == 0)
    if out_pair:                                     # the result as pair rows for the to_out projection's split-bf16 GEMM
        out = _mark_pair(torch.empty(Bo, S, 2 * Cq, dtype=torch.bfloat16, device=q.device), Cq)
    if out is None:
        out = torch.empty(Bo, S, Cq, dtype=q.dtype, device=q.device)
    for rows in passes:
        assert len(rows) == Bo
    esz = q.element_size()
    dcode = L.FFN_BF16X3 if (x3 and q.dtype == torch.float32) else _dt(q)      # split-bf16 arithmetic on fp32 operands
    descs = []
    chunk = L.ATT_MAXB
    if Bo > 1 and Dh == 64 and S >= 128 and Sk % 64 == 0 and q.is_cuda:      # the 256-queries-per-workgroup, one-workgroup-per-CU kernels
        di = q.device.index if q.device.index is not None else torch.cuda.current_device()
        if di not in _CUS:
            _CUS[di] = torch.cuda.get_device_properties(di).multi_processor_count
        chunk = attn_row_split(Bo, heads * -(-S // 256), L.ATT_MAXB, _CUS[di])
    for b0 in range(0, Bo, chunk):
        nb = min(chunk, Bo - b0)
        d = L.AttnDesc()
        d.q, d.k, d.vt, d.w_dev = q.data_ptr(), k.data_ptr(), vt.data_ptr(), _p(w_dev)
        d.out = out.data_ptr() + b0 * S * Cq * esz       # (pair rows: 2 Cq bf16 = Cq fp32 worth of bytes)
        d.Bo, d.S, d.Sk, d.heads, d.D = nb, S, Sk, heads, Dh
        d.ldq, d.ldk, d.ldvt, d.ldo = q.stride(1), k.stride(1), vt.stride(1), (2 * Cq if out_pair else Cq)
        d.out_pair = 1 if out_pair else 0
        d.scale, d.npass = scale, len(passes)
        d.kv_pair = 1 if kv_images else 0
        _set_entries(d, passes, b0, nb)
        descs.append((b0, nb, d))
    # split-bf16 self attention: K / V^T are split ONCE per call into the bf16 images attn_x3w_kernel stages by LDS-DMA (ffn_attn_presplit) where the
    # library runs the launches on them; otherwise attn_x3p_kernel's 16 query-block workgroups per (row, head) each split the whole K / V^T in their key loops
    # (the images are addressed with 32-bit byte offsets: K / V^T beyond 2 GiB keep the in-kernel split instead of failing in ffn_attn)
    if kv_images:
        assert dcode == L.FFN_BF16X3 and kv_images_ok(Dh, S, Sk)
    elif dcode == L.FFN_BF16X3 and _ATTN_PRESPLIT and k.stride(2) == 1 and vt.stride(2) == 1 and k.stride(0) == Sk * k.stride(1) \
            and vt.stride(0) == heads * Dh * vt.stride(1) and k.shape[0] * Sk * heads * Dh * 4 < 2 ** 31 - 65536:
        if all(_takes_kv_images(lib, d) for _, _, d in descs):
            Bk = k.shape[0]
            kp = torch.empty(Bk, Sk, 2 * heads * Dh, dtype=torch.bfloat16, device=q.device)
            vp = torch.empty(Bk, heads * Dh, 2 * Sk, dtype=torch.bfloat16, device=q.device)
            L.check(_timed("attn_presplit_kernel", 0.0, 16.0 * Bk * Sk * heads * Dh,
                           lambda: lib.ffn_attn_presplit(_stream(), k.data_ptr(), vt.data_ptr(), kp.data_ptr(), vp.data_ptr(), Bk, Sk, heads, k.stride(1), vt.stride(1))),
                    "ffn_attn_presplit")
            for _, _, d in descs:
                d.k, d.vt, d.kv_pair = kp.data_ptr(), vp.data_ptr(), 1
                d.ldk, d.ldvt = heads * Dh, Sk              # compact images: the strides of the fp32 tensors they replace
    for b0, nb, d in descs:
        if _PROF is None:
            L.check(lib.ffn_attn(_stream(), dcode, CT.byref(d)), "ffn_attn")
        else:
            nterms = sum(1 for rows in passes for sp in rows[b0:b0 + nb] if sp is not None and (sp.w_const != 0.0 or sp.w_slope != 0.0))
            nbuf = CT.create_string_buffer(160)
            lib.ffn_attn_kernel_name(dcode, CT.byref(d), nbuf, 160)
            L.check(_timed(nbuf.value.decode(), 4.0 * nterms * S * Sk * Cq,
                           esz * nterms * (S * Cq + 2 * Sk * Cq) + esz * nb * S * Cq,
                           lambda: lib.ffn_attn(_stream(), dcode, CT.byref(d))), "ffn_attn")
    return out


# ---------------------------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------------------------
def gn_workspace(B, HW, C, device):
    lib = L.load()
    nchunk = lib.ffn_gn_nchunk(HW)
    return (torch.empty(B * nchunk * 2 * C, dtype=torch.float32, device=device),
            torch.empty(B, C, dtype=torch.float32, device=device), torch.empty(B, C, dtype=torch.float32, device=device))


def groupnorm(x, gamma, beta, G, eps, silu=False, out=None, ws=None, pair=False):
    """x: [B, HW, C].  One fused launch for slices <= 131072 elements per (batch, group), else stats + apply.
    pair (fp32 x): the result as the bf16 pair rows [B, HW, 2C] an FFN_BF16X3 GEMM reads."""
    lib = L.load()
    B, HW, Cc = x.shape
    if pair:
        assert x.dtype == torch.float32 and out is None
        out = _mark_pair(torch.empty(B, HW, 2 * Cc, dtype=torch.bfloat16, device=x.device), Cc)
    if out is None:
        out = torch.empty_like(x)
    nb = B
    if _invariant() and lib.ffn_gn_fused(1, HW, Cc, G) and not lib.ffn_gn_fused(B, HW, Cc, G):
        while not lib.ffn_gn_fused(nb, HW, Cc, G):   # batch_invariant: the form of one row, in chunks of rows that keep the fused kernel
            nb = (nb + 1) // 2
    if lib.ffn_gn_fused(nb, HW, Cc, G):
        partial = scale = shift = None
    else:
        partial, scale, shift = ws if ws is not None else gn_workspace(B, HW, Cc, x.device)
    fl = (L.NORM_SILU if silu else 0) | (L.NORM_OUT_PAIR if pair else 0)
    def call():
        rc = 0
        for b0 in range(0, B, nb):
            n = min(nb, B - b0)
            rc = lib.ffn_groupnorm(_stream(), _dt(x), x.data_ptr() + b0 * HW * Cc * x.element_size(), out.data_ptr() + b0 * HW * out.shape[-1] * out.element_size(),
                                   gamma.data_ptr(), beta.data_ptr(), n, HW, Cc, G, eps, fl, _p(partial), _p(scale), _p(shift))
            if rc:
                break
        return rc
    if _PROF is None:
        L.check(call(), "ffn_groupnorm")
    else:       # algorithmic bytes: one read + one write (the three-launch form reads x twice: that shows as a lower GB/s)
        name = f"gn_fused_kernel<{_tname(x)}>" if partial is None else f"gn_partial+gn_finalize+gn_apply<{_tname(x)}>"
        L.check(_timed(name, 0.0, 2.0 * x.numel() * x.element_size(), call), "ffn_groupnorm")
    return out


def groupnorm_pair_raw(x, gamma, beta, G, eps, silu=False, ws=None):
    """split-bf16 mode, ResBlock with a 1x1 shortcut: (pair rows of act(GroupNorm(x)), pair rows of x itself) from ONE apply pass over x (ffn_groupnorm_pair_raw) --
    the second is what split_pair(x) would give, bit for bit.  Shapes the one-launch fused GroupNorm takes (small tensors) keep that kernel + a split_pair pass."""
    lib = L.load()
    B, HW, Cc = x.shape
    if Cc % 8 != 0 or lib.ffn_gn_fused(1 if _invariant() else B, HW, Cc, G) or not x.is_contiguous():
        return groupnorm(x, gamma, beta, G, eps, silu=silu, pair=True, ws=ws), split_pair(x, Cc)
    assert x.dtype == torch.float32
    y = _mark_pair(torch.empty(B, HW, 2 * Cc, dtype=torch.bfloat16, device=x.device), Cc)
    yr = _mark_pair(torch.empty(B, HW, 2 * Cc, dtype=torch.bfloat16, device=x.device), Cc)
    partial, scale, shift = ws if ws is not None else gn_workspace(B, HW, Cc, x.device)
    call = lambda: lib.ffn_groupnorm_pair_raw(_stream(), x.data_ptr(), y.data_ptr(), yr.data_ptr(), gamma.data_ptr(), beta.data_ptr(), B, HW, Cc, G, eps,
                                              L.NORM_SILU if silu else 0, _p(partial), _p(scale), _p(shift))
    if _PROF is None:
        L.check(call(), "ffn_groupnorm_pair_raw")
    else:       # algorithmic bytes: one read + two writes
        L.check(_timed("gn_partial+gn_finalize+gn_apply<float> (+ raw pair)", 0.0, 3.0 * x.numel() * x.element_size(), call), "ffn_groupnorm_pair_raw")
    return y, yr


def layernorm(x, gamma, beta, eps=1e-5, out=None, pair=False):
    lib = L.load()
    Cc = x.shape[-1]
    M = x.numel() // Cc
    if pair:
        assert x.dtype == torch.float32 and out is None
        out = _mark_pair(torch.empty(*x.shape[:-1], 2 * Cc, dtype=torch.bfloat16, device=x.device), Cc)
        call = lambda: lib.ffn_layernorm_pair(_stream(), x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), M, Cc, eps)
    else:
        if out is None:
            out = torch.empty_like(x)
        call = lambda: lib.ffn_layernorm(_stream(), _dt(x), x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), M, Cc, eps)
    if _PROF is None:
        L.check(call(), "ffn_layernorm")
    else:
        L.check(_timed(f"layernorm_kernel<{_tname(x)}>", 0.0, 2.0 * x.numel() * x.element_size(), call), "ffn_layernorm")
    return out


def pool_layernorm(x, ids, gamma, beta, eps=1e-5, out=None, pair=False):
    """LayerNorm of one row per sequence of x [N, S, C] -> [N, C] (pair: the pair rows [N, 2C], fp32 x only): row 0 (ids None: a ViT's class token) or the first
    position holding the sequence's largest id (ids int32 [N, S] on the device, S <= 96: open_clip's text pooling).  ffn_layernorm's routine on the gathered
    row, bit for bit (ffn_pool_layernorm)."""
    lib = L.load()
    assert x.ndim == 3 and x.is_contiguous()
    N, S, Cc = x.shape
    if ids is not None:
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (N, S) and ids.is_contiguous() and ids.device == x.device
    if pair:
        assert x.dtype == torch.float32
        if out is None:
            out = torch.empty(N, 2 * Cc, dtype=torch.bfloat16, device=x.device)
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (N, 2 * Cc) and out.is_contiguous()
        out = _mark_pair(out, Cc)
    elif out is None:
        out = torch.empty(N, Cc, dtype=x.dtype, device=x.device)
    else:
        assert out.dtype == x.dtype and tuple(out.shape) == (N, Cc) and out.is_contiguous()
    L.check(_timed(f"pool_layernorm_kernel<{_tname(x)}>", 0.0, 2.0 * N * Cc * x.element_size(),
                   lambda: lib.ffn_pool_layernorm(_stream(), _dt(x), x.data_ptr(), _p(ids), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), N, S, Cc, eps,
                                                  int(pair))), "ffn_pool_layernorm")
    return out


def cosine_rows(a, b, out=None):
    """a fp32 [B, P], b fp32 [B, P] or [1, P] -> fp32 [B]: <a_i, b_i> / (max(|a_i|, 1e-12) max(|b_i|, 1e-12)), the cosine of F.normalize'd rows
    (ffn_cosine_rows; deterministic)"""
    lib = L.load()
    assert a.dtype == b.dtype == torch.float32 and a.ndim == b.ndim == 2 and a.is_contiguous() and b.is_contiguous() and a.device == b.device
    B, P = a.shape
    assert b.shape[1] == P
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=a.device)
    else:
        assert out.dtype == torch.float32 and tuple(out.shape) == (B,) and out.is_contiguous()
    L.check(_timed("cosine_rows_kernel", 6.0 * B * P, 4.0 * (B * P + b.shape[0] * P + B),
                   lambda: lib.ffn_cosine_rows(_stream(), a.data_ptr(), b.data_ptr(), out.data_ptr(), B, P, b.shape[0])), "ffn_cosine_rows")
    return out


def softmax_rows(x, scale=1.0, out=None):
    lib = L.load()
    N = x.shape[-1]
    M = x.numel() // N
    if out is None:
        out = torch.empty_like(x)
    L.check(_timed(f"softmax_rows_kernel<{_tname(x)}>", 0.0, 2.0 * x.numel() * x.element_size(),
                   lambda: lib.ffn_softmax_rows(_stream(), _dt(x), x.data_ptr(), out.data_ptr(), M, N, scale)), "ffn_softmax_rows")
    return out


# ---------------------------------------------------------------------------------------------------------------
# scheduler / guidance (fp32 NCHW, like the reference)
# ---------------------------------------------------------------------------------------------------------------
def cfg_masked(eps_u, eps_c, mask_f, cfg, out=None):
    lib = L.load()
    if out is None:
        out = torch.empty_like(eps_u)
    HW = eps_u.shape[-1] * eps_u.shape[-2]
    L.check(_timed("cfg_masked_kernel", 0.0, 12.0 * eps_u.numel(),
                   lambda: lib.ffn_cfg_masked(_stream(), eps_u.data_ptr(), eps_c.data_ptr(), _p(mask_f), float(cfg), out.data_ptr(),
                                              eps_u.numel(), HW)), "ffn_cfg_masked")
    return out


def ddim_inv_step(eps, x, c_bt, c_at, c_an, c_bn, want_pred_x0=False):
    lib = L.load()
    x_next = torch.empty_like(x)
    p0 = torch.empty_like(x) if want_pred_x0 else None
    L.check(_timed("ddim_inv_step_kernel", 0.0, (12.0 + (4.0 if want_pred_x0 else 0.0)) * x.numel(),
                   lambda: lib.ffn_ddim_inv_step(_stream(), eps.data_ptr(), x.data_ptr(), c_bt, c_at, c_an, c_bn, x_next.data_ptr(), _p(p0),
                                                 x.numel())), "ffn_ddim_inv_step")
    return x_next, p0


def ddim_ctrl_step(eps, x, noise, m_f, om_f, c_bt, c_at, c_ap, c_dir, c_dirm, stdv, row_masked, want_pred_x0=False):
    lib = L.load()
    rows = x.shape[0]
    d = L.CtrlStepDesc()
    x_prev = torch.empty_like(x)
    p0 = torch.empty_like(x) if want_pred_x0 else None
    d.eps, d.x, d.noise, d.m, d.om = eps.data_ptr(), x.data_ptr(), _p(noise), m_f.data_ptr(), om_f.data_ptr()
    d.x_prev, d.pred_x0 = x_prev.data_ptr(), _p(p0)
    d.c_bt, d.c_at, d.c_ap, d.c_dir = c_bt, c_at, c_ap, c_dir
    for b in range(rows):
        d.c_dirm[b], d.stdv[b], d.row_masked[b] = c_dirm[b], stdv[b], int(row_masked[b])
    d.rows, d.CHW, d.HW = rows, x[0].numel(), x.shape[-1] * x.shape[-2]
    L.check(_timed("ddim_ctrl_step_kernel", 0.0, 20.0 * x.numel(), lambda: lib.ffn_ddim_ctrl_step(_stream(), CT.byref(d))), "ffn_ddim_ctrl_step")
    return x_prev, p0


# ---------------------------------------------------------------------------------------------------------------
# layout / misc
# ---------------------------------------------------------------------------------------------------------------
def pack_nchw(src, src_rows, CP, dtype, out=None):
    """fp32 NCHW [Bs,Cl,H,W] -> dtype NHWC [len(src_rows), HW, CP]."""
    lib = L.load()
    Bs, Cl, H, W = src.shape
    B = len(src_rows)
    if out is None:
        out = torch.empty(B, H * W, CP, dtype=dtype, device=src.device)
    for b0 in range(0, B, 16):                     # the descriptor names up to 16 source rows per launch
        nb = min(16, B - b0)
        d = L.PackDesc()
        d.src, d.dst = src.data_ptr(), out.data_ptr() + b0 * H * W * CP * out.element_size()
        for i in range(nb):
            d.src_row[i] = src_rows[b0 + i]
        d.B, d.Cl, d.CP, d.HW = nb, Cl, CP, H * W
        L.check(_timed(f"pack_nchw_kernel<{_tname(out)}>", 0.0, nb * H * W * (4.0 * Cl + CP * out.element_size()),
                       lambda: lib.ffn_pack_nchw(_stream(), _dt(out), CT.byref(d))), "ffn_pack_nchw")
    return out


def nhwc_to_nchw_f32(src, C_, H, W, out=None):
    lib = L.load()
    B, HW, ld = src.shape
    if out is None:
        out = torch.empty(B, C_, H, W, dtype=torch.float32, device=src.device)
    L.check(_timed("nhwc_to_nchw_f32_kernel", 0.0, 8.0 * B * HW * C_,
                   lambda: lib.ffn_nhwc_to_nchw_f32(_stream(), src.data_ptr(), out.data_ptr(), B, HW, C_, ld)), "ffn_nhwc_to_nchw_f32")
    return out


def concat(a, b, out=None):
    """[a | b] along the channel axis.  If `a` is the left column view of a cat_dst() buffer (its producer already wrote it in place),
    only b is copied and that buffer is returned."""
    lib = L.load()
    C1, C2 = a.shape[-1], b.shape[-1]
    rows = a.numel() // C1
    base = getattr(a, "_ffn_cat_base", None)
    if out is None and base is not None and base.shape[-1] == C1 + C2:
        L.check(_timed(f"concat_kernel<{_tname(b)}>", 0.0, 2.0 * rows * C2 * b.element_size(),
                       lambda: lib.ffn_concat(_stream(), _dt(b), None, b.data_ptr(), base.data_ptr(), rows, C1, C2)), "ffn_concat")
        return base
    if base is not None:
        a = a.contiguous()
    if out is None:
        out = torch.empty(*a.shape[:-1], C1 + C2, dtype=a.dtype, device=a.device)
    L.check(_timed(f"concat_kernel<{_tname(a)}>", 0.0, 2.0 * rows * (C1 + C2) * a.element_size(),
                   lambda: lib.ffn_concat(_stream(), _dt(a), a.data_ptr(), b.data_ptr(), out.data_ptr(), rows, C1, C2)), "ffn_concat")
    return out


def cat_dst(shape_lead, C1, C2, dtype, device):
    """Destination for a producer whose output will be concatenated with C2 more channels: a [*, C1 + C2] buffer and its left
    [*, C1] column view (pass the view as `out=` to linear / conv3x3; concat(view, skip) then only copies the skip)."""
    base = torch.empty(*shape_lead, C1 + C2, dtype=dtype, device=device)
    view = base[..., :C1]
    view._ffn_cat_base = base
    return view


def timestep_freqs(dim, device, max_period=10000.0, shift=0.0):
    half = dim // 2
    exponent = -math.log(max_period) * torch.arange(half, dtype=torch.float32) / (half - shift)
    return torch.exp(exponent).to(device)


def timestep_embed(t_dev, freq, B, dtype, flip=True, out=None):
    lib = L.load()
    half = freq.numel()
    if out is None:
        out = torch.empty(B, 2 * half, dtype=dtype, device=freq.device)
    L.check(_timed(f"timestep_embed_kernel<{_tname(out)}>", 0.0, float(out.numel() * out.element_size()),
                   lambda: lib.ffn_timestep_embed(_stream(), _dt(out), t_dev.data_ptr(), freq.data_ptr(), out.data_ptr(), B, half,
                                                  1 if flip else 0)), "ffn_timestep_embed")
    return out


def transpose(src, ld_dst=None, out=None):
    """[B,R,C] -> [B,C,ld_dst] (first R columns written)."""
    lib = L.load()
    B, R, Cc = src.shape
    ld_dst = ld_dst or R
    if out is None:
        out = torch.zeros(B, Cc, ld_dst, dtype=src.dtype, device=src.device)
    L.check(_timed(f"transpose_kernel<{_tname(src)}>", 0.0, 2.0 * src.numel() * src.element_size(),
                   lambda: lib.ffn_transpose(_stream(), _dt(src), src.data_ptr(), out.data_ptr(), B, R, Cc, Cc, ld_dst)), "ffn_transpose")
    return out


def cast(src, dtype, out=None):
    lib = L.load()
    if out is None:
        out = torch.empty(src.shape, dtype=dtype, device=src.device)
    L.check(_timed(f"cast_kernel<{_tname(src)}, {_tname(out)}>", 0.0, float(src.numel() * (src.element_size() + out.element_size())),
                   lambda: lib.ffn_cast(_stream(), _dt(src), _dt(out), src.data_ptr(), out.data_ptr(), src.numel())), "ffn_cast")
    return out


def relu(x, out=None):
    """max(x, 0) (fp32 / bf16, numel % 4 == 0)"""
    lib = L.load()
    out = torch.empty_like(x) if out is None else out
    L.check(_timed("eltwise_kernel<relu>", 0.0, 2.0 * x.numel() * x.element_size(),
                   lambda: lib.ffn_eltwise(_stream(), _dt(x), L.ELT_RELU, x.data_ptr(), None, out.data_ptr(), x.numel())), "ffn_eltwise")
    return out


def gelu(x, out=None):
    """x (1 + erf(x / sqrt 2)) / 2 (fp32 / bf16, numel % 4 == 0)"""
    lib = L.load()
    out = torch.empty_like(x) if out is None else out
    L.check(_timed("eltwise_kernel<gelu>", 0.0, 2.0 * x.numel() * x.element_size(),
                   lambda: lib.ffn_eltwise(_stream(), _dt(x), L.ELT_GELU, x.data_ptr(), None, out.data_ptr(), x.numel())), "ffn_eltwise")
    return out


def add(a, b, out=None):
    """a + b (same shape and dtype, contiguous)"""
    lib = L.load()
    assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
    out = torch.empty_like(a) if out is None else out
    L.check(_timed("eltwise_kernel<add>", 0.0, 3.0 * a.numel() * a.element_size(),
                   lambda: lib.ffn_eltwise(_stream(), _dt(a), L.ELT_ADD, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel())), "ffn_eltwise")
    return out


def resize_bilinear(x, B, Hin, Win, Hout, Wout, relu=False):
    """x: [B, Hin*Win, C] NHWC -> [B, Hout*Wout, C]; torch's bilinear interpolation with align_corners=True"""
    lib = L.load()
    C_ = x.shape[-1]
    assert x.is_contiguous() and x.numel() == B * Hin * Win * C_
    out = torch.empty(B, Hout * Wout, C_, dtype=x.dtype, device=x.device)
    L.check(_timed("resize_bilinear_kernel", 0.0, (x.numel() + out.numel()) * x.element_size(),
                   lambda: lib.ffn_resize_bilinear(_stream(), _dt(x), x.data_ptr(), out.data_ptr(), B, Hin, Win, Hout, Wout, C_, 1 if relu else 0)),
            "ffn_resize_bilinear")
    return out


def embed_tokens(ids, table, pos, dtype, out=None):
    """ids int32 [N, S] (device), table fp32 [V, C], pos fp32 [>= S, C] -> [N, S, C] of `dtype`: table[ids] + pos, added in fp32 (ffn_embed_tokens).
    The caller has checked 0 <= id < V on the host."""
    lib = L.load()
    assert ids.dtype == torch.int32 and ids.is_contiguous() and table.dtype == pos.dtype == torch.float32 and table.is_contiguous() and pos.is_contiguous()
    N, S = ids.shape
    V, C = table.shape
    assert pos.shape[0] >= S and pos.shape[1] == C
    if out is None:
        out = torch.empty(N, S, C, dtype=dtype, device=ids.device)
    call = lambda: lib.ffn_embed_tokens(_stream(), _dt(out), ids.data_ptr(), table.data_ptr(), pos.data_ptr(), out.data_ptr(), N * S, S, C, V)
    if _PROF is None:
        L.check(call(), "ffn_embed_tokens")
    else:
        L.check(_timed(f"embed_tokens_kernel<{_tname(out)}>", 0.0, (4.0 + out.element_size()) * out.numel(), call), "ffn_embed_tokens")
    return out


def embed_tokens_ln(ids, table, pos, gamma, beta, dtype, eps=1e-12, out=None):
    """ids int32 [N, S] (device), table fp32 [V, C], pos fp32 [>= S, C], gamma / beta fp32 [C] -> [N, S, C] of `dtype`: LayerNorm(table[ids] + pos), the sum and
    the norm in fp32 (ffn_embed_tokens_ln: BERT's embedding; the fp32 result has the bits of layernorm(embed_tokens(..., float32))).  The caller has checked
    0 <= id < V on the host."""
    lib = L.load()
    assert ids.dtype == torch.int32 and ids.is_contiguous() and table.dtype == pos.dtype == torch.float32 and table.is_contiguous() and pos.is_contiguous()
    N, S = ids.shape
    V, C = table.shape
    assert pos.shape[0] >= S and pos.shape[1] == C
    assert gamma.dtype == beta.dtype == torch.float32 and tuple(gamma.shape) == tuple(beta.shape) == (C,) and gamma.is_contiguous() and beta.is_contiguous()
    if out is None:
        out = torch.empty(N, S, C, dtype=dtype, device=ids.device)
    else:
        assert out.dtype == dtype and tuple(out.shape) == (N, S, C) and out.is_contiguous()
    L.check(_timed(f"embed_tokens_ln_kernel<{_tname(out)}>", 0.0, (8.0 + out.element_size()) * out.numel(),
                   lambda: lib.ffn_embed_tokens_ln(_stream(), _dt(out), ids.data_ptr(), table.data_ptr(), pos.data_ptr(), out.data_ptr(), gamma.data_ptr(),
                                                   beta.data_ptr(), N * S, S, C, V, eps)), "ffn_embed_tokens_ln")
    return out


def affine_chain_params(layers):
    """[(W [n, k], b [n]), ...] fp32 -> (the packed parameter buffer of ffn_affine_chain: W_1, b_1, W_2, b_2 ... back to back, the widths [k_1, n_1, n_2 ...])"""
    dims = [layers[0][0].shape[1]]
    for w, b in layers:
        assert w.ndim == 2 and w.shape[1] == dims[-1] and tuple(b.shape) == (w.shape[0],), "affine_chain: layer widths do not chain"
        dims.append(w.shape[0])
    return torch.cat([t.detach().float().reshape(-1) for w, b in layers for t in (w, b)]).contiguous(), dims


def affine_chain(x, params, dims, shift=0.0, scale=1.0, ldx=None, B=None, out=None):
    """x fp32: B rows of dims[0] values, row b at x.data_ptr() + 4 b ldx (default: the rows of a contiguous [B, dims[0]] tensor; ldx = S * C with x [B, S, C] reads
    row 0 of every sequence); params: affine_chain_params' buffer on x's device -> fp32 [B, dims[-1]]: the layers one after the other, then (y - shift) / scale
    (ffn_affine_chain; deterministic)."""
    lib = L.load()
    dims = [int(d) for d in dims]
    nl = len(dims) - 1
    assert x.dtype == params.dtype == torch.float32 and x.is_contiguous() and params.is_contiguous() and x.device == params.device
    if ldx is None:
        assert x.ndim == 2 and x.shape[1] == dims[0]
        ldx, B = dims[0], x.shape[0]
    assert B is not None and B > 0 and (B - 1) * ldx + dims[0] <= x.numel(), "affine_chain: rows reach outside x"
    assert params.numel() == sum(dims[i + 1] * (dims[i] + 1) for i in range(nl)), "affine_chain: params do not hold the layers of dims"
    if out is None:
        out = torch.empty(B, dims[-1], dtype=torch.float32, device=x.device)
    else:
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, dims[-1]) and out.is_contiguous()
    cd = (CT.c_int * len(dims))(*dims)
    macs = sum(dims[i + 1] * dims[i] for i in range(nl))
    L.check(_timed("affine_chain_kernel", 2.0 * B * macs, 4.0 * (B * (dims[0] + dims[-1]) + params.numel()),
                   lambda: lib.ffn_affine_chain(_stream(), x.data_ptr(), params.data_ptr(), out.data_ptr(), B, ldx, cd, nl, shift, scale)), "ffn_affine_chain")
    return out


_DIFT_WS = {}


def dift_match(rows_src, rows_tgt, hw, HW, kps):
    """The correspondence search of the Mean Distance metric (ffn_dift_match; csrc/dift_match.h).  rows_src / rows_tgt: DIFT activation rows [E, h*w, C] of the
    source and the edited image (fp32 or bf16; rows may be strided, rows.stride(1) >= C, as HipUNet.features leaves them); hw = (h, w); HW = (H, W) the image size;
    kps: K keypoints (row, col) at image resolution, host integers.  For every keypoint: the pixel of the edited image whose bilinearly upsampled feature has
    the largest cosine with the source image's upsampled feature at the keypoint (ensemble means over E; numpy's argmax tie rule).
    -> (rc int32 [K, 2], cos float32 [K]) on the device."""
    import numpy as np
    lib = L.load()
    assert rows_src.ndim == 3 and rows_src.shape == rows_tgt.shape and rows_src.dtype == rows_tgt.dtype and rows_src.device == rows_tgt.device
    assert rows_src.stride(2) == 1 and rows_tgt.stride() == rows_src.stride(), "source and target rows share one layout"
    E, n, C = rows_src.shape
    (h, w), (H, W) = hw, HW
    assert n == h * w, (n, h, w)
    kp = np.ascontiguousarray(np.asarray(kps).reshape(-1, 2), dtype=np.int32)
    K = kp.shape[0]
    key = (rows_src.device, torch.cuda.current_stream().cuda_stream, C, h, w, K)          # one buffer per stream, like the split-K scratch
    ws = _DIFT_WS.get(key)
    if ws is None:
        nbytes = lib.ffn_dift_workspace_bytes(C, h, w, K)
        if nbytes < 0:
            L.check(int(nbytes), "ffn_dift_workspace_bytes")
        if len(_DIFT_WS) > 16:
            _DIFT_WS.clear()
        ws = _DIFT_WS[key] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=rows_src.device)
    rc = torch.empty(K, 2, dtype=torch.int32, device=rows_src.device)
    cos = torch.empty(K, dtype=torch.float32, device=rows_src.device)
    d = L.DiftDesc()
    d.src, d.tgt, d.kps, d.ws, d.out_rc, d.out_cos = rows_src.data_ptr(), rows_tgt.data_ptr(), kp.ctypes.data, ws.data_ptr(), rc.data_ptr(), cos.data_ptr()
    d.ws_bytes, d.es = ws.numel() * 4, (rows_src.stride(0) if E > 1 else 0)
    d.dtype, d.E, d.C, d.ld, d.h, d.w, d.H, d.W, d.K = _dt(rows_src), E, C, rows_src.stride(1), h, w, H, W, K
    L.check(_timed("dift_match", 2.0 * (K + 5) * n * C, (2.0 * E * n * C) * rows_src.element_size(), lambda: lib.ffn_dift_match(_stream(), CT.byref(d))), "ffn_dift_match")
    return rc, cos


# ---------------------------------------------------------------------------------------------------------------
# device image preparation of the DINOv2 feature metrics (csrc/imgprep.h).  torchvision is absent here: the semantics restated below -- Resize((h, w)) of a
# PIL image = Image.resize((w, h), BILINEAR) (antialiased: the support grows with the down-scaling factor), ToTensor = float32(byte) / 255 in CHW,
# Normalize(mean, std) = (x - float32(mean)) / float32(std) in place -- are torchvision's DOCUMENTED ones, not recorded from it.  The resize is pinned to PIL
# itself (tests/test_dino_cpu.py, tests/test_dino_gpu.py).
# ---------------------------------------------------------------------------------------------------------------
_PIL_COEFFS = {}
_PIL_COEFFS_DEV = {}


def pil_bilinear_coeffs(in_size, out_size):
    """The tables of one axis of PIL's Image.resize(BILINEAR) on 8-bit images (libImaging/Resample.c: precompute_coeffs with the bilinear filter of support 1,
    normalize_coeffs_8bpc with PRECISION_BITS = 22), evaluated in float64 like PIL's C doubles.  Pure host function, cached per (in, out).
    -> (bounds int32 [out, 2] = (first source index, number of taps), coef int32 [out, ksize], ksize = 2 ceil(max(in / out, 1)) + 1; taps past the count are 0).
    An output value is clamp((2^21 + sum_x pixel[xmin + x] * coef[x]) >> 22, 0, 255); an axis whose size does not change gets the identity (one tap of 2^22).
    The tap weight is max(0, 1 - |(x + xmin - center + 0.5) * (1 / fs)|): the product with the reciprocal, as PIL's C spells it."""
    import numpy as np
    key = (int(in_size), int(out_size))
    hit = _PIL_COEFFS.get(key)
    if hit is not None:
        return hit
    n_in, n_out = key
    assert n_in >= 1 and n_out >= 1
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        n = min(n_in, int(center + support + 0.5)) - xmin
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(n, dtype=np.float64) + xmin - center + 0.5) * ss))
        tot = 0.0
        for v in w:                                           # PIL sums the weights left to right in a double
            tot += float(v)
        if tot != 0.0:
            w = w / tot
        bounds[xx] = (xmin, n)
        coef[xx, :n] = (w * float(1 << 22) + 0.5).astype(np.int64)      # weights are >= 0: int(0.5 + w 2^22) truncates like the C cast
    bounds.setflags(write=False)
    coef.setflags(write=False)
    hit = _PIL_COEFFS[key] = (bounds, coef)
    return hit


def _pil_coeffs_dev(in_size, out_size, device):
    key = (int(in_size), int(out_size), torch.device(device))
    hit = _PIL_COEFFS_DEV.get(key)
    if hit is None:
        if len(_PIL_COEFFS_DEV) > 64:
            _PIL_COEFFS_DEV.clear()
        b, k = pil_bilinear_coeffs(in_size, out_size)
        hit = _PIL_COEFFS_DEV[key] = (torch.from_numpy(b.copy()).to(device), torch.from_numpy(k.copy()).to(device), k.shape[1])
    return hit


def resize_pil_bilinear_u8(img, oh, ow, out=None, scratch=None):
    """uint8 [B, H, W, 3] (device, contiguous) -> uint8 [B, oh, ow, 3]: PIL's Image.resize((ow, oh), BILINEAR) bit for bit (ffn_resize_pil_bilinear_u8).
    H, W, oh, ow <= _lib.IMGPREP_MAX_SIDE."""
    lib = L.load()
    assert img.dtype == torch.uint8 and img.ndim == 4 and img.shape[-1] == 3 and img.is_contiguous()
    B, H, W, _ = img.shape
    hb, hk, hks = _pil_coeffs_dev(W, ow, img.device)
    vb, vk, vks = _pil_coeffs_dev(H, oh, img.device)
    if out is None:
        out = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=img.device)
    if scratch is None:
        scratch = torch.empty(B, H, ow, 3, dtype=torch.uint8, device=img.device)
    assert out.is_contiguous() and out.numel() == B * oh * ow * 3 and scratch.numel() >= B * H * ow * 3
    L.check(_timed("resize_pil_bilinear_u8", 0.0, 3.0 * B * (H * W + 2 * H * ow + oh * ow),
                   lambda: lib.ffn_resize_pil_bilinear_u8(_stream(), img.data_ptr(), out.data_ptr(), scratch.data_ptr(), B, H, W, oh, ow, hb.data_ptr(), hk.data_ptr(), hks,
                                                          vb.data_ptr(), vk.data_ptr(), vks)), "ffn_resize_pil_bilinear_u8")
    return out


# ---------------------------------------------------------------------------------------------------------------
# the general PIL resize of the consistency metrics (csrc/imgprep.h resize_win_*; evaluation/metrics/VBench/{background,subject}_consistency.py).  CLIP's
# transform is Resize(224, BICUBIC) + CenterCrop(224) of the PIL image, DINO's is torchvision Resize(224) (BILINEAR).  torchvision is absent here: the two
# size rules below (torchvision_resize_size, center_crop_window) are torchvision's DOCUMENTED ones (transforms.functional.resize with an int size: "the smaller
# edge of the image will be matched to this number", the other side int(size * long / short); center_crop: top = int(round((h - size) / 2.0)), likewise left),
# not recorded from it.  The resampling itself is pinned to PIL (tests/test_consistency_cpu.py, tests/test_consistency_gpu.py).
# ---------------------------------------------------------------------------------------------------------------
PIL_FILTERS = ("bilinear", "bicubic")
KEEP_RULES = {"sum_lt128": L.KEEP_SUM_LT128, "gt128": L.KEEP_GT128}


def _pil_bicubic(x):
    """libImaging/Resample.c bicubic_filter (a = -0.5), the C expression operation for operation in float64"""
    import numpy as np
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def pil_resample_coeffs(in_size, out_size, filter="bilinear"):
    """The tables of one axis of PIL's Image.resize on 8-bit images for `filter` in PIL_FILTERS, in the form of pil_bilinear_coeffs (which "bilinear" calls
    through to: the same arrays).  "bicubic": support 2, a = -0.5, ksize = 2 ceil(2 max(in / out, 1)) + 1, SIGNED coefficients rounded as
    normalize_coeffs_8bpc rounds them: int(-0.5 + w 2^22) for w < 0, int(0.5 + w 2^22) otherwise (the C cast truncates towards zero).  An axis whose size does
    not change gets the identity from the filter itself (bicubic(+-1) = bicubic(+-2) = 0).  Pure host function, cached."""
    import numpy as np
    if filter == "bilinear":
        return pil_bilinear_coeffs(in_size, out_size)
    if filter != "bicubic":
        raise ValueError(f"pil_resample_coeffs: filter {filter!r} (one of {PIL_FILTERS})")
    key = (int(in_size), int(out_size), filter)
    hit = _PIL_COEFFS.get(key)
    if hit is not None:
        return hit
    n_in, n_out = key[:2]
    assert n_in >= 1 and n_out >= 1
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        n = min(n_in, int(center + support + 0.5)) - xmin
        w = _pil_bicubic((np.arange(n, dtype=np.float64) + xmin - center + 0.5) * ss)
        tot = 0.0
        for v in w:                                           # PIL sums the weights left to right in a double
            tot += float(v)
        if tot != 0.0:
            w = w / tot
        bounds[xx] = (xmin, n)
        coef[xx, :n] = np.trunc(np.where(w < 0, -0.5, 0.5) + w * float(1 << 22)).astype(np.int64)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    hit = _PIL_COEFFS[key] = (bounds, coef)
    return hit


def _pil_resample_dev(in_size, out_size, filter, device):
    if filter == "bilinear":
        return _pil_coeffs_dev(in_size, out_size, device)
    key = (int(in_size), int(out_size), filter, torch.device(device))
    hit = _PIL_COEFFS_DEV.get(key)
    if hit is None:
        if len(_PIL_COEFFS_DEV) > 64:
            _PIL_COEFFS_DEV.clear()
        b, k = pil_resample_coeffs(in_size, out_size, filter)
        hit = _PIL_COEFFS_DEV[key] = (torch.from_numpy(b.copy()).to(device), torch.from_numpy(k.copy()).to(device), k.shape[1])
    return hit


def torchvision_resize_size(h, w, size):
    """(oh, ow) of torchvision's Resize(size) with an int size (its documented rule, see above): short side -> size, long side -> int(size * long / short)"""
    if h <= w:
        return size, int(size * w / h)
    return int(size * h / w), size


def center_crop_window(h, w, size):
    """(top, left, size, size) of torchvision's CenterCrop(size) on an h x w image with both sides >= size (its documented rule, see above)"""
    assert h >= size and w >= size
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0)), size, size


def resize_pil_u8(img, oh, ow, filter, crop=None, keep=None, out=None, scratch=None):
    """uint8 [B, H, W, C] with C in (1, 3), or [B, H, W] (one channel), device and contiguous -> the window `crop` = (y0, x0, ch, cw) (default: everything) of
    PIL's Image.resize((ow, oh), filter), bit for bit: uint8 [B, ch, cw, C] (or [B, ch, cw]) (ffn_resize_pil_u8).  keep = (rule, m1, m2) with rule in
    KEEP_RULES, m1 / m2 uint8 [B, H, W] on the device (m2 may be None): pixels the rule drops read as 0, the masked image is never stored.
    H, W, oh, ow <= _lib.IMGPREP_MAX_SIDE."""
    lib = L.load()
    assert img.dtype == torch.uint8 and img.ndim in (3, 4) and img.is_contiguous()
    B, H, W = img.shape[:3]
    C = 1 if img.ndim == 3 else img.shape[3]
    y0, x0, ch, cw = (0, 0, oh, ow) if crop is None else (int(v) for v in crop)
    hb, hk, hks = _pil_resample_dev(W, ow, filter, img.device)
    vb, vk, vks = _pil_resample_dev(H, oh, filter, img.device)
    if out is None:
        out = torch.empty((B, ch, cw) + tuple(img.shape[3:]), dtype=torch.uint8, device=img.device)
    if scratch is None:
        scratch = torch.empty(B * H * cw * C, dtype=torch.uint8, device=img.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == B * ch * cw * C and scratch.dtype == torch.uint8 and scratch.numel() >= B * H * cw * C
    d = L.ResizePilDesc()
    d.src, d.dst, d.scratch = img.data_ptr(), out.data_ptr(), scratch.data_ptr()
    d.hbounds, d.hcoef, d.vbounds, d.vcoef = hb.data_ptr(), hk.data_ptr(), vb.data_ptr(), vk.data_ptr()
    d.B, d.H, d.W, d.C, d.oh, d.ow, d.hksize, d.vksize = B, H, W, C, oh, ow, hks, vks
    d.y0, d.x0, d.ch, d.cw = y0, x0, ch, cw
    d.rule = L.KEEP_NONE
    if keep is not None:
        rule, m1, m2 = keep
        for m in (m1, m2):
            assert m is None or (m.dtype == torch.uint8 and tuple(m.shape) == (B, H, W) and m.is_contiguous() and m.device == img.device)
        d.rule, d.m1, d.m2 = KEEP_RULES[rule], m1.data_ptr(), (None if m2 is None else m2.data_ptr())
    L.check(_timed("resize_pil_u8", 0.0, float(C) * B * (H * W + 2 * H * cw + ch * cw), lambda: lib.ffn_resize_pil_u8(_stream(), CT.byref(d))), "ffn_resize_pil_u8")
    return out


# ---------------------------------------------------------------------------------------------------------------
# device case preparation of the GeoBench harness (csrc/caseprep.h): the cv2 restatements of src/utils/vis_utils.py, byte for byte what the numpy functions
# give.  Like them, the interpolating paths are pinned to the numpy restatement, not to OpenCV.  Tables are built on the host in float64.
# ---------------------------------------------------------------------------------------------------------------
def lanczos4_taps(n_dst, n_src):
    """(idx int32 [n_dst, 8], wgt float64 [n_dst, 8]): the taps of cv2's INTER_LANCZOS4 exactly as src.utils.vis_utils._lanczos4_matrix computes them before it
    scatters them into a dense matrix -- 8 taps around floor(x), x = (d + 0.5) * scale - 0.5, kernel sinc(t) sinc(t / 4), normalised, indices clamped."""
    import numpy as np
    scale = n_src / n_dst
    x = (np.arange(n_dst) + 0.5) * scale - 0.5
    x0 = np.floor(x).astype(np.int64)
    fx = x - x0
    taps = np.arange(-3, 5)
    t = fx[:, None] - taps[None, :]
    wgt = np.sinc(t) * np.sinc(t / 4.0)
    wgt /= wgt.sum(axis=1, keepdims=True)
    idx = np.clip(x0[:, None] + taps[None, :], 0, n_src - 1)
    return np.ascontiguousarray(idx.astype(np.int32)), np.ascontiguousarray(wgt)


def nearest_indices(n_dst, n_src):
    """int32 [n_dst]: the source index of cv2's INTER_NEAREST as src.utils.vis_utils._resize_nearest computes it: min(int(d * n_src / n_dst), n_src - 1)"""
    import numpy as np
    return np.minimum((np.arange(n_dst) * (n_src / n_dst)).astype(np.int64), n_src - 1).astype(np.int32)


_CASEPREP_DEV = {}


def _caseprep_tables_dev(kind, n_dst, n_src, device):
    key = (kind, int(n_dst), int(n_src), torch.device(device))
    hit = _CASEPREP_DEV.get(key)
    if hit is None:
        if len(_CASEPREP_DEV) > 64:
            _CASEPREP_DEV.clear()
        tabs = lanczos4_taps(n_dst, n_src) if kind == "lanczos4" else (nearest_indices(n_dst, n_src),)
        hit = _CASEPREP_DEV[key] = tuple(torch.from_numpy(t).to(device) for t in tabs)
    return hit


def _as_bhwc(img):
    """uint8 [H, W], [H, W, C] or [B, H, W, C] (device, contiguous) -> (B, H, W, C)"""
    assert img.dtype == torch.uint8 and img.ndim in (2, 3, 4) and img.is_contiguous()
    if img.ndim == 2:
        return (1,) + tuple(img.shape) + (1,)
    return ((1,) if img.ndim == 3 else ()) + tuple(img.shape)


def resize_lanczos4_u8(img, dsize):
    """src.utils.vis_utils._resize_lanczos4 on the device, byte for byte: uint8 [H, W, C] or [B, H, W, C], C in (1, 3); dsize = (w, h) like cv2
    (ffn_resize_taps8_u8).  Equal sizes: a copy."""
    lib = L.load()
    assert img.ndim in (3, 4)
    B, H, W, C = _as_bhwc(img)
    ow, oh = int(dsize[0]), int(dsize[1])
    if (H, W) == (oh, ow):
        return img.clone()
    iy, wy = _caseprep_tables_dev("lanczos4", oh, H, img.device)
    ix, wx = _caseprep_tables_dev("lanczos4", ow, W, img.device)
    out = torch.empty(tuple(img.shape[:-3]) + (oh, ow, C), dtype=torch.uint8, device=img.device)
    L.check(_timed("resize_taps8_u8", 128.0 * B * oh * ow * C, float(C) * B * (H * W + oh * ow),
                   lambda: lib.ffn_resize_taps8_u8(_stream(), img.data_ptr(), out.data_ptr(), B, H, W, C, oh, ow, iy.data_ptr(), wy.data_ptr(), ix.data_ptr(),
                                                   wx.data_ptr())), "ffn_resize_taps8_u8")
    return out


def resize_nearest_u8(img, dsize, binarise=False):
    """src.utils.vis_utils._resize_nearest on the device: uint8 [H, W], [H, W, C] or [B, H, W, C]; dsize = (w, h).  binarise: nonzero bytes become 1, the
    m[m > 0] = 1 of read_and_resize_mask (ffn_resize_gather_u8)."""
    lib = L.load()
    B, H, W, C = _as_bhwc(img)
    ow, oh = int(dsize[0]), int(dsize[1])
    iy, = _caseprep_tables_dev("nearest", oh, H, img.device)
    ix, = _caseprep_tables_dev("nearest", ow, W, img.device)
    shape = (oh, ow) if img.ndim == 2 else tuple(img.shape[:-3]) + (oh, ow, C)
    out = torch.empty(shape, dtype=torch.uint8, device=img.device)
    L.check(_timed("resize_gather_u8", 0.0, 2.0 * C * B * oh * ow,
                   lambda: lib.ffn_resize_gather_u8(_stream(), img.data_ptr(), out.data_ptr(), B, H, W, C, oh, ow, iy.data_ptr(), ix.data_ptr(), int(bool(binarise)))),
            "ffn_resize_gather_u8")
    return out


def dilate_u8(mask, k):
    """src.utils.vis_utils.dilate_mask on the device: the k x k maximum with anchor k // 2, zeros outside; uint8 [H, W], [H, W, C] or [B, H, W, C] (ffn_dilate_u8)"""
    lib = L.load()
    B, H, W, C = _as_bhwc(mask)
    out, scratch = torch.empty_like(mask), torch.empty_like(mask)
    L.check(_timed("dilate_u8", 0.0, 4.0 * C * B * H * W,
                   lambda: lib.ffn_dilate_u8(_stream(), mask.data_ptr(), out.data_ptr(), scratch.data_ptr(), B, H, W, C, int(k))), "ffn_dilate_u8")
    return out


def _square(t, what):
    if t.ndim < 2 or t.shape[0] != t.shape[1]:
        raise ValueError(f"{what}: the GeoDiffuser warp takes square images (the reference takes sqrt(N) for the side); got {tuple(t.shape)}")
    return int(t.shape[0])


def geo_project(depth_n, pose, focal):
    """ffn_geo_project: depth_n fp32 [S, S] on the device (already normalised), pose 3 x 4 (or 4 x 4) on the host -> (tcoords fp32 [S, S, 3] =
    (X_norm, Y_norm, Z), the reference's t_coords; proj fp32 [S * S, 4], the same points as the splat entry points read them)"""
    lib = L.load()
    S = _square(depth_n, "geo_project")
    assert depth_n.dtype == torch.float32 and depth_n.is_contiguous() and depth_n.ndim == 2
    m = [float(v) for v in torch.as_tensor(pose, dtype=torch.float32).reshape(-1)[:12]]
    tcoords = torch.empty((S, S, 3), dtype=torch.float32, device=depth_n.device)
    proj = torch.empty((S * S, 4), dtype=torch.float32, device=depth_n.device)
    L.check(_timed("geo_project", 30.0 * S * S, 32.0 * S * S,
                   lambda: lib.ffn_geo_project(_stream(), depth_n.data_ptr(), (CT.c_float * 12)(*m), float(focal), S, S, tcoords.data_ptr(), proj.data_ptr())),
            "ffn_geo_project")
    return tcoords, proj


def splat_tile_lists(proj, radius, S):
    """the tile lists of ffn_splat_bin for a square S x S image (count, exclusive scan, fill) -> (offs int32 [tiles + 1], list int32).  The scan's total is
    read back: this call synchronises."""
    lib = L.load()
    n, tiles = int(proj.shape[0]), ((S + 15) // 16) ** 2
    counts = torch.zeros(tiles, dtype=torch.int32, device=proj.device)
    L.check(_timed("splat_bin", 0.0, 16.0 * n, lambda: lib.ffn_splat_bin(_stream(), 0, proj.data_ptr(), n, float(radius), S, S, counts.data_ptr(), None, None)),
            "ffn_splat_bin(count)")
    offs = torch.zeros(tiles + 1, dtype=torch.int32, device=proj.device)
    offs[1:] = torch.cumsum(counts, 0)
    lst = torch.empty(max(int(offs[-1].item()), 1), dtype=torch.int32, device=proj.device)
    counts.zero_()
    L.check(_timed("splat_bin", 0.0, 20.0 * n, lambda: lib.ffn_splat_bin(_stream(), 1, proj.data_ptr(), n, float(radius), S, S, counts.data_ptr(), offs.data_ptr(),
                                                                       lst.data_ptr())), "ffn_splat_bin(fill)")
    return offs, lst


def splat_composite(proj, feat, offs, lst, radius, tau, K, S, round_half=True):
    """ffn_splat_composite: proj fp32 [S * S, 4], feat fp32 [S * S, C] (C <= 8), the tile lists of splat_tile_lists, radius in NDC units -> fp32 [S, S, C]"""
    lib = L.load()
    assert proj.dtype == torch.float32 and feat.dtype == torch.float32 and proj.is_contiguous() and feat.is_contiguous() and feat.ndim == 2
    if feat.shape[0] != S * S or proj.shape[0] != S * S:
        raise ValueError(f"splat_composite: {S} x {S} pixels, {proj.shape[0]} points, {feat.shape[0]} feature rows: every pixel is a point")
    C = int(feat.shape[1])
    out = torch.empty((S, S, C), dtype=torch.float32, device=proj.device)
    L.check(_timed("splat_composite", 0.0, 4.0 * S * S * (4 + 2 * C),
                   lambda: lib.ffn_splat_composite(_stream(), proj.data_ptr(), feat.data_ptr(), offs.data_ptr(), lst.data_ptr(), float(radius), float(tau), int(K), C,
                                                   S, S, 1 if round_half else 0, out.data_ptr())), "ffn_splat_composite")
    return out


def splat_ids(proj, offs, lst, radius, K, S):
    """ffn_splat_ids on the same lists: int32 [S, S, K], the point ids splat_composite blends at each pixel in compositing order, -1 = empty"""
    lib = L.load()
    ids = torch.empty((S, S, int(K)), dtype=torch.int32, device=proj.device)
    L.check(lib.ffn_splat_ids(_stream(), proj.data_ptr(), offs.data_ptr(), lst.data_ptr(), float(radius), int(K), S, S, ids.data_ptr()), "ffn_splat_ids")
    return ids


def mesh_cover(tcoords, obj):
    """ffn_mesh_cover: tcoords fp32 [S, S, 3], obj uint8 [S, S] (nonzero = a vertex of the mask's mesh) -> uint8 [S, S], 1 where a pixel centre lies strictly
    inside a projected triangle"""
    lib = L.load()
    S = _square(tcoords, "mesh_cover")
    assert tcoords.dtype == torch.float32 and tcoords.is_contiguous() and obj.dtype == torch.uint8 and obj.is_contiguous() and tuple(obj.shape) == (S, S)
    cover = torch.zeros((S, S), dtype=torch.uint8, device=tcoords.device)
    L.check(_timed("mesh_cover", 0.0, 13.0 * S * S, lambda: lib.ffn_mesh_cover(_stream(), tcoords.data_ptr(), obj.data_ptr(), S, S, cover.data_ptr())),
            "ffn_mesh_cover")
    return cover


def mask_bbox_u8(mask):
    """int64 numpy [B, 4] = (top, bottom, left, right) of the pixels whose channel 0 is nonzero, mask uint8 [B, H, W] or [B, H, W, C] on the device
    (ffn_mask_bbox_u8: one reduction, 16 bytes per case read back -- this call synchronises).  ValueError on an empty mask, like numpy's ys.min()."""
    lib = L.load()
    assert mask.dtype == torch.uint8 and mask.ndim in (3, 4) and mask.is_contiguous()
    B, H, W = mask.shape[:3]
    C = 1 if mask.ndim == 3 else mask.shape[3]
    box = torch.empty((B, 4), dtype=torch.int32, device=mask.device)
    L.check(_timed("mask_bbox_u8", 0.0, float(B) * H * W, lambda: lib.ffn_mask_bbox_u8(_stream(), mask.data_ptr(), box.data_ptr(), B, H, W, C)), "ffn_mask_bbox_u8")
    b = box.cpu().numpy().astype("int64")
    if (b[:, 1] < 0).any():
        raise ValueError("zero-size array to reduction operation minimum which has no identity (empty mask)")
    b[:, 0] *= -1
    b[:, 2] *= -1
    return b


def edit_inverse_affine(box, edit_param):
    """float64 [6]: rows 0 and 1 of the inverse of the forward matrix src.utils.vis_utils._affine_for_edit builds from the mask's bounding box
    (top, bottom, left, right) and edit_param = (dx, dy, rz, sx, sy) or the 9-tuple (dx, dy, dz, rx, ry, rz, sx, sy, sz); inverted as _warp_affine does."""
    import numpy as np
    if len(edit_param) == 9:
        dx, dy, _, _, _, rz, sx, sy, _ = edit_param
    else:
        dx, dy, rz, sx, sy = edit_param
    top, bottom, left, right = (np.int64(v) for v in box)
    cx, cy = (right + left) / 2, (top + bottom) / 2
    a = np.deg2rad(-rz)                                       # _rotation_matrix_2d((cx, cy), -rz, 1)
    al, be = 1 * np.cos(a), 1 * np.sin(a)
    M = np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]], dtype=np.float64)
    M[0, 2] += dx + (1 - sx) * cx
    M[1, 2] += dy + (1 - sy) * cy
    M[0, 0] *= sx
    M[1, 1] *= sy
    return np.ascontiguousarray(np.linalg.inv(np.vstack([M, [0, 0, 1]]))[:2].reshape(6))


def coarse_edit_2d(src_img, src_mask, edit_param, inp_cur, hole_img=None, hole_mask=None):
    """src.utils.vis_utils.re_edit_2d (hole_img / hole_mask None) or re_edit_3d (the other view's image and mask given) on the device, byte for byte
    (ffn_coarse_edit_2d).  uint8 device tensors: src_img, inp_cur, hole_img [H, W, 3]; src_mask [H, W] or [H, W, 3] (channel 0 is used, any nonzero value is
    set); hole_mask [H, W], [H, W, 1] or [H, W, 3] (per channel, numpy's broadcast).  Batched: a leading dimension on every tensor and a list of edit_params.
    The mask's bounding box comes from a device reduction with one 16-byte read-back per case; the matrix is inverted on the host in float64.
    -> (final, target mask in {0, 255}, trans_hole).  ValueError on an empty mask, before the edit kernel is launched."""
    import numpy as np
    lib = L.load()
    batched = src_img.ndim == 4
    if not batched:
        src_img, src_mask, inp_cur = src_img[None], src_mask[None], inp_cur[None]
        hole_img = None if hole_img is None else hole_img[None]
        hole_mask = None if hole_mask is None else hole_mask[None]
        edit_param = [edit_param]
    B, H, W = src_img.shape[:3]
    assert len(edit_param) == B and (hole_img is None) == (hole_mask is None)
    for t in (src_img, inp_cur, hole_img):
        assert t is None or (t.dtype == torch.uint8 and tuple(t.shape) == (B, H, W, 3) and t.is_contiguous() and t.device == src_img.device)
    for t in (src_mask, hole_mask):
        assert t is None or (t.dtype == torch.uint8 and t.ndim in (3, 4) and tuple(t.shape[:3]) == (B, H, W) and t.is_contiguous() and t.device == src_img.device)
    boxes = mask_bbox_u8(src_mask)
    inv = torch.from_numpy(np.stack([edit_inverse_affine(boxes[b], edit_param[b]) for b in range(B)])).to(src_img.device)
    final, trans_hole = torch.empty_like(src_img), torch.empty_like(src_img)
    tmask = torch.empty((B, H, W), dtype=torch.uint8, device=src_img.device)
    d = L.CoarseEditDesc()
    d.src_img, d.src_mask, d.bg, d.inv = src_img.data_ptr(), src_mask.data_ptr(), inp_cur.data_ptr(), inv.data_ptr()
    d.hole_img, d.hole_mask = (None if hole_img is None else hole_img.data_ptr()), (None if hole_mask is None else hole_mask.data_ptr())
    d.final_img, d.tmask, d.trans_hole = final.data_ptr(), tmask.data_ptr(), trans_hole.data_ptr()
    d.B, d.H, d.W = B, H, W
    d.mask_c = 1 if src_mask.ndim == 3 else src_mask.shape[3]
    d.hole_mask_c = 1 if hole_mask is None or hole_mask.ndim == 3 else hole_mask.shape[3]
    L.check(_timed("coarse_edit_2d", 0.0, 14.0 * B * H * W, lambda: lib.ffn_coarse_edit_2d(_stream(), CT.byref(d))), "ffn_coarse_edit_2d")
    return (final, tmask, trans_hole) if batched else (final[0], tmask[0], trans_hole[0])


def vit_norm_table(mean, std):
    """[3, 256] fp32: ToTensor + Normalize(mean, std) of every byte value per channel, evaluated by the very torch expressions the transform runs on an image
    (float32(byte) / 255, then in place - float32(mean[c]), / float32(std[c])) -- the kernel only looks values up."""
    import numpy as np
    mean32 = torch.as_tensor(np.asarray(mean, dtype=np.float64), dtype=torch.float32)
    std32 = torch.as_tensor(np.asarray(std, dtype=np.float64), dtype=torch.float32)
    return torch.stack([torch.arange(256, dtype=torch.uint8).float().div(255).sub_(mean32[c]).div_(std32[c]) for c in range(3)])


def vit_patch_rows(img, lut, patch, ldo, dtype, out=None):
    """uint8 [B, H, W, 3] (device) + lut fp32 [3, 256] (device) -> [B (H / patch)(W / patch), ldo] of `dtype`: the normalised image as the operand rows of the
    patch-embedding GEMM, columns (channel, ky, kx), zero from 3 patch^2 on (ffn_vit_patch_rows)."""
    lib = L.load()
    assert img.dtype == torch.uint8 and img.ndim == 4 and img.shape[-1] == 3 and img.is_contiguous()
    assert lut.dtype == torch.float32 and lut.shape == (3, 256) and lut.is_contiguous() and lut.device == img.device
    B, H, W, _ = img.shape
    M = B * (H // patch) * (W // patch)
    if out is None:
        out = torch.empty(M, ldo, dtype=dtype, device=img.device)
    assert out.dtype == dtype and out.is_contiguous() and out.numel() == M * ldo
    L.check(_timed(f"patch_rows_kernel<{_tname(out)}>", 0.0, 3.0 * B * H * W + float(M) * ldo * out.element_size(),
                   lambda: lib.ffn_vit_patch_rows(_stream(), _dt(out), img.data_ptr(), lut.data_ptr(), out.data_ptr(), B, H, W, patch, ldo)), "ffn_vit_patch_rows")
    return out


def vit_patch_rows_pair(img, lut, patch, K, out=None):
    """uint8 [B, H, W, 3] (device) + lut fp32 [3, 256] (device) -> bf16 PAIR rows [B (H / patch)(W / patch), 2K] (ffn_vit_patch_rows_pair; layout:
    include/freefine_hip.h FFN_BF16X3): the bytes split_pair(vit_patch_rows(..., K, torch.float32)) gives, in one pass -- the A operand of the split-bf16
    patch-embedding GEMM.  K % 8 == 0; columns from 3 patch^2 on are zero in both halves."""
    lib = L.load()
    assert img.dtype == torch.uint8 and img.ndim == 4 and img.shape[-1] == 3 and img.is_contiguous()
    assert lut.dtype == torch.float32 and lut.shape == (3, 256) and lut.is_contiguous() and lut.device == img.device
    B, H, W, _ = img.shape
    M = B * (H // patch) * (W // patch)
    if out is None:
        out = torch.empty(M, 2 * K, dtype=torch.bfloat16, device=img.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == M * 2 * K
    L.check(_timed("patch_rows_pair_kernel", 0.0, 3.0 * B * H * W + 4.0 * M * K,
                   lambda: lib.ffn_vit_patch_rows_pair(_stream(), img.data_ptr(), lut.data_ptr(), out.data_ptr(), B, H, W, patch, K)), "ffn_vit_patch_rows_pair")
    return _mark_pair(out, K)


def _f3(v):
    return (CT.c_float * 3)(*[float(x) for x in v])


def sam_patch_rows(img, side, patch, ldo, dtype, mean, std, pair=False):
    """uint8 [B, H, W, 3] (device) of any size -> the patch GEMM's operand rows for a side x side input: ToTensor, bilinear resize (ATen, align_corners=False, no
    antialiasing) where the size differs, (x - mean) / std, im2col -- [B (side / patch)^2, ldo] of `dtype` (ffn_sam_patch_rows), or with pair the bf16 PAIR rows
    [.., 2 ldo] of split-bf16 (ffn_sam_patch_rows_pair).  mean, std: three host floats each."""
    lib = L.load()
    assert img.dtype == torch.uint8 and img.ndim == 4 and img.shape[-1] == 3 and img.is_contiguous() and img.is_cuda
    B, H, W, _ = img.shape
    M = B * (side // patch) ** 2
    mean, std = _f3(mean), _f3(std)
    if pair:
        out = torch.empty(M, 2 * ldo, dtype=torch.bfloat16, device=img.device)
        L.check(_timed("sam_patch_rows_pair_kernel", 0.0, 3.0 * B * H * W + 4.0 * M * ldo,
                       lambda: lib.ffn_sam_patch_rows_pair(_stream(), img.data_ptr(), out.data_ptr(), B, H, W, side, patch, ldo, mean, std)), "ffn_sam_patch_rows_pair")
        return _mark_pair(out, ldo)
    out = torch.empty(M, ldo, dtype=dtype, device=img.device)
    L.check(_timed(f"sam_patch_rows_kernel<{_tname(out)}>", 0.0, 3.0 * B * H * W + float(M) * ldo * out.element_size(),
                   lambda: lib.ffn_sam_patch_rows(_stream(), _dt(out), img.data_ptr(), out.data_ptr(), B, H, W, side, patch, ldo, mean, std)), "ffn_sam_patch_rows")
    return out


def hyper_masks(up, hyper):
    """up fp32 [N, hw, C] (NHWC rows), hyper fp32 [N, M, C] -> fp32 [N, M, hw]: per pixel and mask the C-long dot product (ffn_hyper_masks)"""
    lib = L.load()
    assert up.dtype == hyper.dtype == torch.float32 and up.ndim == 3 and hyper.ndim == 3 and up.is_contiguous() and hyper.is_contiguous()
    N, hw, Cc = up.shape
    M = hyper.shape[1]
    assert hyper.shape[0] == N and hyper.shape[2] == Cc
    out = torch.empty(N, M, hw, dtype=torch.float32, device=up.device)
    L.check(_timed("hyper_masks_kernel", 2.0 * N * M * hw * Cc, 4.0 * (up.numel() + out.numel()),
                   lambda: lib.ffn_hyper_masks(_stream(), up.data_ptr(), hyper.data_ptr(), out.data_ptr(), N, hw, Cc, M)), "ffn_hyper_masks")
    return out


def upsample_bicubic(x, H, W, mask=False):
    """fp32 [N, h, w] -> fp32 [N, H, W]: ATen's bicubic interpolation (align_corners=False, A = -0.75); mask: also uint8 [N, H, W] = 255 (result >= 0), from the
    stored values (ffn_upsample_bicubic)"""
    lib = L.load()
    assert x.dtype == torch.float32 and x.ndim == 3 and x.is_contiguous()
    N, h, w = x.shape
    out = torch.empty(N, H, W, dtype=torch.float32, device=x.device)
    m = torch.empty(N, H, W, dtype=torch.uint8, device=x.device) if mask else None
    L.check(_timed("upsample_bicubic_kernel", 0.0, 4.0 * x.numel() + (5.0 if mask else 4.0) * out.numel(),
                   lambda: lib.ffn_upsample_bicubic(_stream(), x.data_ptr(), out.data_ptr(), _p(m), N, h, w, H, W)), "ffn_upsample_bicubic")
    return (out, m) if mask else out


def upsample_bicubic_stats(x, H, W, offset, mask=False):
    """fp32 [N, h, w] -> int32 [N, 8] = (area, n_hi, n_lo, x_min, y_min, x_max, y_max, 0) of the H x W image upsample_bicubic would return, which is not stored:
    area = #(v >= 0), n_hi = #(v > offset), n_lo = #(v > -offset), the extents over v >= 0 (maxima inclusive; an empty map gives 0, 0, 0, 0); mask: also the
    uint8 [N, H, W] = 255 (v >= 0) of upsample_bicubic(..., mask=True), bit for bit (ffn_upsample_bicubic_stats)"""
    lib = L.load()
    assert x.dtype == torch.float32 and x.ndim == 3 and x.is_contiguous()
    N, h, w = x.shape
    stats = torch.empty(N, 8, dtype=torch.int32, device=x.device)
    m = torch.empty(N, H, W, dtype=torch.uint8, device=x.device) if mask else None
    L.check(_timed("upsample_bicubic_stats_kernel", 0.0, 4.0 * x.numel() + 32.0 * N + (float(N) * H * W if mask else 0.0),
                   lambda: lib.ffn_upsample_bicubic_stats(_stream(), x.data_ptr(), stats.data_ptr(), _p(m), N, h, w, H, W, float(offset))), "ffn_upsample_bicubic_stats")
    return (stats, m) if mask else stats


def nms_sweep(suppress):
    """host: the bit matrix of ffn_box_nms as numpy uint64 [M, ceil(M / 64)] -> the rows greedy NMS keeps, ascending: row i unless an earlier KEPT row has bit i set"""
    import numpy as np
    removed = np.zeros(suppress.shape[1], dtype=np.uint64)
    keep = []
    for i in range(suppress.shape[0]):
        if not (int(removed[i >> 6]) >> (i & 63)) & 1:
            keep.append(i)
            removed |= suppress[i]
    return keep


def box_nms(boxes, scores, thresh):
    """boxes fp32 [M, 4] (x1, y1, x2, y2), scores [M] (device) -> int64 [K] (device): greedy non-maximum suppression by box IoU > thresh, as torchvision.ops.nms
    defines it (no "+ 1" in the areas; zero-area boxes never suppress each other).  Order: torch.argsort(scores, descending=True, stable=True); the result indexes
    the caller's boxes, best first.  The pairwise bit matrix is the device's (ffn_box_nms), the sweep over its rows the host's (nms_sweep)."""
    import numpy as np
    lib = L.load()
    assert boxes.dtype == torch.float32 and boxes.ndim == 2 and boxes.shape[1] == 4 and scores.shape == (boxes.shape[0],) and scores.device == boxes.device
    M = boxes.shape[0]
    if M == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    order = torch.argsort(scores, descending=True, stable=True)
    ranked = boxes[order].contiguous()
    nb = (M + 63) // 64
    sup = torch.empty(M, nb, dtype=torch.int64, device=boxes.device)          # the bits of uint64 words
    L.check(_timed("box_nms_kernel", 20.0 * M * M / 2, 16.0 * M + 8.0 * M * nb, lambda: lib.ffn_box_nms(_stream(), ranked.data_ptr(), sup.data_ptr(), M, float(thresh))),
            "ffn_box_nms")
    keep = nms_sweep(sup.cpu().numpy().view(np.uint64))
    return order[torch.as_tensor(keep, dtype=torch.int64, device=boxes.device)]


def image_to_nhwc(img_u8, CP, dtype, out=None):
    """uint8 [B,H,W,3] -> dtype [B,HW,CP] in [-1,1]."""
    lib = L.load()
    B, H, W, _ = img_u8.shape
    if out is None:
        out = torch.empty(B, H * W, CP, dtype=dtype, device=img_u8.device)
    L.check(_timed(f"image_to_nhwc_kernel<{_tname(out)}>", 0.0, B * H * W * (3.0 + CP * out.element_size()),
                   lambda: lib.ffn_image_to_nhwc(_stream(), _dt(out), img_u8.data_ptr(), out.data_ptr(), B * H * W, CP)), "ffn_image_to_nhwc")
    return out


def nhwc_to_image(src, H, W, out=None):
    lib = L.load()
    B, HW, ld = src.shape
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=src.device)
    L.check(_timed(f"nhwc_to_image_kernel<{_tname(src)}>", 0.0, B * HW * 3.0 * (src.element_size() + 4),
                   lambda: lib.ffn_nhwc_to_image(_stream(), _dt(src), src.data_ptr(), out.data_ptr(), B, HW, ld)), "ffn_nhwc_to_image")
    return out


# ---------------------------------------------------------------------------------------------------------------
# the igemm tuner's table as data (persist across processes / broadcast across ranks)
# ---------------------------------------------------------------------------------------------------------------
def tune_table_export():
    """int32 tensor [n, entry_ints] of the bf16 igemm configurations tuned so far in this process."""
    lib = L.load()
    w = lib.ffn_igemm_tune_entry_ints()
    n = lib.ffn_igemm_tune_export(None, 0)
    buf = (CT.c_int * max(1, n * w))()
    n = min(n, lib.ffn_igemm_tune_export(buf, n))
    return torch.tensor(list(buf[:n * w]), dtype=torch.int32).reshape(n, w)


def tune_table_import(table):
    """merge a table produced by tune_table_export (another process, another rank); returns the number of entries taken."""
    lib = L.load()
    table = table.to(torch.int32).contiguous().cpu()
    w = lib.ffn_igemm_tune_entry_ints()
    if table.numel() == 0 or table.shape[1] != w:
        return 0
    buf = (CT.c_int * table.numel())(*table.flatten().tolist())
    return lib.ffn_igemm_tune_import(buf, table.shape[0])


def tune_table_clear():
    return L.load().ffn_igemm_tune_clear()


def tune_enable(on):
    """timing-based tuning of unseen bf16 igemm shapes on / off for this process (off: the deterministic rule); returns the previous setting"""
    return bool(L.load().ffn_igemm_tune_enable(1 if on else 0))


def tune_table_save(path):
    torch.save(tune_table_export(), path)


def tune_table_load(path):
    """a table written by tune_table_save.  weights_only: the file is data (a 2-D int32 tensor), never code; anything else is ignored."""
    if not os.path.exists(path):
        return 0
    table = torch.load(path, weights_only=True, map_location="cpu")
    if not torch.is_tensor(table) or table.ndim != 2 or table.dtype not in (torch.int32, torch.int64):
        return 0
    return tune_table_import(table)


# ---------------------------------------------------------------------------------------------------------------
# the Inception-v3 kernels of FID (csrc/convkk.h): NHWC fp32 tensors [B, H, W, C] that may be channel slices of a wider tensor (column views)
# ---------------------------------------------------------------------------------------------------------------
def _nhwc_view(t):
    """[B, H, W, C] fp32 with contiguous channels and pixels `ld` apart (a tensor or its [..., a:b] slice) -> ld"""
    assert t.dtype == torch.float32 and t.ndim == 4 and t.is_cuda
    B, H, W, C = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else C))
    assert C == 1 or t.stride(3) == 1
    assert (W == 1 or t.stride(2) == ld) and (H == 1 or t.stride(1) == W * ld) and (B == 1 or t.stride(0) == H * W * ld) and ld >= C, (t.shape, t.stride())
    return ld


def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv2d_kk(x, w, bias, kh, kw, stride=1, pad=(0, 0), relu=True, out=None):
    """x [B, H, W, Cin] view, w fp32 [N, Kpad] with columns (ky, kx, ci), bias fp32 [N] or None -> out [B, Hout, Wout, N] (a view to write into, or a new tensor):
    ffn_conv2d, the implicit GEMM on the exact-fp32 MFMA."""
    lib = L.load()
    B, H, W, Cin = x.shape
    N, Kpad = w.shape
    assert w.dtype == torch.float32 and w.is_contiguous() and (bias is None or (bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()))
    Ho, Wo = conv_out_size(H, kh, stride, pad[0]), conv_out_size(W, kw, stride, pad[1])
    if out is None:
        out = torch.empty(B, Ho, Wo, N, dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == (B, Ho, Wo, N), (tuple(out.shape), (B, Ho, Wo, N))
    d = L.Conv2dDesc()
    d.x, d.w, d.bias, d.out = x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr()
    d.B, d.Hin, d.Win, d.Cin, d.N = B, H, W, Cin, N
    d.KH, d.KW, d.stride, d.pad_h, d.pad_w = kh, kw, stride, pad[0], pad[1]
    d.ldx, d.ldo, d.Kpad, d.flags = _nhwc_view(x), _nhwc_view(out), Kpad, (L.CONV_RELU if relu else 0)
    M, K = B * Ho * Wo, kh * kw * Cin
    L.check(_timed(f"convkk_kernel {kh}x{kw} s{stride}", 2.0 * M * N * K, 4.0 * (B * H * W * Cin + N * K + M * N), lambda: lib.ffn_conv2d(_stream(), L.FFN_F32, CT.byref(d))),
            "ffn_conv2d")
    return out


def pool2d(x, op, k=3, stride=1, pad=0, out=None):
    """x [B, H, W, C] view -> [B, Hout, Wout, C]: op "max" (max_pool2d) or "avg_valid" (avg_pool2d(count_include_pad=False)); ffn_pool2d"""
    lib = L.load()
    B, H, W, C = x.shape
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    if out is None:
        out = torch.empty(B, Ho, Wo, C, dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == (B, Ho, Wo, C)
    code = {"max": L.POOL_MAX, "avg_valid": L.POOL_AVG_VALID}[op]
    L.check(_timed(f"pool2d_kernel<{op}>", 0.0, 4.0 * C * B * (H * W + Ho * Wo),
                   lambda: lib.ffn_pool2d(_stream(), code, x.data_ptr(), out.data_ptr(), B, H, W, C, _nhwc_view(x), _nhwc_view(out), k, stride, pad)), "ffn_pool2d")
    return out


def mean_hw(x):
    """x [B, H, W, C] view -> fp32 [B, C]: AdaptiveAvgPool2d(1), pixels summed in ascending order (ffn_mean_hw)"""
    lib = L.load()
    B, H, W, C = x.shape
    out = torch.empty(B, C, dtype=torch.float32, device=x.device)
    L.check(_timed("mean_hw_kernel", 0.0, 4.0 * C * B * (H * W + 1), lambda: lib.ffn_mean_hw(_stream(), x.data_ptr(), out.data_ptr(), B, H * W, C, _nhwc_view(x))),
            "ffn_mean_hw")
    return out


def fid_prep(img, lut, side_out):
    """uint8 [B, S, S, 3] (device) + lut fp32 [3, 256] (vit_norm_table) -> fp32 [B, side_out, side_out, 4]: the lookup, ATen's bilinear resize (align_corners=False),
    2 v - 1, a zero fourth channel (ffn_fid_prep)"""
    lib = L.load()
    assert img.dtype == torch.uint8 and img.ndim == 4 and img.shape[-1] == 3 and img.shape[1] == img.shape[2] and img.is_contiguous() and img.is_cuda
    assert lut.dtype == torch.float32 and lut.shape == (3, 256) and lut.is_contiguous() and lut.device == img.device
    B, S = img.shape[0], img.shape[1]
    out = torch.empty(B, side_out, side_out, 4, dtype=torch.float32, device=img.device)
    L.check(_timed("fid_prep_kernel", 0.0, 3.0 * B * S * S + 16.0 * B * side_out * side_out,
                   lambda: lib.ffn_fid_prep(_stream(), img.data_ptr(), lut.data_ptr(), out.data_ptr(), B, S, side_out)), "ffn_fid_prep")
    return out
