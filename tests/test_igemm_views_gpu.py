"""ffn_igemm on the layouts production uses and the dense tests of test_ops_gpu.py do not: outputs that are column windows of wider buffers (the UNet's
concat destinations), residuals with a row stride of their own, A with lda > K, W with Kpad > K, transposed outputs with row padding.

Method (every test):
  reference   the fp64 statement of the op on the values the kernel is given (bf16-rounded inputs in bf16 mode, dequantised ones in fp8 mode), compared at
              the gates of test_ops_gpu.py: tol(dtype), X3_TOL for split-bf16;
  bit check   the arithmetic order of a kernel does not depend on strides, so wherever ffn_igemm_kernel_name names the same kernel for the strided and the
              compact call (K split pinned) the two results must be torch.equal: any difference is an addressing bug.  Where the names differ the assert
              message of the fp64 check says so and only that check applies;
  canaries    every output is a window of a larger sentinel-filled allocation whose raw bits are snapshot before the launch: every element outside the
              window (columns left and right of it in rows < M, `GUARD` rows behind row M, columns [S, ldo) of a transposed row) must be bit-identical after;
  poison      what the ABI says is never read holds NaN: columns [K, lda) of A, [K, Kpad) of W, the columns of a strided residual outside its window, the gap
              between and the space behind split-bf16 planes.  A NaN in the result is the failure;
  every configuration   bf16 / split-bf16 / fp8 cases run under ffn_igemm_force_config(cfg) for every cfg and once unforced (FFN_F32 and transposed outputs are
              planned by rule: the hook does not reach them, they run once).
First-use timing is switched off for the file: with it, the kernel a first call launches is the timed winner, not the one ffn_igemm_kernel_name names before
the call; off, the choice is the deterministic rule (what a launch under stream capture takes) and the name is the kernel launched.
Each test prints, per case and mode, the worst relative error it measured and how many of its strided launches the bit check covered."""
import ctypes as CT

import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import X3_TOL, _IGEMM_CFG_TILES, _quant_act_f8, pair_value, relerr, rnd, tol

pytestmark = pytest.mark.gpu

SENT = 7.0           # sentinel of the canary regions
GUARD = 300          # rows behind row M
M_DENSE = 2 * 256 + 72          # ragged for the 64-, 128-, 192- and 256-row tiles
DENSE_SHAPES = [(320, 320), (256, 128), (328, 136), (64, 72)]          # (N, K): ping-pong tiles and their smallest K; ragged N; split-bf16 planes, K % 32 != 0
LAYOUTS = [(0, 64), (0, 4), (64, 64), (64, 4)]          # (c0, pad_right): pad_right = 4 makes ldo % 8 == 4 (bf16 row starts 8 bytes apart)
MODES = ["f32", "bf16", "x3"]


@pytest.fixture(autouse=True)
def _rule_based_choice(gpu):
    from freefine_amd import _lib as L
    lib = L.load()
    prev = lib.ffn_igemm_tune_enable(0)
    yield
    lib.ffn_igemm_tune_enable(prev)
    lib.ffn_igemm_force_config(-1)


def _gate(mode):
    return X3_TOL if mode == "x3" else tol(torch.bfloat16 if mode in ("bf16", "fp8") else torch.float32)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Canary:
    """raw bits of an allocation before a launch; check(): everything outside the window is still what it was"""

    def __init__(self, buf):
        self.buf, self.snap = buf, _bits(buf).clone()

    def check(self, window, what):
        changed = _bits(self.buf) != self.snap
        changed[window] = False
        assert not changed.any(), (what, "written outside the window at", changed.nonzero()[:4].tolist())


class Report:
    def __init__(self, what):
        self.what, self.worst, self.bit, self.n, self.kernels = what, 0.0, 0, 0, set()

    def add(self, err, bit, kernel):
        self.worst, self.bit, self.n = max(self.worst, err), self.bit + int(bit), self.n + 1
        self.kernels.add(str(kernel))

    def show(self):
        print(f"igemm views {self.what}: worst relerr {self.worst:.2e}; same-kernel bit check on {self.bit} of {self.n} strided launches; {len(self.kernels)} kernel(s)")


def _launch(fn):
    """fn() under the profiling hook of ops: -> (result, names of the igemm kernels ffn_igemm_kernel_name gave for its launches)"""
    from freefine_amd import ops
    ops.profile_begin()
    try:
        out = fn()
    finally:
        names = sorted(n for n in ops.profile_end() if "igemm" in n)
    return out, names


def _configs(lib, mode):
    """-1 (unforced) and, for the tuned family, every configuration"""
    assert lib.ffn_igemm_num_configs() == len(_IGEMM_CFG_TILES)
    return [-1] + ([] if mode == "f32" else list(range(lib.ffn_igemm_num_configs())))


def _compare(rep, mode, got, ref, compact, same, what):
    assert not torch.isnan(got).any(), (what, "NaN in the result: a region the ABI says is never read was read")
    err = relerr(got, ref)
    rep.add(err, same, what[-1])          # (the last item of `what` names the kernel(s) launched)
    assert err < _gate(mode), (what, err, "same kernel as the compact call" if same else "the compact call runs another kernel: fp64 check only")
    if same:
        assert torch.equal(got, compact), (what, "strided and compact results of the same kernel differ", (got.double() - compact.double()).abs().max().item())


def _operands(mode, M, N, K, gpu, g):
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x, w = rnd((M, K), dt, gpu, g), rnd((N, K), dt, gpu, g, K ** -0.5)
    return dt, x, w


def _poisoned(rows, cols, c0, values):
    """[rows, cols] of NaN with `values` at columns [c0, c0 + values.shape[1]) -> (buffer, window view)"""
    buf = torch.full((rows, cols), float("nan"), dtype=values.dtype, device=values.device)
    buf[:, c0:c0 + values.shape[1]] = values
    return buf, buf[:, c0:c0 + values.shape[1]]


# ---------------------------------------------------------------------------------------------------------------------
# dense A, output window buf[:M, c0:c0 + N] of [M + GUARD, c0 + N + pad_right]
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", DENSE_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_dense_output_window(gpu, mode, N, K):
    """every plain epilogue (bias; bias + residual, the residual a column view with ldr = N + 20; SiLU; fp32 output; row bias with two batches) unsplit, and
    three of them with three K slices (the reduce kernel's stores), into every window layout"""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    g = torch.Generator().manual_seed(N * 3 + K)
    M = M_DENSE
    dt, x, w = _operands(mode, M, N, K, gpu, g)
    wp = ops.pack_linear(w, dt, x3=mode == "x3")
    xa = ops.split_pair(x, K) if mode == "x3" else x
    b, rb, r = rnd((N,), torch.float32, gpu, g), rnd((2, N), torch.float32, gpu, g), rnd((M, N), dt, gpu, g)
    _, rview = _poisoned(M, N + 20, 8, r)
    assert rview.stride(0) != N
    y = x.double() @ w.double().t()
    yb = y + b.double()
    epis = [("bias", dict(bias=b), 1, yb),
            ("bias+residual", dict(bias=b, residual=True), 1, yb + r.double()),
            ("silu", dict(bias=b, silu=True), 1, F.silu(yb)),
            ("out_f32", dict(out_f32=True), 1, y),
            ("rowbias", dict(rowbias=rb, rows_per_batch=M // 2), 1, y + rb.double().repeat_interleave(M // 2, 0)),
            ("bias+residual, 3 K slices", dict(bias=b, residual=True), 3, yb + r.double()),
            ("silu, 3 K slices", dict(bias=b, silu=True), 3, F.silu(yb)),
            ("out_f32, 3 K slices", dict(out_f32=True), 3, y)]
    rep = Report(f"dense output window {mode} N={N} K={K}")
    for cfg in _configs(lib, mode):
        lib.ffn_igemm_force_config(cfg)
        for name, kw, sk, ref in epis:
            kw = dict(kw)
            res = kw.pop("residual", False)
            bias = kw.pop("bias", None)
            odt = torch.float32 if (kw.get("out_f32") or mode == "x3") else dt
            compact, cname = _launch(lambda: ops.linear(xa, wp, bias, K=K, residual=r if res else None, splitk=sk, **kw))
            for c0, pad in LAYOUTS:
                big = torch.full((M + GUARD, c0 + N + pad), SENT, dtype=odt, device=gpu)
                can = Canary(big)
                out = big[:M, c0:c0 + N]
                _, sname = _launch(lambda: ops.linear(xa, wp, bias, K=K, residual=rview if res else None, splitk=sk, out=out, **kw))
                what = (mode, N, K, name, "cfg", cfg, "c0", c0, "pad_right", pad, sname)
                can.check((slice(0, M), slice(c0, c0 + N)), what)
                _compare(rep, mode, out, ref, compact, sname == cname, what)
    rep.show()


@pytest.mark.parametrize("mode", MODES)
def test_geglu_output_window(gpu, mode):
    """GEGLU (N = 2 * 320 packed columns -> 320 output columns) into every window layout"""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    g = torch.Generator().manual_seed(41)
    M, K, Fh = M_DENSE, 320, 320
    dt, x, w = _operands(mode, M, 2 * Fh, K, gpu, g)
    b = rnd((2 * Fh,), torch.float32, gpu, g)
    wp, bp = ops.pack_geglu(w, b, dt, x3=mode == "x3")
    xa = ops.split_pair(x, K) if mode == "x3" else x
    y = x.double() @ w.double().t() + b.double()
    ref = y[:, :Fh] * F.gelu(y[:, Fh:])
    rep = Report(f"GEGLU output window {mode}")
    for cfg in _configs(lib, mode):
        lib.ffn_igemm_force_config(cfg)
        compact, cname = _launch(lambda: ops.linear(xa, wp, bp, K=K, geglu=True, splitk=1))
        for c0, pad in LAYOUTS:
            big = torch.full((M + GUARD, c0 + Fh + pad), SENT, dtype=dt, device=gpu)
            can = Canary(big)
            out = big[:M, c0:c0 + Fh]
            _, sname = _launch(lambda: ops.linear(xa, wp, bp, K=K, geglu=True, splitk=1, out=out))
            what = (mode, "geglu", "cfg", cfg, "c0", c0, "pad_right", pad, sname)
            can.check((slice(0, M), slice(c0, c0 + Fh)), what)
            _compare(rep, mode, out, ref, compact, sname == cname, what)
    rep.show()


def _dense_desc(A, W, out, M, N, K, lda, Kpad, ldo, *, bias=None, residual=None, ldr=0, flags=0, splitk=1, x3=0, a_lo=0):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    d = L.IgemmDesc()
    d.A, d.W, d.out, d.bias, d.residual = A.data_ptr(), W.data_ptr(), out.data_ptr(), ops._p(bias), ops._p(residual)
    d.M, d.N, d.K, d.Kpad, d.lda, d.ldo, d.ldr, d.rows_per_batch = M, N, K, Kpad, lda, ldo, ldr, M
    d.flags, d.alpha, d.conv, d.splitk, d.x3, d.a_lo = flags, 1.0, 0, splitk, x3, a_lo
    d.ws, d.ws_bytes = ops._workspace(out.device).data_ptr(), ops.WS_BYTES
    return d


def _run_desc(lib, dcode, d):
    """-> the kernel ffn_igemm_kernel_name names for d, after launching d"""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    name = ops._igemm_name(lib, dcode, d)
    L.check(lib.ffn_igemm(ops._stream(), dcode, CT.byref(d)), "ffn_igemm")
    return name


@pytest.mark.parametrize("c0", [0, 64])
def test_x3_pair_output_into_a_wider_row(gpu, c0):
    """FFN_IG_OUT_PAIR into a row wider than its columns, in the one form the ABI admits: (ldo / 2) % 32 == 0 and whole 32-column blocks.  N = 320 columns =
    ten 128-byte blocks [hi(32) | lo(32)] of a row of 12 blocks, starting at block c0 / 64: the blocks written are ffn_split_pair of the fp32 result of the
    same kernel bit for bit, hi + lo is the fp64 result at the split-bf16 gate, every other block of the row and the guard rows keep their bits."""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    g = torch.Generator().manual_seed(43 + c0)
    M, N, K = M_DENSE, 320, 320
    x, w = rnd((M, K), torch.float32, gpu, g), rnd((N, K), torch.float32, gpu, g, K ** -0.5)
    b, r = rnd((N,), torch.float32, gpu, g), rnd((M, N), torch.float32, gpu, g)
    wp, xa = ops.pack_linear(w, torch.float32, x3=True), ops.split_pair(x, K)
    _, rview = _poisoned(M, N + 20, 8, r)
    ref = x.double() @ w.double().t() + b.double() + r.double()
    ldo = 2 * (N + 64)
    rep = Report(f"pair output into a wider row, first block {c0 // 64}")
    for cfg in _configs(lib, "x3"):
        lib.ffn_igemm_force_config(cfg)
        for sk in (1, 3):
            f32 = torch.empty(M, N, dtype=torch.float32, device=gpu)
            fname = _run_desc(lib, L.FFN_BF16X3, _dense_desc(xa, wp, f32, M, N, K, 2 * K, 2 * K, N, bias=b, residual=r, ldr=N, splitk=sk, x3=2, a_lo=32))
            big = torch.full((M + GUARD, ldo), SENT, dtype=torch.bfloat16, device=gpu)
            can = Canary(big)
            win = big[:M, c0:c0 + 2 * N]
            d = _dense_desc(xa, wp, win, M, N, K, 2 * K, 2 * K, ldo, bias=b, residual=rview, ldr=rview.stride(0), flags=L.IG_OUT_PAIR, splitk=sk, x3=2, a_lo=32)
            pname = _run_desc(lib, L.FFN_BF16X3, d)
            what = ("pair window", "cfg", cfg, "splitk", sk, pname)
            can.check((slice(0, M), slice(c0, c0 + 2 * N)), what)
            _compare(rep, "x3", pair_value(win, N), ref, None, False, what)
            if pname == fname:
                rep.bit += 1
                assert torch.equal(_bits(win), _bits(ops.split_pair(f32, N))), (what, "pair window differs from ffn_split_pair of the same kernel's fp32 result")
    rep.show()


# ---------------------------------------------------------------------------------------------------------------------
# dense, strided inputs: A = buf[:, a0:a0 + K] with lda = a0 + K + 64, W with Kpad = K + 64, NaN around both
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", DENSE_SHAPES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_dense_strided_inputs(gpu, mode, N, K):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    g = torch.Generator().manual_seed(N * 5 + K)
    M = M_DENSE
    dt, x, w = _operands(mode, M, N, K, gpu, g)
    b, r = rnd((N,), torch.float32, gpu, g), rnd((M, N), dt, gpu, g)
    wp = ops.pack_linear(w, dt)
    _, wview = _poisoned(N, K + 64, 0, w)
    ref = x.double() @ w.double().t() + b.double() + r.double()
    rep = Report(f"dense strided inputs {mode} N={N} K={K}")
    for cfg in _configs(lib, mode):
        lib.ffn_igemm_force_config(cfg)
        for sk in (1, 3):
            compact, cname = _launch(lambda: ops.linear(x, wp, b, K=K, residual=r, splitk=sk))
            for a0 in (0, 64):
                _, xview = _poisoned(M, a0 + K + 64, a0, x)
                assert xview.stride(0) == a0 + K + 64 and wview.stride(0) == K + 64
                out, sname = _launch(lambda: ops.linear(xview, wview, b, K=K, residual=r, splitk=sk))
                _compare(rep, mode, out, ref, compact, sname == cname, (mode, N, K, "cfg", cfg, "splitk", sk, "a0", a0, sname))
    rep.show()


@pytest.mark.parametrize("N,K,layout", [(320, 320, "blocked"), (256, 128, "blocked"), (320, 320, "planes"), (256, 128, "planes"), (328, 136, "planes"), (64, 72, "planes")])
def test_x3_strided_pair_inputs(gpu, N, K, layout):
    """split-bf16 A and W as windows of NaN-filled rows.  Blocked (x3 = 2): pair rows at columns [a0, a0 + 2K), lda = a0 + 2K + 64, W rows of Kpad = 2K + 64.
    Planes (x3 = 1): hi at [a0, a0 + K), lo at a_lo = K + gap behind it (gap = 8 for a0 = 64: the space between the planes is poisoned too),
    lda = a0 + 2K + gap + 64, W = [hi | lo | hi] with Kpad = 3K + 64."""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    g = torch.Generator().manual_seed(N * 7 + K)
    M = M_DENSE
    x, w = rnd((M, K), torch.float32, gpu, g), rnd((N, K), torch.float32, gpu, g, K ** -0.5)
    b, r = rnd((N,), torch.float32, gpu, g), rnd((M, N), torch.float32, gpu, g)
    ref = x.double() @ w.double().t() + b.double() + r.double()
    xh, xl = ops.split_hi_lo(x)
    wh, wl = ops.split_hi_lo(w)
    if layout == "blocked":
        code = 2
        wc = ops.pack_linear(w, torch.float32, x3=True)
        xc = ops.split_pair(x, K)
        assert ops.pair_width(xc) == K and wc._ffn_x3 == 2
    else:
        code = 1
        wc = torch.cat([wh, wl, wh], dim=1).contiguous()
        xc = torch.cat([xh, xl], dim=1).contiguous()
    _, wview = _poisoned(N, wc.shape[1] + 64, 0, wc)
    rep = Report(f"split-bf16 strided inputs, {layout} N={N} K={K}")
    for cfg in _configs(lib, "x3"):
        lib.ffn_igemm_force_config(cfg)
        compact = torch.empty(M, N, dtype=torch.float32, device=gpu)
        cname = _run_desc(lib, L.FFN_BF16X3, _dense_desc(xc, wc, compact, M, N, K, 2 * K, wc.shape[1], N, bias=b, residual=r, ldr=N, x3=code, a_lo=32 if code == 2 else K))
        for a0 in (0, 64):
            gap = 8 if (layout == "planes" and a0) else 0
            lda = a0 + 2 * K + gap + 64
            abuf = torch.full((M, lda), float("nan"), dtype=torch.bfloat16, device=gpu)
            if layout == "blocked":
                abuf[:, a0:a0 + 2 * K] = xc
                a_lo = 32
            else:
                abuf[:, a0:a0 + K] = xh
                abuf[:, a0 + K + gap:a0 + 2 * K + gap] = xl
                a_lo = K + gap
            out = torch.empty(M, N, dtype=torch.float32, device=gpu)
            d = _dense_desc(abuf[:, a0:], wview, out, M, N, K, lda, wview.stride(0), N, bias=b, residual=r, ldr=N, x3=code, a_lo=a_lo)
            sname = _run_desc(lib, L.FFN_BF16X3, d)
            _compare(rep, "x3", out, ref, compact, sname == cname, (layout, N, K, "cfg", cfg, "a0", a0, "a_lo", a_lo, sname))
    rep.show()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_activation_serves_as_w(gpu, mode):
    """attention as a GEMM: scores = scale * q k^T with q and k column windows of one fused [rows, q | k | v] activation buffer -- W rows are Kpad = 3 D apart
    and everything around the two windows is NaN"""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    g = torch.Generator().manual_seed(47)
    M, Sk, D = M_DENSE, 200, 64
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    q, k = rnd((M, D), dt, gpu, g), rnd((Sk, D), dt, gpu, g)
    _, qv = _poisoned(M, 3 * D, 0, q)
    _, kv = _poisoned(Sk, 3 * D, D, k)
    ref = 0.125 * (q.double() @ k.double().t())
    rep = Report(f"activation as W {mode}")
    for cfg in _configs(lib, mode):
        lib.ffn_igemm_force_config(cfg)
        compact, cname = _launch(lambda: ops.linear(q, k, None, K=D, alpha=0.125, splitk=1))
        out, sname = _launch(lambda: ops.linear(qv, kv, None, K=D, alpha=0.125, splitk=1))
        _compare(rep, mode, out, ref, compact, sname == cname, (mode, "cfg", cfg, sname))
    rep.show()


# ---------------------------------------------------------------------------------------------------------------------
# transposed output out[b][n][s] with row padding (the V^T operand of ffn_attn)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,ldo", [(72, 80), (72, 128), (80, 88)])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_transposed_output_padding(gpu, mode, with_bias, S, ldo):
    """B = 3 batches of S rows: with S = 72 a 64-row tile spans two batches (two-stage kernel: rows_per_batch % 16 != 0), with S = 80 the 192-row ping-pong tile
    spans three.  Columns [S, ldo) of every out[b][n] row hold a sentinel, not zeros, and one more batch of sentinel rows follows the last."""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(S + ldo)
    B, N, K = 3, 320, 320
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x, w = rnd((B, S, K), dt, gpu, g), rnd((N, K), dt, gpu, g, K ** -0.5)
    b = rnd((N,), torch.float32, gpu, g) if with_bias else None
    wp = ops.pack_linear(w, dt, x3=mode == "x3")
    xa = ops.split_pair(x, K) if mode == "x3" else x
    ref = (x.double() @ w.double().t() + (b.double() if with_bias else 0.0)).transpose(1, 2)
    compact, cname = _launch(lambda: ops.linear(xa, wp, b, K=K, rows_per_batch=S, transposed_ld=S))
    big = torch.full((B + 1, N, ldo), SENT, dtype=compact.dtype, device=gpu)
    can = Canary(big)
    _, sname = _launch(lambda: ops.linear(xa, wp, b, K=K, rows_per_batch=S, transposed_ld=ldo, out=big[:B]))
    what = (mode, "transposed", S, ldo, with_bias, sname)
    can.check((slice(0, B), slice(None), slice(0, S)), what)
    rep = Report(f"transposed output {mode} S={S} ldo={ldo} bias={with_bias}")
    _compare(rep, mode, big[:B, :, :S], ref, compact, sname == cname, what)
    rep.show()


# ---------------------------------------------------------------------------------------------------------------------
# 3x3 convolution into the left columns of a concat buffer (unet.py: cat_dst + concat), residual a column view of its own
# ---------------------------------------------------------------------------------------------------------------------
def _cat_window(rows_lead, C1, C2, dtype, gpu):
    """ops.cat_dst with sentinel fill and GUARD rows behind: -> (whole allocation [rows + GUARD, C1 + C2], left column view as cat_dst returns it)"""
    rows = rows_lead[0] * rows_lead[1]
    alloc = torch.full((rows + GUARD, C1 + C2), SENT, dtype=dtype, device=gpu)
    base = alloc[:rows].view(*rows_lead, C1 + C2)
    view = base[..., :C1]
    view._ffn_cat_base = base
    return alloc, view


CONV_CASES = [dict(B=3, H=16, W=16, Cin=128, Cout=320, C2=320, stride=1, up=False),
              dict(B=2, H=8, W=8, Cin=64, Cout=96, C2=64, stride=1, up=False),
              dict(B=3, H=16, W=16, Cin=128, Cout=320, C2=320, stride=2, up=False),
              dict(B=2, H=8, W=8, Cin=64, Cout=96, C2=64, stride=1, up=True)]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"{c['B']}x{c['H']}x{c['W']}-{c['Cin']}-{c['Cout']}-s{c['stride']}{'-up' if c['up'] else ''}")
@pytest.mark.parametrize("mode", MODES)
def test_conv3x3_into_concat_buffer(gpu, mode, case):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    B, H, W, Cin, Cout, C2, stride, up = (case[k] for k in ("B", "H", "W", "Cin", "Cout", "C2", "stride", "up"))
    g = torch.Generator().manual_seed(B + H + Cin + stride)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x, w = rnd((B, H * W, Cin), dt, gpu, g), rnd((Cout, Cin, 3, 3), dt, gpu, g, (9 * Cin) ** -0.5)
    xin = x.double().view(B, H, W, Cin).permute(0, 3, 1, 2)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    b, rb = rnd((Cout,), torch.float32, gpu, g), rnd((B, Cout), torch.float32, gpu, g)
    ref = F.conv2d(xin, w.double(), b.double(), stride=stride, padding=1) + rb.double()[:, :, None, None]
    Ho, Wo = ref.shape[-2:]
    r = rnd((B, Ho * Wo, Cout), dt, gpu, g)
    ref = ref.permute(0, 2, 3, 1).reshape(B, Ho * Wo, Cout) + r.double()
    _, rview = _poisoned(B * Ho * Wo, Cout + 20, 8, r.view(B * Ho * Wo, Cout))
    rview = rview.view(B, Ho * Wo, Cout)
    skip = rnd((B, Ho * Wo, C2), dt, gpu, g)
    wp = ops.pack_conv3x3(w, dt, x3=mode == "x3")
    xa = ops.split_pair(x, Cin) if mode == "x3" else x
    kw = dict(stride=stride, pad=1, upsample=up, Hout=Ho, Wout=Wo, rowbias=rb, splitk=1)
    rep = Report(f"3x3 conv into a concat buffer {mode} {case}")
    for cfg in _configs(lib, mode):
        lib.ffn_igemm_force_config(cfg)
        compact, cname = _launch(lambda: ops.conv3x3(xa, wp, b, B, H, W, Cin, residual=r, **kw))
        alloc, view = _cat_window((B, Ho * Wo), Cout, C2, compact.dtype, gpu)
        can = Canary(alloc)
        _, sname = _launch(lambda: ops.conv3x3(xa, wp, b, B, H, W, Cin, residual=rview, out=view, **kw))
        what = (mode, "cfg", cfg, sname)
        can.check((slice(0, B * Ho * Wo), slice(0, Cout)), what)      # the skip half and the guard rows: untouched BEFORE the concat repairs anything
        _compare(rep, mode, view, ref, compact, sname == cname, what)
        got = view.clone()
        whole = ops.concat(view, skip)
        assert whole.data_ptr() == alloc.data_ptr() and torch.equal(whole, torch.cat([got, skip], dim=-1)), what
        assert (alloc[B * Ho * Wo:] == SENT).all(), what
    rep.show()


def test_fp8_conv3x3_wider_rows(gpu):
    """FFN_FP8: (B, H, W, Cin, Cout) = (3, 32, 32, 128, 320), out a window of rows of 384 bf16, the residual of rows of 340"""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    g = torch.Generator().manual_seed(53)
    B, H, W, Cin, Cout = 3, 32, 32, 128, 320
    x = rnd((B, H * W, Cin), torch.float32, gpu, g).abs_() * 0.7
    w = rnd((Cout, Cin, 3, 3), torch.float32, gpu, g, (9 * Cin) ** -0.5)
    b, rb, r = rnd((Cout,), torch.float32, gpu, g), rnd((B, Cout), torch.float32, gpu, g), rnd((B, H * W, Cout), torch.bfloat16, gpu, g)
    wp = ops.pack_conv3x3_f8(w)
    Cp, alpha = wp._ffn_f8
    wdq = wp.view(torch.float8_e4m3fn).float().reshape(Cout, 3, 3, Cp)[..., :Cin].permute(0, 3, 1, 2).double() * (alpha * ops.F8_ACT_SCALE)
    x8, xdq = _quant_act_f8(x, Cp)
    ref = F.conv2d(xdq.reshape(B, H, W, Cin).permute(0, 3, 1, 2), wdq, b.double(), padding=1).permute(0, 2, 3, 1).reshape(B, H * W, Cout)
    ref = ref + rb.double()[:, None] + r.double()
    _, rview = _poisoned(B * H * W, Cout + 20, 8, r.view(B * H * W, Cout))
    rview = rview.view(B, H * W, Cout)
    rep = Report("fp8 3x3 conv, wider out and residual rows")
    for cfg in _configs(lib, "fp8"):
        lib.ffn_igemm_force_config(cfg)
        for sk in (1, 3):          # (nine K tiles of 128 e4m3 values: three slices of three)
            compact, cname = _launch(lambda: ops.conv3x3(x8, wp, b, B, H, W, Cin, rowbias=rb, residual=r, splitk=sk))
            alloc, view = _cat_window((B, H * W), Cout, 64, torch.bfloat16, gpu)
            can = Canary(alloc)
            _, sname = _launch(lambda: ops.conv3x3(x8, wp, b, B, H, W, Cin, rowbias=rb, residual=rview, out=view, splitk=sk))
            what = ("fp8", "cfg", cfg, "splitk", sk, sname)
            can.check((slice(0, B * H * W), slice(0, Cout)), what)
            _compare(rep, "fp8", view, ref, compact, sname == cname, what)
    rep.show()


# ---------------------------------------------------------------------------------------------------------------------
# conv = 2: the four sub-pixel classes of `nearest-2x upsample -> 3x3 conv`, each into its column block of one [M, 4 Cout (+ canary)] buffer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 12, 20, 64, 256), (1, 16, 12, 128, 320)])
@pytest.mark.parametrize("mode", ["bf16", "x3"])
def test_subpixel_classes_into_column_blocks(gpu, mode, B, H, W, Cin, Cout):
    """what ops.conv3x3_up2x launches (class c at column c * Cout), with 64 canary columns behind the fourth class and GUARD rows behind the last pixel: after
    every class launch only that class's block has changed; the pixel shuffle of the four blocks is the fp64 convolution of the upsampled input (with the
    mode's rounding of the original weights) and, same kernel, ops.conv3x3_up2x's own result bit for bit"""
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    assert ops.up2x_eligible(Cin, Cout, B * H * W)
    g = torch.Generator().manual_seed(B + H + Cin)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x = rnd((B, H * W, Cin), dt, gpu, g)
    w = rnd((Cout, Cin, 3, 3), torch.float32, gpu, g, (9 * Cin) ** -0.5)
    b = rnd((Cout,), torch.float32, gpu, g)
    w4 = ops.pack_conv3x3_up2x(w, dt, x3=mode == "x3")
    xa = ops.split_pair(x, Cin) if mode == "x3" else x
    xr = F.interpolate(x.double().view(B, H, W, Cin).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = F.conv2d(xr, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(B, 4 * H * W, Cout)
    M, ldo = B * H * W, 4 * Cout + 64
    rep = Report(f"sub-pixel classes {mode} {B}x{H}x{W} {Cin}->{Cout}")
    for cfg in _configs(lib, mode):
        lib.ffn_igemm_force_config(cfg)
        compact, cnames = _launch(lambda: ops.conv3x3_up2x(xa, w4, b, B, H, W, Cin))
        big = torch.full((M + GUARD, ldo), SENT, dtype=compact.dtype, device=gpu)
        snames = set()
        for c in range(4):
            can = Canary(big)
            d = L.IgemmDesc()
            d.A, d.W, d.bias = xa.data_ptr(), w4[c * Cout:].data_ptr(), b.data_ptr()
            d.out = big[:, c * Cout:].data_ptr()
            d.M, d.N, d.K, d.Kpad, d.ldo, d.rows_per_batch = M, Cout, 4 * Cin, w4.stride(0), ldo, H * W
            d.lda, d.a_lo, d.x3 = (2 * Cin, 32, 2) if mode == "x3" else (Cin, 0, 0)
            d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride, d.pad = H, W, Cin, H, W, 1, 2 * (1 - (c >> 1)) + (1 - (c & 1))
            d.alpha, d.conv, d.splitk = 1.0, 2, 0
            d.ws, d.ws_bytes = ops._workspace(gpu).data_ptr(), ops.WS_BYTES
            snames.add(_run_desc(lib, L.FFN_BF16X3 if mode == "x3" else L.FFN_BF16, d))
            can.check((slice(0, M), slice(c * Cout, (c + 1) * Cout)), (mode, "cfg", cfg, "class", c))
        got = big[:M, :4 * Cout].reshape(B, H, W, 2, 2, Cout).permute(0, 1, 3, 2, 4, 5).reshape(B, 4 * H * W, Cout)
        _compare(rep, mode, got, ref, compact, sorted(snames) == cnames, (mode, "cfg", cfg, sorted(snames)))
    rep.show()


# ---------------------------------------------------------------------------------------------------------------------
# ops.linear / ops.conv3x3: strides of the tensors they are given
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ops_follow_the_residual_stride_and_refuse_a_strided_conv_input(gpu, dtype):
    """a residual that is a column view of a wider buffer is read with that buffer's row stride (it used to be read as if dense: wrong rows, no error); a conv
    input that is such a view is refused (the gather has no pixel stride)"""
    from freefine_amd import ops
    g = torch.Generator().manual_seed(59)
    M, N, K = 200, 64, 64
    x, w, r = rnd((M, K), dtype, gpu, g), rnd((N, K), dtype, gpu, g, K ** -0.5), rnd((M, N), dtype, gpu, g)
    wide = rnd((M, N + 24), dtype, gpu, g)
    wide[:, 8:8 + N] = r
    out = ops.linear(x, ops.pack_linear(w, dtype), None, K=K, residual=wide[:, 8:8 + N])
    e_lin = relerr(out, x.double() @ w.double().t() + r.double())
    B, H, Cin, Cout = 2, 8, 64, 64
    xc, wc = rnd((B, H * H, Cin), dtype, gpu, g), rnd((Cout, Cin, 3, 3), dtype, gpu, g, (9 * Cin) ** -0.5)
    rc = rnd((B, H * H, Cout), dtype, gpu, g)
    widec = rnd((B, H * H, Cout + 24), dtype, gpu, g)
    widec[..., 8:8 + Cout] = rc
    ref = F.conv2d(xc.double().view(B, H, H, Cin).permute(0, 3, 1, 2), wc.double(), None, padding=1).permute(0, 2, 3, 1).reshape(B, H * H, Cout) + rc.double()
    wpc = ops.pack_conv3x3(wc, dtype)
    e_conv = relerr(ops.conv3x3(xc, wpc, None, B, H, H, Cin, residual=widec[..., 8:8 + Cout]), ref)
    print(f"igemm views strided residual through ops {dtype}: linear {e_lin:.2e}, conv {e_conv:.2e}")
    assert e_lin < tol(dtype) and e_conv < tol(dtype)
    xwide = rnd((B, H * H, Cin + 64), dtype, gpu, g)
    with pytest.raises(AssertionError, match="contiguous"):
        ops.conv3x3(xwide[..., :Cin], wpc, None, B, H, H, Cin)
    with pytest.raises(AssertionError, match="contiguous columns"):
        ops.linear(x, ops.pack_linear(w, dtype), None, K=K, residual=r.t().contiguous().t())
