"""Every 3x3 convolution kernel on the geometries production reaches and the even, square, power-of-two images of test_ops_gpu.py do not: odd and non-square
images, one-pixel-wide and one-pixel-high ones, images smaller than a tile (a tile spans dozens of them, every pixel a border pixel), rows per image that
neither divide nor are divided by the tile height, stride 2 from odd sizes, right / bottom-only padding, the fused nearest-2x upsample at y0 = -1, halo tiles
of widths other than 16 / 32 (conv_geometry_cases.py lists the classes A .. G and the channel counts).

Method:
  exact pass      the operands are small integers (conv_geometry_cases.py; tests/test_conv_geometry_ref_cpu.py proves the preconditions): whatever the summation
                  order, the K split or the hi / lo split, a kernel that addresses the right pixels gives the fp64 reference bit for bit, so the assertion is
                  torch.equal(got, ref.to(got.dtype)) for EVERY kernel and mode -- no kernel is held to a tolerance instead.  (igemm_pp_kernel rounds
                  fl(bias + sum) where the others round fl(fl(sum) + bias): both are exact here.)  A failure names the kernel launched, mode, configuration and
                  the first mismatching (image, yo, xo, n) with their border class;
  Gaussian pass   integer data cannot show a mix-up of the hi and lo planes (lo = 0): every case and mode also runs once on rnd() data, unforced and on every
                  halo / ping-pong configuration, at the gates of test_ops_gpu.py (tol(dtype), X3_TOL);
  reference       fp64, on the CPU, once per case and epilogue, never per configuration;
  canaries        the output is a window (ldo = N + 8) of a sentinel-filled buffer with 300 guard rows behind row M: everything outside keeps its bits;
  poison          x lies inside a NaN-filled allocation (e4m3: 0x7f), NaN before image 0 and behind the last: a tap at y = -1 of image 0 or y = H of the last
                  image that is not turned into padding shows as NaN;
  configurations  bf16 / split-bf16 / fp8 cases run unforced and under ffn_igemm_force_config(cfg) for every cfg (fp32 is planned by rule: once), the K split
                  pinned (1, or 3 for the split-K cases).  First-use timing is off for the file, so ffn_igemm_kernel_name names the kernel launched;
  eligibility     conv_geometry_cases.halo_eligible / pp_eligible restate halo_bytes_for / pp_ok of csrc/capi_igemm.hip: a forced halo / ping-pong configuration must
                  run exactly where they say and must be refused (the launch then lands on igemm_glds_kernel) where they do not -- row bias below 128 rows
                  per image (class D), the halo of a 256-wide row piece (class E);
  ledger          every test ends by asserting that each kernel form ran on its class (REQUIRED), and that every generic tile was really launched: a forced
                  configuration that falls back everywhere fails instead of passing.  One line per form with the number of geometries is printed."""
import collections
import re

import pytest
import torch

import conv_geometry_cases as G
from conv_geometry_cases import CASES, N4_CASES, UP2X_CASES, VARIANTS
from test_igemm_views_gpu import Canary, _bits, _configs, _launch
from test_ops_gpu import X3_TOL, _IGEMM_CFG_TILES, _quant_act_f8, relerr, rnd, tol

pytestmark = pytest.mark.gpu

SENT, GUARD, PADC = 7.0, 300, 8
MODES = ["f32", "bf16", "x3", "f8"]
GENERIC_WAVES = [(2, 2), (4, 2), (2, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 2), (3, 4)]          # kCfg of csrc/capi_igemm.hip: wave grid of the nine generic tiles
WIDE = ["256x320", "192x320", "256x256", "192x256"]
LEDGER = collections.defaultdict(set)          # (class, form) -> geometries, over the whole file


@pytest.fixture(autouse=True)
def _rule_based_choice(gpu):
    from freefine_amd import _lib as L
    lib = L.load()
    prev = lib.ffn_igemm_tune_enable(0)
    yield
    lib.ffn_igemm_tune_enable(prev)
    lib.ffn_igemm_force_config(-1)


def required(cls, mode):
    """the kernel forms that must have run on class `cls` in `mode`"""
    split = [f"ping-pong split-K {mode}"] if cls in G.SPLIT_CLASSES else []
    if mode == "f32":
        return ["ring recomputing fp32"]
    if mode == "bf16":
        halo = [f"halo {bm}x{bn}" for bm, bn in G.HALO_CFGS.values()] if cls == "E" else []
        return ["ring recomputing bf16 (Cin % 64 != 0)", "ring streaming (fastk)"] + halo + [f"ping-pong bf16 {t}" for t in WIDE] + split
    if mode == "x3":
        return ["ring recomputing split-bf16 planes", "ring recomputing split-bf16 blocks"] + [f"ping-pong split-bf16 {t}" for t in WIDE + ["256x128"]] + split
    return ["ring recomputing fp8"] + [f"ping-pong fp8 {t}" for t in WIDE] + split


def form_of(name, cin, mode):
    kind, args = re.match(r"void igemm_(glds|halo|pp)_kernel<(.*)>\(", name).groups()
    a = [s.strip() for s in args.split(",")]
    if kind == "halo":
        return f"halo {a[1]}x{a[2]}"
    if kind == "pp":
        assert (a[7] == "true") == (mode == "x3") and (a[8] == "true") == (mode == "f8"), name
        if a[5] == "true":
            return f"ping-pong split-K {mode}"
        return f"ping-pong {'split-bf16' if mode == 'x3' else ('fp8' if mode == 'f8' else 'bf16')} {a[0]}x{a[1]}"
    assert (a[0] == "float") == (mode == "f32") and (a[9] == "true") == (mode == "x3") and (a[10] == "true") == (mode == "f8"), name
    if a[8] == "true":
        return "ring streaming (fastk)"
    if mode == "x3":
        return "ring recomputing split-bf16 " + ("planes" if cin % 32 else "blocks")
    if mode == "bf16":
        assert cin % 64, (name, "whole 64-channel chunks take the streaming loader (igemm_plan, csrc/capi_igemm.hip)")
        return "ring recomputing bf16 (Cin % 64 != 0)"
    return "ring recomputing " + ("fp32" if mode == "f32" else "fp8")


class Ledger:
    def __init__(self, cls, mode):
        self.cls, self.mode, self.forms, self.generic, self.refused, self.launches = cls, mode, collections.defaultdict(set), set(), collections.Counter(), 0

    def add(self, name, geo, cin, cfg):
        form = form_of(name, cin, self.mode)
        self.forms[form].add(geo)
        LEDGER[(self.cls, form)].add(geo)
        self.launches += 1
        if 0 <= cfg < 9:
            bm, bn = _IGEMM_CFG_TILES[cfg]
            if re.search(rf"glds_kernel<\w+, {bm}, {bn}, 1, true, 2, {GENERIC_WAVES[cfg][0]}, {GENERIC_WAVES[cfg][1]},", name):
                self.generic.add(cfg)

    def close(self):
        for form in sorted(self.forms):
            print(f"conv geometry ledger: class {self.cls} {self.mode:4s} {form:42s} {len(self.forms[form]):2d} geometries")
        for why, n in sorted(self.refused.items()):
            print(f"conv geometry ledger: class {self.cls} {self.mode:4s} refused, ran igemm_glds_kernel instead: {why}: {n} launches")
        missing = [f for f in required(self.cls, self.mode) if not self.forms.get(f)]
        assert not missing, (self.cls, self.mode, "kernel forms that never ran", missing)
        if self.mode != "f32":          # every generic tile the mode has was really launched under its forced configuration
            want = set(range(9)) if self.mode == "bf16" else {0, 1, 2}
            assert self.generic >= want, (self.cls, self.mode, "forced generic configurations that fell back everywhere", sorted(want - self.generic))
        if self.mode != "f32" and self.cls == "D":
            assert self.refused["row bias below 128 rows per image on a ping-pong tile"] > 0
        if self.mode == "bf16" and self.cls == "E":
            assert self.refused["halo of a 256-wide row piece (3 x 258 slots)"] > 0


def poisoned(t, guard):
    """t (contiguous) inside a NaN-filled allocation with >= `guard` elements of NaN on either side -> the view that holds t's values"""
    guard = (guard + 63) // 64 * 64
    buf = torch.full((t.numel() + 2 * guard,), 0x7f if t.dtype == torch.uint8 else float("nan"), dtype=t.dtype, device=t.device)
    view = buf[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


Operands = collections.namedtuple("Operands", "xa wp bias rb res odt xref wref")


def prepare(mode, o, gpu, Cin, Cout, guard_pix, pack=None):
    """the device operands of a mode from CPU fp32 x [B, HW, Cin], w [Cout, Cin, 3, 3], bias, rb, res; xref / wref: the fp64 values the kernel is given"""
    from freefine_amd import ops
    pack = pack or ops.pack_conv3x3
    x, w = o["x"].to(gpu), o["w"].to(gpu)
    if mode == "f32":
        xa, wp, odt, xref, wref = x, pack(w, torch.float32), torch.float32, x, w
    elif mode == "bf16":
        xa, wq = x.to(torch.bfloat16), w.to(torch.bfloat16)
        wp, odt, xref, wref = pack(wq, torch.bfloat16), torch.bfloat16, xa, wq
    elif mode == "x3":
        xa, wp, odt, xref, wref = ops.split_pair(x, Cin), pack(w, torch.float32, x3=True), torch.float32, x, w
    else:
        wp = ops.pack_conv3x3_f8(w)
        cp, alpha = wp._ffn_f8
        wref = wp.view(torch.float8_e4m3fn).float().reshape(Cout, 3, 3, cp)[..., :Cin].permute(0, 3, 1, 2) * (alpha * ops.F8_ACT_SCALE)
        xa, xref = _quant_act_f8(x, cp)
        odt = torch.bfloat16
    xp = poisoned(xa, guard_pix * xa.shape[-1])
    if mode == "x3":
        ops._mark_pair(xp, Cin)
    res = o["res"].to(gpu).to(odt)
    return Operands(xp, wp, o["bias"].to(gpu), o["rb"].to(gpu), res, odt, xref.double().cpu(), wref.double().cpu())


def expect_kernel(c, mode, variant, cfg, name, led):
    """a forced halo / ping-pong configuration runs exactly where csrc/capi_igemm.hip's rules admit it; everything else these small problems run is igemm_glds_kernel"""
    for table, pred, kern in ((G.HALO_CFGS, G.halo_eligible, "igemm_halo_kernel<bf16, "), (G.PP_CFGS, G.pp_eligible, "igemm_pp_kernel<")):
        if cfg in table:
            bm, bn = table[cfg]
            want, runs = pred(c, mode, variant, bm, bn), f"{kern}{bm}, {bn}, " in name
            assert want == runs, (G.case_id(c), mode, variant, "cfg", cfg, "eligible by the rule" if want else "not eligible by the rule", "but launched", name)
            if want:
                assert (c.splitk > 1) == form_of(name, c.Cin, mode).startswith("ping-pong split-K"), (G.case_id(c), "splitk", c.splitk, name)
                return
            if table is G.PP_CFGS and VARIANTS[variant][0] and G.rows(c) < 128 and G.pp_eligible(c, mode, "plain", bm, bn):
                led.refused["row bias below 128 rows per image on a ping-pong tile"] += 1
            if table is G.HALO_CFGS and bm == 256 and c.W % 256 == 0 and mode == "bf16" and c.Cin % 64 == 0:
                led.refused["halo of a 256-wide row piece (3 x 258 slots)"] += 1
    assert "igemm_glds_kernel<" in name, (G.case_id(c), mode, variant, "cfg", cfg, name)


def check_canary(can, M, N, what):
    changed = _bits(can.buf) != can.snap
    changed[:M, :N] = False
    if changed.any():
        at = changed.nonzero()[:4].tolist()
        raise AssertionError((what, "written outside the window", [(m, n, "pixel behind M" if m >= M else "column behind N") for m, n in at]))


def check_equal(got, ref, M, ho, wo, what):
    if torch.equal(got, ref):
        return
    bad = got != ref
    rows_, first = ho * wo, []
    for b, r in bad.any(-1).nonzero()[:6].tolist():          # the first mismatching pixels, each with its first mismatching channel
        n = int(bad[b, r].nonzero()[0])
        first.append((G.border_class(b * rows_ + r, M, ho, wo), "n", n, "got", got[b, r, n].item(), "ref", ref[b, r, n].item()))
    nan = bool(torch.isnan(got).any())
    raise AssertionError((what, "NaN in the result: a read outside the tensor" if nan else "wrong value",
                          f"{int(bad.sum())} of {got.numel()} elements in {int(bad.any(-1).sum())} of {M} pixels differ; the first (image, yo, xo, class):", first))


def run_conv(ops, c, P, variant, out):
    rb, res, relu = VARIANTS[variant]
    kw = dict(stride=c.stride, pad=c.pad, upsample=c.up, out=out, rowbias=P.rb if rb else None, residual=P.res if res else None, relu=relu, splitk=c.splitk)
    if c.pad == 0:
        kw["Hout"], kw["Wout"] = G.out_size(c.H, c.W, c.stride, c.pad, c.up)
    _, names = _launch(lambda: ops.conv3x3(P.xa, P.wp, P.bias, c.B, c.H, c.W, c.Cin, **kw))
    assert len(names) == 1, names
    return names[0]


def window(big, B, rows_, N):
    return big[:B * rows_].view(B, rows_, N + PADC)[..., :N]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cls", list(G.GEOMETRIES))
def test_exact_on_integer_operands(gpu, cls, mode):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    led = Ledger(cls, mode)
    for c in (c for c in CASES if c.cls == cls and mode in c.modes):
        o = G.case_operands(c)
        P = prepare(mode, o, gpu, c.Cin, c.Cout, 2 * c.W + 4)
        assert torch.equal(P.xref, o["x"].double()) and torch.equal(P.wref, o["w"].double()), (G.case_id(c), mode, "the mode's encoding changed an integer operand")
        ho, wo = G.out_size(c.H, c.W, c.stride, c.pad, c.up)
        rows_, M, N = ho * wo, c.B * ho * wo, c.Cout
        big = torch.empty(M + GUARD, N + PADC, dtype=P.odt, device=gpu)
        for variant in c.variants:
            ref = G.case_ref(c, o, variant).to(gpu).to(P.odt)          # once per case and epilogue
            for cfg in _configs(lib, mode):
                lib.ffn_igemm_force_config(cfg)
                big.fill_(SENT)
                can = Canary(big)
                out = window(big, c.B, rows_, N)
                name = run_conv(ops, c, P, variant, out)
                what = (G.case_id(c), mode, variant, "cfg", cfg, name)
                expect_kernel(c, mode, variant, cfg, name, led)
                check_canary(can, M, N, what)
                check_equal(out, ref, M, ho, wo, what)
                led.add(name, (c.B, c.H, c.W, c.stride, c.pad, c.up), c.Cin, cfg)
    print(f"conv geometry exact pass: class {cls} {mode}: {led.launches} launches, all torch.equal to the fp64 reference")
    led.close()


def gaussian_operands(B, HW, Cin, Cout, out_rows, mode, odt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, Cin, generator=g)
    if mode == "f8":
        x = x.abs() * 0.7          # SiLU-like range, as test_fp8_conv3x3
    return dict(x=x, w=torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5, bias=torch.randn(Cout, generator=g), rb=torch.randn(B, Cout, generator=g),
                res=torch.randn(B, out_rows, Cout, generator=g).to(odt).float())


def gate(mode):
    return X3_TOL if mode == "x3" else tol(torch.float32 if mode == "f32" else torch.bfloat16)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cls", list(G.GEOMETRIES))
def test_gaussian_pass(gpu, cls, mode):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    worst, n = 0.0, 0
    for c in (c for c in CASES if c.cls == cls and mode in c.modes):
        odt = torch.float32 if mode in ("f32", "x3") else torch.bfloat16
        o = gaussian_operands(c.B, c.H * c.W, c.Cin, c.Cout, G.rows(c), mode, odt, G.seed_of(99, c.B, c.H, c.W, c.Cin, c.Cout, c.stride))
        P = prepare(mode, o, gpu, c.Cin, c.Cout, 2 * c.W + 4)
        variant = c.variants[-1]
        ref = G.case_ref(c, o, variant, x=P.xref, w=P.wref)
        ho, wo = G.out_size(c.H, c.W, c.stride, c.pad, c.up)
        big = torch.empty(c.B * ho * wo + GUARD, c.Cout + PADC, dtype=P.odt, device=gpu)
        for cfg in [-1] + ([] if mode == "f32" else sorted(G.HALO_CFGS) + sorted(G.PP_CFGS)):
            lib.ffn_igemm_force_config(cfg)
            big.fill_(SENT)
            out = window(big, c.B, ho * wo, c.Cout)
            name = run_conv(ops, c, P, variant, out)
            assert not torch.isnan(out).any(), (G.case_id(c), mode, "cfg", cfg, name, "NaN in the result: a read outside the tensor")
            err = relerr(out, ref)
            worst, n = max(worst, err), n + 1
            assert err < gate(mode), (G.case_id(c), mode, variant, "cfg", cfg, name, err)
    print(f"conv geometry Gaussian pass: class {cls} {mode}: worst relerr {worst:.2e} over {n} launches (gate {gate(mode):.1e})")


# ---------------------------------------------------------------------------------------------------------------------
# class F: conv3x3_up2x (conv = 2, four sub-pixel classes + pixel shuffle) against upsample -> conv in fp64
# ---------------------------------------------------------------------------------------------------------------------
def conv2_tile(M, N, cfg):
    """csrc/capi_igemm.hip: a forced ping-pong configuration where the tile applies (N % bn == 0, M >= bm; the 128-column tile never), else conv2_tile's first"""
    if cfg in G.PP_CFGS and G.PP_CFGS[cfg][1] != 128 and N % G.PP_CFGS[cfg][1] == 0 and M >= G.PP_CFGS[cfg][0]:
        return G.PP_CFGS[cfg]
    return next((bm, bn) for bn in (320, 256) for bm in (256, 192) if N % bn == 0 and M >= bm)


@pytest.mark.parametrize("mode", ["bf16", "x3"])
def test_subpixel_upsample_conv_at_odd_sizes(gpu, mode):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    tiles = collections.defaultdict(set)
    for B, H, W, Cin, Cout in UP2X_CASES:
        assert ops.up2x_eligible(Cin, Cout, B * H * W)
        for real in (False, True):
            odt = torch.float32 if mode == "x3" else torch.bfloat16
            o = gaussian_operands(B, H * W, Cin, Cout, 4 * H * W, mode, odt, G.seed_of(98, B, H, W, Cin)) if real else \
                G.integer_operands(B, H, W, Cin, Cout, 4 * H * W, G.seed_of(70, B, H, W, Cin, Cout))
            P = prepare(mode, o, gpu, Cin, Cout, 2 * W + 4, pack=ops.pack_conv3x3_up2x)
            ref = G.conv_ref(P.xref, o["w"].double(), o["bias"], B, H, W, 1, 1, True)          # (the ORIGINAL weights: the four-tap sums are the kernel's business)
            refd = ref.to(gpu).to(P.odt)
            M4 = 4 * B * H * W
            big = torch.empty(M4 + GUARD, Cout + PADC, dtype=P.odt, device=gpu)
            for cfg in _configs(lib, mode):
                lib.ffn_igemm_force_config(cfg)
                big.fill_(SENT)
                can = Canary(big)
                out = window(big, B, 4 * H * W, Cout)
                _, names = _launch(lambda: ops.conv3x3_up2x(P.xa, P.wp, P.bias, B, H, W, Cin, out=out))
                bm, bn = conv2_tile(B * H * W, Cout, cfg)
                what = ("conv3x3_up2x", (B, H, W, Cin, Cout), mode, "gaussian" if real else "integer", "cfg", cfg, names)
                assert len(names) == 1 and f"igemm_pp_kernel<{bm}, {bn}, " in names[0] and form_of(names[0], Cin, mode).startswith("ping-pong"), what
                check_canary(can, M4, Cout, what)
                if real:
                    assert not torch.isnan(out).any() and relerr(out, ref) < gate(mode), (what, relerr(out, ref))
                else:
                    check_equal(out, refd, M4, 2 * H, 2 * W, what)
                    tiles[f"{bm}x{bn}"].add((B, H, W))
                    LEDGER[("F", f"conv == 2 {mode} {bm}x{bn}")].add((B, H, W))
    for t in sorted(tiles):
        print(f"conv geometry ledger: class F {mode:4s} conv == 2 on the {t} ping-pong tile: {len(tiles[t])} geometries")
    assert set(tiles) == set(WIDE), (mode, "conv == 2 tiles that never ran", set(WIDE) - set(tiles))


# ---------------------------------------------------------------------------------------------------------------------
# class G: conv3x3_n4_kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,Cin", N4_CASES)
def test_conv3x3_n4_on_degenerate_images(gpu, dtype, B, H, W, Cin):
    from freefine_amd import _lib as L
    from freefine_amd import ops
    lib = L.load()
    npix = B * H * W
    for real in (False, True):
        o = gaussian_operands(B, H * W, Cin, 4, H * W, "n4", dtype, G.seed_of(97, B, H, W, Cin)) if real else G.integer_operands(B, H, W, Cin, 4, H * W, G.seed_of(71, B, H, W, Cin))
        x = poisoned(o["x"].to(gpu).to(dtype), (2 * W + 4) * Cin)
        w4, bias = ops.pack_conv3x3_n4(o["w"].to(gpu)), o["bias"].to(gpu)
        ref = G.conv_ref(x.double().cpu(), o["w"], o["bias"], B, H, W, 1, 1, False)
        big = torch.full((npix + GUARD, 4), SENT, dtype=torch.float32, device=gpu)
        can = Canary(big)
        L.check(lib.ffn_conv3x3_n4(ops._stream(), ops._dt(x), x.data_ptr(), w4.data_ptr(), bias.data_ptr(), big.data_ptr(), B, H, W, Cin), "ffn_conv3x3_n4")
        what = ("conv3x3_n4_kernel", (B, H, W, Cin), dtype, "gaussian" if real else "integer")
        check_canary(can, npix, 4, what)
        out = big[:npix].view(B, H * W, 4)
        if real:
            assert not torch.isnan(out).any() and relerr(out, ref) < 2e-6, (what, relerr(out, ref))          # (the gate of test_conv3x3_n4_direct)
        else:
            check_equal(out, ref.to(gpu).float(), npix, H, W, what)
    LEDGER[("G", f"conv3x3_n4_kernel {'fp32' if dtype == torch.float32 else 'bf16'}")].add((B, H, W))


def test_ledger_of_the_whole_file(gpu):
    """what ran, one line per class and kernel form; every (class, mode) test above has asserted its own part"""
    for (cls, form), geos in sorted(LEDGER.items()):
        print(f"conv geometry ledger, whole file: class {cls} {form:42s} {len(geos):2d} geometries")
