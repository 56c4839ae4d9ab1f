"""CPU: the C-ABI shared library loads and exports every symbol include/freefine_hip.h declares (no compute calls)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    declared = set(re.findall(r"\b(ffn_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load()
    assert lib.ffn_version() >= 1
    for name in declared:
        assert hasattr(lib, name)


def test_invalid_arguments_are_reported_not_crashed():
    import ctypes
    from freefine_amd import _lib
    lib = _lib.load()
    d = _lib.IgemmDesc()
    assert lib.ffn_igemm(None, 0, ctypes.byref(d)) == -22
    assert b"igemm" in lib.ffn_last_error()
    a = _lib.AttnDesc()
    assert lib.ffn_attn(None, 7, ctypes.byref(a)) == -22


def test_tune_table_roundtrip_and_rejects_foreign_entries(tmp_path):
    """ffn_igemm_tune_export / _import: the tuned (problem -> configuration) table as data.  Entry layout [stamp | key | cfg | splitk]:
    entries with another build's stamp, an unknown configuration or a K split < 1 are skipped (a table written by another build must
    not crash or mis-launch); clear / enable; a tune file that is not a 2-D integer tensor is ignored.  (Whether an
    accepted entry FITS its problem is checked at its first launch, on the GPU: tests/test_ops_gpu.py.)"""
    import torch
    from freefine_amd import _lib, ops
    lib = _lib.load()
    w = lib.ffn_igemm_tune_entry_ints()
    ops.tune_table_clear()
    assert ops.tune_table_export().shape == (0, w)
    t = torch.zeros(4, w, dtype=torch.int32)
    t[:, 0] = lib.ffn_igemm_tune_stamp()
    t[:, 1] = torch.tensor([111, 222, 333, 444]); t[:, 2] = 64; t[:, 3] = 128
    t[:, -2] = torch.tensor([2, lib.ffn_igemm_num_configs() + 5, 0, 2]); t[:, -1] = torch.tensor([1, 1, 0, 1])      # entry 1: unknown cfg; entry 2: split 0
    t[3, 0] ^= 0x100                                                                                                # entry 3: another build's stamp
    assert ops.tune_table_import(t) == 1
    after = ops.tune_table_export()
    assert after.shape[0] == 1 and after[0].tolist() == t[0].tolist()
    f = tmp_path / "tune.pt"
    ops.tune_table_save(str(f))
    assert ops.tune_table_clear() == 1 and ops.tune_table_load(str(f)) == 1
    assert ops.tune_table_load(str(tmp_path / "missing.pt")) == 0
    torch.save({"not": "a table"}, str(tmp_path / "bad.pt"))
    assert ops.tune_table_load(str(tmp_path / "bad.pt")) == 0
    torch.save(torch.zeros(5), str(tmp_path / "bad2.pt"))
    assert ops.tune_table_load(str(tmp_path / "bad2.pt")) == 0
    assert ops.tune_enable(False) is True and ops.tune_enable(True) is False
    ops.tune_table_clear()


def test_controller_plan_tables_host_logic():
    """Attention_Modulator.plan: dispatch + counters mirror the reference protocol (no GPU needed: vectors on CPU)."""
    import torch
    from freefine_amd.attention import Attention_Modulator
    c = Attention_Modulator(start_layer=10)
    c.num_att_layers = 32
    m = torch.zeros(128, 128, dtype=torch.uint8)
    m[30:60, 30:60] = 1
    c.fg_retain_mask = c.fg_ref_mask = c.local_edit_region = m
    c.use_tca, c.method, c.local_edit, c.context_guidance, c.layer_idx = True, "tca", True, 0.5, list(range(10, 16))
    branches = []
    for i in range(32):
        is_cross = bool(i % 2)
        place = "down" if i < 12 else ("mid" if i < 14 else "up")
        branches.append(c.plan("edit", is_cross, place, 4, 64, 2, "cpu")["branch"])
    assert (c.cur_att_layer, c.cur_step) == (0, 1)
    assert branches[0] == "plain" and branches[1] == "cross_local"
    assert [b for b in branches if b.startswith("tca")] == ["tca:tca"] * 6          # blocks 10..15 only
    assert branches[14] == "plain"                                                     # first 'up' self-attn is block 7


def test_legacy_vae_attention_keys_are_renamed_and_bad_checkpoints_fail_clearly():
    """SD-1.5 / SD-2.1 VAE safetensors on the hub name the mid-block attention query/key/value/proj_attn (4-D 1x1 conv weights);
    the loader maps them to to_q/to_k/to_v/to_out.0 like diffusers does, and a checkpoint that does not fit the topology is
    rejected with a message naming the missing parameters."""
    import pytest
    import torch
    from freefine_amd.config import VAEConfig
    from freefine_amd.weights import normalize_state_dict, synthetic_state, vae_param_shapes, validate_state_dict
    shapes = vae_param_shapes(VAEConfig.preset("tiny"))
    st = synthetic_state(shapes, 3)
    legacy = {}
    ren = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    for k, v in st.items():
        for new, old in ren.items():
            if f".attentions.0.{new}." in k:
                k = k.replace(f".{new}.", f".{old}.")
                if v.ndim == 2:
                    v = v[:, :, None, None]
        legacy[k] = v
    assert any(".query.weight" in k for k in legacy) and not any(".to_q." in k for k in legacy)
    fixed = normalize_state_dict(legacy)
    assert set(fixed) == set(st) and all(torch.equal(fixed[k], st[k]) for k in st)
    validate_state_dict(fixed, shapes, "vae")
    broken = dict(fixed)
    broken.pop("decoder.conv_out.bias")
    with pytest.raises(ValueError, match="decoder.conv_out.bias"):
        validate_state_dict(broken, shapes, "vae")


def test_kv64_contract_is_checked_before_any_launch():
    """FFN_IG_OUT_KV64 (round 6): ffn_igemm validates the image-writing epilogue's contract on the host -- wrong arithmetic mode, a boundary that is not a whole
    64-column block, a transposed row stride that is not whole blocks, a residual beside it -- and reports -EINVAL with a message naming the flag (no GPU needed:
    nothing is launched)."""
    import ctypes
    from freefine_amd import _lib
    lib = _lib.load()

    def desc(**kw):
        d = _lib.IgemmDesc()
        d.A = d.W = d.out = 0x10000                   # never dereferenced: validation fails first
        d.M, d.N, d.K, d.Kpad = 4096, 640, 320, 640
        d.lda, d.ldo, d.x3, d.a_lo = 640, 640, 2, 32
        d.rows_per_batch, d.alpha, d.splitk = 4096, 1.0, 1
        d.flags, d.kv64_from = _lib.IG_OUT_KV64, 320
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for dtype, d in ((_lib.FFN_BF16, desc()),                                           # not split-bf16
                     (_lib.FFN_BF16X3, desc(kv64_from=352)),                             # not a 64-column boundary
                     (_lib.FFN_BF16X3, desc(residual=0x20000, ldr=640)),                 # the image cannot carry a residual
                     (_lib.FFN_BF16X3, desc(flags=_lib.IG_OUT_KV64 | _lib.IG_OUT_TRANSPOSED, N=320, ldo=4096 + 8, kv64_from=0))):      # row stride not whole blocks
        assert lib.ffn_igemm(None, dtype, ctypes.byref(d)) == -22
        assert b"KV64" in lib.ffn_last_error(), lib.ffn_last_error()


def test_kv_images_eligibility_rules():
    """ops.kv_images_ok: which self-attention calls may take K / V^T as the pre-split images their projections write (shapes of the one-wave-per-SIMD kernel, no
    degenerate uniform-softmax entry in the plan, buffers the kernels' 32-bit offsets reach)."""
    from freefine_amd import _lib, ops
    km = object()
    ok = [[ops.AttnEntrySpec(0, 1, 0.0, 1.0, kmask=km), ops.AttnEntrySpec(1, 1, 1.0, -1.0)]]
    uni = [[ops.AttnEntrySpec(0, 0, 1.0, 0.0, kmask=km, flags=_lib.ATT_UNIFORM_SEL0)]]
    skipped = [[ops.AttnEntrySpec(0, 0, 0.0, 0.0, kmask=km, flags=_lib.ATT_UNIFORM_SEL1), None]]        # an inactive term does not count
    assert ops.kv_images_ok(64, 4096, 4096) and ops.kv_images_ok(64, 128, 128, ok) and ops.kv_images_ok(64, 1024, 1024, skipped)
    assert not ops.kv_images_ok(64, 1024, 1024, uni)
    assert not ops.kv_images_ok(40, 4096, 4096) and not ops.kv_images_ok(64, 64, 64) and not ops.kv_images_ok(64, 4096, 77)
    assert not ops.kv_images_ok(64, 4096, 4096, None, 2 ** 31)


def test_attention_kernel_choice_table():
    """ffn_attn_kernel_name (nothing is launched: no GPU needed) spells the plan ffn_attn launches from: the kernel of every kind of descriptor,
    ENOSYS for head dims beyond 160 (which ffn_attn refuses), EINVAL for kv_pair (pre-split K / V^T images) on a launch that does not run
    attn_x3w_kernel -- and ops.kv_images_ok gives the library's answer for the split-bf16 kv_pair rows."""
    import ctypes
    from freefine_amd import _lib, ops
    lib = _lib.load()
    F32, BF16, X3 = _lib.FFN_F32, _lib.FFN_BF16, _lib.FFN_BF16X3
    km = object()                                  # stands for a device tensor: only its presence reaches the descriptor
    plain, masked, wq = ops.AttnEntrySpec(0, 0), ops.AttnEntrySpec(0, 0, kmask=km), ops.AttnEntrySpec(0, 0, wq=km)
    uniform = ops.AttnEntrySpec(0, 0, 1.0, 0.0, kmask=km, flags=_lib.ATT_UNIFORM_SEL1)

    def name(dtype, D, S, Sk, passes, kv_pair=0):
        heads = 5
        d = _lib.AttnDesc()
        d.Bo, d.S, d.Sk, d.heads, d.D, d.npass, d.kv_pair = len(passes[0]), S, Sk, heads, D, len(passes), kv_pair
        d.ldq = d.ldk = d.ldo = heads * D
        d.ldvt = Sk
        for p, rows in enumerate(passes):
            for b, sp in enumerate(rows):
                e = d.e[p * _lib.ATT_MAXB + b]
                if sp is not None:
                    e.q_row, e.kv_row, e.w_const, e.w_slope, e.flags = sp.q_row, sp.kv_row, sp.w_const, sp.w_slope, sp.flags
                    e.kmask, e.wq = (0 if sp.kmask is None else 0x10000), (0 if sp.wq is None else 0x20000)
        buf = ctypes.create_string_buffer(160)
        rc = lib.ffn_attn_kernel_name(dtype, ctypes.byref(d), buf, 160)
        return buf.value.decode() if rc == 0 else rc
    rows = [
        (F32, 40, 1024, 77, [[plain]], 0, "attn_kernel<float, 48, 2, 64, 1, true>"),
        (F32, 64, 4096, 4096, [[masked]], 0, "attn_kernel<float, 64, 2, 64, 1, true>"),
        (F32, 80, 1024, 77, [[plain]], 0, "attn_kernel<float, 80, 2, 64, 1, true>"),
        (F32, 160, 1024, 77, [[plain]], 0, "attn_kernel<float, 160, 1, 32, 1, true>"),
        (F32, 200, 1024, 77, [[plain]], 0, -38),
        (X3, 80, 1024, 1024, [[plain]], 0, "attn_kernel<float, 80, 2, 64, 1, true>"),
        (BF16, 64, 4096, 77, [[plain]], 0, "xattn_kernel<5>"),
        (BF16, 64, 4096, 30, [[plain]], 0, "xattn_kernel<2>"),
        (BF16, 64, 1024, 77, [[plain, wq]], 0, "xattn_mp_kernel<5>"),
        (BF16, 64, 1024, 96, [[plain, None], [plain, plain]], 0, "xattn_mp_kernel<6>"),
        (BF16, 64, 4096, 4096, [[plain]], 0, "attn_pp_kernel<false>"),
        (BF16, 64, 4096, 4096, [[masked]], 0, "attn_pp_kernel<true>"),
        (BF16, 64, 4096, 4096, [[uniform]], 0, "attn_kernel<bf16, 64, 2, 64, 2, true>"),
        (BF16, 80, 1024, 77, [[plain]], 0, "attn_kernel<bf16, 96, 2, 64, 1, false>"),
        (BF16, 160, 1024, 77, [[masked]], 0, "attn_kernel<bf16, 160, 1, 64, 1, true>"),
        (BF16, 200, 1024, 77, [[plain]], 0, -38),
        (X3, 64, 1024, 77, [[plain]], 0, "xattn_x3_kernel<5, 4>"),
        (X3, 64, 4096, 77, [[plain]], 0, "xattn_x3_kernel<5, 8>"),
        (X3, 64, 1024, 30, [[plain], [plain]], 0, "xattn_x3_kernel<2, 8>"),
        (X3, 64, 4096, 4096, [[masked]], 0, "attn_x3p_kernel<true>"),
        (X3, 64, 1024, 1024, [[plain]], 0, "attn_x3p_kernel<false>"),
        (X3, 64, 1024, 77, [[masked]], 0, "attn_x3_kernel<true>"),
        (X3, 40, 1024, 1024, [[plain]], 0, "attn_x3_kernel<false>"),
        (X3, 64, 1024, 1024, [[uniform]], 0, "attn_x3_kernel<true>"),
        (X3, 64, 4096, 4096, [[masked, plain], [plain, None]], 1, "attn_x3w_kernel<true>"),
        (X3, 64, 128, 128, [[plain]], 1, "attn_x3w_kernel<false>"),
        (X3, 64, 1024, 1024, [[uniform]], 1, -22),
        (X3, 40, 4096, 4096, [[plain]], 1, -22),
        (X3, 64, 4096, 77, [[plain]], 1, -22),
        (X3, 64, 64, 128, [[plain]], 1, -22),
        (X3, 64, 1024, 64, [[plain]], 1, -22),
        (BF16, 64, 4096, 4096, [[plain]], 1, -22),
        (F32, 200, 1024, 1024, [[plain]], 1, -22),
    ]
    for dtype, D, S, Sk, passes, kv_pair, want in rows:
        got = name(dtype, D, S, Sk, passes, kv_pair)
        assert (got == want) if isinstance(want, int) else (got == f"void {want}({'ffn_attn_desc, int, int' if 'xattn' in want else 'ffn_attn_desc'})"), \
            (dtype, D, S, Sk, kv_pair, got, want)
        if want == -22:
            assert b"kv_pair" in lib.ffn_last_error(), lib.ffn_last_error()
        if dtype == X3 and kv_pair:
            assert ops.kv_images_ok(D, S, Sk, passes) == (got != -22), (D, S, Sk, got)


def test_igemm_kernel_choice_table():
    """ffn_igemm_kernel_name (nothing is launched: no GPU needed, the CU count falls back to 256) spells the plan ffn_igemm launches from.  Rule-based
    rows: the names the library gave before the choice was gathered into one plan, pasted in -- they must not change.  Forced rows: under
    ffn_igemm_force_config the name is that configuration's kernel wherever the configuration is a candidate for the problem, else the rule's.  Error
    rows: a descriptor ffn_igemm refuses gets the same code and message from both entry points."""
    import ctypes
    from freefine_amd import _lib
    lib = _lib.load()
    F32, BF16, X3, F8 = _lib.FFN_F32, _lib.FFN_BF16, _lib.FFN_BF16X3, _lib.FFN_FP8
    TR, GEGLU, KV64 = _lib.IG_OUT_TRANSPOSED, _lib.IG_GEGLU, _lib.IG_OUT_KV64

    def desc(M, N, K, conv=0, hw=32, x3=0, **kw):
        d = _lib.IgemmDesc()
        d.A = d.W = d.out = 0x10000                   # never dereferenced
        d.M, d.N, d.K, d.Kpad, d.lda, d.ldo, d.rows_per_batch, d.alpha = M, N, K, K, K, N, M, 1.0
        if conv:                                      # hw x hw images, stride 1, K = taps * Cin
            taps = 9 if conv == 1 else 4
            d.conv, d.Cin, d.lda, d.Hin, d.Win, d.Hout, d.Wout, d.stride, d.pad, d.rows_per_batch = conv, K // taps, K // taps, hw, hw, hw, hw, 1, 1, hw * hw
        if x3:                                        # 2: blocked operands, 1: planes
            d.x3, d.a_lo, d.lda, d.Kpad = x3, (32 if x3 == 2 else d.lda), 2 * d.lda, (2 if x3 == 2 else 3) * K
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def name(dtype, d):
        buf = ctypes.create_string_buffer(200)
        rc = lib.ffn_igemm_kernel_name(dtype, ctypes.byref(d), buf, 200)
        return buf.value.decode() if rc == 0 else rc

    def glds(t, bm, bn, amode, swap, nwm, nwn, fastk=False, x3=False, f8=False):
        f = lambda v: "true" if v else "false"
        return f"void igemm_glds_kernel<{t}, {bm}, {bn}, {amode}, {f(swap)}, 2, {nwm}, {nwn}, {f(fastk)}, {f(x3)}, {f(f8)}>(ffn_igemm_desc)"

    def pp(bm, bn, amode, res=False, geglu=False, split=False, trans=False, x3=False, f8=False):
        f = lambda v: "true" if v else "false"
        return f"void igemm_pp_kernel<{bm}, {bn}, {amode}, {f(res)}, {f(geglu)}, {f(split)}, {f(trans)}, {f(x3)}, {f(f8)}>(ffn_igemm_desc, int)"
    lib.ffn_igemm_tune_clear()
    lib.ffn_igemm_force_config(-1)
    rows = [
        (F32, desc(64, 320, 320), "igemm_glds_kernel<float, 64, 64, 0, true, 2, 2, 2, false, false, false>"),      # f32 dense: M = 64, 512, 4096 (the rule gives
        (F32, desc(512, 320, 320), "igemm_glds_kernel<float, 128, 64, 0, true, 2, 4, 2, false, false, false>"),      # unsplit dense problems of M >= 128 the 128x64 tile)
        (F32, desc(4096, 320, 320), "igemm_glds_kernel<float, 128, 64, 0, true, 2, 4, 2, false, false, false>"),
        (F32, desc(2048, 320, 576, conv=1), "igemm_glds_kernel<float, 64, 64, 1, true, 2, 2, 2, false, false, false>"),      # f32 3x3 convolution
        (F32, desc(65536, 320, 576, conv=1), "igemm_glds_kernel<float, 128, 128, 1, true, 2, 2, 4, false, false, false>"),      # ... and one large enough for 128x128
        (BF16, desc(65536, 320, 320), "igemm_pp_kernel<256, 320, 0, false, false, false, false, false, false>"),      # bf16 dense on the ping-pong tile: plain,
        (BF16, desc(65536, 320, 320, residual=0x20000, ldr=320), "igemm_pp_kernel<256, 320, 0, true, false, false, false, false, false>"),      # with residual,
        (BF16, desc(16384, 2560, 320, flags=GEGLU, ldo=1280), "igemm_pp_kernel<256, 256, 0, false, true, false, false, false, false>"),      # GEGLU
        (BF16, desc(4096, 320, 72), "igemm_glds_kernel<bf16, 128, 64, 0, true, 2, 4, 2, false, false, false>"),      # K % 64 != 0: no streaming loader
        (BF16, desc(64, 320, 320), "igemm_glds_kernel<bf16, 64, 64, 0, true, 2, 2, 2, true, false, false>"),      # small M
        (BF16, desc(65536, 320, 1152, conv=1), "igemm_pp_kernel<256, 320, 1, false, false, false, false, false, false>"),      # 3x3 convolution on a ping-pong tile
        (BF16, desc(3072, 320, 1152, conv=1), "igemm_glds_kernel<bf16, 64, 64, 1, true, 2, 2, 2, true, false, false>"),      # ... below the 3/4-fill rule
        (BF16, desc(2048, 320, 512, conv=2, pad=3), "igemm_pp_kernel<256, 320, 1, false, false, false, false, false, false>"),      # 2x2 convolution
        (BF16, desc(4096, 320, 320, flags=TR, ldo=4096), "igemm_pp_kernel<192, 320, 0, false, false, false, true, false, false>"),      # transposed: ping-pong tile,
        (BF16, desc(4096, 320, 64, flags=TR, ldo=4096), "igemm_glds_kernel<bf16, 128, 64, 0, false, 2, 4, 2, false, false, false>"),      # generic fallback (K = 64)
        (X3, desc(65536, 320, 320, x3=2), "igemm_pp_kernel<256, 320, 0, false, false, false, false, true, false>"),      # split-bf16, blocked operands: dense,
        (X3, desc(65536, 320, 1152, conv=1, x3=2), "igemm_pp_kernel<256, 320, 1, false, false, false, false, true, false>"),      # 3x3 convolution,
        (X3, desc(4096, 320, 320, x3=2, flags=TR, ldo=4096), "igemm_pp_kernel<192, 320, 0, false, false, false, true, true, false>"),      # transposed,
        (X3, desc(4096, 640, 320, x3=2, flags=KV64, kv64_from=320), "igemm_glds_kernel<bf16, 128, 64, 0, true, 2, 4, 2, false, true, false>"),      # KV64,
        (X3, desc(65536, 128, 1152, conv=1, x3=2), "igemm_pp_kernel<256, 128, 1, false, false, false, false, true, false>"),      # the 256x128 tile
        (X3, desc(4096, 320, 24, x3=1), "igemm_glds_kernel<bf16, 128, 64, 0, true, 2, 4, 2, false, true, false>"),      # split-bf16, planes
        (F8, desc(65536, 320, 1152, conv=1, alpha=0.25), "igemm_pp_kernel<256, 320, 1, false, false, false, false, false, true>"),      # fp8 3x3 convolution
        (BF16, desc(600, 512, 4096, splitk=8, ws=0x30000, ws_bytes=1 << 30), "igemm_glds_kernel<bf16, 128, 128, 0, true, 2, 4, 4, true, false, false>"),      # caller-forced split-K
    ]
    for dtype, d, want in rows:
        assert name(dtype, d) == f"void {want}({'ffn_igemm_desc, int' if 'igemm_pp' in want else 'ffn_igemm_desc'})", (dtype, d.M, d.N, d.K, d.conv, d.flags, want)
    # forced rows: one 3x3 stride-1 convolution, B = 3, 32x32, Cin = 128, N = 320.  kCfg of csrc/capi_igemm.hip: (BM, BN, NWM, NWN), then the halo
    # kernel's four tiles and the ping-pong kernel's five.  Every generic and halo tile is a candidate (M = 3072 is whole tiles of whole image
    # rows); of the ping-pong tiles the two 320 columns wide (N % 256 != 0; the 256x128 tile is for split-bf16 problems)
    kcfg = [(64, 64, 2, 2), (128, 64, 4, 2), (128, 128, 2, 4), (128, 128, 4, 4), (256, 128, 4, 4), (256, 256, 4, 4), (128, 320, 4, 4), (128, 160, 4, 2), (192, 320, 3, 4),
            (128, 320, 4, 4), (256, 128, 4, 4), (256, 256, 4, 4), (128, 128, 4, 4),
            (256, 320, 2, 4), (256, 256, 2, 4), (192, 320, 2, 4), (192, 256, 2, 4), (256, 128, 2, 4)]
    assert lib.ffn_igemm_num_configs() == len(kcfg)
    conv = desc(3072, 320, 1152, conv=1)
    rule = name(BF16, conv)
    try:
        for cfg, (bm, bn, nwm, nwn) in enumerate(kcfg):
            lib.ffn_igemm_force_config(cfg)
            if cfg < 9:
                want = glds("bf16", bm, bn, 1, True, nwm, nwn, fastk=True)
            elif cfg < 13:
                want = f"void igemm_halo_kernel<bf16, {bm}, {bn}, {nwm}, {nwn}>(ffn_igemm_desc, int)"
            else:
                want = pp(bm, bn, 1) if bn == 320 else rule
            assert name(BF16, conv) == want, cfg
    finally:
        lib.ffn_igemm_force_config(-1)
    for dtype, d, msg in [(BF16, desc(2048, 320, 576, conv=1, flags=TR), b"transposed output is only supported for dense A"),
                          (BF16, desc(4096, 2560, 320, flags=GEGLU, ldo=1280, residual=0x20000, ldr=1280), b"GEGLU epilogue is exclusive"),
                          (BF16, desc(2048, 384, 512, conv=2), b"fits no ping-pong tile"),
                          (BF16, desc(4096, 320, 320, Kpad=312), b"Kpad=312")]:
        assert name(dtype, d) == -22
        text = lib.ffn_last_error()
        assert msg in text and text.startswith(b"igemm: "), text
        assert lib.ffn_igemm(None, dtype, ctypes.byref(d)) == -22 and lib.ffn_last_error() == text


def test_igemm_strides_and_residual_alignment_are_checked_before_any_launch():
    """include/freefine_hip.h, "Strides and alignment of ffn_igemm_desc": a row stride shorter than what a row holds (lda < K, ldo < the columns written, ldr < N)
    and a residual pointer off the alignment its loads need are refused with FFN_EINVAL by ffn_igemm (the strides by ffn_igemm_kernel_name too) -- nothing is
    launched, no GPU needed.  Control rows: the same descriptors with the smallest admitted values are accepted, among them ldo % 8 == 4 and ldr % 8 == 4 in bf16 (row starts
    8 bytes apart)."""
    import ctypes
    from freefine_amd import _lib
    lib = _lib.load()
    F32, BF16, X3, F8 = _lib.FFN_F32, _lib.FFN_BF16, _lib.FFN_BF16X3, _lib.FFN_FP8
    TR, GEGLU = _lib.IG_OUT_TRANSPOSED, _lib.IG_GEGLU

    def desc(M=584, N=320, K=320, **kw):
        d = _lib.IgemmDesc()
        d.A = d.W = d.out = 0x10000                   # never dereferenced
        d.M, d.N, d.K, d.Kpad, d.lda, d.ldo, d.rows_per_batch, d.alpha, d.splitk = M, N, K, K, K, N, M, 1.0, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def conv8(**kw):                                  # an fp8 3x3 convolution, 3 images of 32 x 32 x 128
        return desc(3072, 320, 1152, conv=1, Cin=128, lda=128, Hin=32, Win=32, Hout=32, Wout=32, stride=1, pad=1, rows_per_batch=1024, alpha=0.25, **kw)

    def name_rc(dtype, d):
        return lib.ffn_igemm_kernel_name(dtype, ctypes.byref(d), ctypes.create_string_buffer(200), 200)
    lib.ffn_igemm_force_config(-1)
    refused = [(BF16, desc(lda=312), b"lda=312"), (F32, desc(lda=316), b"lda=316"),
               (BF16, desc(ldo=316), b"ldo=316"), (F32, desc(ldo=316), b"ldo=316"), (X3, desc(x3=2, a_lo=32, lda=640, Kpad=640, ldo=316), b"ldo=316"),
               (BF16, desc(N=640, flags=GEGLU, ldo=316), b"ldo=316"),
               (BF16, desc(M=216, rows_per_batch=72, flags=TR, ldo=68), b"transposed ldo=68"), (F32, desc(M=216, rows_per_batch=72, flags=TR, ldo=68), b"transposed ldo=68"),
               (BF16, desc(residual=0x20000, ldr=316), b"ldr=316"), (X3, desc(x3=2, a_lo=32, lda=640, Kpad=640, residual=0x20000, ldr=316), b"ldr=316"),
               (F8, conv8(ldo=316), b"igemm(fp8): ldo=316"), (F8, conv8(residual=0x20000, ldr=316), b"igemm(fp8): ldr=316")]
    for dtype, d, msg in refused:
        assert name_rc(dtype, d) == -22 and msg in lib.ffn_last_error(), (dtype, msg, lib.ffn_last_error())
        assert lib.ffn_igemm(None, dtype, ctypes.byref(d)) == -22 and msg in lib.ffn_last_error(), (dtype, msg, lib.ffn_last_error())
    accepted = [(BF16, desc()), (F32, desc()), (BF16, desc(lda=328, Kpad=384, ldo=324, residual=0x20000, ldr=324)), (BF16, desc(N=640, flags=GEGLU, ldo=320)),
                (BF16, desc(M=216, rows_per_batch=72, flags=TR, ldo=72)), (BF16, desc(M=40, rows_per_batch=72, flags=TR, ldo=40)),
                (F8, conv8(ldo=324, residual=0x20000, ldr=324))]
    for dtype, d in accepted:
        assert name_rc(dtype, d) == 0, (dtype, lib.ffn_last_error())
    # pointer alignment is ffn_igemm's own check (ffn_igemm_kernel_name looks at no buffer): it comes after the shape checks and before the launch
    for dtype, d, msg in [(BF16, desc(residual=0x20004, ldr=320), b"bf16 residual must be 8-byte aligned"),
                          (F8, conv8(residual=0x20004, ldr=320), b"igemm(fp8): bf16 residual must be 8-byte aligned"),
                          (F32, desc(residual=0x20008, ldr=320), b"fp32 residual must be 16-byte aligned"),
                          (X3, desc(x3=2, a_lo=32, lda=640, Kpad=640, residual=0x20008, ldr=320), b"fp32 residual must be 16-byte aligned")]:
        assert name_rc(dtype, d) == 0
        assert lib.ffn_igemm(None, dtype, ctypes.byref(d)) == -22 and msg in lib.ffn_last_error(), (dtype, msg, lib.ffn_last_error())


def test_attention_row_split_minimises_resident_rounds():
    """ops.attn_row_split: rows per launch of a self-attention call on the one-workgroup-per-CU kernels (256 CUs): never more than FFN_ATT_MAXB, never more rounds
    than the fixed 16-row split, the documented cases, every row covered once."""
    from freefine_amd import _lib, ops
    M = _lib.ATT_MAXB

    def rounds(Bo, w, n, cus=256):
        full, rest = divmod(Bo, n)
        return full * -(-n * w // cus) + (-(-rest * w // cus) if rest else 0)
    assert ops.attn_row_split(72, 80, M, 256) == 16 and rounds(72, 80, 16) == 23
    assert ops.attn_row_split(72, 40, M, 256) == 12 and rounds(72, 40, 12) == 12 and rounds(72, 40, 16) == 14
    assert ops.attn_row_split(72, 20, M, 256) == 12 and rounds(72, 20, 12) == 6 and rounds(72, 20, 16) == 9
    assert ops.attn_row_split(48, 80, M, 256) == 16
    for Bo in (1, 2, 3, 7, 16, 17, 24, 48, 72, 96, 100):
        for w in (5, 20, 40, 80, 180):
            n = ops.attn_row_split(Bo, w, M, 256)
            assert 1 <= n <= min(M, Bo) and rounds(Bo, w, n) <= rounds(Bo, w, min(M, Bo))
