"""CPU: what FID rests on besides the kernels.  tests/inception_ref.py's four FID blocks against the reference's own classes (tests/golden/g20_fid_blocks.npz,
tools/gen_golden.py run_g20: which pool stands in front of branch_pool, the concatenation order); the host-side BatchNorm folding against un-folded conv + BN
in fp64; the layer tables of both configurations against the topology and against the restatement's own table; the state-dict errors; the command line; the
parse_data quirk; the refusals of the four C entries (nothing is launched: no GPU needed)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_fid_blocks_equal_the_reference_classes():
    G = np.load(os.path.join(ROOT, "tests", "golden", "g20_fid_blocks.npz"))
    for kind in ("A", "C", "E1", "E2"):
        arg = int(G[f"{kind}/arg"])
        state = IR.seeded_state(IR.block_shapes(kind, int(G[f"{kind}/cin"]), None if arg < 0 else arg), int(G[f"{kind}/seed"]))
        for j in range(2):
            x, y = torch.from_numpy(G[f"{kind}/x{j}"]), torch.from_numpy(G[f"{kind}/y{j}"])
            got = IR.fid_block(kind, state, x)
            assert got.shape == y.shape and (got - y).abs().max().item() <= 1e-12, (kind, j)
    # the two E blocks differ in nothing but the pool: on the same state and input they must disagree, and only in the branch_pool columns
    state = IR.seeded_state(IR.block_shapes("E1", 16), 5)
    x = torch.randn(1, 16, 5, 4, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    a, b = IR.fid_block("E1", state, x), IR.fid_block("E2", state, x)
    assert torch.equal(a[:, :-192], b[:, :-192]) and not torch.equal(a[:, -192:], b[:, -192:])


def test_batchnorm_folding_equals_conv_then_batchnorm_in_fp64():
    from freefine_amd import inception as I
    state = IR.seeded_state(IR.network_shapes("tiny"), 11)
    g = torch.Generator().manual_seed(11)
    for conv in I.all_convs("tiny"):
        if conv.name not in ("Conv2d_1a_3x3", "Mixed_5b.branch5x5_2", "Mixed_6b.branch7x7_2", "Mixed_6b.branch7x7dbl_2", "Mixed_7a.branch3x3_2", "Mixed_7c.branch3x3_2b"):
            continue
        x = torch.randn(2, conv.cin, 9, 8, generator=g, dtype=torch.float64)
        w64, b64 = I.fold_batchnorm64(state, conv)
        want = IR.basic_conv(state, conv.name, x, conv.stride, conv.pad)
        got = F.relu(F.conv2d(x, w64, b64, conv.stride, conv.pad))
        assert (got - want).abs().max().item() <= 1e-12, conv.name
        # the packed fp32 form: columns (ky, kx, ci), the stem's fourth input column zero, one rounding from the fp64 values
        w32, b32 = I.fold_batchnorm(state, conv)
        cin4 = -(-conv.cin // 4) * 4
        assert w32.dtype == torch.float32 and tuple(w32.shape) == (conv.cout, conv.k[0] * conv.k[1] * cin4)
        w4 = w32.view(conv.cout, conv.k[0], conv.k[1], cin4)
        assert torch.equal(w4[..., :conv.cin], w64.permute(0, 2, 3, 1).float()) and (w4[..., conv.cin:] == 0).all() and torch.equal(b32, b64.float())


def test_layer_tables_of_both_configurations():
    from freefine_amd import inception as I
    want_out = {"full": [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048], "tiny": [32, 36, 36, 96, 96, 96, 96, 96, 160, 256, 256]}
    for config in ("full", "tiny"):
        stem, blocks = I.layer_table(config)
        assert [b[1] for b in blocks] == ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c"]
        assert [b[0] for b in blocks] == ["A", "A", "A", "B", "C", "C", "C", "C", "D", "E1", "E2"]
        assert [b[3] for b in blocks] == want_out[config]
        assert all(blocks[i + 1][2] == blocks[i][3] for i in range(len(blocks) - 1)) and blocks[0][2] == stem[-1].cout
        convs = I.all_convs(config)
        assert len(convs) == 94
        for c in convs:
            assert c.cout % 4 == 0 and (c.cin % 4 == 0 or c.name == "Conv2d_1a_3x3"), c.name
            assert c.k[0] in (1, 3, 5, 7) and c.k[1] in (1, 3, 5, 7) and c.stride in (1, 2)
        ref = IR.network_shapes(config)          # the restatement's own table, written separately
        assert [c.name for c in convs] == list(ref) and all(ref[c.name] == (c.cout, c.cin) + c.k for c in convs)
    full = {c.name: c for c in I.all_convs("full")}
    assert (full["Conv2d_1a_3x3"].cin, full["Conv2d_1a_3x3"].cout, full["Conv2d_1a_3x3"].stride) == (3, 32, 2)
    assert (full["Conv2d_3b_1x1"].cout, full["Conv2d_4a_3x3"].cout, full["Conv2d_2b_3x3"].pad) == (80, 192, (1, 1))
    c = full["Mixed_5b.branch5x5_2"]
    assert (c.cin, c.cout, c.k, c.pad) == (48, 64, (5, 5), (2, 2)) and full["Mixed_5b.branch_pool"].cout == 32 and full["Mixed_5c.branch_pool"].cout == 64
    c = full["Mixed_6a.branch3x3"]
    assert (c.cin, c.cout, c.k, c.stride, c.pad) == (288, 384, (3, 3), 2, (0, 0))
    assert [full[f"Mixed_6{x}.branch7x7_1"].cout for x in "bcde"] == [128, 160, 160, 192]
    c, d = full["Mixed_6c.branch7x7_2"], full["Mixed_6c.branch7x7dbl_2"]
    assert (c.k, c.pad, d.k, d.pad) == ((1, 7), (0, 3), (7, 1), (3, 0)) and full["Mixed_6c.branch7x7dbl_5"].cout == 192
    c = full["Mixed_7a.branch3x3_2"]
    assert (c.cin, c.cout, c.stride) == (192, 320, 2) and full["Mixed_7a.branch7x7x3_4"].stride == 2
    c = full["Mixed_7c.branch3x3dbl_2"]
    assert (c.cin, c.cout, c.k, c.pad) == (448, 384, (3, 3), (1, 1)) and full["Mixed_7c.branch1x1"].cin == 2048 and full["Mixed_7b.branch1x1"].cin == 1280
    assert (full["Mixed_7b.branch3x3_2a"].k, full["Mixed_7b.branch3x3_2a"].pad, full["Mixed_7b.branch3x3_2b"].k) == ((1, 3), (0, 1), (3, 1))
    assert [I.width(c, "tiny") for c in (32, 48, 64, 80, 96, 192, 288, 320, 384, 448)] == [4, 8, 8, 12, 12, 24, 36, 40, 48, 56]


def test_state_dict_errors_name_the_key_and_foreign_entries_are_ignored():
    from freefine_amd import inception as I
    state = IR.seeded_state(IR.network_shapes("tiny"), 3, torch.float32)
    packed = I.pack_state("tiny", state)
    extra = dict(state, **{"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008), "Conv2d_1a_3x3.bn.num_batches_tracked": torch.tensor(0),
                           "AuxLogits.conv0.conv.weight": torch.zeros(4, 4, 1, 1)})
    again = I.pack_state("tiny", extra)
    assert set(again) == set(packed) and all(torch.equal(again[k][0], packed[k][0]) and torch.equal(again[k][1], packed[k][1]) for k in packed)
    for key in ("Mixed_6c.branch7x7dbl_4.conv.weight", "Mixed_7c.branch_pool.bn.running_var", "Conv2d_1a_3x3.bn.bias"):
        broken = dict(state)
        broken.pop(key)
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            I.pack_state("tiny", broken)
        broken[key] = torch.zeros(tuple(state[key].shape) + (2,))
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            I.pack_state("tiny", broken)
    with pytest.raises(ValueError, match="Conv2d_1a_3x3.conv.weight"):          # the full network's state does not fit the tiny one
        I.pack_state("tiny", {k: torch.zeros((32, 3, 3, 3) if k == "Conv2d_1a_3x3.conv.weight" else tuple(v.shape)) for k, v in state.items()})
    with pytest.raises(ValueError, match="configuration"):
        I.layer_table("huge")


def test_command_line_fid_options_and_answers_without_weights(tmp_path):
    import importlib.util
    from test_consistency_cpu import load_driver
    drv = load_driver()
    args = drv.build_parser().parse_args(["--path", "x.json", "--fid_weights", "w.pth", "--fid_config", "tiny"])
    assert args.fid_weights == "w.pth" and args.fid_config == "tiny"
    assert drv.build_parser().parse_args(["--path", "x.json"]).fid_weights is None and drv.build_parser().parse_args(["--path", "x.json"]).fid_config == "full"
    with pytest.raises(SystemExit):
        drv.build_parser().parse_args(["--path", "x.json", "--fid_config", "huge"])
    assert "--fid_weights" in drv.__doc__ and "fp32" in drv.build_parser().format_help().split("--precision")[-1]
    path = str(tmp_path / "results.json")
    json.dump({"a": {"instances": {"0": {}}}}, open(path, "w"))
    res = drv.main(["--path", path, "--task", "100000000"])
    assert list(res) == ["FID"] and "not built" in res["FID"] and "--fid_weights" in res["FID"]
    res = drv.main(["--path", path, "--task", "100000000", "--fid_weights", str(tmp_path / "missing.pth")])      # no --fid_path: the file is not opened
    assert "not built" in res["FID"]
    res = drv.main(["--path", path, "--task", "100000000", "--fid_path", str(tmp_path)])
    assert "not built" in res["FID"] and set(drv.NOT_BUILT) == {"FID", "IRS"}
    spec = importlib.util.spec_from_file_location("ffn_metrics_fid", os.path.join(ROOT, "evaluation", "metrics", "FID", "fid.py"))      # the reference's import path
    fid = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fid)
    from freefine_amd import metrics as FM
    assert fid.calculate_fid is FM.calculate_fid and fid.parse_data is FM.parse_data


def test_calculate_fid_reads_the_directory_listing_and_is_the_frechet_distance_of_its_activations(tmp_path):
    """the reference's parse_data quirk: the real set is os.listdir(real_root_path), not the samples' ori_img_path.  A stand-in extractor (three channel means and
    a gradient) keeps this on the host."""
    from PIL import Image
    from freefine_amd import metrics as FM
    rng = np.random.default_rng(0)
    real = tmp_path / "real"
    real.mkdir()

    def write(path, h, w):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)
        return str(path)
    listing = [write(real / f"r{i}.png", 9 + i, 12) for i in range(6)]
    elsewhere = write(tmp_path / "source.png", 8, 8)
    gen = [write(tmp_path / f"g{i}.png", 10, 7 + i % 2) for i in range(7)]
    data = {"img": {"instances": {"0": {f"c{i}": {"ori_img_path": elsewhere, "gen_img_path": g} for i, g in enumerate(gen)}}}}

    class Means:
        seen = []

        def features_u8(self, images):
            self.seen.append(images.shape)
            x = images.astype(np.float64)
            return np.concatenate([x.mean((1, 2)), x[:, -1].mean((1, 2))[:, None] - x[:, 0].mean((1, 2))[:, None]], 1)
    model = Means()
    value = FM.calculate_fid(data, "gen_img_path", str(real), model, batch_size=3)
    r, g = FM.parse_data(data, "gen_img_path", str(real))
    assert sorted(r) == sorted(listing) and elsewhere not in r and g == gen
    fr, fg = FM.get_inception_activations(r, model, 3), FM.get_inception_activations(g, model, 3)
    assert fr.dtype == np.float64 and fr.shape == (6, 4) and fg.shape == (7, 4)
    for files, f in ((r, fr), (g, fg)):          # file order kept across sizes and batches
        for p, row in zip(files, f):
            assert np.allclose(row[:3], np.asarray(Image.open(p).convert("RGB"), np.float64).mean((0, 1)), rtol=0, atol=1e-9)
    want = FM.frechet_distance(fr.mean(0), np.cov(fr, rowvar=False), fg.mean(0), np.cov(fg, rowvar=False))
    assert value == want and np.isfinite(value)
    assert all(s[0] <= 3 for s in model.seen)


def test_inception_entries_are_declared_and_refuse_before_any_launch():
    from freefine_amd import _lib
    lib = _lib.load()
    assert lib.ffn_version() >= 16
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    for name in ("ffn_conv2d", "ffn_pool2d", "ffn_mean_hw", "ffn_fid_prep"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    unit = [u for u, _ in __import__("__graft_entry__").UNITS]
    assert "inception.hip" in unit
    p = 0x10000                                       # never dereferenced

    def desc(**kw):
        d = _lib.Conv2dDesc()
        d.x = d.w = d.out = p
        d.B, d.Hin, d.Win, d.Cin, d.N, d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.ldx, d.ldo, d.Kpad, d.flags = 2, 17, 17, 160, 160, 7, 1, 1, 3, 0, 160, 160, 1120, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for kw, word in ((dict(Cin=158), b"Cin=158"), (dict(N=162), b"N=162"), (dict(KH=4), b"kernel 4 x 1"), (dict(KW=9), b"kernel 7 x 9"), (dict(stride=3), b"stride=3"),
                     (dict(pad_h=-1), b"padding"), (dict(ldx=156), b"ldx=156"), (dict(ldo=156), b"ldo=156"), (dict(ldx=162), b"ldx=162"), (dict(Kpad=1116), b"Kpad=1116"),
                     (dict(Kpad=1122), b"Kpad=1122"), (dict(x=p + 4), b"16-byte"), (dict(out=p + 8), b"16-byte"), (dict(w=p + 4), b"16-byte"), (dict(bias=p + 4), b"16-byte"),
                     (dict(x=None), b"null"), (dict(flags=4), b"flags"), (dict(Hin=3, pad_h=1), b"does not fit"), (dict(B=0), b"bad shape")):
        assert lib.ffn_conv2d(None, _lib.FFN_F32, ctypes.byref(desc(**kw))) == -22, kw
        msg = lib.ffn_last_error()
        assert msg.startswith(b"conv2d: ") and word in msg, (kw, msg)
    for dtype in (_lib.FFN_BF16, _lib.FFN_BF16X3, _lib.FFN_FP8):
        assert lib.ffn_conv2d(None, dtype, ctypes.byref(desc())) == -38
    assert lib.ffn_pool2d(None, 1, p, p, 1, 8, 8, 6, 8, 8, 3, 1, 1) == -22 and b"C=6" in lib.ffn_last_error()
    assert lib.ffn_pool2d(None, 5, p, p, 1, 8, 8, 8, 8, 8, 3, 1, 1) == -22 and b"unknown op" in lib.ffn_last_error()
    assert lib.ffn_pool2d(None, 0, p, p, 1, 8, 8, 8, 8, 8, 3, 2, 2) == -22 and b"pad=2" in lib.ffn_last_error()
    assert lib.ffn_mean_hw(None, p, p, 1, 64, 2046, 2048) == -22 and b"C=2046" in lib.ffn_last_error()
    assert lib.ffn_fid_prep(None, p, p, p + 4, 1, 224, 299) == -22 and b"16-byte" in lib.ffn_last_error()
    assert lib.ffn_fid_prep(None, p, p, p, 1, 224, 5000) == -22 and b"FFN_IMGPREP_MAX_SIDE" in lib.ffn_last_error()
