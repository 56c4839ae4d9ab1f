"""CPU: click-to-mask as far as it runs without a device -- tests/sam_ref.py (the project's restatement of EfficientSAM) pinned to what the reference's source
computes on seeded weights (tests/golden/g16_efficient_sam.npz, tools/gen_golden.py::run_g16), the state layout and its refusals, the click rules, the ABI entries
and their refusals, the command line.  The device: tests/test_sam_gpu.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import sam_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ffn_sam_patch_rows", "ffn_sam_patch_rows_pair", "ffn_hyper_masks", "ffn_upsample_bicubic")
_G16 = {}


def g16():
    if not _G16:
        _G16.update(np.load(os.path.join(ROOT, "tests", "golden", "g16_efficient_sam.npz")))
    return _G16


def golden_view(name, out):
    """the arrays of sam_ref's output that the golden holds for this case, cut the way run_g16 cut them: key -> tensor"""
    if name.startswith("vits"):
        return {"iou": out["iou"], "emb": out["emb"][:, ::8, ::8], "low": out["low"][:, :, 0, ::4, ::4]}
    return {"iou": out["iou"], "emb": out["emb"], "low": out["low"], "full_best": out["full"][0, 0, 0]}


@pytest.mark.parametrize("name", list(SR.G16_CASES))
def test_restatement_equals_the_reference_golden(name):
    """every G16 array within 1e-9 of its maximum (measured while recording: 3e-15 at most)"""
    G = g16()
    cfg, state, img, pts, lab = SR.g16_inputs(name, int(G["seed_" + SR.G16_CASES[name][0]]))
    out = SR.sam_ref(cfg, state, img, pts, lab, "f64")
    for key, got in golden_view(name, out).items():
        want = torch.as_tensor(G[f"{name}/{key}"])
        assert got.shape == want.shape, (name, key, got.shape, want.shape)
        e = ((got - want).abs().max() / want.abs().max()).item()
        print(f"{name} {key}: {e:.2e} of the maximum")
        assert e <= 1e-9, (name, key, e)
    # the sort order is the reference's sorted_ids, and no matter of rounding (the recording conditions hold in the restatement)
    assert torch.equal(out["order"], torch.as_tensor(G[name + "/order"]))
    assert (out["iou"][..., :-1] - out["iou"][..., 1:]).min() >= 1e-2


@pytest.mark.parametrize("cname", ["tiny", "vits"])
def test_shapes_equal_the_reference_state_dict(cname):
    from freefine_amd import sam
    want = {ln.split(" ")[0]: tuple(int(d) for d in ln.split(" ")[1:]) for ln in g16()["keys_" + cname].tolist()}
    got = {k: tuple(v) for k, v in sam.sam_shapes(sam.sam_config(cname)).items()}
    assert got == want, set(got.items()) ^ set(want.items())
    assert list(got) == [ln.split(" ")[0] for ln in g16()["keys_" + cname].tolist()]        # and in the state_dict's order
    st = sam.synthetic_state(sam.sam_config(cname), 3)
    assert {k: tuple(v.shape) for k, v in st.items()} == want and all(v.dtype == torch.float32 for v in st.values())


def test_configurations():
    from freefine_amd import sam
    s, t, y = sam.sam_config("vits"), sam.sam_config("vitt"), sam.sam_config("tiny")
    assert (s.img_size, s.patch, s.depth, s.embed_dim, s.num_heads, s.neck, s.dec_heads, s.dec_mlp, s.up_dims, s.iou_hidden) == (1024, 16, 12, 384, 6, 256, 8, 2048, (64, 32), 256)
    assert (t.embed_dim, t.num_heads, t.depth) == (192, 3, 12)
    assert (y.img_size, y.embed_dim, y.num_heads, y.depth, y.neck, y.dec_heads, y.up_dims) == (128, 128, 2, 2, 64, 2, (32, 16))
    for c in (s, t, y):        # encoder head dim 64; decoder head dims 32 (self) and 16 (cross) at every size
        assert c.embed_dim // c.num_heads == 64 and c.neck // c.dec_heads == 32 and c.neck // c.attn_down // c.dec_heads == 16
    with pytest.raises(ValueError, match="vitx"):
        sam.sam_config("vitx")


def test_state_is_checked_strictly_and_both_layouts_are_accepted():
    from freefine_amd import sam
    cfg = sam.sam_config("tiny")
    sd = sam.synthetic_state(cfg, 1)
    assert sam.check_state(cfg, sd) is sd and sam.check_state(cfg, {"model": sd}) is sd
    k = "mask_decoder.transformer.layers.1.norm4.bias"
    with pytest.raises(KeyError, match=re.escape(k)):
        sam.check_state(cfg, {a: b for a, b in sd.items() if a != k})
    with pytest.raises(KeyError, match="image_encoder.cls_token"):
        sam.check_state(cfg, dict(sd, **{"image_encoder.cls_token": torch.zeros(1)}))
    with pytest.raises(ValueError, match=re.escape(k)):
        sam.check_state(cfg, dict(sd, **{k: torch.zeros(65)}))
    with pytest.raises(ValueError, match="x3"):
        sam.HipEfficientSam(cfg, sd, dtype=torch.bfloat16, x3=True, device="cpu")
    with pytest.raises(KeyError):              # refused before anything touches a device
        sam.HipEfficientSam(cfg, {}, device="cpu")


def test_prompts_are_rescaled_padded_and_cut():
    from freefine_amd import sam
    cfg = sam.sam_config("tiny")
    pts, lab = sam.prepare_prompts(cfg, [[[[10, 20], [-1, -1]]]], [[[1, -1]]], (64, 256))
    assert pts.shape == (1, 6, 2) and lab.shape == (1, 6) and pts.dtype == torch.float32
    assert pts[0, 0].tolist() == [10 * 128 / 256, 20 * 128 / 64] and pts[0, 1:].eq(-1).all() and lab[0].tolist() == [1, -1, -1, -1, -1, -1]
    p7, l7 = SR.g16_prompts((200, 136), "q2")
    pts, lab = sam.prepare_prompts(cfg, p7, l7, (200, 136))
    assert pts.shape == (2, 6, 2) and lab.shape == (2, 6) and lab[1].tolist() == [1, 1, -1, 1, 1, 1] and pts[1, 2].tolist() == [-1, -1]
    assert torch.equal(pts[0], torch.stack([p7[0, 0, :6, 0] * 128 / 136, p7[0, 0, :6, 1] * 128 / 200], dim=-1))


def test_box_from_clicks_on_the_four_click_orders():
    from src.demo.utils import box_from_clicks
    want = ((10, 20), (30, 40))
    for p1, p2 in (((10, 20), (30, 40)), ((10, 40), (30, 20)), ((30, 20), (10, 40)), ((30, 40), (10, 20))):
        assert box_from_clicks(p1, p2) == want
    assert box_from_clicks((5, 7), (5, 7)) == ((5, 7), (5, 7))


def test_segment_with_box_hands_corner_labels_to_the_model():
    from src.demo import utils as U
    seen = {}

    class Model:
        def segment(self, image, points, labels):
            seen.update(points=np.asarray(points).tolist(), labels=np.asarray(labels).tolist())
            return np.zeros(image.shape[:2], np.uint8)
    m = U.segment_with_box(Model(), np.zeros((8, 9, 3), np.uint8), (6, 1), (2, 5))
    assert m.shape == (8, 9) and seen == {"points": [[2, 1], [6, 5]], "labels": [2, 3]}


def test_entries_are_declared_bound_and_exported():
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", header) and name in _lib.SYMBOLS, name
    assert re.search(r"FFN_ELT_GELU\s*=\s*2", header) and _lib.ELT_GELU == 2
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfreefine_hip.so not built")
    lib = _lib.load()
    assert lib.ffn_version() >= 11
    for name in ENTRIES:
        assert hasattr(lib, name)


def test_bad_arguments_are_refused_before_any_launch():
    """no GPU needed: validation comes first.  Null pointers, zero sizes, a side above FFN_IMGPREP_MAX_SIDE."""
    from freefine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfreefine_hip.so not built")
    lib = _lib.load()
    p, big = 0x10000, _lib.IMGPREP_MAX_SIDE + 1                  # never dereferenced
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    ok = dict(B=1, H=8, W=8, side=32, patch=16, cols=768)

    def rows(pair=False, src=p, out=p, mean=f3, std=f3, **kw):
        a = dict(ok, **kw)
        if pair:
            return lib.ffn_sam_patch_rows_pair(None, src, out, a["B"], a["H"], a["W"], a["side"], a["patch"], a["cols"], mean, std)
        return lib.ffn_sam_patch_rows(None, _lib.FFN_F32, src, out, a["B"], a["H"], a["W"], a["side"], a["patch"], a["cols"], mean, std)
    for pair in (False, True):
        assert rows(pair, src=None) == -22 and b"null" in lib.ffn_last_error()
        assert rows(pair, out=None) == -22 and rows(pair, mean=None) == -22 and rows(pair, std=None) == -22
        for bad in (dict(B=0), dict(H=0), dict(W=0), dict(side=0), dict(patch=0), dict(side=40), dict(cols=760)):
            assert rows(pair, **bad) == -22, (pair, bad)
        for bad in (dict(H=big), dict(W=big), dict(side=big)):
            assert rows(pair, **bad) == -22 and b"FFN_IMGPREP_MAX_SIDE" in lib.ffn_last_error(), (pair, bad)
        assert rows(pair, std=(ctypes.c_float * 3)(0.5, 0.0, 0.5)) == -22 and b"std" in lib.ffn_last_error()
    assert lib.ffn_sam_patch_rows(None, _lib.FFN_BF16X3, p, p, 1, 8, 8, 32, 16, 768, f3, f3) == -22 and b"dtype" in lib.ffn_last_error()
    assert rows(True, cols=780) == -22 and b"multiple of 8" in lib.ffn_last_error()
    assert rows(True, out=p + 4) == -22 and b"aligned" in lib.ffn_last_error()
    for args in ((None, p, p, 1, 64, 32, 4), (p, None, p, 1, 64, 32, 4), (p, p, None, 1, 64, 32, 4), (p + 4, p, p, 1, 64, 32, 4), (p, p, p, 0, 64, 32, 4), (p, p, p, 1, 0, 32, 4),
                 (p, p, p, 1, 64, 0, 4), (p, p, p, 1, 64, 30, 4), (p, p, p, 1, 64, 68, 4), (p, p, p, 1, 64, 32, 0), (p, p, p, 1, 64, 32, 9), (p, p, p, 65536, 64, 32, 4)):
        assert lib.ffn_hyper_masks(None, *args) == -22 and b"hyper_masks" in lib.ffn_last_error(), args
    for args in ((None, p, p, 1, 8, 8, 8, 8), (p, None, p, 1, 8, 8, 8, 8), (p, p, None, 0, 8, 8, 8, 8), (p, p, None, 1, 0, 8, 8, 8), (p, p, None, 1, 8, 8, 8, 0),
                 (p, p, None, 1, big, 8, 8, 8), (p, p, None, 1, 8, 8, 8, big), (p, p, None, 65536, 8, 8, 8, 8)):
        assert lib.ffn_upsample_bicubic(None, *args) == -22 and b"upsample_bicubic" in lib.ffn_last_error(), args
    assert lib.ffn_upsample_bicubic(None, p, p, None, 1, 8, big, 8, 8) == -22 and b"FFN_IMGPREP_MAX_SIDE" in lib.ffn_last_error()
    assert lib.ffn_eltwise(None, _lib.FFN_F32, 3, p, None, p, 4) == -22 and lib.ffn_eltwise(None, _lib.FFN_F32, _lib.ELT_GELU, None, None, p, 4) == -22


def test_segment_tool_rejects_a_missing_box_or_point(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import segment
    base = ["--image", "a.png", "--weights", "synthetic:tiny", "--out", "m.png"]
    for extra in ([], ["--box", "1", "2", "3", "4", "--point", "5", "6"], ["--box", "1", "2", "3"]):
        with pytest.raises(SystemExit) as e:
            segment.parse(base + extra)
        assert e.value.code == 2
    assert "--box" in capsys.readouterr().err
    cli = segment.parse(base + ["--point", "5", "6", "--point", "7", "8", "--precision", "x3"])
    assert cli.point == [[5.0, 6.0], [7.0, 8.0]] and cli.box is None and cli.precision == "x3"
    assert segment.parse(base + ["--box", "9", "2", "3", "4"]).box == [9.0, 2.0, 3.0, 4.0]
