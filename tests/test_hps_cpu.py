"""CPU: the Human Preference Score (freefine_amd.hps) as far as it runs without a device -- fp64 restatements of both OpenCLIP ViT-H/14 towers (image: head dim
and activation from the configuration; text: pooled at the first maximum id and projected) checked against transformers' CLIPVisionModelWithProjection /
CLIPTextModelWithProjection in fp64, the configuration checks, both state layouts, the calculate_hps driver with a stub model, and the command-line driver.
tests/test_hps_gpu.py takes its cases and reference errors from here."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from test_text_native_cpu import PROMPTS, _mm, _store, clip_tokens, scale_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# both towers restated (test-local; fp64 sums everywhere); generalised from vision_ref (tests/test_consistency_cpu.py) and tower_ref (tests/test_text_native_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def _act(cfg):
    return (lambda x: x * torch.sigmoid(1.702 * x)) if cfg.hidden_act == "quick_gelu" else torch.nn.functional.gelu


def _blocks(cfg, st, h, mode, causal):
    """the pre-LN blocks over h [B, S, C]; head dim = hidden_size / heads, activation from the configuration"""
    C, nh, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    B, S, _ = h.shape
    D = C // nh
    keep = lambda t: _store(t, mode)
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (C,), st[p + ".weight"], st[p + ".bias"], eps)
    lin = lambda t, p: _mm(t, st[p + ".weight"], mode) + st[p + ".bias"]
    act = _act(cfg)
    mask = torch.ones(S, S, dtype=torch.bool).tril() if causal else None
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        y = keep(ln(h, p + "layer_norm1"))
        heads = lambda u: u.view(B, S, nh, D).transpose(1, 2)
        q, k, v = (heads(keep(lin(y, p + "self_attn." + n))) for n in ("q_proj", "k_proj", "v_proj"))
        s = _mm(q, k, mode) * D ** -0.5
        if mask is not None:
            s = s.masked_fill(~mask, float("-inf"))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        a = _mm(e, v.transpose(-1, -2), mode) / e.sum(-1, keepdim=True)         # the kernels normalise after the second product
        a = keep(a.transpose(1, 2).reshape(B, S, C))
        h = keep(h + lin(a, p + "self_attn.out_proj"))
        y = keep(ln(h, p + "layer_norm2"))
        h = keep(h + lin(keep(act(lin(y, p + "mlp.fc1"))), p + "mlp.fc2"))
    return h


def hps_vision_ref(cfg, state, x, mode="f64"):
    """CLIPVisionModelWithProjection(x).image_embeds restated: x [B, 3, S, S] -> fp64 [B, P].  mode "f64" / "x3" / "bf16" as in tower_ref."""
    st = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v.double() for k, v in state.items()}
    C, eps, ps = cfg.hidden_size, cfg.layer_norm_eps, cfg.patch_size
    B = x.shape[0]
    keep = lambda t: _store(t, mode)
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (C,), st[p + ".weight"], st[p + ".bias"], eps)
    g = x.shape[2] // ps
    rows = keep(x.double().reshape(B, 3, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * ps * ps))
    pos = st["embeddings.position_embedding.weight"]
    t = keep(_mm(rows, st["embeddings.patch_embedding.weight"].reshape(C, -1), mode) + keep(pos[1:]))
    cls = keep(st["embeddings.class_embedding"] + pos[0])
    h = keep(ln(torch.cat([cls.expand(B, 1, C), t], dim=1), "pre_layrnorm"))
    h = _blocks(cfg, st, h, mode, causal=False)
    return keep(_mm(keep(ln(h[:, 0], "post_layernorm")), st["visual_projection.weight"], mode))


def first_max(ids):
    """open_clip's pooling position: the first position holding the row's largest id"""
    return torch.tensor([int((row == row.max()).nonzero()[0]) for row in ids])


def hps_text_ref(cfg, state, ids, mode="f64"):
    """CLIPTextModelWithProjection(ids).text_embeds restated with open_clip's pooling: ids [N, S] int64 -> fp64 [N, P]"""
    st = {(k[len("text_model."):] if k.startswith("text_model.") else k): v.double() for k, v in state.items()}
    C, eps = cfg.hidden_size, cfg.layer_norm_eps
    N, S = ids.shape
    keep = lambda t: _store(t, mode)
    x = keep(st["embeddings.token_embedding.weight"][ids] + st["embeddings.position_embedding.weight"][:S])
    x = _blocks(cfg, st, x, mode, causal=True)
    row = x[torch.arange(N), first_max(ids)]
    row = keep(torch.nn.functional.layer_norm(row, (C,), st["final_layer_norm.weight"], st["final_layer_norm.bias"], eps))
    return keep(_mm(row, st["text_projection.weight"], mode))


# ---------------------------------------------------------------------------------------------------------------------
# the cases (computed once; tests/test_hps_gpu.py shares them)
# ---------------------------------------------------------------------------------------------------------------------
VISION_CASES = {"tiny14": ("tiny14", None, 4), "vith14x4": ("vith14", 4, 2)}          # name -> (configuration, layers it is cut to, batch)
TEXT_CASES = {"tiny": dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, projection_dim=64, hidden_act="gelu"),
              "h14x4": dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=4, num_attention_heads=16, projection_dim=1024,
                            hidden_act="gelu")}


def vision_cfg(name):
    from freefine_amd import hps
    base, layers, B = VISION_CASES[name]
    cfg = hps.openclip_vision_config(base)
    if layers is not None:
        cfg = hps.openclip_vision_config(dict(vars(cfg), num_hidden_layers=layers))
    return cfg, B


def run_vision_module(cfg, st, x):
    """(CLIPVisionModelWithProjection.double() image_embeds, the error of the module in fp32 on the CPU against it)"""
    from transformers import CLIPVisionModelWithProjection
    from freefine_amd import clipvision as CV
    mod = CLIPVisionModelWithProjection(CV.transformers_vision_config(cfg)).eval()
    mod.load_state_dict(st, strict=True)
    with torch.no_grad():
        f32 = mod(pixel_values=x.float()).image_embeds
        want = mod.double()(pixel_values=x.double()).image_embeds
    return want, scale_err(f32, want)


def run_text_module(cfg, st, ids):
    """the same for CLIPTextModelWithProjection text_embeds.  The module's config carries eos_token_id = the largest id of the vocabulary the ids come from, so
    that transformers' rule (first eos) and the first-maximum rule select the same row."""
    from transformers import CLIPTextModelWithProjection
    from freefine_amd import text as FT
    eos = int(ids.max())
    mod = CLIPTextModelWithProjection(FT.transformers_text_config(cfg, eos_token_id=eos, bos_token_id=eos - 1, pad_token_id=0)).eval()
    bad = mod.load_state_dict(st, strict=False)
    assert not bad.unexpected_keys and all("position_ids" in k for k in bad.missing_keys), bad
    with torch.no_grad():
        f32 = mod(input_ids=ids).text_embeds
        want = mod.double()(input_ids=ids).text_embeds
    return want, scale_err(f32, want)


@functools.lru_cache(maxsize=None)
def vision_case(name):
    """(config, seeded state in transformers' layout, normalised input, CLIPVisionModelWithProjection.double() image_embeds, the module's fp32 error on the CPU)"""
    from freefine_amd import clipvision as CV
    cfg, B = vision_cfg(name)
    st = CV.synthetic_state(cfg, seed=14 + len(name))
    x = torch.from_numpy(np.random.default_rng(140 + len(name)).standard_normal((B, 3, cfg.image_size, cfg.image_size)).astype(np.float32))
    return (cfg, st, x) + run_vision_module(cfg, st, x)


@functools.lru_cache(maxsize=None)
def vision_errs(name):
    """the reference errors tower_bound reads: {"f32": the fp32 module, "x3" / "bf16": the emulated arithmetic} against the fp64 module"""
    cfg, st, x, want, f32 = vision_case(name)
    return {"f32": f32, "x3": scale_err(hps_vision_ref(cfg, st, x, "x3"), want), "bf16": scale_err(hps_vision_ref(cfg, st, x, "bf16"), want)}


@functools.lru_cache(maxsize=None)
def text_case(name):
    """(config, seeded state in transformers' layout, ids of PROMPTS, CLIPTextModelWithProjection.double() text_embeds, the module's fp32 error on the CPU)"""
    from freefine_amd import text as FT
    cfg = FT.text_projection_config(TEXT_CASES[name])
    st = FT.synthetic_text_state(cfg, seed=77 + len(name))
    ids = clip_tokens(PROMPTS, vocab=cfg.vocab_size)
    return (cfg, st, ids) + run_text_module(cfg, st, ids)


@functools.lru_cache(maxsize=None)
def text_errs(name):
    cfg, st, ids, want, f32 = text_case(name)
    return {"f32": f32, "x3": scale_err(hps_text_ref(cfg, st, ids, "x3"), want), "bf16": scale_err(hps_text_ref(cfg, st, ids, "bf16"), want)}


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VISION_CASES))
def test_vision_restatement_equals_transformers_fp64(name):
    cfg, st, x, want, f32 = vision_case(name)
    assert cfg.hidden_size // cfg.num_attention_heads == 80 and cfg.hidden_act == "gelu" and cfg.patch_size == 14
    got = hps_vision_ref(cfg, st, x)
    e = scale_err(got, want)
    print(f"vision restatement vs CLIPVisionModelWithProjection.double() ({name}): {e:.2e}; fp32 module {f32:.2e} (|y| max {want.abs().max():.3f})")
    assert got.shape == want.shape == (x.shape[0], cfg.projection_dim) and e <= 1e-12
    assert 0 < f32 < 1e-5


@pytest.mark.parametrize("name", list(TEXT_CASES))
def test_text_restatement_equals_transformers_fp64(name):
    cfg, st, ids, want, f32 = text_case(name)
    pos = first_max(ids)
    assert pos.tolist() == [len(PROMPTS[0]) + 1, 1, 76]            # a short prompt, the empty one (EOS at 1), a truncated one (EOS only at 76)
    assert torch.equal(pos, (ids == cfg.vocab_size - 1).int().argmax(-1))          # transformers' rule selects the same rows
    got = hps_text_ref(cfg, st, ids)
    e = scale_err(got, want)
    print(f"text restatement vs CLIPTextModelWithProjection.double() ({name}): {e:.2e}; fp32 module {f32:.2e} (|y| max {want.abs().max():.3f})")
    assert got.shape == want.shape == (3, cfg.projection_dim) and e <= 1e-12
    assert 0 < f32 < 1e-5


def test_emulated_modes_are_the_same_towers():
    ev, et = vision_errs("tiny14"), text_errs("tiny")
    for e in (ev, et):
        assert 0 < e["x3"] < 1e-4 and e["x3"] < e["bf16"] < 1e-1, e


def test_openclip_vision_config_accepts_and_rejects():
    from freefine_amd import clipvision as CV
    from freefine_amd import hps
    h = hps.openclip_vision_config("vith14")
    assert (h.hidden_size, h.num_hidden_layers, h.num_attention_heads, h.intermediate_size, h.patch_size, h.image_size, h.projection_dim, h.hidden_act,
            h.layer_norm_eps) == (1280, 32, 16, 5120, 14, 224, 1024, "gelu", 1e-5)
    t = hps.openclip_vision_config("tiny14")
    assert (t.hidden_size, t.num_hidden_layers, t.num_attention_heads, t.intermediate_size, t.patch_size, t.image_size, t.projection_dim, t.hidden_act) == \
        (160, 2, 2, 640, 14, 56, 64, "gelu")
    assert hps.openclip_vision_config(t) is t
    assert hps.openclip_vision_config(CV.transformers_vision_config(h)).hidden_size == 1280
    base = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2)
    assert hps.openclip_vision_config(base).hidden_act == "quick_gelu"                       # head dim 64, the defaults of CLIPVisionConfig
    assert hps.openclip_vision_config(dict(base, hidden_act="gelu", hidden_size=160)).hidden_act == "gelu"
    with pytest.raises(ValueError, match="head dim 32"):
        hps.openclip_vision_config(dict(base, num_attention_heads=4))
    with pytest.raises(ValueError, match="head dim"):
        hps.openclip_vision_config(dict(base, hidden_size=130))
    with pytest.raises(ValueError, match="hidden_act 'relu'"):
        hps.openclip_vision_config(dict(base, hidden_act="relu"))
    with pytest.raises(ValueError, match="whole patches"):
        hps.openclip_vision_config(dict(base, patch_size=14, image_size=60))
    with pytest.raises(ValueError, match="one of"):
        hps.openclip_vision_config("vitb32")
    with pytest.raises(ValueError, match="missing"):
        hps.openclip_vision_config({k: v for k, v in base.items() if k != "intermediate_size"})
    # the CLIP ViT-B/32 tower's contract is what it was
    with pytest.raises(ValueError, match="head dim"):
        CV.clip_vision_config(dict(base, num_attention_heads=4))
    with pytest.raises(ValueError, match="head dim"):
        CV.clip_vision_config(dict(base, hidden_size=160))
    with pytest.raises(ValueError, match="hidden_act"):
        CV.clip_vision_config(dict(base, hidden_act="gelu"))
    with pytest.raises(ValueError, match="one of"):
        CV.clip_vision_config("vith14")


def test_text_projection_config():
    from freefine_amd import text as FT
    h = FT.text_projection_config("vith14")
    assert (h.hidden_size, h.num_hidden_layers, h.num_attention_heads, h.intermediate_size, h.hidden_act, h.projection_dim, h.vocab_size) == \
        (1024, 24, 16, 4096, "gelu", 1024, 49408)
    assert FT.text_projection_config("tiny").vocab_size == 259
    with pytest.raises(ValueError, match="projection_dim"):
        FT.text_projection_config({k: v for k, v in TEXT_CASES["tiny"].items() if k != "projection_dim"})
    with pytest.raises(ValueError, match="head dim"):
        FT.text_projection_config(dict(TEXT_CASES["tiny"], num_attention_heads=4))
    with pytest.raises(ValueError, match="one of"):
        FT.text_projection_config("vitl14")


def test_state_layouts_round_trip_for_both_towers():
    from freefine_amd import clipvision as CV
    from freefine_amd import hps
    from freefine_amd import text as FT
    vcfg, vst, *_ = vision_case("tiny14")
    tcfg, tst, *_ = text_case("tiny")
    L = tcfg.num_hidden_layers
    # text: transformers' names with / without the prefix, open_clip's names
    oc = FT.to_openclip_text_layout(tst, L)
    assert oc["text_projection"].shape == (128, 64) and oc["positional_embedding"].shape == (77, 128) and oc["transformer.resblocks.1.attn.in_proj_weight"].shape == (384, 128)
    bare = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in tst.items()}
    packs = [FT.pack_text_projection_state(tcfg, s) for s in (tst, bare, oc)]
    for p in packs[1:]:
        assert set(p) == set(packs[0]) and all(torch.equal(p[k], packs[0][k]) for k in p)
    assert torch.equal(packs[0]["proj.w"], tst["text_projection.weight"]) and packs[0]["proj.w"].shape == (64, 128)
    assert torch.equal(packs[0]["1.qk.w"][128:], tst["text_model.encoder.layers.1.self_attn.k_proj.weight"])
    back = FT._openclip_text_to_transformers(oc, L)
    assert all(torch.equal(back[k], bare[k]) for k in bare)
    # a whole open_clip checkpoint: the towers' transformer.resblocks.* must not be mixed up
    whole = dict(CV.to_openai_layout(vst, vcfg.num_hidden_layers), **oc, logit_scale=torch.tensor(4.6))
    vis, txt = hps.split_state(whole)
    assert all(k.startswith("visual.") for k in vis) and not any(k.startswith("visual.") for k in txt)
    pv = CV.pack_vision_state(vcfg, vis)
    want = CV.pack_vision_state(vcfg, vst)
    assert set(pv) == set(want) and all(torch.equal(pv[k], want[k]) for k in pv) and pv["pe.w"].shape == (160, 588)
    pt = FT.pack_text_projection_state(tcfg, txt)
    assert all(torch.equal(pt[k], packs[0][k]) for k in pt)
    vis2, txt2 = hps.split_state(dict(vst, **tst))
    assert set(vis2) == set(vst) and set(txt2) == set(tst)
    # refusals name the parameter
    for drop, state in (("text_projection.weight", tst), ("text_model.final_layer_norm.bias", tst), ("text_model.encoder.layers.0.mlp.fc2.bias", tst)):
        broken = dict(state)
        broken.pop(drop)
        with pytest.raises(ValueError, match=drop.split("text_model.")[-1]):
            FT.pack_text_projection_state(tcfg, broken)
    for drop in ("ln_final.bias", "text_projection", "transformer.resblocks.1.mlp.c_fc.weight"):
        broken = dict(oc)
        broken.pop(drop)
        with pytest.raises(ValueError, match=drop):
            FT.pack_text_projection_state(tcfg, broken)
    with pytest.raises(ValueError, match="text_projection.weight"):
        FT.pack_text_projection_state(tcfg, dict(tst, **{"text_projection.weight": torch.zeros(32, 128)}))
    with pytest.raises(ValueError, match="position_embedding"):
        FT.pack_text_projection_state(tcfg, dict(oc, positional_embedding=torch.zeros(70, 128)))
    broken = dict(CV.to_openai_layout(vst, vcfg.num_hidden_layers))
    broken.pop("visual.ln_post.bias")
    with pytest.raises(ValueError, match="ln_post.bias"):
        CV.pack_vision_state(vcfg, broken)


# ---------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------
class StubModel:
    """score_u8 = the images' mean byte / 255 + the prompt's length / 1000; records its calls"""

    def __init__(self):
        self.calls = []

    def score_u8(self, images, prompt):
        assert images.dtype == np.uint8 and images.ndim == 4 and images.shape[-1] == 3
        self.calls.append((images.shape, prompt))
        return images.reshape(images.shape[0], -1).mean(1) / 255 + len(prompt) / 1000


def hps_tree():
    """two image entries with captions of their own; files of two sizes, named by their content"""
    files = {"a0": (8, 8, 10), "a1": (8, 12, 20), "a2": (8, 8, 30), "b0": (8, 12, 40), "b1": (8, 12, 50)}
    data = {"imgA": {"4v_caption": "a cup", "instances": {"0": {"c0": {"gen": "a0"}, "c1": {"gen": "a1"}}, "1": {"c0": {"gen": "a2"}}}},
            "imgB": {"4v_caption": "a longer caption", "instances": {"0": {"c0": {"gen": "b0"}, "c1": {"gen": "b1"}}}},
            "imgC": {"4v_caption": "nothing generated", "instances": {}}}
    reader = lambda p: np.full(files[p][:2] + (3,), files[p][2], dtype=np.uint8)
    return data, files, reader


def test_calculate_hps_with_a_stub_model():
    from freefine_amd import metrics as FM
    data, files, reader = hps_tree()
    model = StubModel()
    got = FM.calculate_hps(data, "gen", model, reader=reader)
    cap = {"a": "a cup", "b": "a longer caption"}
    want = sum(v[2] / 255 + len(cap[k[0]]) / 1000 for k, v in files.items()) / 5
    assert abs(got - want) < 1e-12
    # one prompt per image entry, one size per call
    assert sorted(model.calls) == sorted([((2, 8, 8, 3), "a cup"), ((1, 8, 12, 3), "a cup"), ((2, 8, 12, 3), "a longer caption")])
    model = StubModel()
    assert abs(FM.calculate_hps(data, "gen", model, reader=reader, batch_size=1) - want) < 1e-12 and len(model.calls) == 5
    with pytest.raises(ValueError, match="RGB images only"):
        FM.calculate_hps(data, "gen", StubModel(), reader=lambda p: np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(ValueError, match="RGB images only"):
        FM.calculate_hps(data, "gen", StubModel(), reader=lambda p: np.zeros((8, 8), np.uint8))
    with pytest.raises(ValueError, match="no samples"):
        FM.calculate_hps({"imgC": data["imgC"]}, "gen", StubModel(), reader=reader)
    with pytest.raises(ValueError, match="no samples"):
        FM.calculate_hps({}, "gen", StubModel(), reader=reader)
    sys.path.insert(0, os.path.join(ROOT, "evaluation", "metrics"))
    try:
        import human_preference_score as shim
    finally:
        sys.path.pop(0)
    assert shim.calculate_hps is FM.calculate_hps


def test_driver_reports_hps_without_weights(tmp_path, capsys):
    from test_consistency_cpu import load_driver
    drv = load_driver()
    data, *_ = hps_tree()
    path = str(tmp_path / "results.json")
    json.dump(data, open(path, "w"))
    res = drv.main(["--path", path, "--task", "001000000"])
    out = capsys.readouterr().out
    assert list(res) == ["HPS"] and "not built" in res["HPS"] and "--hps_weights" in res["HPS"] and "--hps_tokenizer" in res["HPS"]
    assert "-----HPS-----" in out and all(f"-----{n}-----" not in out for n in drv.NAMES if n != "HPS")
    res = drv.main(["--path", path, "--task", "001000000", "--hps_weights", str(tmp_path / "w.pt")])          # the tokenizer still missing: the file is not opened
    assert "not built" in res["HPS"]
    assert "HPS" not in drv.NOT_BUILT and set(drv.NOT_BUILT) == {"FID", "IRS"}
    assert "HPSv2) have no model code" not in drv.__doc__ and "--hps_weights" in drv.__doc__
    with pytest.raises(ValueError, match="vocab.json"):
        from freefine_amd import hps
        hps.load_tokenizer(str(tmp_path))


def test_abi_declares_the_two_entries():
    import re
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    for name in ("ffn_pool_layernorm", "ffn_cosine_rows"):
        assert re.search(rf"\bint\s+{name}\s*\(", header) and name in _lib.SYMBOLS
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "ffn_pool_layernorm") and hasattr(lib, "ffn_cosine_rows") and lib.ffn_version() >= 8
        # validation runs before any launch: no device needed
        assert lib.ffn_pool_layernorm(None, 0, None, None, None, None, None, 1, 1, 64, 1e-5, 0) == -22 and b"pool_layernorm" in lib.ffn_last_error()
        assert lib.ffn_cosine_rows(None, None, None, None, 1, 4, 1) == -22 and b"cosine_rows" in lib.ffn_last_error()
