"""CPU: the ImageReward score (freefine_amd.irs) as far as it runs without a device -- the fp64 restatement of tests/irs_ref.py against transformers'
BlipVisionModel / BlipTextModel (the text model built with is_decoder=True, called with is_decoder=False) and an nn.Sequential of the head's Linears, the state
mapping, the configuration checks, the tokenizer, calculate_irs with a stub model and the command-line driver.  tests/test_irs_gpu.py takes its cases and
reference errors from here.  All weights are drawn (encoder.draw_state): BlipVisionConfig's own initialiser range of 1e-10 embeds every image alike."""
import functools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irs_ref
from test_hps_cpu import StubModel, hps_tree
from test_text_native_cpu import scale_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VISION_CASES = {"tiny16": ("tiny16", None, 2), "vitl16x2": ("vitl16", 2, 2)}      # name -> (configuration, blocks it is cut to, batch)
TEXT_CASES = {"tiny": ("tiny", None), "medx2": ("med", 2)}                        # name -> (configuration, layers it is cut to)
LIVE = (3, 11, 35)                                                                # live tokens of the three prompts of a text case (of 35)
CAPTIONS = ["a photo of a cup", "two dogs on a beach at sunset", "x"]


# ---------------------------------------------------------------------------------------------------------------------
# the cases (computed once; tests/test_irs_gpu.py shares them)
# ---------------------------------------------------------------------------------------------------------------------
def vision_cfg(name):
    from freefine_amd import irs
    base, depth, B = VISION_CASES[name]
    cfg = irs.blip_vision_config(base)
    return (cfg if depth is None else SimpleNamespace(**dict(vars(cfg), depth=depth))), B


def text_cfg(name):
    from freefine_amd import irs
    base, layers = TEXT_CASES[name]
    cfg = irs.blip_text_config(base)
    return cfg if layers is None else SimpleNamespace(**dict(vars(cfg), num_hidden_layers=layers))


def vision_module(cfg, st):
    from transformers import BlipVisionModel
    from freefine_amd import irs
    mod = BlipVisionModel(irs.transformers_vision_config(cfg)).eval()
    mod.load_state_dict(irs.to_transformers_vision_layout(st, cfg.depth), strict=True)
    return mod


def text_module(cfg, st):
    from transformers import BlipTextModel
    from freefine_amd import irs
    mod = BlipTextModel(irs.transformers_text_config(cfg), add_pooling_layer=False).eval()
    mod.load_state_dict(st, strict=True)
    return mod


def run_vision_module(cfg, st, x):
    """(BlipVisionModel.double() last_hidden_state, the module's output in fp32 on the CPU)"""
    mod = vision_module(cfg, st)
    with torch.no_grad():
        f32 = mod(pixel_values=x.float()).last_hidden_state
        want = mod.double()(pixel_values=x.double()).last_hidden_state
    return want, f32


def run_text_module(cfg, st, ids, mask, embeds):
    """(BlipTextModel.double() last_hidden_state [B, S, C], the module's output in fp32 on the CPU) for embeds given in fp32"""
    mod = text_module(cfg, st)
    call = lambda m, e: m(input_ids=ids, attention_mask=mask, encoder_hidden_states=e, is_decoder=False).last_hidden_state
    with torch.no_grad():
        f32 = call(mod, embeds.float())
        want = call(mod.double(), embeds.double())
    return want, f32


@functools.lru_cache(maxsize=None)
def vision_case(name):
    """(config, drawn state in timm's layout, normalised input, BlipVisionModel.double() last_hidden_state, the module's fp32 error on the CPU)"""
    from freefine_amd import encoder, irs
    cfg, B = vision_cfg(name)
    st = encoder.draw_state(irs.vision_param_shapes(cfg), seed=21 + len(name))
    x = torch.from_numpy(np.random.default_rng(210 + len(name)).standard_normal((B, 3, cfg.img_size, cfg.img_size)).astype(np.float32))
    want, f32 = run_vision_module(cfg, st, x)
    return cfg, st, x, want, scale_err(f32, want)


@functools.lru_cache(maxsize=None)
def vision_errs(name):
    """the reference errors tower_bound reads: {"f32": the fp32 module, "x3" / "bf16": the emulated arithmetic} against the fp64 module"""
    cfg, st, x, want, f32 = vision_case(name)
    return {"f32": f32, "x3": scale_err(irs_ref.vision_ref(cfg, st, x, "x3"), want), "bf16": scale_err(irs_ref.vision_ref(cfg, st, x, "bf16"), want)}


def prompt_ids(V, S=35, live=LIVE, seed=0):
    """(ids, mask) int64 [len(live), S]: row b holds live[b] tokens (id 2 first, then ids drawn from [1, V), V - 1 among them) and padding id 0"""
    g = torch.Generator().manual_seed(seed)
    ids, mask = torch.zeros(len(live), S, dtype=torch.int64), torch.zeros(len(live), S, dtype=torch.int64)
    for b, n in enumerate(live):
        ids[b, :n] = torch.randint(1, V, (n,), generator=g)
        ids[b, 0], ids[b, n - 1] = 2, V - 1
        mask[b, :n] = 1
    return ids, mask


@functools.lru_cache(maxsize=None)
def text_case(name):
    """(config, drawn state in BlipTextModel's names, ids, mask, image tokens fp32 [3, 197, Ce], BlipTextModel.double() row 0 [3, C], the module's fp32 error)"""
    from freefine_amd import irs
    cfg = text_cfg(name)
    st = irs.draw_state(irs.text_param_shapes(cfg), seed=31 + len(name))
    ids, mask = prompt_ids(cfg.vocab_size, seed=len(name))
    embeds = torch.randn(len(LIVE), 197, cfg.encoder_hidden_size, generator=torch.Generator().manual_seed(310 + len(name)))
    want, f32 = run_text_module(cfg, st, ids, mask, embeds)
    return cfg, st, ids, mask, embeds, want[:, 0], scale_err(f32[:, 0], want[:, 0])


@functools.lru_cache(maxsize=None)
def text_errs(name):
    cfg, st, ids, mask, embeds, want, f32 = text_case(name)
    ref = lambda mode: irs_ref.text_ref(cfg, st, ids, mask, embeds, mode)[:, 0]
    return {"f32": f32, "x3": scale_err(ref("x3"), want), "bf16": scale_err(ref("bf16"), want)}


def smooth_images(n, H, W, seed):
    """smooth colour fields with some noise, every one different"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(n):
        f, ph = rng.uniform(0.02, 0.3, (3, 2)), rng.uniform(0, 6.28, (3, 2))
        im = np.stack([127 + 90 * np.sin(f[c, 0] * yy + ph[c, 0]) * np.cos(f[c, 1] * xx + ph[c, 1]) for c in range(3)], -1) + rng.normal(0, 12, (H, W, 3))
        out.append(np.clip(im, 0, 255).astype(np.uint8))
    return np.stack(out)


def tiny_state():
    """(the tiny score's state in ImageReward's layout, vision config, text config)"""
    from freefine_amd import irs
    return irs.synthetic_state("tiny16", "tiny", seed=9), irs.blip_vision_config("tiny16"), irs.blip_text_config("tiny")


def host_rewards(imgs, prompts):
    """(fp64 rewards [B] of the restated score for uint8 images and one prompt or B, the tolerance of each on the device in fp32).  Tolerance: the two towers
    together move the text tower's row 0 by at most delta = tower_bound's fp32 bound, taken from the error of the CPU modules run in fp32 one behind the other
    on these very inputs, times the row's maximum; irs_ref.chain_tol carries that through the head (which is affine: through the exact products of its weights)
    and adds the chain's own rounding."""
    from test_consistency_gpu import clip_host_prepare
    from test_text_native_gpu import tower_bound
    from freefine_amd import irs, text
    st, vcfg, tcfg = tiny_state()
    vst, tst, head = irs.split_state(st)
    x = clip_host_prepare(imgs, size=224)
    tok = text.ByteTokenizer()(list(prompts), max_length=35)
    ids = tok.input_ids
    mask = (ids != 0).long()
    B = x.shape[0]
    want, row = irs_ref.score_ref(vcfg, vst, tcfg, tst, head, x, ids, mask)
    e64, e32 = run_vision_module(vcfg, vst, x)
    r64, _ = run_text_module(tcfg, tst, ids.expand(B, -1), mask.expand(B, -1), e64)
    _, r32 = run_text_module(tcfg, tst, ids.expand(B, -1), mask.expand(B, -1), e32)
    assert scale_err(row, r64[:, 0]) <= 1e-12
    delta = tower_bound({"f32": scale_err(r32[:, 0], r64[:, 0])}, "f32") * row.abs().max().item()
    return want, irs_ref.chain_tol(head, row, delta, irs_ref.REWARD_STD)


@functools.lru_cache(maxsize=None)
def score_case():
    """3 smooth images x the 3 CAPTIONS: (images uint8 [3, 64, 96, 3], fp64 rewards [prompt, image], tolerances alike)"""
    imgs = smooth_images(3, 64, 96, seed=4)
    res = [host_rewards(imgs, [c]) for c in CAPTIONS]
    return imgs, torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res])


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against transformers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VISION_CASES))
def test_vision_restatement_equals_transformers_fp64(name):
    cfg, st, x, want, f32 = vision_case(name)
    got = irs_ref.vision_ref(cfg, st, x)
    e = scale_err(got, want)
    print(f"vision restatement vs BlipVisionModel.double() ({name}): {e:.2e}; fp32 module {f32:.2e} (|y| max {want.abs().max():.3f})")
    assert got.shape == want.shape == (x.shape[0], 197, cfg.embed_dim) and e <= 1e-12
    assert 0 < f32 < 1e-5
    assert (want[0] - want[1]).abs().max() > 0.1 * want.abs().max(), "drawn weights: different images embed differently"


@pytest.mark.parametrize("name", list(TEXT_CASES))
def test_text_restatement_equals_transformers_fp64(name):
    cfg, st, ids, mask, embeds, want, f32 = text_case(name)
    assert mask.sum(1).tolist() == list(LIVE) and int(ids.max()) == cfg.vocab_size - 1 and cfg.encoder_hidden_size != cfg.hidden_size
    got = irs_ref.text_ref(cfg, st, ids, mask, embeds)[:, 0]
    e = scale_err(got, want)
    print(f"text restatement vs BlipTextModel.double() ({name}): {e:.2e}; fp32 module {f32:.2e} (|y| max {want.abs().max():.3f})")
    assert got.shape == want.shape == (3, cfg.hidden_size) and e <= 1e-12
    assert 0 < f32 < 1e-5


def test_the_mask_and_the_image_tokens_reach_row_0():
    """what the issue measured on the module holds for the restatement: a padded id does not move row 0 at all, a live one, the key mask and the image tokens do"""
    cfg, st, ids, mask, embeds, want, _ = text_case("tiny")
    row = lambda i, m, e: irs_ref.text_ref(cfg, st, i, m, e)[:, 0]
    pad = ids.clone()
    pad[0, 5:] = 7
    assert torch.equal(row(pad, mask, embeds)[0], row(ids, mask, embeds)[0])
    live = ids.clone()
    live[0, 1] = 7
    assert scale_err(row(live, mask, embeds)[:1], want[:1]) > 1e-3
    assert scale_err(row(ids, torch.ones_like(mask), embeds)[:1], want[:1]) > 1e-3
    assert scale_err(row(ids, mask, embeds.flip(0))[:1], want[:1]) > 1e-3


def test_emulated_modes_are_the_same_towers():
    for e in (vision_errs("tiny16"), text_errs("tiny")):
        assert 0 < e["x3"] < 1e-4 and e["x3"] < e["bf16"] < 1e-1, e


def test_head_equals_a_sequential_of_the_five_linears():
    from freefine_amd import encoder, irs
    st = encoder.draw_state(irs.head_param_shapes(768), seed=3)
    _, _, head = irs.split_state(st)
    assert [tuple(w.shape) for w, _ in head] == [(1024, 768), (128, 1024), (64, 128), (16, 64), (1, 16)]
    seq = torch.nn.Sequential(torch.nn.Linear(768, 1024), torch.nn.Dropout(0.2), torch.nn.Linear(1024, 128), torch.nn.Dropout(0.2), torch.nn.Linear(128, 64),
                              torch.nn.Dropout(0.1), torch.nn.Linear(64, 16), torch.nn.Linear(16, 1)).double().eval()
    seq.load_state_dict({k[len("mlp.layers."):]: v.double() for k, v in st.items()}, strict=True)
    x = torch.randn(5, 768, generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        want = (seq(x)[:, 0] - irs.REWARD_MEAN) / irs.REWARD_STD
    assert (irs_ref.head_ref(head, x) - want).abs().max() <= 1e-12 * want.abs().max()
    tol = irs_ref.chain_tol(head, x, 0.0, irs.REWARD_STD)
    assert tol.shape == (5,) and 0 < tol.max() < 1e-2


def test_score_case_separates_images_and_prompts():
    """the seeds of the end-to-end GPU test: the fp64 rewards differ across images and across prompts by more than 10 x the tolerance it will hold the device to"""
    _, want, tols = score_case()
    print(f"tiny score: rewards {want.min():.4f} .. {want.max():.4f}; tolerance {tols.max():.2e}; least spread over images "
          f"{(want.max(1).values - want.min(1).values).min():.3e}, over prompts {(want.max(0).values - want.min(0).values).min():.3e}")
    assert want.shape == tols.shape == (3, 3)
    assert (want.max(1).values - want.min(1).values).min() > 10 * tols.max() and (want.max(0).values - want.min(0).values).min() > 10 * tols.max()


# ---------------------------------------------------------------------------------------------------------------------
# states, configurations, tokenizer
# ---------------------------------------------------------------------------------------------------------------------
def test_an_imagereward_state_loads_into_the_transformers_modules():
    from freefine_amd import irs
    st, vcfg, tcfg = tiny_state()
    assert all(k.startswith(("blip.visual_encoder.", "blip.text_encoder.", "mlp.layers.")) for k in st)
    extra = dict(st, **{"blip.text_encoder.embeddings.position_ids": torch.arange(40)[None], "blip.text_encoder.pooler.dense.weight": torch.zeros(2, 2),
                        "blip.vision_proj.weight": torch.zeros(2, 2)})
    vis, txt, head = irs.split_state(extra)
    assert "embeddings.position_ids" in txt and len(head) == 5
    pv, pt = irs.pack_vision_state(vcfg, vis), irs.pack_text_state(tcfg, txt)
    vision_module(vcfg, pv), text_module(tcfg, pt)                       # strict=True inside
    assert pt["encoder.layer.1.crossattention.self.key.weight"].shape == (128, 192)
    # transformers' vision layout comes back to the same tensors; a dict of the three parts is taken as it is
    back = irs.pack_vision_state(vcfg, {"vision_model." + k: v for k, v in irs.to_transformers_vision_layout(pv, vcfg.depth).items()})
    assert set(back) == set(pv) and all(torch.equal(back[k], pv[k]) for k in pv)
    v2, t2, h2 = irs.split_state({"vision": vis, "text": txt, "head": head})
    assert v2 is vis and t2 is txt and all(a[0] is b[0] for a, b in zip(h2, head))
    for drop, fn, state in (("blocks.1.attn.qkv.bias", lambda s: irs.pack_vision_state(vcfg, s), vis), ("encoder.layer.0.crossattention.self.value.weight",
                                                                                                     lambda s: irs.pack_text_state(tcfg, s), txt)):
        broken = dict(state)
        broken.pop(drop)
        with pytest.raises(ValueError, match=drop):
            fn(broken)
    with pytest.raises(ValueError, match="layers.6.weight"):
        irs.split_state({k: v for k, v in st.items() if k != "mlp.layers.6.weight"})


def test_configurations_accept_and_reject():
    from freefine_amd import irs
    v = irs.blip_vision_config("vitl16")
    assert (v.embed_dim, v.depth, v.num_heads, v.patch, v.img_size, v.mlp_ratio, v.ln_eps, v.layerscale) == (1024, 24, 16, 16, 224, 4, 1e-6, False)
    t = irs.blip_text_config("med")
    assert (t.vocab_size, t.hidden_size, t.num_hidden_layers, t.num_attention_heads, t.intermediate_size, t.encoder_hidden_size, t.hidden_act, t.layer_norm_eps) == \
        (30524, 768, 12, 12, 3072, 1024, "gelu", 1e-12)
    tiny = irs.blip_text_config("tiny")
    assert (tiny.hidden_size, tiny.num_attention_heads, tiny.num_hidden_layers, tiny.intermediate_size, tiny.encoder_hidden_size, tiny.vocab_size,
            tiny.max_position_embeddings) == (128, 2, 2, 256, 192, 300, 40)
    assert irs.blip_vision_config("tiny16").embed_dim == tiny.encoder_hidden_size
    assert irs.blip_vision_config(v) is v and irs.blip_text_config(t) is t
    assert irs.blip_vision_config(irs.transformers_vision_config(v)).embed_dim == 1024 and irs.blip_text_config(irs.transformers_text_config(t)).encoder_hidden_size == 1024
    vb = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2)
    tb = dict(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, max_position_embeddings=40, encoder_hidden_size=192)
    with pytest.raises(ValueError, match="head dim 32"):
        irs.blip_vision_config(dict(vb, num_attention_heads=4))
    with pytest.raises(ValueError, match="head dim 32"):
        irs.blip_text_config(dict(tb, num_attention_heads=4))
    with pytest.raises(ValueError, match="hidden_act 'quick_gelu'"):
        irs.blip_vision_config(dict(vb, hidden_act="quick_gelu"))
    with pytest.raises(ValueError, match="hidden_act 'relu'"):
        irs.blip_text_config(dict(tb, hidden_act="relu"))
    with pytest.raises(ValueError, match="whole patches"):
        irs.blip_vision_config(dict(vb, image_size=230))
    with pytest.raises(ValueError, match="one of"):
        irs.blip_vision_config("vitb16")
    with pytest.raises(ValueError, match="missing"):
        irs.blip_text_config({k: v for k, v in tb.items() if k != "encoder_hidden_size"})
    # refusals that come before anything is uploaded: the mode, an image off the 224 grid, an id outside the vocabulary
    st, vcfg, tcfg = tiny_state()
    vis, txt, _ = irs.split_state(st)
    with pytest.raises(ValueError, match="x3"):
        irs.HipBlipText(tcfg, txt, dtype=torch.bfloat16, device="cpu", x3=True)
    with pytest.raises(ValueError, match="x3"):
        irs.HipBlipVision(vcfg, vis, dtype=torch.bfloat16, device="cpu", x3=True)
    vision, tower = irs.HipBlipVision(vcfg, vis, device="cpu"), irs.HipBlipText(tcfg, txt, device="cpu")
    for shape in ((1, 3, 230, 224), (1, 3, 224, 240), (1, 3, 448, 448), (3, 224, 224)):
        with pytest.raises(ValueError, match="fixed grid"):
            vision(torch.zeros(shape))
    embeds, ones = torch.zeros(1, 197, 192), torch.ones(1, 35, dtype=torch.int64)
    for bad in (300, -1):
        with pytest.raises(ValueError, match=r"token ids outside \[0, 300\)"):
            tower(torch.full((1, 35), bad), ones, embeds)
    with pytest.raises(ValueError, match="live token"):
        tower(ones, 0 * ones, embeds)
    with pytest.raises(ValueError, match="41 positions"):
        tower(torch.ones(1, 41, dtype=torch.int64), torch.ones(1, 41, dtype=torch.int64), embeds)
    with pytest.raises(ValueError, match="2 prompts for 1 images"):
        tower(ones.expand(2, -1), ones.expand(2, -1), embeds)
    with pytest.raises(ValueError, match="rows of 192 values"):
        tower(ones, ones, torch.zeros(1, 197, 128))


def test_tokenizer_from_a_local_vocabulary(tmp_path):
    from freefine_amd import irs, text
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "photo", "of", "cup", "##s", "dog", "on", "the", "beach", "##es"]
    (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n")
    tok = irs.load_tokenizer(str(tmp_path))
    assert len(tok) == len(words) + 2 and tok.pad_token_id == 0 and tok.convert_tokens_to_ids(["[DEC]", "[ENC]"]) == [len(words), len(words) + 1]
    out = tok(["A photo of CUPS", "dog " * 60, ""], padding="max_length", truncation=True, max_length=35, return_tensors="pt")
    ids, mask = out.input_ids, out.attention_mask
    assert ids.shape == mask.shape == (3, 35) and torch.equal(mask, (ids != 0).long())
    assert ids[0, :7].tolist() == [2, 5, 6, 7, 8, 9, 3] and mask[0].sum() == 7            # lower-cased, word pieces, [CLS] ... [SEP]
    assert mask[1].sum() == 35 and ids[1, 0] == 2 and ids[1, -1] == 3 and set(ids[1, 1:-1].tolist()) == {10}      # truncated to 35 with its [SEP]
    assert ids[2, :2].tolist() == [2, 3] and mask[2].sum() == 2
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="vocab.txt"):
        irs.load_tokenizer(str(empty))
    assert isinstance(irs.load_tokenizer("bytes"), text.ByteTokenizer)


# ---------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------
def test_calculate_irs_with_a_stub_model():
    from freefine_amd import metrics as FM
    data, files, reader = hps_tree()
    model = StubModel()
    got = FM.calculate_irs(data, "gen", model, reader=reader)
    cap = {"a": "a cup", "b": "a longer caption"}
    want = sum(v[2] / 255 + len(cap[k[0]]) / 1000 for k, v in files.items()) / 5
    assert abs(got - want) < 1e-12
    assert sorted(model.calls) == sorted([((2, 8, 8, 3), "a cup"), ((1, 8, 12, 3), "a cup"), ((2, 8, 12, 3), "a longer caption")])
    model = StubModel()
    assert abs(FM.calculate_irs(data, "gen", model, reader=reader, batch_size=1) - want) < 1e-12 and len(model.calls) == 5
    with pytest.raises(ValueError, match="RGB images only"):
        FM.calculate_irs(data, "gen", StubModel(), reader=lambda p: np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(ValueError, match="calculate_irs: no samples"):
        FM.calculate_irs({"imgC": data["imgC"]}, "gen", StubModel(), reader=reader)
    with pytest.raises(ValueError, match="calculate_hps: no samples"):
        FM.calculate_hps({}, "gen", StubModel(), reader=reader)
    sys.path.insert(0, os.path.join(ROOT, "evaluation", "metrics"))
    try:
        import image_reward as shim
    finally:
        sys.path.pop(0)
    assert shim.calculate_irs is FM.calculate_irs


def test_driver_reports_irs_without_weights(tmp_path, capsys):
    from test_consistency_cpu import load_driver
    drv = load_driver()
    data, *_ = hps_tree()
    path = str(tmp_path / "results.json")
    json.dump(data, open(path, "w"))
    res = drv.main(["--path", path, "--task", "010000000"])
    out = capsys.readouterr().out
    assert list(res) == ["IRS"] and "not built" in res["IRS"] and "--irs_weights" in res["IRS"] and "--irs_tokenizer" in res["IRS"]
    assert "-----IRS-----" in out and all(f"-----{n}-----" not in out for n in drv.NAMES if n != "IRS")
    res = drv.main(["--path", path, "--task", "010000000", "--irs_weights", str(tmp_path / "w.pt")])          # the tokenizer still missing: the file is not opened
    assert "not built" in res["IRS"]
    assert "--irs_weights" in drv.__doc__ and "ImageReward and BLIP) need packages" not in drv.__doc__


def test_abi_declares_the_two_entries():
    import ctypes
    import re
    from freefine_amd import _lib
    header = open(os.path.join(ROOT, "include", "freefine_hip.h")).read()
    for name in ("ffn_embed_tokens_ln", "ffn_affine_chain"):
        assert re.search(rf"\bint\s+{name}\s*\(", header) and name in _lib.SYMBOLS
    assert re.search(r"#define\s+FFN_CHAIN_MAXL\s+8\b", header) and re.search(r"#define\s+FFN_CHAIN_MAXW\s+1024\b", header) and (_lib.CHAIN_MAXL, _lib.CHAIN_MAXW) == (8, 1024)
    lib = _lib.load()
    assert lib.ffn_version() >= 15
    # validation runs before any launch: no device needed
    assert lib.ffn_embed_tokens_ln(None, 0, None, None, None, None, None, None, 35, 35, 768, 100, 1e-12) == -22 and b"embed_tokens_ln" in lib.ffn_last_error()
    P = 0x10000                                                     # never dereferenced, validation fails first
    dims = lambda *d: (ctypes.c_int * len(d))(*d)
    for d, L in ((dims(8, 1025, 1), 2), (dims(0, 1), 1), (dims(*([4] * 10)), 9), (dims(4), 0)):
        assert lib.ffn_affine_chain(None, P, P, P, 1, 2048, d, L, 0.0, 1.0) == -22 and b"affine_chain" in lib.ffn_last_error(), (list(d), L)
    assert lib.ffn_affine_chain(None, P, P, P, 1, 7, dims(8, 1), 1, 0.0, 1.0) == -22 and b"ldx" in lib.ffn_last_error()
    assert lib.ffn_affine_chain(None, P, P, P, 1, 8, dims(8, 1), 1, 0.0, 0.0) == -22 and b"scale" in lib.ffn_last_error()
