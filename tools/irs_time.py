"""Throughput of the ImageReward score at the metric's shape (GPU box): BLIP ViT-L/16 and BLIP's cross-attending BERT at FULL depth (24 image blocks, 12 text
layers), seeded random weights (no ImageReward checkpoint exists offline), 32 decoded 512 x 512 uint8 images and one prompt per call of HipImageReward.score_u8,
in fp32, split-bf16 (x3) and bf16.  The method is tools/hps_time.py's -- per mode: images per second over windows of at least `--window` seconds between two
device events on the launch stream (host work between the events counts: the device waits for it), the shape warmed first; then one profiled call
(ops.profile_begin / profile_end: device time per kernel, from the `_timed` table) split into the igemm, attention, layernorm and the two entries this metric
added (ffn_embed_tokens_ln, ffn_affine_chain).  Nothing gates on these numbers.
python tools/irs_time.py [--out profiles/irs_time.txt] [--batch 32] [--side 512] [--repeats 3] [--layers 24 12]"""
import argparse
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freefine_amd import irs, ops  # noqa: E402
from freefine_amd import text as FT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irs_time.txt"))
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=1.0, help="least seconds of work per timed window")
ap.add_argument("--layers", type=int, nargs=2, default=(24, 12), help="image blocks and text layers (default: ImageReward's)")
cli = ap.parse_args()
assert torch.cuda.is_available(), "irs_time.py measures on the GPU; there is no CPU fallback"
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3


def family(name):
    for key, fam in (("embed_tokens_ln", "embed_tokens_ln (new)"), ("affine_chain", "affine_chain (new)"), ("igemm", "igemm"), ("attn", "attention"),
                     ("layernorm", "layernorm"), ("split_pair", "split_pair"), ("patch_rows", "patch rows"), ("resize", "resize")):
        if key in name:
            return fam
    return name


vcfg = SimpleNamespace(**dict(vars(irs.blip_vision_config("vitl16")), depth=cli.layers[0]))
tcfg = SimpleNamespace(**dict(vars(irs.blip_text_config("med")), num_hidden_layers=cli.layers[1]))
state = irs.synthetic_state(vcfg, tcfg, seed=0)
imgs = np.random.default_rng(0).integers(0, 256, (cli.batch, cli.side, cli.side, 3), dtype=np.uint8)
prompt = "a photo of a red cup on a wooden table, studio lighting"
tok = FT.ByteTokenizer()          # ids < 259 of the 30524-row table: the lookup's cost does not depend on which rows

say(f"ImageReward score, BLIP ViT-L/16 ({cli.layers[0]} image blocks) and BLIP's BERT ({cli.layers[1]} cross-attending layers), {cli.batch} images of {cli.side} x "
    f"{cli.side} uint8 and one prompt per call; seeded random weights (no ImageReward checkpoint offline: parity against the published checkpoint is unmeasured); "
    f"{torch.cuda.get_device_name(0)}")
say(f"device events around windows of >= {cli.window:.1f} s, {cli.repeats} windows per mode; images per second")
for mode, dt, x3 in (("fp32", torch.float32, False), ("x3", torch.float32, True), ("bf16", torch.bfloat16, False)):
    model = irs.HipImageReward.from_state(state, tok, vcfg, tcfg, dtype=dt, device=dev, x3=x3)
    fn = lambda: model.score_u8(imgs, prompt)
    for _ in range(2):
        fn()
    n = max(1, int(math.ceil(cli.window / max(window(fn, 2) / 2, 1e-7))))
    rates = sorted(cli.batch * n / window(fn, n) for _ in range(cli.repeats))
    say(f"  {mode:5s} {n:3d} calls per window: median {rates[len(rates) // 2]:.1f} (min {rates[0]:.1f}, max {rates[-1]:.1f}) img/s")
    ops.profile_begin()
    fn()
    prof = ops.profile_end()
    fam = {}
    for k, d in prof.items():
        f = fam.setdefault(family(k), [0.0, 0.0, 0])
        f[0] += d["total_ms"]
        f[1] += d["flops"]
        f[2] += d["calls"]
    total = sum(v[0] for v in fam.values())
    say(f"    one profiled call, {total:.2f} ms of kernel time: " + "; ".join(
        f"{k} x{v[2]} {v[0]:.3f} ms ({100 * v[0] / total:.1f} %" + (f", {v[1] / v[0] / 1e9:.0f} TFLOP/s" if v[1] and v[0] > 0.05 else "") + ")"
        for k, v in sorted(fam.items(), key=lambda kv: -kv[1][0])))
    del model, fn
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
with open(cli.out, "w") as f:
    f.write("\n".join(lines) + "\n")
