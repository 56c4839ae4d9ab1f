"""Throughput of the Human Preference Score at the metric's shape (GPU box): OpenCLIP ViT-H/14 at FULL depth (32 image layers, 24 text layers), seeded random
weights (no HPSv2 checkpoint exists offline), 64 decoded 512 x 512 uint8 images and one prompt per call of HipHPSv2.score_u8, in fp32, split-bf16 (x3) and bf16.
Per mode: images per second over windows of at least `--window` seconds between two device events on the launch stream (host work between the events counts:
the device waits for it), the shape warmed first; then one profiled call (ops.profile_begin / profile_end: device time per kernel, from the `_timed` table) split
into the igemm, attention, layernorm and the two entries this metric added (ffn_pool_layernorm, ffn_cosine_rows).  Nothing gates on these numbers.
python tools/hps_time.py [--out profiles/hps_throughput.txt] [--batch 64] [--side 512] [--repeats 3] [--layers 32 24]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freefine_amd import clipvision as CV  # noqa: E402
from freefine_amd import hps, ops  # noqa: E402
from freefine_amd import text as FT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hps_throughput.txt"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=1.0, help="least seconds of work per timed window")
ap.add_argument("--layers", type=int, nargs=2, default=(32, 24), help="image and text layers (default: ViT-H/14's)")
cli = ap.parse_args()
assert torch.cuda.is_available(), "hps_time.py measures on the GPU; there is no CPU fallback"
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
    for key, fam in (("pool_layernorm", "pool_layernorm (new)"), ("cosine_rows", "cosine_rows (new)"), ("igemm", "igemm"), ("attn", "attention"),
                     ("layernorm", "layernorm"), ("split_pair", "split_pair"), ("patch_rows", "patch rows"), ("resize", "resize"), ("embed_tokens", "embed_tokens")):
        if key in name:
            return fam
    return name


vcfg = hps.openclip_vision_config(dict(vars(hps.openclip_vision_config("vith14")), num_hidden_layers=cli.layers[0]))
tcfg = FT.text_projection_config(dict(vars(FT.text_projection_config("vith14")), num_hidden_layers=cli.layers[1]))
state = dict(CV.synthetic_state(vcfg, 0), **FT.synthetic_text_state(tcfg, 1))
imgs = np.random.default_rng(0).integers(0, 256, (cli.batch, cli.side, cli.side, 3), dtype=np.uint8)
prompt = "a photo of a red cup on a wooden table, studio lighting"
tok = FT.ByteTokenizer()          # ids < 259 of the 49408-row table: the lookup's cost does not depend on which rows

say(f"Human Preference Score, OpenCLIP ViT-H/14 ({cli.layers[0]} image layers, {cli.layers[1]} text layers), {cli.batch} images of {cli.side} x {cli.side} uint8 and one "
    f"prompt per call; seeded random weights (no HPSv2 checkpoint offline: parity against the published checkpoint is unmeasured); {torch.cuda.get_device_name(0)}")
say(f"device events around windows of >= {cli.window:.1f} s, {cli.repeats} windows per mode; images per second")
for mode, dt, x3 in (("fp32", torch.float32, False), ("x3", torch.float32, True), ("bf16", torch.bfloat16, False)):
    model = hps.HipHPSv2.from_state(state, tok, vcfg, tcfg, dtype=dt, device=dev, x3=x3)
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
