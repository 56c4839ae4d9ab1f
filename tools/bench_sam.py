"""Timings of click-to-mask (GPU box): EfficientSAM ViT-S on 480 x 640 uint8 images, seeded random weights -- `encode` (once per image) at B = 1 and 8 and `predict`
(once per click: one box on a kept embedding, masks at the image size) in each encoder mode (fp32, split-bf16, bf16; the decoder is fp32 in all of them).  Each
figure is the median of --repeats windows of at least --window seconds of calls between two device events, every shape warmed first; host work between the events
(the prompt encoding on the host, the launches) counts, as it does for a caller.  Then one profiled call of each per mode (ops.profile_begin / profile_end: device time
per kernel).
python tools/bench_sam.py [--out profiles/sam_bench.txt] [--name vits] [--repeats 5] [--window 1.0]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freefine_amd import ops, sam  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_bench.txt"))
ap.add_argument("--name", default="vits")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window", type=float, default=1.0, help="least seconds of work per timed window")
cli = ap.parse_args()
assert torch.cuda.is_available(), "bench_sam.py measures on the GPU; there is no CPU fallback"
torch.set_grad_enabled(False)
H, W = 480, 640
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


def timed(fn):
    """median, min, max milliseconds per call"""
    for _ in range(2):
        fn()
    n = max(1, int(math.ceil(cli.window / max(window(fn, 3) / 3, 1e-7))))
    v = sorted(1e3 * window(fn, n) / n for _ in range(cli.repeats))
    return f"median {v[len(v) // 2]:.2f} ms (min {v[0]:.2f}, max {v[-1]:.2f}; {n} calls per window)"


def profile(fn):
    ops.profile_begin()
    fn()
    prof = ops.profile_end()
    total = sum(d["total_ms"] for d in prof.values())
    top = sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])[:6]
    return f"{total:.2f} ms of kernel time in {sum(d['calls'] for d in prof.values())} launches: " + "; ".join(
        f"{k.replace('void ', '').split('(')[0]} x{d['calls']} {d['total_ms']:.2f} ms" for k, d in top)


cfg = sam.sam_config(cli.name)
state = sam.synthetic_state(cfg, seed=0)
imgs = np.random.default_rng(0).integers(0, 256, (8, H, W, 3), dtype=np.uint8)
pts, lab = np.array([[[[0.3 * W, 0.2 * H], [0.8 * W, 0.7 * H]]]], dtype=np.float32), np.array([[[2, 3]]])
say(f"EfficientSAM {cli.name}, {H} x {W} uint8 images, seeded random weights; {torch.cuda.get_device_name(0)}; device events around windows of >= {cli.window:.1f} s")
for mode, dt, x3 in (("fp32", torch.float32, False), ("x3", torch.float32, True), ("bf16", torch.bfloat16, False)):
    net = sam.HipEfficientSam(cfg, state, dtype=dt, x3=x3)
    emb = net.encode(imgs[:1])
    say(f"{mode}:")
    say(f"  encode B=1: {timed(lambda: net.encode(imgs[:1]))}")
    say(f"  encode B=8: {timed(lambda: net.encode(imgs))}")
    say(f"  predict, one box: {timed(lambda: net.predict(emb, pts, lab, (H, W)))}")
    say(f"  encode B=1 profiled: {profile(lambda: net.encode(imgs[:1]))}")
    say(f"  predict profiled: {profile(lambda: net.predict(emb, pts, lab, (H, W)))}")
    del net
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
with open(cli.out, "w") as f:
    f.write("\n".join(lines) + "\n")
