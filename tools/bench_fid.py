"""Timings of the FID feature path at the metric's shape (GPU box): pytorch-fid's Inception-v3 (freefine_amd/inception.py HipFIDInception, full size), batches of
64 decoded uint8 images, fp32 -- the only arithmetic the network has.
  features_u8   from device-resident uint8 images of --side: PIL bilinear resize to 224, ffn_fid_prep to 299, the network
  network       from device-resident 224 x 224 bytes: ffn_fid_prep and the network
each the median of --repeats windows of at least --window seconds between two device events on the launch stream, warmed first; then one profiled batch
(ops.profile_begin / profile_end: device time between events around every launch) summed per layer class -- convolutions by kernel size and stride, pooling,
preparation -- with the convolutions' share of the 157.3 TFLOP/s fp32 MFMA ceiling.  Seeded random weights and images.
python tools/bench_fid.py [--out profiles/fid_bench.txt] [--batch 64] [--side 512] [--repeats 5]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freefine_amd import ops  # noqa: E402
from freefine_amd.inception import HipFIDInception, synthetic_state  # noqa: E402

PEAK_TF = 157.3
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid_bench.txt"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window", type=float, default=1.0, help="least seconds of work per timed window")
cli = ap.parse_args()
assert torch.cuda.is_available(), "bench_fid.py measures on the GPU; there is no CPU fallback"
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


def measure(fn):
    fn()
    one = window(fn, 1)
    n = max(1, math.ceil(cli.window / max(one, 1e-6)))
    return float(np.median([window(fn, n) / n for _ in range(cli.repeats)]))


net = HipFIDInception("full", synthetic_state("full", 0), device=dev)
rng = np.random.default_rng(0)
big = torch.from_numpy(rng.integers(0, 256, (cli.batch, cli.side, cli.side, 3), dtype=np.uint8)).to(dev)
small = ops.resize_pil_bilinear_u8(big, 224, 224)
say(f"FID features, Inception-v3 full size, fp32, batch {cli.batch}, {torch.cuda.get_device_name(0)}")
for name, fn in (("features_u8", lambda: net.features_u8(big)), ("network", lambda: net.features_224(small))):
    t = measure(fn)
    say(f"  {name:12s} {1e3 * t:9.2f} ms per batch   {cli.batch / t:9.1f} images/s")

ops.profile_begin()
net.features_u8(big)
prof = ops.profile_end()
total = sum(d["total_ms"] for d in prof.values())
flops = sum(d["flops"] for d in prof.values())
say(f"one profiled batch: {total:.2f} ms in {sum(d['calls'] for d in prof.values())} launches, {flops / cli.batch * 1e-9:.2f} GFLOP per image")
say(f"  {'layer class':28s} {'calls':>5s} {'ms':>9s} {'share':>7s} {'TFLOP/s':>9s} {'of 157.3':>9s}")
for name, d in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"]):
    tf = d["flops"] / (d["total_ms"] * 1e-3) * 1e-12 if d["flops"] else 0.0
    say(f"  {name:28s} {d['calls']:5d} {d['total_ms']:9.3f} {100 * d['total_ms'] / total:6.1f}% " + (f"{tf:9.1f} {100 * tf / PEAK_TF:8.1f}%" if d["flops"] else f"{'-':>9s} {'-':>9s}"))
conv_ms = sum(d["total_ms"] for d in prof.values() if d["flops"])
say(f"  all convolutions: {flops / (conv_ms * 1e-3) * 1e-12:.1f} TFLOP/s = {100 * flops / (conv_ms * 1e-3) * 1e-12 / PEAK_TF:.1f}% of the fp32 MFMA ceiling")
if cli.out:
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as f:
        f.write("\n".join(lines) + "\n")
