"""Timings of the Background / Subject Consistency feature paths at the metrics' shape (GPU box): CLIP ViT-B/32 and DINO ViT-B/16, batches of decoded 512 x 512
uint8 images with their keep masks, fp32 and bf16.  Two paths per extractor, alternating in one run, each window at least a second of work between two device
events on the launch stream (host work between the events counts: the device waits for it), every shape warmed first:
  device   features_u8 on HOST uint8 arrays: upload of images and masks, ffn_resize_pil_u8 (mask + resize + crop), ffn_vit_patch_rows, the tower
  host     the reference's preparation in this process (numpy mask, PIL resize, crop, ToTensor, Normalize with torch), upload of the float tensor, forward
Seeded random weights, images and masks.  Nothing gates on these numbers.
python tools/bench_consistency.py [--out profiles/consistency_features_bench.txt] [--batch 32] [--side 512] [--repeats 3]"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freefine_amd import clipvision as CV  # noqa: E402
from freefine_amd import dino as FD  # noqa: E402
from freefine_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_features_bench.txt"))
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=1.0, help="least seconds of work per timed window")
cli = ap.parse_args()
assert torch.cuda.is_available(), "bench_consistency.py measures on the GPU; there is no CPU fallback"
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
B, S, SIZE = cli.batch, cli.side, 224
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, n):
    """n calls between two device events -> seconds"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3


def calls_for(fn, cap=20000):
    """warm the shape, then the number of calls that fill the window"""
    for _ in range(2):
        fn()
    t = window(fn, 3) / 3
    return max(1, min(cap, int(math.ceil(cli.window / max(t, 1e-7)))))


def spread(v):
    v = sorted(v)
    return f"median {v[len(v) // 2]:.1f} (min {v[0]:.1f}, max {v[-1]:.1f})"


from PIL import Image  # noqa: E402

rng = np.random.default_rng(0)
imgs = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
m1 = np.zeros((B, S, S), np.uint8)
m2 = np.zeros((B, S, S), np.uint8)
m1[:, S // 8:S // 2, S // 8:S // 2] = 255
m2[:, S // 3:3 * S // 4, S // 3:3 * S // 4] = 255
prep_clock = [0.0]


def host_prepare(kind):
    t0 = time.perf_counter()
    if kind == "clip":
        keep, flt, (mean, std) = ((m1 + m2) < 128), Image.BICUBIC, (CV.CLIP_MEAN, CV.CLIP_STD)
    else:
        keep, flt, (mean, std) = (m1 > 128), Image.BILINEAR, (FD.IMAGENET_MEAN, FD.IMAGENET_STD)
    mean32 = torch.as_tensor(np.array(mean), dtype=torch.float32).view(-1, 1, 1)
    std32 = torch.as_tensor(np.array(std), dtype=torch.float32).view(-1, 1, 1)
    oh, ow = ops.torchvision_resize_size(S, S, SIZE)
    out = torch.empty(B, 3, SIZE, SIZE)
    for i in range(B):
        small = np.array(Image.fromarray(imgs[i] * keep[i][..., None].astype(np.uint8)).resize((ow, oh), flt))[:SIZE, :SIZE]
        out[i] = torch.from_numpy(small).permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(mean32).div_(std32)
    prep_clock[0] += time.perf_counter() - t0
    return out


say(f"Background / Subject Consistency features, {B} images of {S} x {S} uint8 with keep masks per batch -> {SIZE} x {SIZE}; seeded random weights, images and masks; "
    f"{torch.cuda.get_device_name(0)}")
say(f"device events around windows of >= {cli.window:.1f} s, {cli.repeats} windows per path, the paths alternating; images per second")
for kind, label in (("clip", "CLIP ViT-B/32 (BGC, rule SUM_LT128, bicubic + centre crop)"), ("dino", "DINO ViT-B/16 (SUBC, rule GT128, bilinear)")):
    for dt in (torch.float32, torch.bfloat16):
        if kind == "clip":
            cfg = CV.clip_vision_config("vitb32")
            net = CV.HipCLIPVision(cfg, CV.synthetic_state(cfg, 0), dtype=dt, device=dev)
            keep = ("sum_lt128", m1, m2)
        else:
            cfg = FD.dino_config("vitb16")
            net = FD.HipDino(cfg, FD.synthetic_state(cfg, 0), dtype=dt, device=dev)
            keep = ("gt128", m1, None)
        paths = (("device (host uint8 in)", lambda: net.features_u8(imgs, keep=keep)), ("host (numpy + PIL + torch, float upload)", lambda: net.forward(host_prepare(kind))))
        same = torch.equal(net.features_u8(imgs, keep=keep), net.forward(host_prepare(kind)))
        n = [calls_for(fn) for _, fn in paths]
        rates = [[] for _ in paths]
        prep_share = []
        for _ in range(cli.repeats):
            for i, (_, fn) in enumerate(paths):
                prep_clock[0] = 0.0
                t = window(fn, n[i])
                rates[i].append(B * n[i] / t)
                if i == 1:
                    prep_share.append(prep_clock[0] / t)
        say(f"{label}, {dt}: device path == host path bit for bit: {same}")
        for i, (name, _) in enumerate(paths):
            say(f"  {name:42s} {n[i]:4d} calls per window: {spread(rates[i])} img/s")
        say(f"  host path: {100 * float(np.median(prep_share)):.0f} % of its window is the preparation on the host (one process)")
        del net
with open(cli.out, "w") as f:
    f.write("\n".join(lines) + "\n")
