"""Timings of the Background / Subject Consistency feature paths at the metrics' shape (GPU box): CLIP ViT-B/32 and DINO ViT-B/16, batches of decoded 512 x 512
uint8 images with their keep masks, fp32, split-bf16 (x3) and bf16.  Two paths per extractor, alternating in one run, each window at least a second of work between two device
events on the launch stream (host work between the events counts: the device waits for it), every shape warmed first:
  device   features_u8 on HOST uint8 arrays: upload of images and masks, ffn_resize_pil_u8 (mask + resize + crop), ffn_vit_patch_rows, the tower
  host     the reference's preparation in this process (numpy mask, PIL resize, crop, ToTensor, Normalize with torch), upload of the float tensor, forward
Seeded random weights, images and masks.  Nothing gates on these numbers.
--modes runs another measurement instead: the device path of the three arithmetic modes ALTERNATING window by window in one process -- the comparison of x3
against the fp32 mode of the same run -- and one profiled batch per mode (ops.profile_begin / profile_end: device time per kernel family).
python tools/bench_consistency.py [--out profiles/consistency_features_bench.txt] [--batch 32] [--side 512] [--repeats 3] [--modes]"""
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
ap.add_argument("--modes", action="store_true", help="fp32 / x3 / bf16 alternating on the device path, and the kernel families of one batch")
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


MODES = (("fp32", torch.float32, False), ("x3", torch.float32, True), ("bf16", torch.bfloat16, False))


def build(kind, dt, x3):
    if kind == "clip":
        cfg = CV.clip_vision_config("vitb32")
        return CV.HipCLIPVision(cfg, CV.synthetic_state(cfg, 0), dtype=dt, device=dev, x3=x3), ("sum_lt128", m1, m2)
    cfg = FD.dino_config("vitb16")
    return FD.HipDino(cfg, FD.synthetic_state(cfg, 0), dtype=dt, device=dev, x3=x3), ("gt128", m1, None)


def family(name):
    """kernel name -> the family the tables speak of"""
    for key, fam in (("igemm_pp", "igemm_pp (ping-pong GEMM)"), ("igemm", "igemm generic tiles"), ("attn", "attention"), ("layernorm", "layernorm"),
                     ("split_pair", "split_pair"), ("patch_rows", "patch rows"), ("resize", "resize")):
        if key in name:
            return fam
    return name


def bench_modes(kind, label):
    """the device path of the three modes, alternating window by window, then one profiled batch per mode"""
    nets = [(nm,) + build(kind, dt, x3) for nm, dt, x3 in MODES]
    fns = [lambda net=net, keep=keep: net.features_u8(imgs, keep=keep) for _, net, keep in nets]
    n = [calls_for(fn) for fn in fns]
    rates = [[] for _ in fns]
    for _ in range(cli.repeats):
        for i, fn in enumerate(fns):
            rates[i].append(B * n[i] / window(fn, n[i]))
    say(f"{label}: device path (host uint8 in), {cli.repeats} windows per mode, the modes alternating")
    for i, (nm, _, _) in enumerate(nets):
        say(f"  {nm:5s} {n[i]:4d} calls per window: {spread(rates[i])} img/s")
    med = [sorted(r)[len(r) // 2] for r in rates]
    say(f"  x3 / fp32 = {med[1] / med[0]:.2f}x (medians; windows {min(rates[1]) / max(rates[0]):.2f}x .. {max(rates[1]) / min(rates[0]):.2f}x), bf16 / fp32 = {med[2] / med[0]:.2f}x")
    for i, (nm, _, _) in enumerate(nets):
        ops.profile_begin()
        fns[i]()
        prof = ops.profile_end()
        fam = {}
        for k, d in prof.items():
            f = fam.setdefault(family(k), [0.0, 0.0])
            f[0] += d["total_ms"]
            f[1] += d["flops"]
        total = sum(v[0] for v in fam.values())
        say(f"  {nm}: one profiled batch, {total:.2f} ms of kernel time: " + "; ".join(
            f"{k} {v[0]:.2f} ms ({100 * v[0] / total:.0f} %" + (f", {v[1] / v[0] / 1e9:.0f} TFLOP/s" if v[1] else "") + ")" for k, v in sorted(fam.items(), key=lambda kv: -kv[1][0])))
        top = sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])[:4]
        say("    " + "; ".join(f"{k.replace('void ', '').split('(')[0]} x{d['calls']} {d['total_ms']:.2f} ms" for k, d in top))


say(f"Background / Subject Consistency features, {B} images of {S} x {S} uint8 with keep masks per batch -> {SIZE} x {SIZE}; seeded random weights, images and masks; "
    f"{torch.cuda.get_device_name(0)}")
say(f"device events around windows of >= {cli.window:.1f} s, {cli.repeats} windows per path, the paths alternating; images per second")
for kind, label in (("clip", "CLIP ViT-B/32 (BGC, rule SUM_LT128, bicubic + centre crop)"), ("dino", "DINO ViT-B/16 (SUBC, rule GT128, bilinear)")):
    if cli.modes:
        bench_modes(kind, label)
        continue
    for mode, dt, x3 in MODES:
        net, keep = build(kind, dt, x3)
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
        say(f"{label}, {mode} ({dt}): device path == host path bit for bit: {same}")
        for i, (name, _) in enumerate(paths):
            say(f"  {name:42s} {n[i]:4d} calls per window: {spread(rates[i])} img/s")
        say(f"  host path: {100 * float(np.median(prep_share)):.0f} % of its window is the preparation on the host (one process)")
        del net
with open(cli.out, "w") as f:
    f.write("\n".join(lines) + "\n")
