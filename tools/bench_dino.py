"""Timings of the FID-DINO / Kernel Distance feature path at the metric's shape (GPU box): ViT-B/14, batches of 64 decoded 512 x 512 uint8 images, fp32, split-bf16
(x3) and bf16.
Three paths, alternating in one run, each window at least a second of work between two device events on the launch stream (host work between the events counts:
the device waits for it), every shape warmed first:
  device        HipDinoV2.features_u8 on HOST uint8 arrays: upload of the bytes, ffn_resize_pil_bilinear_u8, ffn_vit_patch_rows, encoder
  device-res.   the same with the uint8 batch already in device memory
  host          the reference's preparation in this process (PIL Resize((224, 224)), ToTensor, Normalize with torch), upload of the float tensor, HipDinoV2.forward;
                its preparation share is also taken with the host clock (the reference spreads it over up to 8 dataloader workers; here it is one process)
and the two preparation kernels alone with the bytes they move.  Seeded random weights and images.
--modes runs another measurement instead: the device path (host uint8 in) of the three arithmetic modes ALTERNATING window by window in one process -- the
comparison of x3 against the fp32 mode of the same run -- and one profiled batch per mode (ops.profile_begin / profile_end: device time per kernel family).
python tools/bench_dino.py [--out profiles/dino_features_bench.txt] [--batch 64] [--side 512] [--repeats 5] [--name vitb] [--modes]"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freefine_amd import ops  # noqa: E402
from freefine_amd.dino import IMAGENET_MEAN, IMAGENET_STD, HipDinoV2, dinov2_config, synthetic_state  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_features_bench.txt"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window", type=float, default=1.0, help="least seconds of work per timed window")
ap.add_argument("--name", default="vitb")
ap.add_argument("--modes", action="store_true", help="fp32 / x3 / bf16 alternating on the device path, and the kernel families of one batch")
cli = ap.parse_args()
assert torch.cuda.is_available(), "bench_dino.py measures on the GPU; there is no CPU fallback"
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

imgs = np.random.default_rng(0).integers(0, 256, (B, S, S, 3), dtype=np.uint8)
imgs_dev = torch.from_numpy(imgs).to(dev)
mean32 = torch.as_tensor(np.array(IMAGENET_MEAN), dtype=torch.float32).view(-1, 1, 1)
std32 = torch.as_tensor(np.array(IMAGENET_STD), dtype=torch.float32).view(-1, 1, 1)
prep_clock = [0.0]


def host_prepare():
    t0 = time.perf_counter()
    out = torch.empty(B, 3, SIZE, SIZE)
    for i in range(B):
        small = np.array(Image.fromarray(imgs[i]).resize((SIZE, SIZE), Image.BILINEAR))
        out[i] = torch.from_numpy(small).permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(mean32).div_(std32)
    prep_clock[0] += time.perf_counter() - t0
    return out


MODES = (("fp32", torch.float32, False), ("x3", torch.float32, True), ("bf16", torch.bfloat16, False))


def family(name):
    """kernel name -> the family the tables speak of"""
    for key, fam in (("igemm_pp", "igemm_pp (ping-pong GEMM)"), ("igemm", "igemm generic tiles"), ("attn", "attention"), ("layernorm", "layernorm"),
                     ("split_pair", "split_pair"), ("patch_rows", "patch rows"), ("resize", "resize")):
        if key in name:
            return fam
    return name


def bench_modes(label, build, call):
    """build(dtype, x3) -> net; call(net) runs one batch of B host uint8 images.  The modes alternate window by window."""
    nets = [(nm, build(dt, x3)) for nm, dt, x3 in MODES]
    fns = [lambda net=net: call(net) for _, net in nets]
    n = [calls_for(fn) for fn in fns]
    rates = [[] for _ in fns]
    for _ in range(cli.repeats):
        for i, fn in enumerate(fns):
            rates[i].append(B * n[i] / window(fn, n[i]))
    say(f"{label}: device path (host uint8 in), {cli.repeats} windows per mode, the modes alternating")
    for i, (nm, _) in enumerate(nets):
        say(f"  {nm:5s} {n[i]:4d} calls per window: {spread(rates[i])} img/s")
    med = [sorted(r)[len(r) // 2] for r in rates]
    say(f"  x3 / fp32 = {med[1] / med[0]:.2f}x (medians; windows {min(rates[1]) / max(rates[0]):.2f}x .. {max(rates[1]) / min(rates[0]):.2f}x), bf16 / fp32 = {med[2] / med[0]:.2f}x")
    for i, (nm, net) in enumerate(nets):
        ops.profile_begin()
        call(net)
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


cfg = dinov2_config(cli.name)
state = synthetic_state(cfg, seed=0)
if cli.modes:
    say(f"DINOv2 {cli.name}/14 class-token features, {B} images of {S} x {S} uint8 per batch -> {SIZE} x {SIZE}; seeded random weights and images; {torch.cuda.get_device_name(0)}")
    say(f"device events around windows of >= {cli.window:.1f} s; images per second")
    bench_modes(f"DINOv2 {cli.name}/14", lambda dt, x3: HipDinoV2(cfg, state, dtype=dt, device=dev, x3=x3), lambda net: net.features_u8(imgs))
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)
say(f"DINOv2 {cli.name}/14 class-token features, {B} images of {S} x {S} uint8 per batch -> {SIZE} x {SIZE}; seeded random weights and images; {torch.cuda.get_device_name(0)}")
say(f"device events around windows of >= {cli.window:.1f} s, {cli.repeats} windows per path, the paths alternating; images per second")
for mode, dt, x3 in MODES:
    net = HipDinoV2(cfg, state, dtype=dt, device=dev, x3=x3)
    paths = (("device (host uint8 in)", lambda: net.features_u8(imgs)), ("device-resident uint8", lambda: net.features_u8(imgs_dev)),
             ("host (PIL + torch, float upload)", lambda: net.forward(host_prepare())))
    same = torch.equal(net.features_u8(imgs), net.forward(host_prepare()))
    n = [calls_for(fn) for _, fn in paths]
    rates = [[] for _ in paths]
    prep_share = []
    for _ in range(cli.repeats):
        for i, (_, fn) in enumerate(paths):
            prep_clock[0] = 0.0
            t = window(fn, n[i])
            rates[i].append(B * n[i] / t)
            if i == 2:
                prep_share.append(prep_clock[0] / t)
    say(f"{mode} ({dt}): device path == host path bit for bit: {same}")
    for i, (label, _) in enumerate(paths):
        say(f"  {label:34s} {n[i]:4d} calls per window: {spread(rates[i])} img/s")
    say(f"  host path: {100 * float(np.median(prep_share)):.0f} % of its window is the preparation on the host (PIL resize + torch normalise, one process)")
    med = [sorted(r)[len(r) // 2] for r in rates]
    say(f"  device / host = {med[0] / med[2]:.2f}x, device-resident / host = {med[1] / med[2]:.2f}x (medians)")
    del net
    torch.cuda.empty_cache()

say("the two preparation kernels alone (device events, windows as above; bytes = what the algorithm reads and writes, from the shapes)")
small = ops.resize_pil_bilinear_u8(imgs_dev, SIZE, SIZE)
out_u8, scratch = torch.empty_like(small), torch.empty(B, S, SIZE, 3, dtype=torch.uint8, device=dev)
lut = ops.vit_norm_table(IMAGENET_MEAN, IMAGENET_STD).to(dev)
resize_bytes = 3.0 * B * (S * S + 2 * S * SIZE + SIZE * SIZE)
fn = lambda: ops.resize_pil_bilinear_u8(imgs_dev, SIZE, SIZE, out=out_u8, scratch=scratch)
n = calls_for(fn)
ts = [window(fn, n) / n for _ in range(cli.repeats)]
say(f"  ffn_resize_pil_bilinear_u8 [{B}, {S}, {S}, 3] -> [{B}, {SIZE}, {SIZE}, 3] (2 kernels): {spread([t * 1e6 for t in ts])} us, {resize_bytes / 1e6:.1f} MB "
    f"-> {resize_bytes / sorted(ts)[len(ts) // 2] / 1e9:.0f} GB/s")
M, ldo = B * (SIZE // 14) ** 2, 592
for dt in (torch.float32, torch.bfloat16):
    rows = torch.empty(M, ldo, dtype=dt, device=dev)
    nbytes = 3.0 * B * SIZE * SIZE + float(M) * ldo * rows.element_size()
    fn = lambda: ops.vit_patch_rows(small, lut, 14, ldo, dt, out=rows)
    n = calls_for(fn)
    ts = [window(fn, n) / n for _ in range(cli.repeats)]
    say(f"  ffn_vit_patch_rows [{B}, {SIZE}, {SIZE}, 3] -> [{M}, {ldo}] {dt}: {spread([t * 1e6 for t in ts])} us, {nbytes / 1e6:.1f} MB -> {nbytes / sorted(ts)[len(ts) // 2] / 1e9:.0f} GB/s")
kx = 608
rows = torch.empty(M, 2 * kx, dtype=torch.bfloat16, device=dev)
nbytes = 3.0 * B * SIZE * SIZE + 4.0 * M * kx
fn = lambda: ops.vit_patch_rows_pair(small, lut, 14, kx, out=rows)
n = calls_for(fn)
ts = [window(fn, n) / n for _ in range(cli.repeats)]
say(f"  ffn_vit_patch_rows_pair [{B}, {SIZE}, {SIZE}, 3] -> [{M}, 2 x {kx}] bf16 pair rows: {spread([t * 1e6 for t in ts])} us, {nbytes / 1e6:.1f} MB -> {nbytes / sorted(ts)[len(ts) // 2] / 1e9:.0f} GB/s")
os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
with open(cli.out, "w") as f:
    f.write("\n".join(lines) + "\n")
