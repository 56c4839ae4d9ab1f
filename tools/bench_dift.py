"""Timings of the Mean Distance metric's DIFT path at the SD-2.1 shape (GPU box): ffn_dift_match against torch's brute force (F.interpolate to the image size +
CosineSimilarity + argmax, the reference's mean_distance.py:144-159) on the same device and inputs, and HipSDFeaturizer.pair (VAE encode + 2E-row UNet up to
the end of up_blocks[1]).  Seeded random weights / features.  python tools/bench_dift.py [--dtype bf16x3|bf16|f32] [--no-featurizer]"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freefine_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="bf16x3", choices=["bf16", "f32", "bf16x3"])
ap.add_argument("--no-featurizer", action="store_true")
cli = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
C, h, w, H, W, K, E = 1280, 32, 32, 512, 512, 30, 8


def timed(fn, reps):
    for _ in range(2):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


g = torch.Generator().manual_seed(0)
base = torch.randn(h, w, C, generator=g) + 0.5
tgt = torch.roll(base, (2, 2), (0, 1)) + 0.3 * torch.randn(h, w, C, generator=g)
dev_s, dev_t = (0.2 * torch.randn(E, h * w, C, generator=g) for _ in range(2))
rows_s = (base.reshape(1, h * w, C) + dev_s - dev_s.mean(0)).to(dev)
rows_t = (tgt.reshape(1, h * w, C) + dev_t - dev_t.mean(0)).to(dev)
rng = np.random.default_rng(1)
kps = [(int(r), int(c)) for r, c in zip(rng.integers(8, 470, K), rng.integers(8, 470, K))]


def brute():
    fs = rows_s.mean(0).reshape(1, h, w, C).permute(0, 3, 1, 2)
    ft = rows_t.mean(0).reshape(1, h, w, C).permute(0, 3, 1, 2)
    Fs, Ft = F.interpolate(fs, (H, W), mode="bilinear"), F.interpolate(ft, (H, W), mode="bilinear")
    cos = torch.nn.CosineSimilarity(dim=1)
    return torch.stack([cos(Fs[0, :, r, c].view(1, C, 1, 1), Ft)[0].flatten().argmax() for r, c in kps])


print(f"match at C={C}, {h}x{w} -> {H}x{W}, K={K}, E={E} (fp32 rows, seeded random features; HIP events, mean of the repetitions)")
t_hip = timed(lambda: ops.dift_match(rows_s, rows_t, (h, w), (H, W), kps), 20)
t_ref = timed(brute, 3)
rc, _ = ops.dift_match(rows_s, rows_t, (h, w), (H, W), kps)
same = int(((rc[:, 0].long() * W + rc[:, 1].long()) == brute()).sum())
print(f"  ffn_dift_match (5 kernels, ensemble mean included): {t_hip * 1e3:.0f} us")
print(f"  torch brute force (mean, 2 x F.interpolate, {K} x CosineSimilarity + argmax, fp32): {t_ref:.1f} ms -> ratio {t_ref / t_hip:.0f}; positions equal {same}/{K}")
rows_b = rows_s.bfloat16(), rows_t.bfloat16()
print(f"  ffn_dift_match, bf16 rows: {timed(lambda: ops.dift_match(rows_b[0], rows_b[1], (h, w), (H, W), kps), 20) * 1e3:.0f} us")

if not cli.no_featurizer:
    from freefine_amd.dift import HipSDFeaturizer
    from freefine_amd.pipeline import FreeFinePipeline
    pipe = FreeFinePipeline.from_pretrained("synthetic:sd21-base", torch_dtype=torch.float32 if cli.dtype != "bf16" else torch.bfloat16, device=dev, x3=cli.dtype == "bf16x3")
    feat = HipSDFeaturizer(pipe)
    img = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img2 = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    noise = torch.randn(E, 4, H // 8, W // 8, generator=g)
    out = {}

    def pair():
        out["r"] = feat.pair(img, img2, "a cup", ensemble_size=E, noise=noise)
    t_pair = timed(pair, 3)
    rs, rt, hw = out["r"]
    print(f"featurizer ({cli.dtype}, synthetic sd21-base, 512^2, t=261, up_ft_index=1, E={E}): pair() = 2 VAE encodes + one {2 * E}-row UNet to the end of up_blocks[1]: "
          f"{t_pair:.1f} ms -> rows {tuple(rs.shape)} stride {rs.stride(1)}, map {hw}")
    t_m = timed(lambda: ops.dift_match(rs, rt, hw, (H, W), kps), 20)
    print(f"  match on those rows: {t_m * 1e3:.0f} us = {100 * t_m / (t_pair + t_m):.1f} % of a case")
