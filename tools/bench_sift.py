"""Time of the Mean Distance metric's SIFT keypoints on one 512 x 512 pair (GPU box): sift.sift_matches end to end (two detections, the matcher, the host's sort
and mask filter), its stages on their own, and the share of a metric case.  A seeded low-pass noise texture and a shifted, noised copy of it stand for the source
and the edited image.  A record only: nobody had measured this path, so no speed gate is attached.  python tools/bench_sift.py [--size 512] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sift_ref as R  # noqa: E402
from freefine_amd import sift as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=20)
cli = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_sift.py measures on the GPU: there is no CPU fallback"
dev = torch.device("cuda:0")
N = cli.size
img = R.synthetic("noise", N, N, 7)
gen = R.edited(img)
mask = np.zeros((N, N))
mask[N // 4:3 * N // 4, N // 4:3 * N // 4] = 1.0
sift = S.HipSift(dev)


def wall(fn, reps):
    """host clock around work that ends in a device synchronise (the path returns host arrays: every call synchronises); mean, and the spread of the repetitions"""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.mean(ts)), float(np.min(ts)), float(np.max(ts))


def events(fn, reps):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


kp1, d1 = sift.detect_and_compute(img)
kp2, d2 = sift.detect_and_compute(gen)
pts = S.sift_matches(img, gen, mask, sift)
print(f"sift_matches on one {N} x {N} pair (seeded low-pass noise and its shifted, noised copy; one MI355X): {len(kp1)} / {len(kp2)} keypoints, "
      f"{len(sift.match_ratio(d1, d2))} ratio-test matches, {len(pts)} in the mask")
m, lo, hi = wall(lambda: S.sift_matches(img, gen, mask, sift), cli.reps)
print(f"  sift_matches end to end (host clock, synchronised; {cli.reps} repetitions): mean {m:.2f} ms, min {lo:.2f}, max {hi:.2f}")
m, lo, hi = wall(lambda: sift.detect_and_compute(img), cli.reps)
print(f"  detect_and_compute, one image (uploads, {S.n_octaves((2 * N, 2 * N))} octaves, one count read back per octave, records and descriptors downloaded, host sort): "
      f"mean {m:.2f} ms, min {lo:.2f}, max {hi:.2f}")
base = sift.base(img)
pyr = sift.pyramid(base)
print(f"  device stages (HIP events, mean of {cli.reps}):")
print(f"    base image + pyramid ({sum(5 for _ in pyr) + 1} blurs): {events(lambda: sift.pyramid(sift.base(img)), cli.reps) * 1e3:.0f} us")
D, cand = sift.extrema(pyr[0])
print(f"    DoG + extrema, octave 0 ({pyr[0].shape[1]} x {pyr[0].shape[2]}, {len(cand)} candidates; includes the count's read-back): "
      f"{events(lambda: sift.extrema(pyr[0]), cli.reps) * 1e3:.0f} us")
rec = sift.refine(D, pyr[0], 0, cand)
kp0 = S.records_to_keypoints(rec.cpu().numpy(), 0)
print(f"    refine + orient, octave 0 ({len(cand)} candidates): {events(lambda: sift.refine(D, pyr[0], 0, cand), cli.reps) * 1e3:.0f} us")
print(f"    describe, octave 0 ({len(kp0)} keypoints; includes their upload): {events(lambda: sift.describe(pyr[0], 0, kp0), cli.reps) * 1e3:.0f} us")
a, b = torch.from_numpy(d1).to(dev), torch.from_numpy(d2).to(dev)
print(f"    knn2 ({len(d1)} x {len(d2)} descriptors): {events(lambda: sift.knn2(a, b), cli.reps) * 1e3:.0f} us")
