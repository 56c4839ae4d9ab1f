"""Device time of the GeoDiffuser warp (warp3d.geodiffuser_coarse_edit) at S = 512 next to the present point-cloud warp (warp3d.coarse_edit_3d) of the
same run, per edit: a record for profiles/, not a gate.

    python tools/bench_geowarp.py [--size 512] [--reps 20] [--out profiles/geowarp_step_time.txt]

Per case: the whole call (host clock around a device synchronise: uploads, the host round trips of the scan and the centre, downloads) and, for the new
step, the per-kernel device time from HIP events on the launch stream (ops.profile_begin / profile_end).  Needs a GPU: no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDITS = {
    "identity": [0, 0, 0, 0, 0, 0, 1, 1, 1],
    "shift": [40, -12, 0, 0, 0, 0, 1, 1, 1],
    "ry35": [0, 0, 0, 0, 35, 0, 1, 1, 1],
    "shrink0.5": [0, 0, 0, 0, 0, 0, 0.5, 0.5, 0.5],
    "combined_tz": [10, 5, -120, 5, -10, 15, 0.8, 0.7, 1.0],
}


def inputs(S, seed=0):
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:S, 0:S].astype(np.float64)
    cy, cx, rad = 0.5 * S, 0.5 * S, 0.3 * S
    blob = (ii - cy) ** 2 + (jj - cx) ** 2 < rad ** 2
    dome = 0.55 - 0.15 * np.clip(1 - ((ii - cy) ** 2 + (jj - cx) ** 2) / rad ** 2, 0, 1)
    depth = (np.where(blob, dome, 0.75 + 0.27 * jj / (S - 1)) + rng.uniform(-0.01, 0.01, (S, S))).astype(np.float32)
    return rng.integers(0, 256, (S, S, 3), dtype=np.uint8), blob.astype(np.uint8) * 255, depth, rng.integers(0, 256, (S, S, 3), dtype=np.uint8)


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_geowarp.py measures on the GPU"
    from freefine_amd import ops, warp3d
    S = args.size
    img, mask, depth, bg = inputs(S)
    lines = [f"S = {S}, {args.reps} repetitions after one warm-up, {torch.cuda.get_device_name(0)}; times in ms per call",
             f"{'edit':<12} {'geodiffuser call':>17} {'present warp call':>18}   new step's kernels (device events): name calls total_ms"]
    for name, edit in EDITS.items():
        new = wall(lambda: warp3d.geodiffuser_coarse_edit(img, mask, depth, edit, bg), args.reps)
        sc = S / 512.0
        tf = [edit[0] * sc, edit[1] * sc, edit[2] * sc] + list(edit[3:])
        old = wall(lambda: warp3d.coarse_edit_3d(img, mask, depth + 0.1 * depth.max(), tf, bg, focal_length=550.0 * sc), args.reps)
        ops.profile_begin()
        for _ in range(args.reps):
            warp3d.geodiffuser_coarse_edit(img, mask, depth, edit, bg)
        prof = ops.profile_end()
        kern = "; ".join(f"{k} {v['calls'] // args.reps} {v['total_ms'] / args.reps:.3f}" for k, v in prof.items())
        lines.append(f"{name:<12} {new:>17.3f} {old:>18.3f}   {kern}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
