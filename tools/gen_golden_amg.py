"""Record tests/golden/g19_amg.npz: what the reference's own segment_anything/utils/amg.py computes on seeded logit stacks -- the pin of tests/maskgen_ref.py.

    python tools/gen_golden_amg.py [--reference <root of the reference tree>]

amg.py is loaded by file path (it needs torch and numpy alone).  Per stack (fp32 [7, 8, 8] and [7, 5, 7], offset 1): calculate_stability_score, batched_mask_to_box
of `> 0` (SAM's rule) and of `>= 0` (the project's), box_xyxy_to_xywh of every such box; and build_point_grid(1, 2, 5).  The maps of a stack: all negative; all
positive; one pixel; a region of exact zeros; values exactly +offset and -offset; a cross touching the four borders; seeded noise.  The file holds arrays only."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"a": (8, 8), "b": (5, 7)}
OFFSET, SEED = 1.0, 19


def special_maps(h, w, seed, offset=OFFSET):
    """fp32 [7, h, w]: the maps listed above"""
    g = np.random.default_rng(seed)
    m = np.empty((7, h, w), dtype=np.float32)
    m[0] = -np.abs(g.standard_normal((h, w))) - offset - 0.25      # nothing above -offset: the quotient is 0 / 0
    m[1] = np.abs(g.standard_normal((h, w))) + 0.25
    m[2] = -3.0
    m[2, h // 2, w - 2] = 2.5
    m[3] = -2.0
    m[3, 1:h - 1, 2:w - 1] = 0.0                      # >= 0 but not > 0
    m[4] = g.standard_normal((h, w)) * 2
    m[4, 1, :] = offset                               # not > +offset
    m[4, h - 2, :] = -offset                          # not > -offset
    m[5] = -1.5
    m[5, h // 2, :] = 1.5
    m[5, :, w // 2] = 1.5
    m[6] = g.standard_normal((h, w)) * 2
    return m


def main(argv=None):
    sys.path.insert(0, ROOT)
    from tools import ref_harness as RH
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=RH.REF)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g19_amg.npz"))
    cli = ap.parse_args(argv)
    path = os.path.join(cli.reference, "evaluation", "GeoDiffuser", "GeoDiffuser", "segment_anything", "utils", "amg.py")
    spec = importlib.util.spec_from_file_location("reference_amg", path)
    amg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(amg)
    out = {"offset": np.float32(OFFSET), "seed": np.int64(SEED)}
    for name, (h, w) in SIZES.items():
        x = torch.from_numpy(special_maps(h, w, SEED + h * w))
        out[f"stack_{name}"] = x.numpy()
        stab = amg.calculate_stability_score(x, 0.0, OFFSET)
        assert stab.dtype == torch.float32
        out[f"stability_{name}"] = stab.numpy()
        for rule, mask in (("gt", x > 0.0), ("ge", x >= 0.0)):
            box = amg.batched_mask_to_box(mask)
            out[f"box_{rule}_{name}"] = box.numpy().astype(np.int64)
            out[f"xywh_{rule}_{name}"] = torch.stack([amg.box_xyxy_to_xywh(b) for b in box]).numpy().astype(np.int64)
    for n in (1, 2, 5):
        out[f"grid_{n}"] = amg.build_point_grid(n)
    assert all(isinstance(v, (np.ndarray, np.generic)) and v.dtype != object for v in out.values())
    np.savez_compressed(cli.out, **out)
    print(f"{cli.out}: {len(out)} arrays, {os.path.getsize(cli.out)} bytes; stability a {out['stability_a'].tolist()}")


if __name__ == "__main__":
    main()
