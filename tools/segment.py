"""Clicks -> mask file: EfficientSAM on the HIP engine (freefine_amd/sam.py), the step in front of FreeFine_generation.

python tools/segment.py --image in.png (--box x1 y1 x2 y2 | --point x y [--point x y ...]) --weights <efficient_sam_vits.pt | synthetic:vits> --out mask.png
                        [--precision f32|x3|bf16]

--box takes two opposite corners in any order (the two clicks of the reference's application); --point foreground points (at most six are used).  The mask is
written as an 8-bit single-channel image of the input's size, 255 inside: what the drivers read as `ori_mask`.  `synthetic:<vits|vitt|tiny>` runs seeded random
weights (no checkpoint exists offline; such a mask means nothing, the run shows that the path works)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--image", required=True)
    ap.add_argument("--box", type=float, nargs=4, metavar=("X1", "Y1", "X2", "Y2"))
    ap.add_argument("--point", type=float, nargs=2, action="append", metavar=("X", "Y"))
    ap.add_argument("--weights", required=True, help="checkpoint file, or synthetic:<vits|vitt|tiny>")
    ap.add_argument("--out", required=True)
    ap.add_argument("--precision", default="f32", choices=["f32", "x3", "bf16"])
    cli = ap.parse_args(argv)
    if (cli.box is None) == (cli.point is None):
        ap.error("give either --box x1 y1 x2 y2 or one or more --point x y")
    return cli


def main(argv=None):
    cli = parse(argv)
    import numpy as np
    import torch
    from PIL import Image
    from freefine_amd import sam
    from src.demo import utils as U
    if not torch.cuda.is_available():
        sys.exit("segment.py runs the network on the GPU; there is no CPU fallback")
    if cli.weights.startswith("synthetic:"):
        cfg = sam.sam_config(cli.weights.split(":", 1)[1])
        state = sam.synthetic_state(cfg, seed=0)
    else:
        state = torch.load(cli.weights, map_location="cpu")
        width = state.get("model", state)["image_encoder.pos_embed"].shape[-1]          # ViT-S is 384 wide, ViT-T 192
        cfg = sam.sam_config({384: "vits", 192: "vitt"}[width])
    model = sam.HipEfficientSam(cfg, state, dtype=torch.bfloat16 if cli.precision == "bf16" else torch.float32, x3=cli.precision == "x3")
    image = np.array(Image.open(cli.image).convert("RGB"))
    if cli.box is not None:
        mask = U.segment_with_box(model, image, cli.box[:2], cli.box[2:])
    else:
        mask = model.segment(image, np.array(cli.point, dtype=np.float32), np.full(len(cli.point), U.LABEL_POINT))
    Image.fromarray(mask, mode="L").save(cli.out)
    print(f"{cli.out}: {mask.shape[1]} x {mask.shape[0]}, {100.0 * (mask > 0).mean():.1f} % inside")


if __name__ == "__main__":
    main()
