"""Image -> the masks of everything in it: EfficientSAM's point-grid pass on the HIP engine (HipEfficientSam.generate), the `mask_pool` of the edit calls.

python tools/mask_pool.py --image in.png --weights <efficient_sam_vits.pt | synthetic:vits> --out-dir pool/
                          [--points-per-side 32] [--pred-iou-thresh 0.88] [--stability-thresh 0.95] [--nms-thresh 0.7] [--precision f32|x3|bf16]

Writes pool/mask_000.png, mask_001.png, ... (8-bit single-channel, 255 inside, best predicted IoU first) and pool/records.json: per mask its file, area, bbox
(x, y, w, h), predicted_iou, stability_score and point_coords -- everything but the pixels.  src/demo/utils.py mask_pool_from_records turns the records and the
object's own mask into the list get_constrain_areas takes.  `synthetic:<vits|vitt|tiny>` runs seeded random weights (no checkpoint exists offline; such masks
mean nothing, the run shows that the path works)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--image", required=True)
    ap.add_argument("--weights", required=True, help="checkpoint file, or synthetic:<vits|vitt|tiny>")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--points-per-side", type=int, default=32)
    ap.add_argument("--pred-iou-thresh", type=float, default=0.88)
    ap.add_argument("--stability-thresh", type=float, default=0.95)
    ap.add_argument("--nms-thresh", type=float, default=0.7)
    ap.add_argument("--precision", default="f32", choices=["f32", "x3", "bf16"])
    cli = ap.parse_args(argv)
    if cli.points_per_side < 1:
        ap.error("--points-per-side must be at least 1")
    return cli


def main(argv=None):
    cli = parse(argv)
    import numpy as np
    import torch
    from PIL import Image
    from freefine_amd import sam
    if not torch.cuda.is_available():
        sys.exit("mask_pool.py runs the network on the GPU; there is no CPU fallback")
    if cli.weights.startswith("synthetic:"):
        cfg = sam.sam_config(cli.weights.split(":", 1)[1])
        state = sam.synthetic_state(cfg, seed=0)
    else:
        state = torch.load(cli.weights, map_location="cpu")
        width = state.get("model", state)["image_encoder.pos_embed"].shape[-1]          # ViT-S is 384 wide, ViT-T 192
        cfg = sam.sam_config({384: "vits", 192: "vitt"}[width])
    model = sam.HipEfficientSam(cfg, state, dtype=torch.bfloat16 if cli.precision == "bf16" else torch.float32, x3=cli.precision == "x3")
    image = np.array(Image.open(cli.image).convert("RGB"))
    records = model.generate(image, points_per_side=cli.points_per_side, pred_iou_thresh=cli.pred_iou_thresh, stability_score_thresh=cli.stability_thresh,
                             box_nms_thresh=cli.nms_thresh)
    os.makedirs(cli.out_dir, exist_ok=True)
    listing = []
    for i, rec in enumerate(records):
        name = f"mask_{i:03d}.png"
        Image.fromarray(rec["segmentation"], mode="L").save(os.path.join(cli.out_dir, name))
        listing.append(dict({k: v for k, v in rec.items() if k != "segmentation"}, file=name))
    with open(os.path.join(cli.out_dir, "records.json"), "w") as f:
        json.dump(listing, f, indent=1)
    print(f"{cli.out_dir}: {len(records)} masks of {image.shape[1]} x {image.shape[0]} from {cli.points_per_side ** 2} points")


if __name__ == "__main__":
    main()
