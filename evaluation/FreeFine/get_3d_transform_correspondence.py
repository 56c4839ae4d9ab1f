"""Step 2 of the GeoBench-3D run on the MI355X engine, without the diffusion edit -- the step name of the reference's
evaluation/FreeFine/get_3d_transform_correspondence.py (run_script_3D.sh "Step2"): for every case of <base-dir>/annotations.json the coarse image
Geo-Bench-3D/coarse3d_depth_anything_rgb/<da>/<ins>/<edit>.png, the target mask Geo-Bench-3D/mesh_mask/... and the correspondence map
Geo-Bench-3D/correspondence/<da>/<ins>/<edit>.npy (with Geo-Bench-3D/correspondence_visible/...png beside it).

    python evaluation/FreeFine/get_3d_transform_correspondence.py --base-dir <GeoBenchMeta> [--depth-model <file.pth | synthetic:vitl>] [--warp geodiffuser]

--warp p3d (default) is A NON-PARITY EXTENSION (freefine_amd.geobench.prepare_3d, load_case_3d_rgb): this project's own point-cloud warp
(freefine_amd.warp3d.coarse_edit_3d).  --warp geodiffuser is the reference's step itself: the GeoDiffuser warp (get_transformed_mask and what it
calls under evaluation/GeoDiffuser/GeoDiffuser/utils/, which IS in the reference tree) on the HIP kernels of csrc/geowarp.h, written under the
reference's names: Geo-Bench-3D/coarse3d_depth_anything_blended/, mesh_mask/, md_mask/ and correspondence/.  Its coordinates and mesh topology are
pinned to the reference's code; its two rasterisers restate pytorch3d's (absent here) and are not.  One process per GPU, cases sharded by RANK / WORLD_SIZE."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from freefine_amd.geobench import prepare_3d  # noqa: E402,F401


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-dir", required=True)
    ap.add_argument("--depth-model", default="synthetic:vitl", help="a Depth-Anything state dict (.pth) or synthetic:<vits|vitb|vitl>")
    ap.add_argument("--size", type=int, default=512, help="side the cases are resized to")
    ap.add_argument("--overwrite", action="store_true", help="render again the cases whose files exist")
    ap.add_argument("--warp", default="p3d", choices=["p3d", "geodiffuser"],
                    help="p3d: this project's point-cloud warp; geodiffuser: the reference's GeoDiffuser warp, under the reference's folder names (square sizes only)")
    return ap


def main(argv=None):
    import torch
    from freefine_amd import depth as FDp
    args = build_parser().parse_args(argv)
    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    device = torch.device(f"cuda:{local}")
    if args.depth_model.startswith("synthetic:"):
        dcfg = FDp.depth_config(args.depth_model.split(":")[1])
        dstate = FDp.synthetic_state(dcfg, seed=0)
    else:
        dstate = torch.load(args.depth_model, map_location="cpu", weights_only=True)
        dcfg = FDp.depth_config({384: "vits", 768: "vitb", 1024: "vitl"}[dstate["pretrained.cls_token"].shape[-1]])
    depth_model = FDp.HipDepthAnything(dcfg, dstate, dtype=torch.float32, device=device)
    return prepare_3d(args.base_dir, depth_model, rank=rank, world=world, dsize=(args.size, args.size), check_exist=not args.overwrite, warp=args.warp)


if __name__ == "__main__":
    main()
