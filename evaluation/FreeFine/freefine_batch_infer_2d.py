"""GeoBench-2D batch inference on the MI355X engine -- same entry point as the reference's
evaluation/FreeFine/freefine_batch_infer_2d.py (model setup :148-157, case loop :175-241, result JSON :243-262).

    python evaluation/FreeFine/freefine_batch_infer_2d.py --base-dir <GeoBenchMeta> [--model <SD folder | synthetic:sd21-base>] [--batch 4]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 evaluation/FreeFine/freefine_batch_infer_2d.py --base-dir ...

One process per GPU; cases are sharded like DistributedSampler(shuffle=False), results gathered with all_gather_object, rank 0
writes <base-dir>/generated_results_freefine_2d.json.  The harness itself is freefine_amd/geobench.py."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from src.demo.model import DDIMScheduler, FreeFinePipeline  # noqa: E402
from src.utils.attention import Attention_Modulator, register_attention_control  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-dir", required=True)
    ap.add_argument("--model", default="synthetic:sd21-base")
    ap.add_argument("--dtype", default="bf16x3", choices=["bf16x3", "f32", "bf16"],
                    help="bf16x3 = split-bf16 (default: the mode bench.py times -- holds the 1e-3 latent tolerance at 3x the f32 mode's rate), "
                         "f32 = exact-fp32 parity mode (the reference runs fp32 here), bf16 = fast mode (does NOT hold the tolerance)")
    ap.add_argument("--batch", type=int, default=4, help="cases edited together in one UNet batch")
    ap.add_argument("--variant", default="2d", choices=["2d", "3d_depth", "3d_rgb"],
                    help="3d_rgb: the GeoBench-3D edit with the coarse input rendered here (DepthAnything depth + point-cloud warp) instead of read from disk")
    ap.add_argument("--depth-model", default="synthetic:vitl", help="3d_rgb: a Depth-Anything state dict (.pth) or synthetic:<vits|vitb|vitl>")
    ap.add_argument("--device-prep", action="store_true", help="resize and coarse-edit every case on the device (csrc/caseprep.h) instead of in numpy on the host: "
                                                               "the same bytes, the prefetch thread only decodes the PNG files")
    ap.add_argument("--save-correspondence", action="store_true",
                    help="3d_rgb: also write every case's correspondence map (Geo-Bench-3D/correspondence/<da>/<ins>/<edit>.npy, where Mean Distance looks "
                         "for it) and the visibility image beside it (Geo-Bench-3D/correspondence_visible/...png)")
    ap.add_argument("--warp", default="p3d", choices=["p3d", "geodiffuser"],
                    help="3d_rgb: p3d = this project's point-cloud warp (object pixels only, radius 1.5, K = 5); geodiffuser = the reference's own step 2 "
                         "(the GeoDiffuser warp of get_3d_transform_correspondence.py: every pixel, radius 1.3, K = 15, draw mask = md_mask; square images)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.warp != "p3d" and args.variant != "3d_rgb":
        ap.error("--warp geodiffuser needs --variant 3d_rgb (the other variants do not build the warp)")
    if args.save_correspondence and args.variant != "3d_rgb":
        ap.error("--save-correspondence needs --variant 3d_rgb (the other variants do not build the warp)")
    world = int(os.environ.get("WORLD_SIZE", 1))
    rank, local = int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    device = torch.device(f"cuda:{local}")
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=device)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    model = FreeFinePipeline.from_pretrained(args.model, torch_dtype=dtype, device=device, broadcast="auto", x3=args.dtype == "bf16x3").to(device)
    model._progress_bar_config = {"disable": True}
    model.scheduler = DDIMScheduler.from_config(model.scheduler.config)
    controller = Attention_Modulator(start_layer=10)
    model.controller = controller
    register_attention_control(model, controller)
    model.modify_unet_forward()
    model.enable_attention_slicing()
    model.enable_xformers_memory_efficient_attention()
    model.unet.use_graph = True
    from freefine_amd import geobench
    depth_model = None
    if args.variant == "3d_rgb":
        from freefine_amd import depth as FDp
        if args.depth_model.startswith("synthetic:"):
            dcfg = FDp.depth_config(args.depth_model.split(":")[1])
            dstate = FDp.synthetic_state(dcfg, seed=0)
        else:
            dstate = torch.load(args.depth_model, map_location="cpu", weights_only=True)
            dcfg = FDp.depth_config({384: "vits", 768: "vitb", 1024: "vitl"}[dstate["pretrained.cls_token"].shape[-1]])
        depth_model = FDp.HipDepthAnything(dcfg, dstate, dtype=dtype, device=device)
    geobench.run(model, args.base_dir, batch=args.batch, rank=rank, world=world, variant=args.variant, depth_model=depth_model,
                 device_prep=args.device_prep, save_correspondence=args.save_correspondence, warp=args.warp)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
