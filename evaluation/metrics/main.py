"""The GeoBench metric driver on the MI355X engine -- the same command line as the reference's evaluation/metrics/main.py:

    python evaluation/metrics/main.py --path <generated_results.json> [--task 100111111] [--level 0..3] [--no_rotate] [--3d]
           [--use_relative_path --base_dir <GeoBenchMeta>] [--fid_path <real images>] [--gen_img_key gen_img_path]
           [--clip_weights <file>] [--dino_weights <file>] [--dinov2_weights <file>] [--model <SD folder | synthetic:sd21-base>] [--precision f32|x3]
           [--hps_weights <file> --hps_tokenizer <folder>] [--irs_weights <file> --irs_tokenizer <folder>] [--md_visible_only] [--md_keypoints default|sift]
           [--fid_weights <file>]

--task is nine digits (1 = compute): FID, IRS, HPS, BGC, SUBC, WRAP_E, MD, FID_DINO, FID_KD.  The reference downloads its extractors (clip.load, torch.hub); there
is no download here, the weights are local files: --clip_weights (CLIP ViT-B/32: a transformers CLIPVisionModelWithProjection state dict or the OpenAI
checkpoint's visual.* names), --dino_weights (dino_vitb16), --dinov2_weights (dinov2_vitb14), each a .safetensors file or a torch.save'd state dict;
--model is the Stable-Diffusion checkpoint whose features Mean Distance matches; --hps_weights is `HPS_v2.1_compressed.pt` (its state_dict in open_clip's layout,
or transformers' CLIPModel layout) and --hps_tokenizer a folder with CLIP's vocab.json and merges.txt (HPS: OpenCLIP ViT-H/14, freefine_amd/hps.py);
--irs_weights is `ImageReward.pt` (its state_dict: blip.visual_encoder.*, blip.text_encoder.*, mlp.layers.*) and --irs_tokenizer a folder with
bert-base-uncased's vocab.txt (IRS: BLIP ViT-L/16 and BLIP's cross-attending BERT, freefine_amd/irs.py, pinned to transformers' BlipVisionModel / BlipTextModel;
parity with the published checkpoint is unmeasured); --fid_weights is the `pt_inception-2015-12-05` state dict of pytorch-fid (.pth or .safetensors; FID:
Inception-v3 written from its published topology, freefine_amd/inception.py, held to the torch restatement tests/inception_ref.py -- torchvision is not installed,
parity with the published checkpoint and with torchvision's classes is unmeasured) and needs --fid_path, the folder of real images; without either FID is
reported as `not built` into this run, and the other metrics still run.  A metric whose weights were not given is reported as such, likewise.  FID is always
computed in fp32, whatever --precision says (11.5 GFLOP per image: seconds for a whole run).  --precision is the arithmetic of the networks: f32 (default: exact-fp32 MFMA) or x3 (split-bf16: hi + lo bf16 operand pairs, fp32
accumulation; the ViT towers, HPS's two among them, are built with x3=True and the MD pipeline with from_pretrained(..., x3=True)).
For an edit that is neither a translation, a 2-D rotation nor a uniform scale, MD reads the case's correspondence map: <tree>/correspondence/<da>/<ins>/<edit>.npy
beside the folder of generated images (the 3d_rgb variant of evaluation/FreeFine/freefine_batch_infer_2d.py writes it with --save-correspondence).
--md_visible_only (an extension of the reference's metric, off by default: values compare with the reference's only without it) drops the keypoints the
sibling correspondence_visible/....png marks as hidden in the coarse edit.
--md_keypoints sift takes MD's keypoints as the reference does, from SIFT matches between the source and the edited image that pass Lowe's ratio test and start inside the
object mask (freefine_amd/sift.py, on the device; Lowe's SIFT with OpenCV's default parameters -- parity with cv2's own output is unmeasured, and where the reference falls
back to ORB this falls back to SIFT detections).  The default, `default`, is the sample's own "keypoints" list or every s-th mask pixel, as before."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

NAMES = ("FID", "IRS", "HPS", "BGC", "SUBC", "WRAP_E", "MD", "FID_DINO", "FID_KD")
NOT_BUILT = {"FID": "not built into this run (--fid_weights / --fid_path missing)",
             "IRS": "not built into this run (--irs_weights / --irs_tokenizer missing)"}      # both are built: run() answers them before this table is read
LEVEL_WORDS = {1: ("lightly", "slightly", "gently", "mildly"), 2: ("moderately", "markedly", "appreciably"), 3: ("heavily", "intensely", "significantly", "strongly")}
PATH_KEYS = ("ori_img_path", "coarse_input_path", "ori_mask_path", "tgt_mask_path")


def samples(data):
    """(instance dict, case id, sample) of every case of a result tree data[image]["instances"][instance][case]"""
    for image in data.values():
        for instance in image["instances"].values():
            for case_id in list(instance):
                yield instance, case_id, instance[case_id]


def edit_level(prompt):
    low = prompt.lower()
    for level, words in LEVEL_WORDS.items():
        if any(w in low for w in words):
            return level
    raise ValueError(f"No Level found for {prompt}")


def filter_data(data, args):
    """the reference's filters, in its order: --level keeps the cases whose edit_prompt names that level, --no_rotate drops the cases with a rotation
    (edit_param[5] != 0), --3d takes mask and coarse input from target_mask_0 / coarse_input_path_0, --use_relative_path joins the paths to --base_dir"""
    for instance, case_id, sample in samples(data):
        if args.level and edit_level(sample.get("edit_prompt", "")) != args.level:
            del instance[case_id]
        elif args.no_rotate and sample.get("edit_param", "")[5] != 0:
            del instance[case_id]
    for _, _, sample in samples(data):
        if args.three_d:
            sample["tgt_mask_path"], sample["coarse_input_path"] = sample["target_mask_0"], sample["coarse_input_path_0"]
        if args.use_relative_path:
            for key in PATH_KEYS + (args.gen_img_key,):
                if key in sample:
                    sample[key] = os.path.join(args.base_dir, sample[key])
    return data


def load_state(path):
    """a .safetensors file or a torch.save'd state dict (loaded as data: weights_only)"""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    import torch
    st = torch.load(path, map_location="cpu", weights_only=True)
    return st.get("state_dict", st) if isinstance(st, dict) else st


def build_parser():
    ap = argparse.ArgumentParser(description="Evaluation")
    ap.add_argument("--path", required=True, help="JSON file of generated results")
    ap.add_argument("--level", default=0, type=int, help="edit level (0 = all, 1 = easy, 2 = medium, 3 = hard)")
    ap.add_argument("--task", default="100111111", type=str, help="nine digits, 1 = compute: " + ", ".join(NAMES))
    ap.add_argument("--gen_img_key", default="gen_img_path", help="JSON key of the generated image paths")
    ap.add_argument("--no_rotate", action="store_true", help="leave out the cases with a rotation")
    ap.add_argument("--3d", dest="three_d", action="store_true", help="use the 3-D evaluation's masks and coarse inputs")
    ap.add_argument("--fid_path", default=None, help="folder of real images (FID, FID_DINO, FID_KD)")
    ap.add_argument("--use_relative_path", action="store_true", help="join the JSON's paths to --base_dir")
    ap.add_argument("--base_dir", default=None, help="base folder of relative paths")
    ap.add_argument("--clip_weights", default=None, help="CLIP ViT-B/32 weights (BGC)")
    ap.add_argument("--dino_weights", default=None, help="DINO ViT-B/16 weights (SUBC)")
    ap.add_argument("--dinov2_weights", default=None, help="DINOv2 ViT-B/14 weights (FID_DINO, FID_KD)")
    ap.add_argument("--model", default=None, help="Stable-Diffusion folder or synthetic:<name> (MD)")
    ap.add_argument("--hps_weights", default=None, help="HPS_v2.1_compressed.pt: OpenCLIP ViT-H/14 weights, open_clip or transformers layout (HPS)")
    ap.add_argument("--hps_tokenizer", default=None, help="folder with CLIP's vocab.json and merges.txt (HPS)")
    ap.add_argument("--irs_weights", default=None, help="ImageReward.pt: BLIP ViT-L/16, BLIP's BERT and the reward head (IRS)")
    ap.add_argument("--irs_tokenizer", default=None, help="folder with bert-base-uncased's vocab.txt (IRS)")
    ap.add_argument("--fid_weights", default=None, help="pt_inception-2015-12-05 state dict of pytorch-fid, .pth or .safetensors (FID; needs --fid_path)")
    ap.add_argument("--precision", default="f32", choices=("f32", "x3"), help="arithmetic of the networks: f32 = exact fp32, x3 = split-bf16 (FID stays in fp32)")
    ap.add_argument("--md_visible_only", action="store_true", help="MD: drop keypoints hidden in the coarse 3-D edit (needs correspondence_visible images; "
                                                                   "not the reference's metric)")
    ap.add_argument("--md_keypoints", default="default", choices=("default", "sift"),
                    help="MD: where the keypoints come from.  default = the sample's own list or every s-th mask pixel; sift = SIFT ratio-test matches between "
                         "source and edited image inside the mask, on the device (the reference's kind of point set; parity with cv2 is unmeasured)")
    ap.add_argument("--clip_config", default="vitb32", help=argparse.SUPPRESS)        # "tiny": the test sizes
    ap.add_argument("--dino_config", default="vitb16", help=argparse.SUPPRESS)
    ap.add_argument("--hps_config", default="vith14", choices=("vith14", "tiny"), help=argparse.SUPPRESS)      # with "tiny", --hps_tokenizer bytes: text.ByteTokenizer
    ap.add_argument("--irs_config", default="med", choices=("med", "tiny"), help=argparse.SUPPRESS)            # with "tiny", --irs_tokenizer bytes: text.ByteTokenizer
    ap.add_argument("--fid_config", default="full", choices=("full", "tiny"), help=argparse.SUPPRESS)          # "tiny": the test widths, input side 75
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if len(args.task) != len(NAMES) or set(args.task) - set("01"):
        ap.error(f"--task takes {len(NAMES)} digits of 0 / 1")
    if args.use_relative_path and args.base_dir is None:
        ap.error("--use_relative_path needs --base_dir")
    with open(args.path) as f:
        data = filter_data(json.load(f), args)
    label = args.gen_img_key
    want = [n for n, t in zip(NAMES, args.task) if t == "1"]
    x3 = args.precision == "x3"

    def dinov2():
        return load_state(args.dinov2_weights)

    def run(name):
        import torch
        from freefine_amd import metrics as FM
        if name == "IRS":
            if not args.irs_weights or not args.irs_tokenizer:
                return NOT_BUILT["IRS"]
            from freefine_amd import irs
            vcfg, tcfg = ("tiny16", "tiny") if args.irs_config == "tiny" else ("vitl16", "med")
            model = irs.HipImageReward.from_state(load_state(args.irs_weights), irs.load_tokenizer(args.irs_tokenizer), vcfg, tcfg, dtype=torch.float32, x3=x3)
            return FM.calculate_irs(data, label, model)
        if name == "FID":
            if not args.fid_weights or not args.fid_path:
                return NOT_BUILT["FID"]
            return FM.calculate_fid(data, label, args.fid_path, load_state(args.fid_weights), config=args.fid_config, side=75 if args.fid_config == "tiny" else None)
        if name in NOT_BUILT:
            return NOT_BUILT[name]
        if name == "HPS":
            if not args.hps_weights or not args.hps_tokenizer:
                return "not built into this run (--hps_weights / --hps_tokenizer missing)"
            from freefine_amd import hps
            vcfg, tcfg = ("tiny14", "tiny") if args.hps_config == "tiny" else ("vith14", "vith14")
            model = hps.HipHPSv2.from_state(load_state(args.hps_weights), hps.load_tokenizer(args.hps_tokenizer), vcfg, tcfg, dtype=torch.float32, x3=x3)
            return FM.calculate_hps(data, label, model)
        if name == "BGC":
            if not args.clip_weights:
                return "not run (--clip_weights missing)"
            from freefine_amd.clipvision import HipCLIPVision
            return FM.calculate_bgc(data, label, HipCLIPVision(args.clip_config, load_state(args.clip_weights), dtype=torch.float32, x3=x3))
        if name == "SUBC":
            if not args.dino_weights:
                return "not run (--dino_weights missing)"
            from freefine_amd.dino import HipDino, dino_config
            return FM.calculate_subc(data, label, HipDino(dino_config(args.dino_config), load_state(args.dino_weights), dtype=torch.float32, x3=x3))
        if name == "WRAP_E":
            return FM.calculate_we(data, label)
        if name == "MD":
            if not args.model:
                return "not run (--model missing)"
            from freefine_amd.pipeline import FreeFinePipeline
            return FM.calculate_md(data, label, FreeFinePipeline.from_pretrained(args.model, torch_dtype=torch.float32, device=torch.device("cuda:0"), x3=x3),
                                   keypoints="sift" if args.md_keypoints == "sift" else None, visible_only=args.md_visible_only)
        if not args.dinov2_weights or not args.fid_path:
            return "not run (--dinov2_weights or --fid_path missing)"
        return (FM.calculate_fid_dino if name == "FID_DINO" else FM.calculate_fid_kd)(data, label, args.fid_path, dinov2(), x3=x3)

    result = {}
    for name in want:
        print(f"-----{name}-----", flush=True)
        result[name] = run(name)
    print("-----Result-----")
    for k, v in result.items():
        print(f"{k}: {v}")
    return result


if __name__ == "__main__":
    main()
