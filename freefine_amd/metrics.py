"""The GeoBench metric suite (/root/reference/evaluation/metrics/) as far as it can be built offline.

Model-free arithmetic: warp error, the Frechet distance between two Gaussians of features, and the polynomial-kernel MMD^2 (the "kernel distance" of
fid_kd.py); pinned to the reference's own functions by tests/golden/g11_metrics.npz (tools/gen_golden.py run_g11).  Host-side numpy: a metric pass is a few
reductions over at most thousands of feature rows.

FID-DINO (FID/fid_dino.py) and Kernel Distance (FID/fid_kd.py) feed those functions with DINOv2 ViT-B/14 class tokens.  The reference vendors the DINOv2 source
(torchhub/facebookresearch_dinov2_main), so the extractor is built and pinned: freefine_amd/dino.py HipDinoV2 runs the encoder on the project's kernels (pinned to
the vendored DinoVisionTransformer by tests/golden/g14_dinov2_cls.npz, tools/gen_golden.py run_g14) and prepares the images on the device, bit-exact against
PIL (ops.resize_pil_bilinear_u8, ops.vit_patch_rows).  get_activations / calculate_fid_dino / calculate_fid_kd below are the drivers; the WEIGHTS still come
from the caller (a state dict in hub layout: there is no hub download).

Background Consistency (VBench/background_consistency.py) and Subject Consistency (VBench/subject_consistency.py) say whether an edit kept what it should keep:
the cosine between features of the source and the generated image, the background outside both masks (BGC: CLIP ViT-B/32 image embeddings) or the object inside
its mask (SUBC: DINO ViT-B/16 class tokens).  Their extractors are pinned too: freefine_amd/clipvision.py HipCLIPVision to transformers'
CLIPVisionModelWithProjection (the arithmetic of clip's encode_image), freefine_amd/dino.py HipDino to the vendored DinoVisionTransformer at patch 16 without
LayerScale (tests/golden/g15_dino16_cls.npz).  Masking, resizing (PIL bicubic / bilinear bit for bit) and cropping run on the device in one entry
(ops.resize_pil_u8).  consistency_pairs / calculate_bgc / calculate_subc below are the drivers; weights from the caller.

The Human Preference Score (human_preference_score.py) is the cosine between OpenCLIP ViT-H/14 embeddings of a generated image and of its source image's
caption.  freefine_amd/hps.py HipHPSv2 runs both towers and the cosine on the project's kernels, pinned to transformers' CLIP*ModelWithProjection (the same
arithmetic; hpsv2 and open_clip exist nowhere this is tested).  calculate_hps below is the driver; weights and tokenizer files from the caller.

FID itself (FID/fid.py) feeds the Frechet distance with the 2048-d pool3 features of pytorch-fid's Inception-v3.  torchvision is not installed, so the network
is written from its published topology: freefine_amd/inception.py HipFIDInception runs it on the project's convolution and pooling kernels (csrc/convkk.h), held to
the torch restatement tests/inception_ref.py, whose four patched FID blocks are pinned to the reference's classes by tests/golden/g20_fid_blocks.npz.
get_inception_activations / calculate_fid below are the drivers; the weights (the pt_inception-2015-12-05 state dict) come from the caller, and parity with that
checkpoint is unmeasured.  (The ImageReward score: freefine_amd/irs.py, calculate_irs below.)

Mean Distance (MD/mean_distance.py), the one metric of the suite that measures the GEOMETRY of an edit, needs no foreign network: its feature extractor is
DIFT, i.e. Stable Diffusion itself, and runs on the project's kernels (freefine_amd/dift.py: HipVAE + HipUNet.features; the correspondence search is
ops.dift_match).  transform_coordinates / mean_distance / calculate_md below are the metric; the coordinate maps are pinned to the reference's
get_transform_coordinates by tests/golden/g13_md_coords.npz (tools/gen_golden.py run_g13; translation and uniform scale -- the rotation branch calls cv2 there
and is pinned only to the documented matrix formula, src/utils/vis_utils.py::_rotation_matrix_2d).  The reference finds its keypoints with cv2 SIFT matches (ORB when there are none).  cv2 exists nowhere
this is built; by default keypoints are supplied by the caller or come from a documented deterministic sampler (default_keypoints), and MD values are comparable to
the reference's only when the same keypoints are supplied.  Opt-in, calculate_md(..., keypoints="sift"): the keypoints are SIFT ratio-test matches found on the
device (freefine_amd/sift.py: Lowe's SIFT with OpenCV's default parameters, held to the fp64 restatement tests/sift_ref.py -- the same KIND of point set as the
reference's, textured points that survived the edit; parity with cv2's own output is unmeasured, and the no-match fallback is SIFT detections, not ORB)."""
import numpy as np


def warp_error(coarse, generated, mask):
    """one sample of wrap_error.py:calculate_we (:14-17): images uint8 / float HWC in [0, 255], mask HW in [0, 255];
    sum |coarse * m - generated * m| / sum(m) with m the mask / 255 repeated over the 3 channels"""
    a, b = np.asarray(coarse, np.float64) / 255, np.asarray(generated, np.float64) / 255
    m = np.repeat((np.asarray(mask, np.float64) / 255)[..., None], 3, axis=2)
    return float(np.abs(a * m - b * m).sum() / m.sum())


def calculate_we(data, image_label, reader=None):
    """wrap_error.py:calculate_we over a GeoBench result tree data[image]["instances"][instance][sample] with the paths
    coarse_input_path / <image_label> / tgt_mask_path; `reader` maps a path to an array (default: PIL)"""
    if reader is None:
        from PIL import Image
        reader = lambda p: np.array(Image.open(p))
    total, num = 0.0, 0
    for image in data.values():
        for instance in image["instances"].values():
            for sample in instance.values():
                total += warp_error(reader(sample["coarse_input_path"]), reader(sample[image_label]), reader(sample["tgt_mask_path"]))
                num += 1
    return total / num


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """FID/fid_score.py:calculate_frechet_distance (:146-199): ||mu1 - mu2||^2 + Tr(S1 + S2 - 2 sqrt(S1 S2)), with the eps-regularised retry when
    the matrix square root is not finite and the imaginary round-off dropped"""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        off = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + off).dot(sigma2 + off))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def feature_statistics(features):
    """mean and covariance of feature rows, as calculate_activation_statistics (:201-223) computes them (np.cov, rowvar=False)"""
    f = np.asarray(features, np.float64)
    return f.mean(axis=0), np.cov(f, rowvar=False)


def polynomial_mmd2(X, Y, degree=3, gamma=None, coef0=1.0):
    """FID/mmd.py:compute_polynomial_mmd (:24-35, 38-60): unbiased MMD^2 with k(x, y) = (gamma <x, y> + coef0)^degree, gamma = 1 / dim by default;
    X and Y hold the same number of rows"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    m = X.shape[0]
    assert Y.shape[0] == m
    g = 1.0 / X.shape[1] if gamma is None else gamma
    k = lambda A, B: (g * (A @ B.T) + coef0) ** degree
    kxx, kyy, kxy = k(X, X), k(Y, Y), k(X, Y)
    sxx = kxx.sum() - np.trace(kxx)
    syy = kyy.sum() - np.trace(kyy)
    return float((sxx + syy) / (m * (m - 1)) - 2 * kxy.sum() / (m * m))


def kernel_distance(feat_real, feat_gen, n_subsets=100, subset_size=1000, rng=None):
    """FID/mmd.py:compute_mmd (:5-21): MMD^2 over random equally sized subsets (numpy's global generator unless `rng` is given); the reference
    reports the mean of the returned vector (fid_kd.py:39)"""
    rng = np.random if rng is None else rng
    m = min(min(feat_real.shape[0], feat_gen.shape[0]), subset_size)
    out = np.zeros(n_subsets)
    for i in range(n_subsets):
        g = feat_real[rng.choice(len(feat_real), m, replace=False)]
        r = feat_gen[rng.choice(len(feat_gen), m, replace=False)]
        out[i] = polynomial_mmd2(g, r)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# FID-DINO (FID/fid_dino.py) and Kernel Distance (FID/fid_kd.py): DINOv2 class tokens into the two functions above
# ---------------------------------------------------------------------------------------------------------------------------------------------
def get_activations(files, model, batch_size=64, reader=None):
    """fid_score.py:get_activations (:93-143) -> float64 [len(files), C] in file order.  model: a freefine_amd.dino.HipDinoV2 (anything with
    features_u8(uint8 [B, H, W, 3]) -> [B, C]); the transform of the reference's dataset (Resize((224, 224)), ToTensor, Normalize) runs inside it, on the
    device.  Images are grouped by size so that one launch sees one size, batched by `batch_size` within a group (a model's row does not depend on its
    batch), and the rows scattered back to file order.  `reader` maps a path to a uint8 HWC array (default: PIL, converted to RGB)."""
    if reader is None:
        from PIL import Image
        reader = lambda p: np.array(Image.open(p).convert("RGB"))
    images = [np.ascontiguousarray(reader(p), dtype=np.uint8) for p in files]
    groups = {}
    for i, im in enumerate(images):
        assert im.ndim == 3 and im.shape[2] == 3, f"{files[i]}: expected an RGB image, got shape {im.shape}"
        groups.setdefault(im.shape[:2], []).append(i)
    out = None
    for idx in groups.values():
        for s in range(0, len(idx), batch_size):
            part = idx[s:s + batch_size]
            f = model.features_u8(np.stack([images[i] for i in part]))
            f = f.detach().cpu().numpy() if hasattr(f, "detach") else np.asarray(f)
            if out is None:
                out = np.empty((len(files), f.shape[1]), dtype=np.float64)
            out[part] = f
    return np.empty((0, 0)) if out is None else out


def parse_data(data, image_label, real_root_path):
    """fid_dino.py / fid_kd.py:parse_data -> (real files, generated files).  Quirk kept: the real set is the DIRECTORY LISTING of real_root_path (os.listdir
    order), not the samples' ori_img_path entries, which the reference collects and then overwrites."""
    import os
    gen = [sample[image_label] for image in data.values() for instance in image["instances"].values() for sample in instance.values()]
    return [os.path.join(real_root_path, n) for n in os.listdir(real_root_path)], gen


def _dino_model(model, x3=False):
    """a HipDinoV2 as it is; a state dict (DinoVisionTransformer.state_dict() of dinov2_vitb14, hub layout) becomes one in fp32, like the reference's model
    (x3: in split-bf16 arithmetic -- only where the tower is built here; a ready model keeps its own mode)"""
    if isinstance(model, dict):
        import torch
        from .dino import HipDinoV2, dinov2_config
        return HipDinoV2(dinov2_config("vitb"), model, dtype=torch.float32, x3=x3)
    return model


def calculate_fid_dino(data, image_label, real_root_path, model, batch_size=64, reader=None, x3=False):
    """fid_dino.py:calculate_fid_dino: the Frechet distance between the DINOv2 class tokens of the real images (the listing of real_root_path) and of the generated
    ones (data[...][image_label]).  model: a HipDinoV2 or a dinov2_vitb14 state dict (the reference downloads it from the hub; here the caller brings it);
    x3: a tower built from a state dict runs split-bf16 arithmetic."""
    model = _dino_model(model, x3)
    real, gen = parse_data(data, image_label, real_root_path)
    m1, s1 = feature_statistics(get_activations(real, model, batch_size, reader))
    m2, s2 = feature_statistics(get_activations(gen, model, batch_size, reader))
    return frechet_distance(m1, s1, m2, s2)


def calculate_fid_kd(data, image_label, real_root_path, model, batch_size=64, reader=None, x3=False):
    """fid_kd.py:calculate_fid_kd: the mean of kernel_distance(real, generated) over DINOv2 class tokens (numpy's global generator picks the subsets, as in
    the reference); x3 as in calculate_fid_dino"""
    model = _dino_model(model, x3)
    real, gen = parse_data(data, image_label, real_root_path)
    return kernel_distance(get_activations(real, model, batch_size, reader), get_activations(gen, model, batch_size, reader)).mean()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# FID (FID/fid.py): pool3 features of pytorch-fid's Inception-v3 into frechet_distance
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _inception_model(model, config="full", side=None):
    """a HipFIDInception as it is; a state dict (pt_inception-2015-12-05 in pytorch-fid's layout) becomes one (fp32: the network has no other arithmetic)"""
    if isinstance(model, dict):
        from .inception import HipFIDInception
        return HipFIDInception(config, model, side=side)
    return model


def get_inception_activations(files, model, batch_size=64):
    """fid_score.py:get_activations (:93-143) with the Inception-v3 extractor -> float64 [len(files), 2048] in file order.  Every file is opened with
    Image.open(f).convert("RGB"); any size is accepted.  model: a freefine_amd.inception.HipFIDInception; the dataset's transform (Resize((224, 224)) with PIL's
    bilinear filter, ToTensor, Normalize(imagenet)) and the network's own resize to 299 and rescale run inside it, on the device.  Grouping by size, batching and
    the order of the rows are get_activations's."""
    return get_activations(files, model, batch_size)


def calculate_fid(data, image_label, real_root_path, weights, batch_size=64, config="full", side=None):
    """fid.py:calculate_fid: the Frechet distance between the Inception-v3 pool3 features of the real images and of the generated ones (data[...][image_label]).
    The reference's parse_data quirk is kept: the real set is the directory listing of real_root_path (parse_data above).  Statistics in float64 (np.mean,
    np.cov(rowvar=False)).  weights: a HipFIDInception or the state dict it is built from (the reference downloads it; here the caller brings it)."""
    model = _inception_model(weights, config, side)
    real, gen = parse_data(data, image_label, real_root_path)
    m1, s1 = feature_statistics(get_inception_activations(real, model, batch_size))
    m2, s2 = feature_statistics(get_inception_activations(gen, model, batch_size))
    return frechet_distance(m1, s1, m2, s2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Background Consistency (VBench/background_consistency.py) and Subject Consistency (VBench/subject_consistency.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def consistency_pairs(data, image_label):
    """background_consistency.py:parse_data (:9-16) -> [(ori_img_path, generated image path, ori_mask_path, tgt_mask_path), ...]"""
    return [(sample["ori_img_path"], sample[image_label], sample["ori_mask_path"], sample["tgt_mask_path"])
            for image in data.values() for instance in image["instances"].values() for sample in instance.values()]


def _consistency_read(pair, reader):
    """the four arrays of one pair, checked: RGB uint8 images [H, W, 3], mode-"L" uint8 masks [h, w].  Other modes are refused: the reference multiplies the
    image by mask[..., None], which means something else (or fails) for a palette / RGBA image or a multi-channel / 1-bit / 16-bit mask."""
    if reader is None:
        from PIL import Image
        reader = lambda p: np.array(Image.open(p))
    arrs = [np.asarray(reader(p)) for p in pair]
    for p, a in zip(pair[:2], arrs[:2]):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{p}: RGB images only (8 bits, 3 channels); got dtype {a.dtype}, shape {a.shape}")
    for p, a in zip(pair[2:], arrs[2:]):
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError(f"{p}: mode-\"L\" masks only (8 bits, one channel); got dtype {a.dtype}, shape {a.shape}")
    return [np.ascontiguousarray(a) for a in arrs]


def _mask_to(masks, hw, device):
    """uint8 [B, h, w] -> [B, H, W]: PIL's mask.resize(image.size) with the default filter, which for mode "L" is BICUBIC; on the device (ffn_resize_pil_u8 with
    one channel), skipped when the sizes already agree (GeoBench's do)"""
    if tuple(masks.shape[1:]) == tuple(hw):
        return masks
    import torch
    from . import ops
    if device is None:
        raise ValueError(f"masks of {masks.shape[2]} x {masks.shape[1]} for images of {hw[1]} x {hw[0]}: resizing them needs the extractor's `.device`")
    return ops.resize_pil_u8(torch.as_tensor(masks).to(device).contiguous(), hw[0], hw[1], "bicubic")


def consistency_scores(pairs, model, kind, batch_size=32, reader=None):
    """The per-pair values of calculate_bgc (kind "bgc") / calculate_subc (kind "subc"), in the order of `pairs`.  Pairs are grouped by the sizes of their four
    files so that one launch sees one size, batched by `batch_size` within a group.  model: anything with features_u8(uint8 [B, H, W, 3], keep=(rule, m1, m2))
    -> [B, C] and (for masks that need resizing) a `.device`.
      bgc   both masks resized to the SOURCE image's size; keep where (uint8)(m_ori + m_tgt) < 128 -- numpy's uint8 wrap, as in the reference -- applied to the
            source and to the generated image alike, which therefore must have the source's size (the reference's multiplication fails otherwise)
      subc  the source mask (resized to the source image) keeps the source image where it is > 128, the target mask (resized to the generated image) the
            generated image
    then F.normalize, F.cosine_similarity in fp32 and max(0.0, .) per pair."""
    import torch
    import torch.nn.functional as F
    assert kind in ("bgc", "subc")
    loaded = [_consistency_read(p, reader) for p in pairs]
    groups = {}
    for i, (src, gen, m1, m2) in enumerate(loaded):
        if kind == "bgc" and gen.shape != src.shape:
            raise ValueError(f"{pairs[i][1]}: generated image {gen.shape[1]} x {gen.shape[0]} but source {src.shape[1]} x {src.shape[0]}; Background Consistency "
                             "masks both with one mask of the source's size")
        groups.setdefault((src.shape, gen.shape, m1.shape, m2.shape), []).append(i)
    dev = getattr(model, "device", None)
    out = [None] * len(pairs)
    for idx in groups.values():
        for s in range(0, len(idx), batch_size):
            part = idx[s:s + batch_size]
            src, gen, m1, m2 = (np.stack([loaded[i][j] for i in part]) for j in range(4))
            if kind == "bgc":
                a, b = _mask_to(m1, src.shape[1:3], dev), _mask_to(m2, src.shape[1:3], dev)
                fs, fg = model.features_u8(src, keep=("sum_lt128", a, b)), model.features_u8(gen, keep=("sum_lt128", a, b))
            else:
                fs = model.features_u8(src, keep=("gt128", _mask_to(m1, src.shape[1:3], dev), None))
                fg = model.features_u8(gen, keep=("gt128", _mask_to(m2, gen.shape[1:3], dev), None))
            fs, fg = (F.normalize(torch.as_tensor(f).float(), dim=-1, p=2) for f in (fs, fg))
            cos = F.cosine_similarity(fs, fg).cpu()
            for i, c in zip(part, cos):
                out[i] = max(0.0, c.item())
    return out


def _clip_model(model, x3=False):
    """a HipCLIPVision as it is; a state dict (CLIP ViT-B/32: CLIPVisionModelWithProjection.state_dict() or the OpenAI checkpoint's visual.* names) becomes one in fp32
    (x3: in split-bf16 arithmetic)"""
    if isinstance(model, dict):
        import torch
        from .clipvision import HipCLIPVision
        return HipCLIPVision("vitb32", model, dtype=torch.float32, x3=x3)
    return model


def _dino16_model(model, x3=False):
    """a HipDino as it is; a state dict (dino_vitb16 in the vendored DinoVisionTransformer's layout) becomes one in fp32 (x3: in split-bf16 arithmetic)"""
    if isinstance(model, dict):
        import torch
        from .dino import HipDino, dino_config
        return HipDino(dino_config("vitb16"), model, dtype=torch.float32, x3=x3)
    return model


def calculate_bgc(data, image_label, model, batch_size=32, reader=None, x3=False):
    """background_consistency.py:calculate_bgc: the mean over all pairs of the clamped cosine between the CLIP image embeddings of the masked source and the
    masked generated image.  model: a HipCLIPVision or a CLIP ViT-B/32 state dict (the reference's clip.load downloads it; here the caller brings it); x3: a
    tower built from a state dict runs split-bf16 arithmetic."""
    scores = consistency_scores(consistency_pairs(data, image_label), _clip_model(model, x3), "bgc", batch_size, reader)
    return sum(scores) / len(scores)


def calculate_subc(data, image_label, model, batch_size=32, reader=None, x3=False):
    """subject_consistency.py:calculate_subc: the same over DINO ViT-B/16 class tokens of the object cut out by its own mask.  model: a HipDino or a state dict; x3 as in
    calculate_bgc."""
    scores = consistency_scores(consistency_pairs(data, image_label), _dino16_model(model, x3), "subc", batch_size, reader)
    return sum(scores) / len(scores)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Human Preference Score (human_preference_score.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def calculate_hps(data, image_label, model, reader=None, batch_size=32):
    """human_preference_score.py:calculate_hps (:65-83): for every image entry the prompt is image["4v_caption"] and every sample's data[...][image_label] file is
    scored against it; the result is the sum of the scores over the number of samples.  model: a freefine_amd.hps.HipHPSv2 (anything with
    score_u8(uint8 [B, H, W, 3], prompt) -> [B]).  The files of one entry are grouped by size so that one launch sees one size, batched by `batch_size`
    within a group.  `reader` maps a path to a uint8 HWC array (default: PIL, as decoded); RGB only -- open_clip's transform converts other modes, this
    driver refuses them.  No samples: ValueError (the reference divides by zero)."""
    return _mean_caption_score(data, image_label, model, reader, batch_size, "calculate_hps")


def calculate_irs(data, image_label, model, reader=None, batch_size=32):
    """image_reward.py:calculate_irs: the ImageReward score of every sample's data[...][image_label] file given its image entry's image["4v_caption"], summed and
    divided by the number of samples.  model: a freefine_amd.irs.HipImageReward (anything with score_u8(uint8 [B, H, W, 3], prompt) -> [B]).  Grouping by size,
    batching, `reader`, RGB only and the ValueError on no samples are calculate_hps's: one loop serves both."""
    return _mean_caption_score(data, image_label, model, reader, batch_size, "calculate_irs")


def _mean_caption_score(data, image_label, model, reader, batch_size, what):
    """the loop of calculate_hps and calculate_irs (their docstrings)"""
    if reader is None:
        from PIL import Image
        reader = lambda p: np.array(Image.open(p))
    total, number = 0.0, 0
    for image in data.values():
        files = [sample[image_label] for instance in image["instances"].values() for sample in instance.values()]
        if not files:
            continue
        prompt = image["4v_caption"]
        groups = {}
        for p in files:
            a = np.asarray(reader(p))
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"{p}: RGB images only (8 bits, 3 channels); got dtype {a.dtype}, shape {a.shape}")
            groups.setdefault(a.shape[:2], []).append(np.ascontiguousarray(a))
        for imgs in groups.values():
            for s in range(0, len(imgs), batch_size):
                sc = model.score_u8(np.stack(imgs[s:s + batch_size]), prompt)
                sc = sc.detach().cpu().numpy() if hasattr(sc, "detach") else np.asarray(sc)
                total += float(sc.astype(np.float64).sum())
        number += len(files)
    if number == 0:
        raise ValueError(f"{what}: no samples with {image_label!r} in the data")
    return total / number


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Mean Distance (MD/mean_distance.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def transform_coordinates(edit_param, size, mask, path_3D=None):
    """mean_distance.py:get_transform_coordinates (:81-108): [size[0], size[1], 2] float64, where the edit should have moved every pixel (row, col).  Quirks kept:
    the translation branch (edit_param[0] = dx or edit_param[1] = dy non-zero) is (row + dy, col + dx); the rotation (edit_param[5], degrees) / uniform scale
    (edit_param[6] == edit_param[7]) branch works about scipy.ndimage.center_of_mass(mask), a (row, col) pair passed UNCHANGED as the centre of a matrix that
    is applied to (row, col, 1) points; otherwise the correspondence file `path_3D` (.npy, [size[0], size[1], 2] with last axis (x, y): warp3d.save_correspondence
    writes it) with its last axis reversed -- a map of another size raises ValueError (it was an IndexError or a silently wrong lookup).  The rotation matrix is
    cv2.getRotationMatrix2D as restated by src/utils/vis_utils.py::_rotation_matrix_2d (pinned to that formula only: no cv2 here to record a golden)."""
    if edit_param[0] != 0 or edit_param[1] != 0:
        rows, cols = np.meshgrid(np.arange(size[0]), np.arange(size[1]), indexing="ij")
        return np.stack([rows + edit_param[1], cols + edit_param[0]], axis=-1).astype(np.float64)
    if edit_param[5] != 0 or edit_param[6] != 1:
        from scipy.ndimage import center_of_mass
        center = center_of_mass(np.asarray(mask))
        if edit_param[5] != 0:
            from src.utils.vis_utils import _rotation_matrix_2d
            matrix = _rotation_matrix_2d(center, edit_param[5], 1.0)
        else:
            assert edit_param[6] == edit_param[7], "uniform scale only"
            scale = edit_param[6]
            matrix = np.array([[scale, 0, (1 - scale) * center[0]], [0, scale, (1 - scale) * center[1]]])
        rows, cols = np.meshgrid(np.arange(size[0]), np.arange(size[1]), indexing="ij")
        points = np.stack((rows, cols, np.ones_like(rows)), axis=-1).reshape(-1, 3)
        return np.dot(points, matrix.T).reshape(size[0], size[1], 2)
    corr = np.load(path_3D)
    if corr.ndim != 3 or tuple(corr.shape[:2]) != (int(size[0]), int(size[1])) or corr.shape[2] != 2:
        raise ValueError(f"{path_3D}: the correspondence map is {corr.shape[0]} x {corr.shape[1]} (shape {corr.shape}), the source image "
                         f"{size[0]} x {size[1]}: a map describes the image it was made from, pixel by pixel")
    return corr[..., ::-1].copy()


def default_keypoints(mask, max_points=30):
    """The keypoints used when the caller supplies none -- NOT the reference's (cv2 SIFT matches with an ORB fallback, mean_distance.py:28-79): the pixels with
    mask >= 0.5 in row-major order, every s-th of them with s = ceil(count / max_points), i.e. at most max_points points spread over the object.  Deterministic.
    -> int array [n, 2] of (row, col); an empty mask gives no points (the case then contributes nothing, like the reference's `continue`)."""
    pts = np.argwhere(np.asarray(mask) >= 0.5)
    if len(pts) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    step = -(-len(pts) // max_points)
    return pts[::step]


def mean_distance(featurizer, src_img, gen_img, mask, edit_param, prompt, keypoints, path_3D=None, max_points=30, visible=None, **featurizer_kw):
    """One case of mean_distance.py:calculate_md (:119-165) -> the list of distances of its keypoints.  src_img / gen_img: uint8 HWC arrays; mask: HW array in
    [0, 255]; keypoints: [[row, col], ...] on the source image (the first max_points are used).  The generated image and the mask are resized to the source
    size with PIL BILINEAR and the mask divided by 255 (the reference passes shape[:-1] = (H, W) where PIL wants (W, H): the same for the square images of
    GeoBench; here the source size is meant).  featurizer: freefine_amd.dift.HipSDFeaturizer; featurizer_kw (t, up_ft_index, ensemble_size, noise,
    noise_edited, generator) go to its pair().  Per keypoint: the best cosine match of the source feature among the edited image's features, both upsampled
    bilinearly to the image size (ops.dift_match), and its distance to where the edit should have moved the keypoint.  Keypoints whose target is not finite
    (a correspondence map holds NaN where the warp drew nothing) are dropped.  visible (extension, None = the reference's metric): an [H, W] array of the
    source image's size; keypoints on its zero pixels are dropped BEFORE the max_points cut."""
    from PIL import Image
    from . import ops
    src_img = np.asarray(src_img)
    H, W = src_img.shape[:2]
    gen_img = np.array(Image.fromarray(np.asarray(gen_img)).resize((W, H), Image.BILINEAR))
    mask = np.array(Image.fromarray(np.asarray(mask)).resize((W, H), Image.BILINEAR)) / 255.0
    kps = np.asarray(keypoints(src_img, gen_img, mask) if callable(keypoints) else keypoints).reshape(-1, 2).astype(np.int64)
    if visible is not None:
        visible = np.asarray(visible)
        if visible.shape[:2] != (H, W):
            raise ValueError(f"the visibility image is {visible.shape[0]} x {visible.shape[1]}, the source image {H} x {W}")
        kps = kps[visible.reshape(H, W, -1)[kps[:, 0], kps[:, 1], 0] > 0]
    kps = kps[:max_points]
    if len(kps) == 0:
        return []
    t_coords = transform_coordinates(edit_param, (H, W), mask, path_3D)
    kps = kps[np.isfinite(t_coords[kps[:, 0], kps[:, 1]]).all(-1)]
    if len(kps) == 0:
        return []
    rows_s, rows_e, hw = featurizer.pair(src_img, gen_img, prompt, **featurizer_kw)
    rc, _ = ops.dift_match(rows_s, rows_e, hw, (H, W), kps)
    rc = rc.cpu().numpy()
    out = []
    for k, m in zip(kps, rc):
        d = (t_coords[k[0], k[1]] - m.astype(np.float64)).astype(np.float32)      # (tp - max_rc).float().norm()
        out.append(float(np.sqrt(np.sum(d * d, dtype=np.float32))))
    return out


def correspondence_path(gen_path):
    """Where the reference looks for the correspondence file of a generated image (mean_distance.py:121-122): <tree>/<results folder>/<da>/<ins>/<edit>.png ->
    <tree>/correspondence/<da>/<ins>/<edit>.npy (every occurrence of the folder's name is replaced, and "zkl" by "Hszhu", as there).  None for a path with
    fewer than four components.  warp3d.save_correspondence(<tree>, ...) writes that file."""
    parts = str(gen_path).split("/")
    if len(parts) < 4 or not parts[-4]:
        return None
    return str(gen_path).replace("zkl", "Hszhu").replace(parts[-4], "correspondence").replace(".png", ".npy")


def calculate_md(data, image_label, pipe, keypoints=None, reader=None, max_points=30, visible_only=False, **featurizer_kw):
    """mean_distance.py:calculate_md over a GeoBench result tree data[image]["instances"][instance][sample] with ori_img_path / <image_label> / ori_mask_path /
    edit_param / obj_label (the prompt) -> the mean distance over all keypoints of all cases.  pipe: a FreeFinePipeline (its checkpoint is the feature
    extractor: freefine_amd/dift.py states the two deviations from the reference's SDFeaturizer) or a ready HipSDFeaturizer.  keypoints: a callable
    (src_img, gen_img, mask / 255) -> [[row, col], ...] (a freefine_amd.sift.HipSift is one); "sift" -> a HipSift on the pipeline's device, i.e. sift.sift_matches,
    the counterpart of the reference's get_Matches; None -> the sample's own "keypoints" list when it has one, else default_keypoints(mask).  MD values are
    comparable to the reference's only when the reference's keypoints are supplied.  `reader` maps a path to an array (default: PIL).
    visible_only (extension of the reference's metric, default off; values compare with the reference's only when it is off): where the sibling
    `correspondence_visible/....png` of a case's correspondence file exists (warp3d.save_correspondence writes it), keypoints that are not visible in the
    coarse edit -- self-occluded points have no counterpart in the edited image -- are dropped before the max_points cut."""
    import os
    from .dift import HipSDFeaturizer
    if reader is None:
        from PIL import Image
        reader = lambda p: np.array(Image.open(p))
    feat = pipe if isinstance(pipe, HipSDFeaturizer) else HipSDFeaturizer(pipe)
    if isinstance(keypoints, str):
        if keypoints != "sift":
            raise ValueError(f"calculate_md: keypoints={keypoints!r}; the named detectors are 'sift'")
        from .sift import HipSift
        keypoints = HipSift(getattr(feat.pipe, "device", None))
    dists = []
    for image in data.values():
        for instance in image["instances"].values():
            for sample in instance.values():
                gen_path = sample[image_label]
                path_3D = correspondence_path(gen_path)          # the correspondence file of a 3-D edit, where the reference looks for it
                kp = keypoints
                if kp is None:
                    kp = sample["keypoints"] if "keypoints" in sample else (lambda s, g, m: default_keypoints(m, max_points))
                visible = None
                if visible_only and path_3D is not None:
                    q = path_3D.split("/")
                    vis_path = "/".join(q[:-4] + ["correspondence_visible"] + q[-3:])[:-len(".npy")] + ".png"
                    visible = reader(vis_path) if os.path.exists(vis_path) else None
                dists += mean_distance(feat, reader(sample["ori_img_path"]), reader(gen_path), reader(sample["ori_mask_path"]), sample["edit_param"],
                                       sample["obj_label"], kp, path_3D, max_points, visible=visible, **featurizer_kw)
    return float(np.mean(np.asarray(dists, dtype=np.float32))) if dists else float("nan")
