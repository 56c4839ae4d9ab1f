"""FreeFinePipeline on the MI355X engine: same class name, method names, keyword arguments and return conventions as the
reference pipeline (/root/reference/src/demo/model.py:103-1804), so the GeoBench drivers' and notebooks' call pattern
(`FreeFinePipeline.from_pretrained(...).to(device)`, `model.scheduler = DDIMScheduler.from_config(...)`,
`register_attention_control(model, controller)`, `model.modify_unet_forward()`, `model.FreeFine_generation(...)`)
works unchanged -- but every tensor op of the hot path runs in libfreefine_hip.so (freefine_amd/unet.py, vae.py, ops.py).

Host-side logic that stays Python (like the reference): loop control, the scalar DDIM coefficients (computed with the
same fp32 torch scalar arithmetic as the reference), mask preparation on uint8 tensors (incl. its wrap-around,
SURVEY 0.7) and the controller wiring.  Noise for the masked DDPM step is drawn from torch's GLOBAL CPU generator in
the reference's order (model.py:185-188 with generator=None; exactly n draws after seed_everything), so trajectories are
comparable with the CPU oracle on identical seeds; set `noise_device="cuda"` to draw on the GPU instead.
"""
import os
import random
import sys
from collections import namedtuple
from contextlib import contextmanager
from copy import deepcopy

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .attention import Attention_Modulator
from .config import UNetConfig, VAEConfig
from .scheduler import DDIMScheduler
from .text import ByteTokenizer, NativeTextSpec, SyntheticTextEncoder
from .unet import HipUNet
from .vae import HipVAE
from .weights import load_safetensors_dir, normalize_state_dict, synthetic_state, unet_param_shapes, vae_param_shapes, validate_state_dict


def seed_everything(seed):
    """pytorch_lightning.seed_everything as used at model.py:1018."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    return seed


def _dilate(mask, k):
    from scipy import ndimage
    return ndimage.maximum_filter(mask.astype(np.uint8), size=(k, k), mode="constant", cval=0)  # == cv2.dilate(ones(k,k))


def images_to_u8(images):
    """[K,3,H,W] float images in [0,1] on the device -> K uint8 HWC numpy arrays.  The reference's `(x.permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)`
    (/root/reference/src/demo/model.py:1046-1049) with the fp32 multiply and the truncating cast done on the device: identical bytes, one contiguous
    768 KB-per-image copy to the host instead of K permuted 3 MB ones."""
    u8 = (images.detach().float().permute(0, 2, 3, 1) * 255).to(torch.uint8).contiguous().cpu().numpy()
    return [u8[k] for k in range(u8.shape[0])]


# How the three guided-sampling tasks lay out the one loop (FreeFinePipeline._guided_loop).  An image owns n latent rows: row 0 is the stream
# being sampled, rows 1.. are its references.
#   pair        n = 2; the CFG batch is the pair twice, de-duplicated by _cfg_row_map; cfg_masked / ctrl_step get both rows (ctrl_step masks only
#               row 0).  Otherwise n = 1 + R, the UNet batch is rows [0 .. R, 0] against every text row and only row 0 is stepped.
#   ref_next    loop step j takes rows 1.. of refer[j + 1]; otherwise the whole refer[j] (an inversion of one row per image)
#   replay      how the reference rows re-enter from the inversion's record: "join" (reference-stream replay), "kv" (stored K / V) or None
#   record_all  a trajectory entry is all n rows, aliasing the live latents; otherwise row 0
GuidedLayout = namedtuple("GuidedLayout", "pair ref_next replay record_all")
EDIT = GuidedLayout(pair=True, ref_next=True, replay="join", record_all=True)
BACKGROUND = GuidedLayout(pair=True, ref_next=False, replay=None, record_all=False)
COMPOSE = GuidedLayout(pair=False, ref_next=True, replay="kv", record_all=False)


class FreeFinePipeline:
    _progress_bar_config = {}
    _warned_ref_cache = False

    def __init__(self, unet, vae, tokenizer, text_encoder, scheduler, device="cuda:0"):
        self.unet, self.vae, self.tokenizer, self.text_encoder, self.scheduler = unet, vae, tokenizer, text_encoder, scheduler
        self.device = torch.device(device)
        self.controller = None
        self.method_type = None
        self.noise_device = "cpu"
        self._gen = None
        self._mask_dev = {}
        self._batch_ctrls = {}
        self.text_cache, self.text_cache_max, self._text_cache, self._text_on_device, self.text_encoder_calls = True, 256, {}, False, 0
        self.dedup_rows = True      # exact: identical (latent, text) rows of the CFG batch are evaluated once
        # exact: the guided loop's reference row re-enters the UNet from the state the inversion pass recorded for the same (latent,
        # timestep, "") triple instead of being recomputed from conv_in (HipUNet.forward, `reuse`); off = recompute like the reference
        # Memory: the record holds the join-point state of every inversion step (about 0.7 GB per image in bf16, 1.4 GB in fp32 storage, at 64x64
        # and 50 steps) until the guided loop consumes it; `ref_cache_max_bytes` (FFN_REF_CACHE_GB, default 64 GiB per pipeline) bounds it --
        # above the bound the reference rows are recomputed -- and free_ref_cache() drops a record no guided loop will consume.
        self.reuse_ref_stream = True
        self.ref_cache_max_bytes = int(float(os.environ.get("FFN_REF_CACHE_GB", "64")) * 2**30)
        self.drop_ref_tail = True    # with reuse: reference rows stop after the last K / V projection at every step but the last (their eps is dead)
        self._ref_cache = None

    # ------------------------------------------------------------------------------------------------------------
    # construction (freefine_batch_infer_2d.py:148-157)
    # ------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path, torch_dtype=torch.float32, device="cuda:0", seed=0, broadcast=False, x3=False, fp8_conv=False, native_text=False, **kw):
        """`path` is either a HF-layout Stable-Diffusion folder (unet/, vae/ safetensors + config.json; tokenizer/,
        text_encoder/ loaded through transformers when present) or "synthetic:<unet preset>[:<vae preset>]" for
        seeded random weights of that architecture (no checkpoints exist in the build environment).
        torch_dtype float32 -> exact-fp32 parity mode; float16/bfloat16 -> bf16 MFMA fast mode; float32 with x3=True -> the
        split-bf16 mode (fp32 activations, every UNet GEMM on three bf16 MFMAs per product term: fp32-level results at several
        times the fp32-MFMA rate; the VAE bracket runs in the same mode).
        `broadcast` (OPT-IN; the GeoBench drivers pass broadcast="auto"): construction becomes a COLLECTIVE -- only rank 0 reads /
        generates the UNet and VAE weights, every other rank of the default process group receives them over RCCL straight into device
        memory (freefine_amd.dist.broadcast_state; bf16 payload for the matrices in fast mode), so ALL ranks must call it with the same
        arguments ("auto": only when a process group with more than one rank is initialised).  The default (False) is the reference's
        behaviour: every caller reads the checkpoint itself (freefine_batch_infer_2d.py:149), safe on a subset of ranks.
        `native_text` (checkpoint folders only; default False = transformers' CLIPTextModel as before): the text tower runs on the project's own kernels
        (freefine_amd.text.HipCLIPTextEncoder, read from text_encoder/ without a transformers model class) in the pipeline's mode -- fp32, split-bf16 or bf16;
        the tokenizer stays CLIPTokenizer.  Its embeddings are bit-identical per prompt whatever is encoded beside it, so `_encode_text` hands it all
        missing prompts in one call."""
        ucfg, ust, vcfg, vst, tok, enc, sched, dtype = cls.components(path, torch_dtype, device, seed, broadcast, native_text=native_text)
        if isinstance(enc, NativeTextSpec):
            enc = enc.build(dtype=dtype, device=device, x3=x3)
        return cls.from_state(ucfg, ust, vcfg, vst, tok, enc, sched, dtype, device, x3=x3, fp8_conv=fp8_conv)

    @classmethod
    def components(cls, path, torch_dtype=torch.float32, device="cuda:0", seed=0, broadcast=False, native_text=False):
        """what `from_pretrained` hands to `from_state`: configs, host (or, after a broadcast, device-resident) parameter states, tokenizer, text
        encoder, scheduler, storage dtype -- without building the executors, so the whole loading / broadcasting path runs without a GPU."""
        from . import dist as FD
        dtype = torch.float32 if torch_dtype == torch.float32 else torch.bfloat16
        shared = FD.active() if broadcast == "auto" else bool(broadcast)
        lead = (not shared) or torch.distributed.get_rank() == 0
        ust = vst = None
        if path.startswith("synthetic:"):
            parts = path.split(":")
            ucfg = UNetConfig.preset(parts[1])
            vcfg = VAEConfig.preset(parts[2] if len(parts) > 2 else ("tiny" if parts[1].startswith("tiny") else "sd"))
            if lead:
                ust = synthetic_state(unet_param_shapes(ucfg), seed)
                vst = synthetic_state(vae_param_shapes(vcfg), seed + 1)
            if native_text:
                raise ValueError("native_text needs a checkpoint folder with text_encoder/ (synthetic: pipelines use the byte-level stand-in encoder)")
            tok, enc = ByteTokenizer(), SyntheticTextEncoder(ucfg.cross_attention_dim)
            sched = DDIMScheduler()
        else:
            ucfg, ust, vcfg, vst, tok, enc, sched = cls.load_folder(path, shared=shared, lead=lead, native_text=native_text)
        if shared:
            if lead:        # the shape tables are defined on normalised names: rename legacy VAE keys before the names travel
                ust, vst = normalize_state_dict(ust), normalize_state_dict(vst)
                validate_state_dict(ust, unet_param_shapes(ucfg), "unet")
                validate_state_dict(vst, vae_param_shapes(vcfg), "vae")
            mdt = torch.float32 if dtype == torch.float32 else torch.bfloat16
            ust = FD.broadcast_state(ust, unet_param_shapes(ucfg), device, matrix_dtype=mdt)
            vst = FD.broadcast_state(vst, vae_param_shapes(vcfg), device, matrix_dtype=mdt)
        return ucfg, ust, vcfg, vst, tok, enc, sched, dtype

    @staticmethod
    def read_scheduler_config(path):
        """scheduler/scheduler_config.json of a HF-layout SD folder -> DDIMScheduler kwargs, the way `DDIMScheduler.from_config(model.scheduler.config)`
        consumes SD's PNDM config (/root/reference/evaluation/FreeFine/freefine_batch_infer_2d.py:151, src/demo/model.py:123-127, 384).  The hot path's
        scheduler arithmetic HARD-CODES what these constants mean (epsilon prediction in inv_step / ctrl_step, "leading" timestep spacing with the
        offset, alpha_bar_0 as the final alpha), so nothing is defaulted silently: a missing file or key, a v-prediction checkpoint (SD-2.1 768-v),
        trained betas or another spacing raise here instead of producing a wrong trajectory."""
        import json
        sp = os.path.join(path, "scheduler", "scheduler_config.json")
        if not os.path.exists(sp):
            raise FileNotFoundError(f"{sp} not found: the DDIM constants (betas, steps_offset, set_alpha_to_one, prediction_type) are read from the "
                                    "checkpoint, never assumed")
        with open(sp) as f:
            cfg = json.load(f)
        need = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "steps_offset", "set_alpha_to_one")
        missing = [k for k in need if k not in cfg]
        if missing:
            raise ValueError(f"{sp}: missing {missing}")
        if cfg.get("prediction_type", "epsilon") != "epsilon":
            raise ValueError(f"{sp}: prediction_type={cfg['prediction_type']!r}; FreeFine's inv_step / ctrl_step assume epsilon prediction "
                             "(stable-diffusion-2-1-base, not the 768-v model)")
        if cfg.get("trained_betas") is not None:
            raise ValueError(f"{sp}: trained_betas is set; only the scaled_linear / linear schedules are implemented")
        if cfg["beta_schedule"] not in ("scaled_linear", "linear"):
            raise ValueError(f"{sp}: beta_schedule={cfg['beta_schedule']!r} not implemented")
        if cfg.get("timestep_spacing", "leading") != "leading":
            raise ValueError(f"{sp}: timestep_spacing={cfg['timestep_spacing']!r}; the reference's loops run on leading spacing")
        out = {k: cfg[k] for k in need}
        out["prediction_type"] = "epsilon"
        return out

    @classmethod
    def load_folder(cls, path, shared=False, lead=True, native_text=False):
        """Everything `from_pretrained` reads from a HF-layout Stable-Diffusion folder, on the host: (UNetConfig, unet state, VAEConfig, vae state,
        tokenizer, text encoder, DDIMScheduler).  States are fp32 (fp16 / bf16 shards are up-cast), under current diffusers parameter names (the hub's
        legacy VAE attention names are renamed); with `shared` only the lead rank reads the tensors (the others get None) and the configs travel by
        broadcast_object.  Split out so that the loading path is testable without a GPU (tests/test_checkpoint_cpu.py)."""
        from . import dist as FD
        ucd = vcd = sc = ust = vst = None
        if lead:
            ucd, ust = load_safetensors_dir(path, "unet")
            vcd, vst = load_safetensors_dir(path, "vae")
            sc = cls.read_scheduler_config(path)
        if shared:
            ucd, vcd, sc = FD.broadcast_object((ucd, vcd, sc))
        ucfg = UNetConfig.from_diffusers(ucd)
        vcfg = VAEConfig(block_out_channels=tuple(vcd["block_out_channels"]), layers_per_block=vcd["layers_per_block"],
                         latent_channels=vcd["latent_channels"], norm_num_groups=vcd.get("norm_num_groups", 32),
                         scaling_factor=vcd.get("scaling_factor", 0.18215))
        if abs(vcfg.scaling_factor - 0.18215) > 1e-12:
            raise ValueError(f"vae scaling_factor {vcfg.scaling_factor}: the reference multiplies latents by the literal 0.18215 (src/demo/model.py:267-272)")
        sched = DDIMScheduler(**sc)
        from transformers import CLIPTextModel, CLIPTokenizer
        tok = CLIPTokenizer.from_pretrained(os.path.join(path, "tokenizer"))
        # native_text: the checked config + host state of the tower on the project's kernels (from_pretrained builds the executor in its mode)
        enc = NativeTextSpec(path) if native_text else CLIPTextModel.from_pretrained(os.path.join(path, "text_encoder")).eval()
        if enc.config.hidden_size != ucfg.cross_attention_dim:
            raise ValueError(f"text encoder width {enc.config.hidden_size} != unet cross_attention_dim {ucfg.cross_attention_dim}")
        return ucfg, ust, vcfg, vst, tok, enc, sched

    @classmethod
    def from_state(cls, ucfg, ustate, vcfg, vstate, tokenizer, text_encoder, scheduler=None, dtype=torch.float32, device="cuda:0", x3=False,
                   fp8_conv=False):
        ustate, vstate = normalize_state_dict(ustate), normalize_state_dict(vstate)      # hub checkpoints: legacy VAE attention names
        validate_state_dict(ustate, unet_param_shapes(ucfg), "unet")
        validate_state_dict(vstate, vae_param_shapes(vcfg), "vae")
        unet = HipUNet(ucfg, ustate, dtype=dtype, device=device, x3=x3, fp8_conv=fp8_conv)
        vae = HipVAE(vcfg, vstate, dtype=dtype, device=device, x3=x3)
        return cls(unet, vae, tokenizer, text_encoder, scheduler or DDIMScheduler(), device)

    def to(self, device=None, *a, **k):
        return self

    def share(self):
        """a sibling pipeline over the same weights (see HipUNet.share) for running independent edits concurrently on
        separate HIP streams; give it its own controller with register_attention_control*."""
        other = FreeFinePipeline(self.unet.share(), self.vae, self.tokenizer, self.text_encoder,
                                 DDIMScheduler.from_config(self.scheduler.config), self.device)
        other.noise_device, other.dedup_rows, other.reuse_ref_stream, other.drop_ref_tail = self.noise_device, self.dedup_rows, self.reuse_ref_stream, self.drop_ref_tail
        other.text_cache, other._text_on_device = self.text_cache, self._text_on_device
        return other

    def _seed(self, seed):
        """seed_everything(seed) (model.py:1018) + a pipeline-local CPU generator seeded identically: the DDPM noise is drawn
        from the local generator (same mt19937 stream as the global one would give), so concurrent pipelines do not interleave."""
        seed_everything(seed)
        self._gen = torch.Generator().manual_seed(seed)

    def enable_attention_slicing(self, *a, **k):     # accepted and ignored: the fused kernels never materialise scores
        pass

    def enable_xformers_memory_efficient_attention(self, *a, **k):
        pass

    def modify_unet_forward(self):                   # the executor already returns a bare tensor (attention.py:214-223)
        pass

    # ------------------------------------------------------------------------------------------------------------
    # scheduler steps
    # ------------------------------------------------------------------------------------------------------------
    def inv_step(self, model_output, timestep, x, eta=0., verbose=False):
        """model.py:109-132"""
        next_step = int(timestep)
        t = min(next_step - self.scheduler.config.num_train_timesteps // self.scheduler.num_inference_steps, 999)
        a_t = self.scheduler.alphas_cumprod[t] if t >= 0 else self.scheduler.final_alpha_cumprod
        a_next = self.scheduler.alphas_cumprod[next_step]
        c_bt, c_at = ((1 - a_t) ** 0.5).item(), (a_t ** 0.5).item()
        c_an, c_bn = (a_next ** 0.5).item(), ((1 - a_next) ** 0.5).item()
        return ops.ddim_inv_step(model_output.contiguous(), x.contiguous(), c_bt, c_at, c_an, c_bn, want_pred_x0=True)

    def _get_variance(self, timestep, prev_timestep):
        a_t = self.scheduler.alphas_cumprod[timestep]
        a_prev = self.scheduler.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.scheduler.final_alpha_cumprod
        return ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)

    def ctrl_step(self, model_output, timestep, x, mask, eta=0.0, generator=None, noise=None):
        """model.py:134-198.  `mask` is the [h,w] tensor in its pipeline dtype (uint8): (1 - mask) is evaluated in that dtype."""
        t = int(timestep)
        prev_t = t - self.scheduler.config.num_train_timesteps // self.scheduler.num_inference_steps
        a_t = self.scheduler.alphas_cumprod[t]
        a_prev = self.scheduler.alphas_cumprod[prev_t] if prev_t > 0 else self.scheduler.final_alpha_cumprod
        std = eta * self._get_variance(t, prev_t).to(torch.float32) ** 0.5
        rows = model_output.shape[0]
        if rows == 2:
            stds, masked = [std, torch.zeros_like(std)], [1, 0]
        else:
            stds, masked = [std] * rows, [1] * rows
        if mask is None:
            masked = [0] * rows
            mask = torch.ones(x.shape[-2:], dtype=torch.float32)
        mkey = (mask.data_ptr(), mask._version, tuple(mask.shape), mask.dtype)
        ent = self._mask_dev.get(mkey)
        if ent is None or ent[0] is not mask:
            if len(self._mask_dev) >= 32:
                self._mask_dev.clear()
            m_host = mask.detach().cpu()                # (1 - mask) in the mask's own dtype: uint8 wrap-around preserved
            ent = self._mask_dev[mkey] = (mask, m_host.float().reshape(-1).to(self.device), (1 - m_host).float().reshape(-1).to(self.device))
        m_f, om_f = ent[1], ent[2]
        c_dirm = [((1 - a_prev - s ** 2) ** 0.5).item() for s in stds]
        if generator is None:
            generator = self._gen if self.noise_device == "cpu" else None
        if eta > 0 and noise is None:
            if self.noise_device == "cpu":
                noise = torch.randn(model_output.shape, generator=generator, dtype=torch.float32).to(self.device)
            else:
                noise = torch.randn(model_output.shape, generator=generator, device=self.device, dtype=torch.float32)
        return ops.ddim_ctrl_step(model_output.contiguous(), x.contiguous(), noise if eta > 0 else None, m_f, om_f,
                                  ((1 - a_t) ** 0.5).item(), (a_t ** 0.5).item(), (a_prev ** 0.5).item(), ((1 - a_prev) ** 0.5).item(),
                                  c_dirm, [s.item() for s in stds], masked, want_pred_x0=True)

    def _predraw_noise(self, n, shape, eta):
        """the n randn draws of the loop (model.py:185-188), in order, from the same generator, uploaded ONCE: nothing else
        consumes the generator inside the loop, so the values are identical to drawing one per step."""
        if eta <= 0 or n <= 0:
            return None
        if self.noise_device != "cpu":
            return torch.randn((n,) + tuple(shape), device=self.device, dtype=torch.float32)
        return torch.stack([torch.randn(tuple(shape), generator=self._gen, dtype=torch.float32) for _ in range(n)]).to(self.device)

    def linear_param(self, t, t1, t0, t2, end_scale=0.5):
        """model.py:438-455"""
        if t < t1 or t > t2:
            raise ValueError(f"t must be in [{t1}, {t2}]")
        if t <= t0:
            return 1 + (end_scale - 1) / (t0 - t1) * (t - t1)
        return end_scale + (-end_scale / (t2 - t0)) * (t - t0)

    # ------------------------------------------------------------------------------------------------------------
    # VAE bracket / text
    # ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def image2latent(self, image):
        """model.py:223-268: uint8 HWC ndarray / float NCHW tensor in [-1,1] -> latent mean * 0.18215"""
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(image)
        if image.dtype == torch.uint8:                  # HWC / NHWC bytes: x/127.5-1 happens in the VAE's first kernel
            return self.vae.encode_mean_scaled(img_u8=image[None] if image.ndim == 3 else image)
        if image.ndim == 3:
            image = image.permute(2, 0, 1).unsqueeze(0)
        return self.vae.encode_mean_scaled(x_nchw=image)

    @torch.no_grad()
    def latent2image(self, latents, return_type="np"):
        image = self.vae.decode_image(latents.detach())
        if return_type == "np":
            return images_to_u8(image[:1])[0]
        return image

    @torch.no_grad()
    def _encode_text(self, prompts):
        """tokenizer + text encoder (model.py:536-567, 842-848).  A torch text encoder (transformers CLIPTextModel) is moved to the
        pipeline's device on first use and fed device-side ids -- the reference's `.to(device)` does the same; from_pretrained used to leave it
        on the host.  `text_cache` (default on): embeddings are kept per prompt string (an edit asks for "" five times and the GeoBench
        drivers repeat object labels), at most `text_cache_max` entries, LRU; `text_cache = False` encodes every request."""
        if isinstance(prompts, str):
            prompts = [prompts]
        prompts = list(prompts)
        cache = self._text_cache if self.text_cache else None
        missing = [q for q in dict.fromkeys(prompts) if cache is None or q not in cache]
        # the hits are READ here and moved behind the misses only in the final update (an eviction made room for this call's misses must not
        # remove a prompt of this very call that was counted as a hit; and an encoder failure below leaves the cache as it was)
        hits = [q for q in dict.fromkeys(prompts) if cache is not None and q in cache]
        fresh = {q: cache[q] for q in hits}
        if missing:
            enc = self.text_encoder
            if isinstance(enc, torch.nn.Module) and not self._text_on_device:
                enc.to(self.device)
                self._text_on_device = True
            ids = self.tokenizer(missing, padding="max_length", max_length=77, return_tensors="pt").input_ids
            if isinstance(enc, torch.nn.Module):
                # a torch encoder runs every distinct prompt ON ITS OWN: a library GEMM may pick another kernel / summation order for another
                # batch size, and the exact reductions downstream (reference-stream reuse, CFG row de-duplication) compare embeddings bit for
                # bit -- the "" of the inversion call must equal the "" of the guided call whatever else was asked for beside it
                ids = ids.to(self.device)
                out = torch.cat([enc(ids[j:j + 1])[0] for j in range(len(missing))]).to(self.device, torch.float32)
                self.text_encoder_calls += len(missing)
            else:
                out = enc(ids)[0].to(self.device, torch.float32)
                self.text_encoder_calls += 1
            for j, q in enumerate(missing):
                fresh[q] = out[j]
        if cache is not None:
            for q in hits:
                cache.pop(q)
            for q in missing + hits:                            # most recently used last
                cache[q] = fresh[q]
            while len(cache) > self.text_cache_max:
                cache.pop(next(iter(cache)))
        return torch.stack([fresh[q] for q in prompts]).contiguous()

    @torch.no_grad()
    def get_text_embeddings(self, prompt):
        return self._encode_text(prompt)

    def preprocess_image(self, image, device=None):
        return (torch.from_numpy(image).float() / 127.5 - 1).permute(2, 0, 1).unsqueeze(0).to(self.device)

    @staticmethod
    def _work_size(img):
        """[W, H] bound the other images of an edit are thumbnailed to.  The reference hard-codes 512 x 512 (model.py:1347, :1369);
        here the bound follows the coarse input when that is larger (768 x 768 edits, BASELINE.json configs[4]) and is the
        reference's 512 otherwise, so every call the reference can make behaves as it does there."""
        return [max(512, img.shape[1]), max(512, img.shape[0])]

    def resize_img(self, img, size=None):
        """model.py:1332-1340: PIL thumbnail (never upscales); a no-op for the <=512 inputs of the drivers."""
        if max(img.shape[:2]) <= max(size):
            return img
        from PIL import Image
        im = Image.fromarray(img)
        im.thumbnail(size, Image.Resampling.LANCZOS)
        return np.array(im)

    # ------------------------------------------------------------------------------------------------------------
    # loops
    # ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _min_tca_block(self):
        """first transformer block whose self-attention the registered controller(s) may modulate (None: none)"""
        cs = self.unet._ctrls() or ([self.controller] if self.controller is not None else [])
        idx = [min(c.layer_idx) for c in cs if getattr(c, "layer_idx", None)]
        return min(idx) if idx else None

    def invert(self, image, prompt, num_inference_steps=50, num_actual_inference_steps=None, guidance_scale=7.5, eta=0.0,
               return_intermediates=False, verbose=False, record_rows=None, record_kv=False, **kwds):
        """model.py:816-925 (HOT LOOP 1).  record_rows (reference-stream reuse): batch rows whose state at the UNet's join point
        is recorded at every step for the guided loop that follows (self._ref_cache); record_kv: record their self-attention K / V
        from the first modulated block on instead (hooks that leave the reference rows unmodulated: composition)."""
        batch_size = image.shape[0]
        if isinstance(prompt, list):
            if batch_size == 1:
                image = image.expand(len(prompt), -1, -1, -1)
        elif isinstance(prompt, str) and batch_size > 1:
            prompt = [prompt] * batch_size
        text = self._encode_text(prompt)
        latents = self.image2latent(image)
        if guidance_scale > 1.:
            text = torch.cat([self._encode_text([""] * batch_size), text], dim=0)
            self.controller.use_cfg = True
        self.scheduler.set_timesteps(num_inference_steps)
        latents_list = [latents]
        cache = None
        self._ref_cache = None
        if record_rows and self.reuse_ref_stream and not guidance_scale > 1. and hasattr(self.unet, "join_block"):
            cache = dict(rows=list(record_rows), slots=[], latents=latents_list, text=text[list(record_rows)].clone(),
                         idx=torch.tensor(list(record_rows), device=self.device))
            if record_kv:
                mt = self._min_tca_block()
                cache["kv_from"] = len(self.unet.transformers) if mt is None else int(mt)
            else:
                cache["join"] = self.unet.join_block(self._min_tca_block())[0]
        for i, t in enumerate(reversed(self.scheduler.timesteps)):
            if num_actual_inference_steps is not None and i >= num_actual_inference_steps:
                continue
            model_inputs = torch.cat([latents] * 2) if guidance_scale > 1. else latents
            if cache is not None and "kv_from" in cache:
                noise_pred = self.unet(model_inputs, t, encoder_hidden_states=text, reuse=dict(mode="record", kv_from=cache["kv_from"]))
                cache["slots"].append([(k.index_select(0, cache["idx"]), vt.index_select(0, cache["idx"])) for k, vt in self.unet.last_kv])
            elif cache is not None:
                noise_pred = self.unet(model_inputs, t, encoder_hidden_states=text, reuse=dict(mode="record", join=cache["join"]))
                cache["slots"].append([s.index_select(0, cache["idx"]) for s in self.unet.last_boundary])
            else:
                noise_pred = self.unet(model_inputs, t, encoder_hidden_states=text)
            if cache is not None and len(cache["slots"]) == 1:
                # size guard (the record is 13.8 MB per image and step in bf16 at 64x64, twice that in fp32 storage, x 2.25 at 768^2): if the
                # whole schedule would not fit the budget, stop recording -- the guided loop then recomputes the reference rows like the reference
                first = cache["slots"][0]
                per_step = sum(t_.numel() * t_.element_size() for s_ in first for t_ in (s_ if isinstance(s_, (tuple, list)) else (s_,)))
                n_rec = num_actual_inference_steps if num_actual_inference_steps is not None else len(self.scheduler.timesteps)
                if per_step * n_rec > self.ref_cache_max_bytes:
                    if not FreeFinePipeline._warned_ref_cache:
                        FreeFinePipeline._warned_ref_cache = True
                        print(f"[freefine_amd] reference-stream record of {per_step * n_rec / 2**30:.1f} GiB exceeds ref_cache_max_bytes "
                              f"({self.ref_cache_max_bytes / 2**30:.1f} GiB): recomputing the reference rows instead", file=sys.stderr, flush=True)
                    cache = None
            if guidance_scale > 1.:
                eu, ec = noise_pred.chunk(2, dim=0)
                noise_pred = ops.cfg_masked(eu.contiguous(), ec.contiguous(), None, guidance_scale)
            latents, _ = self.inv_step(noise_pred, t, latents)
            latents_list.append(latents)
        self._ref_cache = cache
        if return_intermediates:
            return latents, latents_list
        return latents

    def free_ref_cache(self):
        """drop the reference-stream record of the last inversion (for callers that invert without running a guided loop afterwards)"""
        self._ref_cache = None

    def _take_ref_cache(self, refer_latents, n_act, text, ref_text_rows, kv=False):
        """the recorded reference stream of the inversion that produced `refer_latents` (checked by identity: guided step k reads
        refer_latents[k + 1] = the input of inversion step n - k - 1, model.py:582 vs :883), or None where reuse does not apply:
        switched off, another inversion, style-align methods (they modulate every block), a modulated block before the join point,
        or reference rows whose prompt is not the inversion's."""
        cache, self._ref_cache = self._ref_cache, None
        if cache is None or not self.reuse_ref_stream or len(cache["slots"]) != n_act or len(refer_latents) != n_act + 1:
            return None
        if kv != ("kv_from" in cache):                        # (kv: the stored-K/V record of a hook whose reference rows stay unmodulated)
            return None
        if any(refer_latents[k + 1] is not cache["latents"][n_act - k - 1] for k in range(n_act)):
            return None
        for c in (self.unet._ctrls() or []):
            if c.use_style_align:
                return None
        mt = self._min_tca_block()
        if mt is not None and mt < (cache["kv_from"] if kv else self.unet.join_block_tb(cache["join"])):
            return None
        if any(not torch.equal(text[r], cache["text"][i % cache["text"].shape[0]]) for i, r in enumerate(ref_text_rows)):
            return None
        return cache

    def _cfg_row_map(self, text, n):
        """CFG batch rows are (latent i mod n, text row i).  Rows whose text embeddings coincide are the same UNet input, bit
        for bit (edit / bg-gen: the reference stream with prompt "" appears twice; with an empty edit prompt so does the edit
        stream) -> evaluate each distinct row once.  Returns (row_map or None, physical latent rows, physical text rows)."""
        if not self.dedup_rows:
            return None, None, None
        row_map, phys = [], []
        for i in range(2 * n):
            hit = next((j for j, (li, ti) in enumerate(phys) if li == i % n and torch.equal(text[ti], text[i])), None)
            if hit is None:
                phys.append((i % n, i))
                hit = len(phys) - 1
            row_map.append(hit)
        if len(phys) == 2 * n:
            return None, None, None
        return row_map, [li for li, _ in phys], [ti for _, ti in phys]

    @staticmethod
    def _merge_row_maps(maps):
        """the `_cfg_row_map` results of K images -> the one (row_map, latent rows, text rows) of the image-major batch: theirs where they
        all agree, else (images disagree on which CFG rows coincide, or de-duplication is off) all four rows"""
        if all(m[0] is not None and m[0] == maps[0][0] for m in maps):
            return maps[0]
        return None, [0, 1, 0, 1], [0, 1, 2, 3]

    def _guided_rows(self, lay, texts, n):
        """what a guided step feeds to the UNet for the K = len(texts) images of n latent rows each: (row_map, the latent rows of the whole
        batch, image-major, and per image: the text rows, which of its latent rows are reference rows, the text rows those run against)"""
        if lay.pair:
            row_map, lat_rows, txt_rows = self._merge_row_maps([self._cfg_row_map(t, 2) for t in texts])
        else:                                                 # [edit_u, ref_1 .. ref_R, edit_c] against every text row
            row_map, lat_rows, txt_rows = None, list(range(n)) + [0], list(range(texts[0].shape[0]))
        ref_flags = tuple(r > 0 for r in lat_rows)
        return row_map, [n * k + r for k in range(len(texts)) for r in lat_rows], txt_rows, ref_flags, [txt_rows[p] for p, f in enumerate(ref_flags) if f]

    def _reuse_arg(self, lay, cache, ref_flags, n_txt, num_steps, i):
        """HipUNet.forward's `reuse` argument of scheduler step i = start_step + j, the loop's step j (None without a record): the reference
        rows re-enter from what inversion step n_act - j - 1 = num_steps - i - 1 recorded for the same latent, timestep and prompt.
        n_txt: text rows per image"""
        if cache is None:
            return None
        slot = cache["slots"][num_steps - i - 1]
        nr = sum(ref_flags)
        if lay.replay == "kv":
            # text rows per image: [""] * (1 + R) + the prompts; the edit rows read text row 0 and the prompt rows
            return dict(mode="replay_kv", kv_from=cache["kv_from"], ref=ref_flags, kv=slot, text_sel=[0] + list(range(1 + nr, n_txt)))
        # every step but the last overwrites the reference latent before anything reads it: the reference rows' eps is dead there and
        # their tail behind the last K / V projection is not run
        return dict(mode="replay", join=cache["join"], ref=ref_flags, state=[s.repeat_interleave(nr, 0) for s in slot] if nr > 1 else slot,
                    drop_tail=self.drop_ref_tail and i + 1 < num_steps)

    def _step_method(self, ctrls, method_type, i, start_step, end_step, num_steps, end_scale):
        """the method's schedule at scheduler step i (model.py:587-591)"""
        for c in ctrls:
            if method_type == "tca":
                c.context_guidance = self.linear_param(i, start_step, end_step, num_steps, end_scale=end_scale)
            elif method_type == "mmsa_es" and i >= end_step:
                c.use_tca = False

    def _configure_method(self, c, method_type, share_attn, local_edit, prompt_length=None):
        self.method_type = method_type
        c.local_edit = local_edit
        if prompt_length is not None:
            c.prompt_length = prompt_length
        if share_attn:
            if method_type == "tca":
                c.use_tca, c.layer_idx, c.method = True, list(range(10, 16)), "tca"
            elif method_type in ("mmsa", "mmsa_es"):
                c.use_tca, c.layer_idx, c.method = True, list(range(10, 16)), "mmsa"
            elif method_type in ("ssa", "sdsa"):
                c.use_style_align, c.method = True, method_type
        c.use_cfg = True

    def _mask_f(self, mask):
        return mask.detach().cpu().float().reshape(-1).to(self.device)

    @torch.no_grad()
    def _guided_loop(self, lay, ctrls, texts, cfg_f, var_masks, noises, latents, refer, traj, method_type, num_steps, start_step, end_step,
                     end_scale, guidance_scale, eta):
        """HOT LOOP 2 (model.py:301-435, 476-622, 656-812) for K = len(texts) images as one image-major batch, laid out by `lay` (EDIT,
        BACKGROUND or COMPOSE above).  Per image: its controller, its logical text rows, cfg mask vector (or None), variance mask and
        pre-drawn noise stack (or None).  `latents` [K n, 4, h, w] holds every image's n rows and is WRITTEN: its reference rows are
        overwritten in place.  `traj`: None, or K lists holding entry 0 that receive one entry per step.  Returns (final latents, traj)."""
        K, n, shape1 = len(texts), latents.shape[0] // len(texts), tuple(latents.shape[1:])
        m = n if lay.pair else 1                              # rows per image that cfg_masked / ctrl_step see
        row_map, lat_rows, txt_rows, ref_flags, ref_txt = self._guided_rows(lay, texts, n)
        text_phys = torch.cat([t[txt_rows] for t in texts], dim=0).contiguous()
        lat_idx = torch.tensor(lat_rows, device=self.device)
        self.scheduler.set_timesteps(num_steps)
        cache = None
        if lay.replay:
            cache = self._take_ref_cache(refer, num_steps - start_step, texts[0], ref_txt, kv=lay.replay == "kv")
            if cache is not None and any(not torch.equal(t[r], cache["text"][0]) for t in texts for r in ref_txt):
                cache = None
        for i, t in enumerate(self.scheduler.timesteps):
            if i < start_step:
                continue
            j = i - start_step
            lat_v = latents.view(K, n, *shape1)
            # the reference rows of this step (model.py:582-586; removal: the aligned latent, :756)
            lat_v[:, 1:] = refer[j + 1].view(K, n, *shape1)[:, 1:] if lay.ref_next else refer[j].view(K, 1, *shape1)
            self._step_method(ctrls, method_type, i, start_step, end_step, num_steps, end_scale)
            reuse = self._reuse_arg(lay, cache, ref_flags, texts[0].shape[0], num_steps, i)
            eps = self.unet(latents.index_select(0, lat_idx), t, encoder_hidden_states=text_phys, row_map=row_map, reuse=reuse)
            eps = eps.view(K, -1, *shape1)
            outs = []
            for k in range(K):
                e = ops.cfg_masked(eps[k, :m].contiguous(), eps[k, -m:].contiguous(), cfg_f[k], guidance_scale)
                outs.append(self.ctrl_step(e, t, lat_v[k, :m], var_masks[k], eta=eta, noise=None if noises[k] is None else noises[k][j])[0])
                if m < n:
                    outs.append(lat_v[k, m:])
            latents = outs[0] if len(outs) == 1 else torch.cat(outs)
            if traj is not None:
                # like the reference's latents_list (model.py:585-616) an entry of all rows ALIASES the live latents: its reference rows
                # are overwritten in place by the next step
                for k in range(K):
                    traj[k].append(latents[n * k:n * (k + 1)] if lay.record_all else latents[n * k])
        return latents, traj

    def _noise_per_case(self, seeds, n, shape, eta):
        """the loop's noise of every case of a batch, each from its own generator seeded like the single call's, drawn in case order"""
        noises = []
        for sd in seeds:
            self._gen = torch.Generator().manual_seed(sd)
            noises.append(self._predraw_noise(n, shape, eta))
        return noises

    @torch.no_grad()
    def forward_sampling(self, prompt, prompt_embeds=None, refer_latents=None, batch_size=1, end_step=None, height=512, width=512,
                         num_inference_steps=50, num_actual_inference_steps=None, guidance_scale=7.5, latents=None,
                         unconditioning=None, neg_prompt=None, return_intermediates=False, eta=0.0, end_scale=0.5,
                         local_var_reg=None, completion_mask_cfg=None, local_edit_text=True, share_attn=True, method_type=None,
                         verbose=False, local_perturbation=True, **kwds):
        """model.py:476-622 (HOT LOOP 2, edit): `latents` = the pair (edit, reference)"""
        assert guidance_scale > 1.0, "USING THIS MODULE CFG Must > 1.0"
        self._configure_method(self.controller, method_type, share_attn, local_edit_text)
        if prompt_embeds is None:
            if isinstance(prompt, list):
                batch_size = len(prompt)
            elif isinstance(prompt, str) and batch_size > 1:
                prompt = [prompt] * batch_size
            text = self._encode_text(prompt)
        else:
            batch_size, text = prompt_embeds.shape[0], prompt_embeds.to(self.device, torch.float32)
        if latents is None:
            latents = torch.randn((batch_size, self.unet.in_channels, height // 8, width // 8)).to(self.device)
        text = torch.cat([self._encode_text([neg_prompt or ""] * batch_size), text], dim=0).contiguous()
        noises = self._predraw_noise(num_actual_inference_steps, (2,) + tuple(latents.shape[1:]), eta)
        latents, traj = self._guided_loop(
            EDIT, [self.controller], [text], [self._mask_f(completion_mask_cfg) if local_edit_text else None],
            [local_var_reg if local_perturbation else torch.ones_like(local_var_reg)], [noises], latents, refer_latents,
            [[latents]] if return_intermediates else None, method_type, num_inference_steps, num_inference_steps - num_actual_inference_steps,
            end_step, end_scale, guidance_scale, eta)
        image = self.latent2image(latents, return_type="pt")
        return (image, traj[0]) if return_intermediates else (image, None)

    @torch.no_grad()
    def forward_sampling_background_gen(self, prompt, batch_size=1, end_step=None, height=512, width=512, num_inference_steps=50,
                                        num_actual_inference_steps=None, guidance_scale=7.5, latents=None, refer_latents=None,
                                        unconditioning=None, neg_prompt=None, return_intermediates=False, eta=0.0,
                                        local_var_reg=None, local_cfg_reg=None, local_text_edit=True, share_attn=True,
                                        method_type="tca", verbose=False, local_perturbation=True, end_scale=0.5,
                                        latent_blended=True, blend_range=(0, 40), **kwds):
        """model.py:656-812 (removal / background generation): row 0 of `latents` is the generated stream, the loop pairs it with the
        inversion's latent of the step; latent_blended / blend_range accepted but inert (:805-806)"""
        assert guidance_scale > 1.0, "USING THIS MODULE CFG Must > 1.0"
        self._configure_method(self.controller, method_type, share_attn, local_text_edit)
        if isinstance(prompt, list):
            batch_size = len(prompt)
        elif isinstance(prompt, str) and batch_size > 1:
            prompt = [prompt] * batch_size
        text = self._encode_text(prompt)
        if latents is None:
            latents = torch.randn((batch_size, self.unet.in_channels, height // 8, width // 8)).to(self.device)
        text = torch.cat([self._encode_text([neg_prompt or ""] * batch_size), text], dim=0).contiguous()
        noises = self._predraw_noise(num_actual_inference_steps, (2,) + tuple(latents.shape[1:]), eta)
        out, traj = self._guided_loop(
            BACKGROUND, [self.controller], [text], [self._mask_f(local_cfg_reg) if local_text_edit else None],
            [local_var_reg if local_perturbation else torch.ones_like(local_var_reg)], [noises], self._with_ref_rows(latents[:1]), refer_latents,
            [[latents]] if return_intermediates else None, method_type, num_inference_steps, num_inference_steps - num_actual_inference_steps,
            end_step, end_scale, guidance_scale, eta)
        image = self.latent2image(out, return_type="pt")
        return (image, traj[0]) if return_intermediates else (image, None)

    @staticmethod
    def _with_ref_rows(init):
        """[K,4,h,w] initial latents of K removals -> the loop's [2K,4,h,w] rows (generated_i, reference_i); the loop fills the reference rows"""
        return torch.stack([init, torch.zeros_like(init)], dim=1).flatten(0, 1)

    @torch.no_grad()
    def forward_sampling_compose(self, prompt, prompt_embeds=None, refer_latents=None, batch_size=1, end_step=None, height=512,
                                 width=512, num_inference_steps=50, num_actual_inference_steps=None, guidance_scale=7.5,
                                 latents=None, unconditioning=None, neg_prompt=None, return_intermediates=False, eta=0.0,
                                 end_scale=0.5, local_var_reg=None, local_edit_text=True, cfg_masks_tensor=None, share_attn=True,
                                 method_type=None, verbose=False, local_perturbation=True, **kwds):
        """model.py:301-435 (cross-image composition / appearance transfer): `latents` = [edit, ref_1..ref_R], UNet batch [edit, ref_1..ref_R, edit]"""
        assert guidance_scale > 1.0, "USING THIS MODULE CFG Must > 1.0"
        prompt.append("")                                      # the reference mutates the caller's list too (model.py:352)
        self._configure_method(self.controller, method_type, share_attn, local_edit_text, prompt_length=len(prompt))
        text = self._encode_text(prompt)
        if latents is None:
            latents = torch.randn((batch_size, self.unet.in_channels, height // 8, width // 8)).to(self.device)
        text = torch.cat([self._encode_text([neg_prompt or ""] * batch_size), text], dim=0).contiguous()
        noises = self._predraw_noise(num_actual_inference_steps, (1,) + tuple(latents.shape[1:]), eta)
        # stored reference K / V: the R reference rows (latent, timestep, "") are the very rows the inversion evaluated, and this hook never
        # modulates them -- only the two edit rows run; the modulated blocks read the references' K / V from the inversion's record
        out, traj = self._guided_loop(
            COMPOSE, [self.controller], [text], [self._mask_f(cfg_masks_tensor) if local_edit_text else None],
            [local_var_reg if local_perturbation else torch.ones_like(local_var_reg)], [noises], latents, refer_latents,
            [[latents]] if return_intermediates else None, method_type, num_inference_steps, num_inference_steps - num_actual_inference_steps,
            end_step, end_scale, guidance_scale, eta)
        image = self.latent2image(out[:1], return_type="pt")[0]
        return (image, traj[0]) if return_intermediates else (image, None)

    # ------------------------------------------------------------------------------------------------------------
    # masks (model.py:927-934, 1431-1639) -- uint8 tensors on the host, arithmetic exactly as the reference
    # ------------------------------------------------------------------------------------------------------------
    def dilate_mask(self, mask, dilate_factor=15):
        return _dilate(mask, dilate_factor)

    def mask_reduce_dim(self, mask):
        return mask[:, :, 0] if mask.ndim == 3 else mask

    def prepare_tensor_mask(self, mask, sup_res_w, sup_res_h, binary=True):
        if mask.ndim == 3:
            mask = mask[:, :, 0]
        t = F.interpolate(torch.tensor(mask)[None, None], (sup_res_h, sup_res_w), mode="nearest")[0, 0]
        if binary:
            t[t > 0.0] = 1.0
        else:
            t = t.float() / t.max()
        return t

    @staticmethod
    def _nearest(t, hw):
        return F.interpolate(t[None, None], hw, mode="nearest")[0, 0]

    @torch.no_grad()
    def prepare_various_mask(self, shifted_mask, ori_mask, draw_mask, sup_res_w, sup_res_h, init_code, verbose=False,
                             use_auto_draw=False, cons_area=None, reduce_inp_artifacts=False):
        ptm = lambda m: self.prepare_tensor_mask(m, sup_res_w, sup_res_h)
        if not use_auto_draw:
            shifted, ori = ptm(shifted_mask), ptm(ori_mask)
            flexible = ptm(draw_mask) * (1 - shifted)
            fg = flexible + shifted
            fg[fg > 0] = 1.0
            complete = flexible
            if not reduce_inp_artifacts:
                local_var = flexible
            else:
                assert cons_area is not None, "for auto artifact expansion use cons area "
                dil, cons = ptm(self.dilate_mask(ori_mask, 30)), ptm(cons_area)
                local_var = (1 - cons) * (1 - shifted) * dil + flexible
                local_var[local_var > 0] = 1
        else:
            assert cons_area is not None, "for auto draw better use cons area "
            dil_tgt = ptm(self.dilate_mask(shifted_mask, 15))
            shifted, ori, cons = ptm(shifted_mask), ptm(ori_mask), ptm(cons_area)
            fg = shifted
            cons = cons - ori                                   # uint8: wraps where ori & ~cons
            if not reduce_inp_artifacts:
                complete = (1 - cons) * (1 - shifted) * dil_tgt
            else:
                complete = ptm(self.dilate_mask(ori_mask, 30)) + dil_tgt
                complete[complete > 0] = 1
                complete *= (1 - cons) * (1 - shifted)
            local_var = complete
        hw = (init_code.shape[2], init_code.shape[3])
        return fg, shifted, ori, self._nearest(complete, hw), self._nearest(local_var, hw)

    @torch.no_grad()
    def prepare_mask_bggen(self, mask, sup_res_w, sup_res_h, init_code):
        t = self.prepare_tensor_mask(mask, sup_res_w, sup_res_h)
        return t, self._nearest(t, (init_code.shape[2], init_code.shape[3]))

    @torch.no_grad()
    def prepare_composition_masks(self, ori_mask_lists, tgt_mask_lists, sup_res_w, sup_res_h, init_code, dil_completion=False,
                                  dil_factor=15, draw_mask=None, appearance_transfer=False):
        ptm = lambda m: self.prepare_tensor_mask(m, sup_res_w, sup_res_h)
        hw = (init_code.shape[2], init_code.shape[3])
        ori = [ptm(m) for m in ori_mask_lists]
        tgt = []
        lp, fg = torch.zeros_like(ori[0]), torch.zeros_like(ori[0])
        if appearance_transfer:
            for sm in tgt_mask_lists:
                d = ptm(self.dilate_mask(sm, dil_factor))
                tgt.append(d)
                lp += d
            lp[lp > 0] = 1
            tgt.append(1 - lp)
            lp = self._nearest(lp, hw)
            return torch.stack(tgt), torch.stack(ori), lp, deepcopy(lp)
        if draw_mask is None:
            for sm in tgt_mask_lists:
                d, s = ptm(self.dilate_mask(sm, dil_factor)), ptm(sm)
                tgt.append(d if dil_completion else s)
                fg += s
                lp += d
            fg[fg > 0] = 1
            lp[lp > 0] = 1
            tgt.append(1 - fg if dil_completion else 1 - lp)
            lp = self._nearest(lp * (1 - fg), hw)
            return torch.stack(tgt), torch.stack(ori), lp, (deepcopy(lp) if dil_completion else torch.zeros_like(lp))
        for i, sm in enumerate(tgt_mask_lists):
            s = ptm(sm)
            d = ptm(draw_mask[i]) + s
            d[d > 0] = 1
            tgt.append(d)
            fg += s
            lp += d
        fg[fg > 0] = 1
        lp[lp > 0] = 1
        tgt.append(1 - lp)
        lp = self._nearest(lp * (1 - fg), hw)
        return torch.stack(tgt), torch.stack(ori), lp, lp

    # ------------------------------------------------------------------------------------------------------------
    # task-level API (model.py:1012-1118, 1341-1388, 1640-1804)
    # ------------------------------------------------------------------------------------------------------------
    def prepare_controller_ref_mask(self, mask, use_mask_expansion=True):
        if mask.ndim == 3:
            mask = mask[:, :, 0]
        mask = torch.Tensor(mask)
        if use_mask_expansion:
            self.controller.obj_mask = mask
            self.controller.log_mask = True
        return mask

    @torch.no_grad()
    def DDIM_inversion_func(self, img, mask, prompt, num_step, start_step=0, ref_img=None, verbose=False):
        imgs = [img] if ref_img is None else [img, self.resize_img(ref_img, size=self._work_size(img))]
        source = torch.from_numpy(np.stack(imgs))                       # uint8 [N,H,W,3]; /127.5-1 happens in the VAE's first kernel
        mask = self.prepare_controller_ref_mask(mask, False)
        latents, latents_list = self.invert(source, prompt, guidance_scale=1.0, num_inference_steps=num_step,
                                            num_actual_inference_steps=num_step - start_step, return_intermediates=True, verbose=verbose,
                                            record_rows=[1] if ref_img is not None else None)      # row 1 = the original image = the guided loop's reference row
        self.controller.reset()
        return mask.detach().cpu().numpy(), latents_list

    @torch.no_grad()
    def DDIM_inversion_func_compose(self, img, compose_imgs, prompt, num_step, start_step=0, verbose=False):
        imgs = [img] + [self.resize_img(r, size=self._work_size(img)) for r in compose_imgs]
        source = torch.from_numpy(np.stack(imgs))
        # rows 1 .. R = the reference images = the guided loop's reference rows: the composition hook leaves them unmodulated
        # (attention.py:1284-1324), so their self-attention K / V are recorded for the loop (stored reference K / V)
        latents, latents_list = self.invert(source, prompt, guidance_scale=1.0, num_inference_steps=num_step,
                                            num_actual_inference_steps=num_step - start_step, return_intermediates=True, verbose=verbose,
                                            record_rows=list(range(1, len(imgs))), record_kv=True)
        self.controller.reset()
        return latents_list

    # per-case set-up: the masks and the controller state of one image, shared by the single calls and the image-batched ones
    def _setup_edit(self, c, hw, init, shifted_mask, ori_mask, draw_mask, method_type, share_attn, **mask_kw):
        """model.py:1640-1692 -> (completion mask of the CFG, variance mask), both at latent size"""
        fg, shifted_t, ori_t, cfg_m, var_m = self.prepare_various_mask(shifted_mask, ori_mask, draw_mask, hw[0], hw[1], init, **mask_kw)
        cfg_m = self._nearest(cfg_m, (init.shape[2], init.shape[3]))
        c.fg_retain_mask, c.fg_retain_mask_st2, c.fg_ref_mask, c.local_edit_region = fg, shifted_t, ori_t, fg
        c.reset()
        c.log_mask = False
        # NB the caller's `local_text_edit` is forwarded under the wrong keyword by the reference (blending=, model.py:1692), so the loop's
        # local_edit_text stays True whatever the caller passed; kept.
        self._configure_method(c, method_type, share_attn, True)
        return cfg_m, var_m

    def _setup_background(self, c, hw, init, ori_mask, method_type, share_attn, local_text_edit):
        """model.py:1088-1118 -> the hole mask at latent size (CFG and variance mask alike)"""
        mask_t, var_m = self.prepare_mask_bggen(ori_mask, hw[0], hw[1], init)
        c.fg_retain_mask, c.local_edit_region = mask_t, mask_t
        c.reset()
        self._configure_method(c, method_type, share_attn, local_text_edit)
        return var_m

    def _setup_compose(self, c, hw, init, ori_mask_lists, tgt_mask_lists, draw_mask, n_prompts, method_type, share_attn, local_text_edit, **mask_kw):
        """model.py:1051-1086 -> (variance mask, CFG mask) at latent size; the loop's prompt list is the caller's n_prompts plus the empty one"""
        tgt_t, ori_t, lp, cfg_m = self.prepare_composition_masks(ori_mask_lists, tgt_mask_lists, hw[0], hw[1], init, draw_mask=draw_mask, **mask_kw)
        c.src_masks, c.tgt_masks = ori_t, tgt_t
        c.reset()
        self._configure_method(c, method_type, share_attn, local_text_edit, prompt_length=n_prompts + 1)
        return lp, cfg_m

    def Details_Preserving_regeneration(self, source_image, inverted_latents, edit_prompt, shifted_mask, ori_mask, draw_mask,
                                        num_steps=100, start_step=30, end_step=10, eta=1, guidance_scale=7.5, share_attn=True,
                                        method_type="tca", verbose=False, local_text_edit=True, local_perturbation=True,
                                        return_intermediates=False, use_auto_draw=False, cons_area=None, use_share_attention=False,
                                        reduce_inp_artifacts=False, end_scale=0.5):
        init_code = deepcopy(inverted_latents[-1])
        c = self.controller
        cfg_m, var_m = self._setup_edit(c, source_image.shape[:2], init_code, shifted_mask, ori_mask, draw_mask, method_type, share_attn,
                                        use_auto_draw=use_auto_draw, cons_area=cons_area, reduce_inp_artifacts=reduce_inp_artifacts)
        gen_images, intermediates = self.forward_sampling(
            prompt=[edit_prompt, ""], refer_latents=inverted_latents[::-1], end_step=end_step, batch_size=2, latents=init_code,
            guidance_scale=guidance_scale, num_inference_steps=num_steps, num_actual_inference_steps=num_steps - start_step, eta=eta,
            completion_mask_cfg=cfg_m, local_var_reg=var_m, share_attn=share_attn, method_type=method_type, verbose=verbose,
            blending=local_text_edit, local_perturbation=local_perturbation, return_intermediates=return_intermediates,
            use_share_attention=use_share_attention, end_scale=end_scale)
        c.reset()
        u8 = images_to_u8(gen_images[:2])
        return u8[0], u8[1], intermediates

    def Details_Preserving_regeneration_compose(self, source_image, inverted_latents, edit_prompt_list, ori_mask_lists, tgt_mask_lists,
                                                draw_mask, num_steps=100, start_step=30, end_step=10, eta=1, guidance_scale=7.5,
                                                dil_completion=False, appearance_transfer=False, share_attn=True, method_type="tca",
                                                verbose=False, local_text_edit=True, local_perturbation=True, return_intermediates=False,
                                                use_share_attention=False, dil_factor=15, end_scale=0.5):
        init_code = deepcopy(inverted_latents[-1])
        c = self.controller
        lp, cfg_m = self._setup_compose(c, source_image.shape[:2], init_code, ori_mask_lists, tgt_mask_lists, draw_mask, len(edit_prompt_list),
                                        method_type, share_attn, local_text_edit, dil_completion=dil_completion, dil_factor=dil_factor,
                                        appearance_transfer=appearance_transfer)
        img, intermediates = self.forward_sampling_compose(
            prompt=edit_prompt_list, refer_latents=inverted_latents[::-1], end_step=end_step, batch_size=init_code.shape[0],
            latents=init_code, guidance_scale=guidance_scale, num_inference_steps=num_steps,
            num_actual_inference_steps=num_steps - start_step, eta=eta, local_var_reg=lp, local_edit_text=local_text_edit,
            cfg_masks_tensor=cfg_m, share_attn=share_attn, method_type=method_type, verbose=verbose,
            local_perturbation=local_perturbation, return_intermediates=return_intermediates, end_scale=end_scale)
        c.reset()
        return images_to_u8(img[None])[0], intermediates

    def Details_Preserving_regeneration_background(self, ori_img, inverted_latents, edit_prompt, ori_mask, num_steps=100, start_step=30,
                                                   end_step=10, guidance_scale=3.5, eta=1, verbose=False, local_text_edit=True,
                                                   local_perturbation=True, end_scale=0.5, return_intermediates=False, share_attn=True,
                                                   method_type="tca", latent_blended=True, blend_range=(0, 40)):
        init_code = deepcopy(inverted_latents[-1])
        c = self.controller
        var_m = self._setup_background(c, ori_img.shape[:2], init_code, ori_mask, method_type, share_attn, local_text_edit)
        gen_images, intermediates = self.forward_sampling_background_gen(
            prompt=[edit_prompt, ""], end_step=end_step, batch_size=2, refer_latents=inverted_latents[::-1], latents=init_code,
            guidance_scale=guidance_scale, num_inference_steps=num_steps, num_actual_inference_steps=num_steps - start_step, eta=eta,
            local_cfg_reg=var_m, local_var_reg=var_m, share_attn=share_attn, method_type=method_type, verbose=verbose,
            local_text_edit=local_text_edit, local_perturbation=local_perturbation, return_intermediates=return_intermediates,
            end_scale=end_scale, latent_blended=latent_blended, blend_range=blend_range)
        c.reset()
        return images_to_u8(gen_images[:1])[0], intermediates

    _METHODS = ["tca", "ssa", "sdsa", "mmsa", "mmsa_es"]

    def FreeFine_generation(self, ori_img, ori_mask, coarse_input, target_mask, guidance_text, guidance_scale, eta, end_step=10,
                            num_step=50, start_step=25, share_attn=True, method_type="tca", local_text_edit=True,
                            local_perturbation=True, verbose=True, return_ori=False, seed=42, draw_mask=None,
                            return_intermediates=False, use_auto_draw=False, cons_area=None, reduce_inp_artifacts=False, end_scale=0.5):
        assert method_type in self._METHODS, f"check method type f{method_type}, which is not in {self._METHODS}"
        self._seed(seed)
        ori_mask, target_mask = self.mask_reduce_dim(ori_mask), self.mask_reduce_dim(target_mask)
        if draw_mask is not None:
            draw_mask = self.mask_reduce_dim(draw_mask)
        _, inverted = self.DDIM_inversion_func(img=coarse_input, mask=target_mask, prompt="", num_step=num_step, start_step=start_step,
                                               ref_img=ori_img, verbose=verbose)
        edit_img, ref_img, inter = self.Details_Preserving_regeneration(
            coarse_input, inverted, guidance_text, target_mask, ori_mask, draw_mask, num_steps=num_step, start_step=start_step,
            end_step=end_step, guidance_scale=guidance_scale, eta=eta, share_attn=share_attn, method_type=method_type, verbose=verbose,
            local_text_edit=local_text_edit, local_perturbation=local_perturbation, return_intermediates=return_intermediates,
            cons_area=cons_area, use_auto_draw=use_auto_draw, end_scale=end_scale, reduce_inp_artifacts=reduce_inp_artifacts)
        self.last_intermediates = inter
        return (edit_img, ref_img) if return_ori else edit_img

    # ------------------------------------------------------------------------------------------------------------
    # image-level batching: K independent FreeFine_generation edits as ONE image-major batch
    # ------------------------------------------------------------------------------------------------------------
    def _controllers_for_batch(self, K):
        """the registered controller plus K-1 siblings with the same layer selection; cached so that their static mask
        vectors (and therefore the captured graphs of the batched forward) survive from one batch to the next"""
        from .attention import Attention_Modulator
        base = self.controller
        assert isinstance(base, Attention_Modulator), "register_attention_control(model, Attention_Modulator(...)) first"
        ctrls = self._batch_ctrls.get(K)
        if ctrls is None or ctrls[0] is not base:
            ctrls = [base]
            for _ in range(K - 1):
                c = Attention_Modulator()
                c.layer_idx, c.num_att_layers, c.LOW_RESOURCE = list(base.layer_idx), base.num_att_layers, base.LOW_RESOURCE
                ctrls.append(c)
            self._batch_ctrls[K] = ctrls
        return ctrls

    @contextmanager
    def _batched_controllers(self, K):
        """K controllers on the UNet for an image-batched call (the registered one alone for K = 1; no graph flush: graphs are keyed by the
        plans); the registered controller is put back on the way out"""
        single = self.controller
        ctrls = self._controllers_for_batch(K)
        self.unet.controller = ctrls if K > 1 else single
        try:
            yield ctrls
        finally:
            self.unet.controller = single

    def _invert_batch(self, ctrls, source, num_step, start_step, **record):
        """the inversion all K cases share (model.py:1341-1388 + 816-925) -> (last latents, `refer_latents` of the guided loop)"""
        for c in ctrls:
            c.reset()
        _, inverted = self.invert(source, "", guidance_scale=1.0, num_inference_steps=num_step, num_actual_inference_steps=num_step - start_step,
                                  return_intermediates=True, **record)
        for c in ctrls:
            c.reset()
        return inverted[-1], inverted[::-1]

    @torch.no_grad()
    def FreeFine_generation_batch(self, cases, guidance_scale, eta, end_step=10, num_step=50, start_step=25, share_attn=True,
                                  method_type="tca", local_perturbation=True, verbose=True, return_ori=False, seeds=42,
                                  return_intermediates=False, end_scale=0.5):
        """K = len(cases) independent FreeFine_generation edits (model.py:1640-1700 each) sharing schedule, method and
        guidance scale, each with its own images, masks, prompt and seed, evaluated together: every UNet forward of the
        inversion runs 2K rows and every forward of the guided sampling K*Bp rows (Bp = 3 with row dedup, else 4), image-major.
        Rows of different images never interact (attention reference rows, GroupNorm and the scheduler are per row / per
        image), so result i equals FreeFine_generation(**cases[i], seed=seeds[i]) up to fp32 summation order where the GEMM
        split-K choice depends on the batch size.
        cases: dicts with ori_img, ori_mask, coarse_input, target_mask, guidance_text, draw_mask (+ optional use_auto_draw,
        cons_area, reduce_inp_artifacts).  Returns a list of edited images (or (edit, ref) pairs with return_ori)."""
        assert method_type in self._METHODS, f"check method type f{method_type}, which is not in {self._METHODS}"
        assert guidance_scale > 1.0, "USING THIS MODULE CFG Must > 1.0"
        K = len(cases)
        seeds = [seeds] * K if isinstance(seeds, int) else list(seeds)
        red = self.mask_reduce_dim
        with self._batched_controllers(K) as ctrls:
            seed_everything(seeds[0])
            # rows (coarse_i, ori_i); the original image's row is the guided loop's reference row
            source = torch.from_numpy(np.concatenate([np.stack([c["coarse_input"], self.resize_img(c["ori_img"], size=self._work_size(c["coarse_input"]))])
                                                      for c in cases]))
            init, refer = self._invert_batch(ctrls, source, num_step, start_step, record_rows=[2 * i + 1 for i in range(K)])
            cfg_f, var_masks, texts = [], [], []
            for case, c in zip(cases, ctrls):
                draw = case.get("draw_mask")
                cfg_m, var_m = self._setup_edit(c, case["coarse_input"].shape[:2], init, red(case["target_mask"]), red(case["ori_mask"]),
                                                None if draw is None else red(draw), method_type, share_attn, use_auto_draw=case.get("use_auto_draw", False),
                                                cons_area=case.get("cons_area"), reduce_inp_artifacts=case.get("reduce_inp_artifacts", False))
                cfg_f.append(self._mask_f(cfg_m))
                var_masks.append(var_m if local_perturbation else torch.ones_like(var_m))
                texts.append(torch.cat([self._encode_text(["", ""]), self._encode_text([case["guidance_text"], ""])], dim=0))
            noises = self._noise_per_case(seeds, num_step - start_step, (2,) + tuple(init.shape[1:]), eta)
            latents = init.clone()                                # [2K,4,h,w]: rows (edit_i, ref_i)
            latents, inter = self._guided_loop(EDIT, ctrls, texts, cfg_f, var_masks, noises, latents, refer,
                                               [[latents[2 * k:2 * k + 2]] for k in range(K)] if return_intermediates else None,
                                               method_type, num_step, start_step, end_step, end_scale, guidance_scale, eta)
            for c in ctrls:
                c.reset()
            self.last_intermediates = inter
            if return_ori:
                u8 = images_to_u8(self.latent2image(latents, return_type="pt"))
                return [(u8[2 * k], u8[2 * k + 1]) for k in range(K)]
            # the reference decodes both streams and drops the reference image unless return_ori (model.py:619, 1046-1049): decode only
            # the edited rows (VAE decode is per row: the kept image is unchanged)
            return images_to_u8(self.latent2image(latents[0::2].contiguous(), return_type="pt"))

    @torch.no_grad()
    def FreeFine_background_generation_batch(self, cases, guidance_scale, eta, end_step=10, num_step=50, start_step=25, share_attn=True,
                                             method_type="tca", local_text_edit=True, local_perturbation=True, verbose=True, seeds=42,
                                             return_intermediates=False, end_scale=0.5):
        """K independent FreeFine_background_generation calls (model.py:1088-1118 each) as one image-major batch: inversion runs K
        rows, guided sampling K*Bp rows (rows of image i: generated stream, re-noised reference stream).  Needs the bg-gen hook
        (register_attention_control_4bggen).  cases: dicts with ori_img, ori_mask, guidance_text.  Returns a list of images."""
        assert method_type in self._METHODS and guidance_scale > 1.0
        assert self.unet.hook == "bggen", "register_attention_control_4bggen(model, controller) first"
        K = len(cases)
        seeds = [seeds] * K if isinstance(seeds, int) else list(seeds)
        with self._batched_controllers(K) as ctrls:
            seed_everything(seeds[0])
            init, refer = self._invert_batch(ctrls, torch.from_numpy(np.stack([c["ori_img"] for c in cases])), num_step, start_step)
            cfg_f, var_masks, texts = [], [], []
            for case, c in zip(cases, ctrls):
                var_m = self._setup_background(c, case["ori_img"].shape[:2], init, self.mask_reduce_dim(case["ori_mask"]), method_type, share_attn,
                                               local_text_edit)
                cfg_f.append(self._mask_f(var_m) if local_text_edit else None)
                var_masks.append(var_m if local_perturbation else torch.ones_like(var_m))
                texts.append(torch.cat([self._encode_text(["", ""]), self._encode_text([case["guidance_text"], ""])], dim=0))
            noises = self._noise_per_case(seeds, num_step - start_step, (2,) + tuple(init.shape[1:]), eta)
            latents, inter = self._guided_loop(BACKGROUND, ctrls, texts, cfg_f, var_masks, noises, self._with_ref_rows(init), refer,
                                               [[init[k:k + 1]] for k in range(K)] if return_intermediates else None,
                                               method_type, num_step, start_step, end_step, end_scale, guidance_scale, eta)
            for c in ctrls:
                c.reset()
            self.last_intermediates = inter
            return images_to_u8(self.latent2image(latents[0::2].contiguous(), return_type="pt"))      # only the generated rows are returned (model.py:1118)

    @torch.no_grad()
    def FreeFine_cross_image_composition_batch(self, cases, guidance_scale, eta, end_step=10, num_step=50, start_step=25, share_attn=True,
                                               method_type="tca", local_text_edit=True, local_perturbation=True, verbose=True, seeds=42,
                                               return_intermediates=False, end_scale=0.5, dil_completion=False, dil_factor=15,
                                               appearance_transfer=False):
        """K independent FreeFine_cross_image_composition calls (model.py:1051-1086 each: appearance transfer / cross-image composition,
        BASELINE.json configs[3]) as ONE image-major batch: the inversion runs K (1 + R) rows, the guided loop K (R + 2) latent rows
        [edit_u, ref_1 .. ref_R, edit_c] against K (1 + R + P) text rows.  All cases share R (reference images) and P - 1 (prompts).
        Needs the composition hook (register_attention_control_compose).  cases: dicts with img_lists, ori_mask_lists, tgt_mask_lists,
        coarse_input, guidance_text_list (+ optional draw_mask).  Returns a list of images; image i equals the single call with
        seed seeds[i]."""
        assert method_type in self._METHODS and guidance_scale > 1.0
        assert self.unet.hook == "compose", "register_attention_control_compose(model, controller) first"
        K = len(cases)
        R, P = len(cases[0]["img_lists"]), len(cases[0]["guidance_text_list"]) + 1
        assert all(len(c["img_lists"]) == R and len(c["guidance_text_list"]) + 1 == P for c in cases), "batched compositions share R and the prompt count"
        seeds = [seeds] * K if isinstance(seeds, int) else list(seeds)
        red = self.mask_reduce_dim
        with self._batched_controllers(K) as ctrls:
            seed_everything(seeds[0])
            # rows (coarse_i, ref_i1 .. ref_iR): the composition hook leaves the reference rows unmodulated, so their K / V are recorded
            source = torch.from_numpy(np.concatenate([np.stack([c["coarse_input"]] + [self.resize_img(r, size=self._work_size(c["coarse_input"]))
                                                                                      for r in c["img_lists"]]) for c in cases]))
            init, refer = self._invert_batch(ctrls, source, num_step, start_step,
                                             record_rows=[k * (1 + R) + r for k in range(K) for r in range(1, 1 + R)], record_kv=True)
            cfg_f, var_masks, texts = [], [], []
            for case, c in zip(cases, ctrls):
                lp, cfg_m = self._setup_compose(c, case["coarse_input"].shape[:2], init, [red(m) for m in case["ori_mask_lists"]],
                                                [red(m) for m in case["tgt_mask_lists"]], case.get("draw_mask"), P - 1, method_type, share_attn,
                                                local_text_edit, dil_completion=dil_completion, dil_factor=dil_factor, appearance_transfer=appearance_transfer)
                cfg_f.append(self._mask_f(cfg_m) if local_text_edit else None)
                var_masks.append(lp if local_perturbation else torch.ones_like(lp))
                texts.append(torch.cat([self._encode_text([""] * (1 + R)), self._encode_text(list(case["guidance_text_list"]) + [""])], dim=0))
            noises = self._noise_per_case(seeds, num_step - start_step, (1,) + tuple(init.shape[1:]), eta)
            latents, inter = self._guided_loop(COMPOSE, ctrls, texts, cfg_f, var_masks, noises, init.clone(), refer,
                                               [[init[(1 + R) * k:(1 + R) * (k + 1)]] for k in range(K)] if return_intermediates else None,
                                               method_type, num_step, start_step, end_step, end_scale, guidance_scale, eta)
            for c in ctrls:
                c.reset()
            self.last_intermediates = inter
            return images_to_u8(self.latent2image(latents[0::1 + R].contiguous(), return_type="pt"))

    def FreeFine_background_generation(self, ori_img, ori_mask, guidance_text, guidance_scale, eta, end_step=10, num_step=50,
                                       start_step=25, share_attn=True, method_type="tca", local_text_edit=True, local_perturbation=True,
                                       verbose=True, seed=42, return_intermediates=False, end_scale=0.5, latent_blended=False,
                                       blend_range=(0, 40)):
        self._seed(seed)
        ori_mask = self.mask_reduce_dim(ori_mask)
        _, inverted = self.DDIM_inversion_func(img=ori_img, mask=ori_mask, prompt="", num_step=num_step, start_step=start_step,
                                               ref_img=None, verbose=verbose)
        img, inter = self.Details_Preserving_regeneration_background(
            ori_img, inverted, guidance_text, ori_mask, num_steps=num_step, start_step=start_step, end_step=end_step,
            guidance_scale=guidance_scale, eta=eta, share_attn=share_attn, method_type=method_type, verbose=verbose, end_scale=end_scale,
            local_text_edit=local_text_edit, local_perturbation=local_perturbation, return_intermediates=return_intermediates,
            latent_blended=latent_blended, blend_range=blend_range)
        self.last_intermediates = inter
        return img

    def FreeFine_cross_image_composition(self, img_lists, ori_mask_lists, tgt_mask_lists, coarse_input, guidance_text_list, guidance_scale,
                                         eta, end_step=10, num_step=50, start_step=25, share_attn=True, method_type="tca",
                                         local_text_edit=True, local_perturbation=True, verbose=True, seed=42, draw_mask=None,
                                         return_intermediates=False, use_auto_draw=False, end_scale=0.5, dil_completion=False,
                                         dil_factor=15, appearance_transfer=False):
        """model.py:1051-1086.  The reference forwards `use_auto_draw` to a callee without that parameter (TypeError as
        released); it is dropped here so the entry point works."""
        assert method_type in self._METHODS, f"check method type f{method_type}, which is not in {self._METHODS}"
        self._seed(seed)
        ori_mask_lists = [self.mask_reduce_dim(m) for m in ori_mask_lists]
        tgt_mask_lists = [self.mask_reduce_dim(m) for m in tgt_mask_lists]
        inverted = self.DDIM_inversion_func_compose(img=coarse_input, compose_imgs=img_lists, prompt="", num_step=num_step,
                                                    start_step=start_step, verbose=verbose)
        img, inter = self.Details_Preserving_regeneration_compose(
            coarse_input, inverted, guidance_text_list, ori_mask_lists, tgt_mask_lists, draw_mask, num_steps=num_step, start_step=start_step,
            end_step=end_step, dil_factor=dil_factor, guidance_scale=guidance_scale, eta=eta, share_attn=share_attn, method_type=method_type,
            verbose=verbose, dil_completion=dil_completion, local_text_edit=local_text_edit, local_perturbation=local_perturbation,
            return_intermediates=return_intermediates, end_scale=end_scale, appearance_transfer=appearance_transfer)
        self.last_intermediates = inter
        return img


class FreeFine:
    """the reference's thin wrapper (model.py:88-102); its run_* methods are empty there as well."""

    def __init__(self, pretrained_model_path="synthetic:sd21-base", device=None):
        self.model = FreeFinePipeline.from_pretrained(pretrained_model_path, torch_dtype=torch.float16)
        self.model.scheduler = DDIMScheduler.from_config(self.model.scheduler.config)

    def run_remove(self):
        pass

    def run_edit(self):
        pass

    def run_compose(self):
        pass
