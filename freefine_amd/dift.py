"""DIFT features (diffusion features: the activations of an up block of the Stable Diffusion UNet on a noised latent) on the project's own kernels.

Replaces SDFeaturizer of the reference's evaluation/metrics/MD/dift_sd.py (:189-236, with MyUNet2DConditionModel.forward :20-159 and
OneStepSDPipeline.__call__ :161-186), the feature extractor of the Mean Distance metric: VAE-encode the image, repeat the latent `ensemble_size` times, add noise
at timestep t, run the UNet up to the end of up block `up_ft_index`, average the feature maps over the ensemble.  Everything runs through HipVAE, the text
encoder of the pipeline and HipUNet.features; the ensemble mean is left to the matcher (ops.dift_match takes it in fp32), so the rows are returned untouched.

Two deviations from the reference, both deliberate:
  * VAE.  The reference SAMPLES the VAE posterior (`latent_dist.sample()`, dift_sd.py:177) from an unseeded device generator, so its features are not
    reproducible run to run.  This project's VAE produces the posterior mean (FreeFinePipeline.image2latent), and that is used here.
  * Weights.  The reference loads stabilityai/stable-diffusion-2-1.  The featurizer uses whatever checkpoint the pipeline holds: only the UNet topology and
    `alphas_cumprod` matter (the prediction type is never used -- no scheduler step is taken).
Noise follows the project's convention: an explicit [E, 4, h, w] tensor, or drawn on the CPU from `generator` / the global CPU generator (the reference draws
torch.randn_like on the device)."""
import numpy as np
import torch


class HipSDFeaturizer:
    def __init__(self, pipe):
        self.pipe = pipe

    def _latent(self, image):
        if isinstance(image, np.ndarray):
            assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3, "uint8 HWC image expected"
            return self.pipe.image2latent(image)
        assert torch.is_tensor(image) and image.is_floating_point() and image.shape[-3] == 3, "float [1, 3, H, W] / [3, H, W] tensor in [-1, 1] expected"
        return self.pipe.image2latent(image[None] if image.ndim == 3 else image)

    def _noisy(self, image, t, ensemble_size, noise, generator):
        """E noised copies of the image's latent: sqrt(abar_t) z + sqrt(1 - abar_t) noise (DDIMScheduler.add_noise)"""
        z = self._latent(image)
        assert z.shape[0] == 1, "one image per call"
        shape = (ensemble_size,) + tuple(z.shape[1:])
        if noise is None:
            noise = torch.randn(shape, generator=generator, dtype=torch.float32)
        assert tuple(noise.shape) == shape, (tuple(noise.shape), shape)
        abar = self.pipe.scheduler.alphas_cumprod[int(t)]
        return float(abar ** 0.5) * z.repeat(ensemble_size, 1, 1, 1) + float((1 - abar) ** 0.5) * noise.to(z.device, torch.float32)

    @torch.no_grad()
    def forward(self, image, prompt, t=261, up_ft_index=1, ensemble_size=8, noise=None, generator=None):
        """image: uint8 HWC array, or a [1, 3, H, W] / [3, H, W] tensor in [-1, 1] -> (rows [E, h*w, C] in the UNet's activation dtype, (h, w)).
        The rows may be strided (HipUNet.features); their mean over E is the reference's feature map."""
        x = self._noisy(image, t, ensemble_size, noise, generator)
        enc = self.pipe._encode_text([prompt]).repeat(ensemble_size, 1, 1)        # one prompt row per ensemble member, no CFG row (dift_sd.py:220-228)
        return self.pipe.unet.features(x, int(t), enc, up_ft_index)

    @torch.no_grad()
    def pair(self, src, edited, prompt, t=261, up_ft_index=1, ensemble_size=8, noise=None, noise_edited=None, generator=None):
        """forward(src) and forward(edited) as the 2E rows of ONE UNet batch -> (rows_src, rows_edited, (h, w)).  noise_edited defaults to `noise` when that
        is given, else to a second draw from the generator (the order two forward() calls would draw in)."""
        xs = self._noisy(src, t, ensemble_size, noise, generator)
        xe = self._noisy(edited, t, ensemble_size, noise_edited if noise_edited is not None else noise, generator)
        assert xs.shape == xe.shape, "source and edited image must have one size"
        enc = self.pipe._encode_text([prompt]).repeat(2 * ensemble_size, 1, 1)
        rows, hw = self.pipe.unet.features(torch.cat([xs, xe]), int(t), enc, up_ft_index)
        return rows[:ensemble_size], rows[ensemble_size:], hw

    @torch.no_grad()
    def forward_nchw(self, image, prompt, **kw):
        """the reference's return value: the ensemble mean as [1, C, h, w] fp32 (a permuted view of the [h*w, C] mean)"""
        rows, (h, w) = self.forward(image, prompt, **kw)
        m = rows.float().mean(0)
        return m.reshape(h, w, -1).permute(2, 0, 1).unsqueeze(0)

    __call__ = forward
