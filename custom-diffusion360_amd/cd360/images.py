"""The first stage as the sampling job and the training step use it: images <-> scaled latents, every kernel HIP.

`FirstStage` is `encode_first_stage` / `decode_first_stage` (diffusion.py:208-219) around `AutoencoderKLInferenceWrapper`
(autoencoder.py:304-322) with the modules the user already has: the HIP `Encoder` / `Decoder` of sgm.modules.diffusionmodules.model and the
reference's two 1 x 1 `nn.Conv2d` modules `quant_conv` / `post_quant_conv`, whose arithmetic -- together with the posterior sample, the two
`scale_factor` multiplications and the uint8 image conversion of sample.py:346 -- runs in the kernels of include/cd360_image.h:

  encode(x, seed, draw)   Encoder -> cd360_posterior_sample_f32     quant_conv + DiagonalGaussianDistribution.sample() + scale_factor * z
  encode_mode(x)          Encoder -> the same, seed NULL             ... .mode() ...
  decode(z)               cd360_post_quant_f32 -> Decoder            1 / scale_factor * z + post_quant_conv, fp32 NCHW image
  decode_u8(z)            cd360_post_quant_f32 -> Decoder.forward_u8 ... + clip(x * 0.5 + 0.5, 0, 1) * 255 -> uint8 [N, H, W, 3]

The posterior's noise is a pure function of (seed, streams[image], draw, channel, pixel), not of torch's generator: `draw` is the training
step (or any call count), so successive samples of one image differ, and a re-run of a step reproduces its latents on any rank layout.
Forward only, under no_grad; a CPU tensor raises.

Keeping part of a picture, or starting from one (masked and image-to-image sampling):

  known = first_stage.encode_mode(picture)                  [P, 4, h, w]: the latents of the pictures to keep / to start from
  masks = latent_mask(region)                               [P, 1, h, w]: 1 = generate, 0 = keep, from an image-resolution mask
  job.sample_images(..., init_latents=known, masks=masks)   keeps the picture outside the region, synthesises inside it
  job.sample_images(..., init_latents=known, masks=masks, first_step=k, latent_hw=(h, w))   and runs only rows k.. of the schedule"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .derived import derived
from .sampler import seed_words


def _conv1x1_pack(conv: nn.Conv2d, n_out: int, n_in: int):
    if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.in_channels == n_in and conv.out_channels == n_out
            and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1):
        raise ValueError(f"a 1 x 1 nn.Conv2d of {n_in} -> {n_out} channels is needed (z_channels = embed_dim = 4), got {conv}")

    def make():
        w = conv.weight.detach().float().reshape(n_out, n_in).contiguous()
        b = conv.bias.detach().float().contiguous() if conv.bias is not None else torch.zeros(n_out, dtype=torch.float32, device=w.device)
        return w, b
    return derived(conv, "_cd360_pack", (conv.weight, conv.bias), make)


def latent_mask(mask: torch.Tensor, factor: int = 8) -> torch.Tensor:
    """An image-resolution mask [N, 1, H, W] or [N, H, W] (bool / uint8 / float; nonzero resp. 1 = generate) -> the mask of the latent's
    pixels [N, 1, H / factor, W / factor] fp32: the area average, so a latent pixel on the region's border blends in proportion.  torch,
    once per image, outside the step; H and W must be multiples of `factor` (the first stage's down-sampling)."""
    if not isinstance(mask, torch.Tensor) or mask.ndim not in (3, 4) or (mask.ndim == 4 and mask.shape[1] != 1):
        raise ValueError(f"mask: [N, 1, H, W] or [N, H, W] is needed, got {tuple(getattr(mask, 'shape', ()))}")
    if mask.ndim == 3:
        mask = mask[:, None]
    H, W = mask.shape[2:]
    if factor <= 0 or H % factor or W % factor or H * W == 0:
        raise ValueError(f"mask of {H} x {W}: both must be positive multiples of factor = {factor}")
    m = (mask != 0) if mask.dtype in (torch.bool, torch.uint8) else mask
    return torch.nn.functional.avg_pool2d(m.float(), factor).contiguous()


class FirstStage:
    def __init__(self, encoder, decoder, quant_conv: nn.Conv2d, post_quant_conv: nn.Conv2d, scale_factor: float = 0.13025):
        self.encoder, self.decoder, self.quant_conv, self.post_quant_conv = encoder, decoder, quant_conv, post_quant_conv
        self.scale_factor = float(scale_factor)
        if quant_conv is not None:
            _conv1x1_pack(quant_conv, 8, 8)
        if post_quant_conv is not None:
            _conv1x1_pack(post_quant_conv, 4, 4)

    @staticmethod
    def _gpu(t: torch.Tensor) -> torch.Tensor:
        if not t.is_cuda:
            raise ops.Cd360Error("the first-stage HIP modules run only on the GPU; got a CPU tensor")
        return t

    # ------------------------------------------------------------------------------------------------ images -> latents
    @torch.no_grad()
    def _moments(self, x: torch.Tensor) -> torch.Tensor:
        return self.encoder(self._gpu(x)).float().contiguous()

    @torch.no_grad()
    def encode(self, x: torch.Tensor, seed: int, draw: int, streams=None) -> torch.Tensor:
        """encode_first_stage with AutoencoderKLInferenceWrapper: x [N, 3, H, W] -> the scaled posterior sample [N, 4, H / 8, W / 8] fp32.
        seed: any Python int; draw: the training step or a call count; streams: one noise stream id per image (default 0 for all)."""
        moments = self._moments(x)
        dev = moments.device
        n = moments.shape[0]
        seed_t = torch.tensor([seed_words(seed)], dtype=torch.int64, device=dev)
        draw_t = torch.tensor([int(draw)], dtype=torch.int32, device=dev)
        if streams is not None and len(streams) != n:
            raise ValueError(f"{len(streams)} noise stream ids for {n} images")
        streams_t = None if streams is None else torch.tensor([int(v) for v in streams], dtype=torch.int32, device=dev)
        w, b = _conv1x1_pack(self.quant_conv, 8, 8)
        return ops.posterior_sample(moments, w, b, seed_t, streams_t, draw_t, self.scale_factor)

    @torch.no_grad()
    def encode_mode(self, x: torch.Tensor) -> torch.Tensor:
        """The mode() form: the scaled posterior mean, no noise."""
        w, b = _conv1x1_pack(self.quant_conv, 8, 8)
        return ops.posterior_sample(self._moments(x), w, b, None, None, None, self.scale_factor)

    # ------------------------------------------------------------------------------------------------ latents -> images
    @torch.no_grad()
    def _decoder_input(self, z: torch.Tensor) -> torch.Tensor:
        w, b = _conv1x1_pack(self.post_quant_conv, 4, 4)
        return ops.post_quant(self._gpu(z).float().contiguous(), w, b, 1.0 / self.scale_factor)

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """decode_first_stage: z [N, 4, h, w] (scaled latents) -> the image [N, 3, 8 h, 8 w], fp32 NCHW."""
        zin = self._decoder_input(z)
        return self.decoder(zin).float()

    @torch.no_grad()
    def decode_u8(self, z: torch.Tensor) -> torch.Tensor:
        """z [N, 4, h, w] -> uint8 [N, 8 h, 8 w, 3]: (clip(decode(z) * 0.5 + 0.5, 0, 1) * 255).to(uint8) in HWC order, written by the decoder's
        last kernel."""
        zin = self._decoder_input(z)
        return self.decoder.forward_u8(zin)
