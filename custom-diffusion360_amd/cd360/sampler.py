"""Sampler / guider / denoiser step on either side of the UNet, restated from scratch.

Reference: EulerEDMSampler (sgm/modules/diffusionmodules/sampling.py:23-136,314-318), ScheduledCFGImgTextRef / VanillaCFGImgRef
(guiders.py:102-166), DiscreteDenoiser + EpsScaling (denoiser.py:6-79, denoiser_scaling.py:26-32), LegacyDDPMDiscretization
(discretizer.py:17-69).  Same class names and call signatures (they are re-exported under the reference's dotted paths in
custom-diffusion360_amd/sgm/modules/diffusionmodules/), so the YAML sampler/denoiser/guider configs resolve unchanged.

Everything stays on the device and nothing synchronises: the sigma -> index quantisation is an argmin + gather on the GPU, and
with `fused=True` the per-step tail (c_out scaling, 3-way or 2-way CFG combine, to_d, Euler update) is one HIP kernel
(cd360_cfg_euler_step_f32) instead of ~10 tiny elementwise launches.  The further samplers and their tables are at the end.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np
import torch


def append_dims(x: torch.Tensor, target_dims: int) -> torch.Tensor:
    return x[(...,) + (None,) * (target_dims - x.ndim)]


# ----------------------------------------------------------------------------------------------- discretisation
class LegacyDDPMDiscretization:
    """sigma_i = sqrt((1 - acp_i) / acp_i) on the SD linear-sqrt beta schedule (discretizer.py:47-69)."""

    def __init__(self, linear_start=0.00085, linear_end=0.0120, num_timesteps=1000):
        self.num_timesteps = num_timesteps
        betas = (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, num_timesteps, dtype=torch.float64) ** 2).numpy()
        self.alphas_cumprod = np.cumprod(1.0 - betas, axis=0)

    def get_sigmas(self, n, device="cpu"):
        if n < self.num_timesteps:
            timesteps = np.linspace(self.num_timesteps - 1, 0, n, endpoint=False).astype(int)[::-1]  # discretizer.py:11-14
            acp = self.alphas_cumprod[timesteps]
        elif n == self.num_timesteps:
            acp = self.alphas_cumprod
        else:
            raise ValueError
        sigmas = torch.tensor((1 - acp) / acp, dtype=torch.float32, device=device) ** 0.5
        return torch.flip(sigmas, (0,))

    def __call__(self, n, do_append_zero=True, device="cpu", flip=False):
        sigmas = self.get_sigmas(n, device=device)
        if do_append_zero:
            sigmas = torch.cat([sigmas, sigmas.new_zeros([1])])
        return sigmas if not flip else torch.flip(sigmas, (0,))


class EDMDiscretization:
    """The Karras rho schedule, sigma_i = (sigma_max^(1/rho) + i / (n - 1) (sigma_min^(1/rho) - sigma_max^(1/rho)))^rho
    (discretizer.py:28-39): the reference's expression in the reference's order, in fp32 on `device`.  Its values lie OFF the 1000-entry
    table DiscreteDenoiser snaps to (on_grid, below): the network then runs at the snapped sigma, the solver on the schedule's own."""

    def __init__(self, sigma_min=0.002, sigma_max=80.0, rho=7.0):
        self.sigma_min, self.sigma_max, self.rho = sigma_min, sigma_max, rho

    __call__ = LegacyDDPMDiscretization.__call__  # the call protocol every discretisation shares (discretizer.py:17-21)

    def get_sigmas(self, n, device="cpu"):
        ramp = torch.linspace(0, 1, n, device=device)
        min_inv_rho = self.sigma_min ** (1 / self.rho)
        max_inv_rho = self.sigma_max ** (1 / self.rho)
        return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** self.rho


class ListDiscretization:
    """A caller's own schedule (a published few-step list): `sigmas` strictly decreasing and positive, handed back as fp32 for exactly
    n = len(sigmas); the zero is appended as by the other discretisations."""

    def __init__(self, sigmas):
        vals = [float(v) for v in (sigmas.detach().cpu().reshape(-1).tolist() if isinstance(sigmas, torch.Tensor) else sigmas)]
        if not vals or not all(v > 0 and v < float("inf") for v in vals):
            raise ValueError(f"a sigma list holds positive finite values, got {vals}")
        self.sigmas = torch.tensor(vals, dtype=torch.float32)
        if not bool((self.sigmas[1:] < self.sigmas[:-1]).all()):  # (compared as the fp32 values the steps will use)
            raise ValueError(f"a sigma list is strictly decreasing, got {vals}")

    __call__ = LegacyDDPMDiscretization.__call__

    def get_sigmas(self, n, device="cpu"):
        if n != self.sigmas.numel():
            raise ValueError(f"this list holds {self.sigmas.numel()} sigmas; asked for {n}")
        return self.sigmas.to(device)


def on_grid(sigmas: torch.Tensor, denoiser: "DiscreteDenoiser") -> bool:
    """Does every non-zero entry of `sigmas` lie ON the denoiser's table, possibly_quantize_sigma(s) == s?  Then c_out, c_in and the time
    embedding (from the snapped sigma) and to_d / dt / the multistep coefficients (from the schedule's own) read one scalar per step, as on
    LegacyDDPMDiscretization; otherwise a step needs both.  Decided once per schedule, in CPU fp32 whatever device the two live on."""
    sig = sigmas.detach().to("cpu", torch.float32).reshape(-1)
    sig = sig[sig != 0]
    return bool(torch.equal(snap_c_in(denoiser, denoiser.sigmas.detach().to("cpu", torch.float32), sig)[1], sig))


# ----------------------------------------------------------------------------------------------- denoiser
class EpsScaling:
    def __call__(self, sigma):
        return torch.ones_like(sigma), -sigma, 1 / (sigma ** 2 + 1.0) ** 0.5, sigma.clone()


class EpsWeighting:
    def __call__(self, sigma):
        return sigma ** -2.0


class DiscreteDenoiser(torch.nn.Module):
    """D(x; sigma) = c_skip x + c_out F(c_in x; idx(sigma)) with sigma snapped to the 1000-entry table (denoiser.py:22-79).
    The reference-stream noise injection of the training path (:26-39) is kept."""

    def __init__(self, weighting_config=None, scaling_config=None, num_idx=1000, discretization_config=None, do_append_zero=False,
                 quantize_c_noise=True, flip=True):
        super().__init__()
        from sgm.util import instantiate_from_config
        self.weighting = instantiate_from_config(weighting_config) if weighting_config else EpsWeighting()
        self.scaling = instantiate_from_config(scaling_config) if scaling_config else EpsScaling()
        disc = instantiate_from_config(discretization_config) if discretization_config else LegacyDDPMDiscretization()
        self.register_buffer("sigmas", disc(num_idx, do_append_zero=do_append_zero, flip=flip))
        self.quantize_c_noise = quantize_c_noise

    def w(self, sigma):
        return self.weighting(sigma)

    def sigma_to_idx(self, sigma):
        return (sigma - self.sigmas[:, None]).abs().argmin(dim=0).view(sigma.shape)

    def idx_to_sigma(self, idx):
        return self.sigmas[idx]

    def possibly_quantize_sigma(self, sigma):
        return self.idx_to_sigma(self.sigma_to_idx(sigma))

    def possibly_quantize_c_noise(self, c_noise):
        return self.sigma_to_idx(c_noise) if self.quantize_c_noise else c_noise

    def network_inputs(self, input, sigma, kwargs):
        """Everything before the network call: (scaled input, c_noise, c_skip, c_out, kwargs)."""
        sigma = self.possibly_quantize_sigma(sigma)
        sigma_shape = sigma.shape
        sigma = append_dims(sigma, input.ndim)
        kwargs = dict(kwargs)
        sigmas_ref = kwargs.pop("sigmas_ref", None)
        if sigmas_ref is not None:
            kwargs["sigmas_ref"] = sigmas_ref
            if kwargs.get("input_ref") is not None:
                xr = kwargs["input_ref"]
                xr = xr + torch.randn_like(xr) * append_dims(sigmas_ref, xr.ndim)
                _, _, c_in_ref, _ = self.scaling(append_dims(sigmas_ref, xr.ndim))
                kwargs["input_ref"] = xr * c_in_ref
                kwargs["sigmas_ref"] = self.possibly_quantize_c_noise(sigmas_ref)
        c_skip, c_out, c_in, c_noise = self.scaling(sigma)
        c_noise = self.possibly_quantize_c_noise(c_noise.reshape(sigma_shape))
        return input * c_in, c_noise, c_skip, c_out, kwargs

    def forward(self, network, input, sigma, cond, sigmas_ref=None, **kwargs):
        if sigmas_ref is not None:
            kwargs["sigmas_ref"] = sigmas_ref
        x_in, c_noise, c_skip, c_out, kw = self.network_inputs(input, sigma, kwargs)
        predict, fg_mask_list, alphas_list, rgb_list = network(x_in, c_noise, cond, **kw)
        return predict * c_out + input * c_skip, fg_mask_list, alphas_list, rgb_list


# ----------------------------------------------------------------------------------------------- guiders
def _split_cat(c, uc, nx, order):
    """rows [0:nx] are the target's conditioning, the rest the reference views' (guiders.py:119-128)."""
    parts = {"uc1": uc[:nx], "uc2": uc[nx:], "c1": c[:nx], "c2": c[nx:]}
    return torch.cat([parts[k] for k in order], 0)


class ScheduledCFGImgTextRef:
    """3-way CFG: x_u + scale (x_c - x_ic) + scale_im (x_ic - x_u)   (guiders.py:102-133)."""

    branches = 3

    def __init__(self, scale: float, scale_im: float):
        self.scale, self.scale_im = scale, scale_im

    def __call__(self, x, sigma):
        x_u, x_ic, x_c = x.chunk(3)
        return x_u + self.scale * (x_c - x_ic) + self.scale_im * (x_ic - x_u)

    def prepare_inputs(self, x, s, c, uc):
        c_out = {}
        for k in c:
            if k in ("vector", "crossattn", "concat"):
                c_out[k] = _split_cat(c[k], uc[k], x.size(0), ("uc1", "uc1", "c1", "uc2", "c2", "c2"))
            else:
                assert c[k] == uc[k]
                c_out[k] = c[k]
        return torch.cat([x] * 3), torch.cat([s] * 3), c_out


class VanillaCFGImgRef:
    """2-way CFG: x_u + scale (x_c - x_u)   (guiders.py:136-166)."""

    branches = 2

    def __init__(self, scale: float):
        self.scale = scale

    def __call__(self, x, sigma):
        x_u, x_c = x.chunk(2)
        return x_u + self.scale * (x_c - x_u)

    def prepare_inputs(self, x, s, c, uc):
        c_out = {}
        for k in c:
            if k in ("vector", "crossattn", "concat"):
                c_out[k] = _split_cat(c[k], uc[k], x.size(0), ("uc1", "c1", "uc2", "c2"))
            else:
                assert c[k] == uc[k]
                c_out[k] = c[k]
        return torch.cat([x] * 2), torch.cat([s] * 2), c_out


class IdentityGuider:
    branches = 1

    def __call__(self, x, sigma):
        return x

    def prepare_inputs(self, x, s, c, uc):
        return x, s, {k: c[k] for k in c}


# ----------------------------------------------------------------------------------------------- sampler
class BaseDiffusionSampler:
    """What every sampler here is built on (sampling.py:23-83): the discretisation, the guider, the set-up of the loop and the guided
    denoiser call.

    `denoiser(x_batched, sigma_batched, cond) -> (denoised, fg_masks, alphas, rgb_list)` is what DiffusionEngine.sample builds
    (sgm/models/diffusion.py:375-401)."""

    def __init__(self, discretization_config=None, num_steps: Optional[int] = None, guider_config=None, verbose: bool = False,
                 device: str = "cuda"):
        from sgm.util import instantiate_from_config
        self.num_steps = num_steps
        self.discretization = instantiate_from_config(discretization_config) if discretization_config else LegacyDDPMDiscretization()
        self.guider = instantiate_from_config(guider_config) if guider_config else IdentityGuider()
        self.verbose, self.device = verbose, device

    def prepare_sampling_loop(self, x, cond, uc=None, num_steps=None):
        sigmas = self.discretization(self.num_steps if num_steps is None else num_steps, device=x.device)
        uc = cond if uc is None else uc
        x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)
        return x, x.new_ones([x.shape[0]]), sigmas, len(sigmas), cond, uc

    def denoise(self, x, denoiser, sigma, cond, uc):
        denoised, _, _, rgb_list = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc))
        return self.guider(denoised, sigma), rgb_list


class EulerEDMSampler(BaseDiffusionSampler):
    """Euler steps over the sub-sampled sigma schedule (sampling.py:85-136, 314-318); with s_churn = 0 DDIM-equivalent under EpsScaling.

    s_churn > 0 (sampling.py:96-100, 120-124): on every step whose sigma lies in [s_tmin, s_tmax] the latent is first pushed to
    sigma_hat = sigma (1 + gamma), gamma = min(s_churn / n_steps, sqrt 2 - 1), by adding noise of standard deviation
    s_noise (sigma_hat^2 - sigma^2)^0.5; the network is then evaluated at sigma_hat (DiscreteDenoiser snaps it to its grid) and the Euler
    step runs from sigma_hat.  gamma = 0 keeps the un-churned arithmetic bit for bit (sigma * 1.0 is sigma).

    `noise_sampler`: with seed=None it is torch.randn_like, the reference's draw.  With seed=<int> it is the library's counter-based generator
    (cd360_sampler_noise_f32: Philox4x32-10 + Box-Muller, stream 0), which is what cd360.job.Sampler(s_churn=..., seed=...) draws inside its
    captured step: GPU tensors only.  Its step word is the INDEX OF THE STEP since __call__ / prepare_sampling_loop began, counted on every
    step whether or not it draws (EulerAncestralSampler counts draws: under an s_tmin / s_tmax window the two differ, and the job's
    kernels read the step index)."""

    def __init__(self, discretization_config=None, num_steps: Optional[int] = None, guider_config=None, verbose: bool = False,
                 device: str = "cuda", s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, seed: Optional[int] = None):
        super().__init__(discretization_config, num_steps, guider_config, verbose, device)
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = s_churn, s_tmin, s_tmax, s_noise
        self.seed, self._step, self._noise = seed, 0, None
        self.noise_sampler = (lambda x: torch.randn_like(x)) if seed is None else self._seeded_noise

    def _seeded_noise(self, x):
        return seeded_noise(self, x, self._step)

    def prepare_sampling_loop(self, x, cond, uc=None, num_steps=None):
        self._step = 0
        return super().prepare_sampling_loop(x, cond, uc, num_steps)

    def euler_step(self, x, d, dt):
        return x + dt * d

    def possible_correction_step(self, euler_step, x, d, dt, next_sigma, denoiser, cond, uc):
        return euler_step

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, gamma=0.0):
        sigma_hat = sigma * (gamma + 1.0)
        if gamma > 0:
            eps = self.noise_sampler(x) * self.s_noise
            x = x + eps * append_dims(sigma_hat ** 2 - sigma ** 2, x.ndim) ** 0.5
        denoised, rgb_list = self.denoise(x, denoiser, sigma_hat, cond, uc)
        d = (x - denoised) / append_dims(sigma_hat, x.ndim)
        dt = append_dims(next_sigma - sigma_hat, x.ndim)
        euler_step = self.euler_step(x, d, dt)
        x = self.possible_correction_step(euler_step, x, d, dt, next_sigma, denoiser, cond, uc)
        self._step += 1
        return x, rgb_list

    def gamma_of(self, sigma, n_steps):
        """the reference's per-step gamma (sampling.py:120-124); without churn 0.0 either way, and no sigma is read back from the device"""
        if not self.s_churn:
            return 0.0
        return min(self.s_churn / n_steps, 2 ** 0.5 - 1) if self.s_tmin <= sigma <= self.s_tmax else 0.0

    def __call__(self, denoiser: Callable, x, cond: Dict, uc=None, num_steps=None, mask=None, init_im=None):
        """`mask` [N or 1, 1, H, W] at latent resolution (1 = generate, 0 = keep) with `init_im` [N, 4, H, W], the known latent as
        encode_first_stage returns it: after every step the region to keep is replaced by init_im at the step's new noise level
        (masked_blend).  The reference takes both arguments and never reads them (sampling.py:112-136).  That noise is torch.randn_like
        for seed=None and, for seed=<int>, ops.edit_noise at the step's index: what cd360.job.Sampler(known=, mask=) draws inside its
        captured step.  mask=None: today's arithmetic and draw order."""
        check_edit_args(x, init_im, mask)
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        rgb_list = None
        for i in range(num_sigmas - 1):
            gamma = self.gamma_of(sigmas[i], num_sigmas - 1)
            x, rgb_list = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc, gamma)
            if mask is not None:
                noise = torch.randn_like(x) if self.seed is None else seeded_edit_noise(self, x, i)
                x = masked_blend(x, init_im, mask, s_in * sigmas[i + 1], noise)
        return x, rgb_list

    forward = __call__


class HeunEDMSampler(EulerEDMSampler):
    """Heun's second-order method on the EDM step (sampling.py:321-337): after the Euler predictor to sigma_next the network is evaluated a
    second time, at (euler_step, sigma_next), and the step is redone with the mean of the two directions; skipped where sigma_next = 0, so n
    steps cost 2n - 1 network evaluations.  Same constructor as EulerEDMSampler (churn included); returns (x, rgb_list) with the rgb_list
    of the step's last `denoise`.

    The reference's class does not run in its own fork as written: BaseDiffusionSampler.denoise returns (denoised, rgb_list) and
    possible_correction_step uses that tuple as a tensor.  Here `denoise` is unpacked -- the arithmetic is the reference's, operation by
    operation, including the host-side skip on torch.sum(next_sigma) < 1e-14 and the torch.where on next_sigma > 0."""

    def possible_correction_step(self, euler_step, x, d, dt, next_sigma, denoiser, cond, uc):
        if torch.sum(next_sigma) < 1e-14:  # save a network evaluation if all noise levels are 0
            return euler_step
        denoised, self._rgb2 = self.denoise(euler_step, denoiser, next_sigma, cond, uc)
        d_new = (euler_step - denoised) / append_dims(next_sigma, euler_step.ndim)
        d_prime = (d + d_new) / 2.0
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0, x + d_prime * dt, euler_step)

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, gamma=0.0):
        self._rgb2 = None
        x, rgb_list = super().sampler_step(sigma, next_sigma, denoiser, x, cond, uc, gamma)
        return x, (rgb_list if self._rgb2 is None else self._rgb2)


def cfg_branch_count(x: torch.Tensor, eps: torch.Tensor, scale_im: Optional[float]) -> int:
    """3 (ScheduledCFGImgTextRef: u | ic | c) or, for scale_im=None, 2 (VanillaCFGImgRef: u | c); eps must hold that many rows per latent."""
    nb = 2 if scale_im is None else 3
    if eps.shape[0] != nb * x.shape[0]:
        raise ValueError(f"eps holds {eps.shape[0]} rows; the {nb}-branch step on {x.shape[0]} latents needs {nb * x.shape[0]}")
    return nb


def cfg_combine(x: torch.Tensor, eps: torch.Tensor, sigma: torch.Tensor, scale: float, scale_im: Optional[float]) -> torch.Tensor:
    """d0 of the fused tails in plain torch, in the kernels' order (csrc/sampler_stage.hip::cfg_combine): den_b = x - sigma eps_b, then the
    guider's combine.  Two branches are the three-branch expression without the image term."""
    if scale_im is None:
        e_u, e_c = eps.float().chunk(2)
        du, dc = x - sigma * e_u, x - sigma * e_c
        return du + scale * (dc - du)
    e_u, e_ic, e_c = eps.float().chunk(3)
    du, dic, dc = x - sigma * e_u, x - sigma * e_ic, x - sigma * e_c
    return du + scale * (dc - dic) + scale_im * (dic - du)


def cfg_euler_update(x: torch.Tensor, eps: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor, scale: float,
                     scale_im: Optional[float] = None, fused: bool = True) -> torch.Tensor:
    """One fused tail of a CFG Euler step with EpsScaling: x [n,...] fp32, sigma / sigma_next 0-d device tensors, den_b = x - sigma eps_b,
    x' = x + (x - d0) / sigma * (sigma_next - sigma) with
      scale_im a number (ScheduledCFGImgTextRef):  eps [3n,...] (u | ic | c),  d0 = den_u + scale (den_c - den_ic) + scale_im (den_ic - den_u)
      scale_im=None     (VanillaCFGImgRef):        eps [2n,...] (u | c),       d0 = den_u + scale (den_c - den_u)."""
    cfg_branch_count(x, eps, scale_im)
    if fused and x.is_cuda:
        from . import ops
        return ops.cfg_euler_step(x, eps, sigma, sigma_next, scale, scale_im)
    d0 = cfg_combine(x, eps, sigma, scale, scale_im)
    return x + (x - d0) / sigma * (sigma_next - sigma)


def guider_scales(guider):
    """(scale, scale_im) as cfg_euler_update takes them: scale_im=None for the two-branch VanillaCFGImgRef."""
    if isinstance(guider, ScheduledCFGImgTextRef):
        return guider.scale, guider.scale_im
    if isinstance(guider, VanillaCFGImgRef):
        return guider.scale, None
    raise TypeError(f"the fused step serves ScheduledCFGImgTextRef and VanillaCFGImgRef, not {type(guider).__name__}")


def cfg_eps(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, sigma: torch.Tensor, branches: int) -> torch.Tensor:
    """The head every fused step shares: the guider's batch [x] * B (the conditioning batch is assembled once per image), DiscreteDenoiser's
    network inputs with sigma snapped to the table ON the device, and the network over the CFG batch -> eps [B n, ...]."""
    xb = x.expand(branches, *x.shape[1:]) if x.shape[0] == 1 else torch.cat([x] * branches)
    x_in, c_noise, _, _, _ = denoiser.network_inputs(xb, sigma.expand(xb.shape[0]), {})
    return network(x_in, c_noise)


def fused_cfg_euler_step(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                         guider, fused: bool = True) -> torch.Tensor:
    """ONE step of EulerEDMSampler.sampler_step (sampling.py:85-136) under ScheduledCFGImgTextRef (guiders.py:102-133) or VanillaCFGImgRef
    (guiders.py:136-166) and DiscreteDenoiser + EpsScaling (denoiser.py:47-79), in the form the product's sampling job launches it
    (cd360/job.py); B = guider.branches:

        xB = [x] * B                                       guider.prepare_inputs (the conditioning batch is assembled once per image)
        x_in, c_noise = c_in(sigma_q) xB, idx(sigma_q)     DiscreteDenoiser.network_inputs, sigma snapped to the table ON the device
        eps = network(x_in, c_noise)                       the UNet over the CFG batch
        x' = cfg_euler_update(x, eps, sigma, sigma_next)   c_out scaling + CFG combine + to_d + Euler: cd360_cfg_euler_step_f32

    `network(x_in, c_noise) -> eps [B n, ...]`; sigma / sigma_next 0-d device tensors of the sampler's schedule (table entries, so the
    snapped sigma_q of c_out equals the sigma of to_d, as in the reference's own run).  No host synchronisation anywhere in the step."""
    scale, scale_im = guider_scales(guider)
    eps = cfg_eps(denoiser, network, x, sigma, guider.branches)
    return cfg_euler_update(x, eps.contiguous(), sigma.reshape(1), sigma_next.reshape(1), scale, scale_im, fused=fused)


def fused_cfg3_euler_step(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor,
                          scale: float, scale_im: float, fused: bool = True) -> torch.Tensor:
    """fused_cfg_euler_step under ScheduledCFGImgTextRef(scale, scale_im): the three-branch step by its earlier name."""
    return fused_cfg_euler_step(denoiser, network, x, sigma, sigma_next, ScheduledCFGImgTextRef(scale, scale_im), fused=fused)


# ----------------------------------------------------------------------------------------------- DPM++ 2M
def to_neg_log_sigma(sigma):  # sampling_utils.py
    return sigma.log().neg()


def to_sigma(neg_log_sigma):
    return neg_log_sigma.neg().exp()


class DPMPP2MSampler(BaseDiffusionSampler):
    """DPM-Solver++(2M): x' = m1 x - m2 dd with dd = denoised on the first step and where sigma_next = 0, (1 + 1/2r) denoised - (1/2r) old_denoised
    otherwise (sampling.py:390-465).  One network evaluation per step, deterministic.

    The reference's class does not run in its own fork as written: BaseDiffusionSampler.denoise returns (denoised, rgb_list), sampler_step
    multiplies that tuple, and __call__ returns x alone where DiffusionEngine.sample unpacks two values.  Here `denoise` is unpacked -- the
    arithmetic is the reference's, operation by operation --, the rgb_list of the last denoise call is kept on the instance, and __call__
    returns (x, rgb_list)."""

    def __init__(self, discretization_config=None, num_steps: Optional[int] = None, guider_config=None, verbose: bool = False, device: str = "cuda"):
        super().__init__(discretization_config, num_steps, guider_config, verbose, device)
        self.rgb_list = None

    def get_variables(self, sigma, next_sigma, previous_sigma=None):
        t, t_next = [to_neg_log_sigma(s) for s in (sigma, next_sigma)]
        h = t_next - t
        if previous_sigma is not None:
            h_last = t - to_neg_log_sigma(previous_sigma)
            r = h_last / h
            return h, r, t, t_next
        return h, None, t, t_next

    def get_mult(self, h, r, t, t_next, previous_sigma):
        mult1 = to_sigma(t_next) / to_sigma(t)
        mult2 = (-h).expm1()
        if previous_sigma is not None:
            mult3 = 1 + 1 / (2 * r)
            mult4 = 1 / (2 * r)
            return mult1, mult2, mult3, mult4
        return mult1, mult2

    def sampler_step(self, old_denoised, previous_sigma, sigma, next_sigma, denoiser, x, cond, uc=None):
        denoised, self.rgb_list = self.denoise(x, denoiser, sigma, cond, uc)
        h, r, t, t_next = self.get_variables(sigma, next_sigma, previous_sigma)
        mult = [append_dims(m, x.ndim) for m in self.get_mult(h, r, t, t_next, previous_sigma)]
        x_standard = mult[0] * x - mult[1] * denoised
        if old_denoised is None or torch.sum(next_sigma) < 1e-14:  # first step, or all noise levels 0: the first-order update
            return x_standard, denoised
        denoised_d = mult[2] * denoised - mult[3] * old_denoised
        x_advanced = mult[0] * x - mult[1] * denoised_d
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0, x_advanced, x_standard), denoised

    def __call__(self, denoiser: Callable, x, cond: Dict, uc=None, num_steps=None, **kwargs):
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        old_denoised = None
        for i in range(num_sigmas - 1):
            x, old_denoised = self.sampler_step(old_denoised, None if i == 0 else s_in * sigmas[i - 1], s_in * sigmas[i], s_in * sigmas[i + 1],
                                                denoiser, x, cond, uc=uc)
        return x, self.rgb_list

    forward = __call__


def dpmpp2m_multipliers(sigmas: torch.Tensor) -> torch.Tensor:
    """The per-schedule table of DPMPP2MSampler: sigmas [n + 1] (the discretisation's output, last = 0) -> [n, 4] fp32 (m1, m2, m3, m4), row i
    = get_variables / get_mult of step i in the reference's own operations and order.  Row 0 and every row with sigma_next < 1e-14 get
    (m3, m4) = (1, 0): the reference's first-order shortcut (sampling.py:433-435), which the kernels read as "do not touch old"; the last
    row of LegacyDDPMDiscretization comes out as (0, -1, 1, 0), i.e. x' = d0.
    Computed in CPU fp32 whatever device `sigmas` lives on, and uploaded by the caller: graph, eager and fresh samplers share its bits."""
    sig = sigmas.detach().to("cpu", torch.float32)
    one = DPMPP2MSampler.__new__(DPMPP2MSampler)
    rows = []
    for i in range(sig.numel() - 1):
        s, sn = sig[i].reshape(1), sig[i + 1].reshape(1)
        prev = None if i == 0 or float(sn) < 1e-14 else sig[i - 1].reshape(1)
        m = one.get_mult(*one.get_variables(s, sn, prev), prev)
        rows.append(torch.cat(list(m) + ([torch.ones(1), torch.zeros(1)] if prev is None else [])))
    return torch.stack(rows).contiguous()


def cfg_dpmpp2m_update(x: torch.Tensor, eps: torch.Tensor, old: Optional[torch.Tensor], sigma: torch.Tensor, mult: torch.Tensor, scale: float,
                       scale_im: Optional[float] = None, fused: bool = True):
    """One fused tail of a CFG DPM++ 2M step with EpsScaling -> (x', d0): den_b = x - sigma eps_b, d0 = the guider's combine as in
    cfg_euler_update, dd = d0 if m4 == 0 else m3 d0 - m4 old, x' = m1 x - m2 dd; mult = one row of dpmpp2m_multipliers, `old` = the d0 the
    previous step returned (not read when m4 == 0: None is fine there).  fused=False: the same chain in plain torch, in the kernels' order."""
    cfg_branch_count(x, eps, scale_im)
    if fused and x.is_cuda:
        from . import ops
        return ops.cfg_dpmpp2m_step(x, eps, torch.empty_like(x) if old is None else old, sigma, mult, scale, scale_im)
    d0 = cfg_combine(x, eps, sigma, scale, scale_im)
    m1, m2, m3, m4 = mult.reshape(4).unbind()
    dd = d0 if float(m4) == 0.0 else m3 * d0 - m4 * old
    return m1 * x - m2 * dd, d0


def dpmpp2m_cout_table(step_tab: torch.Tensor, sigmas: torch.Tensor, denoiser: "DiscreteDenoiser", grid: Optional[bool] = None) -> torch.Tensor:
    """The table the DPM++ 2M tail takes in place of step_tab [n, 4] = (sigma_i, sigma_next, c_in(q_i), 0): the tail reads column 0 for
    c_out ALONE (everything else comes from dpmpp2m_multipliers, built from the schedule's own sigmas), so column 0 becomes q_i =
    denoiser.possibly_quantize_sigma(sigma_i) and columns 1..3 stay.  On a schedule that lies on the denoiser's grid (`grid`; None: asked
    of on_grid) q_i is sigma_i and the result is `step_tab` ITSELF: the same object, the same launch."""
    if on_grid(sigmas, denoiser) if grid is None else grid:
        return step_tab
    tab = step_tab.clone()
    tab[:, 0] = denoiser.possibly_quantize_sigma(sigmas[:-1].to(denoiser.sigmas.device)).to(tab.device, tab.dtype)
    return tab.contiguous()


def fused_cfg_dpmpp2m_step(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, old: Optional[torch.Tensor], sigma: torch.Tensor,
                           mult: torch.Tensor, guider, fused: bool = True, sigma_q: Optional[torch.Tensor] = None):
    """ONE step of DPMPP2MSampler.sampler_step (sampling.py:413-445) in the form the sampling job launches it: fused_cfg_euler_step with the
    tail replaced -- x' , d0 = cfg_dpmpp2m_update(x, eps, old, sigma, mult): cd360_cfg_dpmpp2m_step_f32.  `mult` = row i of
    dpmpp2m_multipliers(sigmas) for sigma = sigmas[i]; `old` = the d0 step i - 1 returned.  Returns (x', d0).
    `sigma_q`: the tail's only scalar is c_out's, the SNAPPED sigma; off the denoiser's grid the caller passes it (a device tensor holding
    possibly_quantize_sigma(sigma): nothing is read back), on the grid it is `sigma`."""
    scale, scale_im = guider_scales(guider)
    eps = cfg_eps(denoiser, network, x, sigma, guider.branches)
    return cfg_dpmpp2m_update(x, eps.contiguous(), old, (sigma if sigma_q is None else sigma_q).reshape(1), mult, scale, scale_im, fused=fused)


# ----------------------------------------------------------------------------------------------- ancestral Euler
def get_ancestral_step(sigma_from, sigma_to, eta=1.0):
    """(sigma_down, sigma_up) of one ancestral step, the reference's expression in the reference's operation order (sampling_utils.py:27-36).
    eta = 0: (sigma_to, 0) with a zero TENSOR where the reference hands back the Python float 0.0 that its own append_dims then rejects."""
    if not eta:
        return sigma_to, torch.zeros_like(sigma_to)
    sigma_up = torch.minimum(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


def snap_c_in(denoiser: "DiscreteDenoiser", grid: torch.Tensor, s: torch.Tensor):
    """(c_in(sq), sq) on the host, sq = s snapped to `grid` (the denoiser's sigmas in CPU fp32) as DiscreteDenoiser.possibly_quantize_sigma
    snaps it, c_in the denoiser's own scaling of it: what the table builders below put into columns 2 and 3."""
    sq = grid[(s - grid[:, None]).abs().argmin(dim=0).view(s.shape)]
    return denoiser.scaling(sq)[2], sq


def seed_words(seed: int) -> int:
    """Any Python int -> the int64 whose 64 bits are the seed's low 64 bits (the device buffer's dtype; the Philox key is its two halves)."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s - (1 << 64) if s >= (1 << 63) else s


class DeviceNoise:
    """The three device buffers that name one draw of the library's generator (include/cd360_stochastic.h): seed int64[1], streams
    int32[bs] or None (stream 0 for every row), step int32[1].  A captured step reads all three on the device."""

    def __init__(self, seed: torch.Tensor, streams: Optional[torch.Tensor], step: torch.Tensor):
        self.seed, self.streams, self.step = seed, streams, step

    def draw(self, x: torch.Tensor) -> torch.Tensor:
        from . import ops
        return ops.sampler_noise(self.seed, self.streams, self.step, x.shape[0], x.shape[2], x.shape[3])


def seeded_noise(sampler, x: torch.Tensor, step: int) -> torch.Tensor:
    """The seed=<int> noise_sampler of the sampler classes: one draw of the library's generator under `sampler.seed`, stream 0 and the step
    word `step`, which the caller counts by its own rule (see the class docstrings); the DeviceNoise is kept on `sampler._noise` per device."""
    if not x.is_cuda:
        from ._lib import Cd360Error
        raise Cd360Error(f"the seeded noise of {type(sampler).__name__} is drawn by a HIP kernel; got a CPU tensor (seed=None draws torch.randn_like)")
    if sampler._noise is None or sampler._noise.seed.device != x.device:
        sampler._noise = DeviceNoise(torch.tensor([seed_words(sampler.seed)], dtype=torch.int64, device=x.device), None,
                                     torch.zeros(1, dtype=torch.int32, device=x.device))
    sampler._noise.step.fill_(step)
    return sampler._noise.draw(x)


# ----------------------------------------------------------------------------------------------- masked sampling (include/edit/cd360_edit.h)
def masked_blend(x: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, sigma_next: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """The end of a masked sampling step, in plain torch (CPU and GPU): the region to keep (mask 0) is replaced by the known latent at the
    step's new noise level,

        kn = known + noise * sigma_next   where sigma_next > 0, else known
        x' = mask * x + (1 - mask) * kn

    one fp32 rounding per operation, in the order cd360_mask_blend_f32 takes them.  x, known, noise [N, 4, H, W]; mask [N or 1, 1, H, W],
    1 = generate; sigma_next [N], [1] or 0-d."""
    s = append_dims(sigma_next.reshape(-1), x.ndim)
    kn = torch.where(s > 0.0, known + noise * s, known)
    return mask * x + (1.0 - mask) * kn


def check_edit_args(x_shape, known, mask) -> None:
    """What every sampler asks of (known latent, mask): both or neither; known shaped like the latent [N, 4, H, W], mask [N or 1, 1, H, W],
    both fp32.  `x_shape`: the latent or its shape."""
    shape = tuple(getattr(x_shape, "shape", x_shape))
    if (known is None) != (mask is None):
        raise ValueError("a mask needs the known latent it keeps (init_im / known) and the reverse: give both or neither")
    if known is None:
        return
    if tuple(known.shape) != shape or known.dtype != torch.float32:
        raise ValueError(f"the known latent must be fp32 of the latent's shape {shape}, got {known.dtype} {tuple(known.shape)}")
    if mask.ndim != 4 or tuple(mask.shape) not in ((shape[0], 1) + shape[2:], (1, 1) + shape[2:]) or mask.dtype != torch.float32:
        raise ValueError(f"the mask must be fp32 [{shape[0]} or 1, 1, {shape[2]}, {shape[3]}] at latent resolution (1 = generate), got "
                         f"{mask.dtype} {tuple(mask.shape)}")


def seeded_edit_noise(sampler, x: torch.Tensor, step: int) -> torch.Tensor:
    """The seed=<int> noise of a masked step of the sampler classes: ops.edit_noise (counter domain 3) under `sampler.seed`, stream 0 and the
    step's index; the buffers are kept on `sampler._edit_noise` per device.  GPU tensors only, as seeded_noise."""
    from . import ops
    if not x.is_cuda:
        from ._lib import Cd360Error
        raise Cd360Error(f"the seeded noise of {type(sampler).__name__} is drawn by a HIP kernel; got a CPU tensor (seed=None draws torch.randn_like)")
    held = getattr(sampler, "_edit_noise", None)
    if held is None or held[0].device != x.device:
        held = sampler._edit_noise = (torch.tensor([seed_words(sampler.seed)], dtype=torch.int64, device=x.device),
                                      torch.zeros(1, dtype=torch.int32, device=x.device))
    held[1].fill_(step)
    return ops.edit_noise(held[0], None, held[1], x.shape[0], x.shape[2], x.shape[3])


class EulerAncestralSampler(BaseDiffusionSampler):
    """Ancestral Euler: x_e = x + (x - denoised) / sigma (sigma_down - sigma), then x' = x_e + noise s_noise sigma_up where sigma_next > 0
    (sampling.py:236-273, 340-347).  One network evaluation per step, like EulerEDMSampler; stochastic.

    The reference's class does not run in its own fork as written: BaseDiffusionSampler.denoise returns (denoised, rgb_list) and sampler_step
    uses that tuple as a tensor, __call__ returns x alone where DiffusionEngine.sample unpacks two values, and eta = 0 hands the Python
    float 0.0 to append_dims.  Here `denoise` is unpacked -- the arithmetic is the reference's, operation by operation --, the rgb_list of
    the last denoise call is kept on the instance, __call__ returns (x, rgb_list), and eta = 0 is served as plain Euler (no noise drawn).

    `noise_sampler` as in the reference: with seed=None it is torch.randn_like.  With seed=<int> it is the library's counter-based generator
    (cd360_sampler_noise_f32: Philox4x32-10 + Box-Muller, stream 0, step = the number of draws since __call__ began), which is what
    cd360.job.Sampler(solver="euler_a", seed=...) draws inside its captured step: GPU tensors only."""

    def __init__(self, eta=1.0, s_noise=1.0, discretization_config=None, num_steps: Optional[int] = None, guider_config=None,
                 verbose: bool = False, device: str = "cuda", seed: Optional[int] = None):
        super().__init__(discretization_config, num_steps, guider_config, verbose, device)
        self.eta, self.s_noise = eta, s_noise
        self.rgb_list = None
        self.seed, self._draws, self._noise = seed, 0, None
        self.noise_sampler = (lambda x: torch.randn_like(x)) if seed is None else self._seeded_noise

    def _seeded_noise(self, x):
        z = seeded_noise(self, x, self._draws)
        self._draws += 1
        return z

    def euler_step(self, x, d, dt):
        return x + dt * d

    def ancestral_euler_step(self, x, denoised, sigma, sigma_down):
        d = (x - denoised) / append_dims(sigma, x.ndim)
        dt = append_dims(sigma_down - sigma, x.ndim)
        return self.euler_step(x, d, dt)

    def ancestral_step(self, x, sigma, next_sigma, sigma_up):
        if not self.eta:  # plain Euler: nothing drawn
            return x
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0, x + self.noise_sampler(x) * self.s_noise * append_dims(sigma_up, x.ndim), x)

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None):
        sigma_down, sigma_up = get_ancestral_step(sigma, next_sigma, eta=self.eta)
        denoised, self.rgb_list = self.denoise(x, denoiser, sigma, cond, uc)
        x = self.ancestral_euler_step(x, denoised, sigma, sigma_down)
        return self.ancestral_step(x, sigma, next_sigma, sigma_up)

    def __call__(self, denoiser: Callable, x, cond: Dict, uc=None, num_steps=None, **kwargs):
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        self._draws = 0
        for i in range(num_sigmas - 1):
            x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc)
        return x, self.rgb_list

    forward = __call__


def euler_ancestral_table(sigmas: torch.Tensor, eta: float = 1.0, s_noise: float = 1.0) -> torch.Tensor:
    """The per-schedule table of EulerAncestralSampler: sigmas [n + 1] (the discretisation's output, last = 0) -> [n, 4] fp32 rows
    (sigma_down, sigma_up, s_noise, 0), row i = get_ancestral_step(sigmas[i], sigmas[i + 1], eta).  The last row comes out as (0, 0): no
    noise where sigma_next = 0 (sampling.py:251-255); eta = 0 gives (sigma_next, 0) in every row: plain Euler.
    Computed in CPU fp32 whatever device `sigmas` lives on, and uploaded by the caller: graph, eager and fresh samplers share its bits."""
    sig = sigmas.detach().to("cpu", torch.float32)
    down, up = get_ancestral_step(sig[:-1], sig[1:], eta=eta)
    return torch.stack([down, up, torch.full_like(down, float(s_noise)), torch.zeros_like(down)], 1).contiguous()


def ancestral_finish(x: torch.Tensor, anc_row: torch.Tensor, noise, fused: bool, kernel: Callable, plain: Callable) -> torch.Tensor:
    """End an update x_n with the ancestral noise of (sigma_down, sigma_up, s_noise, 0) = anc_row: x_n if sigma_up == 0 else x_n + (z * s_noise)
    * sigma_up, for every form of `noise`.  `kernel(ops, anc, n)` launches the solver's fused tail on a 4-element row and a DeviceNoise;
    `plain(sigma_down)` is its update in plain torch without the noise.  A DeviceNoise, fused: ONE launch that draws z itself.  A tensor z
    (a caller's own draw), fused: the kernel's sigma_up = 0 form on a throw-away DeviceNoise, then z added by torch in the kernel's order.
    Otherwise plain torch; None is fine where sigma_up == 0."""
    if fused and x.is_cuda:
        from . import ops
        if isinstance(noise, DeviceNoise):  # (nothing read back: this is the call a captured un-staged step makes)
            return kernel(ops, anc_row.reshape(4), noise)
    sd, su, s_noise, _ = anc_row.reshape(4).unbind()
    noisy = float(su) != 0.0
    if noisy and noise is None:
        raise ValueError("sigma_up != 0: the step needs `noise` (a DeviceNoise or a tensor shaped like x)")
    if fused and x.is_cuda:
        dry = DeviceNoise(torch.zeros(1, dtype=torch.int64, device=x.device), None, torch.zeros(1, dtype=torch.int32, device=x.device))
        x_n = kernel(ops, torch.stack([sd, torch.zeros_like(su), s_noise, torch.zeros_like(su)]), dry)
        return x_n + (noise * s_noise) * su if noisy else x_n
    x_n = plain(sd)
    if not noisy:
        return x_n
    z = noise.draw(x) if isinstance(noise, DeviceNoise) else noise
    return x_n + (z * s_noise) * su


def cfg_euler_ancestral_update(x: torch.Tensor, eps: torch.Tensor, sigma: torch.Tensor, anc_row: torch.Tensor, scale: float,
                               scale_im: Optional[float] = None, noise=None, fused: bool = True) -> torch.Tensor:
    """One fused tail of a CFG ancestral Euler step with EpsScaling: den_b = x - sigma eps_b, d0 = the guider's combine as in
    cfg_euler_update, x_e = x + (x - d0) / sigma * (sigma_down - sigma), x' = x_e if sigma_up == 0 else x_e + (z * s_noise) * sigma_up, with
    (sigma_down, sigma_up, s_noise, 0) = anc_row, one row of euler_ancestral_table.  `noise`: a DeviceNoise -- fused: ONE kernel that draws z
    itself (cd360_cfg_euler_ancestral_step_f32) -- or a tensor z shaped like x (a caller's own draw): the kernel then computes x_e (its
    sigma_up = 0 form) and the given z is added by torch in the kernel's order; not needed when sigma_up == 0.
    fused=False: the same chain in plain torch, in the kernel's order."""
    cfg_branch_count(x, eps, scale_im)
    return ancestral_finish(x, anc_row, noise, fused,
                            lambda ops, anc, n: ops.cfg_euler_ancestral_step(x, eps, sigma, anc, n.seed, n.streams, n.step, scale, scale_im),
                            lambda sd: x + (x - cfg_combine(x, eps, sigma, scale, scale_im)) / sigma * (sd - sigma))


def fused_cfg_euler_ancestral_step(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, sigma: torch.Tensor, anc_row: torch.Tensor,
                                   guider, noise=None, fused: bool = True) -> torch.Tensor:
    """ONE step of EulerAncestralSampler.sampler_step (sampling.py:340-347) in the form the sampling job launches it: fused_cfg_euler_step
    with the tail replaced -- x' = cfg_euler_ancestral_update(x, eps, sigma, anc_row, noise=noise).  `anc_row` = row i of
    euler_ancestral_table(sigmas, eta, s_noise) for sigma = sigmas[i]; `noise` as cfg_euler_ancestral_update takes it."""
    scale, scale_im = guider_scales(guider)
    eps = cfg_eps(denoiser, network, x, sigma, guider.branches)
    return cfg_euler_ancestral_update(x, eps.contiguous(), sigma.reshape(1), anc_row, scale, scale_im, noise=noise, fused=fused)


# ----------------------------------------------------------------------------------------------- EDM with churn, Heun
def edm_tables(sigmas: torch.Tensor, denoiser: "DiscreteDenoiser", s_churn: float = 0.0, s_tmin: float = 0.0, s_tmax: float = float("inf"),
               s_noise: float = 1.0):
    """The per-schedule tables of the EDM family (include/cd360_edm.h): sigmas [n + 1] (the discretisation's output, last = 0) -> three
    [n, 4] fp32 tables, row i in the reference's own expressions (sampling.py:97-100, 120-124):

        edm_tab    (sigma_hat, sigma_next, c_in(sq), sq)            sq = denoiser.possibly_quantize_sigma(sigma_hat): c_in / c_out / the
                                                                    time-embedding row come from it, to_d and dt from sigma_hat
        corr_tab   (sigma_next, sigma_next, c_in(sq'), sq')         sq' = q(sigma_next): the corrector's evaluation (Heun)
        churn_tab  (gamma, noise_std, s_noise, 0)                   gamma = min(s_churn / n, 2**0.5 - 1) where s_tmin <= sigma_i <= s_tmax, else 0;
                                                                    sigma_hat = sigma_i * (gamma + 1.0); noise_std = (sigma_hat**2 - sigma_i**2) ** 0.5

    gamma = 0 rows hold noise_std = 0 and sigma_hat = sigma_i exactly.  Computed in CPU fp32 whatever device `sigmas` and the denoiser live
    on, and uploaded by the caller: graph, eager and fresh samplers share its bits."""
    sig = sigmas.detach().to("cpu", torch.float32)
    grid = denoiser.sigmas.detach().to("cpu", torch.float32)
    n = sig.numel() - 1

    edm, corr, churn = [], [], []
    for i in range(n):
        s, sn = sig[i].reshape(1), sig[i + 1].reshape(1)
        gamma = min(s_churn / n, 2 ** 0.5 - 1) if s_tmin <= sig[i] <= s_tmax else 0.0
        s_hat = s * (gamma + 1.0)
        std = (s_hat ** 2 - s ** 2) ** 0.5 if gamma > 0 else torch.zeros(1)
        c_in, sq = snap_c_in(denoiser, grid, s_hat)
        c_in_n, sq_n = snap_c_in(denoiser, grid, sn)
        edm.append(torch.cat([s_hat, sn, c_in, sq]))
        corr.append(torch.cat([sn, sn, c_in_n, sq_n]))
        churn.append(torch.cat([torch.full((1,), float(gamma)), std, torch.full((1,), float(s_noise)), torch.zeros(1)]))
    return torch.stack(edm).contiguous(), torch.stack(corr).contiguous(), torch.stack(churn).contiguous()


def edm_churn(x: torch.Tensor, churn: torch.Tensor, noise=None, fused: bool = True) -> torch.Tensor:
    """The churn in front of an EDM step: x_hat = x + (z * s_noise) * noise_std, x itself where noise_std == 0.  `noise`: a DeviceNoise --
    fused: ONE kernel that draws z itself (cd360_edm_churn_f32) on a copy of x; `churn` is then the whole churn_tab [n, 4], whose row the
    kernel picks through noise.step on the device (nothing is read back: the call a captured un-staged step makes) -- or a tensor z shaped
    like x (a caller's own draw) with `churn` = one row (gamma, noise_std, s_noise, 0), added by torch in the kernel's order; not needed
    when noise_std == 0.  churn=None: a schedule without churn, x itself."""
    if churn is None:
        return x
    if fused and x.is_cuda and isinstance(noise, DeviceNoise):
        from . import ops
        return ops.edm_churn(x.clone(), churn.reshape(-1, 4), noise.step, noise.seed, noise.streams)
    _, std, s_noise, _ = churn.reshape(4).unbind()
    if float(std) == 0.0:
        return x
    if noise is None:
        raise ValueError("noise_std != 0: the step needs `noise` (a DeviceNoise or a tensor shaped like x)")
    z = noise.draw(x) if isinstance(noise, DeviceNoise) else noise
    return x + (z * s_noise) * std


def cfg_edm_predict(x: torch.Tensor, eps: torch.Tensor, edm_row: torch.Tensor, scale: float, scale_im: Optional[float] = None,
                    fused: bool = True, want_dir: bool = True):
    """The predictor tail of an EDM step with EpsScaling -> (x_e, d): den_b = x - sq eps_b, d0 = the guider's combine as in cfg_euler_update,
    d = (x - d0) / sigma_hat, x_e = x + d * (sigma_next - sigma_hat), with (sigma_hat, sigma_next, c_in, sq) = edm_row, one row of
    edm_tables' first table (cd360_cfg_edm_predict_f32).  want_dir=False: d is None (the churned Euler tail).  fused=False: the same chain
    in plain torch, in the kernel's order."""
    cfg_branch_count(x, eps, scale_im)
    if fused and x.is_cuda:
        from . import ops
        return ops.cfg_edm_predict(x, eps, edm_row.reshape(4), scale, scale_im, want_dir=want_dir)
    sh, sn, _, sq = edm_row.reshape(4).unbind()
    d = (x - cfg_combine(x, eps, sq, scale, scale_im)) / sh
    return x + d * (sn - sh), (d if want_dir else None)


def cfg_edm_correct(x: torch.Tensor, xe: torch.Tensor, d: torch.Tensor, eps2: torch.Tensor, edm_row: torch.Tensor, corr_row: torch.Tensor,
                    scale: float, scale_im: Optional[float] = None, fused: bool = True) -> torch.Tensor:
    """The Heun corrector tail -> x': den_b = x_e - sq' eps2_b, d0' = the guider's combine, d_new = (x_e - d0') / sigma_next, d' = (d + d_new)
    / 2.0, x' = x + d' * (sigma_next - sigma_hat); x_e where sigma_next is not > 0 (eps2 and d are then not read: None is fine).  x = the
    latent the predictor read, (x_e, d) its outputs, eps2 = the network at (x_e, sigma_next), sq' = column 3 of corr_row
    (cd360_cfg_edm_correct_f32).  fused=False: the same chain in plain torch, in the kernel's order."""
    sh, sn = edm_row.reshape(4)[0], edm_row.reshape(4)[1]
    if fused and x.is_cuda:
        from . import ops
        cfg_branch_count(x, eps2, scale_im)
        return ops.cfg_edm_correct(x, xe, d, eps2, edm_row.reshape(4), corr_row.reshape(4), scale, scale_im)
    if not float(sn) > 0.0:
        return xe.clone()
    cfg_branch_count(x, eps2, scale_im)
    d_new = (xe - cfg_combine(xe, eps2, corr_row.reshape(4)[3], scale, scale_im)) / sn
    return x + (d + d_new) / 2.0 * (sn - sh)


def edm_head(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, edm_row: torch.Tensor, churn: torch.Tensor, guider, noise, fused: bool,
             want_dir: bool = True):
    """What the Euler and the Heun step of the EDM family begin with: churn, the network at q(sigma_hat), the predictor tail -> (x_hat, x_e, d);
    d is None for want_dir=False."""
    scale, scale_im = guider_scales(guider)
    x_hat = edm_churn(x, churn, noise, fused=fused)
    eps = cfg_eps(denoiser, network, x_hat, edm_row.reshape(4)[0], guider.branches)
    return (x_hat,) + cfg_edm_predict(x_hat, eps.contiguous(), edm_row, scale, scale_im, fused=fused, want_dir=want_dir)


def fused_cfg_edm_euler_step(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, edm_row: torch.Tensor, churn: torch.Tensor, guider,
                             noise=None, fused: bool = True) -> torch.Tensor:
    """ONE step of EulerEDMSampler.sampler_step with churn (sampling.py:96-110) in the form the sampling job launches it:

        x_hat = edm_churn(x, churn, noise)                 cd360_edm_churn_f32, in front of the network
        eps   = network(c_in(sq) [x_hat] * B, idx(sq))     DiscreteDenoiser.network_inputs snaps sigma_hat ON the device
        x'    = cfg_edm_predict(x_hat, eps, edm_row)[0]    cd360_cfg_edm_predict_f32: c_out at sq, to_d and dt at sigma_hat

    `edm_row` = row i of edm_tables(...)[0]; `churn` and `noise` as edm_churn takes them."""
    return edm_head(denoiser, network, x, edm_row, churn, guider, noise, fused, want_dir=False)[1]


def fused_cfg_heun_step(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, edm_row: torch.Tensor, corr_row: torch.Tensor,
                        churn: torch.Tensor, guider, noise=None, fused: bool = True, last: Optional[bool] = None) -> torch.Tensor:
    """ONE step of HeunEDMSampler.sampler_step (sampling.py:96-110, 321-337) in the form the sampling job launches it:
    fused_cfg_edm_euler_step keeping d, then -- unless `last` -- a second network evaluation at (x_e, sigma_next) and
    cfg_edm_correct(x_hat, x_e, d, eps2, edm_row, corr_row): cd360_cfg_edm_correct_f32.  `last`: the host-side skip of the reference
    (sigma_next < 1e-14); None reads it from edm_row (one read-back: a captured step passes the flag)."""
    scale, scale_im = guider_scales(guider)
    x_hat, xe, d = edm_head(denoiser, network, x, edm_row, churn, guider, noise, fused)
    if last is None:
        last = float(edm_row.reshape(4)[1]) < 1e-14
    if last:
        return xe
    eps2 = cfg_eps(denoiser, network, xe, corr_row.reshape(4)[0], guider.branches)
    return cfg_edm_correct(x_hat, xe, d, eps2.contiguous(), edm_row, corr_row, scale, scale_im, fused=fused)


# ----------------------------------------------------------------------------------------------- DPM++ 2S ancestral
class DPMPP2SAncestralSampler(EulerAncestralSampler):
    """DPM-Solver++(2S) with ancestral noise (sampling.py:350-387): the step to sigma_down is taken through a SECOND network evaluation at
    (x2, to_sigma(s)), s the midpoint of sigma and sigma_down in -log sigma -- x2 = m1 x - m2 denoised, x' = m3 x - m4 denoised2 --, then the
    ancestral noise s_noise sigma_up is added where sigma_next > 0.  Where sigma_down = 0 (the last step; for eta > 1 interior steps as well)
    the step is the ancestral Euler step and costs one evaluation: n steps cost 2n - (such steps) evaluations.  to_sigma(s) is off the
    denoiser's grid; it goes to the denoiser un-snapped and the denoiser snaps it.  Constructor, `noise_sampler` and `seed` as in
    EulerAncestralSampler: seed=None draws torch.randn_like; seed=<int> the library's generator with step word = the number of draws since
    __call__ began -- one per step, the last included, as the reference's torch.where evaluates its noisy branch everywhere.

    The reference's class does not run in its own fork as written, for the reasons EulerAncestralSampler's docstring names: `denoise` returns
    (denoised, rgb_list) and sampler_step uses that tuple as a tensor, __call__ returns x alone, and eta = 0 hands the Python float 0.0 to
    append_dims.  Here `denoise` is unpacked -- the arithmetic is the reference's, operation by operation, get_variables / get_mult included
    --, the rgb_list of the last denoise call is kept on the instance, __call__ returns (x, rgb_list), and eta = 0 is served as the
    deterministic DPM++ 2S (sigma_down = sigma_next, nothing drawn)."""

    def get_variables(self, sigma, sigma_down):
        t, t_next = [to_neg_log_sigma(s) for s in (sigma, sigma_down)]
        h = t_next - t
        s = t + 0.5 * h
        return h, s, t, t_next

    def get_mult(self, h, s, t, t_next):
        mult1 = to_sigma(s) / to_sigma(t)
        mult2 = (-0.5 * h).expm1()
        mult3 = to_sigma(t_next) / to_sigma(t)
        mult4 = (-h).expm1()
        return mult1, mult2, mult3, mult4

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, **kwargs):
        sigma_down, sigma_up = get_ancestral_step(sigma, next_sigma, eta=self.eta)
        denoised, self.rgb_list = self.denoise(x, denoiser, sigma, cond, uc)
        x_euler = self.ancestral_euler_step(x, denoised, sigma, sigma_down)
        if torch.sum(sigma_down) < 1e-14:  # save a network evaluation if all noise levels are 0
            x = x_euler
        else:
            h, s, t, t_next = self.get_variables(sigma, sigma_down)
            mult = [append_dims(m, x.ndim) for m in self.get_mult(h, s, t, t_next)]
            x2 = mult[0] * x - mult[1] * denoised
            denoised2, self.rgb_list = self.denoise(x2, denoiser, to_sigma(s), cond, uc)
            x_dpmpp2s = mult[2] * x - mult[3] * denoised2
            x = torch.where(append_dims(sigma_down, x.ndim) > 0.0, x_dpmpp2s, x_euler)  # apply correction if noise level is not 0
        return self.ancestral_step(x, sigma, next_sigma, sigma_up)


def dpmpp2s_tables(sigmas: torch.Tensor, denoiser: "DiscreteDenoiser", eta: float = 1.0, s_noise: float = 1.0):
    """The per-schedule tables of DPMPP2SAncestralSampler (include/cd360_highorder.h): sigmas [n + 1] (the discretisation's output, last = 0)
    -> three [n, 4] fp32 tables, row i in the reference's own expressions and order (sampling.py:351-363, sampling_utils.py:27-36):

        anc_tab     (sigma_down, sigma_up, s_noise, 0)                  euler_ancestral_table as it is
        mid_tab     (sigma_mid, sigma_down, c_in(sq_mid), sq_mid)       sigma_mid = to_sigma(s), s = t + 0.5 h; sq_mid =
                                                                        denoiser.possibly_quantize_sigma(sigma_mid): the second evaluation's
                                                                        c_in / c_out / time-embedding row (edm_tables' corr_tab layout)
        mult2s_tab  (mult1, mult2, mult3, mult4)                        get_mult(*get_variables(sigma, sigma_down))

    A row with sigma_down < 1e-14 takes ONE evaluation (sampling.py:370-372: the ancestral Euler step) and reads neither mid_tab nor mult2s_tab;
    it holds finite filler -- mid = the step's own (sigma, sigma_next, c_in, sigma), mults = 0 -- so a capture warm-up on it stays finite.
    Computed in CPU fp32 whatever device `sigmas` and the denoiser live on, and uploaded by the caller: graph, eager and fresh samplers share its
    bits."""
    sig = sigmas.detach().to("cpu", torch.float32)
    grid = denoiser.sigmas.detach().to("cpu", torch.float32)
    anc = euler_ancestral_table(sig, eta, s_noise)
    one = DPMPP2SAncestralSampler.__new__(DPMPP2SAncestralSampler)

    mid, mult = [], []
    for i in range(sig.numel() - 1):
        s, sn, sd = sig[i].reshape(1), sig[i + 1].reshape(1), anc[i, 0].reshape(1)
        if float(sd) < 1e-14:
            c_in, sq = snap_c_in(denoiser, grid, s)
            mid.append(torch.cat([s, sn, c_in, sq]))
            mult.append(torch.zeros(4))
            continue
        h, sm, t, t_next = one.get_variables(s, sd)
        s_mid = to_sigma(sm)
        c_in, sq = snap_c_in(denoiser, grid, s_mid)
        mid.append(torch.cat([s_mid, sd, c_in, sq]))
        mult.append(torch.cat(list(one.get_mult(h, sm, t, t_next))))
    return anc, torch.stack(mid).contiguous(), torch.stack(mult).contiguous()


def dpmpp2s_single_rows(anc_tab: torch.Tensor):
    """The rows of a DPM++ 2S schedule that take one evaluation (sigma_down < 1e-14: sampling.py:370), as a host list of bools."""
    return [float(v) < 1e-14 for v in anc_tab.detach().to("cpu")[:, 0]]


def cfg_dpmpp2s_mid(x: torch.Tensor, eps: torch.Tensor, sigma: torch.Tensor, mult: torch.Tensor, scale: float, scale_im: Optional[float] = None,
                    fused: bool = True) -> torch.Tensor:
    """The midpoint tail of a CFG DPM++ 2S step with EpsScaling -> x2 = m1 x - m2 d0: den_b = x - sigma eps_b, d0 = the guider's combine as in
    cfg_euler_update, (m1, m2, ., .) = mult, one row of dpmpp2s_tables' third table (cd360_cfg_dpmpp2s_mid_f32).  fused=False: the same chain
    in plain torch, in the kernel's order."""
    cfg_branch_count(x, eps, scale_im)
    if fused and x.is_cuda:
        from . import ops
        return ops.cfg_dpmpp2s_mid(x, eps, sigma, mult.reshape(4), scale, scale_im)
    m1, m2 = mult.reshape(4)[0], mult.reshape(4)[1]
    return m1 * x - m2 * cfg_combine(x, eps, sigma, scale, scale_im)


def cfg_dpmpp2s_update(x: torch.Tensor, x2: torch.Tensor, eps2: torch.Tensor, mid_row: torch.Tensor, mult: torch.Tensor, anc_row: torch.Tensor,
                       scale: float, scale_im: Optional[float] = None, noise=None, fused: bool = True) -> torch.Tensor:
    """The second tail of a CFG DPM++ 2S step -> x': den_b = x2 - sq_mid eps2_b, d0' = the guider's combine, x_n = m3 x - m4 d0', x' = x_n if
    sigma_up == 0 else x_n + (z * s_noise) * sigma_up; x = the latent the midpoint read, x2 its output, eps2 = the network at (x2, sigma_mid),
    sq_mid = column 3 of mid_row, (., ., m3, m4) = mult, (., sigma_up, s_noise, .) = anc_row (cd360_cfg_dpmpp2s_step_f32).  `noise` as
    cfg_euler_ancestral_update takes it: a DeviceNoise -- fused: ONE kernel that draws z itself -- or a tensor z shaped like x, added by torch
    in the kernel's order behind the kernel's sigma_up = 0 form.  fused=False: the same chain in plain torch, in the kernel's order."""
    cfg_branch_count(x, eps2, scale_im)
    m = mult.reshape(4)
    return ancestral_finish(x, anc_row, noise, fused,
                            lambda ops, anc, n: ops.cfg_dpmpp2s_step(x, x2, eps2, mid_row.reshape(4), m, anc, n.seed, n.streams, n.step, scale, scale_im),
                            lambda sd: m[2] * x - m[3] * cfg_combine(x2, eps2, mid_row.reshape(4)[3], scale, scale_im))


def fused_cfg_dpmpp2s_step(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, sigma: torch.Tensor, anc_row: torch.Tensor,
                           mid_row: torch.Tensor, mult: torch.Tensor, guider, noise=None, fused: bool = True, single: Optional[bool] = None):
    """ONE step of DPMPP2SAncestralSampler.sampler_step (sampling.py:365-387) in the form the sampling job launches it:

        eps  = network(c_in(sigma) [x] * B, idx(sigma))              the first evaluation, on the grid
        x2   = cfg_dpmpp2s_mid(x, eps, sigma, mult)                  cd360_cfg_dpmpp2s_mid_f32
        eps2 = network(c_in(sq_mid) [x2] * B, idx(sq_mid))           DiscreteDenoiser.network_inputs snaps sigma_mid ON the device
        x'   = cfg_dpmpp2s_update(x, x2, eps2, mid_row, mult, anc_row, noise)        cd360_cfg_dpmpp2s_step_f32

    `anc_row` / `mid_row` / `mult` = row i of dpmpp2s_tables(...) for sigma = sigmas[i]; `noise` as cfg_dpmpp2s_update takes it.  `single`:
    the row takes one evaluation (sigma_down < 1e-14) and is fused_cfg_euler_ancestral_step; None reads it from anc_row (one read-back: a
    captured step passes the flag)."""
    if single is None:
        single = float(anc_row.reshape(4)[0]) < 1e-14
    if single:
        return fused_cfg_euler_ancestral_step(denoiser, network, x, sigma, anc_row, guider, noise=noise, fused=fused)
    scale, scale_im = guider_scales(guider)
    eps = cfg_eps(denoiser, network, x, sigma, guider.branches)
    x2 = cfg_dpmpp2s_mid(x, eps.contiguous(), sigma.reshape(1), mult, scale, scale_im, fused=fused)
    eps2 = cfg_eps(denoiser, network, x2, mid_row.reshape(4)[0], guider.branches)
    return cfg_dpmpp2s_update(x, x2, eps2.contiguous(), mid_row, mult, anc_row, scale, scale_im, noise=noise, fused=fused)


# ----------------------------------------------------------------------------------------------- linear multistep
def lms_coefficients(sigmas: torch.Tensor, order: int = 4) -> torch.Tensor:
    """The per-schedule table of LinearMultistepSampler: sigmas [n + 1] (the discretisation's output) -> [n, 4] fp32, row i =
    linear_multistep_coeff(min(i + 1, order), sigmas, i, j) for j < min(i + 1, order) (sampling_utils.py:12-24), zero behind them; order in
    1..4.  The reference integrates the Lagrange basis polynomial over [sigma_i, sigma_(i+1)] with scipy's adaptive quadrature; its degree
    is at most 3, so the 4-point Gauss-Legendre rule used here (float64, on the fp32 sigmas) is exact and scipy is not needed.
    Computed on the host whatever device `sigmas` lives on, and uploaded by the caller: graph, eager and fresh samplers share its bits."""
    if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= 4:
        raise ValueError(f"order {order!r}: the linear multistep solver serves orders 1..4")
    t = sigmas.detach().to("cpu", torch.float32).numpy().astype(np.float64)
    nodes, weights = np.polynomial.legendre.leggauss(4)
    out = np.zeros((t.size - 1, 4), dtype=np.float32)
    for i in range(t.size - 1):
        cur = min(i + 1, order)
        half, centre = 0.5 * (t[i + 1] - t[i]), 0.5 * (t[i + 1] + t[i])
        tau = half * nodes + centre
        for j in range(cur):
            prod = np.ones_like(tau)
            for k in range(cur):
                if j != k:
                    prod = prod * ((tau - t[i - k]) / (t[i - j] - t[i - k]))
            out[i, j] = half * float(np.dot(weights, prod))
    return torch.from_numpy(out).contiguous()


class LinearMultistepSampler(BaseDiffusionSampler):
    """Adams-Bashforth over the sigma schedule (sampling.py:276-311): x' = x + sum_j c_j d_(i - j) over the last min(i + 1, order) directions
    d = to_d(x, sigma, denoised), c_j the integral of the j-th Lagrange basis polynomial of their sigmas over [sigma_i, sigma_(i+1)].  One
    network evaluation per step, deterministic.  `ds` holds at most `order` directions, the coefficients multiply them newest first, and the
    sum is formed in the reference's order (Python's sum) before it is added to x.

    The reference's class does not run in its own fork as written: it unpacks two values from a denoiser that returns four, and __call__
    returns x alone where DiffusionEngine.sample unpacks two values.  Here the denoiser's four values are unpacked -- the arithmetic is the
    reference's, operation by operation --, the rgb_list of the last denoiser call is kept on the instance, and __call__ returns (x,
    rgb_list).  The coefficients come from lms_coefficients (no scipy; exact for these polynomials) and are rounded to fp32 before they
    multiply an fp32 direction, which is what torch does with the reference's Python floats."""

    def __init__(self, order=4, discretization_config=None, num_steps: Optional[int] = None, guider_config=None, verbose: bool = False,
                 device: str = "cuda"):
        super().__init__(discretization_config, num_steps, guider_config, verbose, device)
        self.order = order
        self.rgb_list = None

    def sampler_step(self, ds, coeffs, sigma, denoiser, x, cond, uc=None, **kwargs):
        """One pass of the reference's loop body: `ds` = the list of kept directions (appended to and trimmed IN PLACE), `coeffs` = the step's
        min(i + 1, order) coefficients, newest first."""
        denoised, _, _, self.rgb_list = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc), **kwargs)
        denoised = self.guider(denoised, sigma)
        d = (x - denoised) / append_dims(sigma, x.ndim)
        ds.append(d)
        if len(ds) > self.order:
            ds.pop(0)
        return x + sum(coeff * d for coeff, d in zip(coeffs, reversed(ds)))

    def __call__(self, denoiser: Callable, x, cond: Dict, uc=None, num_steps=None, **kwargs):
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        ds = []
        table = lms_coefficients(sigmas, self.order)
        for i in range(num_sigmas - 1):
            cur_order = min(i + 1, self.order)
            x = self.sampler_step(ds, [float(table[i, j]) for j in range(cur_order)], s_in * sigmas[i], denoiser, x, cond, uc, **kwargs)
        return x, self.rgb_list

    forward = __call__


def cfg_lms_update(x: torch.Tensor, eps: torch.Tensor, ring: torch.Tensor, sigma: torch.Tensor, coef: torch.Tensor, step, scale: float,
                   scale_im: Optional[float] = None, fused: bool = True) -> torch.Tensor:
    """One fused tail of a CFG linear multistep step with EpsScaling -> x': den_b = x - sigma eps_b, d0 = the guider's combine as in
    cfg_euler_update, d = (x - d0) / sigma stored into ring[i % order] IN PLACE, acc = c_0 d, acc += c_j ring[(i - j) % order] for j = 1 ..
    min(i + 1, order) - 1, x' = x + acc; ring [order, *x.shape] fp32, coef = one row of lms_coefficients, i = `step` (an int, or -- fused: the
    device int32 the kernel reads, nothing read back -- a tensor).  Slots with j >= min(i + 1, order) are not read (cd360_cfg_lms_step_f32).
    fused=False: the same chain in plain torch, in the kernel's order."""
    cfg_branch_count(x, eps, scale_im)
    if fused and x.is_cuda:
        from . import ops
        if not isinstance(step, torch.Tensor):
            step = torch.tensor([int(step)], dtype=torch.int32, device=x.device)
        return ops.cfg_lms_step(x, eps, ring, sigma, coef.reshape(4), step, scale, scale_im)
    i, order = int(step), ring.shape[0]
    d = (x - cfg_combine(x, eps, sigma, scale, scale_im)) / sigma
    ring[i % order] = d
    c = coef.reshape(4)
    acc = c[0] * d
    for j in range(1, min(i + 1, order)):
        acc = acc + c[j] * ring[(i - j) % order]
    return x + acc


def fused_cfg_lms_step(denoiser: "DiscreteDenoiser", network: Callable, x: torch.Tensor, ring: torch.Tensor, sigma: torch.Tensor, coef: torch.Tensor,
                       step, guider, fused: bool = True) -> torch.Tensor:
    """ONE pass of LinearMultistepSampler's loop (sampling.py:294-309) in the form the sampling job launches it: fused_cfg_euler_step with the
    tail replaced -- x' = cfg_lms_update(x, eps, ring, sigma, coef, step): cd360_cfg_lms_step_f32.  `coef` = row i of
    lms_coefficients(sigmas, order) for sigma = sigmas[i], `step` = i; `ring` carries the directions between the steps of ONE image."""
    scale, scale_im = guider_scales(guider)
    eps = cfg_eps(denoiser, network, x, sigma, guider.branches)
    return cfg_lms_update(x, eps.contiguous(), ring, sigma.reshape(1), coef, step, scale, scale_im, fused=fused)
