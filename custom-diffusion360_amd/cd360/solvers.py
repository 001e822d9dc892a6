"""What each solver of cd360.job.Sampler knows and the others do not: its per-schedule table and buffers, the row it writes per step on the
un-staged route, the tail kernel that ends a staged step, its un-staged step, and whether it draws noise.  One stateless object per
solver; the state lives on the Sampler `smp` they are handed (smp.mult_tab, smp.gd, smp.anc_tab, smp.seed_buf, smp.streams_buf: the
names tests and tools read), next to the buffers every solver shares (smp.gx, smp.gi, smp._iota, smp.step_tab)."""
from __future__ import annotations

import torch

from . import ops
from . import sampler as S


class Euler:
    """EulerEDMSampler (sampling.py:85-136): sigma and sigma_next are all a step needs."""

    draws_noise = False

    def build(self, smp, x):
        pass

    def set_row(self, smp, i):
        pass

    def tail(self, smp, eps_cl):  # [c_out, CFG, to_d, Euler]
        return ops.cfg_euler_step_cl(smp.gx, eps_cl, smp.step_tab, smp.gi, smp.scale, smp.scale_im)

    def step(self, smp, unet, x, s, s_next):
        return S.fused_cfg_euler_step(smp.denoiser, unet, x, s, s_next, smp.guider)


class DPMPP2M:
    """DPMPP2MSampler (sampling.py:390-465: second order, multistep, the same one UNet evaluation per step)."""

    draws_noise = False

    def build(self, smp, x):
        """The multiplier table (host fp32, uploaded: the same bits in every sampler of a schedule), the un-staged step's 4-float row
        buffer, and gd = the previous step's denoised latent d0, shaped like gx and shared by both captured graphs.  retarget() does not
        reset gd: row 0 of the table has m4 = 0 and the kernels then never read it -- which is also why step(x, i) for i > 0 must follow
        step(., i - 1) of the same image."""
        smp.mult_tab = S.dpmpp2m_multipliers(smp.sigmas).to(x.device)
        smp.gm = smp.mult_tab[0].clone()
        smp.gd = torch.zeros_like(x)

    def set_row(self, smp, i):
        smp.gm.copy_(smp.mult_tab[i])

    def tail(self, smp, eps_cl):  # x and gd in place: [c_out, CFG, multistep update]
        return ops.cfg_dpmpp2m_step_cl(smp.gx, smp.gd, eps_cl, smp.step_tab, smp.mult_tab, smp.gi, smp.scale, smp.scale_im)

    def step(self, smp, unet, x, s, s_next):  # the kernel on the row in gm; this step's d0 moves into gd
        out, d0 = S.fused_cfg_dpmpp2m_step(smp.denoiser, unet, x, smp.gd, s, smp.gm, smp.guider)
        smp.gd.copy_(d0)
        return out


class EulerAncestral:
    """EulerAncestralSampler (sampling.py:236-273, 340-347: stochastic; smp.eta / smp.s_noise as the reference's constructor takes them)."""

    draws_noise = True

    def build(self, smp, x):
        """The (sigma_down, sigma_up, s_noise, 0) table (host fp32, uploaded: the same bits in every sampler of a schedule), the un-staged
        step's 4-float row buffer, and the generator's seed / stream-id buffers the tail kernels read on the device.  Nothing is carried
        from one step to the next."""
        dev = x.device
        smp.anc_tab = S.euler_ancestral_table(smp.sigmas, smp.eta, smp.s_noise).to(dev)
        smp.ga = smp.anc_tab[0].clone()
        smp.seed_buf = torch.tensor([S.seed_words(smp.seed)], dtype=torch.int64, device=dev)
        smp.streams_buf = torch.zeros(x.shape[0], dtype=torch.int32, device=dev)
        if smp.noise_streams is not None:
            smp.set_noise_streams(smp.noise_streams)
        smp.noise = S.DeviceNoise(smp.seed_buf, smp.streams_buf, smp.gi)

    def set_row(self, smp, i):  # (gi is the noise counter's step word on this route as well)
        smp.ga.copy_(smp.anc_tab[i])
        smp.gi.copy_(smp._iota[i:i + 1])

    def tail(self, smp, eps_cl):  # [c_out, CFG, to_d, Euler to sigma_down, + noise sigma_up]
        return ops.cfg_euler_ancestral_step_cl(smp.gx, eps_cl, smp.step_tab, smp.anc_tab, smp.gi, smp.seed_buf, smp.streams_buf, smp.scale,
                                               smp.scale_im)

    def step(self, smp, unet, x, s, s_next):  # the kernel on the row in ga and the step index in gi
        return S.fused_cfg_euler_ancestral_step(smp.denoiser, unet, x, s, smp.ga, smp.guider, noise=smp.noise)


SOLVERS = {"euler": Euler(), "dpmpp2m": DPMPP2M(), "euler_a": EulerAncestral()}
