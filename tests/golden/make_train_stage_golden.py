"""Golden vectors of the two ends of the reference's training step (sgm/modules/diffusionmodules/loss.py:140-187 with
denoiser.py:22-44, sigma_sampling.py:16-53), CPU fp32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_train_stage_golden.py

Writes tests/golden/train_stage.npz.  The reference's StandardDiffusionLossImgRef (the shipped loss_fn_config: CubicSampling over 1000
indices, DiscreteSampling over 50) and DiscreteDenoiser (the shipped denoiser_config: EpsScaling, EpsWeighting, 1000 indices) run their
own __call__.  Its random numbers come from torch's generators, whose streams nobody else can reproduce: inside the reference's loss,
sigma_sampling and denoiser modules the name `torch` is replaced by a stand-in whose rand / randint / randn / randn_like return, in call
order, the draws include/train/cd360_train.h documents (tests/train_cases.py):

    rand((B,))            u = (r0 >> 8) 2^-24                       CubicSampling
    randn_like(input)     the domain-5 normals                      the target noise
    randn(B)              off_tgt                  [level > 0]
    randint(0, 50, (B,))  r1 % 50                                   DiscreteSampling
    randn_like(input_ref) the domain-6 normals                      the loss's noising of the reference views
    randn(B)              off_ref                  [level > 0]
    randn_like(input_ref) the domain-7 normals                      the denoiser's noising of the reference views

The network is a stub that records what it is given and returns a fixed eps.  B = 3 (row 1 with drop_im = 0, applied as shared_step does,
sgm/models/diffusion.py:246), n = 2, 8 x 8, offset_noise_level 0 and 0.1, with and without a mask.  Stored: the inputs, and per case the
network's inputs (x_in, timesteps, input_ref, sigmas_ref), w and loss_l2."""
from __future__ import annotations

import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"  # MKL's reproducible code path, as tests/conftest.py sets it for the suite

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import refshim  # noqa: E402
import weights as W  # noqa: E402
import train_cases as TR  # noqa: E402
from make_golden_params import LOSS_CFG  # noqa: E402

ns = refshim.import_reference_loss()
torch.set_grad_enabled(False)
SEED, STREAMS, STEP, B, N, H = 360, (0, 5, 5), 3, 3, 2, 8
DENOISER_CFG = dict(weighting_config={"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
                    scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000,
                    discretization_config={"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"})


class ScriptedTorch:
    """`torch` for the reference's modules: the four generators hand out the queued draws, each checked against the call that asks."""

    def __init__(self, queue):
        self.queue = list(queue)

    def __getattr__(self, name):
        return getattr(torch, name)

    def _next(self, kind, shape):
        want, value = self.queue.pop(0)
        assert want == kind and tuple(value.shape) == tuple(shape), (want, kind, tuple(value.shape), tuple(shape))
        return value.clone()

    def rand(self, shape, **kw):
        return self._next("rand", shape)

    def randint(self, low, high, shape, **kw):
        v = self._next("randint", shape)
        assert low == 0 and int(v.max()) < high
        return v

    def randn(self, *shape, **kw):
        return self._next("randn", shape[0] if isinstance(shape[0], (tuple, list)) else shape)

    def randn_like(self, x, **kw):
        return self._next("randn_like", x.shape)


def main():
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    x0 = W.tensor("train.x0", (B, 4, H, H), seed=41)
    xr = W.tensor("train.xr", (B, N, 4, H, H), seed=41)
    eps = W.tensor("train.eps", (B, 4, H, H), seed=41)
    mask = (W.tensor("train.mask", (B, 1, H, H), seed=41) > -0.3).float()
    drop = torch.tensor([1.0, 0.0, 1.0])
    out = dict(x0=x0, xr=xr, eps=eps, mask=mask, drop_im=drop, seed=np.int64(SEED), streams=np.asarray(STREAMS, np.int64), step=np.int64(STEP))
    den = ns.denoiser.DiscreteDenoiser(**DENOISER_CFG)
    for tag, level in (("l0", 0.0), ("l1", 0.1)):
        r = TR.restate(np.float32, seed=SEED, streams=STREAMS, step=STEP, x0=x0.numpy(), xr=xr.numpy(), **TR.shipped(level))
        queue = [("rand", t(r["u"])), ("randn_like", t(r["z"]))] + ([("randn", t(r["rows"][:, TR.OFF_TGT]))] if level > 0 else [])
        queue += [("randint", torch.from_numpy(r["ref_sampler_idx"])), ("randn_like", t(r["z_a"]))]
        queue += ([("randn", t(r["rows"][:, TR.OFF_REF]))] if level > 0 else []) + [("randn_like", t(r["z_b"]))]
        for mtag, m in (("m", mask), ("n", None)):
            scripted = ScriptedTorch(queue)
            for mod in (ns.loss, ns.sigma_sampling, ns.denoiser):
                mod.torch = scripted
            loss_fn = ns.loss.StandardDiffusionLossImgRef(offset_noise_level=level, **LOSS_CFG)
            seen = {}

            def network(x_in, c_noise, cond, **kw):
                seen.update(x_in=x_in.clone(), timesteps=c_noise.clone(), input_ref=kw["input_ref"].clone(), sigmas_ref=kw["sigmas_ref"].clone())
                return eps, [], [], []

            real_w = den.w
            den.w = lambda sigma: seen.setdefault("w", real_w(sigma).clone())
            xr_in = drop.reshape(B, 1, 1, 1, 1) * xr + (1 - drop.reshape(B, 1, 1, 1, 1)) * torch.zeros_like(xr)  # diffusion.py:246
            loss_l2, fg, bg, rgb = loss_fn(network, den, lambda batch: {}, x0, None, xr_in, None, m, None, None, {})
            den.w = real_w
            assert not scripted.queue and fg == [] and bg == [] and rgb == []
            for mod in (ns.loss, ns.sigma_sampling, ns.denoiser):
                mod.torch = torch
            if mtag == "m":
                out.update({f"{tag}.{k}": v for k, v in seen.items()})
            out[f"{tag}.loss_l2.{mtag}"] = loss_l2
    out = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    path = os.path.join(HERE, "train_stage.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
