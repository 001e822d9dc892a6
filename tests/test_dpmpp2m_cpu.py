"""DPM++ 2M (cd360.sampler.DPMPP2MSampler, dpmpp2m_multipliers, fused_cfg_dpmpp2m_step) against golden vectors written by the REFERENCE's
DPMPP2MSampler (tests/golden/make_golden_dpmpp2m.py: a subclass that only unpacks `denoise`), the new header against the binding's second
signature table, and the job sampler's `solver` argument.  CPU only; tests/test_dpmpp2m_gpu.py holds the kernels and the captured job."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sampler_cases as SC
from test_sampler_cpu import dummy_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DISC = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
GUIDERS = {"cfg3": {"target": "sgm.modules.diffusionmodules.guiders.ScheduledCFGImgTextRef", "params": {"scale": 7.5, "scale_im": 3.5}},
           "cfg2": {"target": "sgm.modules.diffusionmodules.guiders.VanillaCFGImgRef", "params": {"scale": 7.5}}}
NEW = ("cd360_cfg_dpmpp2m_step_f32", "cd360_cfg_dpmpp2m_step_cl")


def row_network(x_in, c_noise, cond, **kw):
    """test_sampler_cpu.dummy_network plus a term that depends on the batch row: the toy network alone gives the image branch (row 1 of
    [u | ic | c], conditioned on `uc1` like row 0) the unconditional output, and cfg3 == cfg2 on it."""
    pred, a, b, rgb = dummy_network(x_in, c_noise, cond, **kw)
    row = torch.arange(x_in.shape[0], dtype=torch.float32, device=x_in.device).view(-1, 1, 1, 1)
    return pred + 0.04 * row * torch.cos(x_in), a, b, rgb


def load():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "sampler_dpmpp2m.npz")).items()}


def build(guider):
    """by dotted path through instantiate_from_config, as the YAML's sampler_config does"""
    from sgm.util import instantiate_from_config
    den = instantiate_from_config({"target": "sgm.modules.diffusionmodules.denoiser.DiscreteDenoiser", "params": {
        "num_idx": 1000, "weighting_config": {"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        "scaling_config": {"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, "discretization_config": DISC}})
    smp = instantiate_from_config({"target": "sgm.modules.diffusionmodules.sampling.DPMPP2MSampler", "params": {
        "num_steps": 50, "discretization_config": DISC, "guider_config": guider, "device": "cpu"}})
    return den, smp


def conds(g, dev="cpu"):
    return ({"crossattn": g["c_crossattn"].to(dev), "vector": g["c_vector"].to(dev)},
            {"crossattn": g["uc_crossattn"].to(dev), "vector": g["uc_vector"].to(dev)})


def close(got, want):
    return torch.allclose(got, want, atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
@pytest.mark.parametrize("steps", [12, 4])
def test_class_walks_the_reference_trajectory_with_every_intermediate(name, steps):
    """The class, built by the reference's dotted path: __call__ returns (x, rgb_list) and lands on the reference's final latent; driven
    step by step through sampler_step it reproduces every intermediate x and denoised.  Bar: the one test_sampler_cpu.py holds Euler to
    (Euler's own result differs from DPM++ 2M's by 0.15 of max 44 on this setup, so an Euler step cannot pass)."""
    g = load()
    c, uc = conds(g)
    den, smp = build(GUIDERS[name])
    from cd360.sampler import DPMPP2MSampler
    assert type(smp) is DPMPP2MSampler
    denoiser = lambda inp, s, cc: den(row_network, inp, s, cc)  # noqa: E731
    res, rgb = smp(denoiser, g["x"].clone(), c, uc=uc, num_steps=steps)
    want = g[f"{name}_{steps}"]
    print(name, steps, "final vs the reference, max abs:", float((res - want).abs().max()), "of max", float(want.abs().max()))
    assert close(res, want) and rgb is not None and rgb is smp.rgb_list
    x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(g["x"].clone(), c, uc, steps)
    assert num_sigmas == steps + 1
    old = None
    for i in range(steps):
        x, old = smp.sampler_step(old, None if i == 0 else s_in * sigmas[i - 1], s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc=ucond)
        assert close(x, g[f"{name}_{steps}_x"][i]) and close(old, g[f"{name}_{steps}_den"][i]), (name, steps, i)
    assert torch.equal(x, res)


@pytest.mark.parametrize("steps", [12, 4])
def test_multiplier_table_matches_the_reference(steps):
    """dpmpp2m_multipliers against the multipliers the reference computed per step.  Exact where the value is a decision or a limit: (m3, m4)
    = (1, 0) in the first and the last row, (m1, m2) = (0, -1) in the last (sigma_next = 0).  The rest at rtol 1e-6: a chain of four host
    vector-math calls (log, exp, expm1, division), each within one ulp across hosts (test_schedule_and_table_match_reference_bitwise)."""
    from cd360.sampler import LegacyDDPMDiscretization, dpmpp2m_multipliers
    g = load()
    tab = dpmpp2m_multipliers(LegacyDDPMDiscretization()(steps))
    want = g[f"mult_{steps}"]
    assert tab.shape == (steps, 4) == tuple(want.shape) and tab.dtype == torch.float32 and tab.device.type == "cpu" and tab.is_contiguous()
    assert tab[0, 2:].tolist() == [1.0, 0.0] and tab[-1].tolist() == [0.0, -1.0, 1.0, 0.0]
    assert want[0, 2:].tolist() == [1.0, 0.0] and want[-1].tolist() == [0.0, -1.0, 1.0, 0.0]
    assert bool((tab[1:-1, 3] > 0).all())  # the multistep rows are multistep rows
    print("multipliers vs the reference, max rel:", float(((tab - want).abs() / want.abs().clamp_min(1e-30)).max()))
    assert torch.allclose(tab, want, rtol=1e-6, atol=0)
    assert torch.isfinite(tab).all()


def run_product_steps(g, name, dev, fused, steps=12):
    """The trajectory through the product's step function (cd360.sampler.fused_cfg_dpmpp2m_step: what cd360/job.py launches per step for
    solver="dpmpp2m"), around the golden's network; returns (final x, [x_i], [d0_i])."""
    from cd360 import sampler as S
    den = S.DiscreteDenoiser().to(dev)
    guider = S.ScheduledCFGImgTextRef(7.5, 3.5) if name == "cfg3" else S.VanillaCFGImgRef(7.5)
    c, uc = conds(g, dev)
    x = g["x"].to(dev)
    _, _, cond = guider.prepare_inputs(x, x.new_ones(x.shape[0]), c, uc)
    sigmas = S.LegacyDDPMDiscretization()(steps, device=dev)
    mult = S.dpmpp2m_multipliers(sigmas).to(dev)
    x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)
    network = lambda x_in, c_noise: row_network(x_in, c_noise, cond)[0]  # noqa: E731
    old, xs, ds = None, [], []
    for i in range(steps):
        x, old = S.fused_cfg_dpmpp2m_step(den, network, x, old, sigmas[i], mult[i], guider, fused=fused)
        xs.append(x)
        ds.append(old)
    return x, xs, ds


def test_product_step_function_walks_the_reference_trajectory_for_both_guiders():
    """fused_cfg_dpmpp2m_step(fused=False) -- the plain-torch chain in the kernels' order, on the multiplier TABLE -- over 12 steps against the
    reference, every intermediate; and the two guiders' results differ (the network's three branches differ, so scale_im takes part)."""
    g = load()
    finals = {}
    for name in ("cfg3", "cfg2"):
        res, xs, ds = run_product_steps(g, name, "cpu", fused=False)
        print(name, "table-form CPU trajectory vs the reference, max abs:", float((res - g[f"{name}_12"]).abs().max()))
        assert close(res, g[f"{name}_12"])
        for i in range(12):
            assert close(xs[i], g[f"{name}_12_x"][i]) and close(ds[i], g[f"{name}_12_den"][i]), (name, i)
        finals[name] = res
    assert float((finals["cfg3"] - finals["cfg2"]).abs().max()) > 1e-2 * float(finals["cfg3"].abs().max())


def test_first_step_is_the_euler_step():
    """Row 0 is first order: m1 x - m2 d0 with m1 = sigma'/sigma, m2 = sigma'/sigma - 1 is x + (x - d0)/sigma (sigma' - sigma).  The two forms
    differ by fp32 rounding only: 1e-5 of the tensor maximum.  `old` is not needed for it."""
    import weights as W
    from cd360 import sampler as S
    x, eps = W.tensor("x", (2, 4, 8, 8), seed=3), W.tensor("eps", (6, 4, 8, 8), seed=3)
    sigmas = S.LegacyDDPMDiscretization()(12)
    mult = S.dpmpp2m_multipliers(sigmas)
    for scale_im, e in ((3.5, eps), (None, eps[:4])):
        want = S.cfg_euler_update(x, e, sigmas[0].reshape(1), sigmas[1].reshape(1), 7.5, scale_im, fused=False)
        got, d0 = S.cfg_dpmpp2m_update(x, e, None, sigmas[0].reshape(1), mult[0], 7.5, scale_im, fused=False)
        err = float((got - want).abs().max() / want.abs().max())
        print("step 0, DPM++ 2M vs Euler:", err)
        assert err < 1e-5 and torch.isfinite(d0).all()
        nan_old = torch.full_like(x, float("nan"))
        got2, _ = S.cfg_dpmpp2m_update(x, e, nan_old, sigmas[0].reshape(1), mult[0], 7.5, scale_im, fused=False)
        assert torch.equal(got2, got)  # 0 * NaN never reaches x
    with pytest.raises(ValueError):
        S.cfg_dpmpp2m_update(x, eps, None, sigmas[0].reshape(1), mult[0], 7.5, None, fused=False)


def test_solver_header_matches_the_second_signature_table():
    """include/cd360_solvers.h <=> cd360._lib.SOLVER_SIGNATURES, by the rule test_library_exports_every_declared_symbol holds cd360_hip.h
    to (every `cd360_...(` word, comments included); the library exports both symbols, typed; SIGNATURES does not hold the new names and
    cd360_hip.h does not name them."""
    from cd360 import _lib
    older = ("cd360_hip.h",)
    mismatch, in_tables, in_headers, mistyped, lib = SC.check_header_matches_table("cd360_solvers.h", _lib.SOLVER_SIGNATURES, NEW, older)
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    nul = ctypes.c_void_p(None)  # the host refuses null pointers before anything is launched (no GPU needed)
    assert lib.cd360_cfg_dpmpp2m_step_f32(nul, nul, nul, nul, nul, 7.5, 3.5, nul, nul, 16, nul) == -1
    assert lib.cd360_cfg_dpmpp2m_step_cl(nul, nul, nul, nul, nul, nul, 7.5, 3.5, 1, 16, 4, nul) == -1


def test_job_sampler_takes_a_solver_and_refuses_an_unknown_one():
    from cd360 import job, sampling
    from test_cfg2_cpu import _pose_net
    net, _ = _pose_net(1)
    sampling.enable_reference_sampling(net, [0, 2])
    g = torch.Generator().manual_seed(1)
    ctx, y = torch.randn(6, 7, 16, generator=g), torch.randn(6, 12, generator=g)
    pose = [object() for _ in range(6)]
    assert job.Sampler(net, pose, ctx, y, 12).solver == "euler"
    assert job.Sampler(net, pose, ctx, y, 12, solver="dpmpp2m").solver == "dpmpp2m"
    with pytest.raises(ValueError):
        job.Sampler(net, pose, ctx, y, 12, solver="nope")
    sampling.disable_reference_sampling(net)
