"""Ancestral Euler (cd360.sampler.EulerAncestralSampler, euler_ancestral_table, fused_cfg_euler_ancestral_step) against golden vectors
written by the REFERENCE's EulerAncestralSampler (tests/golden/make_golden_euler_a.py: a subclass that only unpacks `denoise`, the noise a
stored tensor), the new header against the binding's third signature table, the job sampler's solver="euler_a", and the numpy restatement
of the device noise (tests/philox_ref.py): known answers and statistics.  CPU only; tests/test_euler_a_gpu.py holds the kernels and the
captured job."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sampler_cases as SC
import philox_ref as P
from test_dpmpp2m_cpu import DISC, GUIDERS, conds, row_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ("cd360_sampler_noise_f32", "cd360_cfg_euler_ancestral_step_f32", "cd360_cfg_euler_ancestral_step_cl")
SETTINGS = {"e10": (1.0, 1.0), "e06": (0.6, 1.05)}  # (eta, s_noise), as the golden script


def load():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "sampler_euler_a.npz")).items()}


def stored_noise(z):
    """the golden script's noise_sampler: row i of z at the i-th call"""
    calls = iter(range(z.shape[0]))
    return lambda x: z[next(calls)].to(x.device).expand_as(x).clone()


def build(guider, eta, s_noise):
    """by dotted path through instantiate_from_config, as the YAML's sampler_config does"""
    from sgm.util import instantiate_from_config
    den = instantiate_from_config({"target": "sgm.modules.diffusionmodules.denoiser.DiscreteDenoiser", "params": {
        "num_idx": 1000, "weighting_config": {"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        "scaling_config": {"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, "discretization_config": DISC}})
    smp = instantiate_from_config({"target": "sgm.modules.diffusionmodules.sampling.EulerAncestralSampler", "params": {
        "eta": eta, "s_noise": s_noise, "num_steps": 50, "discretization_config": DISC, "guider_config": guider, "device": "cpu"}})
    return den, smp


def close(got, want):
    return torch.allclose(got, want, atol=2e-5, rtol=1e-5)


# ================================================================================================ 1: the class
@pytest.mark.parametrize("tag", ["e10", "e06"])
@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
@pytest.mark.parametrize("steps", [12, 4])
def test_class_walks_the_reference_trajectory_with_every_intermediate(name, steps, tag):
    """The class, built by the reference's dotted path: __call__ returns (x, rgb_list) and lands on the reference's final latent; driven
    step by step through sampler_step it reproduces every intermediate x.  Bar: the one test_sampler_cpu.py / test_dpmpp2m_cpu.py hold.
    The plain Euler result differs from the golden by more than 1e-2 of its maximum, so an Euler step cannot pass."""
    from cd360.sampler import EulerAncestralSampler, EulerEDMSampler
    g = load()
    c, uc = conds(g)
    eta, s_noise = SETTINGS[tag]
    den, smp = build(GUIDERS[name], eta, s_noise)
    assert type(smp) is EulerAncestralSampler and (smp.eta, smp.s_noise) == (eta, s_noise) and callable(smp.noise_sampler)
    denoiser = lambda inp, s, cc: den(row_network, inp, s, cc)  # noqa: E731
    want = g[f"{name}_{steps}_{tag}"]
    smp.noise_sampler = stored_noise(g["z"])
    res, rgb = smp(denoiser, g["x"].clone(), c, uc=uc, num_steps=steps)
    print(name, steps, tag, "final vs the reference, max abs:", float((res - want).abs().max()), "of max", float(want.abs().max()))
    assert close(res, want) and rgb is not None and rgb is smp.rgb_list
    smp.noise_sampler = stored_noise(g["z"])
    x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(g["x"].clone(), c, uc, steps)
    assert num_sigmas == steps + 1
    for i in range(steps):
        x = smp.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc=ucond)
        assert close(x, g[f"{name}_{steps}_{tag}_x"][i]), (name, steps, tag, i)
    assert torch.equal(x, res)
    eul = EulerEDMSampler(discretization_config=DISC, num_steps=50, guider_config=GUIDERS[name], device="cpu")
    plain, _ = eul(denoiser, g["x"].clone(), c, uc=uc, num_steps=steps)
    gap = float((plain - want).abs().max() / want.abs().max())
    print(name, steps, tag, "plain Euler vs the ancestral golden, rel:", gap)
    assert gap > 1e-2


def test_constructor_noise_sampler_and_eta_zero():
    """seed=None: noise_sampler draws torch.randn_like (the reference's default).  seed=<int>: the library's generator, GPU tensors only -- a
    host tensor raises like every operator.  eta = 0 is served as plain Euler (the reference hands a float to append_dims there)."""
    from cd360 import _lib
    from cd360.sampler import EulerAncestralSampler, EulerEDMSampler
    g = load()
    c, uc = conds(g)
    smp = EulerAncestralSampler(discretization_config=DISC, num_steps=4, guider_config=GUIDERS["cfg3"], device="cpu")
    torch.manual_seed(3)
    a = smp.noise_sampler(g["x"])
    torch.manual_seed(3)
    assert torch.equal(a, torch.randn_like(g["x"])) and smp.seed is None
    seeded = EulerAncestralSampler(discretization_config=DISC, num_steps=4, guider_config=GUIDERS["cfg3"], device="cpu", seed=7)
    with pytest.raises(_lib.Cd360Error):
        seeded.noise_sampler(g["x"])
    den, zero = build(GUIDERS["cfg3"], 0.0, 1.0)
    denoiser = lambda inp, s, cc: den(row_network, inp, s, cc)  # noqa: E731
    zero.noise_sampler = None  # never called
    got, _ = zero(denoiser, g["x"].clone(), c, uc=uc, num_steps=4)
    want, _ = EulerEDMSampler(discretization_config=DISC, num_steps=50, guider_config=GUIDERS["cfg3"], device="cpu")(
        denoiser, g["x"].clone(), c, uc=uc, num_steps=4)
    assert torch.equal(got, want)


# ================================================================================================ 2: the table
@pytest.mark.parametrize("tag", ["e10", "e06"])
@pytest.mark.parametrize("steps", [12, 4])
def test_ancestral_table_matches_the_reference(steps, tag):
    """euler_ancestral_table against the (sigma_down, sigma_up) the reference computed per step: rtol 1e-6, atol 0 (host vector math, the
    bar of test_multiplier_table_matches_the_reference).  Exact where the value is a decision: the last row (0, 0); eta = 0 rows
    (sigma_next, 0).  sigma_down^2 + sigma_up^2 = sigma_next^2 to 1e-6 relative (evaluated in float64 on the fp32 entries: four fp32
    roundings of at most 6e-8 each)."""
    from cd360.sampler import LegacyDDPMDiscretization, euler_ancestral_table
    g = load()
    eta, s_noise = SETTINGS[tag]
    sig = LegacyDDPMDiscretization()(steps)
    tab = euler_ancestral_table(sig, eta, s_noise)
    want = g[f"anc_{steps}_{tag}"]
    assert tab.shape == (steps, 4) and tuple(want.shape) == (steps, 2) and tab.dtype == torch.float32 and tab.device.type == "cpu" and tab.is_contiguous()
    assert tab[-1, :2].tolist() == [0.0, 0.0] and want[-1].tolist() == [0.0, 0.0]
    assert torch.equal(tab[:, 2], torch.full((steps,), s_noise)) and torch.equal(tab[:, 3], torch.zeros(steps))
    assert bool((tab[:-1, 1] > 0).all()) and bool((tab[:-1, 0] > 0).all()) and torch.isfinite(tab).all()
    print("ancestral table vs the reference, max rel:", float(((tab[:, :2] - want).abs() / want.abs().clamp_min(1e-30)).max()))
    assert torch.allclose(tab[:, :2], want, rtol=1e-6, atol=0)
    t64, s64 = tab.double(), sig.double()
    rel = ((t64[:-1, 0] ** 2 + t64[:-1, 1] ** 2 - s64[1:-1] ** 2).abs() / s64[1:-1] ** 2).max()
    print("sigma_down^2 + sigma_up^2 vs sigma_next^2, max rel:", float(rel))
    assert float(rel) <= 1e-6
    zero = euler_ancestral_table(sig, 0.0, s_noise)
    assert torch.equal(zero[:, 0], sig[1:]) and torch.equal(zero[:, 1], torch.zeros(steps)) and torch.equal(zero[:, 2], tab[:, 2])


def test_get_ancestral_step_is_the_references_expression():
    from cd360.sampler import get_ancestral_step
    s, sn = torch.tensor([14.6, 3.0, 0.5]), torch.tensor([9.1, 1.2, 0.0])
    down, up = get_ancestral_step(s, sn, eta=0.6)
    want_up = torch.minimum(sn, 0.6 * (sn ** 2 * (s ** 2 - sn ** 2) / s ** 2) ** 0.5)
    assert torch.equal(up, want_up) and torch.equal(down, (sn ** 2 - want_up ** 2) ** 0.5) and up[-1] == 0 and down[-1] == 0
    d0, u0 = get_ancestral_step(s, sn, eta=0.0)
    assert d0 is sn and torch.equal(u0, torch.zeros(3))


# ================================================================================================ 3: the product step function
def run_product_steps(g, name, dev, fused, tag="e10", steps=12):
    """The trajectory through the product's step function (cd360.sampler.fused_cfg_euler_ancestral_step: what cd360/job.py launches per
    step for solver="euler_a") with the golden's stored z as the noise, around the golden's network; returns (final x, [x_i])."""
    from cd360 import sampler as S
    eta, s_noise = SETTINGS[tag]
    den = S.DiscreteDenoiser().to(dev)
    guider = S.ScheduledCFGImgTextRef(7.5, 3.5) if name == "cfg3" else S.VanillaCFGImgRef(7.5)
    c, uc = conds(g, dev)
    x = g["x"].to(dev)
    _, _, cond = guider.prepare_inputs(x, x.new_ones(x.shape[0]), c, uc)
    sigmas = S.LegacyDDPMDiscretization()(steps, device=dev)
    anc = S.euler_ancestral_table(sigmas, eta, s_noise).to(dev)
    z = g["z"].to(dev)
    x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)
    network = lambda x_in, c_noise: row_network(x_in, c_noise, cond)[0]  # noqa: E731
    xs = []
    for i in range(steps):
        x = S.fused_cfg_euler_ancestral_step(den, network, x, sigmas[i], anc[i], guider, noise=z[i], fused=fused)
        xs.append(x)
    return x, xs


@pytest.mark.parametrize("tag", ["e10", "e06"])
def test_product_step_function_walks_the_reference_trajectory_for_both_guiders(tag):
    """fused_cfg_euler_ancestral_step(fused=False) -- the plain-torch chain in the kernel's order, on the TABLE, the noise handed in as a
    tensor -- over 12 steps against the reference, every intermediate; and the two guiders' results differ."""
    g = load()
    finals = {}
    for name in ("cfg3", "cfg2"):
        res, xs = run_product_steps(g, name, "cpu", fused=False, tag=tag)
        print(name, tag, "table-form CPU trajectory vs the reference, max abs:", float((res - g[f"{name}_12_{tag}"]).abs().max()))
        assert close(res, g[f"{name}_12_{tag}"])
        for i in range(12):
            assert close(xs[i], g[f"{name}_12_{tag}_x"][i]), (name, i)
        finals[name] = res
    assert float((finals["cfg3"] - finals["cfg2"]).abs().max()) > 1e-2 * float(finals["cfg3"].abs().max())


def test_update_needs_noise_only_where_sigma_up_is_nonzero():
    import weights as W
    from cd360 import sampler as S
    x, eps = W.tensor("x", (2, 4, 8, 8), seed=3), W.tensor("eps", (6, 4, 8, 8), seed=3)
    sigmas = S.LegacyDDPMDiscretization()(4)
    anc = S.euler_ancestral_table(sigmas)
    last = S.cfg_euler_ancestral_update(x, eps, sigmas[3].reshape(1), anc[3], 7.5, 3.5, fused=False)  # sigma_up = 0: no noise asked for
    assert torch.equal(last, S.cfg_euler_update(x, eps, sigmas[3].reshape(1), sigmas[4].reshape(1), 7.5, 3.5, fused=False))
    with pytest.raises(ValueError):
        S.cfg_euler_ancestral_update(x, eps, sigmas[0].reshape(1), anc[0], 7.5, 3.5, fused=False)
    with pytest.raises(ValueError):
        S.cfg_euler_ancestral_update(x, eps, sigmas[0].reshape(1), anc[0], 7.5, None, noise=x, fused=False)  # six rows, two branches


# ================================================================================================ 4: header and table
def test_stochastic_header_matches_the_third_signature_table():
    """include/cd360_stochastic.h <=> cd360._lib.STOCHASTIC_SIGNATURES, by the rule test_library_exports_every_declared_symbol holds
    cd360_hip.h to (every `cd360_...(` word, comments included); the library exports the three symbols, typed; neither older table holds
    the new names and neither older header names them; null pointers are refused on the host (no GPU needed)."""
    from cd360 import _lib
    older = ("cd360_hip.h", "cd360_solvers.h")
    mismatch, in_tables, in_headers, mistyped, lib = SC.check_header_matches_table("cd360_stochastic.h", _lib.STOCHASTIC_SIGNATURES, NEW, older)
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    nul = ctypes.c_void_p(None)
    assert lib.cd360_sampler_noise_f32(nul, nul, nul, nul, 1, 16, nul) == -1
    assert lib.cd360_cfg_euler_ancestral_step_f32(nul, nul, nul, nul, nul, nul, nul, 7.5, 3.5, nul, 1, 16, nul) == -1
    assert lib.cd360_cfg_euler_ancestral_step_cl(nul, nul, nul, nul, nul, nul, nul, 7.5, 3.5, 1, 16, 4, nul) == -1


# ================================================================================================ 5: the job constructor
def test_job_sampler_takes_euler_a_and_refuses_an_unknown_solver():
    from cd360 import job, sampling
    from test_cfg2_cpu import _pose_net
    net, _ = _pose_net(1)
    sampling.enable_reference_sampling(net, [0, 2])
    g = torch.Generator().manual_seed(1)
    ctx, y = torch.randn(6, 7, 16, generator=g), torch.randn(6, 12, generator=g)
    pose = [object() for _ in range(6)]
    assert job.Sampler.SOLVERS == ("euler", "dpmpp2m", "euler_a")
    smp = job.Sampler(net, pose, ctx, y, 12, solver="euler_a")
    assert smp.solver == "euler_a" and (smp.eta, smp.s_noise, smp.seed, smp.noise_streams) == (1.0, 1.0, 0, None)
    smp = job.Sampler(net, pose, ctx, y, 12, solver="euler_a", eta=0.6, s_noise=1.05, seed=2 ** 63 + 12345, noise_streams=[0, 1])
    assert (smp.eta, smp.s_noise, smp.seed, smp.noise_streams) == (0.6, 1.05, 2 ** 63 + 12345, [0, 1])
    smp.reseed(5)
    assert smp.seed == 5
    with pytest.raises(ValueError):
        smp.set_noise_streams([0, 1, 2])  # bs = 2 replay rows
    with pytest.raises(ValueError):
        job.Sampler(net, pose, ctx, y, 12).reseed(1)  # Euler draws no noise
    with pytest.raises(ValueError):
        job.Sampler(net, pose, ctx, y, 12, solver="nope")
    sampling.disable_reference_sampling(net)


# ================================================================================================ 6: the restatement
def test_philox_known_answers():
    """The three Random123 known answers of philox4x32-10, and the seed -> key split the kernels use."""
    for counter, key, want in P.KAT:
        got = tuple(int(v) for v in P.philox4x32_10(counter, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    assert P.key_of(2 ** 63 + 12345) == (12345, 0x80000000) and P.key_of(-1) == (P.MASK, P.MASK) and P.key_of(30) == (30, 0)
    from cd360.sampler import seed_words
    for seed in (0, 30, 2 ** 63 + 12345, -1, 2 ** 64 + 5):
        w = seed_words(seed)
        assert -2 ** 63 <= w < 2 ** 63 and P.key_of(w) == P.key_of(seed)
    r = P.philox4x32_10((np.arange(5), 3, 1, 0), P.key_of(30))  # vectorised == one by one
    for px in range(5):
        assert tuple(int(v[px]) for v in r) == tuple(int(v) for v in P.philox4x32_10((px, 3, 1, 0), P.key_of(30)))


def test_restated_noise_statistics():
    """Conditions the GPU test then holds the kernel to: seeds 30, 0, 2^63 + 12345, HW = 4096, steps 0..3 (N = 65 536 values per seed) --
    |mean| <= 0.020, |var - 1| <= 0.028, |m4 - 3| <= 0.19 (five standard errors), and |correlation| <= 5 / sqrt(n) between steps 0 / 1,
    streams 0 / 1, seeds s / s + 1, channel pairs and neighbouring pixels.  Also: the uniforms stay in their intervals, so no value is
    infinite, and float32 evaluation follows float64."""
    worst = P.check_statistics(lambda seed, stream, step: P.normals(seed, stream, step, P.STAT_HW))
    print("restatement, worst figures: mean %.2e var %.2e m4 %.3f, correlation %.2f standard errors" % (worst["mean"], worst["var"], worst["m4"], worst["corr"]))
    z64, z32 = P.normals(30, 0, 0, P.STAT_HW), P.normals(30, 0, 0, P.STAT_HW, np.float32)
    assert z32.dtype == np.float32 and np.isfinite(z64).all() and np.abs(z64).max() < 5.8  # sqrt(-2 log 2^-24) = 5.77
    print("float32 vs float64 restatement, seed 30, HW 4096: max abs", float(np.abs(z32 - z64).max()))
    assert float(np.abs(z32 - z64).max()) < 1e-5
    za, zb = P.box_muller(np.array([0, P.MASK], np.uint32), np.array([0, P.MASK], np.uint32))  # the interval ends: u1 = 2^-24 and 1
    assert np.isfinite(za).all() and np.isfinite(zb).all() and abs(za[0] - np.sqrt(48 * np.log(2.0))) < 1e-12 and za[1] == 0
