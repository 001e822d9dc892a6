"""DPM++ 2S ancestral and linear multistep (cd360.sampler.DPMPP2SAncestralSampler, LinearMultistepSampler, dpmpp2s_tables, lms_coefficients,
fused_cfg_dpmpp2s_step, fused_cfg_lms_step) against golden vectors written by the REFERENCE's classes (tests/golden/make_golden_highorder.py:
DPMPP2SAncestralSampler with only `denoise` unpacked, LinearMultistepSampler around a denoiser returning the pair it unpacks, the noise a
stored tensor), the new header against the binding's fifth signature table, and the job sampler's solver="dpmpp2s_a" / "lms".  CPU only;
tests/test_highorder_gpu.py holds the kernels and the captured job."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sampler_cases as SC
from test_dpmpp2m_cpu import DISC, GUIDERS, conds, row_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ("cd360_cfg_dpmpp2s_mid_cl", "cd360_cfg_dpmpp2s_mid_f32", "cd360_cfg_dpmpp2s_step_cl", "cd360_cfg_dpmpp2s_step_f32", "cd360_cfg_lms_step_cl",
       "cd360_cfg_lms_step_f32")
SETTINGS = {"e10": (1.0, 1.0), "e06": (0.6, 1.05), "e15": (1.5, 1.0)}  # (eta, s_noise), as the golden script
ORDERS = (4, 3, 1)
SINGLE_E15_12 = [0, 1, 2, 3, 4, 8, 9, 10, 11]  # the one-evaluation rows of 12 steps at eta 1.5, as the golden script asserts them
PATH = "sgm.modules.diffusionmodules.sampling."


def load():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "sampler_highorder.npz")).items()}


def stored_noise(z):
    """the golden script's draw: row k of z at the k-th call"""
    calls = iter(range(z.shape[0]))
    return lambda x: z[next(calls)].to(x.device).expand_as(x).clone()


def build(cls, guider, **params):
    """by dotted path through instantiate_from_config, as the YAML's sampler_config does"""
    from sgm.util import instantiate_from_config
    den = instantiate_from_config({"target": "sgm.modules.diffusionmodules.denoiser.DiscreteDenoiser", "params": {
        "num_idx": 1000, "weighting_config": {"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        "scaling_config": {"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, "discretization_config": DISC}})
    smp = instantiate_from_config({"target": PATH + cls, "params": dict(num_steps=50, discretization_config=DISC, guider_config=guider, device="cpu",
                                                                        **params)})
    return den, smp


def close(got, want):  # test_dpmpp2m_cpu.py::close
    return torch.allclose(got, want, atol=2e-5, rtol=1e-5)


# ================================================================================================ 1: the classes
@pytest.mark.parametrize("tag", list(SETTINGS))
@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
@pytest.mark.parametrize("steps", [12, 4])
def test_dpmpp2s_class_walks_the_reference_trajectory_with_every_intermediate(name, steps, tag):
    """The class, built by the reference's dotted path: __call__ returns (x, rgb_list) and lands on the reference's final latent; driven step
    by step through sampler_step it reproduces every intermediate x (stored for the 12-step runs) and hands the denoiser the recorded sigmas
    in the recorded order -- 2n - (one-evaluation rows) calls, the second of a step at to_sigma(s), un-snapped.  One draw per step."""
    from cd360 import sampler as S
    g = load()
    c, uc = conds(g)
    eta, s_noise = SETTINGS[tag]
    den, smp = build("DPMPP2SAncestralSampler", GUIDERS[name], eta=eta, s_noise=s_noise)
    assert type(smp) is S.DPMPP2SAncestralSampler and callable(smp.noise_sampler) and smp.seed is None and (smp.eta, smp.s_noise) == (eta, s_noise)
    seen = []

    def denoiser(inp, s, cc):
        seen.append(s[0].clone())
        return den(row_network, inp, s, cc)

    key = f"2s_{name}_{steps}_{tag}"
    want, tab = g[key], g[f"2s_tab_{steps}_{tag}"]
    singles = [i for i in range(steps) if tab[i, 7] > 0]
    draws = []
    noise = stored_noise(g["z"])
    smp.noise_sampler = lambda x: (draws.append(1), noise(x))[1]
    res, rgb = smp(denoiser, g["x"].clone(), c, uc=uc, num_steps=steps)
    print(key, "final vs the reference, max abs:", float((res - want).abs().max()), "of max", float(want.abs().max()))
    assert close(res, want) and rgb is not None and rgb is smp.rgb_list
    dsig = g[f"2s_{steps}_{tag}_dsig"]
    assert len(seen) == dsig.numel() == 2 * steps - len(singles) and len(draws) == steps
    assert torch.allclose(torch.stack(seen), dsig, rtol=1e-6, atol=0)
    if tag == "e15" and steps == 12:
        assert singles == SINGLE_E15_12
    if tag != "e15":
        assert singles == [steps - 1]
    smp.noise_sampler = stored_noise(g["z"])
    x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(g["x"].clone(), c, uc, steps)
    assert num_sigmas == steps + 1
    for i in range(steps):
        before = len(seen)
        x = smp.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc=ucond)
        assert len(seen) - before == (1 if i in singles else 2), i
        if steps == 12:
            assert close(x, g[key + "_x"][i]), (key, i)
    assert torch.equal(x, res)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
@pytest.mark.parametrize("steps", [12, 4])
def test_lms_class_walks_the_reference_trajectory_with_every_intermediate(name, steps, order):
    """The class, built by the reference's dotted path: __call__ returns (x, rgb_list) and lands on the reference's final latent; driven step
    by step through sampler_step on lms_coefficients it reproduces every intermediate x (stored for the 12-step runs), `ds` never holds more
    than `order` directions, and the denoiser sees the schedule's sigmas in order, once each."""
    from cd360 import sampler as S
    g = load()
    c, uc = conds(g)
    den, smp = build("LinearMultistepSampler", GUIDERS[name], order=order)
    assert type(smp) is S.LinearMultistepSampler and smp.order == order
    seen = []

    def denoiser(inp, s, cc):
        seen.append(s[0].clone())
        return den(row_network, inp, s, cc)

    key = f"lms_{name}_{steps}_o{order}"
    want = g[key]
    res, rgb = smp(denoiser, g["x"].clone(), c, uc=uc, num_steps=steps)
    print(key, "final vs the reference, max abs:", float((res - want).abs().max()), "of max", float(want.abs().max()))
    assert close(res, want) and rgb is not None and rgb is smp.rgb_list
    dsig = g[f"lms_{steps}_dsig"]
    assert len(seen) == dsig.numel() == steps and torch.allclose(torch.stack(seen), dsig, rtol=1e-6, atol=0)
    x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(g["x"].clone(), c, uc, steps)
    table, ds = S.lms_coefficients(sigmas, order), []
    for i in range(steps):
        cur = min(i + 1, order)
        x = smp.sampler_step(ds, [float(table[i, j]) for j in range(cur)], s_in * sigmas[i], denoiser, x, cond, uc=ucond)
        assert len(ds) == cur
        if steps == 12:
            assert close(x, g[key + "_x"][i]), (key, i)
    assert torch.equal(x, res)
    if order == 1:  # first order is Euler: (sigma_next - sigma) d
        eul = S.EulerEDMSampler(discretization_config=DISC, num_steps=50, guider_config=GUIDERS[name], device="cpu")
        plain, _ = eul(lambda inp, s, cc: den(row_network, inp, s, cc), g["x"].clone(), c, uc=uc, num_steps=steps)
        assert close(plain, res)


def test_settings_differ_and_eta_zero_is_deterministic():
    """The goldens of the settings differ pairwise by more than 1e-2 (a class that ignored eta, s_noise or order could not pass them all).
    eta = 0: sigma_down = sigma_next, nothing is drawn (noise_sampler is never called), two evaluations on every row but the last.
    seed=<int> asks for the library's generator: a host tensor raises like every operator."""
    from cd360 import _lib
    from cd360 import sampler as S
    g = load()
    for a, b in (("2s_cfg3_12_e10", "2s_cfg3_12_e06"), ("2s_cfg3_12_e10", "2s_cfg3_12_e15"), ("lms_cfg3_12_o4", "lms_cfg3_12_o3"),
                 ("lms_cfg3_12_o3", "lms_cfg3_12_o1"), ("2s_cfg3_12_e10", "lms_cfg3_12_o4")):
        assert float((g[a] - g[b]).abs().max()) > 1e-2, (a, b)
    c, uc = conds(g)
    den, smp = build("DPMPP2SAncestralSampler", GUIDERS["cfg3"], eta=0.0)
    smp.noise_sampler = None  # never called
    calls = []
    res, _ = smp(lambda inp, s, cc: (calls.append(1), den(row_network, inp, s, cc))[1], g["x"].clone(), c, uc=uc, num_steps=4)
    assert torch.isfinite(res).all() and len(calls) == 7
    anc, mid, mult = S.dpmpp2s_tables(S.LegacyDDPMDiscretization()(4), den, eta=0.0)
    assert torch.equal(anc[:, 0], S.LegacyDDPMDiscretization()(4)[1:]) and not anc[:, 1].any()
    seeded = S.DPMPP2SAncestralSampler(discretization_config=DISC, num_steps=4, guider_config=GUIDERS["cfg3"], device="cpu", seed=7)
    assert seeded.seed == 7
    with pytest.raises(_lib.Cd360Error):
        seeded.noise_sampler(g["x"])


# ================================================================================================ 2: the tables
@pytest.mark.parametrize("tag", list(SETTINGS))
@pytest.mark.parametrize("steps", [12, 4])
def test_dpmpp2s_tables_match_the_reference(steps, tag):
    """dpmpp2s_tables against the (sigma_down, sigma_up, sigma_mid, mult1..4) the reference computed per step: rtol 1e-6, atol 0 (host
    vector math; the bar dpmpp2m_multipliers is held to).  Exact where the value is a decision: anc_tab is euler_ancestral_table; the
    one-evaluation rows are the recorded ones and hold the documented finite filler; column 3 of mid_tab is
    DiscreteDenoiser.possibly_quantize_sigma(sigma_mid), column 2 its c_in, column 1 sigma_down; sigma_mid lies strictly between sigma_down
    and sigma, off the grid."""
    from cd360 import sampler as S
    g = load()
    den = S.DiscreteDenoiser()
    sig = S.LegacyDDPMDiscretization()(steps)
    eta, s_noise = SETTINGS[tag]
    anc, mid, mult = S.dpmpp2s_tables(sig, den, eta, s_noise)
    for t in (anc, mid, mult):
        assert t.shape == (steps, 4) and t.dtype == torch.float32 and t.device.type == "cpu" and t.is_contiguous() and torch.isfinite(t).all()
    assert torch.equal(anc, S.euler_ancestral_table(sig, eta, s_noise))
    want = g[f"2s_tab_{steps}_{tag}"]
    single = want[:, 7] > 0
    assert S.dpmpp2s_single_rows(anc) == single.tolist()
    two = ~single
    for col, (got, ref) in {"sigma_down": (anc[:, 0], want[:, 0]), "sigma_up": (anc[:, 1], want[:, 1]), "sigma_mid": (mid[two, 0], want[two, 2]),
                            "mult1": (mult[two, 0], want[two, 3]), "mult2": (mult[two, 1], want[two, 4]), "mult3": (mult[two, 2], want[two, 5]),
                            "mult4": (mult[two, 3], want[two, 6])}.items():
        if got.numel():
            print(steps, tag, col, "vs the reference, max rel:", float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max()))
        assert torch.allclose(got, ref, rtol=1e-6, atol=0), col
    assert torch.equal(mid[two, 1], anc[two, 0])
    assert torch.equal(mid[:, 3], den.possibly_quantize_sigma(mid[:, 0])) and torch.equal(mid[:, 2], den.scaling(mid[:, 3])[2])
    assert bool((mid[two, 0] < sig[:-1][two]).all()) and bool((mid[two, 0] > anc[two, 0]).all())
    if two.any():
        assert bool((mid[two, 3] != mid[two, 0]).any())  # off the grid: the snapped sigma is another number
    assert torch.equal(mult[single], torch.zeros(int(single.sum()), 4))
    assert torch.equal(mid[single, 0], sig[:-1][single]) and torch.equal(mid[single, 1], sig[1:][single]) and torch.equal(mid[single, 3], sig[:-1][single])
    assert bool(single[-1]) and float(anc[-1, 1]) == 0.0


@pytest.mark.parametrize("steps", [12, 4])
def test_lms_coefficients_match_the_reference(steps):
    """lms_coefficients against the coefficients the reference computed (scipy's quad on the fp32 sigmas, as it runs): at most 2^-22 = 2.4e-7
    -- two fp32 ulps -- of the row's largest coefficient (the golden script measured 7.1e-8: the fp32 rounding of the table plus the
    reference's fp32 integrand).  The zero padding is exact; the rows of an order's table sum to sigma_next - sigma (a constant is
    integrated exactly); orders 0 and 5 raise, and scipy is not imported."""
    from cd360 import sampler as S
    g = load()
    sig = S.LegacyDDPMDiscretization()(steps)
    assert torch.equal(sig, g[f"sigmas_{steps}"])
    for order in ORDERS:
        tab = S.lms_coefficients(sig, order)
        assert tab.shape == (steps, 4) and tab.dtype == torch.float32 and tab.is_contiguous()
        ref = g[f"lms_coef_{steps}_o{order}"]
        worst = 0.0
        for i in range(steps):
            cur = min(i + 1, order)
            assert torch.equal(tab[i, cur:], torch.zeros(4 - cur)) and bool((tab[i, :cur] != 0).all())
            worst = max(worst, float((tab[i].double() - ref[i]).abs().max() / ref[i].abs().max()))
        print(f"lms_coefficients {steps} steps order {order}: max |table - reference| / max |row| = {worst:.3e} | bar {2.0 ** -22:.3e}")
        assert worst <= 2.0 ** -22
        assert torch.allclose(tab.double().sum(1), (sig[1:] - sig[:-1]).double(), rtol=1e-6, atol=0)
    for bad in (0, 5, -1, 2.0, True):
        with pytest.raises(ValueError):
            S.lms_coefficients(sig, bad)
    assert not re.search(r"^\s*(import|from)\s+scipy", open(S.__file__).read(), re.M)


# ================================================================================================ 3: the product step functions
def run_product_steps(g, solver, name, dev, fused, tag, steps=12):
    """The trajectory through the product's step functions (cd360.sampler.fused_cfg_dpmpp2s_step / fused_cfg_lms_step: what cd360/job.py
    launches per step on the un-staged route) on the tables, with the golden's stored z as the noise, around the golden's network; tag = a
    key of SETTINGS (solver "2s") or an order (solver "lms"); returns (final x, [x_i])."""
    from cd360 import sampler as S
    den = S.DiscreteDenoiser().to(dev)
    guider = S.ScheduledCFGImgTextRef(7.5, 3.5) if name == "cfg3" else S.VanillaCFGImgRef(7.5)
    c, uc = conds(g, dev)
    x = g["x"].to(dev)
    _, _, cond = guider.prepare_inputs(x, x.new_ones(x.shape[0]), c, uc)
    sigmas = S.LegacyDDPMDiscretization()(steps, device=dev)
    z = g["z"].to(dev)
    x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)
    network = lambda x_in, c_noise: row_network(x_in, c_noise, cond)[0]  # noqa: E731
    xs = []
    if solver == "2s":
        anc, mid, mult = (t.to(dev) for t in S.dpmpp2s_tables(sigmas, den, *SETTINGS[tag]))
        for i in range(steps):  # (the reference drew row i of z at step i)
            x = S.fused_cfg_dpmpp2s_step(den, network, x, sigmas[i], anc[i], mid[i], mult[i], guider, noise=z[i].expand_as(x), fused=fused)
            xs.append(x)
        return x, xs
    tab = S.lms_coefficients(sigmas, tag).to(dev)
    ring = torch.full((tag,) + tuple(x.shape), float("nan"), device=dev)  # unread slots hold NaN: it must not reach x
    for i in range(steps):
        x = S.fused_cfg_lms_step(den, network, x, ring, sigmas[i], tab[i], i, guider, fused=fused)
        xs.append(x)
    return x, xs


RUNS = [("2s", t) for t in SETTINGS] + [("lms", o) for o in ORDERS]


def golden_key(solver, name, tag):
    return f"2s_{name}_12_{tag}" if solver == "2s" else f"lms_{name}_12_o{tag}"


@pytest.mark.parametrize("solver,tag", RUNS)
def test_product_step_functions_walk_the_reference_trajectory_for_both_guiders(solver, tag):
    """fused_cfg_dpmpp2s_step / fused_cfg_lms_step (fused=False) -- the plain-torch chain in the kernels' order, on the TABLES, the noise
    handed in as a tensor, the linear multistep history in a NaN-filled ring -- over 12 steps against the reference, every intermediate;
    and the two guiders' results differ."""
    g = load()
    finals = {}
    for name in ("cfg3", "cfg2"):
        res, xs = run_product_steps(g, solver, name, "cpu", fused=False, tag=tag)
        key = golden_key(solver, name, tag)
        print(key, "table-form CPU trajectory vs the reference, max abs:", float((res - g[key]).abs().max()))
        assert close(res, g[key])
        for i in range(12):
            assert close(xs[i], g[key + "_x"][i]), (key, i)
        finals[name] = res
    assert float((finals["cfg3"] - finals["cfg2"]).abs().max()) > 1e-2 * float(finals["cfg3"].abs().max())


def test_flat_forms_on_their_edge_rows():
    """A one-evaluation row of fused_cfg_dpmpp2s_step is fused_cfg_euler_ancestral_step bit for bit and calls the network once; a noisy row
    without noise, and a wrong branch count, raise; the linear multistep update writes slot i % order and leaves the others alone."""
    import weights as W
    from cd360 import sampler as S
    x, eps = W.tensor("x", (2, 4, 8, 8), seed=3), W.tensor("eps", (6, 4, 8, 8), seed=3)
    den, sig = S.DiscreteDenoiser(), S.LegacyDDPMDiscretization()(4)
    anc, mid, mult = S.dpmpp2s_tables(sig, den, 1.0, 1.0)
    guider = S.ScheduledCFGImgTextRef(7.5, 3.5)
    calls = []
    network = lambda x_in, c_noise: (calls.append(1), eps * x_in.mean())[1]  # noqa: E731
    got = S.fused_cfg_dpmpp2s_step(den, network, x, sig[3], anc[3], mid[3], mult[3], guider, fused=False)
    assert len(calls) == 1
    assert torch.equal(got, S.fused_cfg_euler_ancestral_step(den, network, x, sig[3], anc[3], guider, fused=False))
    del calls[:]
    z = torch.ones_like(x)
    S.fused_cfg_dpmpp2s_step(den, network, x, sig[1], anc[1], mid[1], mult[1], guider, noise=z, fused=False)
    assert len(calls) == 2
    with pytest.raises(ValueError):
        S.fused_cfg_dpmpp2s_step(den, network, x, sig[1], anc[1], mid[1], mult[1], guider, fused=False)  # sigma_up != 0, no noise
    with pytest.raises(ValueError):
        S.cfg_dpmpp2s_mid(x, eps, sig[1].reshape(1), mult[1], 7.5, None, fused=False)  # six rows, two branches
    with pytest.raises(ValueError):
        S.cfg_lms_update(x, eps, torch.zeros(3, *x.shape), sig[1].reshape(1), torch.ones(4), 1, 7.5, None, fused=False)
    tab = S.lms_coefficients(sig, 3)
    ring = torch.full((3,) + tuple(x.shape), 7.0)
    out = S.cfg_lms_update(x, eps, ring, sig[0].reshape(1), tab[0], 0, 7.5, 3.5, fused=False)
    d = (x - S.cfg_combine(x, eps, sig[0].reshape(1), 7.5, 3.5)) / sig[0]
    assert torch.equal(ring[0], d) and bool((ring[1:] == 7.0).all()) and torch.equal(out, x + tab[0, 0] * d)
    S.cfg_lms_update(x, eps, ring, sig[3].reshape(1), tab[3], 3, 7.5, 3.5, fused=False)  # 3 % 3: slot 0 again
    assert not torch.equal(ring[0], d) and bool((ring[1:] == 7.0).all())


# ================================================================================================ 4: header and table
def test_highorder_header_matches_the_fifth_signature_table():
    """include/cd360_highorder.h <=> cd360._lib.HIGHORDER_SIGNATURES, by the rule test_edm_header_matches_the_fourth_signature_table holds
    (every `cd360_...(` word, comments included); the library exports the six symbols, typed; no older table holds the new names and no
    older header names them; null pointers are refused on the host (no GPU needed)."""
    from cd360 import _lib
    older = ("cd360_hip.h", "cd360_solvers.h", "cd360_stochastic.h", "cd360_edm.h")
    mismatch, in_tables, in_headers, mistyped, lib = SC.check_header_matches_table("cd360_highorder.h", _lib.HIGHORDER_SIGNATURES, NEW, older)
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    nul = ctypes.c_void_p(None)
    assert lib.cd360_cfg_dpmpp2s_mid_cl(nul, nul, nul, nul, nul, 7.5, 3.5, nul, 1, 16, 4, nul) == -1
    assert lib.cd360_cfg_dpmpp2s_mid_f32(nul, nul, nul, nul, 7.5, 3.5, nul, 16, nul) == -1
    assert lib.cd360_cfg_dpmpp2s_step_cl(nul, nul, nul, nul, nul, nul, nul, nul, nul, 7.5, 3.5, 1, 16, 4, nul) == -1
    assert lib.cd360_cfg_dpmpp2s_step_f32(nul, nul, nul, nul, nul, nul, nul, nul, nul, 7.5, 3.5, nul, 1, 16, nul) == -1
    assert lib.cd360_cfg_lms_step_cl(nul, nul, nul, nul, nul, nul, 7.5, 3.5, 4, 1, 16, 4, nul) == -1
    assert lib.cd360_cfg_lms_step_f32(nul, nul, nul, nul, nul, nul, 7.5, 3.5, 4, nul, 16, nul) == -1


# ================================================================================================ 5: the job constructor
def test_job_sampler_takes_both_solvers_and_refuses_an_unknown_one():
    from cd360 import job, sampling, solvers
    from test_cfg2_cpu import _pose_net
    net, _ = _pose_net(1)
    sampling.enable_reference_sampling(net, [0, 2])
    g = torch.Generator().manual_seed(1)
    ctx, y = torch.randn(6, 7, 16, generator=g), torch.randn(6, 12, generator=g)
    pose = [object() for _ in range(6)]
    assert job.Sampler.HIGHORDER_SOLVERS == ("dpmpp2s_a", "lms") == tuple(solvers.HIGHORDER_SOLVERS)
    assert job.Sampler.SOLVERS == ("euler", "dpmpp2m", "euler_a") and job.Sampler.EDM_SOLVERS == ("heun",)  # the older registries keep their contents
    smp = job.Sampler(net, pose, ctx, y, 12, solver="dpmpp2s_a", eta=0.6, s_noise=1.05, seed=2 ** 63 + 12345, noise_streams=[0, 1])
    assert smp.solver == "dpmpp2s_a" and smp._solver is solvers.HIGHORDER_SOLVERS["dpmpp2s_a"] and smp._solver.draws(smp)
    assert (smp.eta, smp.s_noise, smp.seed, smp.noise_streams, smp.order) == (0.6, 1.05, 2 ** 63 + 12345, [0, 1], 4)
    smp.reseed(5)
    assert smp.seed == 5
    smp.set_noise_streams([1, 0])
    assert smp.noise_streams == [1, 0]
    with pytest.raises(ValueError):
        smp.set_noise_streams([0, 1, 2])  # bs = 2 replay rows
    lms = job.Sampler(net, pose, ctx, y, 12, solver="lms", order=3)
    assert lms.solver == "lms" and lms._solver is solvers.HIGHORDER_SOLVERS["lms"] and lms.order == 3 and not lms._solver.draws(lms)
    assert job.Sampler(net, pose, ctx, y, 12, solver="lms").order == 4
    with pytest.raises(ValueError):
        lms.reseed(1)  # deterministic
    with pytest.raises(ValueError):
        lms.set_noise_streams([0, 1])
    for bad in (0, 5):
        with pytest.raises(ValueError):
            job.Sampler(net, pose, ctx, y, 12, solver="lms", order=bad)
    heun = job.Sampler(net, pose, ctx, y, 12, solver="heun")  # the per-row question, by its default: Heun's last row only
    assert [heun._solver.single_row(heun, i) for i in range(12)] == [False] * 11 + [True]
    assert not any(solvers.SOLVERS["euler"].single_row(smp, i) for i in range(12))
    with pytest.raises(ValueError) as e:
        job.Sampler(net, pose, ctx, y, 12, solver="nope")
    assert all(re.search(rf"\b{n}\b", str(e.value)) for n in ("euler", "dpmpp2m", "euler_a", "heun", "dpmpp2s_a", "lms"))
    sampling.disable_reference_sampling(net)
