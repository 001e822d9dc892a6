"""The EDM family with churn and the Heun corrector (cd360.sampler.EulerEDMSampler(s_churn=...), HeunEDMSampler, edm_tables,
fused_cfg_edm_euler_step, fused_cfg_heun_step) against golden vectors written by the REFERENCE's classes (tests/golden/make_golden_edm.py:
EulerEDMSampler as written, HeunEDMSampler with only `denoise` unpacked, the noise a stored tensor), the new header against the binding's
fourth signature table, and the job sampler's solver="heun" / s_churn.  CPU only; tests/test_edm_gpu.py holds the kernels and the captured
job."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sampler_cases as SC
from test_dpmpp2m_cpu import DISC, GUIDERS, conds, row_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ("cd360_edm_churn_f32", "cd360_cfg_edm_predict_cl", "cd360_cfg_edm_predict_f32", "cd360_cfg_edm_correct_cl", "cd360_cfg_edm_correct_f32")
CHURN = {"c0": dict(), "c1": dict(s_churn=1.0, s_noise=1.003), "cw": dict(s_churn=40.0, s_tmin=0.05, s_tmax=10.0, s_noise=1.0)}  # as the golden script
RUNS = (("euler", "c1"), ("euler", "cw"), ("heun", "c0"), ("heun", "cw"))
CLASSES = {"euler": "EulerEDMSampler", "heun": "HeunEDMSampler"}


def load():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "sampler_edm.npz")).items()}


def stored_noise(z):
    """the golden script's draw: row k of z at the k-th call"""
    calls = iter(range(z.shape[0]))
    return lambda x: z[next(calls)].to(x.device).expand_as(x).clone()


def build(solver, guider, **churn):
    """by dotted path through instantiate_from_config, as the YAML's sampler_config does"""
    from sgm.util import instantiate_from_config
    den = instantiate_from_config({"target": "sgm.modules.diffusionmodules.denoiser.DiscreteDenoiser", "params": {
        "num_idx": 1000, "weighting_config": {"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        "scaling_config": {"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, "discretization_config": DISC}})
    smp = instantiate_from_config({"target": "sgm.modules.diffusionmodules.sampling." + CLASSES[solver], "params": dict(
        num_steps=50, discretization_config=DISC, guider_config=guider, device="cpu", **churn)})
    return den, smp


def close(got, want):
    return torch.allclose(got, want, atol=2e-5, rtol=1e-5)


# ================================================================================================ 1: the classes
@pytest.mark.parametrize("solver,tag", RUNS)
@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
@pytest.mark.parametrize("steps", [12, 4])
def test_classes_walk_the_reference_trajectory_with_every_intermediate(name, steps, solver, tag):
    """The classes, built by the reference's dotted path: __call__ returns (x, rgb_list) and lands on the reference's final latent; driven
    step by step through sampler_step with the reference's gamma they reproduce every intermediate x (stored for the 12-step runs) and
    hand the denoiser the recorded sigmas in the recorded order: 2n - 1 calls for Heun, none after the last predictor.  Bar: the one
    test_euler_a_cpu.py::close holds.  Plain Euler differs from every golden by more than 1e-2 of its maximum."""
    from cd360 import sampler as S
    g = load()
    c, uc = conds(g)
    den, smp = build(solver, GUIDERS[name], **CHURN[tag])
    assert type(smp) is getattr(S, CLASSES[solver]) and isinstance(smp, S.EulerEDMSampler) and callable(smp.noise_sampler) and smp.seed is None
    seen = []

    def denoiser(inp, s, cc):
        seen.append(s[0].clone())
        return den(row_network, inp, s, cc)

    key = f"{solver}_{name}_{steps}_{tag}"
    want = g[key]
    smp.noise_sampler = stored_noise(g["z"])
    res, rgb = smp(denoiser, g["x"].clone(), c, uc=uc, num_steps=steps)
    print(key, "final vs the reference, max abs:", float((res - want).abs().max()), "of max", float(want.abs().max()))
    assert close(res, want) and rgb is not None
    dsig = g[f"{solver}_{steps}_{tag}_dsig"]
    assert len(seen) == dsig.numel() == (2 * steps - 1 if solver == "heun" else steps)
    assert torch.allclose(torch.stack(seen), dsig, rtol=1e-6, atol=0)
    smp.noise_sampler = stored_noise(g["z"])
    x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(g["x"].clone(), c, uc, steps)
    assert num_sigmas == steps + 1
    for i in range(steps):
        gamma = smp.gamma_of(sigmas[i], steps)
        assert gamma == pytest.approx(float(g[f"churn_{steps}_{tag}"][i, 0]), rel=1e-6)
        x, _ = smp.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc=ucond, gamma=gamma)
        if steps == 12:
            assert close(x, g[key + "_x"][i]), (key, i)
    assert torch.equal(x, res)
    eul = S.EulerEDMSampler(discretization_config=DISC, num_steps=50, guider_config=GUIDERS[name], device="cpu")
    plain, _ = eul(lambda inp, s, cc: den(row_network, inp, s, cc), g["x"].clone(), c, uc=uc, num_steps=steps)
    gap = float((plain - want).abs().max() / want.abs().max())
    print(key, "plain Euler vs the golden, rel:", gap)
    assert gap > 1e-2


@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
def test_unchurned_euler_keeps_its_arithmetic(name):
    """s_churn = 0: the class lands on tests/golden/sampler.npz at that file's bar (test_sampler_cpu.py), and is BIT-equal to the parent
    commit's arithmetic -- d = (x - denoised) / sigma, x + (sigma_next - sigma) d -- restated here; nothing is drawn."""
    from cd360 import sampler as S
    g = load()
    c, uc = conds(g)
    den, smp = build("euler", GUIDERS[name])
    assert (smp.s_churn, smp.s_tmin, smp.s_tmax, smp.s_noise) == (0.0, 0.0, float("inf"), 1.0)
    smp.noise_sampler = None  # never called
    denoiser = lambda inp, s, cc: den(row_network, inp, s, cc)  # noqa: E731
    got, _ = smp(denoiser, g["x"].clone(), c, uc=uc, num_steps=12)
    x, s_in, sigmas, n, cond, ucond = smp.prepare_sampling_loop(g["x"].clone(), c, uc, 12)
    for i in range(n - 1):
        s, sn = s_in * sigmas[i], s_in * sigmas[i + 1]
        denoised, _ = smp.denoise(x, denoiser, s, cond, ucond)
        x = x + S.append_dims(sn - s, x.ndim) * ((x - denoised) / S.append_dims(s, x.ndim))
    assert torch.equal(got, x)
    from test_sampler_cpu import dummy_network
    old = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "sampler.npz")).items()}
    oc, ouc = conds(old)
    res, rgb = smp(lambda inp, s, cc: den(dummy_network, inp, s, cc), old["x"].clone(), oc, uc=ouc, num_steps=12)
    assert torch.allclose(res, old[name], atol=2e-5, rtol=1e-5) and rgb is not None  # (test_full_trajectories_match_reference's bar)


def test_constructor_noise_sampler_seed_and_step_word():
    """seed=None: noise_sampler draws torch.randn_like (the reference's default).  seed=<int>: the library's generator, GPU tensors only -- a
    host tensor raises like every operator.  The step counter counts every step, drawn or not, and restarts with the loop."""
    from cd360 import _lib
    from cd360.sampler import EulerEDMSampler, HeunEDMSampler
    g = load()
    c, uc = conds(g)
    for cls in (EulerEDMSampler, HeunEDMSampler):
        smp = cls(discretization_config=DISC, num_steps=4, guider_config=GUIDERS["cfg3"], device="cpu", s_churn=40.0, s_tmin=0.05, s_tmax=10.0)
        torch.manual_seed(3)
        a = smp.noise_sampler(g["x"])
        torch.manual_seed(3)
        assert torch.equal(a, torch.randn_like(g["x"])) and smp.seed is None
        seeded = cls(discretization_config=DISC, num_steps=4, guider_config=GUIDERS["cfg3"], device="cpu", s_churn=1.0, seed=7)
        assert seeded.seed == 7
        with pytest.raises(_lib.Cd360Error):
            seeded.noise_sampler(g["x"])
        den, _ = build("euler", GUIDERS["cfg3"])
        words = []
        smp.noise_sampler = lambda x: (words.append(smp._step), torch.zeros_like(x))[1]  # noqa: B023
        smp(lambda inp, s, cc: den(row_network, inp, s, cc), g["x"].clone(), c, uc=uc, num_steps=4)
        assert words == [1, 2, 3] and smp._step == 4  # row 0 lies outside the window: the first draw carries step word 1
        smp.prepare_sampling_loop(g["x"].clone(), c, uc, 4)
        assert smp._step == 0


# ================================================================================================ 2: the tables
@pytest.mark.parametrize("tag", ["c0", "c1", "cw"])
@pytest.mark.parametrize("steps", [12, 4])
def test_edm_tables_match_the_reference(steps, tag):
    """edm_tables against the (gamma, sigma_hat, noise_std) the reference computed per step: rtol 1e-6, atol 0 (host vector math).  Exact
    where the value is a decision: gamma == 0 rows hold noise_std == 0 and sigma_hat == sigma; the last corr_tab row has sigma_next == 0;
    column 3 of edm_tab is DiscreteDenoiser.possibly_quantize_sigma(sigma_hat), column 2 its c_in; row 0 of cw is un-churned; with
    s_churn = 0 column 3 equals column 0 bitwise (the schedule lies on the grid)."""
    from cd360 import sampler as S
    g = load()
    den = S.DiscreteDenoiser()
    sig = S.LegacyDDPMDiscretization()(steps)
    kw = CHURN[tag]
    edm, corr, churn = S.edm_tables(sig, den, **kw)
    for t in (edm, corr, churn):
        assert t.shape == (steps, 4) and t.dtype == torch.float32 and t.device.type == "cpu" and t.is_contiguous() and torch.isfinite(t).all()
    if tag != "c0":
        want = g[f"churn_{steps}_{tag}"]
        assert tuple(want.shape) == (steps, 4)
        for col, (got, ref) in {"gamma": (churn[:, 0], want[:, 0]), "sigma_hat": (edm[:, 0], want[:, 1]), "noise_std": (churn[:, 1], want[:, 2])}.items():
            print(steps, tag, col, "vs the reference, max rel:", float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max()))
            assert torch.allclose(got, ref, rtol=1e-6, atol=0), col
        assert torch.equal(churn[:, 1] > 0, want[:, 3] > 0)  # the rows that drew
    zero = churn[:, 0] == 0
    assert torch.equal(churn[zero, 1], torch.zeros(int(zero.sum()))) and torch.equal(edm[zero, 0], sig[:-1][zero])
    assert bool((churn[~zero, 1] > 0).all()) and bool((edm[~zero, 0] > sig[:-1][~zero]).all())
    assert torch.equal(churn[:, 2], torch.full((steps,), float(kw.get("s_noise", 1.0)))) and torch.equal(churn[:, 3], torch.zeros(steps))
    assert torch.equal(edm[:, 1], sig[1:]) and torch.equal(corr[:, 0], sig[1:]) and torch.equal(corr[:, 1], sig[1:]) and corr[-1, 0] == 0
    assert torch.equal(edm[:, 3], den.possibly_quantize_sigma(edm[:, 0])) and torch.equal(corr[:, 3], den.possibly_quantize_sigma(corr[:, 0]))
    assert torch.equal(edm[:, 2], den.scaling(edm[:, 3])[2]) and torch.equal(corr[:, 2], den.scaling(corr[:, 3])[2])
    assert torch.equal(corr[:-1, 3], sig[1:-1])  # sigma_next lies on the grid; the last row snaps 0 to the grid's smallest entry
    assert corr[-1, 3] == den.sigmas.min()
    if tag == "c0":
        assert bool(zero.all()) and torch.equal(edm[:, 3], edm[:, 0]) and torch.equal(edm[:, 0], sig[:-1])
    if tag == "cw":
        assert bool(zero[0]) and not bool(zero[1:].all()) and float(churn[:, 0].max()) == float(torch.tensor(2 ** 0.5 - 1))
        assert edm[0, 3] == edm[0, 0]
    if tag == "c1":
        assert not bool(zero.any()) and bool((edm[:, 3] != edm[:, 0]).any())
        assert edm[0, 3] == sig[0] and edm[0, 0] > sig[0]  # row 0: sigma_hat lies above the grid and snaps back to sigma_max


# ================================================================================================ 3: the product step functions
def draw_rows(g, steps, tag):
    """step -> the row of z the reference drew there (the k-th draw took row k), None where it drew nothing"""
    if tag == "c0":
        return [None] * steps
    drew, rows, k = g[f"churn_{steps}_{tag}"][:, 3] > 0, [], 0
    for i in range(steps):
        rows.append(k if drew[i] else None)
        k += int(drew[i])
    return rows


def run_product_steps(g, solver, name, dev, fused, tag, steps=12):
    """The trajectory through the product's step functions (cd360.sampler.fused_cfg_edm_euler_step / fused_cfg_heun_step: what cd360/job.py
    launches per step) on the tables, with the golden's stored z as the noise, around the golden's network; returns (final x, [x_i])."""
    from cd360 import sampler as S
    den = S.DiscreteDenoiser().to(dev)
    guider = S.ScheduledCFGImgTextRef(7.5, 3.5) if name == "cfg3" else S.VanillaCFGImgRef(7.5)
    c, uc = conds(g, dev)
    x = g["x"].to(dev)
    _, _, cond = guider.prepare_inputs(x, x.new_ones(x.shape[0]), c, uc)
    sigmas = S.LegacyDDPMDiscretization()(steps, device=dev)
    edm, corr, churn = (t.to(dev) for t in S.edm_tables(sigmas, den, **CHURN[tag]))
    z, rows = g["z"].to(dev), draw_rows(g, steps, tag)
    x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)
    network = lambda x_in, c_noise: row_network(x_in, c_noise, cond)[0]  # noqa: E731
    xs = []
    for i in range(steps):
        noise = None if rows[i] is None else z[rows[i]]
        if solver == "euler":
            x = S.fused_cfg_edm_euler_step(den, network, x, edm[i], churn[i], guider, noise=noise, fused=fused)
        else:
            x = S.fused_cfg_heun_step(den, network, x, edm[i], corr[i], churn[i], guider, noise=noise, fused=fused)
        xs.append(x)
    return x, xs


@pytest.mark.parametrize("solver,tag", RUNS)
def test_product_step_functions_walk_the_reference_trajectory_for_both_guiders(solver, tag):
    """fused_cfg_edm_euler_step / fused_cfg_heun_step (fused=False) -- the plain-torch chain in the kernels' order, on the TABLES, the noise
    handed in as a tensor -- over 12 steps against the reference, every intermediate; and the two guiders' results differ."""
    g = load()
    finals = {}
    for name in ("cfg3", "cfg2"):
        res, xs = run_product_steps(g, solver, name, "cpu", fused=False, tag=tag)
        key = f"{solver}_{name}_12_{tag}"
        print(key, "table-form CPU trajectory vs the reference, max abs:", float((res - g[key]).abs().max()))
        assert close(res, g[key])
        for i in range(12):
            assert close(xs[i], g[key + "_x"][i]), (key, i)
        finals[name] = res
    assert float((finals["cfg3"] - finals["cfg2"]).abs().max()) > 1e-2 * float(finals["cfg3"].abs().max())


def test_flat_forms_on_their_edge_rows():
    """The predictor with sq == sigma_hat is cfg_euler_update bit for bit; the corrector on a sigma_next = 0 row hands back x_e without
    eps2 or d; a churned row without noise, and a wrong branch count, raise."""
    import weights as W
    from cd360 import sampler as S
    x, eps = W.tensor("x", (2, 4, 8, 8), seed=3), W.tensor("eps", (6, 4, 8, 8), seed=3)
    sig = S.LegacyDDPMDiscretization()(4)
    edm, corr, churn = S.edm_tables(sig, S.DiscreteDenoiser(), s_churn=1.0)
    plain, _, _ = S.edm_tables(sig, S.DiscreteDenoiser())
    for i in range(4):
        xe, d = S.cfg_edm_predict(x, eps, plain[i], 7.5, 3.5, fused=False)
        assert torch.equal(xe, S.cfg_euler_update(x, eps, sig[i].reshape(1), sig[i + 1].reshape(1), 7.5, 3.5, fused=False))
        assert torch.equal(S.cfg_edm_predict(x, eps, plain[i], 7.5, 3.5, fused=False, want_dir=False)[0], xe)
    xe, d = S.cfg_edm_predict(x, eps, edm[3], 7.5, 3.5, fused=False)
    assert torch.equal(S.cfg_edm_correct(x, xe, None, None, edm[3], corr[3], 7.5, 3.5, fused=False), xe)
    assert not torch.equal(S.cfg_edm_correct(x, xe, d, eps, edm[1], corr[1], 7.5, 3.5, fused=False), xe)
    assert S.edm_churn(x, plain.new_zeros(4), None, fused=False) is x and S.edm_churn(x, None) is x
    with pytest.raises(ValueError):
        S.edm_churn(x, churn[0], None, fused=False)
    with pytest.raises(ValueError):
        S.cfg_edm_predict(x, eps, edm[0], 7.5, None, fused=False)  # six rows, two branches


# ================================================================================================ 4: header and table
def test_edm_header_matches_the_fourth_signature_table():
    """include/cd360_edm.h <=> cd360._lib.EDM_SIGNATURES, by the rule test_stochastic_header_matches_the_third_signature_table holds (every
    `cd360_...(` word, comments included); the library exports the five symbols, typed; no older table holds the new names and no older
    header names them; null pointers are refused on the host (no GPU needed)."""
    from cd360 import _lib
    older = ("cd360_hip.h", "cd360_solvers.h", "cd360_stochastic.h")
    mismatch, in_tables, in_headers, mistyped, lib = SC.check_header_matches_table("cd360_edm.h", _lib.EDM_SIGNATURES, NEW, older)
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    nul = ctypes.c_void_p(None)
    assert lib.cd360_edm_churn_f32(nul, nul, nul, nul, nul, 1, 16, nul) == -1
    assert lib.cd360_cfg_edm_predict_cl(nul, nul, nul, nul, 7.5, 3.5, nul, nul, 1, 16, 4, nul) == -1
    assert lib.cd360_cfg_edm_predict_f32(nul, nul, nul, 7.5, 3.5, nul, nul, 16, nul) == -1
    assert lib.cd360_cfg_edm_correct_cl(nul, nul, nul, nul, nul, nul, nul, 7.5, 3.5, 1, 16, 4, nul) == -1
    assert lib.cd360_cfg_edm_correct_f32(nul, nul, nul, nul, nul, nul, 7.5, 3.5, nul, 16, nul) == -1


# ================================================================================================ 5: the job constructor
def test_job_sampler_takes_heun_and_churn_and_refuses_an_unknown_solver():
    from cd360 import job, sampling, solvers
    from test_cfg2_cpu import _pose_net
    net, _ = _pose_net(1)
    sampling.enable_reference_sampling(net, [0, 2])
    g = torch.Generator().manual_seed(1)
    ctx, y = torch.randn(6, 7, 16, generator=g), torch.randn(6, 12, generator=g)
    pose = [object() for _ in range(6)]
    assert job.Sampler.SOLVERS == ("euler", "dpmpp2m", "euler_a") == tuple(solvers.SOLVERS) and job.Sampler.EDM_SOLVERS == ("heun",)
    assert set(solvers.EDM_SOLVERS) == {"euler", "heun"}
    smp = job.Sampler(net, pose, ctx, y, 12, solver="heun")
    assert smp.solver == "heun" and smp._solver is solvers.EDM_SOLVERS["heun"] and (smp.s_churn, smp.s_tmin, smp.s_tmax) == (0.0, 0.0, float("inf"))
    with pytest.raises(ValueError):
        smp.reseed(1)  # un-churned Heun draws no noise
    plain = job.Sampler(net, pose, ctx, y, 12)
    assert plain._solver is solvers.SOLVERS["euler"]  # s_churn = 0: the object it has always run
    with pytest.raises(ValueError):
        plain.reseed(1)
    for solver in ("euler", "heun"):
        smp = job.Sampler(net, pose, ctx, y, 12, solver=solver, s_churn=40.0, s_tmin=0.05, s_tmax=10.0, s_noise=1.003, seed=2 ** 63 + 12345,
                          noise_streams=[0, 1])
        assert smp._solver is solvers.EDM_SOLVERS[solver] and (smp.s_churn, smp.s_tmin, smp.s_tmax, smp.s_noise) == (40.0, 0.05, 10.0, 1.003)
        assert (smp.seed, smp.noise_streams) == (2 ** 63 + 12345, [0, 1])
        smp.reseed(5)
        assert smp.seed == 5
        smp.set_noise_streams([1, 0])
        assert smp.noise_streams == [1, 0]
        with pytest.raises(ValueError):
            smp.set_noise_streams([0, 1, 2])  # bs = 2 replay rows
    with pytest.raises(ValueError) as e:
        job.Sampler(net, pose, ctx, y, 12, solver="nope")
    assert all(n in str(e.value) for n in ("euler", "dpmpp2m", "euler_a", "heun"))
    sampling.disable_reference_sampling(net)
