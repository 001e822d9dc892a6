"""Karras and listed sigma schedules, the parts that need no GPU: EDMDiscretization against the REFERENCE's own class
(tests/golden/schedules.npz, written by tests/golden/make_schedule_golden.py), the un-captured Euler trajectory off the denoiser's grid
against the reference's, ListDiscretization, on_grid, and what the job sampler selects, builds and refuses per schedule.  CPU only;
tests/test_schedules_gpu.py holds the captured job."""
import pytest
import torch

import schedule_cases as KC
from schedule_cases import K3, K80, SETS
from test_sampler_cpu import dummy_network
from test_sampler_cpu import load as load_sampler_golden

GUIDER3 = {"target": "sgm.modules.diffusionmodules.guiders.ScheduledCFGImgTextRef", "params": {"scale": 7.5, "scale_im": 3.5}}


# ================================================================================================ 1: the discretisation
def test_edm_discretization_resolves_from_yaml_and_matches_the_reference():
    """The YAML target resolves through the module alias; every parameter set equals the reference's output, with and without the appended
    zero, under the rule test_sampler_cpu holds the legacy sigmas to (a stored power: at most one float32 ulp); flip and do_append_zero
    behave as for LegacyDDPMDiscretization."""
    from sgm.util import instantiate_from_config
    from cd360 import sampler as S
    g = KC.load()
    assert isinstance(instantiate_from_config({"target": KC.EDM}), S.EDMDiscretization)
    d = instantiate_from_config({"target": KC.EDM})
    assert (d.sigma_min, d.sigma_max, d.rho) == (0.002, 80.0, 7.0)
    for k, s in enumerate(SETS):
        disc = instantiate_from_config(KC.config(s))
        got0, got = disc(s[0]), disc(s[0], do_append_zero=False)
        assert got0.dtype == torch.float32 and got0.shape == (s[0] + 1,) and float(got0[-1]) == 0.0 and torch.equal(got0[:-1], got)
        assert KC.one_ulp(got, g[f"sig_{k}"]) and KC.one_ulp(got0, g[f"sig0_{k}"]), (s, got0, g[f"sig0_{k}"])
        assert bool((got[1:] < got[:-1]).all())
        legacy = S.LegacyDDPMDiscretization()
        for kw in (dict(flip=True), dict(flip=True, do_append_zero=False)):
            assert torch.equal(disc(s[0], **kw), torch.flip(disc(s[0], do_append_zero=kw.get("do_append_zero", True)), (0,)))
            assert legacy(s[0], **kw).shape == disc(s[0], **kw).shape
        assert float(disc(s[0], flip=True)[0]) == 0.0
    assert [round(float(v), 4) for v in KC.karras(K80)(4)[:4]] == [80.0, 9.7232, 0.47, 0.002]


# ================================================================================================ 2: the un-captured trajectory
def test_uncaptured_euler_walks_the_reference_trajectory_off_the_grid():
    """EulerEDMSampler built from the YAML with the (4, 0.002, 80, 7) schedule around the toy network of tests/golden/sampler.npz: the
    final latent of the reference's own class, at the bar test_sampler_cpu grants its on-grid trajectory (atol 2e-5, rtol 1e-5).  Every
    sigma is off the denoiser's grid (row 0 by a factor of five): c_out / c_in / c_noise from the snapped sigma, to_d and dt from the
    schedule's own."""
    from sgm.util import instantiate_from_config
    g, gs = KC.load(), load_sampler_golden()
    den = instantiate_from_config({"target": "sgm.modules.diffusionmodules.denoiser.DiscreteDenoiser", "params": {
        "num_idx": 1000, "weighting_config": {"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        "scaling_config": {"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"},
        "discretization_config": {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}}})
    smp = instantiate_from_config({"target": "sgm.modules.diffusionmodules.sampling.EulerEDMSampler", "params": {
        "num_steps": K80[0], "discretization_config": KC.config(K80), "guider_config": GUIDER3, "device": "cpu"}})
    c = {"crossattn": gs["c_crossattn"], "vector": gs["c_vector"]}
    uc = {"crossattn": gs["uc_crossattn"], "vector": gs["uc_vector"]}
    res, rgb = smp(lambda inp, s, cc: den(dummy_network, inp, s, cc), gs["x"].clone(), c, uc=uc)
    want = g["euler_k80"]
    print("off-grid Euler vs the reference: max abs", float((res - want).abs().max()), "of max", float(want.abs().max()))
    assert torch.allclose(res, want, atol=2e-5, rtol=1e-5), (res - want).abs().max()
    assert rgb is not None
    q = den.possibly_quantize_sigma(smp.discretization(4)[:4])
    assert [round(float(v), 4) for v in q] == [14.6146, 9.7015, 0.4696, 0.0292]


# ================================================================================================ 3: ListDiscretization
def test_list_discretization_round_trip_and_refusals():
    from cd360 import sampler as S
    vals = [14.6146, 2.5, 0.7, 0.03]
    disc = S.ListDiscretization(vals)
    want = torch.tensor(vals, dtype=torch.float32)
    assert torch.equal(disc(4, do_append_zero=False), want) and torch.equal(disc(4), torch.cat([want, torch.zeros(1)]))
    assert torch.equal(disc(4, flip=True), torch.flip(disc(4), (0,)))
    assert torch.equal(S.ListDiscretization(want)(4), disc(4)) and torch.equal(S.ListDiscretization(tuple(vals))(4), disc(4))
    with pytest.raises(ValueError):
        disc(5)  # another n
    with pytest.raises(ValueError):
        disc(3)
    for bad in ([0.7, 2.5, 0.03], [2.5, 2.5, 0.03], [2.5, 0.7, 0.0], [2.5, -0.7], [float("nan"), 0.5], [float("inf"), 0.5], []):
        with pytest.raises(ValueError):
            S.ListDiscretization(bad)


# ================================================================================================ 4: on_grid
def test_on_grid_tells_the_legacy_table_from_a_karras_schedule():
    from cd360 import sampler as S
    den = S.DiscreteDenoiser()
    legacy = S.LegacyDDPMDiscretization()
    for n in (10, 50, 1000):
        assert S.on_grid(legacy(n), den) is True and S.on_grid(legacy(n, do_append_zero=False), den) is True
    assert S.on_grid(S.ListDiscretization(legacy(10, do_append_zero=False))(10), den) is True
    assert S.on_grid(S.ListDiscretization(legacy(50)[[0, 7, 20, 49]])(4), den) is True  # any selection of table entries
    for s in SETS:
        sig = KC.karras(s)(s[0])
        assert S.on_grid(sig, den) is False, s
        q = den.possibly_quantize_sigma(sig[:-1])
        assert int((q != sig[:-1]).sum()) == s[0], (s, q, sig)  # every row off the grid
    one_off = legacy(10).clone()
    one_off[4] = torch.nextafter(one_off[4], torch.tensor(float("inf")))
    assert S.on_grid(one_off, den) is False


# ================================================================================================ 5, 6: the job constructor
@pytest.fixture(scope="module")
def stub():
    """The CPU stand-in of test_edm_cpu's constructor test: (net, pose, ctx, y) for 3 branches x 2 rows."""
    from cd360 import sampling
    from test_cfg2_cpu import _pose_net
    net, _ = _pose_net(1)
    sampling.enable_reference_sampling(net, [0, 2])
    g = torch.Generator().manual_seed(1)
    yield net, [object() for _ in range(6)], torch.randn(6, 7, 16, generator=g), torch.randn(6, 12, generator=g)
    sampling.disable_reference_sampling(net)


def test_job_sampler_selects_by_schedule_and_keeps_the_registries(stub):
    from cd360 import job, solvers
    from cd360 import sampler as S
    assert job.Sampler.SOLVERS == ("euler", "dpmpp2m", "euler_a") == tuple(solvers.SOLVERS) and job.Sampler.EDM_SOLVERS == ("heun",)
    assert set(solvers.EDM_SOLVERS) == {"euler", "heun"} and job.Sampler.HIGHORDER_SOLVERS == ("dpmpp2s_a", "lms") == tuple(solvers.HIGHORDER_SOLVERS)
    assert solvers.NAMES == ("euler", "dpmpp2m", "euler_a", "heun", "dpmpp2s_a", "lms")
    plain = job.Sampler(*stub, 12)
    assert plain._solver is solvers.SOLVERS["euler"] and plain.on_grid is True
    explicit = job.Sampler(*stub, 12, discretization=S.LegacyDDPMDiscretization())
    assert explicit._solver is solvers.SOLVERS["euler"] and explicit.on_grid is True and torch.equal(explicit.sigmas, plain.sigmas)
    listed = job.Sampler(*stub, 12, sigmas=plain.sigmas[:-1].tolist())
    assert listed._solver is solvers.SOLVERS["euler"] and listed.on_grid is True and torch.equal(listed.sigmas, plain.sigmas)
    for s in (K3, K80):
        smp = job.Sampler(*stub, s[0], discretization=KC.karras(s))
        assert smp._solver is solvers.EDM_SOLVERS["euler"] and smp.s_churn == 0 and smp.on_grid is False
        assert torch.equal(smp.sigmas, KC.karras(s)(s[0])) and not smp._solver.draws(smp)
        with pytest.raises(ValueError):
            smp.reseed(1)  # gamma = 0 everywhere: no noise
        assert job.Sampler(*stub, s[0], solver="heun", discretization=KC.karras(s))._solver is solvers.EDM_SOLVERS["heun"]
        assert job.Sampler(*stub, s[0], solver="dpmpp2m", discretization=KC.karras(s))._solver is solvers.SOLVERS["dpmpp2m"]
    assert solvers.select("euler") is solvers.SOLVERS["euler"] and solvers.select("euler", 0.0, True) is solvers.SOLVERS["euler"]
    assert solvers.select("euler", 0.0, on_grid=False) is solvers.EDM_SOLVERS["euler"] is solvers.select("euler", 1.0)


def test_dpmpp2m_tables_carry_the_snapped_sigma_for_c_out_alone(stub):
    """The host builder: column 0 = the denoiser's snap of sigma_i, columns 1..3 step_tab's; on the legacy schedule step_tab ITSELF.  The
    multipliers come from the schedule's own sigmas.  The un-staged route (all a CPU sampler has) carries the row in gq, off the grid only."""
    from cd360 import job, solvers
    from cd360 import sampler as S
    x = torch.zeros(2, 4, 8, 8)
    for s in (K3, K80):
        smp = job.Sampler(*stub, s[0], solver="dpmpp2m", discretization=KC.karras(s))
        step_tab, sq = smp.step_table()
        tab = S.dpmpp2m_cout_table(step_tab, smp.sigmas, smp.denoiser)
        q = smp.denoiser.possibly_quantize_sigma(smp.sigmas[:-1])
        assert tab is not step_tab and tab.shape == step_tab.shape and tab.dtype == torch.float32 and tab.is_contiguous()
        assert torch.equal(tab[:, 0], q) and torch.equal(q, sq) and torch.equal(tab[:, 1:], step_tab[:, 1:])
        assert torch.equal(step_tab[:, 0], smp.sigmas[:-1]) and int((tab[:, 0] != step_tab[:, 0]).sum()) == s[0]
        assert torch.equal(step_tab[:, 2], smp.denoiser.scaling(q)[2])  # stage-in's c_in comes from q already
        assert torch.equal(S.dpmpp2m_cout_table(step_tab, smp.sigmas, smp.denoiser, False), tab)
        smp._solver.build(smp, x)
        assert torch.equal(smp.cout_tab, tab) and torch.equal(smp.mult_tab, S.dpmpp2m_multipliers(smp.sigmas))
        assert not torch.equal(smp.mult_tab, S.dpmpp2m_multipliers(torch.cat([q, torch.zeros(1)])))
        assert smp._solver.rows_of(smp) == (("gm", "mult_tab"), ("gq", "cout_tab")) and torch.equal(smp.gq, tab[0])
        smp._solver.set_row(smp, 2)
        assert torch.equal(smp.gq, tab[2]) and torch.equal(smp.gm, smp.mult_tab[2]) and float(smp.gq[0]) == float(q[2])
    smp = job.Sampler(*stub, 12, solver="dpmpp2m")  # the legacy schedule
    step_tab, _ = smp.step_table()
    assert S.dpmpp2m_cout_table(step_tab, smp.sigmas, smp.denoiser) is step_tab
    assert S.dpmpp2m_cout_table(step_tab, smp.sigmas, smp.denoiser, True) is step_tab
    smp.step_tab = step_tab  # (as the staged sampler holds it before its solver's tables are built)
    smp._solver.build(smp, x)
    assert smp.cout_tab is smp.step_tab and smp._solver.rows_of(smp) == solvers.DPMPP2M.rows == (("gm", "mult_tab"),) and not hasattr(smp, "gq")


def test_off_grid_schedules_are_refused_where_one_sigma_serves_c_out_and_to_d(stub):
    from cd360 import job, solvers
    from cd360 import sampler as S
    legacy = S.LegacyDDPMDiscretization()(4, do_append_zero=False)
    for solver in KC.REFUSED:
        for s in (K3, K80):
            with pytest.raises(ValueError) as e:
                job.Sampler(*stub, s[0], solver=solver, discretization=KC.karras(s))
            assert all(n in str(e.value).replace(solver, "") for n in KC.OFF_GRID), str(e.value)
            with pytest.raises(ValueError):
                job.Sampler(*stub, s[0], solver=solver, sigmas=KC.karras(s)(s[0], do_append_zero=False).tolist())
        with pytest.raises(ValueError):
            solvers.select(solver, 0.0, on_grid=False)
        for kw in (dict(discretization=S.ListDiscretization(legacy)), dict(sigmas=legacy.tolist()), dict(sigmas=legacy)):
            smp = job.Sampler(*stub, 4, solver=solver, **kw)  # on the grid, whatever class produced it
            assert smp.on_grid is True and smp._solver is solvers.select(solver) and torch.equal(smp.sigmas[:-1], legacy)
    with pytest.raises(ValueError):
        job.Sampler(*stub, 4, discretization=KC.karras(K3), sigmas=legacy.tolist())
    for n in (3, 5):
        with pytest.raises(ValueError):
            job.Sampler(*stub, n, sigmas=legacy.tolist())
    with pytest.raises(ValueError):
        job.Sampler(*stub, 3, sigmas=[1.0, 2.0, 0.5])  # unsorted
