"""Karras and listed sigma schedules on the captured HIP sampling step: the job sampler with solver euler / heun / dpmpp2m on schedules whose
every sigma lies OFF the denoiser's grid, against the un-captured module route on the same schedule, through its graphs bit for bit, on
the un-staged route, and down to the images; the legacy schedule named explicitly gives the bits it always gave.  Needs an MI355X.

K3 = (4 steps, sigma_min 0.0292, sigma_max 14.6146, rho 3): inside the denoiser's table.  K80 = (4, 0.002, 80, 7), the reference's
defaults: the snapped sigma of row 0 is 0.18 of sigma_0, so a kernel that reads the wrong one of the two is off by a factor of five."""
import pytest
import torch

import sampler_cases as SC
import schedule_cases as KC
from sampler_cases import DEV, LATENT, POSES, SEED, STEPS

# The module-route yardstick of the solvers' own GPU files: the SAME comparison (captured job sampler against the un-captured module
# route, n_steps = 4, all 4 steps, latent 32 / 6 views, bs = 1) under plain EULER on the legacy schedule, measured with
# tools/solver_report.py, per branch count (tests/test_edm_gpu.py:24, tests/test_highorder_gpu.py:25, tests/test_dpmpp2m_gpu.py:17) ...
PARENT_EULER_JOB_VS_MODULE_REL = {3: 0.05488, 2: 0.06147}
# ... and what each solver's file grants its solver ON THE LEGACY SCHEDULE: Euler and Heun tests/test_edm_gpu.py:25 (times the figure of
# the branch count), DPM++ 2M tests/test_dpmpp2m_gpu.py:278 (twice the three-branch figure for both branch counts).  The kernels and the
# operation order per step are the legacy schedule's, so an off-grid schedule is granted the same bar and no more.
# Measured with tools/solver_report.py [--schedule karras:0.0292:14.6146:3 | karras:0.002:80:7] on one MI355X in the session of this
# change, relative to the module route's maximum:
#
#   solver                  legacy, parent commit   legacy, this change   K3          K80         bar
#   euler                   5.488e-2                5.488e-2              6.163e-2    6.768e-2    1.098e-1
#   heun                    7.385e-2                7.385e-2              7.021e-2    9.262e-2    2.195e-1
#   dpmpp2m                 6.085e-2                6.085e-2              7.420e-2    7.936e-2    1.098e-1
#   dpmpp2m, two branches   6.430e-2                6.430e-2              8.556e-2    --          1.098e-1
#
# No off-grid figure exceeds its solver's legacy bar: no bar is raised.  The un-staged route on K3 measured 0 / 0 / 1.020e-2.


def bar(solver, nb):
    if solver == "dpmpp2m":
        return 2 * PARENT_EULER_JOB_VS_MODULE_REL[3]
    return {"euler": 2, "heun": 4}[solver] * PARENT_EULER_JOB_VS_MODULE_REL[nb]


DISC = {}


def disc(name):
    """ONE discretisation object per schedule (sampler_cases.walk keys its cache on the keyword values)."""
    if name not in DISC:
        DISC[name] = KC.karras(KC.SCHEDULES[name])
    return DISC[name]


MODULES = {"euler": "EulerEDMSampler", "heun": "HeunEDMSampler", "dpmpp2m": "DPMPP2MSampler"}


def module_route(solver, name, nb, pose, ctx, y, x0):
    """sampler_cases.module_route with the solver's class built on the same discretization_config."""
    from cd360 import sampler as S
    mod = getattr(S, MODULES[solver])(num_steps=STEPS, guider_config=SC.guider_config(nb), device=DEV,
                                      discretization_config=KC.config(KC.SCHEDULES[name]))
    assert torch.equal(mod.discretization(STEPS, device=DEV), disc(name)(STEPS, device=DEV))
    return SC.module_route(SC.net(), mod, solver, nb, pose, ctx, y, x0, STEPS)


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_job():
    yield
    SC.release()


def _check_tables(smp, solver):
    """What the off-grid sampler holds: which table carries the snapped sigma for which kernel."""
    from cd360 import solvers
    q = smp.denoiser.possibly_quantize_sigma(smp.sigmas[:-1])
    assert smp.on_grid is False and int((q != smp.sigmas[:-1]).sum()) == STEPS
    assert torch.equal(smp.step_tab[:, 0], smp.sigmas[:-1]) and torch.equal(smp.step_tab[:, 2], smp.denoiser.scaling(q)[2])
    if solver == "dpmpp2m":
        assert smp._solver is solvers.SOLVERS["dpmpp2m"] and smp.cout_tab is not smp.step_tab
        assert torch.equal(smp.cout_tab[:, 0], q) and torch.equal(smp.cout_tab[:, 1:], smp.step_tab[:, 1:])
        from cd360 import sampler as S
        assert torch.equal(smp.mult_tab.cpu(), S.dpmpp2m_multipliers(smp.sigmas))
    else:
        assert smp._solver is solvers.EDM_SOLVERS[solver] and not smp.churned and not hasattr(smp, "seed_buf")
        assert torch.equal(smp.edm_tab[:, 0], smp.sigmas[:-1]) and torch.equal(smp.edm_tab[:, 1], smp.sigmas[1:]) and torch.equal(smp.edm_tab[:, 3], q)
        assert torch.equal(smp.edm_tab[:, 2], smp.step_tab[:, 2]) and torch.equal(smp.edm_temb, smp.temb_tab)
        assert torch.equal(smp.corr_tab[:-1, 3], q[1:]) and torch.equal(smp.corr_tab[:, 0], smp.sigmas[1:])


# ================================================================================================ 7: against the module route
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("solver,name,nb", [(s, k, 3) for k in ("K3", "K80") for s in KC.OFF_GRID] + [("dpmpp2m", "K3", 2)])
def test_off_grid_job_agrees_with_the_uncaptured_module_route(solver, name, nb):
    """Whole trajectory, n_steps = 4, all 4 steps: the same UNet under the solver's un-captured class + the guider + DiscreteDenoiser on the
    SAME discretization_config (the YAML's classes, eager: the denoiser snaps every sigma on the device, the class steps on the schedule's
    own) against the job sampler (captured, staged, the tables).  The two differ as on the legacy schedule -- by the staged input
    convolution rounding a few bf16 values to the other neighbour, amplified by 70 random-init blocks -- so the bar is the one the solver's
    own file grants this comparison on the legacy schedule (bar(), above).  A sampler that mixed the two sigmas up would miss it on K80 by
    far: c_out would be off by a factor of five on row 0.  Measured figures: the table above and DESIGN.md section 6.6."""
    from cd360 import job
    pose, ctx, y, x0 = SC.job(0, nb)
    smp = SC.sampler(pose, ctx, y, scale_im=3.5 if nb == 3 else 0, solver=solver, discretization=disc(name))
    got = job.sample_assigned(smp, [(pose, ctx, y, x0)], STEPS)[0]
    assert smp.staged and smp.graph is not None and smp.rgraph is not None and smp.branches == nb
    _check_tables(smp, solver)
    x = module_route(solver, name, nb, pose, ctx, y, x0)
    dev = float((got - x).abs().max() / x.abs().max())
    print(f"{solver} on {name}, {nb}-branch job vs module route, 4 steps: max abs", float((got - x).abs().max()), "rel", dev, "| bar", bar(solver, nb))
    assert torch.isfinite(got).all() and dev <= bar(solver, nb), (dev, bar(solver, nb))


# ================================================================================================ 8: through the captured graphs
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("solver", KC.OFF_GRID)
def test_off_grid_job_through_its_captured_graphs(solver):
    """Sampler(n_steps=4, use_graph=True, discretization=K3) over 3 poses x all 4 steps, as test_highorder_job_through_its_captured_graphs
    holds its solvers: all graphs captured and staged (Heun its third, for the sigma_next = 0 step), every pose bit-identical to a fresh
    graph-mode sampler's and to use_graph=False, and it is not the legacy walk."""
    from cd360 import job
    kw = dict(solver=solver, discretization=disc("K3"))
    latents, smp = SC.walk(**kw)
    assert latents.shape == (POSES, 4, LATENT, LATENT) and torch.isfinite(latents).all()
    assert smp.staged and smp.graph is not None and smp.rgraph is not None and (smp.lgraph is not None) == (solver == "heun")
    _check_tables(smp, solver)
    for p in range(POSES):
        pose, ctx, y, x0 = SC.job(p)
        fresh = job.sample_assigned(SC.sampler(pose, ctx, y, **kw), [(pose, ctx, y, x0)], STEPS)[0]
        assert torch.equal(fresh, latents[p:p + 1]), (p, float((fresh - latents[p:p + 1]).abs().max()))
        eager = job.sample_assigned(SC.sampler(pose, ctx, y, use_graph=False, **kw), [(pose, ctx, y, x0)], STEPS)[0]
        assert torch.equal(eager, latents[p:p + 1]), (p, float((eager - latents[p:p + 1]).abs().max()))
    legacy, _ = SC.walk(solver=solver)
    for p in range(POSES):
        assert float((legacy[p] - latents[p]).abs().max() / latents[p].abs().max()) > 1e-3, p


# ================================================================================================ 9: the un-staged route
def _restated(x, e, old, s, m, scale, scale_im):
    """tests/test_dpmpp2m_gpu.py::_restated: cd360_cfg_dpmpp2m_step_f32's expression in the kernel's order, one fp32 rounding per operation."""
    d0 = SC.combine(x, e, s, scale, scale_im)
    m1, m2, m3, m4 = m.unbind()
    dd = d0 if float(m4) == 0.0 else m3 * d0 - m4 * old
    return m1 * x - m2 * dd, d0


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("solver", KC.OFF_GRID)
def test_unstaged_route_serves_off_grid_schedules(solver):
    """With routes.no_stage the un-staged route carries K3 as well: graph mode equal to its own eager run, and against the module route
    under the bar of the staged comparison.  DPM++ 2M: the first step's result IS cd360_cfg_dpmpp2m_step_f32's expression restated in
    torch with q(sigma_0) as the scalar and row 0 of the multipliers of the schedule's own sigmas, bit for bit -- and is not that
    expression on sigma_0."""
    from cd360 import job, routes, sampling
    pose, ctx, y, x0 = SC.job(0)
    kw = dict(solver=solver, discretization=disc("K3"))
    with routes.override(no_stage=True):
        g_smp, e_smp = SC.sampler(pose, ctx, y, **kw), SC.sampler(pose, ctx, y, use_graph=False, **kw)
        assert not g_smp.staged and not e_smp.staged and e_smp.on_grid is False
        got_g = job.sample_assigned(g_smp, [(pose, ctx, y, x0)], STEPS)[0]
        got_e = job.sample_assigned(e_smp, [(pose, ctx, y, x0)], STEPS)[0]
        assert g_smp.graph is not None and torch.isfinite(got_g).all()
        assert torch.equal(got_g, got_e), float((got_g - got_e).abs().max())
        if solver == "dpmpp2m":
            first = e_smp.step(x0.clone(), 0)
            sampling.clear_rendered_feat(SC.net())
            eps = e_smp.eps(x0, 0)
            sampling.clear_rendered_feat(SC.net())
            q0 = e_smp.denoiser.possibly_quantize_sigma(e_smp.sigmas[:1])
            assert float(q0) != float(e_smp.sigmas[0]) and torch.equal(e_smp.cout_tab[0, :1], q0) and torch.equal(e_smp.gq[:1], q0)
            want, d0 = _restated(x0, eps, torch.zeros_like(x0), q0, e_smp.mult_tab[0], 7.5, 3.5)
            assert torch.equal(first, want), float((first - want).abs().max())
            assert torch.equal(e_smp.gd, d0)
            assert not torch.equal(first, _restated(x0, eps, torch.zeros_like(x0), e_smp.sigmas[:1], e_smp.mult_tab[0], 7.5, 3.5)[0])
    x = module_route(solver, "K3", 3, pose, ctx, y, x0)
    dev = float((got_g - x).abs().max() / x.abs().max())
    print(f"{solver} on K3, un-staged job vs module route, 4 steps: max abs", float((got_g - x).abs().max()), "rel", dev, "| bar", bar(solver, 3))
    assert dev <= bar(solver, 3), (dev, bar(solver, 3))


# ================================================================================================ 10: the legacy schedule, named
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_naming_the_legacy_schedule_changes_no_bit(solver):
    """Sampler(..., discretization=LegacyDDPMDiscretization()) over the 3-pose walk: the latents of the default construction, bit for bit,
    on the objects, tables and graphs the default runs on."""
    from cd360 import sampler as S
    from cd360 import solvers
    want, plain = SC.walk(solver=solver)
    got, smp = SC.walk(solver=solver, discretization=S.LegacyDDPMDiscretization())
    assert smp is not plain and smp.on_grid is True and plain.on_grid is True and torch.equal(smp.sigmas, plain.sigmas)
    assert smp._solver is solvers.SOLVERS[solver] is plain._solver and smp.lgraph is None and smp.graph is not None and smp.rgraph is not None
    if solver == "dpmpp2m":
        assert smp.cout_tab is smp.step_tab and plain.cout_tab is plain.step_tab
    assert torch.equal(smp.step_tab, plain.step_tab)
    assert torch.equal(got, want), float((got - want).abs().max())
    pose, ctx, y, x0 = SC.job(0)
    listed = SC.sampler(pose, ctx, y, solver=solver, sigmas=S.LegacyDDPMDiscretization()(STEPS, do_append_zero=False).tolist())
    assert listed.on_grid is True and listed._solver is plain._solver and KC.one_ulp(listed.sigmas.cpu(), plain.sigmas.cpu())


@pytest.mark.gpu
def test_the_devices_last_bit_moves_no_legacy_sigma_off_the_grid():
    """The denoiser's table is the HOST's evaluation of the legacy schedule; the device's square root differs from it in the last bit of
    some entries from 10 steps on (one of 12, ten of 50 on an MI355X).  on_grid is decided on the host's evaluation of the schedule, so
    the default construction keeps its solver objects at every step count, and the solvers an off-grid schedule is refused construct."""
    from cd360 import sampler as S
    from cd360 import solvers
    pose, ctx, y, _ = SC.job(0)
    for n in (12, 50):
        smp = SC.sampler(pose, ctx, y, n_steps=n, use_graph=False)
        assert smp.on_grid is True and smp._solver is solvers.SOLVERS["euler"] and smp.sigmas.is_cuda
        assert KC.one_ulp(smp.sigmas.cpu(), S.LegacyDDPMDiscretization()(n))
        for solver in KC.REFUSED:
            assert SC.sampler(pose, ctx, y, n_steps=n, use_graph=False, solver=solver)._solver is solvers.select(solver)


# ================================================================================================ 11: the start latent
@pytest.mark.gpu
@torch.no_grad()
def test_start_latent_scales_by_the_schedules_own_sigma_0():
    from cd360 import job, ops
    pose, ctx, y, _ = SC.job(0)
    smp = SC.sampler(pose, ctx, y, use_graph=False, solver="dpmpp2m", discretization=disc("K80"))
    sig0 = disc("K80")(STEPS, device=DEV)[0]
    scale = torch.sqrt(1.0 + sig0 ** 2.0).float().reshape(1)
    assert abs(float(scale) - (1 + 80.0 ** 2) ** 0.5) < 1e-3
    got = job.start_latent(smp, LATENT, LATENT, SEED)
    assert torch.equal(got, ops.start_noise(SC.seed_t(SEED), None, scale, 1, LATENT, LATENT))
    assert 60.0 < float(got.std()) < 100.0


# ================================================================================================ 12: down to the images
@pytest.mark.gpu
@torch.no_grad()
def test_sample_images_on_a_karras_schedule():
    """Two poses, DPM++ 2M on K3, x0 = None: sample_images returns the uint8 images first_stage.decode_u8 gives on sample_poses' latents
    from the same start latent (the narrow first stage of tests/test_images_gpu.py)."""
    from cd360 import job as J
    from test_images_gpu import _first_stage
    fs, _ = _first_stage()
    held = {}

    def make_sampler(pose, ctx, y):
        if "smp" not in held:
            held["smp"] = SC.sampler(pose, ctx, y, solver="dpmpp2m", discretization=disc("K3"))
        else:
            held["smp"].retarget(pose, ctx, y)
        return held["smp"]

    images, mine = J.sample_images(make_sampler, lambda p: SC.job(p)[:3] + (None,), 2, STEPS, fs, seed=SEED, latent_hw=(LATENT, LATENT))
    assert mine == [0, 1] and images.shape == (2, 4 * LATENT, 4 * LATENT, 3) and images.dtype == torch.uint8
    assert held["smp"].on_grid is False
    x0 = J.start_latent(held["smp"], LATENT, LATENT, SEED)
    latents, _ = J.sample_poses(make_sampler, lambda p: SC.job(p)[:3] + (x0,), 2, STEPS)
    assert torch.isfinite(latents).all()
    want = fs.decode_u8(latents)
    assert torch.equal(images, want), int((images != want).sum())
    assert not torch.equal(images[0], images[1]) and int((images > 0).sum()) > 0 and int((images < 255).sum()) > 0
