#!/usr/bin/env python
"""Euler against DPM++ 2M, ancestral Euler, Heun, churned Euler, DPM++ 2S ancestral and linear multistep through cd360.job.Sampler: the figures of DESIGN.md's sections on the
further solvers.  Calls the job sampler directly (bench.py keeps measuring the Euler headline).

  --solver euler|dpmpp2m|euler_a|heun|dpmpp2s_a|lms   which step (euler also runs on a checkout that predates the `solver` argument: --repo
                           PATH imports that checkout); euler_a, dpmpp2s_a and every churned run: seed 360 on both routes
  --eta                    the eta of the ancestral solvers' constructors, for --solver euler_a and dpmpp2s_a (default 1.0)
  --order                  the order of LinearMultistepSampler's constructor, for --solver lms (default 4)
  --s-churn / --s-tmin / --s-tmax / --s-noise   the churn of EDMSampler's constructor, for --solver euler and heun (default: none)
  --branches 2|3           which guider
  --schedule legacy|karras:<min>:<max>:<rho>|list:<v,v,...>   the sigma schedule of BOTH routes (default legacy: LegacyDDPMDiscretization, also
                           on a checkout that predates the option); karras = EDMDiscretization, list = ListDiscretization (n_steps values).
                           Off the denoiser's grid the job serves --solver euler, heun and dpmpp2m
  --what deviation         n_steps = 4, all 4 steps at latent 32 / 6 views: the captured job sampler against the un-captured module route
                           (cd360.sampler's EulerEDMSampler / DPMPP2MSampler / EulerAncestralSampler / HeunEDMSampler / DPMPP2SAncestralSampler /
                           LinearMultistepSampler + the guider + DiscreteDenoiser around the same UNet, eager),
                           max |difference| / max |module-route latent|: the yardstick and the figure of
                           tests/test_dpmpp2m_gpu.py::test_dpmpp2m_job_agrees_with_the_uncaptured_module_route and
                           tests/test_euler_a_gpu.py::test_euler_a_job_agrees_with_the_uncaptured_module_route and
                           tests/test_edm_gpu.py::test_edm_job_agrees_with_the_uncaptured_module_route and
                           tests/test_highorder_gpu.py::test_highorder_job_agrees_with_the_uncaptured_module_route
  --what timing            steady-step replay time of the graph sampler under Euler AND --solver in this process (median of --reps replays after
                           warm-up, interleaved), at --latent / --refs (default 128 / 50); a Heun steady step holds two
                           evaluations (compare with two Euler steps), as does a DPM++ 2S step; a churned Euler step one launch more than
                           the plain one
Prints one JSON line per figure."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--solver", default="dpmpp2m", choices=("euler", "dpmpp2m", "euler_a", "heun", "dpmpp2s_a", "lms"))
ap.add_argument("--eta", type=float, default=1.0)
ap.add_argument("--order", type=int, default=4)
ap.add_argument("--s-churn", type=float, default=0.0)
ap.add_argument("--s-tmin", type=float, default=0.0)
ap.add_argument("--s-tmax", type=float, default=float("inf"))
ap.add_argument("--s-noise", type=float, default=1.0)
ap.add_argument("--branches", type=int, default=3, choices=(2, 3))
ap.add_argument("--schedule", default="legacy")
ap.add_argument("--what", default="deviation", choices=("deviation", "timing"))
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--refs", type=int, default=50)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
ROOT = os.path.abspath(args.repo)
sys.path[:0] = [ROOT, os.path.join(ROOT, "custom-diffusion360_amd")]
import torch  # noqa: E402
import bench  # noqa: E402
from cd360 import job, sampling, synth  # noqa: E402
from cd360 import sampler as S  # noqa: E402

DEV, BF, NB = "cuda", torch.bfloat16, args.branches
SCALE_IM = 3.5 if NB == 3 else 0
SEED = 360
CHURN = dict(s_churn=args.s_churn, s_tmin=args.s_tmin, s_tmax=args.s_tmax, s_noise=args.s_noise) if args.s_churn > 0 else {}
if CHURN and args.solver not in ("euler", "heun"):
    ap.error("--s-churn applies to --solver euler and heun")
LABEL = args.solver + ("_churn" if CHURN else "")


def schedule():
    """--schedule -> (the discretisation object for job.Sampler, the discretization_config of the un-captured classes); (None, None): legacy."""
    kind, _, rest = args.schedule.partition(":")
    try:
        if kind == "legacy" and not rest:
            return None, None
        if kind == "karras":
            lo, hi, rho = (float(v) for v in rest.split(":"))
            params = {"sigma_min": lo, "sigma_max": hi, "rho": rho}
            return S.EDMDiscretization(**params), {"target": "sgm.modules.diffusionmodules.discretizer.EDMDiscretization", "params": params}
        if kind == "list":
            vals = [float(v) for v in rest.split(",")]
            return S.ListDiscretization(vals), {"target": "sgm.modules.diffusionmodules.discretizer.ListDiscretization", "params": {"sigmas": vals}}
    except ValueError as e:
        ap.error(f"--schedule {args.schedule}: {e}")
    ap.error("--schedule takes legacy, karras:<min>:<max>:<rho> or list:<v,v,...>")


DISC, DISC_CFG = schedule()
SCHED = {} if DISC_CFG is None else {"discretization_config": DISC_CFG}  # (for the un-captured classes)


def one_pose(p, latent, refs):
    cam = synth.pose_batch(1, refs, seed=100 + p, n_train=50)[0]
    g = torch.Generator(device=DEV).manual_seed(7 + p)
    ctx = torch.randn(2, 77, 2048, generator=g, device=DEV).to(BF)
    y = torch.randn(2, 2816, generator=g, device=DEV).to(BF)
    return cam, ctx, y, torch.randn(1, 4, latent, latent, generator=g, device=DEV)


def batch(p, latent, refs):
    """The job's inputs for pose p: NB camera batches, ctx / y = [uc | (uc) | c]."""
    cam, c, v, x = one_pose(p, latent, refs)
    return [cam] * NB, torch.cat([c[0:1]] * (NB - 1) + [c[1:2]]), torch.cat([v[0:1]] * (NB - 1) + [v[1:2]]), x


def make(net, pose, ctx, y, n_steps, solver, churn=None):
    kw = {} if solver == "euler" else {"solver": solver}  # (a checkout that predates the argument serves Euler)
    if solver in ("euler_a", "dpmpp2s_a") or churn:
        kw["seed"] = SEED
    if solver in ("euler_a", "dpmpp2s_a") and args.eta != 1.0:
        kw["eta"] = args.eta
    if solver == "lms":
        kw["order"] = args.order
    kw.update(churn or {})
    if DISC is not None:
        kw["discretization"] = DISC
    return job.Sampler(net, pose, ctx, y, n_steps, scale_im=SCALE_IM, use_graph=True, **kw)


def out(**kw):
    print(json.dumps(dict(branches=NB, **kw)), flush=True)


@torch.no_grad()
def deviation():
    latent, refs, steps = 32, 6, 4
    net = bench.build_model(latent, refs, 50, DEV)
    pose, ctx, y, x0 = batch(0, latent, refs)
    smp = make(net, pose, ctx, y, steps, args.solver, CHURN)
    got = job.sample_assigned(smp, [(pose, ctx, y, x0)], steps)[0]
    gcfg = ({"target": "sgm.modules.diffusionmodules.guiders.VanillaCFGImgRef", "params": {"scale": 7.5}} if NB == 2 else
            {"target": "sgm.modules.diffusionmodules.guiders.ScheduledCFGImgTextRef", "params": {"scale": 7.5, "scale_im": 3.5}})
    if args.solver in ("euler_a", "dpmpp2s_a"):
        cls = S.EulerAncestralSampler if args.solver == "euler_a" else S.DPMPP2SAncestralSampler
        mod = cls(eta=args.eta, num_steps=steps, guider_config=gcfg, device=DEV, seed=SEED, **SCHED)
    elif args.solver == "lms":
        mod = S.LinearMultistepSampler(order=args.order, num_steps=steps, guider_config=gcfg, device=DEV, **SCHED)
    elif args.solver == "heun" or CHURN:
        mod = (S.HeunEDMSampler if args.solver == "heun" else S.EulerEDMSampler)(num_steps=steps, guider_config=gcfg, device=DEV, seed=SEED, **CHURN, **SCHED)
    else:
        mod = (S.EulerEDMSampler if args.solver == "euler" else S.DPMPP2MSampler)(num_steps=steps, guider_config=gcfg, device=DEV, **SCHED)
    den = S.DiscreteDenoiser().to(DEV)
    sampling.set_cfg_branches(net, NB)
    sampling.clear_rendered_feat(net)
    c, uc = {"crossattn": ctx[NB - 1:], "vector": y[NB - 1:]}, {"crossattn": ctx[:1], "vector": y[:1]}
    network = lambda x_in, t, cond: (net(x_in, timesteps=t, context=cond["crossattn"], y=cond["vector"], pose=pose)[0], None, None, None)  # noqa: E731
    denoiser = lambda inp, sig, cond: den(network, inp, sig, cond)  # noqa: E731
    sig = mod.discretization(steps, device=DEV)
    x, old, ds = x0.clone(), None, []
    table = S.lms_coefficients(sig, args.order) if args.solver == "lms" else None
    for i in range(steps):
        s, sn = sig[i].reshape(1), sig[i + 1].reshape(1)
        if args.solver == "heun" or CHURN:
            x, _ = mod.sampler_step(s, sn, denoiser, x, c, uc, mod.gamma_of(sig[i], steps))
        elif args.solver == "euler":
            x, _ = mod.sampler_step(s, sn, denoiser, x, c, uc)
        elif args.solver in ("euler_a", "dpmpp2s_a"):
            x = mod.sampler_step(s, sn, denoiser, x, c, uc)
        elif args.solver == "lms":
            x = mod.sampler_step(ds, [float(table[i, j]) for j in range(min(i + 1, args.order))], s, denoiser, x, c, uc)
        else:
            x, old = mod.sampler_step(old, None if i == 0 else sig[i - 1].reshape(1), s, sn, denoiser, x, c, uc)
    sampling.clear_rendered_feat(net)
    out(figure="job_vs_module_route", solver=LABEL, schedule=args.schedule, on_grid=bool(getattr(smp, "on_grid", True)), n_steps=steps, steps=steps, max_abs=float((got - x).abs().max()),
        rel=float((got - x).abs().max() / x.abs().max()), latent_max=float(x.abs().max()), staged=bool(smp.staged))


@torch.no_grad()
def timing():
    latent, refs = args.latent, args.refs
    net = bench.build_model(latent, refs, 50, DEV)
    pose, ctx, y, x0 = batch(0, latent, refs)
    smps = {}
    for label, solver, churn in (("euler", "euler", None), ("dpmpp2m", "dpmpp2m", None) if LABEL == "euler" else (LABEL, args.solver, CHURN)):
        smp = make(net, pose, ctx, y, 50, solver, churn)
        x = smp.step(x0.clone(), 0, alias=True)
        for i in range(1, 4):
            x = smp.step(x, i, alias=True)
        smps[label] = smp
    torch.cuda.synchronize()

    def timed(smp, i):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        smp.step(smp.gx, i, alias=True)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    # (steady replays only: both samplers keep the render of pose 0 pinned in buffers of the shared UNet, written with identical values)
    ms = {k: [] for k in smps}
    for k in range(args.reps):
        for solver, smp in smps.items():
            ms[solver].append(timed(smp, 4 + k % 40))
    out(figure="steady_step_ms", latent=latent, refs=refs, reps=args.reps, staged=all(s.staged for s in smps.values()),
        **{f"{k}_median": round(statistics.median(v), 3) for k, v in ms.items()}, **{f"{k}_min": round(min(v), 3) for k, v in ms.items()})


if __name__ == "__main__":
    deviation() if args.what == "deviation" else timing()
