#!/usr/bin/env python
"""Two-branch (VanillaCFGImgRef) against three-branch (ScheduledCFGImgTextRef) sampling through cd360.job.Sampler: the figures of DESIGN.md's
section on two-way CFG.  Calls the job sampler directly (bench.py keeps measuring the three-branch headline).

  --branches 2|3     which guider (3 also runs on a checkout that predates the two-branch path: --repo PATH imports that checkout)
  --what deviation   3 steps at latent 32 / 6 views: the captured job sampler against the un-captured module route (cd360.sampler.EulerEDMSampler
                     + the guider + DiscreteDenoiser around the same UNet, eager), max |difference| / max |module-route latent|; and pose 0 of a
                     bs = 1 replay against pose 0 of a bs = 2 / bs = 3 replay
  --what timing      latent 128 / 50 views: render-step and steady-step time of the graph sampler (median of --reps replays after warm-up),
                     and the kernel launches of one steady step (torch.profiler over one replay, or over the eager launch of the same staged step)
Prints one JSON line per figure."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--branches", type=int, default=2, choices=(2, 3))
ap.add_argument("--what", default="deviation", choices=("deviation", "timing"))
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def one_pose(p, latent, refs):
    """(camera batch, uc / c context rows, uc / c vector rows, start latent) of target pose p."""
    cam = synth.pose_batch(1, refs, seed=100 + p, n_train=50)[0]
    g = torch.Generator(device=DEV).manual_seed(7 + p)
    ctx = torch.randn(2, 77, 2048, generator=g, device=DEV).to(BF)
    y = torch.randn(2, 2816, generator=g, device=DEV).to(BF)
    return cam, ctx, y, torch.randn(1, 4, latent, latent, generator=g, device=DEV)


def batch(poses, latent, refs):
    """The job's inputs for `poses` in ONE replay: pose = NB x bs camera batches, ctx / y = [uc x bs | (filler x bs) | c x bs]."""
    P = [one_pose(p, latent, refs) for p in poses]
    cams = [c for c, _, _, _ in P]
    parts = [[c[0:1] for _, c, _, _ in P]] + [[c[0:1] for _, c, _, _ in P]] * (NB - 2) + [[c[1:2] for _, c, _, _ in P]]
    ctx = torch.cat([t for part in parts for t in part])
    parts = [[v[0:1] for _, _, v, _ in P]] + [[v[0:1] for _, _, v, _ in P]] * (NB - 2) + [[v[1:2] for _, _, v, _ in P]]
    y = torch.cat([t for part in parts for t in part])
    return cams * NB, ctx, y, torch.cat([x for _, _, _, x in P])


def out(**kw):
    print(json.dumps(dict(branches=NB, **kw)), flush=True)


@torch.no_grad()
def deviation():
    latent, refs, steps = 32, 6, 3
    net = bench.build_model(latent, refs, 50, DEV)
    pose, ctx, y, x0 = batch([0], latent, refs)
    smp = job.Sampler(net, pose, ctx, y, 50, scale_im=SCALE_IM, use_graph=True)
    got = job.sample_assigned(smp, [(pose, ctx, y, x0)], steps)[0]
    # the un-captured module route: the YAML's classes, eager, around the same UNet
    guider = S.VanillaCFGImgRef(7.5) if NB == 2 else S.ScheduledCFGImgTextRef(7.5, 3.5)
    eul = S.EulerEDMSampler(num_steps=50, device=DEV)
    eul.guider = guider
    den = S.DiscreteDenoiser().to(DEV)
    if hasattr(sampling, "set_cfg_branches"):
        sampling.set_cfg_branches(net, NB)
    sampling.clear_rendered_feat(net)
    c = {"crossattn": ctx[NB - 1:], "vector": y[NB - 1:]}
    uc = {"crossattn": ctx[:1], "vector": y[:1]}
    network = lambda x_in, t, cond: (net(x_in, timesteps=t, context=cond["crossattn"], y=cond["vector"], pose=pose)[0], None, None, None)  # noqa: E731
    denoiser = lambda inp, sig, cond: den(network, inp, sig, cond)  # noqa: E731
    sig = eul.discretization(50, device=DEV)
    x = x0.clone()
    for i in range(steps):
        x, _ = eul.sampler_step(sig[i].reshape(1), sig[i + 1].reshape(1), denoiser, x, c, uc)
    sampling.clear_rendered_feat(net)
    out(figure="job_vs_module_route", steps=steps, max_abs=float((got - x).abs().max()), rel=float((got - x).abs().max() / x.abs().max()),
        staged=bool(smp.staged))
    # is a sample's latent independent of how many samples share the replay?
    for bs in (2, 3):
        pose_b, ctx_b, y_b, x_b = batch(list(range(bs)), latent, refs)
        smp_b = job.Sampler(net, pose_b, ctx_b, y_b, 50, scale_im=SCALE_IM, use_graph=True)
        got_b = job.sample_assigned(smp_b, [(pose_b, ctx_b, y_b, x_b)], steps)[0]
        d = (got_b[:1] - got).abs().max()
        out(figure=f"pose0_bs1_vs_bs{bs}", equal=bool(torch.equal(got_b[:1], got)), max_abs=float(d), rel=float(d / got.abs().max()))


@torch.no_grad()
def timing():
    latent, refs = 128, 50
    net = bench.build_model(latent, refs, 50, DEV)
    pose, ctx, y, x0 = batch([0], latent, refs)
    smp = job.Sampler(net, pose, ctx, y, 50, scale_im=SCALE_IM, use_graph=True)
    x = smp.step(x0.clone(), 0, alias=True)
    for i in range(1, 4):
        x = smp.step(x, i, alias=True)
    torch.cuda.synchronize()

    def timed(i):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        smp.step(smp.gx if smp.staged else x, i, alias=True)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    steady = [timed(4 + k) for k in range(args.reps)]
    render = [timed(0) for _ in range(max(3, args.reps // 4))]
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        smp.step(smp.gx if smp.staged else x, 5, alias=True)
        torch.cuda.synchronize()
    def device_kernels(prof):
        return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]

    kernels = device_kernels(prof)
    if not kernels:  # the profiler does not itemise a replay on this stack: the eager launch of the SAME staged step, itemised
        eager = job.Sampler(net, pose, ctx, y, 50, scale_im=SCALE_IM, use_graph=False)
        xe = eager.step(x0.clone(), 0, alias=True)
        xe = eager.step(xe, 1, alias=True)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            eager.step(xe, 2, alias=True)
            torch.cuda.synchronize()
        kernels = device_kernels(prof)
    foreign = sorted({e.name[:60] for e in kernels if any(s in e.name for s in ("at::native", "elementwise_kernel", "vectorized"))})
    out(figure="graph_sampler_ms", latent=latent, refs=refs, images=int(smp.y.shape[0]), steady_ms=round(statistics.median(steady), 3),
        steady_min_ms=round(min(steady), 3), render_ms=round(statistics.median(render), 3), steady_launches=len(kernels), torch_issued=foreign,
        staged=bool(smp.staged), render_captured=smp.rgraph is not None)


if __name__ == "__main__":
    deviation() if args.what == "deviation" else timing()
