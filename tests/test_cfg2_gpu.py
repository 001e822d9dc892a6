"""Two-way CFG (VanillaCFGImgRef: uncond | image+text) on the captured HIP sampling step: the two-branch forms of the tail kernels, their
memory safety, the GPU trajectory against the reference's golden, and the sampling job in two-branch mode.  Needs an MI355X."""
import functools
import os

import pytest
import torch

import guarded as G
import sampler_cases as SC
import weights as W
from sampler_cases import BF, DEV

pytestmark = pytest.mark.gpu
R = functools.partial(SC.R, dtype=BF)

# test 9's yardstick: the SAME comparison (captured job sampler against the un-captured module route, 3 steps, latent 32 / 6 views, bs = 1)
# for THREE branches on the parent commit, measured with tools/cfg_branches_report.py on the box and in the session of this change
# (max |difference| 0.4049 of max |latent| 12.34).  The two-branch figure of the same session: 0.04114 (max |difference| 0.5061).
PARENT_CFG3_JOB_VS_MODULE_REL = 0.03281


def rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-12)


# ================================================================================================ 5: the tail kernels
def test_two_branch_f32_kernel_matches_the_torch_chain():
    """cd360_cfg_euler_step_f32 in two-branch form against cfg_euler_update(scale_im=None, fused=False) (== VanillaCFGImgRef -> to_d ->
    Euler: tests/test_cfg2_cpu.py); the bar of test_cfg_euler_step_kernel_matches_sampler_chain: 1e-6 of the tensor maximum."""
    from cd360.sampler import cfg_euler_update
    x, eps = W.tensor("x", (2, 4, 16, 16), seed=3), W.tensor("eps", (4, 4, 16, 16), seed=3)
    s, sn = torch.tensor([3.3]), torch.tensor([2.9])
    want = cfg_euler_update(x, eps, s, sn, 7.5, None, fused=False)
    got = cfg_euler_update(x.to(DEV), eps.to(DEV), s.to(DEV), sn.to(DEV), 7.5, None, fused=True)
    assert got.is_cuda and rel(got, want) < 1e-6
    from cd360 import ops
    with pytest.raises(ValueError):  # a three-branch eps under the two-branch request, and the other way round: refused on the host
        ops.cfg_euler_step(x.to(DEV), torch.cat([eps, eps[:2]]).to(DEV), s.to(DEV), sn.to(DEV), 7.5, None)
    with pytest.raises(ValueError):
        ops.cfg_euler_step(x.to(DEV), eps.to(DEV), s.to(DEV), sn.to(DEV), 7.5, 3.5)
    with pytest.raises(ValueError):  # a NaN handed in as a number is not the request
        ops.cfg_euler_step(x.to(DEV), torch.cat([eps, eps[:2]]).to(DEV), s.to(DEV), sn.to(DEV), 7.5, float("nan"))


def test_two_branch_cl_kernel_equals_the_f32_kernel_on_the_same_rows():
    """cd360_cfg_euler_step_cl in two-branch form, in place, against the fp32 kernel fed the fp32 copy of the same bf16 channels-last rows:
    bit-equal, at a ragged size (W = 40 is not a multiple of 64), for two step indices, from 16-wide rows (the row stride is passed)."""
    from cd360 import ops
    g = torch.Generator(device=DEV).manual_seed(3)
    bs, H, Wd, nsteps = 2, 24, 40, 5
    x = torch.randn(bs, 4, H, Wd, generator=g, device=DEV)
    tab = torch.rand(nsteps, 4, generator=g, device=DEV) + 0.5
    for step in (0, 3):
        gi = torch.tensor([step], dtype=torch.int32, device=DEV)
        eps16 = torch.randn(2 * bs, H * Wd, 16, generator=g, device=DEV).to(BF)
        eps_nchw = eps16[..., :4].float().reshape(2 * bs, H, Wd, 4).permute(0, 3, 1, 2).contiguous()
        want_x = ops.cfg_euler_step(x, eps_nchw, tab[step, 0].reshape(1).contiguous(), tab[step, 1].reshape(1).contiguous(), 7.5, None)
        x2 = x.clone()
        out = ops.cfg_euler_step_cl(x2, eps16[..., :4], tab, gi, 7.5, None)
        assert out is x2 and torch.equal(x2, want_x) and not torch.equal(x2, x)
    with pytest.raises(ValueError):
        ops.cfg_euler_step_cl(x.clone(), torch.cat([eps16, eps16[:bs]])[..., :4], tab, gi, 7.5, None)


def _restated(x, e, s, sn, scale, scale_im):
    """The kernels' expression in the kernels' order, one fp32 rounding per operation (torch's elementwise kernels do not contract)."""
    return x + (x - SC.combine(x, e, s, scale, scale_im)) / s * (sn - s)


@pytest.mark.parametrize("scale_im", [3.5, 0.0, -1.25, None])
def test_both_kernels_equal_a_torch_restatement_in_the_kernels_order(scale_im):
    """Three branches (any finite scale_im, zero and negative included: they stay three-branch calls) and two, both kernels: bit-equal to
    the expression evaluated operation by operation in fp32 in the documented order -- a changed three-branch instantiation is caught here.
    The two-branch case also runs the `_cl` kernel at 4097 x 4096 pixels, where its grid-stride loop takes a second trip."""
    from cd360 import ops
    nb = 2 if scale_im is None else 3
    g = torch.Generator(device=DEV).manual_seed(11)
    bs, H, Wd = 2, 24, 40
    x = torch.randn(bs, 4, H, Wd, generator=g, device=DEV)
    eps16 = torch.randn(nb * bs, H * Wd, 16, generator=g, device=DEV).to(BF)
    e = eps16[..., :4].float().reshape(nb * bs, H, Wd, 4).permute(0, 3, 1, 2).contiguous()
    tab = torch.rand(5, 4, generator=g, device=DEV) + 0.5
    gi = torch.tensor([2], dtype=torch.int32, device=DEV)
    s, sn = tab[2, 0].reshape(1).contiguous(), tab[2, 1].reshape(1).contiguous()
    want = _restated(x, e, s, sn, 7.5, scale_im)
    assert torch.equal(ops.cfg_euler_step(x, e, s, sn, 7.5, scale_im), want)
    x2 = x.clone()
    ops.cfg_euler_step_cl(x2, eps16[..., :4], tab, gi, 7.5, scale_im)
    assert torch.equal(x2, want)
    if scale_im is None:
        # one more input, the `_cl` kernel alone: bs = 1, 4097 x 4096 pixels = the first size past 65536 workgroups x 256 threads, so the
        # grid-stride loop takes a second trip; 4-wide rows (ld = 4).  The restatement is elementwise, so it is evaluated band by band of
        # 256 image rows and the device holds x, its updated copy and eps only (0.8 GB).
        H, Wd = 4097, 4096
        x = torch.randn(1, 4, H, Wd, generator=g, device=DEV)
        eps4 = torch.randn(2, H * Wd, 4, generator=g, device=DEV, dtype=BF)
        x2 = x.clone()
        ops.cfg_euler_step_cl(x2, eps4, tab, gi, 7.5, None)
        for h0 in range(0, H, 256):
            h1 = min(h0 + 256, H)
            e = eps4[:, h0 * Wd:h1 * Wd].float().reshape(2, h1 - h0, Wd, 4).permute(0, 3, 1, 2)
            assert torch.equal(x2[:, :, h0:h1], _restated(x[:, :, h0:h1], e, s, sn, 7.5, None)), h0


# ================================================================================================ 6: guarded runs
@pytest.mark.parametrize("bs,H,Wd", [(1, 5, 7), (2, 24, 40)])
def test_two_branch_tails_read_two_branches_and_write_their_output_only(bs, H, Wd):
    """Both two-branch tails under tests/guarded.py, both poison patterns.  `eps` lives in arena blocks: once with EXACTLY 2 bs images
    between canaries, once as the first 2 bs images of a 3 bs block whose last bs stay poisoned (0xFF: NaN; 0x7F: 3.39e38) -- a kernel
    that still reads a third branch gives a non-finite result under the first poison or different bits under the second.  No guard byte
    changes, the results are bit-equal between the poisons and between the two allocations, eps is unchanged, x changes in place only."""
    from cd360 import ops
    d = dict(x=R(bs, 4, H, Wd, seed=1, dtype=torch.float32), e=R(2 * bs, 4, H, Wd, seed=2, dtype=torch.float32), e16=R(2 * bs, H * Wd, 16, seed=7),
             tab=R(5, 4, seed=2, dtype=torch.float32).abs() + 0.5, step=torch.tensor([3], dtype=torch.int32, device=DEV),
             s0=torch.tensor([1.7], device=DEV), s1=torch.tensor([1.1], device=DEV), xc=R(bs, 4, H, Wd, seed=1, dtype=torch.float32))

    @SC.guardfn
    def fn(x, e, e16, tab, step, s0, s1, xc, guard):
        outs = []
        for tail in (0, bs):  # exact allocation; poisoned third behind the two branches
            ge = guard.torch.empty(2 * bs + tail, 4, H, Wd, dtype=torch.float32, device=DEV)
            ge[:2 * bs].copy_(e)
            ge16 = guard.torch.empty(2 * bs + tail, H * Wd, 16, dtype=BF, device=DEV)
            ge16[:2 * bs].copy_(e16)
            keep, keep16 = ge[:2 * bs].clone(), ge16[:2 * bs].clone()
            out = ops.cfg_euler_step(x, ge[:2 * bs], s0, s1, 7.5, None)
            gx = guard.torch.empty(bs, 4, H, Wd, dtype=torch.float32, device=DEV)
            gx.copy_(x)
            assert ops.cfg_euler_step_cl(gx, ge16[:2 * bs, :, :4], tab, step, 7.5, None) is gx
            assert torch.equal(ge[:2 * bs], keep) and torch.equal(ge16[:2 * bs], keep16), "eps was written"
            outs += [out, gx]
        ops.cfg_euler_step_cl(xc, e16[..., :4], tab, step, 7.5, None)  # the caller's own latent, in place
        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]) and torch.equal(outs[1], xc)
        return outs

    res, _ = G.run_twice(fn, d, declares=["cd360_cfg_euler_step_f32", "cd360_cfg_euler_step_cl"], inout=("xc",))
    assert torch.equal(res[0], _restated(d["x"], d["e"], d["s0"], d["s1"], 7.5, None))
    assert not torch.equal(res[1], d["x"])


# ================================================================================================ 7: the GPU trajectory
@torch.no_grad()
def test_fused_two_branch_step_on_the_gpu_walks_the_reference_trajectory():
    """EulerEDMSampler + VanillaCFGImgRef + DiscreteDenoiser as the product launches them per denoise step in two-branch mode
    (cd360.sampler.fused_cfg_euler_step, the tail on cd360_cfg_euler_step_f32) ON THE GPU over the 12-step cfg2 trajectory of
    tests/golden/sampler.npz, written by the REFERENCE's own classes; the bar the cfg3 twin in tests/test_f_rows_gpu.py holds."""
    from test_cfg2_cpu import run_product_steps2
    from test_sampler_cpu import load
    g = load()
    got = run_product_steps2(g, DEV, fused=True)
    assert got.is_cuda
    err = float((got.cpu() - g["cfg2"]).abs().max())
    print("cfg2: fused GPU trajectory vs the reference's golden, max abs:", err, "of max", float(g["cfg2"].abs().max()))
    assert torch.allclose(got.cpu(), g["cfg2"], atol=2e-5, rtol=1e-5), err


# ================================================================================================ 8, 9: the job
def _pose(p, latent, refs):
    """Target pose p: its camera batch, [uc | c] context and vector rows, start latent."""
    from cd360 import synth
    cam = synth.pose_batch(1, refs, seed=100 + p, n_train=50)[0]
    g = torch.Generator(device=DEV).manual_seed(7 + p)
    ctx = torch.randn(2, 77, 2048, generator=g, device=DEV).to(BF)
    y = torch.randn(2, 2816, generator=g, device=DEV).to(BF)
    return cam, ctx, y, torch.randn(1, 4, latent, latent, generator=g, device=DEV)


def _job2(poses, latent, refs):
    """The two-branch job inputs for `poses` in one replay: 2 bs camera batches, ctx / y = [uc x bs | c x bs] (sample.py:172-177)."""
    P = [_pose(p, latent, refs) for p in poses]
    ctx = torch.cat([c[0:1] for _, c, _, _ in P] + [c[1:2] for _, c, _, _ in P])
    y = torch.cat([v[0:1] for _, _, v, _ in P] + [v[1:2] for _, _, v, _ in P])
    return [c for c, _, _, _ in P] * 2, ctx, y, torch.cat([x for _, _, _, x in P])


@torch.no_grad()
def test_two_branch_job_through_two_captured_graphs():
    """Sampler(scale_im=0, use_graph=True) over 3 poses x 3 steps through job.sample_poses.
    (a) both graphs captured, the staged step's UNet input holds 2 bs images (not 3), latents finite;
    (b) every pose's latent bit-identical to a fresh graph-mode two-branch sampler's: a retarget leaves nothing behind;
    (c) graph mode bit-identical to use_graph=False (both run the staged step);
    (d) the first pose block's cached render: branch 0 is the oracle's render of the NULL image, branch 1 of the chosen references
        (oracle.reference_attn's chain on every ray, 1e-2 of the tensor maximum: the bar tests/test_job_gpu.py holds three branches to)."""
    import bench
    from cd360 import job, sampling, shard
    from cd360.cameras import pack_cameras
    from test_modules_gpu import _oracle_render_on_rays, rel as mrel
    latent, refs, steps, P = 32, 6, 3, 3
    net = bench.build_model(latent, refs, 50, DEV)
    name0, blk0 = sampling.pose_blocks(net)[0]
    held = {}

    def make_sampler(pose, ctx, y):
        held["smp"] = job.Sampler(net, pose, ctx, y, 50, scale_im=0, use_graph=True)
        return held["smp"]

    latents, mine = job.sample_poses(make_sampler, lambda p: _job2([p], latent, refs), P, steps, world=1, rank=0)
    smp = held["smp"]
    assert mine == list(range(P)) and latents.shape == (P, 4, latent, latent) and torch.isfinite(latents).all()  # (a)
    assert smp.branches == 2 and smp.bs == 1 and smp.graph is not None and smp.rgraph is not None and smp.staged
    assert smp.h0.shape[0] == 2 * smp.bs and smp.emb_act.shape[0] == 2 and smp.ctx.shape[0] == 2 and smp.pose.packed.shape[0] == 2
    assert all(blk.cfg_branches == 2 and blk.rendered_feat.shape[0] == 2 for _, blk in sampling.pose_blocks(net))
    rend_last = blk0.rendered_feat.float().clone()  # pose 2's render, produced by a replay of the graph captured at pose 0
    for p in range(P):
        pose, ctx, y, x0 = _job2([p], latent, refs)
        fresh = job.sample_assigned(job.Sampler(net, pose, ctx, y, 50, scale_im=0, use_graph=True), [(pose, ctx, y, x0)], steps)[0]
        assert torch.equal(fresh, latents[p:p + 1]), (p, float((fresh - latents[p:p + 1]).abs().max()))  # (b)
        eager = job.sample_assigned(job.Sampler(net, pose, ctx, y, 50, scale_im=None, use_graph=False), [(pose, ctx, y, x0)], steps)[0]
        assert torch.equal(eager, latents[p:p + 1]), (p, float((eager - latents[p:p + 1]).abs().max()))  # (c)
    assert float((latents[0] - latents[1]).abs().max() / latents[1].abs().max()) > 1e-2  # different trajectories
    # (d)
    w = {k: v.detach().float().cpu() for k, v in blk0.state_dict().items() if "references" not in k and "raymarcher" not in k}
    allrefs = blk0.references.float().cpu()
    choices = list(blk0.reference_choices)
    idx = torch.arange(allrefs.shape[1])
    cond = allrefs[:-1][torch.tensor(choices)][None]
    null = allrefs[-1:][None].expand(1, len(choices), -1, -1)
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    pose, ctx, y, _ = _job2([P - 1], latent, refs)
    cams = pack_cameras(pose[:1]).float().cpu()
    smp_ctx = job.Sampler(net, pose, ctx, y, 50, scale_im=0, use_graph=False).ctx.float().cpu()
    errs = []
    for br in range(2):
        want = _oracle_render_on_rays(w, cams, null if br == 0 else cond, smp_ctx[br:br + 1], blk0.attn2.heads,
                                      blk0.pose_featurenerf.num_samples, float(blk0.pose_featurenerf.far), idx)
        errs.append(mrel(rend_last[br:br + 1], want[0]))
    print(f"pose {P - 1}: rendered features of {name0} vs oracle per CFG branch (two branches):", [round(e, 5) for e in errs])
    assert max(errs) < 1e-2, errs


@torch.no_grad()
def test_six_rows_run_as_two_branches_of_three_poses():
    """(e) bs = 3: six rows, which `batch % 3` reads as three branches of two.  The sampler states the layout, so the render holds 3 null-image
    rows + 3 reference rows, and pose 0's latent is BIT-IDENTICAL to the bs = 1 run of the same pose and start latent.
    (The three-branch job on the parent commit is bit-independent of bs as well -- pose 0 of a bs = 2 replay against bs = 1, 3 steps,
    latent 32 / 6 views: max |difference| 0.0, tools/cfg_branches_report.py --branches 3 -- so the comparison stays `equal`.)"""
    import bench
    from cd360 import job, sampling
    latent, refs, steps = 32, 6, 3
    net = bench.build_model(latent, refs, 50, DEV)
    pose1, ctx1, y1, x1 = _job2([0], latent, refs)
    one = job.sample_assigned(job.Sampler(net, pose1, ctx1, y1, 50, scale_im=0, use_graph=True), [(pose1, ctx1, y1, x1)], steps)[0]
    pose3, ctx3, y3, x3 = _job2([0, 1, 2], latent, refs)
    smp = job.Sampler(net, pose3, ctx3, y3, 50, scale_im=0, use_graph=True)
    assert smp.bs == 3 and smp.branches == 2 and torch.equal(x3[:1], x1)
    three = job.sample_assigned(smp, [(pose3, ctx3, y3, x3)], steps)[0]
    assert smp.graph is not None and smp.rgraph is not None and smp.h0.shape[0] == 6 and torch.isfinite(three).all()
    name0, blk0 = sampling.pose_blocks(net)[0]
    rf = blk0.rendered_feat.float()
    assert rf.shape[0] == 6
    # null-image rows differ from reference rows of the same pose; under the `% 3` reading row 2 would be a reference row of pose 0
    pose_n, ctx_n, y_n, x_n = _job2([2], latent, refs)
    job.sample_assigned(job.Sampler(net, pose_n, ctx_n, y_n, 50, scale_im=0, use_graph=True), [(pose_n, ctx_n, y_n, x_n)], 1)
    rf1 = blk0.rendered_feat.float()
    print("bs = 3 render rows 2 / 5 against pose 2 alone:", float((rf[2:3] - rf1[0:1]).abs().max()), float((rf[5:6] - rf1[1:2]).abs().max()),
          "of", float(rf1.abs().max()))
    assert float((rf[2:3] - rf1[0:1]).abs().max()) <= 1e-2 * float(rf1.abs().max())  # row 2 = pose 2's NULL-image render
    assert float((rf[5:6] - rf1[1:2]).abs().max()) <= 1e-2 * float(rf1.abs().max())  # row 5 = pose 2's reference render
    d = float((three[:1] - one).abs().max())
    print("bs = 3 pose 0 vs bs = 1:", d, "of", float(one.abs().max()))
    assert torch.equal(three[:1], one), d


@torch.no_grad()
def test_two_branch_job_agrees_with_the_uncaptured_module_route():
    """Whole trajectory, 3 steps: the same UNet under cd360.sampler.EulerEDMSampler + VanillaCFGImgRef + DiscreteDenoiser (the YAML's
    classes, eager, the implicit-GEMM input convolution) against the two-branch job sampler (captured, staged).  The two differ by the
    staged input convolution rounding a few bf16 values to the other neighbour, amplified by 70 random-init blocks (cd360/job.py).
    Bar: twice what the SAME comparison gives for THREE branches on the parent commit, measured on the same box in the same session
    (tools/cfg_branches_report.py --what deviation); the margin covers the box's run-to-run spread only.
    Measured (MI355X, one session): three branches on the parent commit 3.281e-2 of the latent's maximum (and the same, bit for bit, on
    this tree); two branches 4.114e-2; bar 6.562e-2.  DESIGN.md section 6.1."""
    import bench
    from cd360 import job
    from cd360 import sampler as S
    latent, refs, steps = 32, 6, 3
    net = bench.build_model(latent, refs, 50, DEV)
    pose, ctx, y, x0 = _job2([0], latent, refs)
    got = job.sample_assigned(job.Sampler(net, pose, ctx, y, 50, scale_im=0, use_graph=True), [(pose, ctx, y, x0)], steps)[0]
    eul = S.EulerEDMSampler(num_steps=50, guider_config=SC.guider_config(2), device=DEV)
    x = SC.module_route(net, eul, "euler", 2, pose, ctx, y, x0, steps)
    dev = float((got - x).abs().max() / x.abs().max())
    print("two-branch job vs module route, 3 steps: max abs", float((got - x).abs().max()), "rel", dev, "| parent, three branches:",
          PARENT_CFG3_JOB_VS_MODULE_REL)
    assert torch.isfinite(got).all() and dev <= 2 * PARENT_CFG3_JOB_VS_MODULE_REL, (dev, PARENT_CFG3_JOB_VS_MODULE_REL)
