"""Two-way CFG (VanillaCFGImgRef, guiders.py:136-166: uncond | image+text) through the product's step function, its tail formula, the
stated CFG layout of the pose blocks and the job sampler's argument handling.  CPU only; tests/test_cfg2_gpu.py holds the kernels, the
captured job and the trajectory on the GPU."""
import pytest
import torch

import weights as W
from test_sampler_cpu import dummy_network, load


def run_product_steps2(g, dev, fused):
    """The 12-step cfg2 trajectory of sampler.npz through the product's step function in two-branch mode (cd360.sampler.fused_cfg_euler_step
    under VanillaCFGImgRef: what cd360/job.py's Sampler launches per denoise step for scale_im <= 0), around the golden's dummy network."""
    from cd360 import sampler as S
    den = S.DiscreteDenoiser().to(dev)
    guider = S.VanillaCFGImgRef(7.5)
    c = {"crossattn": g["c_crossattn"].to(dev), "vector": g["c_vector"].to(dev)}
    uc = {"crossattn": g["uc_crossattn"].to(dev), "vector": g["uc_vector"].to(dev)}
    x = g["x"].to(dev)
    _, _, cond2 = guider.prepare_inputs(x, x.new_ones(x.shape[0]), c, uc)  # once per image: constant over the trajectory
    n = x.shape[0]  # rows [0, 2n) = [u | c] of the target; the golden's conditioning carries its reference views' rows behind them
    assert torch.equal(cond2["crossattn"][:n], uc["crossattn"][:n]) and torch.equal(cond2["crossattn"][n:2 * n], c["crossattn"][:n])
    sigmas = S.LegacyDDPMDiscretization()(12, device=dev)
    x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)  # EulerEDMSampler.prepare_sampling_loop (sampling.py:52-66)
    network = lambda x_in, c_noise: dummy_network(x_in, c_noise, cond2)[0]  # noqa: E731
    for i in range(12):
        x = S.fused_cfg_euler_step(den, network, x, sigmas[i], sigmas[i + 1], guider, fused=fused)
    return x


def test_product_step_function_walks_the_reference_cfg2_trajectory():
    """The un-fused form of the product's two-branch step reproduces the 12-step trajectory the REFERENCE's EulerEDMSampler +
    VanillaCFGImgRef + DiscreteDenoiser wrote into tests/golden/sampler.npz["cfg2"]; the bar test_sampler_cpu.py holds cfg3 to.
    (For the golden's dummy network the image branch equals the unconditional one, so cfg2 == cfg3: this pins the arithmetic and the
    [u | c] layout; that no third branch is computed or read is tests/test_cfg2_gpu.py's business.)"""
    g = load()
    res = run_product_steps2(g, "cpu", fused=False)
    err = float((res - g["cfg2"]).abs().max())
    print("cfg2: un-fused CPU trajectory vs the reference's golden, max abs:", err, "of max", float(g["cfg2"].abs().max()))
    assert torch.allclose(res, g["cfg2"], atol=2e-5, rtol=1e-5), err


def test_two_branch_tail_formula_equals_the_unfused_chain():
    """cfg_euler_update(scale_im=None)'s algebra (what the two-branch cd360_cfg_euler_step_f32 computes) == denoiser c_out +
    VanillaCFGImgRef + to_d + Euler, on CPU; a three-branch eps is refused, as is a two-branch eps with a scale_im."""
    from cd360.sampler import VanillaCFGImgRef, cfg_euler_update
    x, eps = W.tensor("x", (2, 4, 8, 8), seed=3), W.tensor("eps", (4, 4, 8, 8), seed=3)
    s, sn = torch.tensor(3.3), torch.tensor(2.9)
    den = torch.cat([x, x]) - s * eps
    d0 = VanillaCFGImgRef(7.5)(den, None)
    want = x + (x - d0) / s * (sn - s)
    assert torch.allclose(cfg_euler_update(x, eps, s, sn, 7.5, scale_im=None, fused=False), want, atol=1e-6)
    with pytest.raises(ValueError):
        cfg_euler_update(x, W.tensor("eps", (6, 4, 8, 8), seed=3), s, sn, 7.5, scale_im=None, fused=False)
    with pytest.raises(ValueError):
        cfg_euler_update(x, eps, s, sn, 7.5, 3.5, fused=False)


def _pose_net(n_blocks=2):
    from sgm.modules.attention import BasicTransformerBlock
    net = torch.nn.ModuleList([BasicTransformerBlock(64, 1, 64, context_dim=32, checkpoint=False, attn_mode="softmax-xformers", image_cross=True,
                                                     num_samples=4, rgb_predict=True, mode="feature-nerf") for _ in range(n_blocks)])
    refs = torch.arange(5 * 4 * 64, dtype=torch.float32).reshape(5, 4, 64)
    for blk in net:
        blk.register_buffer("references", refs.clone())
    return net, refs


def test_stated_cfg_layout_replaces_the_modulo_three_guess():
    """Six rows are two branches of three poses as well as three branches of two.  enable_reference_sampling(branches=2) states it on every
    pose block: (n_null, n_cond) = (3, 3), the reference context is [null x 3 | chosen x 3], no branch is taken for a duplicate.
    branches=None keeps sample.py:89's inference (2 null + 4 conditional rows); a batch the stated count does not divide raises."""
    from cd360 import sampling
    net, refs = _pose_net()
    names = sampling.enable_reference_sampling(net, [0, 2], branches=2)
    assert len(names) == 2
    for blk in net:
        assert blk.cfg_branches == 2
        assert blk._cfg_layout(6, blk.cfg_branches) == (3, 3)
        c = blk._references_as_context(6)
        assert c.shape == (6, 2, 4, 64)
        for i in range(3):
            assert torch.equal(c[i, 0], refs[4]) and torch.equal(c[i, 1], refs[4])
            assert torch.equal(c[3 + i, 0], refs[0]) and torch.equal(c[3 + i, 1], refs[2])
        pose = [object() for _ in range(3)]
        pose = pose + pose  # [uc poses | c poses]: rows 2 and 4 would be "the same object" for nobody, rows i and 3 + i are
        assert blk._duplicate_cfg_branch(pose, (6, 2, 4, 64), blk.cfg_branches) == 0
        same = [pose[0]] * 6  # even where every row is one object, two stated branches hold no duplicate
        assert blk._duplicate_cfg_branch(same, (6, 2, 4, 64), 2) == 0 and blk._duplicate_cfg_branch(same, (6, 2, 4, 64), None) == 2
    # the unchanged inference
    sampling.enable_reference_sampling(net, [0, 2])
    for blk in net:
        assert blk.cfg_branches is None
        assert blk._cfg_layout(6, blk.cfg_branches) == (2, 4) and blk._cfg_layout(6) == (2, 4) and blk._cfg_layout(4) == (2, 2)
        c = blk._references_as_context(6)
        assert torch.equal(c[1, 0], refs[4]) and torch.equal(c[2, 0], refs[0]) and torch.equal(c[5, 1], refs[2])
    # three stated branches: today's thirds; four rows are not three branches
    sampling.enable_reference_sampling(net, [0, 2], branches=3)
    for blk in net:
        assert blk._cfg_layout(6, blk.cfg_branches) == (2, 4)
        assert torch.equal(blk._references_as_context(6), torch.cat([refs[4:5][None].expand(2, 2, -1, -1)] + [refs[[0, 2]][None].expand(2, -1, -1, -1)] * 2))
        with pytest.raises(ValueError):
            blk._cfg_layout(4, blk.cfg_branches)
        with pytest.raises(ValueError):
            blk._references_as_context(4)
    with pytest.raises(ValueError):
        sampling.enable_reference_sampling(net, [0, 2], branches=4)
    sampling.disable_reference_sampling(net)
    assert all(blk.cfg_branches is None and blk.reference_choices is None for blk in net)


@pytest.mark.parametrize("scale_im,branches", [(0, 2), (-1, 2), (None, 2), (0.0, 2), (3.5, 3)])
def test_sampler_picks_its_guider_like_sample_py(scale_im, branches):
    """sample.py:231-240: scale_im > 0 builds ScheduledCFGImgTextRef, anything else VanillaCFGImgRef.  The job sampler reads bs from the
    guider's branch count -- six context rows are bs = 3 under two branches and bs = 2 under three --, assembles the guider's conditioning
    batch, states the layout on the pose blocks and hands the tail kernels scale_im=None for two branches."""
    from cd360 import job, sampler as S, sampling
    net, _ = _pose_net(1)
    sampling.enable_reference_sampling(net, [0, 2])
    g = torch.Generator().manual_seed(1)
    ctx, y = torch.randn(6, 7, 16, generator=g), torch.randn(6, 12, generator=g)
    pose = [object() for _ in range(6)]
    smp = job.Sampler(net, pose, ctx, y, 12, scale=7.5, scale_im=scale_im)
    assert smp.branches == branches and smp.guider.branches == branches and smp.bs == 6 // branches
    assert isinstance(smp.guider, S.VanillaCFGImgRef if branches == 2 else S.ScheduledCFGImgTextRef)
    assert all(blk.cfg_branches == branches for blk in net)
    assert not smp.staged  # (no UNet here)
    if branches == 2:
        assert smp.scale_im is None and smp.guider.scale == 7.5
        assert torch.equal(smp.ctx, ctx) and torch.equal(smp.y, y)  # [uc x 3 | c x 3] as handed in
        ctx2, y2 = ctx.flip(0).contiguous(), y.flip(0).contiguous()
        smp.retarget(pose, ctx2, y2)
        assert torch.equal(smp.ctx, ctx2) and torch.equal(smp.y, y2)
        with pytest.raises(ValueError):
            job.Sampler(net, pose[:3], ctx[:3], y[:3], 12, scale_im=scale_im)  # three rows are not [uc | c]
    else:
        assert smp.scale_im == 3.5
        assert torch.equal(smp.ctx, torch.cat([ctx[:2], ctx[:2], ctx[4:]])) and torch.equal(smp.y, torch.cat([y[:2], y[:2], y[4:]]))
        with pytest.raises(ValueError):
            job.Sampler(net, pose[:4], ctx[:4], y[:4], 12, scale_im=scale_im)
