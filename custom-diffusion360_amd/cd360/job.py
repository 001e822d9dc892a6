"""The sampling job of the pose path: one captured sampler per GPU walking its share of the target poses, one all-gather of the final
latents at the end (BASELINE.json configs[1] and [2]).

The reference samples its target poses one after the other on one GPU (sample.py:331-349: for every pose, `sampler(denoiser, randn, cond,
uc)` with the patched UNet, `clear_rendered_feat` between images).  Here every rank takes the contiguous share `shard.assign_poses` gives
it, samples those poses with ONE `Sampler` -- whose render step and steady-state step are each captured once into a hipGraph and re-pointed
at the next pose by `Sampler.retarget` (camera buffer and conditioning rewritten in place) -- and the ranks exchange nothing until
`shard.gather_latents` collects the final latents (RCCL all-gather over xGMI; gloo in the CPU tests).  `bench.py` times exactly this loop.
`sample_images` is the same job from a seed to uint8 images: the start latent drawn on the device (`start_latent`), every rank decoding its
own poses through the first stage (cd360/images.py), and the one all-gather moving the images instead of the latents.
A `Sampler` built with `known` / `mask` keeps a given latent outside a region (one more launch per step, include/edit/cd360_edit.h);
`start_from` and `first_step` run only the tail of the schedule from a given latent.
"""
from __future__ import annotations

import sys
from typing import Callable, List, Sequence

import torch

from . import shard, solvers


def check_known(bs: int, known, mask, latent_shape=None) -> None:
    """What a masked Sampler asks of (known, mask), on the host and before anything is launched: both or neither; known [bs or 1, 4, H, W]
    and mask [bs or 1, 1, H, W] fp32 tensors of one H x W -- that of `latent_shape` = (bs, 4, H, W) once the latent has been seen."""
    if (known is None) != (mask is None):
        raise ValueError("`known` and `mask` go together: the latent to keep and the region (1 = generate, 0 = keep); give both or neither")
    if known is None:
        return
    if not isinstance(known, torch.Tensor) or known.dtype != torch.float32 or known.ndim != 4 or known.shape[1] != 4 or known.shape[0] not in (1, bs):
        raise ValueError(f"known: an fp32 tensor [{bs} or 1, 4, H, W] is needed, got {getattr(known, 'dtype', type(known))} "
                         f"{tuple(getattr(known, 'shape', ()))}")
    want = (1,) + tuple(known.shape[2:])
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.float32 or mask.ndim != 4 or tuple(mask.shape[1:]) != want or mask.shape[0] not in (1, bs):
        raise ValueError(f"mask: an fp32 tensor [{bs} or 1, 1, {want[1]}, {want[2]}] at latent resolution is needed, got "
                         f"{getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    if latent_shape is not None and tuple(known.shape[2:]) != tuple(latent_shape[2:]):
        raise ValueError(f"known is {tuple(known.shape[2:])}, the latent {tuple(latent_shape[2:])}")


def check_first_step(solver, first_step: int, n_steps: int) -> None:
    """A trajectory that begins at row `first_step` of an `n_steps` schedule: rows 0 .. n_steps - 1, and past row 0 only under the solvers
    whose kernels do not key "no history yet" on row 0 (Sampler.PARTIAL_START).  `solver`: the name, or None for a sampler without one."""
    if isinstance(first_step, bool) or not isinstance(first_step, int) or not 0 <= first_step < n_steps:
        raise ValueError(f"first_step {first_step!r}: a row 0 .. {n_steps - 1} of the {n_steps}-step schedule is needed")
    if first_step > 0 and solver is not None and solver not in Sampler.PARTIAL_START:
        raise ValueError(f"solver {solver!r} keeps earlier steps' results and reads none of them on row 0 only: a trajectory cannot begin at row "
                         f"{first_step}.  Partial starts are served by 'euler' (with and without churn), 'heun', 'euler_a' and 'dpmpp2s_a'")


class Sampler:
    """One sampling step of the pose path under the 3-way image/text CFG of guiders.py:102-133 (uncond | image | image+text) or, for
    `scale_im is None or scale_im <= 0`, the 2-way VanillaCFGImgRef of guiders.py:136-166 (uncond | image+text) -- the switch of
    sample.py:231-240.  B = guider.branches: `ctx` / `y` hold B bs rows ([uc x bs | . | c x bs] resp. [uc x bs | c x bs]), `pose` B bs camera
    batches, and the UNet runs on B bs images (two branches: a third less work per step, not a duplicated branch).
    With `use_graph` the steady-state step (cached render) and the render step are each captured once into a hipGraph and
    replayed: ~3000 launches per step are then issued by the GPU front end instead of the Python interpreter.
    `solver` names the update, one class of cd360/solvers.py each, whose docstring says what it computes and what it carries between steps:
    "euler" (Euler; ChurnedEuler as soon as `s_churn` > 0, with `s_tmin` / `s_tmax` / `s_noise` as EDMSampler's constructor takes them),
    "dpmpp2m" (DPMPP2M), "euler_a" (EulerAncestral: `eta` / `s_noise`), "heun" (Heun: churn as for Euler), "dpmpp2s_a" (DPMPP2SAncestral:
    `eta` / `s_noise`) and "lms" (LMS: `order` in 1..4).  The multistep solvers ("dpmpp2m", "lms") keep earlier steps' results, which are
    not reset between images: `step(x, i)` for i > 0 must follow `step(., i - 1)` of the SAME image (`eps()` is unaffected).
    A solver that draws noise draws it INSIDE its kernels as a pure function of (`seed`, the row's noise stream, step index, channel, pixel)
    (include/cd360_stochastic.h), so graph, eager, fresh and un-staged runs add the same bits and no state is kept between steps.
    `discretization` / `sigmas`: the sigma schedule -- an object with LegacyDDPMDiscretization's call protocol (cd360.sampler:
    EDMDiscretization, the Karras rho schedule; ListDiscretization), or the `n_steps` values themselves; neither: the legacy schedule.
    Where a schedule leaves the denoiser's 1000-entry grid (`on_grid` False) the network runs at the snapped sigma and the solver steps
    on the schedule's own: "euler", "heun" and "dpmpp2m" serve that (solvers.select), the other solvers refuse it with a ValueError.
    `noise_streams`: one id per replay row (default: stream 0 everywhere -- all poses of a job share the injected noise, as
    sample.py:290-292 shares the start noise); `reseed` / `set_noise_streams` rewrite the device buffers, no re-capture.
    `known` / `mask` (both or neither): masked sampling.  known [bs, 4, H, W] fp32 = the latent to keep, mask [bs or 1, 1, H, W] fp32 at latent
    resolution, 1 = generate, 0 = keep.  Every step then ends in ONE more launch, after the solver's whole step (never between a solver's
    two evaluations): the region to keep is replaced by `known` at the step's new noise level (cd360_mask_blend_f32 of
    include/edit/cd360_edit.h, captured inside all three graphs; its noise is counter domain 3 under `seed` and the rows' streams, so such
    a sampler owns the seed / stream buffers and `reseed` / `set_noise_streams` serve it under a deterministic solver as well).  Both live
    in buffers the sampler owns: `set_known` rewrites them in place, no re-capture.  Without them the step is what it was: no buffer,
    launch or graph node is added.
    `step(x, i, first=True)` makes row i the first step of an image (the render runs there): with `start_from` the tail of a schedule from a
    given picture, image-to-image.  The solvers of PARTIAL_START serve it."""

    # a trajectory may begin at a row > 0 under these: "dpmpp2m" and "lms" key "no history yet" on row 0 of their tables
    PARTIAL_START = ("euler", "heun", "euler_a", "dpmpp2s_a")

    SOLVERS = tuple(solvers.SOLVERS)
    EDM_SOLVERS = tuple(k for k in solvers.EDM_SOLVERS if k not in solvers.SOLVERS)  # the names only the EDM registry serves
    HIGHORDER_SOLVERS = tuple(solvers.HIGHORDER_SOLVERS)

    def __init__(self, net, pose, ctx, y, n_steps, scale=7.5, scale_im=3.5, use_graph=False, prefetch=None, graph_render=True, solver="euler",
                 eta=1.0, s_noise=1.0, seed=0, noise_streams=None, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), order=4, discretization=None,
                 sigmas=None, known=None, mask=None):
        from cd360 import sampler as S
        if solver not in solvers.NAMES:
            raise ValueError(f"solver {solver!r}: the job sampler serves {', '.join(solvers.NAMES)}")
        if solver == "lms" and (isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= 4):
            raise ValueError(f"order {order!r}: the linear multistep solver serves orders 1..4")
        if discretization is not None and sigmas is not None:
            raise ValueError("give `discretization` or `sigmas`, not both")
        if sigmas is not None:
            if len(sigmas) != n_steps:
                raise ValueError(f"{len(sigmas)} sigmas for n_steps = {n_steps}")
            discretization = S.ListDiscretization(sigmas)
        self.solver, self.order = solver, order
        self.eta, self.s_noise, self.seed, self.noise_streams = eta, s_noise, seed, noise_streams
        self.s_churn, self.s_tmin, self.s_tmax = s_churn, s_tmin, s_tmax
        self.last_row = False  # True while the step at hand is a one-evaluation row of a two-evaluation solver (Solver.single_row)
        self.net, self.pose, self.n_steps = net, pose, n_steps
        if use_graph:  # the graphs read the cameras through ONE buffer this sampler owns (retarget rewrites it in place)
            from sgm.modules.utils_cameraray import PoseBuffer
            self.pose = PoseBuffer(pose, ctx.device)
        self.scale, self.scale_im = scale, scale_im
        dev = ctx.device
        # the reference's own stack (cd360/sampler.py mirrors sampling.py / guiders.py / denoiser.py; parity: tests/test_sampler_cpu.py)
        self.denoiser = S.DiscreteDenoiser().to(dev)
        two = scale_im is None or scale_im <= 0  # sample.py:231-240
        self.guider = S.VanillaCFGImgRef(scale) if two else S.ScheduledCFGImgTextRef(scale, scale_im)
        self.branches = nb = self.guider.branches
        if two:
            self.scale_im = None  # (the tail kernels' two-branch request)
        if ctx.shape[0] % nb or y.shape[0] != ctx.shape[0] or (isinstance(pose, (list, tuple)) and len(pose) != ctx.shape[0]):
            raise ValueError(f"the {nb}-branch guider takes ctx / y / pose of {nb} x bs rows, got {ctx.shape[0]} / {y.shape[0]} / "
                             f"{len(pose) if isinstance(pose, (list, tuple)) else '?'}")
        # n_steps + 1 values, last = 0: the legacy schedule unless the caller names another (cd360.sampler: EDMDiscretization,
        # ListDiscretization, or anything with their call protocol)
        disc = S.LegacyDDPMDiscretization() if discretization is None else discretization
        self.sigmas = disc(n_steps, device=dev)
        # once per schedule, on the host's own evaluation of it (no step reads anything back): the denoiser's table is the host's evaluation
        # of the legacy schedule, and the device's square root may differ from it in the last bit -- which moves no sigma off the grid
        self.on_grid = S.on_grid(disc(n_steps), self.denoiser)
        self._solver = solvers.select(solver, s_churn, self.on_grid)  # what only that solver knows (off the grid: or a ValueError)
        # conditioning is constant over a trajectory: the guider's (uc, uc, c) / (uc, c) batch is assembled once per image, not per step
        self.bs = bs = ctx.shape[0] // nb  # diffusion samples (target poses) per replay: ctx / y hold [uc x bs | . | c x bs] / [uc x bs | c x bs]
        cond3 = self._cond_batch(ctx, y)
        self.ctx, self.y = cond3["crossattn"].contiguous(), cond3["vector"].contiguous()
        self.prefetch = prefetch  # cd360.prefetch.WeightPrefetcher or None: armed around both captures
        self.use_graph, self.graph, self.lgraph, self._prepared = use_graph, None, None, False
        self.gi = None  # the device-side step index: _build_state, on the first step
        self.graph_render, self.rgraph = use_graph and graph_render, None  # graph_render=False: the render step launched eagerly (A/B)
        # staged steps (round 6): the captured graphs read every per-step scalar from tables through a device-side step index and start /
        # end on cd360_unet_stage_in / cd360_cfg_euler_step_cl, so a replay holds no torch-issued kernel (cd360.routes.no_stage: the A/B partner);
        # eager launches (use_graph=False) run the same staged step
        from cd360 import routes
        self.staged = bool(not routes.no_stage and self._stageable())
        check_known(self.bs, known, mask)
        self.masked = known is not None  # decided once: the captured graphs hold the blend or they do not
        self.known_buf = self.mask_buf = None  # _build_state, on the first step; until then the caller's tensors wait here
        self._known = (known, mask)
        self._state_layout()

    def _state_layout(self):
        """Tell the pose blocks how this sampler's CFG batch is laid out (B bs rows, the first bs unconditional) instead of leaving them to
        infer it from `batch % 3`: six rows are two branches of three poses as well as three branches of two.  Restated before every
        render, so samplers of both guiders can share one UNet."""
        from cd360 import sampling
        sampling.set_cfg_branches(self.net, self.branches)

    def _cond_batch(self, ctx, y):
        """The guider's conditioning batch ((uc, uc, c) resp. (uc, c) rows) from ctx / y = [uc x bs | . | c x bs] resp. [uc x bs | c x bs]."""
        bs, nb = self.bs, self.branches
        c = {"crossattn": ctx[(nb - 1) * bs:], "vector": y[(nb - 1) * bs:]}
        uc = {"crossattn": ctx[:bs], "vector": y[:bs]}
        return self.guider.prepare_inputs(ctx.new_zeros(bs, 1), ctx.new_zeros(bs), c, uc)[2]

    def retarget(self, pose, ctx, y):
        """Point the sampler at another target pose / conditioning (the next pose of this rank's share).  The captured graphs read both
        through fixed device buffers, so the new values are copied INTO them: the CFG conditioning batch, and the packed
        [B bs, n+1, 16] camera tensor this sampler owns (sgm/modules/utils_cameraray.py::PoseBuffer)."""
        cond3 = self._cond_batch(ctx, y)
        self.ctx.copy_(cond3["crossattn"])
        self.y.copy_(cond3["vector"])
        if self.use_graph:
            self.pose.rewrite(pose)
        else:
            self.pose = pose
        if self.staged and getattr(self, "lab", None) is not None:
            self.lab.copy_(self.net.label_emb(self.y.to(self.net.dtype)))

    # ------------------------------------------------------------------------------------------------ staged steps
    def _stageable(self) -> bool:
        """The staged step serves the UNet this package builds (4 -> C input convolution, 4-channel output, merged emb projections)."""
        from cd360 import routes
        net = self.net
        try:
            conv = net.input_blocks[0][0]
            return (isinstance(conv, torch.nn.Conv2d) and conv.in_channels == 4 and conv.kernel_size == (3, 3) and conv.padding == (1, 1)
                    and conv.stride == (1, 1) and conv.out_channels % 8 == 0 and conv.weight.dtype == torch.bfloat16 and conv.weight.is_cuda
                    and net.out[2].out_channels == 4 and hasattr(net, "forward_staged") and not routes.no_emb_merge)
        except (AttributeError, IndexError, TypeError):
            return False

    def _build_state(self, x):
        """What a step of every route reads on the device besides the latent: the step index gi (_iota holds its values, so setting it is
        one 4-byte device copy) and the solver's own table and buffers."""
        self._iota = torch.arange(self.n_steps, dtype=torch.int32, device=x.device)
        self.gi = torch.zeros(1, dtype=torch.int32, device=x.device)
        self._solver.build(self, x)
        if self.masked:
            known, mask = self._known
            check_known(self.bs, known, mask, tuple(x.shape))
            self.known_buf = known.to(x.device).expand(x.shape).contiguous().clone()
            self.mask_buf = mask.to(x.device).contiguous().clone()
            self._known = None
            if not self._solver.draws(self):  # a masked sampler draws the kept region's noise even under a deterministic solver
                solvers.Solver.noise_buffers(self, x)

    @torch.no_grad()
    def _build_stage(self, x):
        """Per-schedule tables and static buffers of the staged steps: row i = what step i of the trajectory derives from sigma_i alone,
        computed with the denoiser's / the UNet's own modules exactly as the un-staged step computes them inside its graph."""
        self.step_tab, sqs = self.step_table()  # (before the solver's own tables: one of them may be this table with a column replaced)
        self._build_state(x)
        net, dev, dt = self.net, x.device, self.net.dtype
        self.temb_tab = self.temb_rows(sqs)
        conv = net.input_blocks[0][0]
        self.w36 = conv.weight.detach().float().permute(2, 3, 1, 0).reshape(36, conv.out_channels).contiguous()
        self.b_in = (conv.bias.detach().float() if conv.bias is not None else torch.zeros(conv.out_channels, device=dev)).contiguous()
        self.lab = net.label_emb(self.y.to(dt)).contiguous()
        nbs, (H, W) = self.y.shape[0], x.shape[2:]  # B bs images
        self.h0 = torch.empty(nbs, H * W, conv.out_channels, dtype=dt, device=dev)
        self.emb_act = torch.empty_like(self.lab)
        self._solver.build_stage(self)

    @torch.no_grad()
    def step_table(self):
        """(step_tab [n, 4] fp32 = (sigma_i, sigma_next, c_in(q_i), 0), q [n]) with q_i = the denoiser's snap of sigma_i, c_in through the
        denoiser's own module on the device."""
        rows, sqs = [], []
        for i in range(self.n_steps):
            sq = self.denoiser.possibly_quantize_sigma(self.sigmas[i].reshape(1))
            c_in = self.denoiser.scaling(sq)[2]
            rows.append(torch.stack([self.sigmas[i], self.sigmas[i + 1], c_in[0], torch.zeros_like(c_in[0])]))
            sqs.append(sq[0])
        return torch.stack(rows).float().contiguous(), torch.stack(sqs)

    @torch.no_grad()
    def temb_rows(self, sq):
        """A time-embedding table: sq [n] = sigmas ON the denoiser's grid (the schedule's own for temb_tab; a solver's other evaluation
        points) -> [n, E], row by row through the denoiser's / the UNet's own modules, so equal grid entries give equal bits."""
        from sgm.modules.diffusionmodules.util import timestep_embedding
        net, dt = self.net, self.net.dtype
        tembs = []
        for i in range(sq.numel()):
            c_noise = self.denoiser.possibly_quantize_c_noise(self.denoiser.scaling(sq[i].reshape(1))[3])
            tembs.append(net.time_embed(timestep_embedding(c_noise.expand(self.branches), net.model_channels).to(dt))[0])
        return torch.stack(tembs).to(dt).contiguous()

    def set_known(self, known, mask):
        """Another picture to keep and / or another region (the next pose of a job): copied INTO the buffers the captured blend reads, no
        re-capture.  known [bs or 1, 4, H, W], mask [1, 1, H, W] or as many rows as the sampler was built with."""
        if not self.masked:
            raise ValueError("this sampler was built without known / mask: its step and its graphs hold no blend")
        if self.known_buf is None:  # before the first step
            check_known(self.bs, known, mask)
            self._known = (known, mask)
            return
        check_known(self.bs, known, mask, tuple(self.known_buf.shape))
        if mask.shape[0] not in (1, self.mask_buf.shape[0]):
            raise ValueError(f"a mask of {mask.shape[0]} rows for a sampler built with {self.mask_buf.shape[0]}")
        self.known_buf.copy_(known)
        self.mask_buf.copy_(mask)

    def _blend(self, out, sigma_next):
        """The end of a masked step, stated once for every solver and route: `out` = the latent after the solver's whole step, sigma_next
        the step table (staged: the kernel reads column 1 of the step's row) or the schedule's own sigma_next as a device scalar."""
        if not self.masked:
            return out
        from cd360 import ops
        return ops.mask_blend(out, self.known_buf, self.mask_buf, sigma_next, self.gi, self.seed_buf, self.streams_buf)

    def _need_noise(self):
        if not (self.masked or self._solver.draws(self)):
            raise ValueError(f"solver {self.solver!r} with s_churn = {self.s_churn} draws no noise")

    def reseed(self, seed):
        """Another seed for the injected noise: one 8-byte copy into the buffer the captured tails read (no re-capture)."""
        from cd360.sampler import seed_words
        self._need_noise()
        self.seed = seed
        if getattr(self, "seed_buf", None) is not None:
            self.seed_buf.copy_(torch.tensor([seed_words(seed)], dtype=torch.int64))

    def set_noise_streams(self, ids):
        """One noise stream id per replay row (rows of equal id receive equal noise): copied into the buffer the captured tails read."""
        self._need_noise()
        ids = [int(v) for v in ids]
        if len(ids) != self.bs:
            raise ValueError(f"{len(ids)} noise stream ids for {self.bs} replay rows")
        self.noise_streams = ids
        if getattr(self, "streams_buf", None) is not None:
            self.streams_buf.copy_(torch.tensor(ids, dtype=torch.int32))

    def _evaluate(self, x, tab, temb):
        """One staged network evaluation on latent x: stage-in kernel (rep = B) on the step's row of `tab` / `temb` -> UNet trunk -> the
        output convolution's rows as they lie."""
        from cd360 import ops
        H, W = x.shape[2:]
        ops.unet_stage_in(x, tab, self.gi, self.w36, self.b_in, temb, self.lab, self.h0, self.emb_act)
        return self.net.forward_staged(self.h0, self.emb_act, self.ctx, self.pose, H, W)

    def _math_staged(self):
        """One sampler step on the static buffers, in place on self.gx, as the solver lays it out: for the one-evaluation solvers stage-in
        on step_tab / temb_tab -> UNet trunk -> the solver's tail kernel (for Euler the fused [c_out, CFG, to_d, Euler])."""
        return self._blend(self._solver.staged_step(self, self._evaluate), self.step_tab)

    def _unet(self, x_in, c_noise):
        return self.net(x_in, timesteps=c_noise, context=self.ctx, y=self.y, pose=self.pose)[0]

    def _math(self, x, s, s_next):
        """One un-staged sampler step = guider.prepare_inputs -> DiscreteDenoiser (sigma -> table index, c_in) -> UNet -> the solver's
        fused tail kernel (for Euler [c_out, CFG, to_d, Euler]) on the row _set_step wrote."""
        return self._blend(self._solver.step(self, self._unet, x, s, s_next), s_next)

    def _math_static(self):
        """The step as both graphs capture it: on the sampler's own buffers."""
        return self._math_staged() if self.staged else self._math(self.gx, self.gs[0], self.gs[1])

    @torch.no_grad()
    def eps(self, x, i):
        """The UNet's output for step i of the schedule (the guider's CFG branches), launched eagerly: what --fp8-attn's tolerance report compares."""
        from cd360.sampler import cfg_eps
        self._state_layout()
        return cfg_eps(self.denoiser, self._unet, x, self.sigmas[i], self.branches).float()

    def _pin_rendered(self):
        """Keep every block's cached render in a fixed buffer so a captured graph keeps reading the current image's render."""
        from cd360 import sampling
        for _, blk in sampling.pose_blocks(self.net):
            blk.pin_rendered()  # render + its pose_emb_layers half (rendered_feat @ Wb^T) in buffers that stay put across images
        for att in sampling._cross_attentions(self.net):  # same for the per-image context K / V^T cache
            if att._kv_cache is None:
                continue
            key, (k, vt, nk) = att._kv_cache[:2]
            st = getattr(att, "_static_kv", None)
            if st is None or st[0].shape != k.shape:
                att._static_kv = (k.clone(), vt.clone())
            else:
                st[0].copy_(k)
                st[1].copy_(vt)
            att._kv_cache = (key, (att._static_kv[0], att._static_kv[1], nk)) + tuple(att._kv_cache[2:])
            from cd360 import routes
            if routes.fp8_attn and 64 < nk <= 96:  # --fp8-attn: the e4m3 image of the pinned K / V, re-packed by every (captured) render step
                sk = att._static_kv[0]
                if getattr(att, "_static_kv8", None) is None or att._static_kv8[0].shape[0] != sk.shape[0]:
                    att._static_kv8 = ops_kv8_buffers(sk, att.heads)
                from cd360 import ops
                ops.kv_pack_fp8(sk, att._static_kv[1], nk, att.heads, out=att._static_kv8)
                att._kv8_cache = (sk, sk._version, att._static_kv8)

    def _capture(self, fn):
        """Warm `fn` on a side stream (allocator / library workspaces), then capture it into a hipGraph."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        # under torch.distributed the process group's watchdog thread may still poll the events of finished collectives (the launch
        # barrier) while this thread captures: only the thread-local capture mode tolerates that (tools/probe/rccl_graph_probe.py)
        import torch.distributed as dist
        mode = "thread_local" if dist.is_available() and dist.is_initialized() else "global"
        import contextlib
        from . import memo
        memo.new_epoch()  # values memoised by the eager warm-up (or by the other capture) must be re-derived inside this graph
        with torch.cuda.graph(graph, capture_error_mode=mode):
            # every GEMM / convolution launch of the captured step also enqueues, on a forked side stream, a touch of its weights that runs
            # beside the preceding launches (one step streams 5.3 GB of weights through a 256 MB Infinity Cache: cd360/prefetch.py)
            with (self.prefetch if self.prefetch is not None else contextlib.nullcontext()):
                out = fn()
        memo.new_epoch()
        return graph, out

    def _render(self):
        """Step 0 of an image: clear the cached render, run the full step (all 12 FeatureNeRF renders), re-pin the caches."""
        from cd360 import sampling
        sampling.clear_rendered_feat(self.net)
        self._state_layout()
        out = self._math_static()
        self._pin_rendered()
        return out

    @torch.no_grad()
    def prepare(self, x):
        """Untimed set-up of the graph mode: one eager render (builds the per-image tables and the static cache buffers), then the
        steady-state step and the render step are each captured once -- and, for a solver some of whose rows have another shape (Heun's
        sigma_next = 0 step, DPM++ 2S's sigma_down = 0 rows: one evaluation instead of two), that shape a third time.  All graphs read /
        write the same static buffers."""
        if not self.use_graph or self._prepared:
            return
        self._prepared = True
        self.gx, self.gs = x.clone(), self.sigmas[0:2].clone()
        if self.staged:
            self._build_stage(x)
        else:
            self._build_state(x)
        single = [self._solver.single_row(self, i) for i in range(self.n_steps)]
        if single[0] and self.n_steps == 1:
            return  # the only step renders AND is a one-evaluation row: launched un-captured
        self._render()
        if self.staged:
            self.gx.copy_(x)  # (the staged step updates gx in place: captures and warm-ups below start from a sane latent again)
        self.graph, self.gout = self._capture(self._math_static)
        if any(single):
            self.last_row = True
            try:
                self.lgraph, self.lout = self._capture(self._math_static)
            finally:
                self.last_row = False
        if self.graph_render and not single[0]:  # (a one-evaluation row 0 renders un-captured)
            try:
                self.rgraph, self.rout = self._capture(self._render)
                self._pins = self._snapshot_pins()
            except Exception as e:  # a host synchronisation inside the render path would make it uncapturable: stay eager
                print(f"[bench] render step not captured ({type(e).__name__}: {e}); launching it eagerly", file=sys.stderr)
                self.rgraph = None
                torch.cuda.synchronize()

    def _snapshot_pins(self):
        from cd360 import sampling
        return ([(blk, blk.rendered_feat, blk._rendered_proj) for _, blk in sampling.pose_blocks(self.net)],
                [(att, att._kv_cache) for att in sampling._cross_attentions(self.net)])

    def _restore_pins(self):
        for blk, r, proj in self._pins[0]:
            blk.rendered_feat, blk._rendered_proj = r, proj
        for att, kv in self._pins[1]:
            att._kv_cache = kv

    def _set_step(self, i):
        """Every per-step buffer write.  Staged: the step index alone (the kernels pick their table rows through it).  Un-staged: the
        solver's own row and, for the captured step, sigma / sigma_next."""
        if self.staged:
            self.gi.copy_(self._iota[i:i + 1])
            return
        self._solver.set_row(self, i)
        if self.masked and solvers.GI not in self._solver.rows_of(self):  # (the blend's step word, where the solver itself reads none)
            self.gi.copy_(self._iota[i:i + 1])
        if self.use_graph:
            self.gs[0].copy_(self.sigmas[i])
            self.gs[1].copy_(self.sigmas[i + 1])

    @torch.no_grad()
    def step(self, x, i, alias: bool = False, first: bool = False):
        """Step i of the schedule on latent x.  alias=True (the job loop): the result may be the sampler's own latent buffer, valid until
        the next call, and passing it straight back skips the copy-in -- a staged replay is then ONE 4-byte index copy plus the graph.
        first=True: row i is the first step of an image (a trajectory that begins at `start_from`'s latent): the cached render is cleared
        and the render runs there as it does on row 0 -- the render graph where row i has the captured shape, un-captured otherwise."""
        i = i % self.n_steps
        if first:
            check_first_step(self.solver, i, self.n_steps)
        # (eager launches of a staged sampler run the SAME staged step: the stage-in kernel's input convolution rounds a few outputs to the
        # other bf16 neighbour than the implicit-GEMM kernel does, and 70 random-init blocks amplify that to 1e-2 of eps -- graph and eager
        # must not differ by it; tests/test_f_rows_gpu.py holds the staged ends against the module arithmetic op by op)
        if self.use_graph:
            self.prepare(x)
        elif self.gi is None:
            if self.staged:
                self.gx = x.clone()
                self._build_stage(x)
            else:
                self._build_state(x)
        if (self.staged or self.use_graph) and x is not self.gx:  # these steps run on the sampler's own latent buffer
            self.gx.copy_(x)
        self._set_step(i)
        self.last_row = last = self._solver.single_row(self, i)
        render = i == 0 or first
        if not self.use_graph:
            if render:
                from cd360 import sampling
                sampling.clear_rendered_feat(self.net)  # new image: the render runs again
                self._state_layout()
            out = self._math_staged() if self.staged else self._math(x, self.sigmas[i], self.sigmas[i + 1])
        elif not render:
            (self.lgraph if last else self.graph).replay()
            out = self.lout if last else self.gout
        elif self.rgraph is not None and not last:
            self.rgraph.replay()
            self._restore_pins()
            out = self.rout
        else:
            out = self._render()
        if self.staged:  # out is gx
            return out if alias else out.clone()
        return out.clone() if self.use_graph else out


def ops_kv8_buffers(k, heads):
    return (torch.empty(k.shape[0], heads, 96 * 64 + 64 * 128, dtype=torch.uint8, device=k.device),
            torch.empty(k.shape[0], heads, 2, dtype=torch.float32, device=k.device))


def sample_assigned(sampler, jobs: Sequence[tuple], steps: int, first_step: int = 0, edits=None) -> List[torch.Tensor]:
    """The per-rank loop of the job: `jobs` = [(pose, ctx, y, x0), ...] for the poses of this rank, in `shard.assign_poses` order; every
    pose walks rows `first_step` .. `steps` - 1 of the sampler's schedule from its own start latent (the first of them renders).  `sampler`
    needs `retarget(pose, ctx, y)` and `step(x, i)` -- `Sampler` above; the gloo tests drive the same loop with a CPU stand-in.
    `edits`: one (known, mask) per job, handed to `sampler.set_known` before the pose's first step (masked sampling)."""
    if first_step:
        check_first_step(getattr(sampler, "solver", None), first_step, steps)
    finals = []
    for j, (pose, ctx, y, x0) in enumerate(jobs):
        if j > 0:
            sampler.retarget(pose, ctx, y)
        if edits is not None:
            sampler.set_known(*edits[j])
        x = x0.clone()
        alias = isinstance(sampler, Sampler)  # (the CPU stand-ins of the gloo tests take (x, i) only)
        for i in range(first_step, steps):
            x = sampler.step(x, i, alias=True, first=i == first_step) if alias else sampler.step(x, i)
        finals.append(x.clone() if alias else x)
    return finals


def sample_poses(make_sampler: Callable, make_job: Callable[[int], tuple], num_poses: int, steps: int, world: int = 1, rank: int = 0,
                 first_step: int = 0):
    """BASELINE configs[2] as a function: `num_poses` target poses over `world` ranks.  `make_job(p)` builds pose p's (pose, ctx, y, x0);
    `make_sampler(pose, ctx, y)` the rank's sampler for its first pose.  Returns (latents of ALL poses [num_poses, 4, L, L] in pose
    order, identical on every rank; this rank's pose indices).  No collective on the data path; one all-gather at the end.
    `first_step`: every pose walks rows first_step .. steps - 1 from its x0 (`start_from` makes one from a known latent)."""
    if num_poses < world:  # decided from the arguments alone, so EVERY rank raises (a rank-local check would leave the others in the all-gather)
        raise ValueError("more ranks than target poses: every rank needs at least one pose (the all-gather is sized per rank)")
    mine = shard.assign_poses(num_poses, world, rank)
    jobs = [make_job(p) for p in mine]
    sampler = make_sampler(*jobs[0][:3])
    finals = sample_assigned(sampler, jobs, steps, first_step)
    return shard.gather_latents(torch.cat(finals, 0), num_poses), mine


@torch.no_grad()
def start_from(sampler, known: torch.Tensor, k: int, seed: int, streams=None) -> torch.Tensor:
    """The latent a trajectory begins with at row k >= 1 of the sampler's schedule when it starts from a known latent instead of pure
    noise (image-to-image): known + sigma_k z, [bs, 4, H, W] fp32, z = counter domain 3 at step word k - 1 under `seed` and the rows'
    stream ids (default: stream 0 everywhere).  Computed by the blend itself with the mask 0 everywhere on row k - 1, so it is exactly the
    latent a fully-kept masked run holds after step k - 1.  k = 0 is `start_latent`.  Reads `sampler.sigmas` / `sampler.bs` alone."""
    from cd360 import ops
    from cd360.sampler import seed_words
    sig = sampler.sigmas
    n = sig.numel() - 1
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k < n:
        raise ValueError(f"k = {k!r}: start_from serves rows 1 .. {n - 1} of the {n}-step schedule (row 0 starts from noise alone: start_latent)")
    bs = int(getattr(sampler, "bs", 1))
    if streams is not None and len(streams) != bs:
        raise ValueError(f"{len(streams)} noise stream ids for {bs} replay rows")
    check_known(bs, known, torch.zeros((1, 1) + tuple(known.shape[2:])) if isinstance(known, torch.Tensor) and known.ndim == 4 else None)
    dev = sig.device
    known = known.to(dev).expand((bs,) + tuple(known.shape[1:])).contiguous()
    seed_t = torch.tensor([seed_words(seed)], dtype=torch.int64, device=dev)
    streams_t = None if streams is None else torch.tensor([int(v) for v in streams], dtype=torch.int32, device=dev)
    step_t = torch.tensor([k - 1], dtype=torch.int32, device=dev)
    keep = torch.zeros((1, 1) + tuple(known.shape[2:]), dtype=torch.float32, device=dev)
    return ops.mask_blend(torch.zeros_like(known), known, keep, sig[k:k + 1].float().contiguous(), step_t, seed_t, streams_t)


@torch.no_grad()
def start_latent(sampler, H: int, W: int, seed: int, streams=None) -> torch.Tensor:
    """The start latent of a trajectory, [bs, 4, H, W] fp32 on the sampler's device: what `torch.randn` (sample.py:290-292) and
    `x *= torch.sqrt(1.0 + sigmas[0] ** 2.0)` (sampling.py:50) give the reference, drawn by cd360_start_noise_f32 as a pure function of
    (`seed`, the row's stream id, channel, pixel) -- not of torch's generator state, and unrelated to the noise a stochastic solver injects
    under the same seed (another domain of the counter, include/cd360_image.h).  `streams`: one id per row (default: stream 0 everywhere,
    every row the same latent).  Serves every solver: it reads `sampler.sigmas` / `sampler.bs` and none of the sampler's noise state."""
    from cd360 import ops
    from cd360.sampler import seed_words
    sig = sampler.sigmas
    bs = int(getattr(sampler, "bs", 1))
    if streams is not None and len(streams) != bs:
        raise ValueError(f"{len(streams)} noise stream ids for {bs} replay rows")
    scale = torch.sqrt(1.0 + sig[0] ** 2.0).float().reshape(1)  # sampling.py:50, by torch on the schedule's own sigma_0
    seed_t = torch.tensor([seed_words(seed)], dtype=torch.int64, device=sig.device)
    streams_t = None if streams is None else torch.tensor([int(v) for v in streams], dtype=torch.int32, device=sig.device)
    return ops.start_noise(seed_t, streams_t, scale, bs, H, W)


def sample_images(make_sampler: Callable, make_job: Callable[[int], tuple], num_poses: int, steps: int, first_stage, world: int = 1, rank: int = 0,
                  seed: int = 0, latent_hw=None, first_step: int = 0, init_latents=None, masks=None):
    """Poses and a seed in, images out: `sample_poses` with the first stage on every rank.  `make_job(p)` builds pose p's (pose, ctx, y, x0);
    where x0 is None the pose starts from `start_latent(sampler, *latent_hw, seed)` -- stream 0, so all poses share their start noise as in
    sample.py:290-292 -- and `latent_hw` = (H, W) of the latent must be given.  Each rank decodes ITS poses with `first_stage.decode_u8`
    (cd360/images.py::FirstStage, or anything with that method); the one collective is an all-gather of the uint8 images.  Returns (images
    [num_poses, H, W, 3] uint8 in pose order, identical on every rank and for every `world`; this rank's pose indices).
    `init_latents` [num_poses or 1, 4, H, W] (FirstStage.encode's output) with `masks` [num_poses or 1, 1, H, W] (images.latent_mask):
    masked sampling -- `make_sampler` must build its Sampler with a known / mask of that shape, and every pose's own pair is handed to it
    with `set_known`.  `first_step` > 0: every pose walks rows first_step .. steps - 1 only, and where x0 is None it starts from
    `start_from(sampler, its init latent, first_step, seed)` (image-to-image; `init_latents` alone is enough for that)."""
    if num_poses < world:  # decided from the arguments alone, so EVERY rank raises (see sample_poses)
        raise ValueError("more ranks than target poses: every rank needs at least one pose (the all-gather is sized per rank)")
    if masks is not None and init_latents is None:
        raise ValueError("`masks` without `init_latents`: a region to keep needs the latent it keeps")
    for name, t in (("init_latents", init_latents), ("masks", masks)):
        if t is not None and (t.ndim != 4 or t.shape[0] not in (1, num_poses)):
            raise ValueError(f"{name}: [{num_poses} or 1, ...] is needed, got {tuple(t.shape)}")
    mine = shard.assign_poses(num_poses, world, rank)
    jobs = [make_job(p) for p in mine]
    sampler = make_sampler(*jobs[0][:3])
    of_pose = lambda t, p: t[p:p + 1] if t.shape[0] > 1 else t  # noqa: E731
    if first_step:
        check_first_step(getattr(sampler, "solver", None), first_step, steps)
        if init_latents is None and any(j[3] is None for j in jobs):
            raise ValueError("first_step > 0 with x0 = None: sample_images needs `init_latents` to start from")
        jobs = [(pose, ctx, y, start_from(sampler, of_pose(init_latents, p), first_step, seed) if x is None else x)
                for p, (pose, ctx, y, x) in zip(mine, jobs)]
    if any(j[3] is None for j in jobs):
        if latent_hw is None:
            raise ValueError("make_job returned x0 = None: sample_images needs latent_hw = (H, W) to draw the start latent")
        x0 = start_latent(sampler, int(latent_hw[0]), int(latent_hw[1]), seed)
        jobs = [(pose, ctx, y, x0 if x is None else x) for pose, ctx, y, x in jobs]
    edits = None if masks is None else [(of_pose(init_latents, p), of_pose(masks, p)) for p in mine]
    finals = sample_assigned(sampler, jobs, steps, first_step, edits)
    images = torch.cat([first_stage.decode_u8(x) for x in finals], 0)
    return shard.gather_latents(images, num_poses), mine
