"""The live optimiser step on the GPU (include/optim/cd360_optim.h): the same bits as the closed AdamW kernel, an exact norm, clipping
against the torch fall-back, the EMA bit for bit against its torch restatement, a schedule reaching the replays of a captured step, and
every entry point under the guarded allocator.  Needs an MI355X.  Shapes: optim_cases.SHAPES."""
import functools
import math
import types

import pytest
import torch

import guarded as G
import optim_cases as OC
import sampler_cases as SC
import weights as W

DEV = "cuda"
BF = torch.bfloat16
KW = dict(lr=1e-4, betas=(0.9, 0.95), eps=1e-6)
KINDS = {"closed": {}, "live": {"live": True}, "loose": {"max_grad_norm": 1e9}}


# ================================================================================================ shared runs
@functools.lru_cache(maxsize=None)
def _base():
    return tuple(OC.tensors(7))


@functools.lru_cache(maxsize=None)
def _grads(steps=6, scale=1.0):
    """steps x tensors bf16 gradients, the misaligned tensor's misaligned again; computed once, never written."""
    return tuple(tuple(OC.tensors(100 + it, scale=scale)) for it in range(steps))


def _set_grads(ps, gs, skip=None):
    for i, (p, g) in enumerate(zip(ps, gs)):
        p.grad = None if i == skip else g


def _state(opt, ps):
    return dict(master=opt._master.clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(), steps=opt.steps.clone(),
                params=torch.cat([p.detach().reshape(-1) for p in ps]))


@functools.lru_cache(maxsize=None)
def _three_steps(kind):
    """3 steps of MasterAdamW(**KINDS[kind]) on the ragged set, tensor 2 without a gradient in the second; -> (state, library calls)."""
    from cd360 import _lib, _optim, finetune
    ps = OC.parameters(_base())
    opt = finetune.MasterAdamW(OC.groups(ps), **KW, **KINDS[kind])
    assert opt.fused and opt.live == (kind != "closed")
    recs = [G.Recorder(_lib.load()), G.Recorder(_optim.load())]
    saved = _lib.load, _optim.load
    _lib.load, _optim.load = (lambda check_symbols=True: recs[0]), (lambda: recs[1])
    try:
        for it in range(3):
            _set_grads(ps, _grads()[it], skip=2 if it == 1 else None)
            opt.step()
    finally:
        _lib.load, _optim.load = saved
    st = _state(opt, ps)
    st["coef"] = opt.clip_coef.clone() if opt.live else None
    return st, (tuple(recs[0].called), tuple(recs[1].called))


def _same(a, b, keys=("master", "exp_avg", "exp_avg_sq", "steps", "params")):
    return [k for k in keys if not torch.equal(a[k], b[k])]


# ================================================================================================ 5: same bits as the closed kernel
@pytest.mark.gpu
def test_live_kernel_without_clip_and_ema_writes_the_bits_of_the_closed_kernel():
    """cd360_adamw_live_bf16 with null coef and ema, lr / weight decay from the device table, against cd360_adamw_bf16 over 3 steps, tensor 2
    without a gradient in the second: masters, both moments, the step count and the bf16 parameters are torch.equal.  An optimiser built
    without the new arguments launches what it launched -- one tick and one cd360_adamw_bf16 per chunk and step, nothing of the third
    library -- and the live one the same count of its own kernel."""
    closed, calls_closed = _three_steps("closed")
    live, calls_live = _three_steps("live")
    assert not _same(live, closed), _same(live, closed)
    assert float(closed["steps"]) == 3
    assert calls_closed == (("cd360_adamw_tick", "cd360_adamw_bf16", "cd360_adamw_bf16") * 3, ())
    assert calls_live == (("cd360_adamw_tick",) * 3, ("cd360_adamw_live_bf16",) * 6)
    assert torch.equal(live["params"], torch.cat([m.reshape(-1) for m in _unflat(live["master"])]).to(BF))


def _unflat(master):
    out, off = [], 0
    for s in OC.SHAPES:
        n = math.prod(s)
        out.append(master[off:off + n])
        off += (n + 7) // 8 * 8
    return out


@pytest.mark.gpu
def test_live_kernel_equals_the_closed_kernel_where_the_grid_is_capped():
    """One tensor of 4096 x 256 + 300 vectors and 3 values: the update's grid stops at 4096 workgroups and every thread walks its stride a
    second time.  One step, live against closed: the same bits."""
    from cd360 import finetune
    n = (4096 * 256 + 300) * 8 + 3
    g = torch.Generator(device=DEV).manual_seed(5)
    base = torch.randn(n, generator=g, device=DEV).mul_(0.1).to(BF)
    grad = torch.randn(n, generator=g, device=DEV).to(BF)
    got = []
    for kw in ({}, {"live": True}):
        p = torch.nn.Parameter(base.clone())
        opt = finetune.MasterAdamW([p], **KW, **kw)
        p.grad = grad
        opt.step()
        got.append(_state(opt, [p]))
    assert not _same(got[1], got[0]), _same(got[1], got[0])
    assert not torch.equal(got[0]["params"], base)


# ================================================================================================ 6: exact norm
def _norm_of(grads, max_norm, chunk=None):
    """(sumsq, norm, coef, 0) of `grads` through ops.grad_clip_coef, with at most `chunk` tensors per launch; -> (out, npartials, launches)."""
    from cd360 import ops
    saved = ops.ADAMW_MAX_TENSORS
    try:
        if chunk is not None:
            ops.ADAMW_MAX_TENSORS = chunk
        plan = ops.LiveAdamwPlan([torch.empty_like(g) for g in grads], [0] * len(grads), list(range(len(grads))))
    finally:
        ops.ADAMW_MAX_TENSORS = saved
    partials = torch.full((plan.npartials,), float("nan"), device=DEV)
    out = torch.full((4,), float("nan"), device=DEV)
    ops.grad_clip_coef(plan, grads, partials, max_norm, out)
    return out.cpu(), plan.npartials, len(plan.chunks)


@pytest.mark.gpu
def test_norm_of_exactly_summable_gradients_is_exact():
    """Gradients from {0, +-0.5, +-1, +-2}: every square is a multiple of 0.25 and the total stays below 2^22, so every fp32 addition is
    exact in any order.  out[0] equals the fp64 sum; out[1] and out[2] equal torch's fp32 sqrt and division from it on the CPU, bit for bit;
    out[3] is 0; a loose max_norm gives exactly 1.  Reversed, and in launches of at most 7 tensors, the grid and the number of partials
    change, sumsq does not."""
    table = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], device=DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    grads = []
    for i, s in enumerate(OC.SHAPES):
        n = math.prod(s)
        t = table[torch.randint(0, 7, (n + 1,), generator=g, device=DEV)].to(BF)
        grads.append(t[1:] if i == OC.UNALIGNED else t[:n].clone())
    assert grads[OC.UNALIGNED].data_ptr() % 16 == 2
    exact = sum(float(t.double().square().sum()) for t in grads)
    assert 0 < exact < 2 ** 22 and exact * 4 == int(exact * 4)
    max_norm = 3.0
    s32 = torch.tensor(exact, dtype=torch.float32)
    assert float(s32) == exact
    norm = torch.sqrt(s32)
    coef = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)
    assert float(coef) < 1
    seen = set()
    for order, chunk in ((grads, None), (grads[::-1], None), (grads, 7)):
        out, npartials, launches = _norm_of(order, max_norm, chunk)
        seen.add((npartials, launches))
        print(f"sumsq {float(out[0])} (exact {exact}), norm {float(out[1])!r} (torch {float(norm)!r}), coef {float(out[2])!r} (torch {float(coef)!r}); "
              f"{npartials} partials in {launches} launches")
        assert float(out[0]) == exact
        assert torch.equal(out[1], norm) and torch.equal(out[2], coef) and float(out[3]) == 0.0
    assert len(seen) >= 2, seen
    out, _, _ = _norm_of(grads, 1e9)
    assert float(out[0]) == exact and float(out[2]) == 1.0


# ================================================================================================ 7: clipping
@pytest.mark.gpu
def test_a_loose_max_grad_norm_leaves_the_bits_of_the_unclipped_step():
    """max_grad_norm far above the norm: coef == 1 on the device, and g * 1 is g -- masters, moments and parameters are those of the run
    of test 5, bit for bit."""
    live, _ = _three_steps("live")
    loose, calls = _three_steps("loose")
    assert float(loose["coef"]) == 1.0
    assert not _same(loose, live), _same(loose, live)
    assert calls[1] == (("cd360_grad_sumsq_bf16",) * 2 + ("cd360_grad_clip_f32",) + ("cd360_adamw_live_bf16",) * 2) * 3


@pytest.mark.gpu
def test_a_binding_max_grad_norm_follows_clip_grad_norm_and_adamw():
    """max_grad_norm = 0.5 under gradients of norm ~ 150: 6 steps against MasterAdamW(fused=False, max_grad_norm=0.5) (clip_grad_norm_ on
    the fp32 master gradients + torch.optim.AdamW) on the same gradients.  Masters and both moments of every tensor at the bar of
    test_fused_adamw_matches_torch_adamw_on_fp32_masters: 2e-6 of the tensor's largest magnitude, for each tensor of 15 values or more by
    itself and for the 72 tensors of 1 to 8 values taken together.  A tensor of one value has no scale of its own: its master is the start
    value plus six updates of ~ lr each, torch forms the step size in float64 and the kernel in fp32 (1e-7 of each update), and where the
    sum happens to pass near zero that is any fraction of what is left -- measured per tensor: 4.3e-6 on the master of tensor 31 (value
    -3.1e-5 after a drift of ~ 1e-3) and 2.1e-6 on exp_avg of tensor 7 (a signed sum cancelled to 1/20 of its terms).  The bf16
    parameters are the rounded masters.  grad_norm against
    the fp64 norm: every square passes through 1 rounding of its own, OPTIM_SUMSQ_DEPTH additions inside its thread, 8 levels of the
    workgroup's tree, ceil(partials / 256) additions and 8 more levels in the clip kernel, each within 2^-24 relative of a sum of positive
    terms; the square root halves that and adds its own rounding.  For the launch this test runs that is below the bar of 1e-6."""
    from cd360 import finetune, ops
    pa, pb = OC.parameters(_base()), OC.parameters(_base())
    fused = finetune.MasterAdamW(OC.groups(pa), max_grad_norm=0.5, **KW)
    plain = finetune.MasterAdamW(OC.groups(pb), max_grad_norm=0.5, fused=False, **KW)
    assert fused.live and not plain.fused
    u = 2.0 ** -24
    for it in range(6):
        gs = _grads()[it]
        _set_grads(pa, gs)
        _set_grads(pb, gs)
        fused.step()
        plain.step()
        exact = math.sqrt(sum(float(g.double().square().sum()) for g in gs))
        depth = 1 + ops.OPTIM_SUMSQ_DEPTH + 8 + (fused._plan.npartials + 255) // 256 + 8
        bound = (1 + ((1 + u) ** depth - 1) / 2) * (1 + u) - 1
        err = abs(float(fused.grad_norm) - exact) / exact
        print(f"step {it + 1}: grad_norm {float(fused.grad_norm)!r}, fp64 {exact!r}, relative error {err:.2e} (bound {bound:.2e}), coef {float(fused.clip_coef):.6e}")
        assert bound <= 1e-6 and err <= bound
        assert 0 < float(fused.clip_coef) < 0.01 and 0 < float(plain.clip_coef) < 0.01
    assert float(fused.steps) == 6 and fused._plan.npartials == 3 and len(fused._plan.chunks) == 2
    rel = lambda x, y: float((x.float() - y.float()).abs().max() / y.float().abs().max().clamp_min(1e-12))
    assert all(torch.equal(a.detach(), ma.to(BF)) for a, ma in zip(pa, fused.master))
    big = [i for i, m in enumerate(fused.master) if m.numel() >= 15]
    small = [i for i, m in enumerate(fused.master) if m.numel() < 15]
    assert big == [0, 2, 4, 5, 6] and len(small) == 72
    cat = lambda ts, idx: torch.cat([ts[i].reshape(-1) for i in idx])
    for key, ours, theirs in (("master", fused.master, plain.master),
                              ("exp_avg", None, [plain.opt.state[mb]["exp_avg"] for mb in plain.master]),
                              ("exp_avg_sq", None, [plain.opt.state[mb]["exp_avg_sq"] for mb in plain.master])):
        if ours is None:
            ours = [getattr(fused, key)[b:b + m.numel()] for b, m in zip(fused._begin, fused.master)]
        worst = [rel(ours[i].reshape(-1), theirs[i].reshape(-1)) for i in big] + [rel(cat(ours, small), cat(theirs, small))]
        print(key, "tensors 0, 2, 4, 5, 6 and the 72 small ones together:", " ".join("%.2e" % w for w in worst))
        assert max(worst) < 2e-6, (key, worst)


# ================================================================================================ 8: EMA
@pytest.mark.gpu
def test_ema_equals_its_torch_restatement_bit_for_bit_and_ema_scope_swaps_it_in():
    """ema_decay = 0.5, clipping on.  After each of 4 steps the flat EMA equals optim_cases.ema_update (one fp32 operation at a time) of the
    previous EMA and the masters the kernel itself wrote.  (1 + t) / (10 + t) stays below 0.5 up to t = 8, so those 4 steps take the
    warm-up branch only; the step counter is then set to 6 and 4 more steps run, t = 7 .. 10: below the cap, equal to it, and twice at
    the cap.  ema_scope(): inside, the parameters are bf16(ema) and a pack derived from one of them (cd360.derived, keyed on `_version`)
    is rebuilt; after, they are bf16(master) again and the pack is rebuilt once more."""
    from cd360 import finetune
    from cd360.derived import derived
    ps = OC.parameters(_base())
    opt = finetune.MasterAdamW(OC.groups(ps), max_grad_norm=0.5, ema_decay=0.5, **KW)
    assert opt.live and opt._ema.dtype == torch.float32 and torch.equal(opt._ema, opt._master) and opt._ema.data_ptr() != opt._master.data_ptr()
    ts = []
    for it in range(8):
        if it == 4:
            opt.steps.fill_(6.0)
        t = float(opt.steps) + 1
        ts.append(t)
        prev = opt._ema.clone()
        _set_grads(ps, _grads()[it % 6])
        opt.step()
        assert float(opt.steps) == t
        want = OC.ema_update(prev, opt._master, t, 0.5)
        assert torch.equal(opt._ema, want), (t, int((opt._ema != want).sum()))
        assert not torch.equal(opt._ema, prev) and not torch.equal(opt._ema, opt._master)
    assert ts == [1, 2, 3, 4, 7, 8, 9, 10]
    assert [(1 + t) / (10 + t) > 0.5 for t in ts] == [False] * 6 + [True] * 2  # both branches of the min
    assert all(torch.equal(e.reshape(-1), opt._ema[b:b + e.numel()]) for e, b in zip(opt.ema, opt._begin))
    owner, p = types.SimpleNamespace(), ps[0]
    pack = lambda: derived(owner, "_pack_t", [p], lambda: p.detach().t().contiguous().clone())
    before = pack()
    assert pack() is before
    with opt.ema_scope():
        assert all(torch.equal(q.detach(), e.to(BF)) for q, e in zip(ps, opt.ema))
        inside = pack()
        assert inside is not before and torch.equal(inside, opt.ema[0].to(BF).t())
        assert not torch.equal(inside, before)
    after = pack()
    assert after is not inside and torch.equal(after, before)
    assert all(torch.equal(q.detach(), m.to(BF)) for q, m in zip(ps, opt.master))
    sd = opt.ema_state_dict([f"w{i}" for i in range(len(ps))])
    assert all(v.dtype == torch.float32 and torch.equal(v, e) for v, e in zip(sd.values(), opt.ema))


# ================================================================================================ 9: live lr on replays
def _schedule():
    from sgm.lr_scheduler import LambdaLinearScheduler
    return LambdaLinearScheduler(warm_up_steps=[2], f_min=[0.0], f_max=[1.0], f_start=[0.1], cycle_lengths=[10])


def _live_opt(scheduled=True):
    from cd360 import finetune
    ps = OC.parameters(_base())
    opt = finetune.MasterAdamW(OC.groups(ps), max_grad_norm=0.5, ema_decay=0.5, **KW)
    sched = finetune.LRSchedule(opt, _schedule())
    return ps, opt, sched


def _full_state(opt, ps):
    return dict(_state(opt, ps), ema=opt._ema.clone())


@pytest.mark.gpu
def test_a_schedule_reaches_the_replays_of_a_captured_live_step():
    """opt.step() alone (clipping and EMA on, static gradient buffers) captured into one torch.cuda.graph and replayed 4 times under
    LRSchedule(LambdaLinearScheduler), sync_hyper() between the replays: masters, moments, EMA, parameters and the step count are
    torch.equal to an eager live optimiser that took the same 4 steps, and differ from a run whose lr stayed at its capture value."""
    keys = ("master", "exp_avg", "exp_avg_sq", "steps", "params", "ema")
    runs = {}
    for name in ("eager", "frozen"):
        ps, opt, sched = _live_opt()
        lrs = []
        for it in range(4):
            _set_grads(ps, _grads()[it])
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            if name == "eager":
                sched.step()
        runs[name] = _full_state(opt, ps)
        assert (len(set(lrs)) == 4) == (name == "eager")
    ps, opt, sched = _live_opt()
    static = [g.clone() if g.storage_offset() == 0 else torch.cat([g[:1], g])[1:] for g in _grads()[0]]
    _set_grads(ps, static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    assert float(opt.steps) == 0  # the capture executes nothing
    for it in range(4):
        for s, g in zip(static, _grads()[it]):
            s.copy_(g)
        assert opt.sync_hyper() is True and opt.sync_hyper() is False  # this step's lr differs from the table's; then nothing to do
        graph.replay()
        sched.step()
    opt.bump_versions()
    torch.cuda.synchronize()
    got = _full_state(opt, ps)
    assert not _same(got, runs["eager"], keys), _same(got, runs["eager"], keys)
    assert float(got["steps"]) == 4
    assert set(_same(got, runs["frozen"], keys)) == {"master", "params", "ema"}  # (the moments do not depend on lr)


def _tiny():
    """The model of tests/test_lora_gpu.py's GraphedTrainStep test, without adapters."""
    from make_golden_params import UNET_TINY
    from sgm.modules.diffusionmodules.openaimodel import UNetModel
    torch.manual_seed(3)
    net = UNetModel(**{**UNET_TINY, "add_lora": False, "use_prev_weights_imp_sample": False})
    W.load_into(net, seed=4)
    return net.to(DEV, BF)


def _batch(seed=5, b=2, n=2, L=16):
    from cd360 import synth
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    return dict(noised=rn(b, 4, L, L), timesteps=torch.full((b,), 500.0, device=DEV), context=rn(b + b * n, 77, 32), y=rn(b + b * n, 16),
                pose=synth.pose_batch(b, n, seed=3), input_ref=rn(b, n, 4, L, L), sigmas_ref=torch.full((b,), 3.0, device=DEV),
                target=rn(b, 4, L, L), target_rgb=rn(b, 3, 8 * L, 8 * L).clamp(-1, 1), w=torch.full((b, 1, 1, 1), 0.7, device=DEV),
                mask=torch.ones(b, 1, L, L, device=DEV), opacity=torch.sigmoid(3 * rn(b, 1, 8 * L, 8 * L)))


@pytest.mark.gpu
def test_graphed_train_step_follows_a_schedule_down_to_lr_zero():
    """GraphedTrainStep on the tiny UNet with max_grad_norm set, under a schedule of factors 1, 0.5, 0 over 3 replays: the losses are finite,
    the step count is the warm-up's plus one per replay, the second replay (lr x 0.5) moves the masters and the last (lr x 0: decay
    1 - 0 x wd = 1, step size 0) leaves every master as it was while the moments still move -- the replay read this step's lr."""
    from cd360 import finetune
    from make_golden_params import LOSS_CFG
    from sgm.lr_scheduler import LambdaLinearScheduler
    from sgm.util import instantiate_from_config
    net = _tiny()
    net.eval()
    finetune.select_trainable(net, "pose")
    loss_fn = instantiate_from_config({"target": "sgm.modules.diffusionmodules.loss.StandardDiffusionLossImgRef", "params": LOSS_CFG})
    opt = finetune.MasterAdamW(finetune.optimizer_param_groups(net, "pose", lr=1e-3), lr=1e-3, max_grad_norm=1.0)
    assert opt.fused and opt.live
    sched = finetune.LRSchedule(opt, LambdaLinearScheduler(warm_up_steps=[0], f_min=[0.0], f_max=[1.0], f_start=[1.0], cycle_lengths=[2]))
    warmup = 2
    step = finetune.GraphedTrainStep(net, loss_fn, opt, _batch(), warmup=warmup)
    print("steps after construction:", float(opt.steps))
    assert float(opt.steps) == warmup  # the capture executes nothing
    losses, moved = [], []
    for it in range(3):
        before = (opt._master.clone(), opt.exp_avg.clone())
        losses.append(float(step()[0]))
        moved.append((not torch.equal(opt._master, before[0]), not torch.equal(opt.exp_avg, before[1])))
        if it < 2:
            sched.step()
    print("losses:", losses, "factors 1, 0.5, 0; (masters, moments) moved:", moved, "grad_norm", float(opt.grad_norm), "coef", float(opt.clip_coef))
    assert all(math.isfinite(v) for v in losses)
    assert float(opt.steps) == warmup + 3
    assert moved == [(True, True), (True, True), (False, True)]
    assert math.isfinite(float(opt.grad_norm)) and 0 < float(opt.clip_coef) <= 1


# ================================================================================================ 10: guarded memory
GUARDED = [("three-entry-points-ragged", OC.NEW)]
G_SHAPES = [(20000,), (1,), (3, 5), (77,)]  # two workgroups of the sum of squares; tails of 1, 7 and 5 values; the last one misaligned


@pytest.mark.gpu
@pytest.mark.parametrize("declares", [c[1] for c in GUARDED], ids=[c[0] for c in GUARDED])
def test_optim_entry_points_write_their_outputs_only(declares):
    """The three entry points under tests/guarded.py, both poison patterns: gradients, parameters, the hyper table, the partials, the 4
    result values, masters, moments, EMA and the step count live in arena blocks between canaries (the padding between tensors of the flat
    buffers is poisoned too), so no guard byte changes; the results are finite and bit-equal between the poisons; gradients and hyper are
    unchanged by all three, the partials by the clip kernel; all three entry points ran."""
    from cd360 import _optim, ops
    g = torch.Generator(device=DEV).manual_seed(3)
    inputs = {}
    for i, s in enumerate(G_SHAPES):
        inputs[f"g{i}"] = torch.randn(*s, generator=g, device=DEV).to(BF)
        inputs[f"w{i}"] = torch.randn(*s, generator=g, device=DEV).mul_(0.1).to(BF)
    inputs["hyper"] = torch.tensor([[1e-3, 0.1], [3e-4, 0.01]], device=DEV)
    k = len(G_SHAPES)

    @SC.guardfn
    def fn(guard, **t):
        T = guard.torch
        gg, gw = [], []
        for i in range(k):
            for dst, src in ((gg, t[f"g{i}"]), (gw, t[f"w{i}"])):
                n = src.numel()
                buf = T.empty((n + 1,) if i == k - 1 else (n,), dtype=BF, device=DEV)
                buf = buf[1:] if i == k - 1 else buf
                buf.copy_(src.reshape(-1))
                dst.append(buf)
        assert gg[-1].data_ptr() % 16 == 2 and gw[-1].data_ptr() % 16 == 2
        begin, total = [], 0
        for w in gw:
            begin.append(total)
            total += (w.numel() + 7) // 8 * 8
        hyper = T.empty((2, 2), dtype=torch.float32, device=DEV)
        hyper.copy_(t["hyper"])
        plan = ops.LiveAdamwPlan(gw, begin, [0, 1, 1, 0])
        partials = T.empty((plan.npartials,), dtype=torch.float32, device=DEV)
        out = T.empty((4,), dtype=torch.float32, device=DEV)
        master, ema = (T.empty((total,), dtype=torch.float32, device=DEV) for _ in range(2))
        m1, m2 = (T.zeros((total,), dtype=torch.float32, device=DEV) for _ in range(2))
        step = T.zeros((1,), dtype=torch.float32, device=DEV)
        views = lambda flat: [flat[b:b + w.numel()] for b, w in zip(begin, gw)]
        for vm, ve, w in zip(views(master), views(ema), gw):
            vm.copy_(w)
            ve.copy_(w)
        with G.recorded(guard, _optim) as rec:
            ops.grad_clip_coef(plan, gg, partials, 0.5, out)
            kept, first = partials.clone(), out.clone()
            assert rec.cd360_grad_clip_f32(partials.data_ptr(), plan.npartials, 0.5, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
            assert torch.equal(partials, kept) and torch.equal(out, first)  # the clip kernel reads the partials only
            for _ in range(2):
                ops.adamw_live_step(plan, gg, hyper, master, m1, m2, step, 0.9, 0.95, 1e-6, coef=out[2:3], ema=ema, ema_decay=0.5)
        assert plan.npartials == 2 and float(step) == 2
        assert all(torch.equal(a, t[f"g{i}"].reshape(-1)) for i, a in enumerate(gg)) and torch.equal(hyper, t["hyper"])
        assert torch.equal(partials, kept) and torch.equal(out, first)  # ... and the update neither
        return dict(partials=partials, out=out, step=step, params=gw, master=views(master), m1=views(m1), m2=views(m2), ema=views(ema))

    res, _ = G.run_twice(fn, inputs, declares=declares)
    assert 0 < float(res["out"][2]) < 1 and all(not torch.equal(w, inputs[f"w{i}"].reshape(-1)) for i, w in enumerate(res["params"]))


def test_every_optim_entry_point_has_a_guarded_case():
    """Runs without a GPU: every `int cd360_...(` include/optim/cd360_optim.h declares is in a guarded case's `declares` above, and is typed
    in OPTIM_SIGNATURES."""
    from cd360 import _optim
    untyped, unknown, uncovered = SC.check_guarded_cover(OC.HEADER, _optim.OPTIM_SIGNATURES, GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"
