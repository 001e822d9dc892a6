"""The live optimiser step without a GPU: the third library's header <=> table <=> exports and its host-side refusals, the resource record
of its object, sgm/lr_scheduler.py against multipliers recorded from the reference's own classes, and LRSchedule / the torch fall-back of
MasterAdamW (clipping, EMA) against torch."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import optim_cases as OC
import sampler_cases as SC


# ================================================================================================ 1: header, table, library
def _arrays(k=2, numel=(16, 5), begin=(0, 16), row=(0, 1)):
    P = ctypes.c_void_p
    return dict(grads=(P * k)(*[0x100000 * (i + 1) for i in range(k)]), params=(P * k)(*[0x900000 + 0x100000 * i for i in range(k)]),
                begin=(ctypes.c_int64 * k)(*begin), numel=(ctypes.c_int64 * k)(*numel), row=(ctypes.c_int32 * k)(*row))


def test_optim_header_matches_its_table_and_the_older_libraries_are_closed():
    """include/optim/cd360_optim.h <=> cd360._optim.OPTIM_SIGNATURES <=> libcd360_optim.so (every `cd360_...(` word, comments included); no
    new name is in a table of cd360._lib.ABI, in EDIT_SIGNATURES, in a header of the first two libraries or exported by either; the
    binding reads no environment variable; the constants of the header are those cd360.ops computes slice lengths with."""
    from cd360 import _edit, _lib, _optim, ops
    mismatch, in_tables, in_headers, mistyped, lib = SC.check_library_matches_table(OC.LIBRARY)
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    assert "OPTIM_SIGNATURES" not in vars(_lib) and "OPTIM_SIGNATURES" not in vars(_edit)
    first, second = _lib.load(check_symbols=True), _edit.load()
    for name in OC.NEW:
        assert not hasattr(first, name) and not hasattr(second, name), name
    src = open(_optim.__file__).read()
    assert "os.environ" not in src and "getenv" not in src
    assert SC.header_constant(OC.HEADER, "CD360_OPTIM_SUMSQ_VECS") == ops.OPTIM_SUMSQ_VECS and SC.header_constant(OC.HEADER, "CD360_OPTIM_SUMSQ_TERMS") == ops.OPTIM_SUMSQ_TERMS
    assert ops.OPTIM_SUMSQ_VECS * 8 == 256 * ops.OPTIM_SUMSQ_TERMS  # 256 threads, each its share of the workgroup's vectors
    assert SC.header_constant(OC.HEADER, "CD360_OPTIM_SUMSQ_DEPTH") == ops.OPTIM_SUMSQ_DEPTH and 2 ** ops.OPTIM_SUMSQ_DEPTH == ops.OPTIM_SUMSQ_TERMS
    assert ops.sumsq_partials([1]) == 1 and ops.sumsq_partials([8 * 2048]) == 1 and ops.sumsq_partials([8 * 2048 + 1]) == 2
    assert ops.sumsq_partials([8 * 2047, 1, 1]) == 2  # vectors, not values: every tensor's tail is a vector of its own


def test_optim_entry_points_refuse_bad_arguments_on_the_host():
    """Fabricated non-null pointers: every call below returns CD360_ERR_ARG (-1) or CD360_ERR_SHAPE (-2) before anything launches."""
    from cd360 import _optim
    lib = _optim.load()
    nul, P = ctypes.c_void_p(None), ctypes.c_void_p
    a = _arrays()
    part, out = P(0x2000000), P(0x3000000)
    # ---- cd360_grad_sumsq_bf16(n, grads, numel, partials, stream)
    sumsq = lib.cd360_grad_sumsq_bf16
    assert sumsq(2, nul, a["numel"], part, nul) == -1 and sumsq(2, a["grads"], nul, part, nul) == -1 and sumsq(2, a["grads"], a["numel"], nul, nul) == -1
    for n in (0, -1, 65):
        assert sumsq(n, a["grads"], a["numel"], part, nul) == -1, n
    assert sumsq(2, a["grads"], a["numel"], P(0x2000002), nul) == -1
    assert sumsq(2, (P * 2)(0x100000, None), a["numel"], part, nul) == -1
    assert sumsq(2, a["grads"], (ctypes.c_int64 * 2)(16, 0), part, nul) == -1
    assert sumsq(2, (P * 2)(0x100000, 0x200001), a["numel"], part, nul) == -2
    # ---- cd360_grad_clip_f32(partials, count, max_norm, out, stream)
    clip = lib.cd360_grad_clip_f32
    assert clip(nul, 4, 1.0, out, nul) == -1 and clip(part, 4, 1.0, nul, nul) == -1
    assert clip(part, 0, 1.0, out, nul) == -1 and clip(part, -3, 1.0, out, nul) == -1
    assert clip(part, 4, -1.0, out, nul) == -1 and clip(part, 4, float("nan"), out, nul) == -1
    assert clip(part, 4, 1.0, P(0x3000004), nul) == -1 and clip(P(0x2000002), 4, 1.0, out, nul) == -1
    assert clip(part, 8, 1.0, P(0x2000010), nul) == -1  # out inside the partials
    # ---- cd360_adamw_live_bf16(n, grads, params, begin, numel, row, hyper, hyper_rows, coef, master, exp_avg, exp_avg_sq, ema, ema_decay, step, b1, b2, eps, stream)
    live = lib.cd360_adamw_live_bf16
    hyper, coef, master, m1, m2, ema, step = P(0x4000000), P(0x4100008), P(0x5000000), P(0x6000000), P(0x7000000), P(0x8000000), P(0x4200000)

    def call(n=2, grads=a["grads"], params=a["params"], begin=a["begin"], numel=a["numel"], row=a["row"], hyper=hyper, rows=2, coef=coef, master=master,
             m1=m1, m2=m2, ema=ema, step=step):
        return live(n, grads, params, begin, numel, row, hyper, rows, coef, master, m1, m2, ema, 0.5, step, 0.9, 0.999, 1e-8, nul)

    for name in ("grads", "params", "begin", "numel", "row", "hyper", "master", "m1", "m2", "step"):  # coef and ema may be null
        assert call(**{name: nul}) == -1, name
    for n in (0, -2, 65):
        assert call(n=n) == -1, n
    for name in ("master", "m1", "m2", "ema"):
        assert call(**{name: P(0x5000008)}) == -1, name  # a flat buffer off its 16-byte boundary
    assert call(step=P(0x4200002)) == -1 and call(hyper=P(0x4000001)) == -1 and call(coef=P(0x4100002)) == -1
    assert call(rows=0) == -1
    assert call(row=(ctypes.c_int32 * 2)(0, -1)) == -1 and call(row=(ctypes.c_int32 * 2)(2, 0)) == -1  # a negative row; a row behind the table
    assert call(begin=(ctypes.c_int64 * 2)(0, -8)) == -1 and call(numel=(ctypes.c_int64 * 2)(16, 0)) == -1
    assert call(grads=(P * 2)(0x100000, None)) == -1 and call(params=(P * 2)(None, 0x900000)) == -1
    assert call(ema=master) == -1  # ema overlapping master
    assert call(ema=P(0x5000000 + 16 * 4)) == -1  # ... its second tensor (the tensors span 16 + 5 values)
    assert call(ema=m1) == -1 and call(ema=m2) == -1
    assert call(begin=(ctypes.c_int64 * 2)(0, 12)) == -2
    assert call(grads=(P * 2)(0x100001, 0x200000)) == -2 and call(params=(P * 2)(0x900000, 0xA00001)) == -2


# ================================================================================================ 2: resource record
def test_optim_kernels_are_recorded_without_scratch():
    """build() leaves the new object's resource record where test_no_kernel_keeps_a_stack_object_in_scratch_memory reads it: the three
    kernels (two of them index a by-value argument struct dynamically), no scratch, no spill."""
    rec = json.load(open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "lib", "obj", "optim_step.o.resources.json")))
    assert len(rec) == len(OC.KERNELS) and all(any(k in name for name in rec) for k in OC.KERNELS), sorted(rec)
    for name, r in rec.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


# ================================================================================================ 3: sgm/lr_scheduler.py
def test_lr_schedulers_equal_the_reference_multipliers():
    """tests/golden/lr_schedules.npz holds what the reference's own classes return (make_lr_schedule_golden.py) for n = 0 .. N: below the
    warm-up, past the end of the decay, on a cycle boundary and into the next cycle.  Exact float64 equality; resolvable as YAML targets."""
    import make_lr_schedule_golden as M
    from sgm import lr_scheduler as L
    from sgm.util import instantiate_from_config
    gold = np.load(os.path.join(SC.ROOT, "tests", "golden", "lr_schedules.npz"))
    assert sorted(gold.files) == sorted(f"{c}_{k}" for c, cfgs in M.CONFIGS.items() for k in range(len(cfgs)))
    for cls, cfgs in M.CONFIGS.items():
        for k, (cfg, last) in enumerate(zip(cfgs, M.N[cls])):
            want = gold[f"{cls}_{k}"]
            assert want.dtype == np.float64 and want.shape == (last + 1,)
            for sched in (getattr(L, cls)(**cfg), instantiate_from_config({"target": f"sgm.lr_scheduler.{cls}", "params": cfg})):
                got = np.asarray([float(sched.schedule(n)) for n in range(last + 1)], dtype=np.float64)
                assert np.array_equal(got, want), (cls, k, np.flatnonzero(got != want)[:4])
                assert float(sched(last)) == want[-1]  # __call__ is schedule
    with pytest.raises(ValueError):
        L.LambdaLinearScheduler(**M.CONFIGS["LambdaLinearScheduler"][1]).schedule(38)  # behind the last cycle
    with pytest.raises(ValueError):
        L.LambdaWarmUpCosineScheduler2(warm_up_steps=[1, 2], f_min=[0.0], f_max=[1.0], f_start=[0.0], cycle_lengths=[5])


# ================================================================================================ 4: LRSchedule and the torch fall-back
def _cpu_params(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in ((7, 5), (3,), (1,), (4, 6))], g


def _grads(g, ps, scale=1.0):
    return [torch.randn(p.shape, generator=g) * scale for p in ps]


def test_lrschedule_on_the_fallback_equals_torch_adamw_with_lambdalr():
    """finetune.LRSchedule on MasterAdamW(fused=False) over CPU fp32 parameters against torch.optim.AdamW + LambdaLR on the same gradients,
    6 steps, bit for bit, under a LambdaLinearScheduler with a warm-up and a decay to zero."""
    from cd360 import finetune
    from sgm.lr_scheduler import LambdaLinearScheduler
    base, g = _cpu_params()
    pa = [torch.nn.Parameter(b.clone()) for b in base]
    pb = [torch.nn.Parameter(b.clone()) for b in base]
    mk = lambda ps: [{"params": ps[:2], "lr": 1e-2, "weight_decay": 0.1}, {"params": ps[2:], "lr": 3e-3}]
    sched = lambda: LambdaLinearScheduler(warm_up_steps=[2], f_min=[0.0], f_max=[1.0], f_start=[0.25], cycle_lengths=[6])
    ours = finetune.MasterAdamW(mk(pa), lr=1e-3, fused=False, betas=(0.9, 0.95))
    assert not ours.fused and not ours.live
    ls = finetune.LRSchedule(ours, sched())
    ref = torch.optim.AdamW(mk(pb), lr=1e-3, betas=(0.9, 0.95))
    with pytest.raises(TypeError):
        torch.optim.lr_scheduler.LambdaLR(ours, sched().schedule)  # what LRSchedule is for
    lr = torch.optim.lr_scheduler.LambdaLR(ref, sched().schedule)
    assert ls.get_last_lr() == lr.get_last_lr() == [1e-2 * 0.25, 3e-3 * 0.25]
    seen = []
    for it in range(6):
        for a, b, gr in zip(pa, pb, _grads(g, pa)):
            a.grad, b.grad = gr.clone(), gr.clone()
        ours.step()
        ref.step()
        ls.step()
        lr.step()
        assert ls.get_last_lr() == lr.get_last_lr()
        seen.append(ls.get_last_lr()[0])
        for a, b in zip(pa, pb):
            assert torch.equal(a.detach(), b.detach()), it
    assert seen[0] > 1e-2 * 0.25 and seen[-1] == 0.0 and len(set(seen)) == 6  # the schedule moved in every step and ended at zero


def test_fallback_clipping_equals_clip_grad_norm_and_its_ema_the_formula():
    """MasterAdamW(fused=False, max_grad_norm=, ema_decay=) on CPU fp32 parameters: the step equals clip_grad_norm_ + torch.optim.AdamW bit
    for bit (a binding max_norm: the factor is below 1 in every step), grad_norm / clip_coef are clip_grad_norm_'s, and after every step
    the shadows equal optim_cases.ema_update applied to the previous shadows and the new masters -- (1 + t) / (10 + t) exceeds the cap 0.5 from
    t = 9, so 8 steps run below it and the ninth at it.  ema_scope swaps the shadows in and the masters back; a tensor without a gradient is skipped."""
    from cd360 import finetune
    base, g = _cpu_params(seed=5)
    pa = [torch.nn.Parameter(b.clone()) for b in base]
    pb = [torch.nn.Parameter(b.clone()) for b in base]
    ours = finetune.MasterAdamW(pa, lr=1e-2, fused=False, max_grad_norm=0.5, ema_decay=0.5, weight_decay=0.05)
    ref = torch.optim.AdamW(pb, lr=1e-2, weight_decay=0.05)
    assert all(torch.equal(e, p.detach()) and e.dtype == torch.float32 for e, p in zip(ours.ema, pa))
    for it in range(9):
        t = it + 1
        prev = [e.clone() for e in ours.ema]
        skip = 1 if it == 4 else None
        for i, (a, b, gr) in enumerate(zip(pa, pb, _grads(g, pa, scale=2.0))):
            a.grad, b.grad = (None, None) if i == skip else (gr.clone(), gr.clone())
        ours.step()
        norm = torch.nn.utils.clip_grad_norm_([b for b in pb if b.grad is not None], 0.5)
        ref.step()
        assert torch.equal(ours.grad_norm, norm) and float(norm) > 0.5
        assert torch.equal(ours.clip_coef, torch.clamp(0.5 / (norm + 1e-6), max=1.0)) and float(ours.clip_coef) < 1
        for i, (a, b, e, p) in enumerate(zip(pa, pb, ours.ema, prev)):
            assert torch.equal(a.detach(), b.detach()), (it, i)
            assert torch.equal(e, p if i == skip else OC.ema_update(p, a.detach(), t, 0.5)), (it, i)
        assert ((1 + t) / (10 + t) > 0.5) == (t >= 9)
    with ours.ema_scope():
        assert all(torch.equal(a.detach(), e) for a, e in zip(pa, ours.ema))
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(pa, pb))
    sd = ours.ema_state_dict(["w%d" % i for i in range(len(pa))])
    assert list(sd) == ["w0", "w1", "w2", "w3"] and all(torch.equal(sd["w%d" % i], e) and sd["w%d" % i] is not e for i, e in enumerate(ours.ema))
    plain = finetune.MasterAdamW(pa, lr=1e-2, fused=False)
    with pytest.raises(ValueError):
        plain.ema_scope().__enter__()
    with pytest.raises(ValueError):
        finetune.MasterAdamW(pa, lr=1e-2, fused=False, ema_decay=1.5)
    with pytest.raises(ValueError):
        finetune.MasterAdamW(pa, lr=1e-2, fused=False, max_grad_norm=-1.0)
    assert plain.sync_hyper() is False  # not live: nothing to refresh
