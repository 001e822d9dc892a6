"""The two ends of a training step on the GPU: the four kernels of include/train/cd360_train.h against the float64 restatement of
tests/train_cases.py, per element; their memory safety under tests/guarded.py; the step counter; NoiseStage inside an eager and a captured
fine-tuning step.  Bars: integers exactly; the scalars derived from a table's sigma at 2 ulp; everything that carries Philox / Box-Muller
noise at 4 x the distance between the fp32 and the fp64 host restatement on the same inputs (the way tests/test_euler_a_gpu.py sizes the
bar of cd360_sampler_noise_f32), measured per case and printed beside the measurement."""
import functools

import numpy as np
import pytest
import torch

import guarded as G
import philox_ref as PR
import sampler_cases as SC
import train_cases as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SEEDS = (0, 30, 2 ** 63 + 12345)
STEPS = (0, 1, 2 ** 31 - 1)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _inputs(B, n, H, Wd, seed):
    g = np.random.default_rng(seed)
    x0 = g.standard_normal((B, 4, H, Wd)).astype(np.float32)
    xr = g.standard_normal((B, n, 4, H, Wd)).astype(np.float32) if n else None
    drop = np.asarray([1.0, 0.0, 1.0][:B], np.float32) if B > 1 else None
    return x0, xr, drop


def _streams(B, kind):
    return {"null": None, "repeated": [7] * B, "distinct": [3 + 5 * b for b in range(B)]}[kind]


def _tables(cfg):
    return _t(cfg["table"]), _t(cfg["tgt_table"]), _t(cfg["ref_table"])


def _run_stage(cfg, seed, streams, step, x0, xr, drop, dtype, advance=False):
    """The two front launches through cd360.ops -> (rows, timesteps, ref_idx, step_used, x_t, x_in, xr_in, step)."""
    from cd360 import ops
    table, tgt, ref = _tables(cfg)
    B = x0.shape[0]
    step_t = SC.step_t(((step + 2 ** 31) % 2 ** 32) - 2 ** 31)
    seed_t, streams_t = SC.seed_t(seed), SC.streams_t(streams)
    rows, ts, ri, used = ops.train_sigmas(table, tgt, cfg["tgt_kind"], cfg["tgt_start"], ref, cfg["ref_kind"], cfg["ref_start"], seed_t, streams_t, step_t,
                                          B, advance=advance)
    x_t, x_in, xr_in = ops.train_noise(_t(x0), None if xr is None else _t(xr), None if drop is None else _t(drop), rows, seed_t, streams_t, used,
                                       cfg["level"], dtype=dtype)
    return rows, ts, ri, used, x_t, x_in, xr_in, step_t


CASES = [(B, n, H, Wd) for B in (1, 3) for n in (0, 1, 2) for H, Wd in ((8, 8), (6, 10))] + [(3, 2, 5, 7), (2, 1, 128, 128)]


# ================================================================================================ 5: the front kernels, per element
@pytest.mark.parametrize("B,n,H,Wd", CASES, ids=[f"B{B}-n{n}-{H}x{Wd}" for B, n, H, Wd in CASES])
def test_stage_kernels_equal_the_float64_restatement(B, n, H, Wd):
    """cd360_train_sigmas_f32 + cd360_train_noise_f32 against tests/train_cases.py in float64.  Shapes: one and several rows, no / one / two
    reference views, 8 x 8 (H W % 8 == 0: bf16 planes written eight pixels at a time), 6 x 10 (15 vector units of four pixels, a ragged last
    workgroup; bf16 in 8-byte pieces), 5 x 7 (H W % 4 != 0: the scalar form of the loop, a ragged
    last unit) and one 128 x 128; seeds, steps (2^31 - 1 included) and stream layouts rotate over the cases so that every value meets
    every path; offset_noise_level 0.1 and 0; a dropped row where B = 3; a DiscreteSampling target sampler with num_idx_start in one case.
    timesteps, sigmas_ref_idx, step_used: exact.  sigma, w, c_skip, c_out, c_in, sigma_ref, c_in_ref: 2 ulp of the float64 value rounded
    to fp32.  off_tgt, off_ref, x_t, x_in, input_ref carry noise: 4 x max |fp32 restatement - fp64| of that output.  The bf16 outputs are
    the fp32 outputs' .to(bfloat16), bit for bit."""
    i = CASES.index((B, n, H, Wd))
    x0, xr, drop = _inputs(B, n, H, Wd, seed=100 + i)
    worst = {}
    for j, level in enumerate((0.1, 0.0)):
        seed, step = SEEDS[(i + j) % 3], STEPS[(i // 3 + j) % 3]
        streams = _streams(B, ("null", "repeated", "distinct")[(i + 2 * j) % 3])
        cfg = TR.shipped(level)
        if (B, n, H, Wd) == (3, 1, 6, 10):  # a discrete target sampler that starts inside its table, a cubic reference sampler
            cfg.update(tgt_kind=TR.DISCRETE, tgt_start=400, ref_kind=TR.CUBIC)
        kw = dict(seed=seed, streams=streams, step=step, x0=x0, xr=xr, drop=drop, **cfg)
        r64, r32 = TR.restate(np.float64, **kw), TR.restate(np.float32, **kw)
        rows, ts, ri, used, x_t, x_in, xr_in, _ = _run_stage(cfg, seed, streams, step, x0, xr, drop, torch.float32)
        assert ts.dtype == torch.int64 and ri.dtype == torch.int64 and used.dtype == torch.int32
        assert np.array_equal(ts.cpu().numpy(), r64["timesteps"]) and np.array_equal(ri.cpu().numpy(), r64["sigmas_ref_idx"])
        assert int(used.item()) & PR.MASK == step
        rows = rows.cpu().numpy()
        det = [TR.SIGMA, TR.W, TR.C_SKIP, TR.C_OUT, TR.C_IN, TR.SIGMA_REF, TR.C_IN_REF]
        u = TR.ulps(rows[:, det], r64["rows"][:, det].astype(np.float32))
        assert u <= 2, u
        assert not rows[:, 9:].any() and np.array_equal(rows[:, TR.SIGMA], r32["rows"][:, TR.SIGMA])
        got = {"off": rows[:, [TR.OFF_TGT, TR.OFF_REF]], "x_t": x_t.cpu().numpy(), "x_in": x_in.cpu().numpy()}
        want = {"off": ("rows", [TR.OFF_TGT, TR.OFF_REF]), "x_t": ("x_t", None), "x_in": ("x_in", None)}
        if n:
            got["input_ref"], want["input_ref"] = xr_in.cpu().numpy(), ("xr_in", None)
        else:
            assert xr_in is None
        for name, (key, cols) in want.items():
            a64, a32 = (r[key] if cols is None else r[key][:, cols] for r in (r64, r32))
            bar = 4 * float(np.abs(a32.astype(np.float64) - a64).max())
            err = float(np.abs(got[name].astype(np.float64) - a64).max())
            print(f"B{B} n{n} {H}x{Wd} level {level} seed {seed} step {step} streams {streams}: {name} max |kernel - float64| {err:.3e} | bar {bar:.3e} | scalars {u} ulp")
            worst[name] = max(worst.get(name, 0.0), err / bar)
            assert err <= bar, (name, err, bar)
        b16 = _run_stage(cfg, seed, streams, step, x0, xr, drop, BF)
        assert b16[5].dtype == BF and torch.equal(b16[5], x_in.to(BF)) and torch.equal(b16[4], x_t)
        assert (b16[6] is None) if not n else (b16[6].dtype == BF and torch.equal(b16[6], xr_in.to(BF)))
    print(f"B{B} n{n} {H}x{Wd}: worst error / bar {worst}")


def test_rows_of_one_stream_share_their_noise_and_the_domains_are_unrelated():
    """Zero latents, offset level 0: x_t = z sigma and input_ref = (z_a sigma_ref + z_b sigma_ref) c_in_ref are the noise itself.  Rows with
    equal stream ids hold equal bits, a row with another id does not, and a row's values do not depend on the batch around it.  The noise of
    domain 5 (from x_t) and the sum of domains 6 and 7 (from input_ref) are uncorrelated, and so are domains 5, 6 and 7 pairwise in the
    restatement the kernel has just been compared with element by element: |corr| <= 5 standard errors = 5 / sqrt(N)."""
    B, n, H, Wd = 3, 2, 32, 32
    cfg = TR.shipped(0.0)
    x0, xr = np.zeros((B, 4, H, Wd), np.float32), np.zeros((B, n, 4, H, Wd), np.float32)
    rows, ts, ri, _, x_t, _, xr_in, _ = _run_stage(cfg, 30, [5, 5, 9], 2, x0, xr, None, torch.float32)
    assert torch.equal(x_t[0], x_t[1]) and torch.equal(xr_in[0], xr_in[1]) and torch.equal(rows[0], rows[1]) and ts[0] == ts[1] and ri[0] == ri[1]
    assert not torch.equal(x_t[0], x_t[2]) and not torch.equal(xr_in[0], xr_in[2])
    alone = _run_stage(cfg, 30, [9], 2, x0[:1], xr[:1], None, torch.float32)
    assert torch.equal(alone[4][0], x_t[2]) and torch.equal(alone[6][0], xr_in[2]) and torch.equal(alone[0][0], rows[2])
    assert not torch.equal(xr_in[0, 0], xr_in[0, 1])  # the views of a sample draw at different pixel words
    r = TR.restate(np.float64, seed=30, streams=[5, 5, 9], step=2, x0=x0, xr=xr, **cfg)
    z5 = (x_t[2] / rows[2, TR.SIGMA]).cpu().numpy()
    zab = (xr_in[2, 0] / (rows[2, TR.C_IN_REF] * rows[2, TR.SIGMA_REF])).cpu().numpy()
    pairs = {"kernel 5 / 6+7": (z5, zab), "5 / 6": (r["z"][2], r["z_a"][2, 0]), "5 / 7": (r["z"][2], r["z_b"][2, 0]), "6 / 7": (r["z_a"][2], r["z_b"][2])}
    for what, (a, b) in pairs.items():
        c, se = abs(PR.corr(a, b)), 1.0 / np.sqrt(np.asarray(a).size)
        print(f"domains {what}: |corr| {c:.3e} = {c / se:.2f} standard errors")
        assert c <= 5 * se, (what, c)
    m = PR.moments(z5)
    assert m[0] <= 5 / np.sqrt(z5.size) and m[1] <= 5 * np.sqrt(2 / z5.size)


# ================================================================================================ 6: the l2 term and its gradient
def _eps_layout(eps32, layout):
    e = _t(eps32)
    if layout == "bf16-channels-last":
        return e.to(BF).contiguous(memory_format=torch.channels_last)
    if layout == "fp32-nchw":
        return e
    if layout == "fp32-channels-last":
        return e.contiguous(memory_format=torch.channels_last)
    if layout == "bf16-nchw":
        return e.to(BF)
    assert layout == "bf16-strided"  # a window of a wider, taller buffer: no dense layout
    B, C, H, Wd = e.shape
    buf = torch.zeros(B, C + 1, H + 2, Wd + 3, dtype=BF, device=DEV)
    buf[:, :C, 1:H + 1, 2:Wd + 2] = e.to(BF)
    return buf[:, :C, 1:H + 1, 2:Wd + 2]


L2_CASES = [("bf16-channels-last", "mask", 8, 8), ("bf16-channels-last", "none", 6, 10), ("bf16-channels-last", "zero-row", 32, 32),
            ("fp32-nchw", "mask", 6, 10), ("fp32-nchw", "none", 8, 8), ("fp32-channels-last", "zero-row", 8, 8), ("bf16-nchw", "mask", 8, 8),
            ("bf16-strided", "mask", 8, 8), ("bf16-channels-last", "mask", 5, 7), ("fp32-nchw", "none", 5, 7), ("bf16-channels-last", "mask", 128, 128)]


@pytest.mark.parametrize("layout,masking,H,Wd", L2_CASES, ids=["-".join(map(str, c)) for c in L2_CASES])
def test_l2_forward_and_backward_equal_the_float64_restatement(layout, masking, H, Wd):
    """cd360_train_l2_f32 / cd360_train_l2_bwd_f32 against the float64 restatement and its analytic gradient: with a mask, without one, with
    an all-zero mask row (loss 0, gradient an exact 0); eps in bf16 channels-last (what the UNet returns), fp32 NCHW, fp32 channels-last,
    bf16 NCHW and a strided bf16 window; H W % 4 != 0 (the scalar form); g with a zero entry (an exact zero row).  Bar: 4 x the largest
    |fp32 host restatement - fp64| over the case, for the loss and for the gradient; a bf16 gradient adds bf16's half ulp, at most 2^-8 |value|.
    Two runs are bit-identical; autograd through ops.train_l2 returns the same bits as the backward entry point."""
    from cd360 import ops
    B = 3
    i = L2_CASES.index((layout, masking, H, Wd))
    g = np.random.default_rng(200 + i)
    x0 = g.standard_normal((B, 4, H, Wd)).astype(np.float32)
    eps32 = g.standard_normal((B, 4, H, Wd)).astype(np.float32)
    mask = None
    if masking != "none":
        mask = (g.random((B, 1, H, Wd)) > 0.3).astype(np.float32)
        if masking == "zero-row":
            mask[1] = 0.0
    gr = np.asarray([0.7, 1.3, 0.0], np.float32)
    eps = _eps_layout(eps32, layout)
    cfg = TR.shipped(0.1)
    kw = dict(seed=30, streams=[0, 1, 2], step=4, x0=x0, eps=eps.float().cpu().numpy(), mask=mask, g=gr, **cfg)
    r64, r32 = TR.restate(np.float64, **kw), TR.restate(np.float32, **kw)
    rows, _, _, _, x_t, _, _, _ = _run_stage(cfg, 30, [0, 1, 2], 4, x0, None, None, torch.float32)
    x0_t, mask_t, g_t = _t(x0), None if mask is None else _t(mask), _t(gr)
    loss, den = ops._train_l2_fwd(eps, x_t, x0_t, rows, mask_t)
    d_eps = ops.train_l2_bwd(eps, x_t, x0_t, rows, mask_t, den, g_t)
    assert loss.shape == (B,) and loss.dtype == torch.float32 and d_eps.dtype == eps.dtype and d_eps.shape == eps.shape
    if layout != "bf16-strided":
        assert d_eps.stride() == eps.stride()
    # x_t itself differs from the restatement's by the noise kernel's error: the restatement is evaluated on the kernel's x_t
    def on_kernel_xt(dtype):
        dt = np.dtype(dtype).type
        rr = r64 if dtype is np.float64 else r32
        xt, e, rw = x_t.cpu().numpy().astype(dt), eps.float().cpu().numpy().astype(dt), rows.cpu().numpy().astype(dt)
        bc = lambda v: v.reshape(B, 1, 1, 1)
        err = (e * bc(rw[:, TR.C_OUT]) + xt * bc(rw[:, TR.C_SKIP])) - x0.astype(dt)
        t = bc(rw[:, TR.W]) * (err * err)
        m = None if mask is None else mask.astype(dt)
        t = t if m is None else t * m
        d = ((dt(2.0) * bc(rw[:, TR.W])) * err) * bc(rw[:, TR.C_OUT])
        d = d if m is None else d * m
        d = d / bc(rr["den"].astype(dt))
        gb = bc(gr.astype(dt))
        return t.reshape(B, -1).sum(1, dtype=dt) / rr["den"].astype(dt), np.where(gb == 0, dt(0.0), gb * d)

    (l64, d64), (l32, d32) = on_kernel_xt(np.float64), on_kernel_xt(np.float32)
    assert TR.ulps(den.cpu().numpy(), r64["den"].astype(np.float32)) <= 2
    bar_l = 4 * float(np.abs(l32.astype(np.float64) - l64).max())
    err_l = float(np.abs(loss.cpu().numpy().astype(np.float64) - l64).max())
    bar_d = 4 * float(np.abs(d32.astype(np.float64) - d64).max())
    got_d = d_eps.float().cpu().numpy().astype(np.float64)
    slack = np.abs(d64) * 2.0 ** -8 if eps.dtype == BF else 0.0  # 8 significand bits: half an ulp of v in [2^e, 2^(e+1)) is 2^(e-8) <= 2^-8 |v|
    err_d = float((np.abs(got_d - d64) - slack).max())
    print(f"l2 {layout} {masking} {H}x{Wd}: loss max |kernel - float64| {err_l:.3e} | bar {bar_l:.3e};  d_eps (beyond bf16's half ulp) {err_d:.3e} | bar {bar_d:.3e}")
    assert err_l <= bar_l and err_d <= bar_d
    assert not got_d[2].any()  # g[2] == 0
    if masking == "zero-row":
        assert float(loss[1]) == 0.0 and not got_d[1].any()
    assert bool((got_d[0] != 0).any())
    # bit-reproducible, and the same through autograd
    again = ops._train_l2_fwd(eps, x_t, x0_t, rows, mask_t)
    assert torch.equal(again[0], loss) and torch.equal(again[1], den) and torch.equal(ops.train_l2_bwd(eps, x_t, x0_t, rows, mask_t, den, g_t), d_eps)
    leaf = eps.detach().clone().requires_grad_(True) if layout != "bf16-strided" else None
    if leaf is not None:
        assert leaf.stride() == eps.stride()
        out = ops.train_l2(leaf, x_t, x0_t, rows, mask_t)
        assert torch.equal(out.detach(), loss)
        (out * g_t).sum().backward()
        assert torch.equal(leaf.grad, d_eps)
    assert torch.equal(ops.train_l2(eps, x_t, x0_t, rows, mask_t), loss)


# ================================================================================================ 7: memory safety
def _guarded_case(case):
    from cd360 import _train, ops
    cfg = TR.shipped(0.1)
    tabs = dict(zip(("table", "tgt", "ref"), _tables(cfg)))
    if case == "sigmas":
        inputs = dict(tabs, seed=SC.seed_t(30), streams=SC.streams_t([4, 4, 9]), step=SC.step_t(2 ** 31 - 1))

        @SC.guardfn
        def fn(guard, table, tgt, ref, seed, streams, step):
            with G.recorded(guard, _train):
                a = ops.train_sigmas(table, tgt, TR.CUBIC, 0, ref, TR.DISCRETE, 0, seed, streams, step, 3, advance=True)
                b = ops.train_sigmas(table, ref, TR.DISCRETE, 7, tgt, TR.CUBIC, 0, seed, None, step, 1, advance=False)
            return dict(a=a, b=b)
        return fn, inputs, ("step",)
    if case == "noise-both-dtypes":
        x0a, xra, _ = _inputs(3, 2, 6, 10, seed=301)
        x0b, xrb, _ = _inputs(3, 2, 5, 7, seed=302)
        x0c, xrc, _ = _inputs(3, 2, 8, 8, seed=304)  # H W % 8 == 0: the bf16 planes are written eight pixels at a time
        inputs = dict(tabs, seed=SC.seed_t(2 ** 63 + 12345), streams=SC.streams_t([1, 2, 3]), step=SC.step_t(6), x0a=_t(x0a), xra=_t(xra), x0b=_t(x0b), xrb=_t(xrb), x0c=_t(x0c), xrc=_t(xrc),
                      drop=_t(np.asarray([1.0, 0.0, 1.0], np.float32)))

        @SC.guardfn
        def fn(guard, table, tgt, ref, seed, streams, step, x0a, xra, x0b, xrb, x0c, xrc, drop):
            with G.recorded(guard, _train):
                rows, _, _, used = ops.train_sigmas(table, tgt, TR.CUBIC, 0, ref, TR.DISCRETE, 0, seed, streams, step, 3)
                outs = [ops.train_noise(x0, xr, d, rows, seed, streams, used, 0.1, dtype=dt)
                        for x0, xr in ((x0a, xra), (x0b, xrb), (x0c, xrc), (x0a, None)) for d in (drop, None) for dt in (torch.float32, BF)]
            return dict(rows=rows, outs=[[t for t in o if t is not None] for o in outs])
        return fn, inputs, ()
    assert case == "l2-forward-backward"
    g = np.random.default_rng(303)
    inputs = dict(rows=_t(TR.restate(np.float32, seed=1, streams=None, step=0, x0=np.zeros((3, 4, 2, 2), np.float32), **cfg)["rows"]),
                  g=_t(np.asarray([1.0, 0.0, 0.5], np.float32)))
    for tag, (H, Wd) in (("a", (6, 10)), ("b", (5, 7))):
        e = g.standard_normal((3, 4, H, Wd)).astype(np.float32)
        inputs.update({f"cl{tag}": _eps_layout(e, "bf16-channels-last"), f"pl{tag}": _eps_layout(e, "fp32-nchw"), f"st{tag}": _eps_layout(e, "bf16-strided"),
                       f"xt{tag}": _t(g.standard_normal(e.shape).astype(np.float32)), f"x0{tag}": _t(g.standard_normal(e.shape).astype(np.float32)),
                       f"m{tag}": _t((g.random((3, 1, H, Wd)) > 0.3).astype(np.float32))})

    @SC.guardfn
    def fn(guard, rows, g, **kw):
        outs = []
        with G.recorded(guard, _train):
            for tag in ("a", "b"):
                for eps in (kw["cl" + tag], kw["pl" + tag], kw["st" + tag]):
                    for m in (kw["m" + tag], None):
                        loss, den = ops._train_l2_fwd(eps, kw["xt" + tag], kw["x0" + tag], rows, m)
                        outs.append((loss, den, ops.train_l2_bwd(eps, kw["xt" + tag], kw["x0" + tag], rows, m, den, g)))
        return dict(outs=outs)
    return fn, inputs, ()


@pytest.mark.parametrize("case,declares", TR.GUARDED, ids=[c[0] for c in TR.GUARDED])
def test_train_entry_points_write_their_outputs_only(case, declares):
    """Every entry point under tests/guarded.py, both poison patterns: every output is an arena block between canaries, so no guard byte
    changes; the results are finite and bit-equal between the poisons (all twelve values of a scalar row are written); the operands are
    unchanged -- `step` excepted, which the header documents as in/out under advance (compared between the runs instead)."""
    fn, inputs, inout = _guarded_case(case)
    G.run_twice(fn, inputs, declares=declares, inout=inout)


# ================================================================================================ 8: the step counter
def _stage(seed=360, streams=None, level=0.1, dtype=BF):
    from cd360 import finetune, sampler as S
    from make_golden_params import LOSS_CFG
    from sgm.util import instantiate_from_config
    loss_fn = instantiate_from_config({"target": "sgm.modules.diffusionmodules.loss.StandardDiffusionLossImgRef",
                                       "params": dict(LOSS_CFG, offset_noise_level=level)})
    den = S.DiscreteDenoiser().to(DEV)
    return finetune.NoiseStage(den, loss_fn, seed, streams=streams, dtype=dtype), loss_fn


def _snapshot(st):
    return {k: getattr(st, k).clone() for k in ("x_t", "x_in", "timesteps", "input_ref", "sigmas_ref", "scalars", "step_used")}


@pytest.mark.parametrize("k", [5, 2 ** 31 - 2])
def test_advance_walks_the_step_counter_on_the_device(k):
    """With advance on, three calls draw at steps k, k + 1, k + 2 and leave the counter at k + 3 (as a 32-bit word: 2^31 - 2 walks through
    the sign); set_step(j) followed by a call reproduces call j bit for bit, on another stage as well; without advance the counter
    stays; reseed and set_streams reach the next call; the buffers are the same memory on every call."""
    from cd360 import ops
    x0, xr, drop = (_t(a) for a in _inputs(3, 2, 6, 10, seed=400))
    stage, _ = _stage(streams=[0, 1, 2])
    stage.set_step(k)
    shots, ptrs = [], set()
    for j in range(3):
        st = stage(x0, xr, drop)
        assert int(st.step_used.item()) & PR.MASK == (k + j) & PR.MASK
        shots.append(_snapshot(st))
        ptrs.add((st.x_t.data_ptr(), st.x_in.data_ptr(), st.input_ref.data_ptr(), st.scalars.data_ptr(), st.timesteps.data_ptr()))
    assert int(stage.step.item()) & PR.MASK == (k + 3) & PR.MASK and len(ptrs) == 1
    assert not torch.equal(shots[0]["x_in"], shots[1]["x_in"]) and not torch.equal(shots[1]["input_ref"], shots[2]["input_ref"])
    r = TR.restate(np.float64, seed=360, streams=[0, 1, 2], step=(k + 1) & PR.MASK, x0=x0.cpu().numpy(), **TR.shipped(0.1))
    assert np.array_equal(shots[1]["timesteps"].cpu().numpy(), r["timesteps"]) and np.array_equal(shots[1]["sigmas_ref"].cpu().numpy(), r["sigmas_ref_idx"])
    other, _ = _stage(streams=[0, 1, 2])
    for s in (stage, other):
        s.set_step(k + 1)
        again = _snapshot(s(x0, xr, drop, advance=False))
        assert all(torch.equal(again[name], shots[1][name]) for name in again), [name for name in again if not torch.equal(again[name], shots[1][name])]
        assert int(s.step.item()) & PR.MASK == (k + 1) & PR.MASK
    other.reseed(361)
    moved = _snapshot(other(x0, xr, drop, advance=False))
    assert not torch.equal(moved["x_in"], shots[1]["x_in"])
    other.reseed(360)
    other.set_streams([0, 1, 7])
    moved = _snapshot(other(x0, xr, drop, advance=False))
    assert torch.equal(moved["x_in"][:2], shots[1]["x_in"][:2]) and not torch.equal(moved["x_in"][2], shots[1]["x_in"][2])
    with pytest.raises(ValueError):
        other.set_streams([0, 1])
    with pytest.raises(ops.Cd360Error):
        other(x0.cpu(), xr, drop)
    with pytest.raises(ops.Cd360Error):
        other.l2(shots[0]["x_in"].cpu(), x0, None)


# ================================================================================================ 9, 10: the stage in a training step
@functools.lru_cache(maxsize=1)
def _train_setup():
    import copy
    from cd360 import finetune, synth
    from test_modules_gpu import _sdxl_net
    net, g = _sdxl_net(seed=43)
    net.eval()
    names = finetune.select_trainable(net, "pose")
    b, n, L = 2, 2, 32
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    batch = dict(x0=rn(b, 4, L, L), x_ref=rn(b, n, 4, L, L), context=rn(b + b * n, 77, 2048), y=rn(b + b * n, 2816), pose=synth.pose_batch(b, n, seed=3),
                 target_rgb=rn(b, 3, 8 * L, 8 * L).clamp(-1, 1), mask=torch.ones(b, 1, L, L, device=DEV), opacity=torch.sigmoid(3 * rn(b, 1, 8 * L, 8 * L)))
    start = copy.deepcopy({k: v for k, v in net.state_dict().items() if "pose" in k})
    return net, names, batch, start


def _fresh(net, start):
    from cd360 import finetune
    net.load_state_dict(start, strict=False)
    return finetune.MasterAdamW(finetune.optimizer_param_groups(net, "pose", lr=1e-4), lr=1e-4)


def test_stage_in_a_captured_training_step_follows_the_eager_steps():
    """The net and shapes of test_config4_train_step_replayed_from_a_hipgraph_follows_the_eager_steps (b = 2, n = 2, L = 32, eval-mode
    raymarchers) from CLEAN latents.  Six eager train_step_latents, then GraphedTrainStep(stage=...) with two warm-up steps and four
    replays: after every replay the stage's x_in, input_ref and timesteps are bit-equal to an eager call of another stage at the same
    step; the losses follow the eager ones to 1e-4 relative and the trained weights to 2e-2 (that test's bars); successive steps differ.
    The old path fed what the stage made -- noised = x_in, target = the noise -(x_t - x0) / c_out, w = 1, mask of ones -- gives the latent
    step's total loss to 1e-4 relative: with eps-scaling w (D - x0)^2 = (eps - noise)^2."""
    from cd360 import finetune
    net, names, batch, start = _train_setup()
    stage, loss_fn = _stage(seed=77, streams=[0, 1])
    probe, _ = _stage(seed=77, streams=[0, 1])
    opt = _fresh(net, start)
    eager = [float(finetune.train_step_latents(net, loss_fn, opt, stage, **batch)[0]) for _ in range(6)]
    assert int(stage.step.item()) == 6
    w_eager = {k: dict(net.named_parameters())[k].detach().clone() for k in names}
    opt = _fresh(net, start)
    stage.set_step(0)
    step = finetune.GraphedTrainStep(net, loss_fn, opt, batch, warmup=2, stage=stage)
    assert int(stage.step.item()) == 2
    graphed = []
    for k in range(2, 6):
        graphed.append(float(step()[0]))
        probe.set_step(k)
        want = probe(batch["x0"], batch["x_ref"], None)
        got = stage._last
        assert int(stage.step.item()) == k + 1 and int(got.step_used.item()) == k
        assert torch.equal(got.x_in, want.x_in) and torch.equal(got.input_ref, want.input_ref) and torch.equal(got.timesteps, want.timesteps)
        assert got.x_in.dtype == BF == net.dtype
    print("eager:", [round(v, 5) for v in eager], "graph (steps 3-6):", [round(v, 5) for v in graphed])
    assert all(abs(a - e) <= 1e-4 * abs(e) for a, e in zip(graphed, eager[2:]))
    assert all(abs(a - b) > 1e-6 * abs(a) for a, b in zip(eager, eager[1:]))
    params = dict(net.named_parameters())
    worst = max(float((params[k].detach().float() - w_eager[k].float()).abs().max() / w_eager[k].float().abs().max().clamp_min(1e-6)) for k in names)
    assert worst < 2e-2, worst
    # warmup_restore puts the counter back
    opt = _fresh(net, start)
    stage.set_step(11)
    finetune.GraphedTrainStep(net, loss_fn, opt, batch, warmup=1, warmup_restore=True, stage=stage)
    assert int(stage.step.item()) == 11
    # the old path on what the stage made
    opt = _fresh(net, start)
    stage.set_step(0)
    st = stage(batch["x0"], batch["x_ref"], None, advance=False)
    rows = st.scalars
    target = -(st.x_t - batch["x0"]) / rows[:, TR.C_OUT].view(-1, 1, 1, 1)
    old = dict(noised=st.x_in.float(), timesteps=st.timesteps.clone(), input_ref=st.input_ref.float(), sigmas_ref=st.sigmas_ref.clone(), target=target,
               w=torch.ones(2, 1, 1, 1, device=DEV), **{k: batch[k] for k in ("context", "y", "pose", "target_rgb", "mask", "opacity")})
    t_old = float(finetune.train_step(net, loss_fn, opt, **old)[0])
    opt = _fresh(net, start)
    t_new = float(finetune.train_step_latents(net, loss_fn, opt, stage, **batch)[0])
    print(f"old path on the stage's tensors {t_old:.6f} | latent step {t_new:.6f}")
    assert abs(t_old - t_new) <= 1e-4 * abs(t_new) and abs(t_new - eager[0]) <= 1e-4 * abs(eager[0])


def test_a_graphed_step_without_a_stage_is_what_it_was():
    """GraphedTrainStep(stage=None): no entry point of libcd360_train.so is reached while it is built and replayed, it holds no stage, and
    the entry points of the main library it reaches are those an eager train_step reaches, in the same order and number: nothing was
    added to the library launches of a replay.  This is the second form of the check: it counts C-ABI calls, neither the nodes of the
    hipGraph nor the launches torch issues itself (torch exposes no node count of a captured graph)."""
    from cd360 import _lib, _train, finetune
    from make_golden_params import LOSS_CFG
    from sgm.util import instantiate_from_config
    net, names, batch, start = _train_setup()
    loss_fn = instantiate_from_config({"target": "sgm.modules.diffusionmodules.loss.StandardDiffusionLossImgRef", "params": LOSS_CFG})
    b, L = 2, 32
    g = torch.Generator(device=DEV).manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    old = dict(noised=rn(b, 4, L, L), timesteps=torch.full((b,), 500.0, device=DEV), input_ref=batch["x_ref"], sigmas_ref=torch.full((b,), 3.0, device=DEV),
               target=rn(b, 4, L, L), w=torch.full((b, 1, 1, 1), 0.7, device=DEV), **{k: batch[k] for k in ("context", "y", "pose", "target_rgb", "mask", "opacity")})
    calls = {"train": [], "main": []}
    rec_t, rec_m = G.Recorder(_train.load()), G.Recorder(_lib.load())
    saved = _train.load, _lib.load
    _train.load, _lib.load = (lambda: rec_t), (lambda check_symbols=True: rec_m)
    try:
        opt = _fresh(net, start)
        finetune.train_step(net, loss_fn, opt, **old)  # settles every cache
        del rec_m.called[:]
        finetune.train_step(net, loss_fn, opt, **old)
        eager_calls = list(rec_m.called)
        opt = _fresh(net, start)
        del rec_m.called[:]
        step = finetune.GraphedTrainStep(net, loss_fn, opt, old, warmup=1)
        graph_calls = list(rec_m.called)
        total = step()[0]
    finally:
        _train.load, _lib.load = saved
    assert step.stage is None and not rec_t.called and torch.isfinite(total)
    launching = lambda names_: [c for c in names_ if not c.endswith(("_bytes", "_rows", "_slabs", "_route", "_splits", "_tile_n", "_order", "_padded")) and "tuning" not in c
                                and "query" not in c]
    e, gcalls = launching(eager_calls), launching(graph_calls)
    print(f"entry points per eager step {len(e)}; warm-up + capture of a stage-less GraphedTrainStep {len(gcalls)}")
    assert e and len(e) > 1000, len(e)  # the recorder does see the step's calls
    assert len(gcalls) == 2 * len(e) and gcalls[len(e):] == e
