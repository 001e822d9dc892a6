"""The method of tests/attn_round_cases.py, checked without a GPU on every case the GPU file runs:

  * the roundings: rnd() against torch's own bf16 conversion, truncation and rounding away against their definitions, near_midpoint() on
    constructed values;
  * the constants: fp32 restatements of every pipeline, in two summation orders, against the float64 emulation.  The fp32 p (P, dS) stays
    within HALF of tau (E) of the float64 one on every (row, key) pair, so every rounding that can go the other way is flagged with a factor
    two to spare; what remains of |o32 - o64| after the flip allowance stays within HALF of EPS A; and the rounded fp32 result is inside
    the bar on every element.  (A flagged pair that does flip uses its whole allowance -- ulp |v| / l is exactly what it moves the output
    by -- so the half is asked of tau and of EPS, not of F.)
  * the caps: flagged pairs <= 1 % (P), <= 2 % (dS); rows of the lazy pipeline with a marginal move_ref decision <= 0.5 %;
  * lse of the routes that return it: the fp32 restatement within half of LSE_REL (|lse| + 1); l summed from the rounded P leaves it;
  * the bias statistic on the positive family: |T_rne| <= |T_trunc| / 20;
  * every fault model of faults_for() / bwd_faults_for() leaves the bar on >= 10 % of the elements of a tensor it touches, or (positive
    family) the bias bar |T| <= |T_trunc| / 4.
Each test prints its figures (ATTN-ROUND-CPU ...) before it asserts."""
import pytest
import torch

import attn_round_cases as RC

FORWARD = RC.all_forward_specs()
BACKWARD = RC.all_bwd_specs()


def test_roundings():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(20000, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-20, 20, (20000,), generator=g).double())
    x = x.float().double()   # (torch converts through fp32: start there, so that both round once)
    assert torch.equal(RC.rnd(x), x.bfloat16().double())
    t, a = RC.rnd(x, "trunc"), RC.rnd(x, "away")
    assert torch.equal(t.bfloat16().double(), t) and torch.equal(a.bfloat16().double(), a)
    assert bool((t.abs() <= x.abs()).all()) and bool((a.abs() >= x.abs()).all())
    _, u = RC.grid(x)
    assert bool(((a - t).abs() <= u).all()) and bool((((a - t).abs() == u) | (t == x)).all())
    # 1 + 2^-8 is the midpoint of 1 and 1 + 2^-7: ties go to even, and the flag answers to the distance asked
    one = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.5], dtype=torch.float64)
    assert RC.rnd(one).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 1.5]
    flag, ulp = RC.near_midpoint(one, torch.full_like(one, 2.0 ** -20))
    assert flag.tolist() == [True, True, True, False] and ulp.tolist() == [2.0 ** -7] * 4
    assert RC.near_midpoint(one, torch.full_like(one, 2.0 ** -21))[0].tolist() == [True, True, False, False]
    assert RC.C != 1.0 and abs(RC.C - 0.125 * 1.4426950408889634) < 1e-8


def test_q_direct_is_invisible():
    """Why q_direct is on no list: it changes q~ on a handful of elements."""
    case = RC.make_case(RC.lazy_spec("peaked"))
    n = int((RC.q_tilde(case.q, RC.C, "q_direct") != RC.q_tilde(case.q)).sum())
    print(f"ATTN-ROUND-CPU q_direct differs on {n} of {case.q.numel()} elements of q~")
    assert n <= case.q.numel() * 2.0 ** -12
    for f in ("q_unrounded", "q_bf16_mul"):
        assert float((RC.q_tilde(case.q, RC.C, f) != RC.q_tilde(case.q)).double().mean()) > 0.3


@pytest.mark.parametrize("pipeline,sp", FORWARD, ids=[f"{p}-{RC.spec_id(sp)}" for p, sp in FORWARD])
def test_forward_pipeline(pipeline, sp):
    case = RC.make_case(sp)
    ex = RC.exact(case)
    fn = RC.PIPELINES[pipeline]
    emu = fn(case)
    want, A = RC.flat(ex.out), RC.flat(ex.A)
    t_rne = RC.bias(emu.out(), want, A)
    t_trunc = RC.bias(fn(case, "p_trunc").out(), want, A)
    marginal = float(emu.marginal.any(-1).double().mean()) if pipeline == "lazy" else 0.0
    figs = []
    for order in (0, 1):
        e32 = fn(case, f32=True, order=order)
        assert e32.moves == emu.moves   # (lazy: the fp32 run takes the decisions of the float64 one; no row of these cases is marginal)
        tau_use = max(float(((a - b).abs() / (b * t).clamp_min(1e-300)).max()) for a, b, t in zip(e32.ps, emu.ps, emu.taus))
        eps_use = float((((e32.o - emu.o).abs() - emu.F) / (RC.EPS * ex.A)).max())
        worst = float(RC.forward_ratios(e32.out(), emu, ex.A).max())
        lse_use = 0.0 if pipeline == "single" else float(RC.lse_ratios(e32.lse.reshape(-1, sp.Nq), emu).max())
        figs.append((tau_use, eps_use, worst, lse_use))
    print(f"ATTN-ROUND-CPU {pipeline} {RC.spec_id(sp)} flagged={emu.flagged:.5f} marginal_rows={marginal:.5f} moves={emu.moves} "
          f"T_rne={t_rne:.2e} T_trunc={t_trunc:.2e} fp32 (tau use, eps use, worst err/bar, lse use) order 0: " + " ".join(f"{x:.3f}" for x in figs[0])
          + " order 1: " + " ".join(f"{x:.3f}" for x in figs[1]))
    assert emu.flagged <= RC.FLAG_CAP_P
    assert marginal <= RC.MARGINAL_CAP
    for tau_use, eps_use, worst, lse_use in figs:
        assert tau_use <= 0.5 and eps_use <= 0.5 and worst <= 1.0 and lse_use <= 0.5
    if sp.family == "positive":
        assert abs(t_trunc) > 5e-4 and abs(t_rne) <= abs(t_trunc) / 20
    for fault in RC.faults_for(pipeline, sp):
        fe = fn(case, fault)
        out = fe.out(fault)
        share = float((RC.forward_ratios(out, emu, ex.A) > 1).double().mean())
        t = RC.bias(out, want, A)
        biased = sp.family == "positive" and abs(t) > abs(t_trunc) / 4
        lse_share = 0.0 if pipeline == "single" else float((RC.lse_ratios(fe.lse.reshape(-1, sp.Nq), emu) > 1).double().mean())
        print(f"ATTN-ROUND-CPU   fault {fault}: outside the bar {share:.3f}, T={t:.2e}, lse rows outside {lse_share:.3f}")
        assert share >= 0.10 or biased or (fault == "l_bf16" and lse_share >= 0.10), fault


def test_lazy_case_moves_its_reference():
    """The peaked lazy case takes move_ref after tile 0 on some rows (alpha = exp2(-d), no power of two), the spread one on none; the
    pre-scaled entry sees the same fragments as the plain one."""
    peaked, spread = RC.emulate_lazy(RC.make_case(RC.lazy_spec("peaked"))), RC.emulate_lazy(RC.make_case(RC.lazy_spec("spread")))
    assert peaked.moves >= 8 and spread.moves == 0
    case = RC.make_case(RC.lazy_spec("peaked"))
    assert torch.equal(RC.emulate_lazy(case, prescaled=True).o, peaked.o)
    # an inverted decision changes the rows it marks and no other
    flip = torch.zeros_like(peaked.marginal)
    flip[0, 0, 5, 1] = True
    other = RC.emulate_lazy(case, flip=flip)
    diff = (other.o != peaked.o).any(-1)
    assert bool(diff[0, 0, 5]) and int(diff.sum()) == 1


@pytest.mark.parametrize("sp", BACKWARD, ids=[RC.spec_id(sp) for sp in BACKWARD])
def test_backward_pipeline(sp):
    case = RC.make_case(sp)
    g = RC.bwd_ref(case)
    emu = RC.emulate_bwd(case)
    want, A = RC.flat(g.dv), RC.flat(g.A_dv)
    t_rne = RC.bias(emu.outs()[2], want, A)
    t_trunc = RC.bias(RC.emulate_bwd(case, "p_trunc").outs()[2], want, A)
    figs = []
    for order in (0, 1):
        e32 = RC.emulate_bwd(case, f32=True, order=order)
        tau_use = float(((e32.P - emu.P).abs() / (emu.P * emu.tau_p)).max())
        e_use = float(((e32.dS - emu.dS).abs() / emu.err_ds).max())
        eps_use = max(float((((a - b).abs() - F) / (RC.EPS * Ax)).max()) for a, b, Ax, F in
                      ((e32.dq, emu.dq, g.A_dq, emu.F_dq), (e32.dk, emu.dk, g.A_dk, emu.F_dk), (e32.dv, emu.dv, g.A_dv, emu.F_dv)))
        worst = max(float(r.max()) for r in RC.bwd_ratios(e32.outs(), emu, g))
        figs.append((tau_use, e_use, eps_use, worst))
    print(f"ATTN-ROUND-CPU bwd {RC.spec_id(sp)} flagged P={emu.flagged_p:.5f} dS={emu.flagged_ds:.5f} T_rne={t_rne:.2e} T_trunc={t_trunc:.2e} "
          f"fp32 (tau use, E use, eps use, worst err/bar) order 0: " + " ".join(f"{x:.3f}" for x in figs[0]) + " order 1: " + " ".join(f"{x:.3f}" for x in figs[1]))
    assert emu.flagged_p <= RC.FLAG_CAP_P and emu.flagged_ds <= RC.FLAG_CAP_DS
    for tau_use, e_use, eps_use, worst in figs:
        assert tau_use <= 0.5 and e_use <= 0.5 and eps_use <= 0.5 and worst <= 1.0
    if sp.family == "positive":
        assert abs(t_trunc) > 5e-4 and abs(t_rne) <= abs(t_trunc) / 20
    touched = {"p_trunc": (2,), "p_away": (2,), "ds_trunc": (0, 1), "ds_from_bf16_p": (0, 1), "delta_exact_o": (0, 1), "out_trunc": (0, 1, 2)}
    for fault in RC.bwd_faults_for(sp):
        outs = RC.emulate_bwd(case, fault).outs(fault)
        shares = [float((r > 1).double().mean()) for r in RC.bwd_ratios(outs, emu, g)]
        t = RC.bias(outs[2], want, A)
        biased = sp.family == "positive" and 2 in touched[fault] and abs(t) > abs(t_trunc) / 4
        print(f"ATTN-ROUND-CPU   fault {fault}: outside the bar dq {shares[0]:.3f} dk {shares[1]:.3f} dv {shares[2]:.3f}, T={t:.2e}")
        assert all(shares[i] >= 0.10 for i in touched[fault]) or biased, fault
        assert all(shares[i] == 0.0 for i in range(3) if i not in touched[fault]), fault
