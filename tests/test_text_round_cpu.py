"""The method of tests/text_round_cases.py, checked without a GPU: the fp32 restatements of text_causal_attn_kernel and of
textgrad_causal_attn_bwd_kernel in the kernels' own order stay within half of the fp32 slack of their bars on every case (and would not
at half the constants), the float64 run of the same order is the float64 reference, and every fault model is caught where it is listed.
Prints TEXT-ATTN-CPU lines with the measured use."""
import pytest
import torch

import text_round_cases as TC

IDS = [TC.spec_id(sp) for sp in TC.ALL]


def _use(sp):
    c, r = TC.make_case(sp), TC.reference(sp)
    o32 = TC.forward(c)
    b32 = TC.backward(c)
    refs = ((r.dq, r.A_dq), (r.dk, r.A_dk), (r.dv, r.A_dv))
    use_t = float(((o32 - r.o).abs() / r.A).max()) / TC.EPS_T
    use_b = max(float(((x - y).abs() / A.clamp_min(1e-300)).max()) for x, (y, A) in zip(b32, refs)) / TC.EPS_B
    worst_f = float(TC.ratios(TC.store(o32), TC.flat(r.o), TC.flat(r.A), TC.EPS_T).max())
    worst_b = max(float(TC.ratios(TC.store(x), TC.flat(y), TC.flat(A), TC.EPS_B).max()) for x, (y, A) in zip(b32, refs))
    return use_t, use_b, worst_f, worst_b


@pytest.mark.parametrize("sp", TC.ALL, ids=IDS)
def test_fp32_restatement_and_faults(sp):
    c, r = TC.make_case(sp), TC.reference(sp)
    use_t, use_b, worst_f, worst_b = _use(sp)
    # the kernels' order in float64 is the reference
    assert float((TC.forward(c, torch.float64) - r.o).abs().max()) < 1e-13
    for x, y in zip(TC.backward(c, torch.float64), (r.dq, r.dk, r.dv)):
        assert float((x - y).abs().max()) < 1e-12 * max(1.0, float(y.abs().max()))
    print(f"TEXT-ATTN-CPU {TC.spec_id(sp)} fp32 use of EPS_T {use_t:.3f} of EPS_B {use_b:.3f}, worst err/bar forward {worst_f:.3f} backward {worst_b:.3f}")
    assert use_t <= 0.5 and use_b <= 0.5 and worst_f <= 1.0 and worst_b <= 1.0
    for fault in TC.fwd_faults_for(sp):
        out = TC.store(TC.forward(c, torch.float64, fault), fault)
        reg = TC.fwd_region(sp, fault)
        share = float((TC.ratios(out, TC.flat(r.o), TC.flat(r.A), TC.EPS_T)[reg] > 1).double().mean())
        print(f"TEXT-ATTN-CPU   forward fault {fault}: outside the bar {share:.3f} of {int(reg.sum())}")
        assert share >= 0.10, fault
    refs = ((r.dq, r.A_dq), (r.dk, r.A_dk), (r.dv, r.A_dv))
    for fault, touched in TC.bwd_faults_for(sp):
        outs = [TC.store(x, fault) for x in TC.backward(c, torch.float64, fault)]
        shares = [float((TC.ratios(outs[i], TC.flat(refs[i][0]), TC.flat(refs[i][1]), TC.EPS_B) > 1).double().mean()) for i in touched]
        print(f"TEXT-ATTN-CPU   backward fault {fault}: outside the bar " + " / ".join(f"{x:.3f}" for x in shares))
        assert max(shares) >= 0.10, fault


def test_slack_constants():
    """EPS_T and EPS_B are the smallest powers of two that hold half of themselves over the whole list."""
    uses = [_use(sp)[:2] for sp in TC.ALL]
    ut, ub = max(u[0] for u in uses), max(u[1] for u in uses)
    print(f"TEXT-ATTN-CPU worst fp32 use of EPS_T = 2^{torch.log2(torch.tensor(TC.EPS_T)).item():.0f}: {ut:.3f}, of EPS_B = 2^{torch.log2(torch.tensor(TC.EPS_B)).item():.0f}: {ub:.3f}")
    assert 0.25 < ut <= 0.5 and 0.25 < ub <= 0.5


def test_every_fault_model_is_listed():
    assert set(f for sp in TC.ALL for f in TC.fwd_faults_for(sp)) == set(TC.FWD_FAULTS)
    assert set(f for sp in TC.ALL for f, _ in TC.bwd_faults_for(sp)) == set(TC.BWD_FAULTS)
    assert {sp.N for sp in TC.ALL} == {1, 15, 16, 17, 64, 65, 77, 128} and {sp.family for sp in TC.ALL} == set(TC.FAMILIES)


def test_stairs_move_the_maximum():
    """stair-up: nearly every key of a row is a new maximum; stair-down: hardly any after the first."""
    for fam, lo, hi in (("stair-up", 0.6, 1.0), ("stair-down", 0.0, 0.1)):
        c = TC.make_case(TC.Spec(fam, 128))
        x = torch.matmul(c.q, c.k.transpose(-1, -2))
        new_max = (x[..., 1:] > torch.cummax(x, -1).values[..., :-1]) & TC.causal(128)[:, 1:]
        share = float(new_max.sum() / TC.causal(128)[:, 1:].sum() / (TC.B * TC.H))
        print(f"TEXT-ATTN-CPU {fam}: {share:.3f} of the keys behind the first move the maximum")
        assert lo <= share <= hi
