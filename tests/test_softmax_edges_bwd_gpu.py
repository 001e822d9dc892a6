"""attn_bwd_kernel on peaked rows, ties, uniform heads, large common offsets and an lse far from 0: the backward cases of
tests/softmax_cases.py against the float64 autograd gradient of float64 softmax attention on the same bf16 inputs.  Needs an MI355X.

Crafted queries sit four to a 32-query block (every wave of the dQ role's 128-row tile, every 64-query tile the dK / dV role streams);
the dominating keys sit one per wave of a 128-key tile plus one in the ragged last key tile, and each wins >= 8 crafted queries from all
64-query tiles, the ragged last one included.

Bars: rel < 2e-2 per tensor (tests/test_backward_gpu.py, unchanged); the same bar on the crafted rows alone (error over crafted query
rows for dq, over crafted / dominating keys for dk and dv, divided by the tensor-wide max |want|) -- for peaked rows an absolute bound:
the true dq is ~0 and what remains is the bf16 rounding of O inside delta.
dv of a dominating key: its won rows enter with P = 1 (1/2 on a tie; tests/test_softmax_cases_cpu.py proves it to 2^-40), so
dv_j = sum of the won dO rows + what the uncrafted queries add (a dominating key is still a key to every other query; that part is
taken from the reference).  The error of dv_j is held to 2e-2 of the max of that SUM where a correct kernel can reach it.  It cannot
everywhere: the crafted dO rows are scaled down (2^-6, 2^-9 on a tie) so that no crafted gradient is the tensor's largest, the sum is
then ~0.02-0.3 while dv_j itself is ~0.5-2 and leaves the kernel rounded to bf16 once (2^-9 of dv_j).  So per key the bar is
max(2e-2, twice the error of a float64 emulation of the kernel's documented roundings: P to bf16, dv to bf16), both relative to the
sum's max.  Measured on the MI355X and emulated agree to every printed digit (worst key per case): late-spike 256x256 7.1e-3,
200x77 2.5e-2, 333x130 1.5e-2, 512x512 4.1e-3; tie 256x256 5.7e-2, 200x77 1.0e-1, 333x130 1.5e-1, 512x512 4.0e-2.
Each test prints its figures (SOFTMAX-EDGE-BWD ...) before it asserts."""
import pytest
import torch

import softmax_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
BAR = 2e-2


def won_sums(case):
    """[(b, h, j, sum over the won queries of P dO, emulated dv_j)] per dominating key, P = 1 or 1/2; the emulation rounds P and the
    result to bf16 as the kernel does, everything else in float64."""
    if not case.dominating:
        return []
    do = case.do.double().reshape(case.B, case.Nq, case.H, case.D)
    p = S.logits(case)[1]
    w = 0.5 if case.family == "tie" else 1.0
    return [(b, h, j, w * do[b, list(won), h].sum(0), S.bf(S.bf(p[b, h, :, j].float()).double() @ do[b, :, h]).double())
            for b, h, j, won in case.dominating]


def emulate_with_rounded_q(case):
    """float64 emulation of attention_bwd behind attn_self_kernel on the plain entry: o and lse come from scores of q~ = bf16(q c) (the
    kernel's pre-scaled q fragments), P = exp(s - lse) from the exact q, P, dS, o and the results rounded to bf16.  -> (dq, dk, dv)"""
    q, k, v, do = (case.heads4(t.double()) for t in (case.q, case.k, case.v, case.do))
    s = torch.matmul(q, k.transpose(-1, -2)) * (case.c * S.LN2)
    s_fwd = torch.matmul(S.bf((q * case.c).float()).double(), k.transpose(-1, -2)) * S.LN2
    lse = torch.logsumexp(s_fwd, -1, keepdim=True)
    o = S.bf(torch.matmul(S.bf(torch.exp(s_fwd - lse).float()).double(), v).float()).double()
    p = torch.exp(s - lse)
    ds = S.bf((p * (torch.matmul(do, v.transpose(-1, -2)) - (do * o).sum(-1, keepdim=True))).float()).double()
    pb = S.bf(p.float()).double()
    scale = case.c * S.LN2

    def back(t):
        return S.bf(t.permute(0, 2, 1, 3).reshape(case.B, t.shape[2], case.H * case.D).float()).double()

    return back(torch.matmul(ds, k) * scale), back(torch.matmul(ds.transpose(-1, -2), q) * scale), back(torch.matmul(pb.transpose(-1, -2), do))


def check(label, sp, case, dq, dk, dv, emu=None):
    """emu: (dq, dk, dv) of a float64 emulation of the kernels' documented roundings; a bar it cannot meet becomes twice its error."""
    ref = S.reference(case, grads=True)
    figs, ok = [], True
    for n, (name, got, want, rows) in enumerate((("dq", dq, ref.dq, S.q_rows), ("dk", dk, ref.dk, S.k_rows), ("dv", dv, ref.dv, S.k_rows))):
        if got is None:
            continue
        full = got.float().cpu().double()
        assert (full[:, case.Nk:] == 0).all() or name == "dq"  # rows at or beyond Nk exactly 0
        g = full if name == "dq" else full[:, :case.Nk]
        finite = bool(torch.isfinite(g).all())
        scale = want.abs().max().item()
        err = (g - want).abs()
        sub = rows(case, err)
        tensor, crafted = err.max().item() / scale, (sub.max().item() / scale if sub.numel() else 0.0)
        bar_t = bar_c = BAR
        if emu is not None:
            e_err = (emu[n] - want).abs()
            e_sub = rows(case, e_err)
            bar_t, bar_c = max(BAR, 2 * e_err.max().item() / scale), max(BAR, 2 * e_sub.max().item() / scale if e_sub.numel() else 0.0)
        figs.append(f"{name}: finite={finite} tensor={tensor:.3e}/{bar_t:.3e} crafted={crafted:.3e}/{bar_c:.3e}")
        ok = ok and finite and tensor < bar_t and crafted < bar_c
    worst = worst_emu = 0.0
    if dv is not None:
        g = dv.float().cpu().double().reshape(case.B, dv.shape[1], case.H, case.D)
        w = ref.dv.reshape(case.B, case.Nk, case.H, case.D)
        e4 = None if emu is None else emu[2].reshape(case.B, case.Nk, case.H, case.D)
        for b, h, j, s, emu_j in won_sums(case):
            emu_j = emu_j if e4 is None else e4[b, j, h]
            e = (g[b, j, h] - w[b, j, h]).abs().max().item() / s.abs().max().item()
            e = e if e == e else float("inf")  # a NaN row must not drop out of the maximum
            e_emu = (emu_j - w[b, j, h]).abs().max().item() / s.abs().max().item()
            ok = ok and e < max(BAR, 2 * e_emu)
            worst, worst_emu = max(worst, e), max(worst_emu, e_emu)
    print(f"SOFTMAX-EDGE-BWD {label} {S.spec_id(sp)} bar={BAR:g} " + " ".join(figs) + f" dv-of-dominating-keys={worst:.3e} emulated={worst_emu:.3e}")
    assert ok


def padded_leaves(case, kv_grad=True):
    q, k, v = S.device_inputs(case, pad=True)
    return q.requires_grad_(True), k.detach().requires_grad_(kv_grad), v.detach().requires_grad_(kv_grad)


@pytest.mark.parametrize("sp", S.BWD_CASES, ids=S.spec_id)
def test_attention_under_autograd_and_direct(sp):
    """grad.AttentionFn through ops.attention (k / v NaN-padded slices of one tensor), then ops.attention_bwd called directly: the
    dk / dv-only launch (stand-alone delta kernel) equals the fused-delta launch bit for bit on dk and dv."""
    from cd360 import ops
    case = S.make_case(*sp)
    do = case.do.to(DEV, BF)
    q, k, v = padded_leaves(case)
    out = ops.attention(q, k, v, case.H, nk=case.Nk)
    out.backward(do)
    check("autograd", sp, case, q.grad, k.grad, v.grad)
    with torch.no_grad():
        o, lse = ops.attention(q, k, v, case.H, nk=case.Nk, want_lse=True)
        dq, dk, dv = ops.attention_bwd(q, k, v, o, do, lse, case.H, case.Nk)
        none, dk2, dv2 = ops.attention_bwd(q, k, v, o, do, lse, case.H, case.Nk, need_dq=False)
    check("direct", sp, case, dq, dk, dv)
    assert none is None and torch.equal(dk, dk2) and torch.equal(dv, dv2)


@pytest.mark.parametrize("sp", [s for s in S.BWD_CASES if s[3] == s[4]], ids=S.spec_id)
def test_self_attention_qkv_merged_gradient(sp):
    """ops.self_attention_qkv: dq, dk, dv written by the kernel into the three column slices of ONE d(q|k|v) buffer."""
    from cd360 import ops
    case = S.make_case(*sp)
    HD = case.H * case.D
    qkv = torch.cat([case.q, case.k, case.v], -1).to(DEV, BF).requires_grad_(True)
    out = ops.self_attention_qkv(qkv, case.H)
    out.backward(case.do.to(DEV, BF))
    g = qkv.grad
    check("merged", sp, case, g[..., :HD], g[..., HD:2 * HD], g[..., 2 * HD:])


LAZY = [pytest.param(g, s, id=f"attn_self{g}-{S.spec_id(s)}") for s in S.BWD_CASES if s[3] % 128 == 0 and s[4] % 64 == 0
        for g in ((1, 2) if s[3] % 512 == 0 else (1,))]


@pytest.mark.parametrize("gen,sp", LAZY)
def test_backward_from_the_lazy_maximum_lse(gen, sp, tune):
    """attention_bwd fed o and lse of attn_self_kernel (lse = log2 l - negm, a different expression from the first generation's).
    On the plain entry that kernel scores with q~ = bf16(q c), the backward with the exact q: lse is off by up to 2^-9 of the row's
    largest logit (0.1-0.2 at 150 units) and every P of the row by e^that.  Where the 2e-2 bars are out of a correct kernel's reach
    they become twice the error of emulate_with_rounded_q (printed next to each figure).  Measured with the bars at 2e-2 alone:
    offset 256x256 dq 2.9e-2, cold-start 512x512 dk 3.7e-2, dv of dominating keys up to 9.5e-2 of the won sum; all else below 2e-2."""
    from cd360 import ops
    case = S.make_case(*sp)
    tune(attn_self=gen)
    q, k, v = S.device_inputs(case)
    with torch.no_grad():
        o, lse = ops.attention(q, k, v, case.H, nk=case.Nk, want_lse=True)
        dq, dk, dv = ops.attention_bwd(q, k, v, o, case.do.to(DEV, BF), lse, case.H, case.Nk)
    check(f"lazy-lse-gen{gen}", sp, case, dq, dk, dv, emu=emulate_with_rounded_q(case))
