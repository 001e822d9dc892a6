"""cd360_text_causal_attn_bf16 and cd360_textgrad_causal_attn_bwd_bf16 per element against float64 causal attention and its gradients
(tests/text_round_cases.py states the bars and how their constants were fixed; tests/test_text_round_cpu.py checks the method).
Needs an MI355X.

Both kernels keep P in fp32, so nothing can flip; per element, nothing excluded:
    forward    |o - ref| <= 2^-8 |ref| + EPS_T A
    backward   |dq, dk, dv - ref| <= 2^-8 |ref| + EPS_B A_x
N = 1, 15, 16, 17, 64, 65, 77, 128 x spread, peaked, positive, stair-up, stair-down, wide; B = 2, H = 2, scale 1 / 8; q | k | v the column
slices of one merged [B, N + 8, 3 H 64] buffer whose rows >= N are NaN, dO likewise padded; the outputs are NaN-filled, rows >= N must stay so.
Each test prints TEXT-ATTN <kernel> <case> worst=<err / bar> before it asserts."""
import pytest
import torch

import text_round_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
IDS = [TC.spec_id(sp) for sp in TC.ALL]


def device_inputs(sp):
    """(q, k, v) the slices of the merged buffer, dO [B, N + 8, H * 64]; rows >= N NaN."""
    c = TC.make_case(sp)
    C = TC.H * TC.D
    m = torch.full((TC.B, sp.N + TC.PAD, 3 * C), NAN, dtype=torch.float64)
    m[:, :sp.N, :C], m[:, :sp.N, C:2 * C], m[:, :sp.N, 2 * C:] = TC.flat(c.q), TC.flat(c.k), TC.flat(c.v)
    g = torch.full((TC.B, sp.N + TC.PAD, C), NAN, dtype=torch.float64)
    g[:, :sp.N] = TC.flat(c.do)
    m, g = m.to(DEV, BF), g.to(DEV, BF)
    return m[..., :C], m[..., C:2 * C], m[..., 2 * C:], g


@pytest.mark.parametrize("sp", TC.ALL, ids=IDS)
def test_causal_attention_forward(sp):
    from cd360 import ops
    r = TC.reference(sp)
    q, k, v, _ = device_inputs(sp)
    runs = []
    for _ in range(2):
        out = torch.full((TC.B, sp.N + TC.PAD, TC.H * TC.D), NAN, dtype=BF, device=DEV)
        ops.causal_attention(q, k, v, TC.H, scale=TC.SCALE, n=sp.N, out=out[:, :sp.N])
        runs.append(out)
    got = runs[0][:, :sp.N].float().cpu().double()
    worst = float(TC.ratios(got, TC.flat(r.o), TC.flat(r.A), TC.EPS_T).max())
    print(f"TEXT-ATTN text_causal_attn_kernel {TC.spec_id(sp)} worst={worst:.3f}/1")
    assert worst <= 1.0
    assert bool(torch.isnan(runs[0][:, sp.N:]).all()), "rows >= N written"
    assert torch.equal(runs[0][:, :sp.N].view(torch.int16), runs[1][:, :sp.N].view(torch.int16)), "two runs differ"


@pytest.mark.parametrize("sp", TC.ALL, ids=IDS)
def test_causal_attention_backward(sp):
    from cd360 import ops
    r = TC.reference(sp)
    q, k, v, g = device_inputs(sp)
    C = TC.H * TC.D
    runs = []
    for _ in range(2):
        buf = torch.full((TC.B, sp.N + TC.PAD, 3 * C), NAN, dtype=BF, device=DEV)
        ops.causal_attention_bwd(q, k, v, g, TC.H, scale=TC.SCALE, n=sp.N, out=(buf[:, :sp.N, :C], buf[:, :sp.N, C:2 * C], buf[:, :sp.N, 2 * C:]))
        runs.append(buf)
    got = runs[0][:, :sp.N].float().cpu().double()
    refs = ((r.dq, r.A_dq), (r.dk, r.A_dk), (r.dv, r.A_dv))
    worst = [float(TC.ratios(got[..., i * C:(i + 1) * C], TC.flat(y), TC.flat(A), TC.EPS_B).max()) for i, (y, A) in enumerate(refs)]
    print(f"TEXT-ATTN textgrad_causal_attn_bwd_kernel {TC.spec_id(sp)} worst={max(worst):.3f}/1 dq={worst[0]:.3f} dk={worst[1]:.3f} dv={worst[2]:.3f}")
    assert max(worst) <= 1.0
    assert bool(torch.isnan(runs[0][:, sp.N:]).all()), "rows >= N written"
    assert torch.equal(runs[0][:, :sp.N].view(torch.int16), runs[1][:, :sp.N].view(torch.int16)), "two runs differ"
