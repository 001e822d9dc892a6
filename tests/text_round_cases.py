"""Per-element cases for the causal attention of the prompt encoders and its backward (cd360_text_causal_attn_bf16, csrc_text/
text_encoder.hip; cd360_textgrad_causal_attn_bwd_bf16, csrc_textgrad/text_backward.hip).  CPU only, no HIP import;
tests/test_text_round_cpu.py checks the method, tests/test_text_round_gpu.py runs the kernels.

Both kernels keep P in fp32 from the scores to the last sum, so nothing can flip: the references are plain float64 causal attention and
its gradients, and the bars are one bf16 rounding of the output plus an fp32 slack on the sum of the absolute terms, per element, nothing
excluded:

    forward    |o - ref| <= 2^-8 |ref| + EPS_T A          A = sum_j p_j |v_j|
    backward   |dx - ref| <= 2^-8 |ref| + EPS_B A_x       A_dq = scale sum_j p_j (|dO| . |v_j| + sum_l p_l |dO| . |v_l|) |k_j|, A_dk likewise
                                                          over the queries with |q_i|, A_dv = sum_i p_ij |dO_i|

EPS_T, EPS_B: the smallest powers of two at which fp32 restatements of the kernels' own order -- one key at a time, expf of m - mn and
s - mn, the fixed tree over a lane's 16 products and the two shuffles, one rounding per operation (the build passes -ffp-contract=off);
the backward's three passes with (max, 1 / l, D) handed over -- stay within HALF of the slack on every case (tests/test_text_round_cpu.py
asserts it and that half of each would not do; never fixed against a kernel).

Families, at scale 1 / 8, q, k, v, dO bf16:
  spread      q gain 1     peaked    q gain 3     positive   peaked, v = |randn| + 0.5 and dO likewise
  stair-up    logits rising by about 1 / 2 per key: every key moves the maximum and rescales l and the accumulators
  stair-down  falling by about 1 / 2 per key: the first key holds the maximum, p_j of about e^{-j / 2}
  wide        q gain 8: CLIP-sized logits of several tens
N = 1, 15, 16, 17 (a wave holds 16 rows), 64, 65, 77, 128; B = 2, H = 2."""
import functools
import math
from dataclasses import dataclass

import torch

from attn_round_cases import bf, flat, rnd

SCALE = 0.125
B, H, D = 2, 2, 64
NS = (1, 15, 16, 17, 64, 65, 77, 128)
FAMILIES = ("spread", "peaked", "positive", "stair-up", "stair-down", "wide")
GAIN = {"spread": 1.0, "peaked": 3.0, "positive": 3.0, "wide": 8.0}
REL = 2.0 ** -8
EPS_T = 2.0 ** -16      # measured use: tests/test_text_round_cpu.py::test_slack_constants prints it (DESIGN 4.1 records it)
EPS_B = 2.0 ** -16
PAD = 8


@dataclass(frozen=True)
class Spec:
    family: str
    N: int


def spec_id(sp):
    return f"{sp.family}-n{sp.N}"


ALL = [Spec(f, n) for f in FAMILIES for n in NS]


@dataclass
class Case:
    spec: Spec
    q: torch.Tensor     # [B, H, N, 64] float64, bf16 values
    k: torch.Tensor
    v: torch.Tensor
    do: torch.Tensor


@functools.lru_cache(maxsize=8)
def make_case(sp: Spec) -> Case:
    g = torch.Generator().manual_seed(7919 * sp.N + 31 * FAMILIES.index(sp.family) + 5)
    r = lambda: torch.randn(B, H, sp.N, D, generator=g, dtype=torch.float32)
    q, k, v, do = r(), r(), r(), r()
    if sp.family in GAIN:
        q = q * GAIN[sp.family]
    else:   # q . k = sum_d (r + 1) (r' / 4 +- j / 16): scale times that rises (falls) by 1 / 2 per key, with noise of about 1 / 3
        step = torch.arange(sp.N, dtype=torch.float32)[None, None, :, None] / 16
        q, k = q + 1, k / 4 + (step if sp.family == "stair-up" else -step)
    if sp.family == "positive":
        v, do = v.abs() + 0.5, do.abs() + 0.5
    return Case(sp, *(bf(x).double() for x in (q, k, v, do)))


def causal(n):
    return torch.ones(n, n, dtype=torch.bool).tril()


# ---- float64 references ------------------------------------------------------------------------------------------------------------------

@dataclass
class Ref:
    o: torch.Tensor
    A: torch.Tensor
    p: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor
    A_dq: torch.Tensor
    A_dk: torch.Tensor
    A_dv: torch.Tensor


@functools.lru_cache(maxsize=8)
def reference(sp: Spec) -> Ref:
    c = make_case(sp)
    x = torch.matmul(c.q, c.k.transpose(-1, -2)) * SCALE
    x = x.masked_fill(~causal(sp.N), float("-inf"))
    p = torch.softmax(x, -1)
    o = torch.matmul(p, c.v)
    dp = torch.matmul(c.do, c.v.transpose(-1, -2))
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dpa = torch.matmul(c.do.abs(), c.v.abs().transpose(-1, -2))
    mag = p * (dpa + (p * dpa).sum(-1, keepdim=True))
    return Ref(o, torch.matmul(p, c.v.abs()), p, torch.matmul(ds, c.k) * SCALE, torch.matmul(ds.transpose(-1, -2), c.q) * SCALE,
               torch.matmul(p.transpose(-1, -2), c.do), torch.matmul(mag, c.k.abs()) * SCALE, torch.matmul(mag.transpose(-1, -2), c.q.abs()) * SCALE,
               torch.matmul(p.transpose(-1, -2), c.do.abs()))


def ratios(got, ref, A, eps):
    """|got - ref| / (2^-8 |ref| + eps A) per element; NaN and inf count as infinite; 0 / 0 (an exact element with no slack) as 0."""
    err = (got.double() - ref).abs()
    r = err / (REL * ref.abs() + eps * A)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))


# ---- the kernels' own order, in fp32 (dtype float32) or float64 ---------------------------------------------------------------------------

FWD_FAULTS = ("diag_skipped", "key_shift", "l_not_rescaled", "quad3", "out_trunc")
BWD_FAULTS = ("delta_rounded_o", "ds_noscale", "quad3", "out_trunc")


def quad_dot(a, b, fault=None):
    """a [.., 64] . b [.., 64] as quad_dot of the kernels: the fixed tree over each lane's 16 products, then the two shuffles."""
    d = a * b
    d = d.reshape(d.shape[:-1] + (4, 16))
    for _ in range(4):
        d = d[..., 0::2] + d[..., 1::2]
    t = d[..., 0]
    if fault == "quad3":
        t = torch.cat([t[..., :3], torch.zeros_like(t[..., 3:])], -1)
    return (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])


def _scores(c: Case, dt, fault=None):
    """(s, dP) [B, H, N, N]: s = fp(quad_dot(q_i, k_j) * scale), dP = quad_dot(dO_i, v_j)."""
    q, k, v, g = (x.to(dt) for x in (c.q, c.k, c.v, c.do))
    s = quad_dot(q[:, :, :, None, :], k[:, :, None, :, :], fault) * SCALE
    return s, quad_dot(g[:, :, :, None, :], v[:, :, None, :, :], fault)


def _mask(n, fault=None):
    m = causal(n)
    if fault == "diag_skipped":
        m = torch.ones(n, n, dtype=torch.bool).tril(-1)
    if fault == "key_shift":
        m = torch.ones(n, n, dtype=torch.bool).tril(1)
    return m


def forward(c: Case, dt=torch.float32, fault=None):
    """text_causal_attn_kernel -> o [B, H, N, 64] in front of the bf16 store."""
    n = c.spec.N
    s, _ = _scores(c, dt, fault)
    v = c.v.to(dt)
    live = _mask(n, fault)
    m = torch.full((B, H, n), float("-inf"), dtype=dt)
    l = torch.zeros(B, H, n, dtype=dt)
    acc = torch.zeros(B, H, n, D, dtype=dt)
    for j in range(n):
        on = live[:, j]
        sj = s[..., j]
        mn = torch.maximum(sj, m)
        alpha, pj = torch.exp(m - mn), torch.exp(sj - mn)
        l2 = (l if fault == "l_not_rescaled" else l * alpha) + pj
        acc2 = acc * alpha[..., None] + pj[..., None] * v[:, :, j, None, :]
        m, l, acc = torch.where(on, mn, m), torch.where(on, l2, l), torch.where(on[:, None], acc2, acc)
    return (acc / l[..., None]).double()


def backward(c: Case, dt=torch.float32, fault=None):
    """textgrad_causal_attn_bwd_kernel -> (dq, dk, dv) in front of their bf16 stores."""
    n = c.spec.N
    s, dp = _scores(c, dt, fault)
    q, k, g = (x.to(dt) for x in (c.q, c.k, c.do))
    live = causal(n)
    m = torch.full((B, H, n), float("-inf"), dtype=dt)
    l = torch.zeros(B, H, n, dtype=dt)
    dd = torch.zeros(B, H, n, dtype=dt)
    for j in range(n):
        on = live[:, j]
        sj = s[..., j]
        mn = torch.maximum(sj, m)
        alpha, pj = torch.exp(m - mn), torch.exp(sj - mn)
        l2, dd2 = l * alpha + pj, dd * alpha + pj * dp[..., j]
        m, l, dd = torch.where(on, mn, m), torch.where(on, l2, l), torch.where(on, dd2, dd)
    inv = 1.0 / l
    dd = dd * inv
    if fault == "delta_rounded_o":   # delta from the forward's bf16 output instead of the fp32 sum of p dP
        o = rnd(forward(c, dt)).to(dt)
        dd = (g * o).sum(-1)
    P = torch.where(live, torch.exp(s - m[..., None]) * inv[..., None], torch.zeros_like(s))
    dS = P * (dp - dd[..., None])
    dq = torch.zeros(B, H, n, D, dtype=dt)
    for j in range(n):      # key by key, in rising order
        dq = dq + dS[..., j, None] * k[:, :, j, None, :]
    dk, dv = torch.zeros(B, H, n, D, dtype=dt), torch.zeros(B, H, n, D, dtype=dt)
    for i in range(n):      # query by query, in rising order (the wave starts at its first row: the rows before a key add nothing)
        dk = dk + dS[:, :, i, :, None] * q[:, :, i, None, :]
        dv = dv + P[:, :, i, :, None] * g[:, :, i, None, :]
    if fault != "ds_noscale":
        dq, dk = dq * SCALE, dk * SCALE
    return dq.double(), dk.double(), dv.double()


def store(x, fault=None):
    """[B, H, N, 64] -> [B, N, H * 64] as the kernel stores it."""
    return rnd(flat(x), "trunc" if fault == "out_trunc" else "rne")


def fwd_faults_for(sp: Spec):
    """The fault models a forward case must expose on >= 10 % of the elements of the region they touch.  Removed where they cannot show, by the
    properties of the case:
      N = 1            one key with probability 1: o = v_0 whatever the score, exact in bf16 -- only diag_skipped (no key at all) shows
      l_not_rescaled   needs a maximum that moves after the first key: on stair-down the first key holds it."""
    if sp.N == 1:
        return ["diag_skipped"]
    return [f for f in FWD_FAULTS if not (f == "l_not_rescaled" and sp.family == "stair-down")]


def fwd_region(sp: Spec, fault):
    """Boolean [B, N, H * 64].  One key more or less weighs 1 / (i + 1) of row i on flat rows and e^{-i / 2} on stair-down: diag_skipped and
    key_shift are judged on the rows of the first wave (i < 16; stair-down: i < 8), the other models on every row."""
    m = torch.ones(B, sp.N, H * D, dtype=torch.bool)
    if fault in ("diag_skipped", "key_shift"):
        m[:, (8 if sp.family == "stair-down" else 16):] = False
    return m


def bwd_faults_for(sp: Spec):
    """(fault, the tensors it touches).  N = 1: P = 1 and dS = 0 exactly, dq = dk = 0 and dv = dO: nothing to expose.  delta_rounded_o is
    removed on the spread family: on flat rows delta averages tens of comparable dP, dP - delta is carried by dP, and the 2^-9 |o| that a
    rounded o moves delta by stays below the store's rounding (as delta_exact_o in attn_round_cases).  A model is caught when ONE of the
    tensors it touches has >= 10 % of its elements outside the bar."""
    if sp.N == 1:
        return []
    f = [("ds_noscale", (0, 1)), ("quad3", (0, 1, 2)), ("out_trunc", (0, 1, 2))]
    return f + ([] if sp.family == "spread" else [("delta_rounded_o", (0, 1))])
