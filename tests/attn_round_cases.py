"""Off-grid rounding cases for every attention kernel that rounds P (and, in the backward, dS) to bf16 in front of an MFMA (CPU only, no
HIP import; tests/test_attn_round_cpu.py checks the method, tests/test_attn_round_gpu.py runs the kernels).  The power-of-two suites
(attn_grid_cases.py, attn_tile_cases.py) cannot see these roundings: on their inputs every p is a power of two.  Here q, k, v and dO are
`randn` rounded to bf16, the softmax scale is the ordinary 1 / 8 (scale * log2(e) is not 1), and three families set how much one bf16 ulp
of P weighs:

  spread    q gain 1: flat rows, tens of comparable keys
  peaked    q gain 3: a handful of keys carry the row, with non-integer logits
  positive  peaked q, v = bf16(|randn| + 0.5) (and dO likewise in the backward): a P that is truncated biases every output low

Method.  Each pipeline is restated in float64 with an explicit round-to-nearest-even to bf16 at exactly the points where the kernel
source rounds, and nowhere else:

  row     attn_smallk_kernel<1..3, false> and the <= 96-key epilogue of the fused q projection (csrc/gemm8p.hip): one maximum per row,
          x = fma(s, c, -m c), p = exp2(x), l = sum of the fp32 p, P = bf16(p), o = bf16(O / l)
  eager   attn_fwd_kernel: the same per 64-key tile with the running maximum; P is rounded AT THAT TILE'S SCALE, l and O are rescaled by
          alpha = exp2((m_old - m_new) c), which is no power of two
  lazy    attn_self_kernel: q~ = bf16(fp32(q c)) (c = 1 on the pre-scaled entry: q~ = q), scores in exp2 units less m_ref; m_ref starts
          at 0, follows the .ref key half of tile 0 wherever it stands and of a later tile when that stands more than 8 above it
          (move_ref, alpha = exp2(-d)); catch_up then moves on by a whole number of units (an exact power of two: no trace in P)
  single  attn_single_kernel + attn_single_combine_kernel: s = fp32(s qscale), 32-key tiles with an eager maximum, per split a normalised
          fp32 part O / l and lse2 = m + log2(l); the combine weighs the parts by exp2(lse2 - max lse2) and rounds once
  bwd     attn_bwd_kernel: lse2 = fp32(lse log2 e), P = exp2(fma(s, c, -lse2)), delta = rowsum(dO o) of the bf16 o, dS = P (dP - delta)
          from the fp32 P; bf16(P) feeds dV, bf16(dS) feeds dQ and dK, which are scaled and rounded once on store.  o (bf16) and lse
          (fp32) are inputs, computed on the host in float64, so both sides share them bit for bit.

The bar, per element, nothing excluded:   |got - emu| <= 2^-8 |emu| + EPS A + F

emu is the emulation in front of its output rounding (2^-8 |emu| is that rounding), A the softmax-weighted mean of |v| (backward: of the
magnitudes of the tensor's own products) and F the FLIP ALLOWANCE: the kernel's fp32 p differs from the float64 p by a relative error of
at most tau, so a p within tau of a bf16 rounding midpoint may round the other way.  Every (row, key) pair flagged that way adds
ulp_bf16(p) |v| / l to F, carried through the same alpha rescales as O.  In the backward a flagged P feeds dV, a flagged dS feeds dQ and
dK; the flag of dS uses an absolute bound, since dP - delta cancels.

    tau   = ln 2 (C_QK sum_d |q_d k_d| c + C_X |x|) + C_E        x: the argument of exp2
    E(dS) = P C_D (sum |dO v| + sum |dO o|) + tau |dS|

C_QK, C_X, C_E, C_D, EPS and LSE_REL are fixed on the CPU (never against a kernel): the smallest powers of two at which fp32
restatements of the pipelines, in two summation orders, keep every fp32 p (P, dS) within HALF of tau (E) of the float64 one -- whatever
can flip is then flagged with a factor two to spare --, what is left of |o32 - o64| after F within HALF of EPS A, and lse within half of
LSE_REL (|lse| + 1) (tests/test_attn_round_cpu.py asserts it; DESIGN section 4.1 records how far inside).  A flagged pair that does flip
uses its whole allowance (ulp |v| / l is exactly what it moves the output by), so the half is asked of tau, E and EPS and not of F.
C_E alone is not the measured minimum: it stays at one ulp of v_exp_f32.

lse.  The entries that return lse (cd360_attn_fwd_lse_bf16 on the row, eager and lazy pipelines) are held to |lse - emu| <= LSE_REL
(|emu| + 1): l summed from the rounded P, which the output's own rounding hides in o, shows there.

Signed bias.  On the positive family T = mean((got - exact64) / A) against float64 softmax attention with no P rounding at all; the bar
is |T| <= |T_trunc| / 4, T_trunc being the statistic of the emulation with P truncated.  The round-to-nearest pipeline stays below
|T_trunc| / 20."""
import functools
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from attn_tile_cases import _pv, _sum, key_half
from softmax_cases import SINGLE_KT, single_splits

SCALE = 0.125
LOG2E_F32 = np.float32(1.4426950408889634)
LN2_F32 = np.float32(0.6931471805599453)
C = float(np.float32(SCALE) * LOG2E_F32)    # scale * log2(e) as the entry points form it, in fp32
SLACK = 8.0
MARGIN = 2.0 ** -10                         # a move_ref decision closer than this to the slack may go either way
PAD = 8                                     # NaN rows behind the real keys on the device

C_QK = 2.0 ** -21
C_X = 2.0 ** -24
C_E = 2.0 ** -23
C_D = 2.0 ** -23
EPS = 2.0 ** -17
LSE_REL = 2.0 ** -21     # |lse - emu| <= LSE_REL (|emu| + 1), fixed like EPS
REL = 2.0 ** -8

FAMILIES = ("spread", "peaked", "positive")
GAIN = {"spread": 1.0, "peaked": 3.0, "positive": 3.0}
FLAG_CAP_P, FLAG_CAP_DS, MARGINAL_CAP = 0.01, 0.02, 0.005


@dataclass(frozen=True)
class Spec:
    family: str
    Nq: int
    Nk: int
    B: int = 2
    H: int = 2
    D: int = 64
    seed: int = 0
    dup: int = 0         # fused q projection: 1 = both output batch elements come from query batch 0 (on the keys of batch 0 and of batch 1)


def spec_id(sp: Spec) -> str:
    return f"{sp.family}-b{sp.B}h{sp.H}-{sp.Nq}x{sp.Nk}" + (f"-d{sp.D}" if sp.D != 64 else "") + ("-dup" if sp.dup else "")


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.bfloat16().to(x.dtype)


@dataclass
class Case:
    spec: Spec
    q: torch.Tensor       # [B, H, Nq, D] float64, bf16 values
    k: torch.Tensor       # [B, H, Nk, D]
    v: torch.Tensor
    do: torch.Tensor      # [B, H, Nq, D]


@functools.lru_cache(maxsize=8)
def make_case(sp: Spec) -> Case:
    assert sp.family in FAMILIES
    g = torch.Generator().manual_seed(1009 * sp.Nk + 17 * sp.Nq + sp.D + 7 * sp.B + sp.H + 100003 * sp.seed)
    r = lambda n: torch.randn(sp.B, sp.H, n, sp.D, generator=g, dtype=torch.float32)
    # (head dims above 64 keep the scale of 1 / 8: the gain carries sqrt(64 / D), so the logits have the statistics of head dim 64)
    q, k, v, do = r(sp.Nq) * (GAIN[sp.family] * math.sqrt(64.0 / sp.D)), r(sp.Nk), r(sp.Nk), r(sp.Nq)
    if sp.family == "positive":
        v, do = v.abs() + 0.5, do.abs() + 0.5
    if sp.dup:
        assert sp.B == 2
        q[1] = q[0]
    return Case(sp, *(bf(x).double() for x in (q, k, v, do)))


def flat(x):
    """[B, H, N, D] -> [B, N, H * D], the layout of the kernels' outputs."""
    return x.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[2], -1)


def heads(x, H):
    """[B, N, H * D] -> [B, H, N, D]."""
    return x.reshape(x.shape[0], x.shape[1], H, -1).permute(0, 2, 1, 3)


# ---- roundings to the bf16 grid, in float64 -----------------------------------------------------------------------------------------

def grid(x):
    """(y, u): x = y u with |y| in [128, 256) and u the bf16 spacing in x's binade (x = 0: y = 0, u = 2^-8)."""
    _, e = torch.frexp(x)
    u = torch.ldexp(torch.ones_like(x), e - 8)
    return x / u, u


def rnd(x, mode="rne"):
    """x on the bf16 grid: round to nearest even, truncated, or away from zero (no overflow or subnormal handling: |x| stays far from both)."""
    y, u = grid(x)
    if mode == "rne":
        y = torch.round(y)
    elif mode == "trunc":
        y = torch.trunc(y)
    else:
        assert mode == "away"
        y = torch.sign(y) * torch.ceil(y.abs())
    return y * u


def near_midpoint(x, err):
    """(flag, ulp): |x| lies within err (absolute) of the midpoint of two neighbouring bf16 values."""
    y, u = grid(x)
    y = y.abs()
    return ((y - torch.floor(y) - 0.5).abs() * u <= err) & (x != 0), u


def midpoints_within(x, err):
    """(count, ulp): how many bf16 rounding midpoints lie within err (absolute) of |x|, counted at the spacing of x's own binade -- for an err
    below half a spacing this is near_midpoint's flag."""
    y, u = grid(x)
    y, e = y.abs(), err / u
    n = torch.floor(y + e - 0.5) - torch.ceil(y - e - 0.5) + 1
    return n.clamp_min(0) * (x != 0), u


def tau(sa_c, x):
    return math.log(2.0) * (C_QK * sa_c + C_X * x.abs()) + C_E


def R(x, f32):
    """The fp32 restatements round every intermediate to fp32; the float64 emulation does not."""
    return x.float().double() if f32 else x


def mm(a, b, f32, order=0):
    """a @ b; in fp32 and, order 1, with the reduction split in two halves taken in the other order."""
    if not f32:
        return torch.matmul(a, b)
    return _pv(a.float(), b.float(), order).double() if a.shape[-1] % 2 == 0 else torch.matmul(a.float(), b.float()).double()


def rowsum(p, f32, order=0):
    if not f32:
        return p.sum(-1)
    n = p.shape[-1]
    if n % 4:
        p = torch.cat([p, p.new_zeros(p.shape[:-1] + (4 - n % 4,))], -1)
    return _sum(p.float(), order).double()


def exp2(x, f32):
    return torch.exp2(x.float()).double() if f32 else torch.exp2(x)


# ---- float64 softmax attention with no P rounding at all -------------------------------------------------------------------------------

@dataclass
class Exact:
    out: torch.Tensor     # [B, H, Nq, D]
    A: torch.Tensor       # the softmax-weighted mean of |v|
    p: torch.Tensor       # [B, H, Nq, Nk], normalised
    lse: torch.Tensor     # [B, H, Nq] natural logarithm
    x: torch.Tensor       # logits in exp2 units


def exact_of(q, k, v, c=C) -> Exact:
    x = torch.matmul(q, k.transpose(-1, -2)) * c
    mx = x.amax(-1, keepdim=True)
    p = torch.exp2(x - mx)
    l = p.sum(-1, keepdim=True)
    p = p / l
    return Exact(torch.matmul(p, v), torch.matmul(p, v.abs()), p, math.log(2.0) * (mx + torch.log2(l)).squeeze(-1), x)


@functools.lru_cache(maxsize=8)
def _exact(sp: Spec) -> Exact:
    case = make_case(sp)
    return exact_of(case.q, case.k, case.v)


def exact(case: Case) -> Exact:
    return _exact(case.spec)


# ---- the forward pipelines ---------------------------------------------------------------------------------------------------------------

FWD_FAULTS = ("p_trunc", "p_away", "p_norm", "p_alpha", "l_bf16", "out_trunc")
Q_FAULTS = ("q_unrounded", "q_bf16_mul", "q_direct")
P_MODE = {"p_trunc": "trunc", "p_away": "away"}


@dataclass
class Fwd:
    o: torch.Tensor                 # [B, H, Nq, D] in front of the output rounding
    F: torch.Tensor                 # flip allowance, same shape
    flagged: float = 0.0            # share of the (row, key) pairs
    m: Optional[torch.Tensor] = None      # final reference (exp2 units), l relative to it
    l: Optional[torch.Tensor] = None
    ms: list = field(default_factory=list)   # the reference after every tile
    marginal: Optional[torch.Tensor] = None  # lazy: [B, H, Nq, tiles] decisions inside MARGIN
    moves: int = 0
    lse2: Optional[torch.Tensor] = None
    ps: list = field(default_factory=list)   # per tile: p in front of its rounding, and (float64 run) tau
    taus: list = field(default_factory=list)
    lse: Optional[torch.Tensor] = None    # [B, H, Nq] natural logarithm, as cd360_attn_fwd_lse_bf16 returns it (row, eager, lazy)

    def out(self, fault=None):
        """[B, Nq, H * D] rounded to bf16 as the kernel stores it."""
        return rnd(flat(self.o), "trunc" if fault == "out_trunc" else "rne")


def _round_p(p, fault, g):
    """bf16(P) as the MFMA takes it.  g [rows]: the fault models that round at another scale round p g and undo g afterwards."""
    if g is not None:
        return rnd(p * g[..., None]) / g[..., None]
    return rnd(p, P_MODE.get(fault, "rne"))


def _lse(m2, l, f32):
    """(m + log2(l)) ln 2, m in exp2 units."""
    return R(R(m2 + (torch.log2(l.float()).double() if f32 else torch.log2(l)), f32) * float(LN2_F32), f32)


def _tiled(s_all, sa_c, v, c, tile, fault=None, f32=False, order=0, clean=None, tau_extra=None) -> Fwd:
    """The eager pipeline over the keys given: s_all raw scores [B, H, Nq, n], x = fma(s, c, -m c).  tile >= n: the whole-row pipeline.
    clean: the fault-free run of the same call (p_norm, p_alpha read their scales from it).  tau_extra [B, H, Nq, n]: a relative
    uncertainty of p from outside the pipeline (a q that may round either way, tests/qproj_cases.py), added to tau."""
    n = s_all.shape[-1]
    shape = s_all.shape[:-1]
    m = s_all.new_full(shape, float("-inf"))
    l = s_all.new_zeros(shape)
    O = s_all.new_zeros(shape + (v.shape[-1],))
    F = torch.zeros_like(O)
    nflag, ms, ps, taus = 0, [], [], []
    nt = -(-n // tile)
    for t in range(nt):
        s, vt, sa = s_all[..., t * tile:(t + 1) * tile], v[..., t * tile:(t + 1) * tile, :], sa_c[..., t * tile:(t + 1) * tile]
        m_new = torch.maximum(m, s.amax(-1))
        alpha = R(exp2(R((m - m_new) * c, f32), f32), f32)
        mc = R(-m_new * c, f32)
        x = R(s * c + mc[..., None], f32)
        p = exp2(x, f32)
        g = None
        if fault == "p_norm":
            g = torch.exp2((m_new - clean.m) * c) / clean.l
        if fault == "p_alpha" and t + 1 < nt:
            g = torch.exp2((m_new - clean.ms[t + 1]) * c)
        pb = _round_p(p, fault, g)
        l = R(R(l * alpha, f32) + rowsum(pb if fault == "l_bf16" else p, f32, order), f32)
        O = R(R(O * alpha[..., None], f32) + mm(pb, vt, f32, order), f32)
        ps.append(p)
        if not f32:
            tp = tau(sa, x)
            if tau_extra is not None:    # (may exceed a spacing of p: every midpoint it reaches counts)
                tp = tp + tau_extra[..., t * tile:(t + 1) * tile]
            taus.append(tp)
            flag, u = near_midpoint(p, tp * p) if tau_extra is None else midpoints_within(p, tp * p)
            nflag += int((flag > 0).sum())
            F = F * alpha[..., None] + torch.matmul(flag * u, vt.abs())
        m = m_new
        ms.append(m)
    inv = R(1.0 / l, f32)
    return Fwd(R(O * inv[..., None], f32), F / l[..., None], nflag / s_all.numel(), m, l, ms, ps=ps, taus=taus, lse=_lse(R(m * c, f32), l, f32))


def scores(q, k, f32=False, order=0):
    """q k^T and |q| |k|^T."""
    return mm(q, k.transpose(-1, -2), f32, order), torch.matmul(q.abs(), k.abs().transpose(-1, -2))


def emulate_row(case: Case, fault=None, f32=False, order=0, tau_extra=None) -> Fwd:
    """attn_smallk_kernel<NKB, false> / the <= 96-key epilogue of the fused q projection."""
    s, sa = scores(case.q, case.k, f32, order)
    clean = _tiled(s, sa * C, case.v, C, 1 << 30) if fault in ("p_norm", "p_alpha") else None
    return _tiled(s, sa * C, case.v, C, 1 << 30, fault, f32, order, clean, tau_extra)


def emulate_eager(case: Case, fault=None, f32=False, order=0) -> Fwd:
    """attn_fwd_kernel."""
    s, sa = scores(case.q, case.k, f32, order)
    clean = _tiled(s, sa * C, case.v, C, 64) if fault in ("p_norm", "p_alpha") else None
    return _tiled(s, sa * C, case.v, C, 64, fault, f32, order, clean)


def q_tilde(q, c=C, fault=None):
    """The pre-scaled q fragments of attn_self_kernel: pack_bf16x2 of the fp32 products q c."""
    if c == 1.0:
        return q
    if fault == "q_unrounded":
        return q * c
    if fault == "q_bf16_mul":    # rounded twice: c itself to bf16 (a packed bf16 multiply), then the product.  (Two bf16 steps through the
        return rnd(q * float(rnd(torch.tensor(c, dtype=torch.float64))))   # scale and log2 e are no fault model here: 1 / 8 is a power of two)
    if fault == "q_direct":      # the exact product rounded to bf16 without the fp32 rounding in between
        return rnd(q * c)
    return bf((q * c).float()).double()


def emulate_lazy(case: Case, fault=None, f32=False, order=0, prescaled=False, flip=None, clean=None) -> Fwd:
    """attn_self_kernel.  prescaled: the entry that takes q~ as its input (the test passes q_tilde(q) there, so both entries see the same
    fragments).  flip [B, H, Nq, tiles] inverts the move_ref decisions it marks."""
    sp = case.spec
    assert sp.Nk % 64 == 0 and sp.D == 64
    qt = q_tilde(case.q, C, None if prescaled else fault)
    s_all, sa_all = scores(qt, case.k, f32, order)
    if fault in ("p_norm", "p_alpha") and clean is None:
        clean = emulate_lazy(case, None, prescaled=prescaled)
    hf = torch.from_numpy(key_half(np.arange(64))).bool()
    shape = s_all.shape[:-1]
    m, l = s_all.new_zeros(shape), s_all.new_zeros(shape)
    O = s_all.new_zeros(shape + (sp.D,))
    F = torch.zeros_like(O)
    nt = sp.Nk // 64
    marginal = torch.zeros(shape + (nt,), dtype=torch.bool)
    nflag = moves = 0
    ms, ps, taus = [], [], []
    for t in range(nt):
        vt, sa = case.v[..., t * 64:(t + 1) * 64, :], sa_all[..., t * 64:(t + 1) * 64]
        s = R(s_all[..., t * 64:(t + 1) * 64] - m[..., None], f32)
        ref, both = s[..., ~hf].amax(-1), s.amax(-1)
        if t == 0:
            take = torch.ones_like(ref, dtype=torch.bool)
        else:
            take = ref > SLACK
            marginal[..., t] = (ref - SLACK).abs() < MARGIN
            if flip is not None:
                take = take ^ flip[..., t]
            moves += int(take.sum())
        d = torch.where(take, ref, torch.zeros_like(ref))
        rest = both - d
        n = torch.where(rest > SLACK, rest.floor(), torch.zeros_like(rest))
        alpha = R(exp2(-d.clamp_min(0), f32), f32) * torch.exp2(-n)
        s = R(R(s - d[..., None], f32) - n[..., None], f32)
        m = R(R(m + d, f32) + n, f32)
        l, O, F = R(l * alpha, f32), R(O * alpha[..., None], f32), F * alpha[..., None]
        p = exp2(s, f32)
        g = None
        if fault == "p_norm":
            g = torch.exp2(m - clean.m) / clean.l
        if fault == "p_alpha" and t + 1 < nt:
            g = torch.exp2(m - clean.ms[t + 1])
        pb = _round_p(p, fault, g)
        l = R(l + rowsum(pb if fault == "l_bf16" else p, f32, order), f32)
        O = R(O + mm(pb, vt, f32, order), f32)
        ps.append(p)
        if not f32:
            tp = tau(sa, s)
            taus.append(tp)
            flag, u = near_midpoint(p, tp * p)
            nflag += int(flag.sum())
            F = F + torch.matmul(flag * u, vt.abs())
        ms.append(m)
    inv = R(1.0 / l, f32)
    return Fwd(R(O * inv[..., None], f32), F / l[..., None], nflag / s_all.numel(), m, l, ms, marginal, moves, ps=ps, taus=taus, lse=_lse(m, l, f32))


def emulate_single(case: Case, fault=None, f32=False, order=0, qscale=C, qmul=1.0) -> Fwd:
    """attn_single_kernel (+ attn_single_combine_kernel where the keys are split), H = 1.  qmul multiplies q exactly (a doubled q under
    qscale / 2 gives the same scores bit for bit)."""
    sp = case.spec
    s_raw, sa = scores(case.q * qmul, case.k, f32, order)
    s_all, sa_c = R(s_raw * qscale, f32), sa * (qmul * qscale)
    ns, per = single_splits(sp.Nk)
    parts = []
    for i in range(ns):
        sl = slice(i * per, min((i + 1) * per, sp.Nk))
        clean = _tiled(s_all[..., sl], sa_c[..., sl], case.v[..., sl, :], 1.0, SINGLE_KT) if fault in ("p_norm", "p_alpha") else None
        part = _tiled(s_all[..., sl], sa_c[..., sl], case.v[..., sl, :], 1.0, SINGLE_KT, fault, f32, order, clean)
        part.lse2 = R(part.m + (torch.log2(part.l.float()).double() if f32 else torch.log2(part.l)), f32)
        parts.append(part)
    flagged = sum(p.flagged * (min((i + 1) * per, sp.Nk) - i * per) for i, p in enumerate(parts)) / sp.Nk
    ps, taus = sum((p.ps for p in parts), []), sum((p.taus for p in parts), [])
    if ns == 1:
        return Fwd(parts[0].o, parts[0].F, flagged, ps=ps, taus=taus)
    L = torch.stack([p.lse2 for p in parts])
    w = exp2(R(L - L.amax(0), f32), f32)
    tot, Ft, wsum = torch.zeros_like(parts[0].o), torch.zeros_like(parts[0].o), torch.zeros_like(w[0])
    for i in (range(ns) if order == 0 else range(ns - 1, -1, -1)):
        tot = R(tot + R(w[i][..., None] * parts[i].o, f32), f32)
        Ft = Ft + w[i][..., None] * parts[i].F
        wsum = R(wsum + w[i], f32)
    inv = R(1.0 / wsum, f32)
    return Fwd(R(tot * inv[..., None], f32), Ft / wsum[..., None], flagged, ps=ps, taus=taus)


PIPELINES = {"row": emulate_row, "eager": emulate_eager, "lazy": emulate_lazy, "single": emulate_single}


def faults_for(pipeline: str, sp: Spec, prescaled=False):
    """The fault models a case must expose, either on >= 10 % of the elements or through the bias statistic.  Removed where they cannot show,
    by the properties of the case and not by what a run gives:
      l_bf16     shows in lse and nowhere else (l enters o as 1 / l alone: summing the rounded P moves it by about 2^-9 / sqrt(keys that
                 carry the row), below the output's own rounding, and round-to-nearest leaves no bias).  Listed for the pipelines whose
                 entry returns lse (row through cd360_attn_fwd_lse_bf16, eager, lazy); the single-head kernel and the fused projection
                 return none.
      p_alpha    has no meaning without an alpha (row) and none in the lazy pipeline, whose rescales are exact powers of two except in
                 move_ref (a few rows of these cases).  In the eager and single pipelines only the rows whose maximum still moves AFTER the
                 tile in question are touched: enough of them on the spread family from three tiles on, a few per cent on peaked rows,
                 whose maximum settles early.
      p_norm, p_alpha, q_*   on the positive family: every term of a row has the same sign, A = |o|, and errors that are random from key to key
                 average out against that bar.  The family is there for the bias statistic, which truncation and rounding away answer to.
      q_*        the plain entry of the lazy pipeline alone forms q~.
      q_direct   bf16(q c) and bf16(fp32(q c)) differ only where the fp32 rounding crosses a bf16 midpoint, about 2^-15 of the elements of q:
                 a handful of scores per case, nothing an output statistic can see.  Never listed."""
    f = ["p_trunc", "p_away", "out_trunc"] + (["l_bf16"] if pipeline != "single" else [])
    if sp.family != "positive":
        f.append("p_norm")
        if sp.family == "spread" and (pipeline == "single" or (pipeline == "eager" and sp.Nk > 128)):
            f.append("p_alpha")
        if pipeline == "lazy" and not prescaled:
            f += ["q_unrounded", "q_bf16_mul"]
    return f


# ---- verdicts ----------------------------------------------------------------------------------------------------------------------------

def ratios(got, emu_o, A, F):
    """|got - emu| / (2^-8 |emu| + EPS A + F) per element (NaN and inf count as infinite); all arguments in the same layout."""
    r = (got.double() - emu_o).abs() / (REL * emu_o.abs() + EPS * A + F)
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))


def forward_ratios(got, emu: Fwd, A, alt: Optional[Fwd] = None):
    """got [B, Nq, H * D].  alt: the lazy pipeline's emulation with its marginal decisions inverted; the rows that have one are judged
    against the envelope of both."""
    r = ratios(got, flat(emu.o), flat(A), flat(emu.F))
    if alt is not None:
        r2 = ratios(got, flat(alt.o), flat(A), flat(alt.F))
        rows = flat(emu.marginal.any(-1)[..., None].expand_as(emu.o))
        r = torch.where(rows, torch.minimum(r, r2), r)
    return r


def lse_ratios(got, emu: Fwd, alt: Optional[Fwd] = None):
    """got [B * H, Nq] -> |got - emu| / (LSE_REL (|emu| + 1)) per row; a row with a marginal decision against the nearer of the two."""
    def one(e):
        want = e.lse.reshape(got.shape)
        r = (got.double() - want).abs() / (LSE_REL * (want.abs() + 1))
        return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    r = one(emu)
    if alt is not None:
        r = torch.where(emu.marginal.any(-1).reshape(got.shape), torch.minimum(r, one(alt)), r)
    return r


def bias(got, want, A):
    """T: the mean over all elements of (got - want) / A."""
    return float(((got.double() - want) / A).mean())


def lazy_pair(case: Case, prescaled=False):
    """(emulation, the emulation with every marginal move_ref decision inverted or None, share of rows with a marginal decision)."""
    emu = emulate_lazy(case, prescaled=prescaled)
    rows = emu.marginal.any(-1)
    alt = emulate_lazy(case, prescaled=prescaled, flip=emu.marginal) if bool(rows.any()) else None
    return emu, alt, float(rows.double().mean())


# ---- the backward ------------------------------------------------------------------------------------------------------------------------

BWD_FAULTS = ("p_trunc", "p_away", "ds_trunc", "ds_from_bf16_p", "delta_exact_o", "out_trunc")


@dataclass
class Bwd:
    dq: torch.Tensor      # [B, H, Nq, D] in front of the output rounding
    dk: torch.Tensor
    dv: torch.Tensor
    F_dq: torch.Tensor
    F_dk: torch.Tensor
    F_dv: torch.Tensor
    flagged_p: float = 0.0
    flagged_ds: float = 0.0
    P: Optional[torch.Tensor] = None      # in front of their roundings, with the error bounds their flags use (relative for P, absolute for dS)
    dS: Optional[torch.Tensor] = None
    tau_p: Optional[torch.Tensor] = None
    err_ds: Optional[torch.Tensor] = None

    def outs(self, fault=None):
        return tuple(rnd(flat(x), "trunc" if fault == "out_trunc" else "rne") for x in (self.dq, self.dk, self.dv))


@dataclass
class BwdRef:
    o: torch.Tensor       # [B, H, Nq, D] bf16 values: the forward's output as the host hands it over
    lse: torch.Tensor     # [B, H, Nq] fp32 values
    dv: torch.Tensor      # float64, no rounding at all
    A_dq: torch.Tensor    # scale sum_k P (|dO| . |v_k| + |dO| . |o|) |k_kd|
    A_dk: torch.Tensor
    A_dv: torch.Tensor    # sum_i P |dO_id|


@functools.lru_cache(maxsize=4)
def _bwd_ref(sp: Spec) -> BwdRef:
    case = make_case(sp)
    ex = exact(case)
    o = bf(ex.out.float()).double()
    mag = ex.p * (torch.matmul(case.do.abs(), case.v.abs().transpose(-1, -2)) + (case.do.abs() * o.abs()).sum(-1, keepdim=True))
    return BwdRef(o, ex.lse.float().double(), torch.matmul(ex.p.transpose(-1, -2), case.do), torch.matmul(mag, case.k.abs()) * SCALE,
                  torch.matmul(mag.transpose(-1, -2), case.q.abs()) * SCALE, torch.matmul(ex.p.transpose(-1, -2), case.do.abs()))


def bwd_ref(case: Case) -> BwdRef:
    return _bwd_ref(case.spec)


def emulate_bwd(case: Case, fault=None, f32=False, order=0) -> Bwd:
    """Both roles of attn_bwd_kernel (they form P and dS alike; delta of the stand-alone kernel is the same sum)."""
    g = bwd_ref(case)
    q, k, v, do = case.q, case.k, case.v, case.do
    o = exact(case).out if fault == "delta_exact_o" else g.o
    lse2 = R(g.lse * float(LOG2E_F32), f32)
    s, sa = scores(q, k, f32, order)
    x = R(s * C - lse2[..., None], f32)
    P = exp2(x, f32)
    delta = rowsum(R(do * o, f32), f32, order)
    dP = mm(do, v.transpose(-1, -2), f32, order)
    Pb = rnd(P, P_MODE.get(fault, "rne"))
    dS = R((Pb if fault == "ds_from_bf16_p" else P) * R(dP - delta[..., None], f32), f32)
    dSb = rnd(dS, "trunc" if fault == "ds_trunc" else "rne")
    sc = float(np.float32(SCALE))
    dq = R(mm(dSb, k, f32, order) * sc, f32)
    dk = R(mm(dSb.transpose(-1, -2), q, f32, order) * sc, f32)
    dv = mm(Pb.transpose(-1, -2), do, f32, order)
    tp = tau(sa * C, x)
    fp, up = near_midpoint(P, tp * P)
    err = P * C_D * (torch.matmul(do.abs(), v.abs().transpose(-1, -2)) + (do.abs() * o.abs()).sum(-1, keepdim=True)) + tp * dS.abs()
    fs, us = near_midpoint(dS, err)
    w = fs * us
    return Bwd(dq, dk, dv, torch.matmul(w, k.abs()) * sc, torch.matmul(w.transpose(-1, -2), q.abs()) * sc, torch.matmul((fp * up).transpose(-1, -2), do.abs()),
               float(fp.double().mean()), float(fs.double().mean()), P, dS, tp, err)


def bwd_faults_for(sp: Spec):
    """delta_exact_o is removed on the spread family: on flat rows dP - delta is carried by dP, and the 2^-9 |o| that the rounding of o moves
    delta by stays below the rounding of dS."""
    return [f for f in BWD_FAULTS if not (f == "delta_exact_o" and sp.family == "spread")]


def bwd_ratios(got, emu: Bwd, g: BwdRef):
    """got: (dq, dk, dv) [B, N, H * D], any of them None.  -> the per-element ratios of those given."""
    pairs = ((emu.dq, g.A_dq, emu.F_dq), (emu.dk, g.A_dk, emu.F_dk), (emu.dv, g.A_dv, emu.F_dv))
    return tuple(None if x is None else ratios(x, flat(e), flat(A), flat(F)) for x, (e, A, F) in zip(got, pairs))


# ---- the case lists of the GPU tests -------------------------------------------------------------------------------------------------------

ROW_NK = (24, 64, 77)                                    # NKB 1, 2, 3
ROW_NQ = 160
QPROJ_NK = (40, 77, 96)
QPROJ_NQ, QPROJ_N, QPROJ_K = 256, 128, 128
EAGER_SHAPES = ((200, 97), (200, 200), (200, 333))       # (Nq, Nk)
LAZY_SHAPE = (512, 256)                                  # B H = 2
SINGLE = ((256, 128), (512, 128), (1024, 128), (512, 512))   # (N, head dim): 1, 2, 4 and 2 splits
SINGLE_SPLITS = {256: 1, 512: 2, 1024: 4}
BWD_SHAPES = ((128, 128), (200, 77), (256, 333))


def row_spec(family, nk, nq=ROW_NQ, dup=0):
    return Spec(family, nq, nk, dup=dup)


def eager_spec(family, nq, nk):
    return Spec(family, nq, nk)


def lazy_spec(family):
    return Spec(family, LAZY_SHAPE[0], LAZY_SHAPE[1], B=1, H=2)


def single_spec(family, n, d):
    return Spec(family, n, n, B=1, H=1, D=d)


def bwd_spec(family, nq, nk):
    return Spec(family, nq, nk, B=1, H=2)


def selection(n=QPROJ_N, kdim=QPROJ_K):
    """The signed selection of attn_grid_cases as a projection weight: row j of W [n, kdim] holds sigma(j) at column pi(j), so that
    a[..., pi] = sigma q gives a W^T = q exactly.  -> (W, pi, sigma)"""
    j = np.arange(n)
    pi = (5 * j + 3) % kdim
    sigma = np.where(j % 3 == 1, -1.0, 1.0)
    assert len(set(pi.tolist())) == n
    w = np.zeros((n, kdim))
    w[j, pi] = sigma
    return torch.from_numpy(w), torch.from_numpy(pi), torch.from_numpy(sigma)


def all_bwd_specs():
    return [bwd_spec(f, nq, nk) for f in FAMILIES for nq, nk in BWD_SHAPES]


def all_forward_specs():
    """(pipeline, spec) of every forward case the GPU file runs, once."""
    out = []
    for f in FAMILIES:
        out += [("row", row_spec(f, nk)) for nk in ROW_NK]
        out += [("row", row_spec(f, nk, QPROJ_NQ, dup)) for nk in QPROJ_NK for dup in (0, 1)]
        out += [("eager", eager_spec(f, nq, nk)) for nq, nk in EAGER_SHAPES]
        out += [("lazy", lazy_spec(f))]
        out += [("single", single_spec(f, n, d)) for n, d in SINGLE]
    return out
