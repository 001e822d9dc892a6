"""Per-element cases for the fused q projection + attention (cd360_qproj_attn_dedup_bf16, csrc/gemm8p.hip) on DENSE weights, at the real
K, with bias, the LayerNorm fold and the split launch (CPU only, no HIP import; tests/test_qproj_cases_cpu.py checks the method,
tests/test_qproj_exact_gpu.py runs the kernels).  The exact and off-grid attention suites reach this kernel only behind a signed
selection matrix at N = K = 128; here the projection itself is under test, and integer operands make it exact (the method of gemm_cases):

  a holds integers, W integers times one power of two 2^-j per case (both lossless in bf16), the bias integers times 2^-j in fp32, and the
  builder asserts sum |a| |w| + |bias| < 2^24 per element in units of 2^-j.  Every partial sum is then exact in fp32 in ANY order -- through
  any tile, ring slot, wave group or mover schedule --, t = a W^T + bias has one right value and q = bf16(t) is one round-to-nearest-even.
  2^-j is chosen per K so that q has its ordinary size (std about 1 on the spread family, about 3 on peaked and positive), and the row
  pipeline of attn_round_cases (emulate_row, exact_of, the flip allowance F for P, the bias statistic T) applies unchanged at SCALE = 1 / 8.

Family A: bias, no LayerNorm: q exact.  The builder asserts that >= 10 % of the q elements change under the bf16 rounding and >= 2 % are
exact ties (round-half-even is decided), that every 8-column bias slice and every K tile of a and W differs from its neighbours.

Family B: the LayerNorm fold of the attention epilogue, t = fma(acc, rstd, fma(-rstd mean, wsum, bias)), with ln_stats the exact integer
(sum, sum of squares) of the rows in 1 or K / 128 partials and ln_eps = 1e-5.  acc stays exact; mean, rstd and the two fmas round in
fp32, so q is judged with a flip allowance of its own: with

    unit = C_T [ |r (acc - mu wsum)| (4 + 2 kappa) + 3 |r mu wsum| + |r mu wsum - bias| + |t| ],   kappa = (ss / K + mu^2) / (var + eps)

(the places an fp32 rounding enters, each with the number of roundings it sees: rstd -- the sum var + eps, rsqrtf and its +-1 ulp, and ss inv,
mean and mean^2, which the cancellation in ss / K - mu^2 amplifies by kappa --; mean, 1.f / ln_dim and a_c2 = -rstd mean; the inner
fma; the outer fma), a q element whose float64 t lies within `unit` of a bf16 midpoint is FLAGGED, and the
bar of its (token, head) row grows by the first-order effect of that element moving one bf16 spacing, times two for the second order:

    Fq_e = 2 sum_d flagged ulp(q_d) c ln 2 sum_j p_j |k_jd| (|v_je| + |o_e|)

(|v_j| + |o| and not |v_j - o|: the numerator sums the ROUNDED P, which stands still while q_d moves unless a P flips, and the denominator
the fp32 p, which follows at once, so the first-order cancellation between the two does not happen element by element)

and, since the moved q_d moves every p_j of the row by the relative ln 2 c ulp(q_d) (|k_jd| + max_j |k_jd|) -- thousands of times tau --,
that much is added to tau for the row's P flags (attn_round_cases._tiled, tau_extra): most of such a row's P may round either way, and
where the shift exceeds a spacing of p every midpoint it reaches counts.  (The first statement of this model had |v_j - o| and left the P flags out; the fp32 restatement itself then missed the bar by up to 29
times on the rows with a flagged q, so the model was corrected on the CPU.)  The rows with a flagged q are reported as rows_q.

C_T is the smallest power of two at which the fp32 restatement of the source's expression order -- 1.f / ln_dim, ss inv - mean^2 plain and
contracted either way, rsqrtf at +-1 ulp, the two fmas -- stays within HALF of unit on every case (fixed on the CPU, never against the
kernel).  The builder asserts flagged q <= 0.5 % per case.  Rows are plain (|mean| / std <= 1) or offset (ratio about 16-20, where
ss / K - mean^2 cancels); in one case wsum is deliberately NOT sum_k W (the reference uses the one given).

The bar, per output element, nothing excluded:  |got - emu| <= 2^-8 |emu| + EPS A + F + Fq, and on the positive family |T| <= |T_trunc| / 4.
K, V: bf16 randn, rows >= Nk NaN on the device; a carries NaN rows behind its M rows."""
import functools
import math
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np
import torch

import attn_round_cases as RC

KT = 64                    # the K tile of every tiling
LN_EPS = float(np.float32(1e-5))
C_T = 2.0 ** -23           # fixed by tests/test_qproj_cases_cpu.py::test_fp32_restatements
FLAG_CAP_Q = 0.005
BQ = 2                     # query batch elements; the output has BQ + dup
W_LO, W_HI = 3, 15
OFFSET_EVERY = 32
TARGET = {"spread": 1.0, "peaked": 3.0, "positive": 3.0}

# qattn_cfg -> (WM, WN, NCB, NMB, NBUF, mover waves): launch_epi<...> of qattn_launch; movers as launch_ks decides them by default
TILES = {1: (2, 4, 2, 4, 2, 0), 2: (4, 2, 2, 1, 4, 4), 3: (2, 2, 2, 2, 2, 0), 4: (4, 2, 2, 2, 2, 0)}
NK_EPI = ((20, 2), (40, 3), (77, 7), (96, 4))     # Nk and the epilogue it is named for (77 with qattn_keys16 = 0: EPI 4)


def inst_name(cfg, epi):
    wm, wn, ncb, nmb, nbuf, mv = TILES[cfg]
    return f"epi<{wm},{wn},{ncb},{nmb},{nbuf},E{epi}>" + ("+mv" if mv else "")


@dataclass(frozen=True)
class Data:
    """What the emulation depends on."""
    kind: str                 # "A" | "B"
    family: str               # spread | peaked | positive
    K: int
    N: int
    Nk: int
    Nq: int = 256
    dup: int = 0
    amax: int = 7             # a in -amax .. amax (family A; B: see rows)
    rows: str = "-"           # B: plain | offset
    parts: int = 1
    free_wsum: bool = False

    @property
    def H(self):
        return self.N // 64

    @property
    def M(self):
        return BQ * self.Nq


@dataclass(frozen=True)
class Launch:
    data: Data
    cfg: int
    split: int = 0
    keys16: Optional[int] = None      # None: the default (on)
    inst: tuple = ()                  # the instantiations the launch is named for, in launch order


def data_id(d: Data) -> str:
    s = f"{d.kind}-{d.family}-k{d.K}n{d.N}-{d.Nq}x{d.Nk}-a{d.amax}"
    if d.kind == "B":
        s += f"-{d.rows}-parts{d.parts}" + ("-freewsum" if d.free_wsum else "")
    return s + ("-dup" if d.dup else "")


def launch_id(l: Launch) -> str:
    return f"{data_id(l.data)}-qcfg{l.cfg}" + ("-split" if l.split else "") + ("-keys16off" if l.keys16 == 0 else "")


# ---- the dispatch of cd360_qproj_attn_dedup_bf16 and qattn_launch, restated ---------------------------------------------------------------

def epi_of(nk, keys16=True):
    if nk <= 32:
        return 2
    if nk <= 64:
        return 3
    return 7 if nk <= 80 and keys16 else 4


def route(M, N, Nq, Nk, cfg, split=0, keys16=None):
    """-> [(instantiation, first column, columns)] in launch order, or None where the entry refuses the shape."""
    if N % 64 or Nk > 96 or Nq % 128 or M % Nq:
        return None
    if cfg < 1 or cfg > 4:
        cfg = 1 if (M // 256) * ((N + 255) // 256) >= 200 else (4 if (M // 256) * ((N + 127) // 128) >= 200 else 2)
    if Nq % 256 and cfg in (1, 4):
        cfg = 2
    e = epi_of(Nk, keys16 != 0)
    if cfg == 1 and N > 256 and N % 256 == 128 and split > 0:
        return [(inst_name(1, e), 0, N - 128), (inst_name(4, e), N - 128, 128)]
    return [(inst_name(cfg, e), 0, N)]


def forced_ok(d: Data, cfg):
    """The forced tile is the one that runs (256-token tiles need Nq % 256 == 0)."""
    return not (d.Nq % 256 and cfg in (1, 4))


# ---- builders ------------------------------------------------------------------------------------------------------------------------------

@dataclass
class Built:
    d: Data
    j: int
    a: torch.Tensor            # [BQ, Nq, K] float64 integers
    a_beyond: torch.Tensor     # [Nq, K]: what a kernel that read rows >= M as data would see (the device holds NaN there)
    w: torch.Tensor            # [N, K] integers times 2^-j
    bias: torch.Tensor         # [N]
    wsum: Optional[torch.Tensor]
    stats: Optional[torch.Tensor]    # [M, parts, 2]
    k: torch.Tensor            # [BQ + dup, H, Nk, 64]
    v: torch.Tensor
    t: torch.Tensor            # [BQ, Nq, N] float64, in front of the bf16 rounding
    unit: Optional[torch.Tensor]
    rounded: float = 0.0
    ties: float = 0.0


def _gen(d: Data, salt=0):
    h = 17
    for s in (d.K, d.N, d.Nk, d.Nq, d.dup, d.amax, d.parts, len(d.rows), ord(d.kind), ord(d.family[1]), int(d.free_wsum), salt):
        h = (h * 1000003 + int(s)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _rows(d: Data, g, n):
    """[n, Nq, K] integer rows."""
    if d.kind == "A":
        return _ints(g, (n, d.Nq, d.K), -d.amax, d.amax)
    # plain: noise -7 .. 7 (std 4.3) around an offset of 1 .. 2: |mean| / std about 0.2 .. 0.5, not centred
    x = _ints(g, (n, d.Nq, d.K), -7, 7) + _ints(g, (n, d.Nq, 1), 1, 2) * (_ints(g, (n, d.Nq, 1), 0, 1) * 2 - 1)
    if d.rows == "plain":
        return x
    assert d.rows == "offset"  # one row in OFFSET_EVERY (see offset_rows): noise -2 .. 2 (std 1.41) around an offset of 23 .. 28, ratio 16 .. 20
    off = _ints(g, (n, d.Nq, 1), 23, 28) * (_ints(g, (n, d.Nq, 1), 0, 1) * 2 - 1)
    return torch.where(offset_rows(d, n)[..., None], _ints(g, (n, d.Nq, d.K), -2, 2) + off, x)


def offset_rows(d: Data, n=BQ):
    """Boolean [n, Nq]: the offset rows of an "offset" case, one in OFFSET_EVERY at a position that walks through the 32 rows of a wave's block
    (row 32 i + (5 i) % 32).  Only so many: the cancellation in ss / K - mean^2 leaves rstd -- and with it every q element of
    the row -- uncertain by about 2^-14 relative, which flags several per cent of such a row against the cap of 0.5 % per case."""
    i = torch.arange(d.Nq)
    return ((i % OFFSET_EVERY) == (5 * (i // OFFSET_EVERY)) % OFFSET_EVERY)[None].expand(n, d.Nq)


def tiles(x):
    """[..., K] -> the list of its 64-wide K tiles."""
    return list(x.split(KT, -1))


def fold_terms(b_or_stats, K, parts_used=None):
    """(mean, var, rstd, ss / K) in float64 from the partial sums [M, parts, 2]."""
    st = b_or_stats if parts_used is None else b_or_stats[:, :parts_used]
    s, ss = st[..., 0].sum(-1), st[..., 1].sum(-1)
    mean = s / K
    var = (ss / K - mean * mean).clamp_min(0)
    return mean, var, 1.0 / torch.sqrt(var + LN_EPS), ss / K


def finish(d: Data, acc, bias, wsum, stats, fault=None):
    """float64 t [BQ, Nq, N] from the exact acc."""
    if d.kind == "A":
        return acc + bias
    mean, var, rstd, _ = fold_terms(stats, d.K, 1 if fault == "parts_first" else None)
    if fault in ("stats_next_row", "stats_row128"):
        sh = -1 if fault == "stats_next_row" else -128
        mean, rstd = mean.roll(sh, 0), rstd.roll(sh, 0)
    mean, rstd = mean.reshape(BQ, d.Nq, 1), rstd.reshape(BQ, d.Nq, 1)
    c2 = rstd * mean if fault == "c2_sign" else -rstd * mean
    return acc * rstd + (c2 * wsum + bias)


def fold_unit(d: Data, acc, bias, wsum, stats):
    mean, var, rstd, m2 = fold_terms(stats, d.K)
    kappa = (m2 + mean * mean) / (var + LN_EPS)
    mean, rstd, kappa = (x.reshape(BQ, d.Nq, 1) for x in (mean, rstd, kappa))
    t = acc * rstd + (-rstd * mean * wsum + bias)
    inner = -rstd * mean * wsum + bias
    return C_T * ((rstd * (acc - mean * wsum)).abs() * (4 + 2 * kappa) + 3 * (rstd * mean * wsum).abs() + inner.abs() + t.abs())


def finish_f32(d: Data, acc, bias, wsum, stats, variant=0, ulp=0):
    """The fold in fp32 in the source's expression order (gemm8p.hip: a_c1 = rstd, a_c2 = -rstd * mean; t = fmaf(acc, a_c1, fmaf(a_c2,
    wsum, bias))).  variant: ss * inv - mean * mean 0 = two roundings, 1 = fma(ss, inv, -(mean * mean)), 2 = fma(-mean, mean, ss * inv);
    ulp: rsqrtf moved by that many fp32 ulps.  (A float64 product of two fp32 values is exact, so rounding a float64 a * b + c to fp32 is
    the fused operation up to a double rounding of relative size 2^-53.)"""
    f = lambda x: x.float().double()
    if d.kind == "A":
        return acc + bias
    inv = f(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(d.K), dtype=torch.float32))
    s, ss = stats[..., 0].sum(-1), stats[..., 1].sum(-1)      # exact integers below 2^24
    mean = f(s * inv)
    if variant == 0:
        var = f(f(ss * inv) - f(mean * mean))
    elif variant == 1:
        var = f(ss * inv - f(mean * mean))
    else:
        var = f(f(ss * inv) - mean * mean)
    rstd = f(1.0 / torch.sqrt(f(var.clamp_min(0) + f(torch.tensor(LN_EPS, dtype=torch.float64)))))
    rstd = f(rstd * (1.0 + ulp * 2.0 ** -23))
    c1, c2 = rstd.reshape(BQ, d.Nq, 1), f(-rstd * mean).reshape(BQ, d.Nq, 1)
    return f(acc * c1 + f(c2 * wsum + bias))


def accumulate(a, w, fault=None, nbuf=2):
    """a W^T tile by tile; exact whatever the order, so the faults are the only thing the tiles are kept apart for."""
    at, wt = tiles(a), tiles(w)
    nt = len(at)
    acc = a.new_zeros(a.shape[:-1] + (w.shape[0],))
    for t in range(nt):
        if fault == "skip_last" and t == nt - 1:
            continue
        src = t - nbuf if fault == "stale_slot" and t == nt - 1 else t
        acc = acc + at[src] @ wt[src].T
        if fault == "tile_twice" and t == nt // 2:
            acc = acc + at[t] @ wt[t].T
    if fault == "k_drop":       # one k index of tile 2 lost in the 32 x 32 block of tokens 32 .. 63 (batch 0), channels 32 .. 63
        kk = 2 * KT + 37
        acc[0, 32:64, 32:64] -= a[0, 32:64, kk, None] * w[None, 32:64, kk]
    return acc


def _j_for(d: Data, a_rms):
    std = a_rms * math.sqrt((W_LO + W_HI) ** 2 / 4 + ((W_HI - W_LO + 1) ** 2 - 1) / 12) * math.sqrt(d.K)
    return round(math.log2(std / TARGET[d.family]))


@functools.lru_cache(maxsize=3)
def build(d: Data) -> Built:
    assert d.kind in "AB" and d.family in RC.FAMILIES and d.K % KT == 0 and d.N % 64 == 0 and d.dup in (0, 1)
    g = _gen(d)
    a = _rows(d, g, BQ + 1)
    a, a_beyond = a[:BQ], a[BQ]
    wi = _ints(g, (d.N, d.K), W_LO, W_HI) * (_ints(g, (d.N, d.K), 0, 1) * 2 - 1)
    # B: t is the projection of the NORMALISED rows (unit variance), A: of a itself
    j = _j_for(d, 1.0 if d.kind == "B" else math.sqrt(((2 * d.amax + 1) ** 2 - 1) / 12))
    u = 2.0 ** -j
    bi = _ints(g, (d.N,), -2 ** j, 2 ** j)                  # |bias| <= 1
    w, bias = wi * u, bi * u
    assert torch.equal(RC.bf(a), a) and torch.equal(RC.bf(w), w) and torch.equal(bias.float().double(), bias)
    exact_cond = a.abs() @ wi.abs().T + bi.abs()
    assert float(exact_cond.max()) < 2 ** 24, "a partial sum may leave the fp32 integers"
    # distinct neighbours: 8-column bias slices, K tiles of W and of a
    bs = bias.reshape(-1, 8)
    assert bool((bs[1:] != bs[:-1]).any(-1).all()) and not torch.equal(bias, bias.roll(64))
    for x in (w, a.reshape(-1, d.K)):
        tl = tiles(x)
        assert all(not torch.equal(p, q) for p, q in zip(tl[1:], tl[:-1]))
    acc = a @ w.T
    wsum = stats = unit = None
    if d.kind == "B":
        wsum = w.sum(-1)
        if d.free_wsum:      # not sum_k W: the neighbouring 8-column slice's values, doubled
            wsum = 2 * wsum.roll(8)
        assert torch.equal(wsum.float().double(), wsum)
        assert d.K % d.parts == 0
        ap = a.reshape(d.M, d.parts, d.K // d.parts)
        stats = torch.stack([ap.sum(-1), (ap * ap).sum(-1)], -1)
        assert float(stats.sum(1).max()) < 2 ** 24
        mean, var, _, _ = fold_terms(stats, d.K)
        ratio = mean.abs() / var.sqrt()
        off = offset_rows(d).reshape(-1) if d.rows == "offset" else torch.zeros(d.M, dtype=torch.bool)
        assert float(ratio[~off].max()) <= 1.0 and float(ratio[~off].mean()) > 0.2, "plain rows: |mean| / std <= 1"
        assert not bool(off.any()) or (14.0 <= float(ratio[off].min()) and float(ratio[off].max()) <= 24.0), "offset rows: |mean| / std about 16 .. 20"
        unit = fold_unit(d, acc, bias, wsum, stats)
    t = finish(d, acc, bias, wsum, stats)
    q = RC.rnd(t)
    rounded = float((q != t).double().mean())
    y, _ = RC.grid(t)
    ties = float(((y.abs() - y.abs().floor()) == 0.5).double().mean())
    if d.kind == "A":
        assert rounded >= 0.10, f"only {rounded:.3f} of q changes under the bf16 rounding"
        assert ties >= 0.02, f"only {ties:.3f} of q are ties"
    gk = _gen(d, 1)
    r = lambda: RC.bf(torch.randn(BQ + d.dup, d.H, d.Nk, 64, generator=gk, dtype=torch.float32)).double()
    k, v = r(), r()
    if d.family == "positive":
        v = RC.bf(v.abs() + 0.5)
    return Built(d, j, a, a_beyond, w, bias, wsum, stats, k, v, t, unit, rounded, ties)


# ---- the chain: projection -> q -> the row pipeline ---------------------------------------------------------------------------------------

Q_FAULTS = ("k_drop", "stale_slot2", "stale_slot4", "skip_last", "tile_twice", "bias_shift8", "bias_head", "wsum_head", "stats_next_row", "stats_row128",
            "c2_sign", "parts_first", "q_trunc", "q_after_scale", "split_cols0", "dup_first_keys", "rows_beyond_m")


def project(b: Built, fault=None, f32=None):
    """t [BQ, Nq, N] in front of its rounding.  f32 = (variant, ulp): the fp32 restatement of the fold."""
    d = b.d
    bias, wsum = b.bias, b.wsum
    if fault == "bias_shift8":
        bias = bias.roll(-8)
    if fault == "bias_head":
        bias = bias.roll(-64)
    if fault == "wsum_head":
        wsum = wsum.roll(-64)
    if fault == "split_cols0":
        bias = torch.cat([bias[:-128], bias[:128]])
        wsum = None if wsum is None else torch.cat([wsum[:-128], wsum[:128]])
    mm_fault = {"stale_slot2": "stale_slot", "stale_slot4": "stale_slot"}.get(fault, fault)
    acc = accumulate(b.a, b.w, mm_fault, 4 if fault == "stale_slot4" else 2)
    if f32 is not None:
        return finish_f32(d, acc, bias, wsum, b.stats, *f32)
    return finish(d, acc, bias, wsum, b.stats, fault)


def q_of(b: Built, t, fault=None):
    """The bf16 q as the epilogue's MFMA takes it, [BQ + dup, H, Nq, 64]."""
    d = b.d
    if fault == "q_trunc":
        q = RC.rnd(t, "trunc")
    elif fault == "q_after_scale":
        q = RC.rnd(t * RC.C) / RC.C
    else:
        q = RC.rnd(t)
    q = RC.heads(q, d.H)
    if d.dup:
        extra = q[BQ - d.dup:]
        if fault == "rows_beyond_m":
            extra = RC.heads(RC.rnd(project(replace_rows(b), None))[:1], d.H)
        q = torch.cat([q, extra])
    return q


def replace_rows(b: Built) -> Built:
    """b with query batch 0 replaced by the rows behind M (and, family B, their statistics)."""
    d = b.d
    a = torch.stack([b.a_beyond, b.a[1]])
    stats = b.stats
    if stats is not None:
        ap = a.reshape(d.M, d.parts, d.K // d.parts)
        stats = torch.stack([ap.sum(-1), (ap * ap).sum(-1)], -1)
    return replace(b, a=a, stats=stats)


def case_of(b: Built, t, fault=None) -> RC.Case:
    d = b.d
    k, v = b.k, b.v
    if fault == "split_cols0":
        k, v = (torch.cat([x[:, :-2], x[:, :2]], 1) for x in (k, v))
    if fault == "dup_first_keys":
        k, v = (torch.cat([x[:BQ], x[BQ - d.dup:BQ]]) for x in (k, v))
    sp = RC.Spec(d.family, d.Nq, d.Nk, B=BQ + d.dup, H=d.H, dup=d.dup)
    return RC.Case(sp, q_of(b, t, fault), k, v, None)


def q_flip_allowance(flag, u, ex: RC.Exact, k, v):
    """Fq [B, H, Nq, 64]: per flagged (row, d) the first-order effect of q_d moving one bf16 spacing, times two."""
    Fq = torch.zeros_like(ex.out)
    idx = flag.nonzero()
    for ch in idx.split(256):
        bi, hi, ii, di = ch.unbind(1)
        wgt = ex.p[bi, hi, ii] * k[bi, hi, :, di].abs()                             # [n, Nk]
        dv = v[bi, hi].abs() + ex.out[bi, hi, ii][:, None, :].abs()                 # [n, Nk, 64]
        c = 2.0 * u[bi, hi, ii, di, None] * (RC.C * math.log(2.0)) * (wgt[:, :, None] * dv).sum(1)
        Fq.index_put_((bi, hi, ii), c, accumulate=True)
    return Fq


@dataclass
class Emu:
    b: Built
    case: RC.Case
    ex: RC.Exact
    fwd: RC.Fwd
    F: torch.Tensor            # F of P plus Fq, [B, H, Nq, 64]
    flagged_q: float
    t_trunc: Optional[float]
    flagged_p: float = 0.0     # by tau alone, as attn_round_cases counts it
    rows_q: float = 0.0        # share of the (token, head) rows with a flagged q element: their P may round either way


@functools.lru_cache(maxsize=3)
def emulate(d: Data) -> Emu:
    b = build(d)
    case = case_of(b, b.t)
    ex = RC.exact_of(case.q, case.k, case.v)
    fwd = RC.emulate_row(case)
    F, fq, fp, rows_q = fwd.F, 0.0, fwd.flagged, 0.0
    if d.kind == "B":
        flag, u = RC.near_midpoint(b.t, b.unit)
        fq = float(flag.double().mean())
        assert fq <= FLAG_CAP_Q, f"{fq:.4f} of the q elements lie within their unit of a bf16 midpoint"
        fl, uu = RC.heads(flag, d.H), RC.heads(u, d.H)
        if d.dup:
            fl, uu = torch.cat([fl, fl[BQ - d.dup:]]), torch.cat([uu, uu[BQ - d.dup:]])
        rows_q = float(fl.any(-1).double().mean())
        # a flagged q_d that moves by its spacing moves x_j by c ulp |k_jd| and the row maximum by no more than the largest of these: the
        # P of that row within that distance of a midpoint may round the other way too
        dx = RC.C * torch.matmul(fl * uu, case.k.abs().transpose(-1, -2))
        fwd = RC.emulate_row(case, tau_extra=math.log(2.0) * (dx + dx.amax(-1, keepdim=True)))
        F = fwd.F + q_flip_allowance(fl, uu, ex, case.k, case.v)
    t_trunc = None
    if d.family == "positive":
        t_trunc = RC.bias(RC.emulate_row(case, "p_trunc").out(), RC.flat(ex.out), RC.flat(ex.A))
    return Emu(b, case, ex, fwd, F, fq, t_trunc, fp, rows_q)


def ratios(got, e: Emu):
    """got [BQ + dup, Nq, N] -> |got - emu| / (2^-8 |emu| + EPS A + F + Fq) per element."""
    return RC.ratios(got, RC.flat(e.fwd.o), RC.flat(e.ex.A), RC.flat(e.F))


def faulty_out(e: Emu, fault):
    """The emulation's output [BQ + dup, Nq, N] under a fault model."""
    b = e.b
    t = project(b, fault)
    return RC.emulate_row(case_of(b, t, fault)).out()


def region(d: Data, fault):
    """Boolean [BQ + dup, Nq, N]: the outputs the fault touches."""
    m = torch.zeros(BQ + d.dup, d.Nq, d.N, dtype=torch.bool)
    if fault == "k_drop":
        m[0, 32:64, 0:64] = True
    elif fault == "split_cols0":
        m[..., -128:] = True
    elif fault in ("dup_first_keys", "rows_beyond_m"):
        m[BQ:] = True
    else:
        m[:] = True
    return m


def faults_for(d: Data):
    """The fault models a case must expose on >= 10 % of the elements of the region touched, or through T.  Removed where they cannot
    occur, by the properties of the case and not by what a run gives:
      k_drop, stale_slot2 / 4   need a K tile beyond the second / more tiles than ring slots (K >= 192 / 192 / 320)
      wsum_head, stats_*, c2_sign   the fold only; parts_first: more than one partial
      split_cols0   widths the split launch serves (N > 256, N % 256 == 128)
      dup_first_keys, rows_beyond_m   dup = 1
      q_trunc, q_after_scale   on the positive family: every term of a row has the same sign and A = |o|, the widest bar against the spread
                    of v.  Rounding q c goes up as often as down, and a q truncated towards zero flattens the softmax, which moves o
                    towards the row's mean v -- up on one channel, down on the next --, so T does not answer either (as q_* in
                    attn_round_cases)."""
    nt = d.K // KT
    f = ["skip_last", "tile_twice", "bias_shift8", "bias_head"]
    if d.family != "positive":
        f += ["q_trunc", "q_after_scale"]
    if nt >= 3:
        f += ["k_drop", "stale_slot2"]
    if nt >= 5:
        f.append("stale_slot4")
    if d.kind == "B":
        f += ["wsum_head", "stats_next_row", "stats_row128", "c2_sign"] + (["parts_first"] if d.parts > 1 else [])
    if d.N > 256 and d.N % 256 == 128:
        f.append("split_cols0")
    if d.dup:
        f += ["dup_first_keys", "rows_beyond_m"]
    return f


# ---- the covering list ----------------------------------------------------------------------------------------------------------------------

def _data_cases(kind):
    """Few data cases, each run on several launches: the float64 emulation is computed once per data case."""
    fam = ("spread", "peaked", "positive")
    out = []
    i = 0
    for K in (64, 1280):
        for nk, _ in NK_EPI:
            kw = dict(amax=7 if i % 2 else 15)
            if kind == "B":
                kw = dict(rows="offset" if i % 2 else "plain", parts=(K // 128 if K >= 128 and i % 4 < 2 else 1))
            out.append(Data(kind, fam[i % 3], K, 128, nk, **kw))
            i += 1
    b = (lambda rows, parts, **kw: dict(rows=rows, parts=parts, **kw)) if kind == "B" else (lambda rows, parts, **kw: {})
    out.append(Data(kind, "peaked", 192, 384, 77, **b("offset", 1)))
    out.append(Data(kind, "spread", 640, 640, 77, amax=15 if kind == "A" else 7, **b("plain", 5, free_wsum=True)))
    out.append(Data(kind, "positive", 640, 128, 40, dup=1, **b("offset", 5)))
    out.append(Data(kind, "spread", 192, 128, 96, Nq=384, **b("plain", 1)))
    return out


def launches(kind):
    out = []
    for d in _data_cases(kind):
        e = dict(NK_EPI)[d.Nk]
        for cfg in (1, 2, 3, 4):
            if not forced_ok(d, cfg):
                continue      # a forced tile that the shape cannot take is never run under that name
            out.append(Launch(d, cfg, inst=(inst_name(cfg, e),)))
            if cfg == 1 and d.N > 256 and d.N % 256 == 128:
                out.append(Launch(d, 1, split=1, inst=(inst_name(1, e), inst_name(4, e))))
            if d.K == 64 and d.Nk == 77:
                out.append(Launch(d, cfg, keys16=0, inst=(inst_name(cfg, 4),)))
    return out
