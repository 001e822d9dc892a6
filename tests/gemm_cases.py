"""Exact-integer inputs for the MFMA GEMM family (cd360_gemm_bf16, cd360_gemm_cstats_bf16, cd360_gemm_tn_bf16, cd360_lowrank_add_bf16)
with a float64 reference.  CPU only: nothing here imports the HIP library.

The method.  bf16 holds every integer of magnitude <= 256 exactly.  With integer operands every product is an integer and so is every
partial sum, whatever the order (MFMA k-steps, wave groups, k-split partial tiles exchanged through the LDS, TN slabs); while every such
integer stays below 2^24 the fp32 accumulator holds it exactly on EVERY schedule.  An integer fp32 bias and an integer bf16 residual keep
acc + bias + res exact, and the only rounding left is the final fp32 -> bf16 round-to-nearest-even, which has one right answer.  So the
expected output is the float64 product, cast to fp32 (exact), cast to bf16 (RNE), and the GPU tests compare with torch.equal.

Every builder asserts the conditions its exactness rests on (`check_*`): operands bf16-representable, sum |a||w| + |bias| + |res| < 2^24,
and for the statistics cases sum |v| < 2^24 and sum v^2 < 2^24 over the STORED (rounded) values of a whole row / a 64-row slab, which
contains every partial any tiling forms.  A builder also makes sure the case is not exact merely because nothing rounds: it walks a
fixed seed sequence until the shares of outputs that need rounding and that are exact ties reach the floors below (the first seed does
for all but the smallest shapes).

`*_faults` restate the reference with one defect each, the ways a kernel of this family goes wrong; tests/test_gemm_cases_cpu.py holds
every case to detecting every defect that applies to it, before any of it runs on a GPU."""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Tuple

import torch

TWO24 = 2 ** 24
BF = torch.bfloat16

# value ranges (inclusive, symmetric): operands, bias, residual
MAIN = dict(a=16, w=8, b=64, r=128)    # every output route; K up to 10240 stays below 2^24 (16 * 8 * 10240 + 192 = 1.3e6)
# K <= 320: row / slab sums of v and v^2 stay below 2^24 (standard deviation 130 .. 150) while a few per cent of the outputs still round
STATS = {False: dict(a=8, w=4, b=64, r=128), True: dict(a=8, w=2, b=64, r=128)}  # by K > 128
MIN_INEXACT, MIN_TIES, MIN_ROUNDING_FAULT = 0.25, 0.05, 0.01  # main family: shares of outputs; rounding defects must move >= 1 %

STATS_MIN_OUTPUTS, MIN_STATS_INEXACT = 1024, 0.01

EPILOGUES = ("none", "bias", "bias_res", "bias_res_stats")


# ---- bf16 rounding, by the bits of the exact fp32 value -----------------------------------------------------------------------------
def exact_f32(x64: torch.Tensor) -> torch.Tensor:
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "not exact in fp32"
    return x32


def rne(x64: torch.Tensor) -> torch.Tensor:
    """float64 -> fp32 (must be exact) -> bf16, round to nearest even."""
    return exact_f32(x64).to(BF)


def truncate(x64: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero): the defect RNE is tested against."""
    bits = exact_f32(x64).contiguous().view(torch.int32)
    return (bits & -65536).view(torch.float32).to(BF)


def low16(x64: torch.Tensor) -> torch.Tensor:
    return exact_f32(x64).contiguous().view(torch.int32) & 0xFFFF


def rounding_shares(x64: torch.Tensor) -> Tuple[float, float, float]:
    """(share not bf16-representable, share exactly halfway between two bf16 values, share where truncation != RNE)."""
    lo = low16(x64)
    n = max(lo.numel(), 1)
    differs = (rne(x64) != truncate(x64))
    return (lo != 0).sum().item() / n, (lo == 0x8000).sum().item() / n, differs.sum().item() / n


def is_bf16(x64: torch.Tensor) -> bool:
    return torch.equal(x64.to(BF).double(), x64)


def _ints(gen: torch.Generator, shape, amp: int) -> torch.Tensor:
    return torch.randint(-amp, amp + 1, shape, generator=gen, dtype=torch.int64).double()


def _seed(*key) -> int:
    return zlib.crc32("-".join(str(k) for k in key).encode())


# ---- cd360_gemm_bf16 / cd360_gemm_cstats_bf16: out = A W^T (+ bias) (+ res) ---------------------------------------------------------------
@dataclass(frozen=True)
class LinearCase:
    family: str
    M: int
    N: int
    K: int
    seed: int
    a: torch.Tensor     # [M, K] float64 integers
    w: torch.Tensor     # [N, K]
    bias: torch.Tensor  # [N]
    res: torch.Tensor   # [M, N]
    acc: torch.Tensor   # [M, N] = a w^T, float64

    def pre(self, epilogue: str) -> torch.Tensor:
        """The exact value in front of the one rounding."""
        if epilogue == "none":
            return self.acc
        if epilogue == "bias":
            return self.acc + self.bias
        assert epilogue in ("bias_res", "bias_res_stats")
        return self.acc + self.bias + self.res

    def want(self, epilogue: str) -> torch.Tensor:
        return rne(self.pre(epilogue))


def row_stats(stored: torch.Tensor, tile_n: int) -> torch.Tensor:
    """stats_out of cd360_gemm_bf16: [M, ceil(N / tile_n), 2] float64 (sum, sum of squares) of the stored values per row and N tile."""
    v = stored.double()
    M, N = v.shape
    parts = -(-N // tile_n)
    v = torch.nn.functional.pad(v, (0, parts * tile_n - N)).reshape(M, parts, tile_n)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], -1)


def slab_stats(stored: torch.Tensor, slab: int) -> torch.Tensor:
    """cstats of cd360_gemm_cstats_bf16: [M / slab, N, 2] float64 (sum, sum of squares) of the stored values per row slab and channel."""
    v = stored.double()
    M, N = v.shape
    assert M % slab == 0
    v = v.reshape(M // slab, slab, N)
    return torch.stack([v.sum(1), (v * v).sum(1)], -1)


def check_linear(c: LinearCase) -> None:
    """The conditions the exactness argument rests on; raises AssertionError."""
    for name in ("a", "w", "res"):
        assert is_bf16(getattr(c, name)), f"{name} is not bf16-representable"
    assert torch.equal(c.bias.float().double(), c.bias), "bias is not fp32-representable"
    tail = c.bias.abs().max().item() + c.res.abs().max().item()
    assert c.K * c.a.abs().max().item() * c.w.abs().max().item() + tail < TWO24  # (so the fp32 product below is itself exact)
    bound = (c.a.abs().float() @ c.w.abs().float().t()).max().item() + tail
    assert bound < TWO24, f"sum |a||w| + |bias| + |res| = {bound} reaches 2^24"
    if c.family == "stats":
        v = c.want("bias_res_stats").double()
        assert v.abs().sum(1).max().item() < TWO24 and (v * v).sum(1).max().item() < TWO24, "row statistics reach 2^24"
        for r0 in range(0, c.M, 64):  # 64-row slabs contain the 32-row ones
            s = v[r0:r0 + 64]
            assert s.abs().sum(0).max().item() < TWO24 and (s * s).sum(0).max().item() < TWO24, "slab statistics reach 2^24"


def stats_blocks_round(c: LinearCase) -> bool:
    """Every (64-row slab, 128-column tile) block of the stored output holds an output that rounded: each row-statistics partial of a
    slab and each slab-statistics partial of a tile then differs between stored and unrounded values."""
    lo = low16(c.pre("bias_res")) != 0
    return all(bool(lo[r0:r0 + 64, c0:c0 + 128].any()) for r0 in range(0, c.M, 64) for c0 in range(0, c.N, 128))


def nontrivial_linear(c: LinearCase) -> bool:
    """main family: in every epilogue at least 25 % of the outputs are not bf16-representable before rounding and at least 5 % are exact
    ties.  stats family (standard deviation near 140, so few values beyond 256): from 1024 outputs on at least 1 % of the outputs round
    and every 64-row x 128-column block holds one that does, so that stored != unrounded in every partial of the statistics."""
    if c.family == "stats":
        return c.M * c.N < STATS_MIN_OUTPUTS or (rounding_shares(c.pre("bias_res"))[0] >= MIN_STATS_INEXACT and stats_blocks_round(c))
    for e in ("none", "bias", "bias_res"):
        inexact, ties, _ = rounding_shares(c.pre(e))
        if inexact < MIN_INEXACT or ties < MIN_TIES:
            return False
    return True


@functools.lru_cache(maxsize=None)
def linear_case(M: int, N: int, K: int, family: str = "main") -> LinearCase:
    rng = MAIN if family == "main" else STATS[K > 128]
    assert K % 64 == 0 and N % 16 == 0
    for attempt in range(256):
        seed = _seed("linear", family, M, N, K) + attempt
        g = torch.Generator().manual_seed(seed)
        a, w = _ints(g, (M, K), rng["a"]), _ints(g, (N, K), rng["w"])
        bias, res = _ints(g, (N,), rng["b"]), _ints(g, (M, N), rng["r"])
        c = LinearCase(family, M, N, K, seed, a, w, bias, res, a @ w.t())
        check_linear(c)
        if nontrivial_linear(c):
            return c
    raise AssertionError(f"no non-trivial case for {family} {M} x {N} x {K}: widen the value range")


def _last_tile(n: int, tile: int) -> int:
    return (n - 1) // tile * tile


def _last_live_k(x: torch.Tensor, y: torch.Tensor) -> int:
    """The last contraction index at which both operand blocks hold a non-zero (dropping a zero product is no defect)."""
    live = ((x != 0).any(0) & (y != 0).any(0)).nonzero()
    assert live.numel(), "an all-zero operand block"
    return int(live[-1])


def linear_faults(c: LinearCase, epilogue: str) -> Iterator[Tuple[str, bool, torch.Tensor]]:
    """(name, is a rounding defect, defective output) for every defect that applies to this case and epilogue.  The rounding defects
    belong to the main family: the stats family keeps its values small, few of its outputs round."""
    rounding = c.family == "main"
    pre = c.pre(epilogue)
    r0, c0 = _last_tile(c.M, 32), _last_tile(c.N, 32)
    k = _last_live_k(c.a[r0:r0 + 32], c.w[c0:c0 + 32])
    d = pre.clone()  # one k index dropped for one 32 x 32 block (the last, ragged one)
    d[r0:r0 + 32, c0:c0 + 32] -= c.a[r0:r0 + 32, k:k + 1] @ c.w[c0:c0 + 32, k:k + 1].t()
    yield "k-index-dropped-in-one-block", False, rne(d)
    kt = _last_tile(c.K, 64)
    yield "k-tile-added-twice", False, rne(pre + c.a[:, kt:kt + 64] @ c.w[:, kt:kt + 64].t())
    if rounding:
        yield "truncation", True, truncate(pre)
    if rounding and epilogue in ("bias_res", "bias_res_stats"):
        yield "rounded-before-res", True, rne(rne(c.acc + c.bias).double() + c.res)
    if epilogue != "none":  # the last N tile's bias slice fetched 8 columns off (128-column tiles; wider tiles shift the same columns or more)
        b = c.bias.clone()
        n0 = _last_tile(c.N, 128)
        b[n0:] = torch.cat([c.bias[n0 + 8:], torch.zeros(8, dtype=b.dtype)])
        yield "bias-slice-shifted-8", False, rne(pre - c.bias + b)
    if c.N >= 32:
        g = rne(pre).clone()
        g[:, c.N - 16:] = g[:, c.N - 32:c.N - 16]
        yield "last-16-columns-from-neighbour", False, g


def stats_faults(c: LinearCase, tile_n: int = 128, slab: int = 64) -> Iterator[Tuple[str, torch.Tensor, torch.Tensor]]:
    """(name, right, defective) statistics: sums over the unrounded instead of the stored values (cases of >= 1024 outputs)."""
    if c.M * c.N < STATS_MIN_OUTPUTS:
        return
    pre, stored = c.pre("bias_res_stats"), c.want("bias_res_stats")
    yield "row-stats-of-unrounded", row_stats(stored, tile_n), row_stats(pre, tile_n)
    if c.M % slab == 0:
        yield "slab-stats-of-unrounded", slab_stats(stored, slab), slab_stats(pre, slab)


# ---- GEGLU epilogue (flag bit 0): out[:, j] = v_j * gelu(g_j), value rows | gate rows of the projection ------------------------------------
# c = half of Abramowitz-Stegun 7.1.26's absolute bound on erf (1.5e-7: gelu(g) = g / 2 * (1 + erf)) + four fp32 roundings of a value
# near 1.0 (2^-24 each) for the evaluation: 3.13e-7.  delta = c |v| max(|g|, 1).
GEGLU_C = 0.5 * 1.5e-7 + 4 * 2.0 ** -24


@dataclass(frozen=True)
class GegluCase:
    M: int
    N: int  # rows of the projection: N / 2 values | N / 2 gates
    K: int
    a: torch.Tensor     # [M, K] in {-1, 0, 1}
    w: torch.Tensor     # [N, K] in {-1, 0, 1}: rows 0 .. N/2 - 1 values, N/2 .. N - 1 gates (the module's layout, not yet packed)
    bias: torch.Tensor  # [N]
    v: torch.Tensor     # [M, N / 2] exact value pre-activations
    g: torch.Tensor     # [M, N / 2] exact gate pre-activations
    want: torch.Tensor  # [M, N / 2] float64 v * gelu(g)


def geglu_row_order(inner: int) -> torch.Tensor:
    """The packing cd360_gemm_bf16 documents for flag bit 0, restated: per 32 output columns their 32 value rows, then their 32 gate rows."""
    rows = []
    for j0 in range(0, inner, 32):
        rows += list(range(j0, j0 + 32)) + list(range(inner + j0, inner + j0 + 32))
    return torch.tensor(rows, dtype=torch.int64)


def gelu64(g: torch.Tensor) -> torch.Tensor:
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def check_geglu(c: GegluCase) -> None:
    for t in (c.a, c.w):
        assert is_bf16(t) and t.abs().max().item() <= 1
    assert torch.equal(c.bias.float().double(), c.bias)
    assert c.K + c.bias.abs().max().item() < TWO24
    inner = c.N // 2
    pre = c.a @ c.w.t() + c.bias
    assert torch.equal(c.v, pre[:, :inner]) and torch.equal(c.g, pre[:, inner:])
    inside = (c.g.abs() <= 6).double().mean().item()
    assert inside >= 0.9, f"only {inside:.2f} of the gates lie in [-6, 6]"
    assert c.g.unique().numel() >= min(7, c.g.numel() // 2) and (c.want != 0).double().mean().item() >= 0.4, "GELU is trivial on these gates"


@functools.lru_cache(maxsize=None)
def geglu_case(M: int, N: int, K: int) -> GegluCase:
    assert N % 64 == 0 and K % 64 == 0
    g = torch.Generator().manual_seed(_seed("geglu", M, N, K))
    keep = 2.0 / math.sqrt(K)  # share of non-zero operands: the pre-activations come out with a standard deviation near 2

    def sparse(shape):
        return _ints(g, shape, 1) * (torch.rand(shape, generator=g, dtype=torch.float64) < keep * 1.5).double()
    a, w = sparse((M, K)), sparse((N, K))
    bias = _ints(g, (N,), 2)
    pre = a @ w.t() + bias
    v, gate = pre[:, :N // 2].contiguous(), pre[:, N // 2:].contiguous()
    c = GegluCase(M, N, K, a, w, bias, v, gate, v * gelu64(gate))
    check_geglu(c)
    return c


def geglu_band(c: GegluCase, want: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(lo, hi, delta): got must lie in [bf16(want - delta), bf16(want + delta)], delta = GEGLU_C |v| max(|g|, 1)."""
    want = c.want if want is None else want
    delta = GEGLU_C * c.v.abs() * c.g.abs().clamp_min(1.0)
    return (want - delta).to(BF), (want + delta).to(BF), delta


def geglu_accepts(c: GegluCase, got: torch.Tensor) -> Tuple[bool, float]:
    """(every element inside its band, worst error relative to delta).  The error of an element is the least |x - want| over the fp32
    values x that round to the bf16 value seen (|got - want| minus half a bf16 step of got, at least 0): what the kernel's fp32 result
    must have been off by at the least."""
    lo, hi, delta = geglu_band(c)
    got = got.cpu()
    assert got.dtype == BF and got.shape == c.want.shape
    ok = bool(((got.double() >= lo.double()) & (got.double() <= hi.double())).all())
    g64 = got.double()
    exp = torch.frexp(g64.float())[1].double()       # got = m 2^exp, 0.5 <= |m| < 1: bf16 step 2^(exp - 8)
    half_step = torch.where(g64 == 0, torch.zeros_like(g64), 2.0 ** (exp - 9))
    err = ((g64 - c.want).abs() - half_step).clamp_min(0.0)
    ratio = torch.where(delta > 0, err / delta.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return ok, ratio.max().item()


def geglu_faults(c: GegluCase) -> Iterator[Tuple[str, torch.Tensor]]:
    """Defective outputs (bf16) the band rule has to reject."""
    inner = c.N // 2
    yield "value-and-gate-swapped", (c.g * gelu64(c.v)).to(BF)
    if inner >= 64:  # gate block of the neighbouring 32 columns
        g = torch.cat([c.g[:, 32:], c.g[:, :32]], 1)
        yield "gate-of-the-neighbouring-block", (c.v * gelu64(g)).to(BF)
    sh = torch.cat([c.want[:, 8:], c.want[:, :8]], 1)
    yield "output-columns-shifted-8", sh.to(BF)
    yield "tanh-form-gelu", (c.v * 0.5 * c.g * (1 + torch.tanh(math.sqrt(2 / math.pi) * (c.g + 0.044715 * c.g ** 3)))).to(BF)
    yield "gate-bias-missing", (c.v * gelu64(c.g - c.bias[inner:])).to(BF)


# ---- cd360_gemm_tn_bf16: out[N, K] = A[M, N]^T B[M, K] ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TnCase:
    M: int
    N: int
    K: int
    a: torch.Tensor    # [M, N]
    b: torch.Tensor    # [M, K]
    out: torch.Tensor  # [N, K] float64, an exact integer: the fp32 output allows no rounding at all


def check_tn(c: TnCase) -> None:
    assert is_bf16(c.a) and is_bf16(c.b)
    bound = (c.a.abs().t() @ c.b.abs()).max().item()
    assert bound < TWO24, f"sum |a||b| = {bound} reaches 2^24"
    assert torch.equal(c.out, c.a.t() @ c.b)
    exact_f32(c.out)


@functools.lru_cache(maxsize=None)
def tn_case(M: int, N: int, K: int) -> TnCase:
    g = torch.Generator().manual_seed(_seed("tn", M, N, K))
    a, b = _ints(g, (M, N), MAIN["a"]), _ints(g, (M, K), MAIN["w"])
    c = TnCase(M, N, K, a, b, a.t() @ b)
    check_tn(c)
    return c


def tn_faults(c: TnCase) -> Iterator[Tuple[str, torch.Tensor]]:
    """Defective float64 products."""
    m0 = _last_tile(c.M, 64)
    if m0 > 0:  # one slab's partial tile left out (the last 64-row tile is the last slab's tail on every split)
        yield "partial-tile-left-out", c.out - c.a[m0:].t() @ c.b[m0:]
    if c.M % 64:  # rows >= M of the last 64-row tile read as data (here: the operand's first rows again) instead of zero
        n = 64 - c.M % 64
        idx = torch.arange(n) % c.M
        yield "rows-past-M-read-as-data", c.out + c.a[idx].t() @ c.b[idx]
    yield "one-row-dropped", c.out - c.a[c.M - 1:].t() @ c.b[c.M - 1:]


# ---- cd360_lowrank_add_bf16 (p = 0): out = base + T U^T -----------------------------------------------------------------------------------
LOWRANK = dict(t=64, u=32, base=128)  # wide enough that a rank-8 product rounds: sum |t||u| <= 64 * 64 * 32 = 131072


@dataclass(frozen=True)
class LowrankCase:
    M: int
    N: int
    r: int
    t: torch.Tensor     # [M, r]
    u: torch.Tensor     # [N, r]
    base: torch.Tensor  # [M, N]
    prod: torch.Tensor  # [M, N] float64 t u^T

    def want(self, with_base: bool) -> torch.Tensor:
        return rne(self.prod + self.base if with_base else self.prod)


def check_lowrank(c: LowrankCase) -> None:
    assert is_bf16(c.t) and is_bf16(c.u) and is_bf16(c.base)
    bound = (c.t.abs() @ c.u.abs().t()).max().item() + c.base.abs().max().item()
    assert bound < TWO24
    assert torch.equal(c.prod, c.t @ c.u.t())


@functools.lru_cache(maxsize=None)
def lowrank_case(M: int, N: int, r: int) -> LowrankCase:
    for attempt in range(256):
        g = torch.Generator().manual_seed(_seed("lowrank", M, N, r) + attempt)
        t, u, base = _ints(g, (M, r), LOWRANK["t"]), _ints(g, (N, r), LOWRANK["u"]), _ints(g, (M, N), LOWRANK["base"])
        c = LowrankCase(M, N, r, t, u, base, t @ u.t())
        check_lowrank(c)
        if all(rounding_shares(x)[0] >= MIN_INEXACT and rounding_shares(x)[1] >= MIN_TIES for x in (c.prod, c.prod + c.base)):
            return c
    raise AssertionError(f"no non-trivial low-rank case for {M} x {N} x {r}")


def lowrank_faults(c: LowrankCase, with_base: bool) -> Iterator[Tuple[str, bool, torch.Tensor]]:
    pre = c.prod + c.base if with_base else c.prod
    yield "truncation", True, truncate(pre)
    if with_base:
        yield "rounded-before-base", True, rne(rne(c.prod).double() + c.base)
        yield "base-left-out", False, rne(c.prod)
    k = _last_live_k(c.t, c.u)
    yield "k-index-dropped", False, rne(pre - c.t[:, k:k + 1] @ c.u[:, k:k + 1].t())
    g = rne(pre).clone()
    g[:, c.N - 16:] = g[:, c.N - 32:c.N - 16]
    yield "last-16-columns-from-neighbour", False, g


# ---- case lists of tests/test_gemm_exact_gpu.py -------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 16), (40, 48), (128, 128), (300, 272), (520, 208)]  # one row; below a tile; one tile; ragged against 64 .. 256 with N % 32 = 16
K_TILES = tuple(range(1, 13))   # K = 64 t: every residue of the two-, three-, four-buffer and five-slot rings, loops that leave in the prologue
K_TILES_LONG = (20, 48, 80)     # 3072: the k-step groups switch on by default; 5120: a long loop
STATS_K_TILES = (1, 2, 3, 4, 5)  # K <= 320
SWITCH_SHAPE = (4096, 1280, 1280)  # 320 tiles of 128 x 128 (> 256: cfg 2; <= 512 and K >= 1280: the host moves it to cfg 5)

# gemm_asm4 = 1 acts only where the default dispatch chose a 256 x 256 tiling (cfg 3 / 7 -> 9): 1024 tiles of 128 x 128 (> 512) and
# N > 1536 send a plain launch to pick_cfg's efficiency rule, where 256 tiles of 256 x 256 (one full round of the 256 CUs) beat 352 of
# 256 x 192 (two rounds).  K = 192: three K-tiles; the loop itself runs at every K under the forced cfg 9.
ASM4_SHAPE = (4096, 4096, 192)
BIG_SHAPES = (SWITCH_SHAPE, ASM4_SHAPE)


def default_picks_256x256(M: int, N: int) -> bool:
    """pick_cfg of gemm8p.hip for a plain launch with every tuning field at its default, restated: True where it returns cfg 3."""
    nwg = -(-M // 128) * -(-N // 128)
    if nwg <= 128:
        return False           # cfg 8
    if N <= 1536:
        return M >= 65536      # else cfg 4 / 2
    if nwg <= 512:
        return False           # cfg 4 / 5

    def eff(bm, bn):
        tm, tn = -(-M // bm), -(-N // bn)
        rounds = -(-tm * tn // 256)
        return tm * tn / (rounds * 256) * N / (tn * bn)
    return not eff(256, 192) * 0.95 > eff(256, 256)


MOVER_CFGS = (1, 2, 4, 5, 6, 8)  # the arrangements with room for four mover waves (gemm8p.hip: launch_ks)


def _routes() -> List[Tuple[str, Dict[str, int], bool]]:
    """(id, tuning fields, also at the long K)"""
    out: List[Tuple[str, Dict[str, int], bool]] = [("default", {}, True), ("small-off", dict(gemm_small=0), True)]
    for cfg in range(1, 10):
        if cfg not in (4, 8):
            out.append((f"cfg{cfg}", dict(gemm_cfg=cfg), cfg in (3, 5, 9)))
    out += [(f"cfg4-ksplit{k}", dict(gemm_cfg=4, gemm_ksplit=k), True) for k in (0, 1, 2)]
    out += [(f"cfg8-ksplit{k}", dict(gemm_cfg=8, gemm_ksplit=k), True) for k in (0, 1)]
    for cfg in MOVER_CFGS:
        out += [(f"cfg{cfg}-movers{mv}", dict(gemm_cfg=cfg, gemm_movers=mv), False) for mv in (0, 4)]
    out += [("cfg4-ksplit1-movers0", dict(gemm_cfg=4, gemm_ksplit=1, gemm_movers=0), False),
            ("cfg4-ksplit1-movers4", dict(gemm_cfg=4, gemm_ksplit=1, gemm_movers=4), False)]
    return out


GEMM_ROUTES = _routes()
GEMM_ROUTES_LONG = [r for r in GEMM_ROUTES if r[2]]

# cd360_gemm_cstats_bf16: 64-row slabs on the 128 x 128 tilings (cfg 2, cfg 4 in both wave arrangements), 32-row slabs on 64 x 128 (cfg 8)
CSTATS_ROUTES = [("cfg2", dict(gemm_cfg=2), 64), ("cfg4-ksplit0", dict(gemm_cfg=4, gemm_ksplit=0), 64), ("cfg4-ksplit1", dict(gemm_cfg=4, gemm_ksplit=1), 64),
                 ("cfg8-ksplit0", dict(gemm_cfg=8, gemm_ksplit=0), 32), ("cfg8-ksplit1", dict(gemm_cfg=8, gemm_ksplit=1), 32), ("default", {}, None)]
CSTATS_M = (64, 192, 1024)
CSTATS_NK = [(48, 64), (272, 192), (128, 320)]

# (asm4: the GEGLU default is cfg 7, which gemm_asm4 = 1 moves onto the generated loop)
GEGLU_ROUTES = [("default", {})] + [(f"cfg{c}", dict(gemm_cfg=c)) for c in (1, 3, 5, 7, 9)] + [("asm4", dict(gemm_cfg=-1, gemm_asm4=1))]
GEGLU_SHAPES = [(1, 64), (40, 128), (300, 320), (520, 704)]  # N / 2 = 32 .. 352: one packed group, below a tile, ragged against 128 and 256
GEGLU_K = (64, 192)

TN_M = (1, 63, 64, 65, 200, 1024, 4100)
TN_NK = [(8, 8), (136, 72), (128, 128), (264, 320)]

LOWRANK_R = (8, 16, 32, 64)
LOWRANK_M = (1, 77, 333)
LOWRANK_N = (320, 640)


def linear_cases() -> Iterator[Tuple[str, int, int, int]]:
    """Every (family, M, N, K) the GPU tests build.  The value ranges are the same for every shape; where the first seed of a case
    misses the floors the builder takes the next one (linear_case), which happens at the smallest shapes only -- the 16 outputs of
    (1, 16) are seed-selected, from (40, 48) on the first or second seed serves (LinearCase.seed records it)."""
    for M, N in GEMM_SHAPES:
        for t in K_TILES + K_TILES_LONG:
            yield "main", M, N, 64 * t
        for t in STATS_K_TILES:
            yield "stats", M, N, 64 * t
    for shape in BIG_SHAPES:
        yield ("main",) + shape
    for M in CSTATS_M:
        for N, K in CSTATS_NK:
            yield "stats", M, N, K
