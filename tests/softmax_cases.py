"""Deterministic attention inputs whose softmax rows reach the data-dependent paths of the online-softmax kernels, with a float64
reference.  CPU only: nothing here imports the HIP library.

Logits are counted in exp2 units, u = c * (q . k) with c = softmax scale * log2 e (c = 1 for a pre-scaled q): the kernels'
exponentials are exp2, their lazy-maximum slack is 8 units, and exp2 leaves fp32 at +-128 units.

A case is q, k, v (and dO), rounded to bf16, of which a small share of rows is CRAFTED; every other row stays randn.  Crafted queries
sit in EVERY 32-query block of every (batch, head) at lane offsets 0, 3, 17, 31 in turn, so each (wave, query block) slot of each
kernel geometry (4 x 32, 8 x 32, 8 x 64 queries per workgroup; 4 x 16 for the single-head kernel) holds one, in more than one workgroup.
The crafted rows of a head fall into a few GROUPS; a group is one direction e_g (orthonormal within the head, so groups do not see
each other's keys), its queries q_i = s * |q| * e_g, and its keys k_j = a * q_i with a chosen for a target logit T:

  late-spike   one key at T = 150: the group's key sits in one position class (first / interior / last tile, rows 0-31 / 32-63 of the
               tile, the last real key; for the key-split kernel first / interior / last split).  One group per class.
  tie          two IDENTICAL keys at T = 150, one in the first and one in the last tile (split), their v >= 0: the row is exactly
               (v_a + v_b) / 2, and no element of it is a cancelled difference.
  stair-up     one key per 64-key tile at T = 16 + 12 t: the maximum moves by 12 units at every tile, the last tile wins.
  stair-down   T = 190 in the first tile (split), 50 in the last: nothing rescales after tile 0, a whole split's weight underflows.
  cold-start   every key of the first tile at T = -150 (below -128 units), the rest ordinary.
  offset       every key of the head carries a * u, the crafted queries are +-u + half a randn row: all of their logits sit near +-L.
               The other rows of the head see one common shift per row, to which softmax is invariant.
  uniform      the last (batch, head): all keys identical, v >= 0: every row is the mean of v and lse = s + ln Nk.

s = 8 (2 for stair-up) trades the two kinds of cross-talk: an uncrafted query meets a crafted key at T z / (s sqrt D) units (2.3 z at
T = 150), a crafted query meets an uncrafted key at 1.44 s z units (margins are measured, not assumed: tests/test_softmax_cases_cpu.py).
T = 150 and not 40 + spread: only beyond 128 units does a maximum that failed to move overflow exp2.

For the backward cases (per_block = 4) every 32-query block holds four crafted queries, a group's queries come from all 64-query
tiles, and dO of the crafted queries is scaled by 2^-6 so that the sum of the >= 8 dO rows a dominating key wins stays below the
largest uncrafted gradient: the max-normalised bars are then set by ordinary rows.  (2^-9 for tie: there dS = +-(dP_a - dP_b) / 4 does
not vanish, and dk of the two keys gathers it times the crafted queries' large q.)"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
LANE_OFFSETS = (0, 3, 17, 31)
FAMILIES = ("late-spike", "tie", "stair-up", "stair-down", "cold-start", "offset", "uniform")
T_SPIKE, T_TOP, T_LOW, T_COLD, STAIR_BASE, STAIR_STEP = 150.0, 190.0, 50.0, -150.0, 16.0, 12.0
DO_SCALE = {"tie": 2.0 ** -9}  # of the crafted queries' dO rows; 2^-6 for every other family
SINGLE_KT, SINGLE_QB, SINGLE_MAX_SPLIT = 32, 64, 16


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def single_splits(n: int) -> Tuple[int, int]:
    """(splits, keys per split) of the single-head kernel for n pixels: the launch arithmetic of cd360_attn_single_bf16, restated so
    that cases can be placed without the library (the GPU test holds the count against attention_single_splits)."""
    qblocks, ntiles = -(-n // SINGLE_QB), -(-n // SINGLE_KT)
    s = min(-(-1024 // qblocks), SINGLE_MAX_SPLIT, ntiles // 8)
    if s < 2:
        return 1, ntiles * SINGLE_KT
    per = -(-ntiles // s)
    return -(-ntiles // per), per * SINGLE_KT


def key_classes(geometry: str, nk: int) -> List[Tuple[str, int, int]]:
    """Position classes [name, first key, end) a dominating key is placed in, for one kernel geometry."""
    if geometry == "smallk":  # register-resident keys: the two ends (key Nk - 1 is the neighbour of the -1e30 padding) and the middle
        return [("key0", 0, 1), ("mid", nk // 2, nk // 2 + 1), ("last-key", nk - 1, nk)]
    if geometry == "single":
        ns, per = single_splits(nk)
        out = [("split0-lo", 0, 16), ("split0-hi", 16, min(32, nk))]
        if ns >= 3:
            mid = ns // 2
            out.append((f"split{mid}", mid * per + 40, mid * per + 64))
        if ns >= 2:
            last_tile = (nk - 1) // SINGLE_KT * SINGLE_KT
            out.append((f"split{ns - 1}-last-tile", last_tile, nk - 1))
        out.append(("last-key", nk - 1, nk))
        return [c for c in out if c[2] > c[1]]
    if geometry == "bwd":  # dK / dV role: 128-key tiles, 32 stationary keys per wave; a ragged last tile where there is one
        n128 = nk // 128
        out = [(f"ktile{w % max(n128, 1)}-wave{w}", 128 * (w % max(n128, 1)) + 32 * w, min(128 * (w % max(n128, 1)) + 32 * w + 32, nk)) for w in range(4)]
        if n128 and nk % 128:
            out.append((f"ktile{n128}-ragged", 128 * n128, nk))
        return [c for c in out if c[2] > c[1]]
    nt = -(-nk // 64)
    out = [("tile0-lo", 0, 32), ("tile0-hi", 32, min(64, nk))]
    if nt >= 3:
        t = nt // 2
        out += [(f"tile{t}-lo", 64 * t, 64 * t + 32), (f"tile{t}-hi", 64 * t + 32, 64 * t + 64)]
    if nt >= 2:
        lo = 64 * (nt - 1)
        out.append((f"tile{nt - 1}-lo", lo, min(lo + 32, nk - 1)))
        if nk - 1 > lo + 32:
            out.append((f"tile{nt - 1}-hi", lo + 32, nk - 1))
    out.append(("last-key", nk - 1, nk))
    return [c for c in out if c[2] > c[1]]


@dataclass
class Row:
    """One crafted query row and what is asserted about it."""
    b: int
    h: int
    i: int
    family: str
    group: int
    keys: Tuple[int, ...] = ()       # the keys this row is built to be dominated by (winning key first)
    where: str = ""                  # position class of the winning key
    margin: float = 0.0              # claimed lower bound, in units, of winner minus every other key (0: not dominated)
    target: Optional[torch.Tensor] = None  # [D] float64: the value every element must meet within 2^-7 relative (dominated rows only)


@dataclass
class Case:
    name: str
    family: str
    geometry: str
    B: int
    H: int
    Nq: int
    Nk: int
    D: int
    c: float                         # exp2 units per unit of q . k
    q: torch.Tensor                  # [B, Nq, H * D] float32 holding bf16 values
    k: torch.Tensor                  # [B, Nk, H * D]
    v: torch.Tensor
    do: torch.Tensor                 # [B, Nq, H * D]
    rows: List[Row] = field(default_factory=list)
    crafted_keys: List[Tuple[int, int, int]] = field(default_factory=list)  # (b, h, j): keys overwritten
    dominating: List[Tuple[int, int, int, Tuple[int, ...]]] = field(default_factory=list)  # (b, h, j, queries i it wins)
    uniform_heads: List[Tuple[int, int]] = field(default_factory=list)
    L: float = 0.0

    def heads4(self, t: torch.Tensor) -> torch.Tensor:
        """[B, N, H * D] -> [B, H, N, D]"""
        return t.reshape(t.shape[0], t.shape[1], self.H, self.D).permute(0, 2, 1, 3)

    def crafted_q_mask(self) -> torch.Tensor:
        """[B, Nq, H] bool"""
        m = torch.zeros(self.B, self.Nq, self.H, dtype=torch.bool)
        for r in self.rows:
            m[r.b, r.i, r.h] = True
        return m

    def crafted_k_mask(self) -> torch.Tensor:
        m = torch.zeros(self.B, self.Nk, self.H, dtype=torch.bool)
        for b, h, j in self.crafted_keys:
            m[b, j, h] = True
        for b, h in self.uniform_heads:
            m[b, :, h] = True
        return m


def _query_rows(nq: int, per_block: int, shift: int, tail: int = 0) -> List[int]:
    """Crafted query rows of one head: per_block rows in every 32-query block, at most nq / 8 in all; tail > 0: at least `tail` of them
    in the last (ragged) 64-query tile, at the end of the list, so that every group gets one."""
    rows = []
    for blk in range(-(-nq // 32)):
        for j in range(per_block):
            off = LANE_OFFSETS[(blk + shift) % 4] if per_block == 1 else LANE_OFFSETS[j]
            i = blk * 32 + off % min(32, nq - blk * 32)  # ragged last block: folded into the rows that exist
            if i not in rows:
                rows.append(i)
    start = (nq - 1) // 64 * 64 if tail else nq
    last = [i for i in rows if i >= start]
    last += [i for i in range(nq - 1, start - 1, -1) if i not in last][:max(0, tail - len(last))]
    head = [i for i in rows if i < start]
    for t in range(max(0, len(head) + len(last) - nq // 8)):  # over the share: thin the blocks out from the end, one row each
        del head[len(head) - 1 - (per_block - 1) * t]
    return head + sorted(last)


@functools.lru_cache(maxsize=None)
def make_case(family: str, B: int, H: int, Nq: int, Nk: int, D: int = 64, mode: str = "plain", geometry: str = "tiled", per_block: int = 1,
              L: float = 60.0, signs: str = "both") -> Case:
    """mode: 'plain' (c = D^-0.5 log2 e, q ~ randn), 'prescaled' (q already carries that factor: c = 1).  geometry: 'tiled' (64-key
    tiles), 'smallk' (all keys at once), 'single' (one head of D channels, 32-key tiles, key splits)."""
    assert family in FAMILIES
    c0 = D ** -0.5 * LOG2E
    c, qstd = (1.0, c0) if mode == "prescaled" else (c0, 1.0)
    if geometry == "single":  # qscale is an argument of that entry: 2 D^-0.5 log2 e keeps the largest of 4100 ordinary weights above 1 %
        c *= 2.0
    # the crafted queries' scale s of the module docstring: 4 at the single-head entry (same logit spread); 16 for the backward, where a
    # dominating key must look like any other key to the uncrafted queries or its dk / dv would be the largest of the tensor
    big = {"single": 4.0, "bwd": 16.0}.get(geometry, 8.0)
    name = f"{family}-{mode}-{geometry}-b{B}h{H}-q{Nq}-k{Nk}-d{D}-pb{per_block}-L{L:g}{signs}"
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    q = bf(torch.randn(B, Nq, H, D, generator=g) * qstd)
    k = bf(torch.randn(B, Nk, H, D, generator=g))
    v = bf(torch.randn(B, Nk, H, D, generator=g))
    do = bf(torch.randn(B, Nq, H, D, generator=g))
    case = Case(name, family, geometry, B, H, Nq, Nk, D, c, q, k, v, do, L=L)
    qn = qstd * math.sqrt(D)
    tile = SINGLE_KT if geometry == "single" else 64
    classes = key_classes(geometry, Nk)
    heads = [(b, h) for b in range(B) for h in range(H)]

    if family == "uniform":
        b, h = heads[-1]
        k[b, :, h] = k[b, 0, h]
        v[b, :, h] = v[b, :, h].abs()
        case.uniform_heads.append((b, h))
        target = v[b, :, h].double().mean(0)
        for i in range(Nq):
            case.rows.append(Row(b, h, i, family, 0, target=target))
        return _finish(case)
    assert family != "cold-start" or Nk >= 2 * tile

    for hi, (b, h) in enumerate(heads):
        pairs = 2 if len(classes) >= 4 else 1  # groups of the two-key families
        n_groups = {"late-spike": len(classes), "tie": pairs, "stair-down": pairs}.get(family, 1)
        E = torch.linalg.qr(torch.randn(D, n_groups, generator=g, dtype=torch.float64))[0]  # orthonormal columns
        used = set()

        def vec(gi, s):
            return bf((s * qn * E[:, gi]).float())

        def place(cls, salt):
            _, lo, hi_ = cls
            free = [j for j in range(lo, hi_) if j not in used] or [j for j in range(lo - 1, -1, -1) if j not in used]
            j = free[(7 * salt + 3 * hi) % len(free)] if free[0] >= lo else free[0]
            used.add(j)
            return j

        def key_for(qv, T):  # k = a q with c * a * |q|^2 = T
            return bf(qv * (T / (c * float(qv.double().pow(2).sum()))))

        groups = []  # per group: (q vector, [(key index, key vector)], winning keys, position name, claimed margin, target)
        if family == "late-spike":
            for gi, cls in enumerate(classes):
                qv = vec(gi, big)
                j = place(cls, gi)
                groups.append((qv, [(j, key_for(qv, T_SPIKE))], (j,), cls[0], 40.0, "v"))
        elif family == "tie":
            for gi in range(pairs):
                qv = vec(gi, big)
                first, last = classes[gi], classes[-1 - gi]
                ja, jb = place(first, gi), place(last, gi)
                kv = key_for(qv, T_SPIKE)
                v[b, ja, h], v[b, jb, h] = v[b, ja, h].abs(), v[b, jb, h].abs()  # no cancellation in the mean: the bound is relative
                groups.append((qv, [(ja, kv), (jb, kv)], (ja, jb), f"{first[0]}+{last[0]}", 40.0, "mean"))
        elif family == "stair-up":
            nt = -(-Nk // 64)
            assert geometry == "tiled" and STAIR_BASE + STAIR_STEP * (nt - 1) <= 196.0
            qv = vec(0, big / 4)
            ks = []
            for t in range(nt):
                width = min(64, Nk - 64 * t)
                ks.append((64 * t + (5 + 37 * t + hi) % width, key_for(qv, STAIR_BASE + STAIR_STEP * t)))
            groups.append((qv, ks, (ks[-1][0],), "every-tile", 0.0, None))
        elif family == "stair-down":
            low = classes[-2] if len(classes) >= 3 else classes[-1]
            for gi in range(pairs):
                qv = vec(gi, big)
                ja, jb = place(classes[gi], gi), place(low, gi)
                groups.append((qv, [(ja, key_for(qv, T_TOP)), (jb, key_for(qv, T_LOW))], (ja,), f"{classes[gi][0]}>{low[0]}", 40.0, "v"))
        elif family == "cold-start":
            qv = vec(0, big)
            kv = key_for(qv, T_COLD)
            groups.append((qv, [(j, kv) for j in range(tile)], (), "tile0", 0.0, None))
        elif family == "offset":
            u = vec(0, 1.0)
            k[b, :, h] = bf(k[b, :, h] + u * (abs(L) / (c * float(u.double().pow(2).sum()))))
            groups.append((u, [], (), "all-keys", 0.0, None))

        if (len(case.crafted_keys) + sum(len(g_[1]) for g_ in groups)) * 8 > B * H * Nk:
            continue  # the 1/8 share of key rows is spent (few keys, or cold-start's whole first tile): this head stays ordinary
        for gi, (qv, ks, win, where, margin, kind) in enumerate(groups):
            for j, kv in ks:
                k[b, j, h] = kv
                case.crafted_keys.append((b, h, j))
        rows = _query_rows(Nq, per_block, hi, tail=len(groups) if geometry == "bwd" else 0)
        won = {gi: [] for gi in range(len(groups))}
        for n, i in enumerate(rows):
            gi = n % len(groups)
            qv, ks, win, where, margin, kind = groups[gi]
            if family == "offset":
                sign = -1.0 if (signs == "minus" or (signs == "both" and n % 2)) else 1.0
                sign = math.copysign(1.0, L) * sign
                q[b, i, h] = bf(sign * qv + 0.5 * q[b, i, h])
            else:
                q[b, i, h] = qv
            do[b, i, h] = bf(do[b, i, h] * DO_SCALE.get(family, 2.0 ** -6))
            target = None
            if kind == "v":
                target = v[b, win[0], h].double()
            elif kind == "mean":
                target = (v[b, win[0], h].double() + v[b, win[1], h].double()) / 2
            case.rows.append(Row(b, h, i, family, gi, win, where, margin, target))
            won[gi].append(i)
        for gi, (qv, ks, win, where, margin, kind) in enumerate(groups):
            for j in win if kind else ():
                case.dominating.append((b, h, j, tuple(won[gi])))
    return _finish(case)


def _finish(case: Case) -> Case:
    B, H, D = case.B, case.H, case.D
    case.q, case.k, case.v, case.do = (t.reshape(B, t.shape[1], H * D).contiguous() for t in (case.q, case.k, case.v, case.do))
    return case


@dataclass
class Reference:
    out: torch.Tensor      # [B, Nq, H * D] float64
    lse: torch.Tensor      # [B * H, Nq] float64, natural log-sum-exp of the scaled scores
    dq: Optional[torch.Tensor] = None
    dk: Optional[torch.Tensor] = None
    dv: Optional[torch.Tensor] = None


def attention_f64(case: Case, q, k, v):
    units = torch.matmul(case.heads4(q), case.heads4(k).transpose(-1, -2)) * case.c
    s = units * LN2
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = torch.matmul(p, case.heads4(v)).permute(0, 2, 1, 3).reshape(case.B, case.Nq, case.H * case.D)
    return out, lse.reshape(case.B * case.H, case.Nq), units, p


_REFS = {}


def reference(case: Case, grads: bool = False) -> Reference:
    """float64 softmax attention on the bf16-rounded inputs (and its autograd gradients for dO); computed once per case and shared."""
    key = (case.name, grads)
    if key in _REFS:
        return _REFS[key]
    q, k, v = (t.double() for t in (case.q, case.k, case.v))
    if not grads:
        with torch.no_grad():
            ref = Reference(*attention_f64(case, q, k, v)[:2])
    else:
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        out, lse, units, p = attention_f64(case, q, k, v)
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), case.do.double())
        ref = Reference(out.detach(), lse.detach(), dq, dk, dv)
    _REFS[key] = ref
    return ref


def logits(case: Case):
    """(units [B, H, Nq, Nk], softmax p) in float64: what the CPU test proves the builder's claims from."""
    with torch.no_grad():
        return attention_f64(case, case.q.double(), case.k.double(), case.v.double())[2:]


def device_inputs(case: Case, pad: bool = False, device: str = "cuda"):
    """q, k, v as bf16 on the device in the projection layouts: one merged q|k|v tensor for self-attention; otherwise k and v as column
    slices of one wider tensor with a gap between them and, with pad, NaN rows beyond Nk (neither may ever be read as data)."""
    HD = case.H * case.D
    if case.Nq == case.Nk and not pad:
        d = torch.cat([case.q, case.k, case.v], -1).to(device, torch.bfloat16)
        return d[..., :HD], d[..., HD:2 * HD], d[..., 2 * HD:]
    nkp = (case.Nk + 7) // 8 * 8 + (8 if pad else 0)
    kv = torch.full((case.B, nkp, 2 * HD + 64), float("nan"))
    kv[:, :case.Nk, :HD] = case.k
    kv[:, :case.Nk, HD + 64:] = case.v
    kvd = kv.to(device, torch.bfloat16)
    return case.q.to(device, torch.bfloat16), kvd[..., :HD], kvd[..., HD + 64:]


def q_rows(case: Case, t: torch.Tensor) -> torch.Tensor:
    """The crafted query rows of a [B, Nq, H * D] tensor, [n, D]."""
    return t.reshape(case.B, t.shape[1], case.H, case.D)[case.crafted_q_mask()]


def k_rows(case: Case, t: torch.Tensor) -> torch.Tensor:
    return t.reshape(case.B, t.shape[1], case.H, case.D)[:, :case.Nk][case.crafted_k_mask()]


def row_of(case: Case, t: torch.Tensor, b: int, h: int, i: int) -> torch.Tensor:
    return t[b, i, h * case.D:(h + 1) * case.D]


# ------------------------------------------------------------------------------------------------ the cases the GPU tests run
def spec(family, B, H, Nq, Nk, D=64, mode="plain", geometry="tiled", per_block=1, L=60.0, signs="both"):
    return (family, B, H, Nq, Nk, D, mode, geometry, per_block, L, signs)


def spec_id(s) -> str:
    family, B, H, Nq, Nk, D, mode, geometry, per_block, L, signs = s
    tail = f"-L{L:g}" if family == "offset" else ""
    return f"{family}-{geometry}-{mode}-b{B}h{H}-{Nq}x{Nk}" + (f"-d{D}" if D != 64 else "") + tail


SELF_SHAPES = [(128, 128), (256, 256), (512, 512), (1024, 1024), (512, 128), (512, 192), (512, 320)]
SELF_FAMILIES = ("late-spike", "tie", "stair-up", "stair-down", "cold-start")
SELF_CASES = [spec(f, 2, 2, nq, nk) for nq, nk in SELF_SHAPES for f in SELF_FAMILIES]
PRESCALED_CASES = [spec(f, 2, 2, nq, nk, mode="prescaled") for nq, nk in SELF_SHAPES + [(200, 200)] for f in SELF_FAMILIES + ("offset",)]
RAGGED_SHAPES = [(200, 333), (100, 97), (333, 130)]
RAGGED_CASES = [spec(f, 2, 2, nq, nk) for nq, nk in RAGGED_SHAPES for f in SELF_FAMILIES + ("offset", "uniform") if f != "cold-start" or nk >= 128]
SMALLK_FAMILIES = ("late-spike", "tie", "stair-down", "offset", "uniform")
SMALLK_CASES = [spec(f, 2, 2, nq, nk, geometry="smallk", L=-60.0, signs="plus") for nq in (200, 256) for nk in (20, 40, 77) for f in SMALLK_FAMILIES]
SINGLE_CASES = [spec(f, 1, 1, n, n, D=d, geometry="single") for d in (64, 512) for n in (33, 500, 4100)
                for f in ("late-spike", "tie", "stair-down", "offset", "uniform", "cold-start") if f != "cold-start" or n >= 256]
XFORMERS_CASES = [spec(f, 4, 1, 300, 300) for f in ("late-spike", "tie")]
BWD_SHAPES = [(256, 256), (200, 77), (333, 130), (512, 512)]
BWD_CASES = [spec(f, 2, 2, nq, nk, geometry="bwd", per_block=4) for nq, nk in BWD_SHAPES
             for f in ("late-spike", "tie", "uniform", "offset", "cold-start") if f != "cold-start" or nk >= 128]
FORWARD_CASES = SELF_CASES + PRESCALED_CASES + RAGGED_CASES + SMALLK_CASES + SINGLE_CASES + XFORMERS_CASES
