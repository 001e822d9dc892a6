"""Inputs on which a float64 softmax attention is the exact answer of every attention kernel that STREAMS its keys in tiles, up to the
one bf16 rounding of the output (CPU only, no HIP import; tests/test_attn_tile_cpu.py checks the builders, tests/test_attn_tile_gpu.py
runs the kernels): attn_fwd_kernel (64-key tiles, eager maximum), attn_self_kernel<QB, NW> (64-key tiles, lazy maximum with an 8-unit
slack, 4-slot ring), attn_single_kernel + attn_single_combine_kernel (head dim 128 .. 512, 32-key tiles, key splits) and both roles of
attn_bwd_kernel.  The method is that of tests/attn_grid_cases.py: K and V are integers in [-7, 7] times a power of two per (batch,
head) (2^j, j in {0, 1, -1}, different for K and V, for neighbouring heads and batch elements), q carries 2^-j of K, and the scale
passed through the C ABI makes scale * log2(e) exactly 1.0f.  Every logit is then an INTEGER number of exp2 units, so every p, every
alpha of a moving maximum (eager or lazy: move_ref, catch_up's ldexpf) is a power of two, and the result does not depend on when a
maximum moves.  k rows >= Nk (8 of them, inside the allocation) are attractive padding, v rows >= Nk are 7.

Three case families:

  mix     rows of four kinds interleaved by row, kind = i % 4, so every 32-query block (one wave's wave-uniform move_ref branch) serves
          rows that need a move beside rows that do not.  Per head five channels are reserved: `bias` (K = 1 on every real key), three
          `level` channels (the balanced base-15 digits, each in [-7, 7], of a per-key level lv) and `half` (K = +7 on keys with
          key % 8 >= 4, -7 on the others: the two key halves of TileMax -- .ref is the maximum over the keys held by lanes 0-31, which
          are the keys with key % 8 < 4).  Every other channel of K holds 1 .. 7 (times a sign per channel), with a 7 planted in every
          (16-key block, key half, channel).  Every row has q = +-1 on one of these channels d0 (cycling with the row), which gives it
          the BAND kk[key, d0] in 1 .. 7: six units wide, many keys per level.
            band    q[bias] = beta: the row maximum is L = 7 + beta, beta from BETAS: negative (L <= -10 on every real key: a
                    zero-filled unmasked key takes the row), 0 .. 8 and well above 8.  Bit budget (asserted in check_conditions): every p
                    is 2^-6 .. 1 of the row maximum, so in units of 2^-6 each partial sum of l is an integer below Nk 2^6 -- 6 +
                    log2 Nk <= 16 bits -- and each partial sum of O (|v| <= 7 2^j) needs 3 more: 19 <= 24.  l and O are exact sums in
                    fp32 in any order, whatever power of two the lazy m_ref contributes.
            up      q[level m] = 15^m: logit = band + lv(key).  lv rises from tile to tile by STEPS (3 .. 8: inside the slack, no move;
                    9 .. 12: a move); the keys that carry the tile's level sit in the lower / upper 32 keys and in the .ref / other key
                    half in turn ((block, half) = (t % 2, ((t + 1) / 2) % 2): all four combinations), the rest of the tile is 4 below.
                    In tile DOUBLE the .ref half rises by 10 and the other half by 10 more: move_ref then catch_up in one tile.  The
                    last tile wins.
            down    q[level m] = -15^m: the maximum is in tile 0, tile t >= 1 is lv(t) >= 10 units below it.
            half    band + beta and q[half] = 10: the keys with key % 8 >= 4 stand 140 units above the others in EVERY tile.  A maximum
                    taken from the lower key half alone (the fault the v_permlane32_swap comment in csrc/attn_fwd.hip records) leaves
                    m_ref 140 below the row maximum: exp2 overflows.
  onehot  q is dense: the winning key's row itself (integers in [-7, 7], a +-7 in channel 0) times 2^e; the winner is >= 24 units
          above every other key and above the padding and cycles with the query over ALL keys (Nq >= Nk), so every key slot of every
          tile, ring slot and split is the winner of some row in every (batch, head).  The output is bf16(v_winner) bit for bit.  (A
          family of its own and not a fifth row kind: one row per key leaves no rows for the others, and its K is dense.)
  bwd     one-hot for the backward: key j holds +-4 in two channels (a pair no other key or padding row has), q = 2 k_winner: the
          winner's logit is 64 units, every other key is at -32, 0 or 32, so |s| <= 64 (the fp32 rounding of lse moves P by <= 2^-18)
          and the margin is 32.  dO = +-(1 .. 3), the sign a function of the channel, so the per-key sums are non-zero small integers.

The single-head kernel takes the same families at head dim D with H = 1 and 32-key tiles (levels per 32-key tile: every split and
the ragged last tile hold one; one-hot winners visit every key)."""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from attn_grid_cases import BAR_ABS, BAR_REL, SCALE, c_f32, jk_of, jv_of, sgn0
from softmax_cases import SINGLE_KT, single_splits

LN2_F32 = np.float32(0.6931471805599453)
LOG2E_F32 = np.float32(1.4426950408889634)
PAD = 8
SLACK = 8.0
BETAS = (-17, 1, 30, -9, 5, -7, 13, 0, 2, -3, 9, 20)   # band rows: L = 7 + beta
STEPS = (10, 5, 5, 11, 3, 9, 8, 12, 6, 10, 4, 9, 7)       # rise of the tile level, tile t - 1 -> t (t >= 1), cycled
DOUBLE = 2                                             # the tile in which both key halves rise by 10 (tile 1 where there are only two)
OTHERS_BELOW = 4
HALF_GAIN = 10                                         # times +-7: the key halves of a `half` row stand 140 units apart
KINDS = ("band", "up", "down", "half")


@dataclass(frozen=True)
class Spec:
    family: str          # "mix" | "onehot" | "bwd"
    Nq: int
    Nk: int
    H: int = 2
    B: int = 2
    D: int = 64
    tile: int = 64       # keys per tile of the kernel the case is built for (the level plan follows it)


def spec_id(sp: Spec) -> str:
    return f"{sp.family}-b{sp.B}h{sp.H}-{sp.Nq}x{sp.Nk}" + (f"-d{sp.D}" if sp.D != 64 else "")


@dataclass
class Case:
    spec: Spec
    q: torch.Tensor      # [B, Nq, H, D] float64
    k: torch.Tensor      # [B, Nk + 8, H, D] float64, padding rows included
    v: torch.Tensor
    do: Optional[torch.Tensor]       # bwd: [B, Nq, H, D]
    winner: Optional[torch.Tensor]   # onehot, bwd: [Nq] key index
    kind: Optional[np.ndarray]       # mix: [Nq] index into KINDS

    @property
    def rows(self):
        return self.k.shape[1]


def reserved(h, D):
    """(bias, level 0, level 1, level 2, half) channels of head h."""
    b = (7 + 13 * h) % D
    return [(b + i) % D for i in range(5)]


def digits15(x):
    """Balanced base-15 digits (each in [-7, 7]) of the integers x, least significant first: x = d0 + 15 d1 + 225 d2."""
    x = np.asarray(x, dtype=np.int64).copy()
    out = []
    for _ in range(3):
        d = (x + 7) % 15 - 7
        out.append(d)
        x = (x - d) // 15
    assert not x.any()
    return out


def key_half(key):
    """0: the key is held by lanes 0-31 of the S^T accumulator (TileMax.ref), 1: by lanes 32-63."""
    return (np.asarray(key) % 8) // 4


def level_plan(nk, tile):
    """lv [nk] of the real keys and T [tiles], the tile levels."""
    nt = -(-nk // tile)
    double = min(DOUBLE, nt - 1)
    T = [0]
    for t in range(1, nt):
        T.append(T[-1] + (20 if t == double else STEPS[(t - 1) % len(STEPS)]))
    key = np.arange(nk)
    t = key // tile
    blk, hf = (key % tile) // (tile // 2), key_half(key)
    at = (blk == t % 2) & (hf == ((t + 1) // 2) % 2)
    lv = np.where(at, np.array(T)[t], np.array(T)[t] - OTHERS_BELOW)
    for tt in range(nt):   # a ragged tile without a key at its place: all of its keys carry the level
        if not at[t == tt].any():
            lv[t == tt] = T[tt]
    if double >= 1:
        lv[t == double] = np.where(hf[t == double] == 0, T[double] - 10, T[double])
    return lv, np.array(T)


def beta_of(i):
    i = np.asarray(i)
    return np.array(BETAS)[(i // 4 + i // 32) % len(BETAS)]


@functools.lru_cache(maxsize=8)
def make_case(sp: Spec) -> Case:
    assert sp.family in ("mix", "onehot", "bwd") and sp.D % 64 == 0
    B, H, D, Nq, Nk = sp.B, sp.H, sp.D, sp.Nq, sp.Nk
    rows = Nk + PAD
    rng = np.random.default_rng(7919 * Nk + 31 * Nq + D + {"mix": 0, "onehot": 1, "bwd": 2}[sp.family])
    i = np.arange(Nq)
    q = np.zeros((B, Nq, H, D))
    k = np.zeros((B, rows, H, D))
    v = rng.integers(1, 7, size=(B, rows, H, D)) * np.where(rng.random((B, rows, H, D)) < 0.5, 1.0, -1.0)   # no zero
    v[:, Nk:] = 7
    do = winner = kind = None
    if sp.family == "mix":
        kind = i % 4
        lv, _ = level_plan(Nk, sp.tile)
        dig = digits15(lv)
        key = np.arange(Nk)
        group = (key // 16) * 2 + key_half(key)
        for h in range(H):
            res = reserved(h, D)
            free = [d for d in range(D) if d not in res]
            sg = sgn0(np.arange(D), h)
            kk = rng.integers(1, 8, size=(B, Nk, D))
            for b in range(B):   # a 7 in every (16-key block, key half, channel)
                for g in range(group.max() + 1):
                    members = key[group == g]
                    kk[b, members[rng.integers(0, len(members), size=D)], np.arange(D)] = 7
            k[:, :Nk, h] = kk * sg
            k[:, Nk:, h] = 7 * sg
            k[:, :Nk, h, res[0]] = 1
            for m in range(3):
                k[:, :Nk, h, res[1 + m]] = dig[m]
            k[:, :Nk, h, res[4]] = np.where(key_half(key) == 1, 7, -7)
            k[:, Nk:, h, res] = 7
            d0 = np.array(free)[(i + 11 * h) % len(free)]
            q[:, i, h, d0] = sg[d0]
            q[:, i, h, res[0]] = np.where((kind == 0) | (kind == 3), beta_of(i), (i // 4) % 5 - 2)
            for m in range(3):
                q[:, i, h, res[1 + m]] = np.where(kind == 1, 15 ** m, np.where(kind == 2, -(15 ** m), 0))
            q[:, i, h, res[4]] = np.where(kind == 3, HALF_GAIN, 0)
    elif sp.family == "onehot":
        assert Nq >= Nk
        kk = rng.integers(-7, 8, size=(B, rows, H, D)).astype(np.float64)
        kk[..., 0] = 7 * np.where(rng.random((B, rows, H)) < 0.5, 1.0, -1.0)
        k[:] = kk
        winner = i % Nk
        q[:] = kk[:, winner] * (2.0 ** ((i + 2 * (i // 32)) % 3))[None, :, None, None]
    else:
        assert Nq >= Nk and D == 64 and rows <= 64 * 5
        j = np.arange(rows)
        ca, cb = j % 64, (j % 64 + 1 + j // 64) % 64
        assert len({frozenset(p) for p in zip(ca.tolist(), cb.tolist())}) == rows
        for b in range(B):
            for h in range(H):
                k[b, j, h, ca] = 4 * np.where(rng.random(rows) < 0.5, 1.0, -1.0)
                k[b, j, h, cb] = 4 * np.where(rng.random(rows) < 0.5, 1.0, -1.0)
        winner = i % Nk
        q[:] = 2 * k[:, winner]
        do = rng.integers(1, 4, size=(B, Nq, H, D)) * np.stack([sgn0(np.arange(D), h + 1) for h in range(H)])[None, None]
    for b in range(B):
        for h in range(H):
            if sp.family != "bwd":   # the plant: a -7 among the real keys of V in every (batch, head)
                v[b, (2 * h + b + 1) % Nk, h, (5 * h) % D] = -7
            k[b, :, h] *= 2.0 ** jk_of(b, h)
            q[b, :, h] *= 2.0 ** -jk_of(b, h)
            v[b, :, h] *= 2.0 ** jv_of(b, h)
    t = torch.from_numpy
    return Case(sp, t(q), t(k), t(v), None if do is None else t(do), None if winner is None else t(winner), kind)


# ---- float64 reference --------------------------------------------------------------------------------------------------------------

@dataclass
class Ref:
    out: torch.Tensor     # [B, Nq, H * D] float64
    A: torch.Tensor       # the softmax-weighted mean of |v|, same shape
    logits: torch.Tensor  # [B, H, Nq, Nk] in exp2 units
    lse: torch.Tensor     # [B * H, Nq]: ln 2 (max + log2 l)
    p: torch.Tensor       # [B, H, Nq, Nk]


@functools.lru_cache(maxsize=8)
def _reference(sp: Spec) -> Ref:
    case = make_case(sp)
    k, v = case.k[:, :sp.Nk], case.v[:, :sp.Nk]
    s = torch.einsum("bqhd,bkhd->bhqk", case.q, k) * float(c_f32())
    mx = s.amax(-1, keepdim=True)
    p = torch.exp2(s - mx)
    l = p.sum(-1, keepdim=True)
    p = p / l
    shape = (sp.B, sp.Nq, sp.H * sp.D)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(shape)
    A = torch.einsum("bhqk,bkhd->bqhd", p, v.abs()).reshape(shape)
    lse = (math.log(2.0) * (mx + torch.log2(l))).reshape(sp.B * sp.H, sp.Nq)
    return Ref(out, A, s, lse, p)


def reference(case: Case) -> Ref:
    return _reference(case.spec)


def ratio(got, want, A):
    """max |got - want| / (2^-8 |want| + 2^-10 A) over ALL elements (NaN and inf count as infinite)."""
    r = (got.double() - want).abs() / (BAR_REL * want.abs() + BAR_ABS * A)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


def worst_ratio(got, ref: Ref) -> float:
    assert got.shape == ref.out.shape
    return ratio(got, ref.out, ref.A)


def onehot_target(case: Case) -> torch.Tensor:
    sp = case.spec
    return case.v[:, case.winner].reshape(sp.B, sp.Nq, sp.H * sp.D)


def tile_tops(case: Case):
    """[B, H, Nq, tiles] the maximum logit of every tile, and the same per key half [.., tiles, 2] (-inf where a half has no key)."""
    sp, s = case.spec, reference(case).logits
    nt = -(-sp.Nk // sp.tile)
    pad = torch.full(s.shape[:-1] + (nt * sp.tile - sp.Nk,), float("-inf"), dtype=s.dtype)
    s = torch.cat([s, pad], -1).reshape(s.shape[:-1] + (nt, sp.tile))
    hf = torch.from_numpy(key_half(np.arange(sp.tile))).bool()
    halves = torch.stack([s[..., ~hf].amax(-1), s[..., hf].amax(-1)], -1)
    return s.amax(-1), halves


def check_conditions(case: Case):
    """What makes float64 the exact answer on this case, and what the family promises; raises AssertionError otherwise."""
    sp = case.spec
    B, H, D, Nq, Nk = sp.B, sp.H, sp.D, sp.Nq, sp.Nk
    assert float(c_f32()) == 1.0, "scale * log2(e) must be exactly 1.0f"
    assert case.rows >= Nk + 8 and case.k.shape == case.v.shape == (B, case.rows, H, D), "8 padding rows inside the allocation"
    assert H >= 2 or D > 64
    for name, x, jf in (("k", case.k, jk_of), ("v", case.v, jv_of)):
        assert torch.equal(x.bfloat16().double(), x), f"{name} is not bf16"
        for b in range(B):
            for h in range(H):
                r = x[b, :, h] * 2.0 ** -jf(b, h)
                assert torch.equal(r, r.round()) and float(r.abs().max()) <= 7.0, f"{name}[{b}, :, {h}]: integers in [-7, 7]"
                assert float(r[:Nk].abs().max()) == 7.0 or sp.family == "bwd"
    assert (case.v != 0).all()
    assert jk_of(0, 0) != jk_of(0, 1) and jk_of(0, 0) != jk_of(1, 0) and all(jk_of(b, h) != jv_of(b, h) for b in range(B) for h in range(H))
    assert torch.equal(case.q.bfloat16().double(), case.q), "q is not bf16"
    ref = reference(case)
    s = ref.logits
    assert torch.equal(s, s.round()) and float(s.abs().max()) < 2 ** 23, "every logit is an integer number of exp2 units"
    top = s.amax(-1)
    pad = torch.einsum("bqhd,bkhd->bhqk", case.q, case.k[:, Nk:]).amax(-1)
    if sp.family == "mix":
        kind = torch.from_numpy(case.kind)
        assert all(set(case.kind[r:r + 32].tolist()) == {0, 1, 2, 3} for r in range(0, Nq - 31, 32)), "four kinds in every 32-query block"
        band = s[:, :, kind == 0]
        L = band.amax(-1)
        assert float((L[..., None] - band).max()) <= 6, "band rows: every logit within 6 units of the row maximum"
        want_L = torch.from_numpy(7 + beta_of(np.arange(Nq)))[kind == 0].double()
        assert torch.equal(L, want_L.expand_as(L))
        nb = int((kind == 0).sum())
        if nb >= len(BETAS):
            assert (L <= -10).any() and ((L >= 0) & (L <= 8)).any() and (L >= 20).any()
        levels = (L[..., None] - band)
        assert all(int((levels == d).sum(-1).min()) >= 2 for d in range(7)) or Nk < 64, "many keys share each level"
        # bit budget of the band rows: p is 2^-6 .. 1 of the row maximum (times one power of two where m_ref stands below it), so in units
        # of 2^-6 every partial sum of l is an integer below Nk 2^6, and in units of 2^(jv - 6) every partial sum of O one below 7 Nk 2^6
        bits_l, bits_o = 6 + math.ceil(math.log2(Nk)), 6 + 3 + math.ceil(math.log2(Nk))
        assert bits_l <= bits_o <= 24, f"band rows: l needs {bits_l} bits, O {bits_o}"
        tops, halves = tile_tops(case)
        nt = tops.shape[-1]
        if nt >= 2:
            up, down = tops[:, :, kind == 1], tops[:, :, kind == 2]
            rise = up[..., 1:] - up[..., :-1]
            assert float(rise.min()) >= 3 and ((rise <= 8).any() or nt <= 3), "up rows: the tile maximum rises by 3 .. 8 (no move)"
            assert ((rise >= 9) & (rise <= 12) | (rise == 20)).any(), "... and by 9 .. 12 (a move)"
            assert torch.equal(s[:, :, kind == 1].argmax(-1) // sp.tile, torch.full_like(up[..., 0], nt - 1).long()), "the last tile wins"
            assert float((down[..., :1] - down[..., 1:]).min()) >= 10, "down rows: later tiles sit 10 and more units below tile 0"
            dbl = min(DOUBLE, nt - 1)
            h_up = halves[:, :, kind == 1]
            full = h_up[..., dbl, 1] > float("-inf")
            assert bool(((h_up[..., dbl, 0] - up[..., dbl - 1] > 8) & (h_up[..., dbl, 1] - h_up[..., dbl, 0] > 8))[full].all()), "the double step"
            whole = Nk // sp.tile   # over the whole tiles: the maximum sits in both key halves and in both 32-key (16-key) blocks in turn
            if whole >= 3:
                lead = h_up[..., :whole, 1] > h_up[..., :whole, 0]
                assert bool((lead.any(-1) & (~lead).any(-1)).all()), "the rise alternates between the key halves"
                su = s[:, :, kind == 1][..., :whole * sp.tile].reshape(B, H, -1, whole, sp.tile)
                blk = su.argmax(-1) // (sp.tile // 2)
                assert bool(((blk == 0).any(-1) & (blk == 1).any(-1)).all()), "... and between the lower and upper keys of the tile"
        hrows = halves[:, :, kind == 3]
        assert float((hrows[..., 0, 1] - hrows[..., 0, 0]).min()) >= 128, "half rows: the upper key half > 128 units above the lower"
        assert float(((pad > top).double()).mean()) > 0.5, "the padding must beat the real keys of most rows"
        assert (top <= -10).any(), "rows whose every logit is below zero (a zero padding key would win them)"
    else:
        win = case.winner[None, None, :].expand(B, H, Nq)
        second = s.clone().scatter_(-1, win[..., None], float("-inf"))
        assert torch.equal(s.argmax(-1), win)
        margin = 24 if sp.family == "onehot" else 32
        assert float((top - second.amax(-1)).min()) >= margin and float((top - pad).min()) >= margin, "the winner's margin"
        assert set(case.winner.tolist()) == set(range(Nk)), "every key is the winner of some row"
        if sp.family == "bwd":
            assert float(s.abs().max()) <= 64 and float(pad.abs().max()) <= 64
            g = reference_bwd(case)
            assert float((g.dq.abs() / (BAR_ABS * g.A_dq)).max()) < 0.01 and float((g.dk.abs() / (BAR_ABS * g.A_dk)).max()) < 0.01, \
                "float64 dQ and dK far below the absolute part of the bar"
            assert torch.equal(g.dv_target.bfloat16().double(), g.dv_target) and (g.dv_target != 0).all()


# ---- fp32 emulations of the three forward pipelines, with the fault models -------------------------------------------------------------

KV_FAULTS = ("v_swap4", "k_chan_swap", "k_head", "v_head", "k_batch", "v_batch")
TILE_FAULTS = ("tile_late", "drop_key", "dup_key", "pad_zero", "pad_rows")
LAZY_FAULTS = ("mref_no_l", "mref_no_o", "max_lower_half")
SINGLE_FAULTS = ("split_swap", "qscale_ignored")


def pow2(x):
    """2^x in fp32 for integer-valued x, exactly (-inf -> 0, beyond fp32 -> inf)."""
    xi = torch.nan_to_num(x, nan=0.0, posinf=300.0, neginf=-300.0).clamp(-300, 300).round().int()
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), xi)


def _f32_inputs(case: Case, fault):
    """q [B, H, Nq, D], k, v [B, H, rows, D] fp32 with the faults that act on K / V as a whole."""
    sp = case.spec
    q, k, v = (x.float().permute(0, 2, 1, 3).contiguous() for x in (case.q, case.k, case.v))
    if fault == "v_swap4":   # members 1 and 2 of every complete group of four real keys
        g = sp.Nk // 4 * 4
        idx = torch.arange(g).view(-1, 4)[:, [0, 2, 1, 3]].reshape(-1)
        v[:, :, :g] = v[:, :, idx]
    if fault == "k_chan_swap":
        for a, b in ((2, 3), (17, 30), (40, 41), (55, 62)):
            k[..., [a, b]] = k[..., [b, a]]
    if fault == "k_head":
        k = k.roll(-1, 1)
    if fault == "v_head":
        v = v.roll(-1, 1)
    if fault == "k_batch":
        k = k.roll(-1, 0)
    if fault == "v_batch":
        v = v.roll(-1, 0)
    return q, k, v


def _tile(k, v, t, tile, nk, fault):
    """K, V of tile t as the kernels see them (keys >= Nk zero-filled) and the mask of its valid keys."""
    lo = t * tile
    nt = -(-nk // tile)
    kt, vt = k[:, :, lo:lo + tile].clone(), v[:, :, lo:lo + tile].clone()
    valid = torch.arange(lo, lo + tile) < nk
    if kt.shape[2] < tile:
        z = torch.zeros(kt.shape[:2] + (tile - kt.shape[2], kt.shape[3]))
        kt, vt = torch.cat([kt, z], 2), torch.cat([vt, z], 2)
    if fault != "pad_rows":
        kt[:, :, ~valid] = 0
        vt[:, :, ~valid] = 0
    if fault in ("pad_zero", "pad_rows") and t == nt - 1 and nk % tile:
        valid[nk - lo] = True
    if fault == "drop_key":
        valid[min(tile, nk - lo) - 1] = False
    return kt, vt, valid


def late_tile(nk, tile):
    """tile_late: tile 1 (tile 0 where there are only two) arrives as the tile one slot on, for one wave: the 32-query block whose
    one-hot winners it holds."""
    return min(1, -(-nk // tile) - 2)


def _sum(p, order):
    return p.sum(-1) if order == 0 else p.flip(-1).reshape(p.shape[:-1] + (4, -1)).sum(-1).sum(-1)


def _pv(p, v, order):
    if order == 0:
        return torch.matmul(p, v)
    h = p.shape[-1] // 2   # the other order: the upper half of the tile's keys first, each half its own product
    return torch.matmul(p[..., h:], v[..., h:, :]) + torch.matmul(p[..., :h], v[..., :h, :])


def _scores(case, q, k, v, t, tile, fault, qscale=1.0):
    """Scores of tile t [B, H, Nq, tile] (masked keys -inf) and its V (tile_late: both tiles' V and the rows that see the late one)."""
    nk = case.spec.Nk
    kt, vt, valid = _tile(k, v, t, tile, nk, fault)
    s = torch.matmul(q, kt.transpose(-1, -2)) * qscale
    if fault == "tile_late" and t == late_tile(nk, tile):
        k2, v2, valid2 = _tile(k, v, t + 1, tile, nk, None)
        s2 = torch.matmul(q, k2.transpose(-1, -2)) * qscale
        s2 = s2.masked_fill(~valid2, float("-inf"))
        s = s.masked_fill(~valid, float("-inf"))
        blk = (torch.arange(case.spec.Nq) // 32 == t * tile // 32)[:, None]
        s = torch.where(blk, s2, s)
        vt = (vt, v2, blk)
        return s, vt
    return s.masked_fill(~valid, float("-inf")), vt


def _accumulate(O, p, vt, order):
    pb = p.bfloat16().float()
    if isinstance(vt, tuple):
        v1, v2, blk = vt
        return O + torch.where(blk, _pv(pb, v2, order), _pv(pb, v1, order))
    return O + _pv(pb, vt, order)


def _dup(p, t, fault):
    if fault == "dup_key" and t == 0:
        p = p.clone()
        p[..., 5] *= 2
    return p


def _finish(case, O, l, lse2, round_out, want_lse):
    sp = case.spec
    o = (O / l[..., None]).permute(0, 2, 1, 3).reshape(sp.B, sp.Nq, sp.H * sp.D)
    o = o.bfloat16() if round_out else o
    if want_lse:
        return o, (lse2 * float(LN2_F32)).reshape(sp.B * sp.H, sp.Nq)
    return o


def emulate_eager(case: Case, fault=None, order=0, round_out=True, want_lse=False):
    """attn_fwd_kernel in fp32 torch: the running maximum follows every 64-key tile, alpha = exp2(m_old - m_new) rescales l and O at every
    tile, the row sum is that of the fp32 p, P is rounded to bf16, o = O / l; lse = (m c + log2f(l)) ln 2."""
    sp = case.spec
    q, k, v = _f32_inputs(case, fault)
    nt = -(-sp.Nk // 64)
    m = torch.full((sp.B, sp.H, sp.Nq), float("-inf"))
    l = torch.zeros(sp.B, sp.H, sp.Nq)
    O = torch.zeros(sp.B, sp.H, sp.Nq, sp.D)
    for t in range(nt):
        s, vt = _scores(case, q, k, v, t, 64, fault)
        m_new = torch.maximum(m, s.amax(-1))
        alpha = pow2(m - m_new)
        p = _dup(pow2(s - m_new[..., None]), t, fault)
        l = l * alpha + _sum(p, order)
        O = _accumulate(O * alpha[..., None], p, vt, order)
        m = m_new
    return _finish(case, O, l, m * float(c_f32()) + torch.log2(l), round_out, want_lse)


def emulate_lazy(case: Case, fault=None, order=0, round_out=True, want_lse=False, count=None):
    """attn_self_kernel in fp32 torch: m_ref starts at 0, follows the .ref key half (keys with key % 8 < 4) of tile 0 wherever it stands
    and of a later tile only when that exceeds m_ref by more than 8 units (move_ref); catch_up then moves it on by a whole number of
    units when the maximum over both halves still stands more than 8 above it.  p = exp2(s - m_ref) unnormalised (up to 2^8), fp32 row
    sum, P rounded to bf16, o = O / l; lse = (log2f(l) + m_ref) ln 2.  count: a dict that receives how many rows took each path."""
    sp = case.spec
    assert sp.Nk % 64 == 0
    q, k, v = _f32_inputs(case, fault)
    hf = torch.from_numpy(key_half(np.arange(64))).bool()
    m = torch.zeros(sp.B, sp.H, sp.Nq)
    l = torch.zeros(sp.B, sp.H, sp.Nq)
    O = torch.zeros(sp.B, sp.H, sp.Nq, sp.D)
    moves = catches = 0
    for t in range(sp.Nk // 64):
        s, vt = _scores(case, q, k, v, t, 64, fault)
        s = s - m[..., None]
        ref = s[..., ~hf].amax(-1)
        both = ref if fault == "max_lower_half" else s.amax(-1)
        d = ref if t == 0 else torch.where(ref > SLACK, ref, torch.zeros_like(ref))
        rest = both - d
        n = torch.where(rest > SLACK, rest.floor(), torch.zeros_like(rest))
        if t > 0:
            moves += int((d > 0).sum())
        catches += int((n > 0).sum())
        a1, a2 = pow2(-d.clamp_min(0)), pow2(-n)
        if not (fault == "mref_no_l" and t > 0):
            l = l * a1 * a2
        if not (fault == "mref_no_o" and t > 0):
            O = O * (a1 * a2)[..., None]
        m = m + d + n
        p = _dup(pow2(s - (d + n)[..., None]), t, fault)
        l = l + _sum(p, order)
        O = _accumulate(O, p, vt, order)
    if count is not None:
        count.update(moves=moves, catch_ups=catches)
    return _finish(case, O, l, torch.log2(l) + m, round_out, want_lse)


def emulate_single(case: Case, fault=None, order=0, round_out=True, qscale=1.0, qmul=1.0):
    """attn_single_kernel + attn_single_combine_kernel in fp32 torch: 32-key tiles with an eager maximum, s = (q . k) qscale, per split a
    normalised part O / l and lse2 = m + log2f(l); the combine weighs the parts by 2^(lse2 - max lse2).  qmul multiplies q (exactly)."""
    sp = case.spec
    q, k, v = _f32_inputs(case, fault)
    q = q * qmul
    if fault == "qscale_ignored":
        qscale = 1.0
    ns, per = single_splits(sp.Nk)
    parts, lse2 = [], []
    for sidx in range(ns):
        t0, t1 = sidx * per // SINGLE_KT, min((sidx + 1) * per, -(-sp.Nk // SINGLE_KT) * SINGLE_KT) // SINGLE_KT
        m = torch.full((sp.B, sp.H, sp.Nq), float("-inf"))
        l = torch.zeros(sp.B, sp.H, sp.Nq)
        O = torch.zeros(sp.B, sp.H, sp.Nq, sp.D)
        for t in range(t0, t1):
            s, vt = _scores(case, q, k, v, t, SINGLE_KT, fault, qscale)
            m_new = torch.maximum(m, s.amax(-1))
            alpha = pow2(m - m_new)
            p = _dup(pow2(s - m_new[..., None]), t, fault)
            l = l * alpha + _sum(p, order)
            O = _accumulate(O * alpha[..., None], p, vt, order)
            m = m_new
        parts.append(O * (1.0 / l)[..., None])
        lse2.append(m + torch.log2(l))
    if ns == 1:
        o = parts[0]
    else:
        L = torch.stack(lse2)
        w = torch.exp2(L - L.amax(0))
        if fault == "split_swap":
            w = w[[1, 0] + list(range(2, ns))]
        order_s = range(ns) if order == 0 else range(ns - 1, -1, -1)
        tot, wsum = torch.zeros_like(parts[0]), torch.zeros_like(w[0])
        for sidx in order_s:
            tot = tot + w[sidx][..., None] * parts[sidx]
            wsum = wsum + w[sidx]
        o = tot * (1.0 / wsum)[..., None]
    o = o.permute(0, 2, 1, 3).reshape(sp.B, sp.Nq, sp.H * sp.D)
    return o.bfloat16() if round_out else o


def faults_for(sp: Spec, pipeline: str):
    """The fault models a case must expose on a pipeline ("eager", "lazy", "single").  The one-hot family answers to what moves the
    winner or its v row; a key counted twice (in l and in O alike) or a maximum that moved badly leaves a one-hot row as it is."""
    nt = -(-sp.Nk // (SINGLE_KT if pipeline == "single" else 64))
    f = ["v_swap4", "drop_key", "k_batch", "v_batch"] if sp.B >= 2 else ["v_swap4", "drop_key"]
    if sp.H >= 2:
        f += ["k_head", "v_head"]
    if nt >= 2:
        f.append("tile_late")
    if sp.family == "mix":
        f += ["k_chan_swap", "dup_key"]
        if sp.Nk % (SINGLE_KT if pipeline == "single" else 64):
            f += ["pad_zero", "pad_rows"]
        if pipeline == "lazy":
            f += list(LAZY_FAULTS)
        if pipeline == "single" and single_splits(sp.Nk)[0] >= 2:
            f.append("split_swap")
    return f


# ---- the backward: float64 reference, the bar's weighted means, an fp32 emulation with its fault models ----------------------------------

@dataclass
class RefBwd:
    dq: torch.Tensor          # [B, Nq, H * 64] float64
    dk: torch.Tensor          # [B, Nk, H * 64]
    dv: torch.Tensor
    A_dq: torch.Tensor        # the weighted mean of the magnitudes of dQ's own products: scale sum_k P (|dO| . |v_k| + |dO| . |o|) max_d |k_k|
    A_dk: torch.Tensor        # scale sum_i P (|dO_i| . |v| + |dO_i| . |o_i|) max_d |q_i|
    dv_target: torch.Tensor   # [B, Nk, H * 64]: the sum of the dO rows each key wins


@functools.lru_cache(maxsize=4)
def _reference_bwd(sp: Spec) -> RefBwd:
    case = make_case(sp)
    ref = reference(case)
    B, H, D, Nq, Nk = sp.B, sp.H, sp.D, sp.Nq, sp.Nk
    k, v, do, q = case.k[:, :Nk], case.v[:, :Nk], case.do, case.q
    P = ref.p
    o = ref.out.reshape(B, Nq, H, D)
    dP = torch.einsum("bqhd,bkhd->bhqk", do, v)
    delta = (do * o).sum(-1).permute(0, 2, 1)
    dS = P * (dP - delta[..., None])
    mag = P * (torch.einsum("bqhd,bkhd->bhqk", do.abs(), v.abs()) + (do.abs() * o.abs()).sum(-1).permute(0, 2, 1)[..., None])
    flat = lambda x, n: x.reshape(B, n, H * D)
    dq = flat(torch.einsum("bhqk,bkhd->bqhd", dS, k) * SCALE, Nq)
    dk = flat(torch.einsum("bhqk,bqhd->bkhd", dS, q) * SCALE, Nk)
    dv = flat(torch.einsum("bhqk,bqhd->bkhd", P, do), Nk)
    # (each streamed row at its largest channel: K, and with it q, is sparse in this family, and the bf16 rounding of dS, 2^-9 of every
    # product, has to fit under 2^-10 A on the channels where only the losing keys meet)
    A_dq = flat(torch.einsum("bhqk,bkhd->bqhd", mag, k.abs().amax(-1, keepdim=True).expand_as(k)) * SCALE, Nq)
    A_dk = flat(torch.einsum("bhqk,bqhd->bkhd", mag, q.abs().amax(-1, keepdim=True).expand_as(q)) * SCALE, Nk)
    onehot = torch.zeros(Nq, Nk, dtype=torch.float64)
    onehot[torch.arange(Nq), case.winner] = 1
    target = flat(torch.einsum("qk,bqhd->bkhd", onehot, do), Nk)
    return RefBwd(dq, dk, dv, A_dq, A_dk, target)


def reference_bwd(case: Case) -> RefBwd:
    return _reference_bwd(case.spec)


BWD_FAULTS = ("dv_perm4", "delta_neighbour")


def emulate_bwd(case: Case, fault=None, round_out=True):
    """attn_bwd_kernel in fp32 torch from the emulated forward's bf16 o and fp32 lse: lse2 = lse log2(e), P = exp2(s c - lse2), delta =
    rowsum(dO o), dS = P (dP - delta), P and dS rounded to bf16, fp32 products, dQ and dK times the scale, one bf16 rounding.
    -> (dq, dk, dv)"""
    sp = case.spec
    B, H, D, Nq, Nk = sp.B, sp.H, sp.D, sp.Nq, sp.Nk
    o, lse = emulate_eager(case, want_lse=True)
    q, k, v = _f32_inputs(case, None)
    k, v = k[:, :, :Nk], v[:, :, :Nk]
    do = case.do.float().permute(0, 2, 1, 3)
    o = o.float().reshape(B, Nq, H, D).permute(0, 2, 1, 3)
    lse2 = lse.reshape(B, H, Nq) * float(LOG2E_F32)
    s = torch.matmul(q, k.transpose(-1, -2))
    P = torch.exp2(s * float(c_f32()) - lse2[..., None])
    delta = (do * o).sum(-1)
    if fault == "delta_neighbour":
        delta = delta.roll(-1, -1)
    dS = (P * (torch.matmul(do, v.transpose(-1, -2)) - delta[..., None])).bfloat16().float()
    Pb = P.bfloat16().float()
    dq = torch.matmul(dS, k) * float(np.float32(SCALE))
    dk = torch.matmul(dS.transpose(-1, -2), q) * float(np.float32(SCALE))
    dv = torch.matmul(Pb.transpose(-1, -2), do)
    if fault == "dv_perm4":
        g = Nk // 4 * 4
        idx = torch.arange(g).view(-1, 4)[:, [0, 2, 1, 3]].reshape(-1)
        dv[:, :, :g] = dv[:, :, idx]
    flat = lambda x: x.permute(0, 2, 1, 3).reshape(B, x.shape[2], H * D)
    outs = tuple(flat(x) for x in (dq, dk, dv))
    return tuple(x.bfloat16() for x in outs) if round_out else outs


def bwd_ratios(dq, dk, dv, g: RefBwd):
    """(worst dQ ratio, worst dK ratio, dV bit-equal to the per-key sums of dO)."""
    return ratio(dq, g.dq, g.A_dq), ratio(dk, g.dk, g.A_dk), bool(torch.equal(dv.bfloat16(), g.dv_target.bfloat16()))


# ---- lse ---------------------------------------------------------------------------------------------------------------------------

LSE_REL = 7.2e-7   # 4 x the worst |fp32 restatement - float64| / (|lse| + 1) over the forward cases (tests/test_attn_tile_cpu.py holds it there)


def lse_ratio(got, ref: Ref, rel=LSE_REL):
    r = (got.double() - ref.lse).abs() / (rel * (ref.lse.abs() + 1))
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


# ---- which kernel a call reaches: the dispatch of attn_launch (csrc/attn_fwd.hip), restated -------------------------------------------

def route(entry, B, H, Nq, Nk, attn_self=None, attn_fast=None, aligned=True, k_row_stride=None):
    """entry: "plain" | "lse" | "xformers" (cd360_attn_fwd_bf16 and what forwards to it) or "prescaled".  aligned: the output's strides are
    multiples of 8 elements and its address of 16 bytes.  -> "smallk", "gen1-fast", "gen1-guarded", "self<1,4>", "self<2,8>", "self<1,8>"."""
    if Nk <= 96 and aligned:
        return "smallk"
    span_ok = k_row_stride is None or Nk * k_row_stride * 2 < 2 ** 31
    gen2 = Nk % 64 == 0 and Nq % 128 == 0 and span_ok and aligned
    pick = -1 if entry == "prescaled" else 0
    if attn_self is not None and attn_self >= 0:
        pick = attn_self
    if gen2 and pick:
        wide = Nq % 512 == 0 and B * H * (Nq // 512) >= 240
        if pick > 0:
            wide = pick == 2 and Nq % 512 == 0
        if pick == 3 and Nq % 256 == 0:
            return "self<1,8>"
        return "self<2,8>" if wide else "self<1,4>"
    return "gen1-fast" if span_ok and attn_fast != 0 else "gen1-guarded"


FORCED = {1: "self<1,4>", 2: "self<2,8>", 3: "self<1,8>"}


# ---- the case lists of the GPU tests ---------------------------------------------------------------------------------------------------

FAMILIES = ("mix", "onehot")
GEN1_SHAPES = ((200, 97), (200, 200), (333, 333), (256, 256))
SELF_SHAPES = {1: (256, 640), 3: (256, 768), 2: (512, 1024)}
# (test id, entry, tuning, Nq, Nk, the kernel the case is named for)
FORWARD = [(f"gen1-fast{fast}-{nq}x{nk}", "plain", dict(attn_self=0, attn_fast=fast), nq, nk, "gen1-fast" if fast else "gen1-guarded")
           for fast in (1, 0) for nq, nk in GEN1_SHAPES]
FORWARD += [(f"attn_self{g}-{n}x{n}", "plain", dict(attn_self=g), n, n, FORCED[g]) for g in (1, 3, 2) for n in SELF_SHAPES[g]]
FORWARD += [("prescaled-by-shape-256x256", "prescaled", {}, 256, 256, "self<1,4>"), ("prescaled-by-shape-512x512", "prescaled", {}, 512, 512, "self<1,4>"),
            ("prescaled-by-shape-200x200", "prescaled", {}, 200, 200, "gen1-fast"), ("xformers-bh4-200x200", "xformers", {}, 200, 200, "gen1-fast")]
SINGLE = ((2, 256, 512), (1, 520, 320), (1, 1024, 128), (1, 600, 512))   # (b, n, D)
SINGLE_SPLITS = {256: 1, 520: 2, 1024: 4, 600: 2}
BWD_SHAPES = ((200, 200), (256, 256), (200, 97))


def tiled_spec(family, nq, nk):
    return Spec(family, nq, nk)


def single_spec(family, b, n, d):
    return Spec(family, n, n, 1, b, d, SINGLE_KT)


def bwd_spec(nq, nk):
    return Spec("bwd", nq, nk)


def pipeline_of(kernel):
    return "lazy" if kernel.startswith("self") else "eager"


def forward_specs():
    """(spec, pipeline) of every tiled forward case the GPU file runs, once."""
    seen = {}
    for _, _, _, nq, nk, kernel in FORWARD:
        for f in FAMILIES:
            seen[(tiled_spec(f, nq, nk), pipeline_of(kernel))] = True
    return list(seen)
