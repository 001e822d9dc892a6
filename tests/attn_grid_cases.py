"""Inputs on which a float64 softmax attention is the exact answer of the <= 96-key attention kernels, bf16 and fp8 alike, up to the one
bf16 rounding of the output (CPU only, no HIP import; tests/test_attn_grid_cpu.py checks the builders, tests/test_attn_grid_gpu.py
runs the kernels).

Two families, both with K and V integers in [-7, 7] times a power of two per (batch, head) -- 2^j, j in {0, 1, -1}, different for K and
V, for neighbouring heads and for neighbouring batch elements -- and a +-7 planted in every (batch, head) of K and of V, so amax / 448 is
the power of two 2^(j - 6) and every scaled element is 64 n, an e4m3 value (v holds no zero, so A >= 2^j):

  grid     q is sparse: per token and head channel d0 holds +-7 2^i and channel d1 holds e 2^i, |e| <= 3, the rest is zero; d0 and d1
           cycle over the 64 channels with the token, i (1, 2 or 3, so that every logit is an integer) varies inside each 32-token
           block and between blocks.  The per-token e4m3 q (max -> 448) is exact, the scale passed through the C ABI makes
           scale * log2(e) exactly 1.0f, so every p = 2^(s - max) is a power of two: exact in bf16, exact in e4m3 (as p 2^8) down to
           2^-17.  One channel per head (`anti`) is negative on every real key: its tokens have every logit below zero, so a padding
           key that arrives as zeros and is not masked takes the row.  k rows >= Nk are attractive padding (they beat the real keys of
           most tokens), v rows >= Nk are 7.
  onehot   q is dense: the token's winning key row itself (integers in [-7, 7], maximum 7) times 2^i; the winner is >= 24 units
           above every other key and above the padding, cycles over all keys with the token, and v has no zero, so the output is
           bf16(v_winner) bit for bit.

The projection is a signed selection: W [N, K], row n = +-1 at column pi(n), so q = +-a[pi] exactly.  With dup > 0 k and v hold B + dup
batch elements and output batch B + i is query batch B - dup + i on the keys of batch B + i.

kv_image restates the layout of the packed e4m3 image from the comment above kv_pack_fp8_kernel (csrc/gemm8p.hip)."""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

D = 64
SLOTS = 96           # key slots of the packed image and of the widest epilogue
IMAGE_BYTES = 96 * 64 + 64 * 128
SCALE = float(np.float32(0.6931472))
LOG2E_F32 = np.float32(1.4426950408889634)
J = (0, 1, -1)
BAR_REL, BAR_ABS = 2.0 ** -8, 2.0 ** -10


def jk_of(b, h):
    return J[(b + h) % 3]


def jv_of(b, h):
    return J[(b + h + 1) % 3]


def anti_channel(h):
    return (7 + 13 * h) % 64


def sgn0(d, h):
    return np.where((3 * d + h) % 5 < 3, 1.0, -1.0)


def q_exponent(t, imode):
    """i of token t: 'vary' changes inside every 32-token block and between a token and the one 32 rows on; an integer pins it."""
    t = np.asarray(t)
    return 1 + (t + 2 * (t // 32)) % 3 if imode == "vary" else np.full(t.shape, 1 + int(imode))


@dataclass(frozen=True)
class Spec:
    family: str      # "grid" | "onehot"
    N: int           # heads * 64
    K: int           # projection depth, >= N
    Nk: int
    dup: int = 0
    Nq: int = 256
    B: int = 2
    imode: object = "vary"   # "vary" or 0, 1, 2 (i = 1 + imode for every token)


def spec_id(sp: Spec) -> str:
    return f"{sp.family}-N{sp.N}-K{sp.K}-nk{sp.Nk}-dup{sp.dup}-nq{sp.Nq}-i{sp.imode}"


@dataclass
class Case:
    spec: Spec
    a: torch.Tensor      # [B, Nq, K] float64: the projection's input
    w: torch.Tensor      # [N, K] float64, one +-1 per row
    q: torch.Tensor      # [B, Nq, H, 64] float64 = a W^T
    k: torch.Tensor      # [B + dup, rows, H, 64] float64, rows >= 96: padding included
    v: torch.Tensor
    qi: torch.Tensor     # [B, Nq] int: exponent i of the token
    winner: Optional[torch.Tensor]   # onehot: [B + dup, Nq] key index per OUTPUT batch element

    @property
    def H(self):
        return self.spec.N // D

    @property
    def rows(self):
        return self.k.shape[1]


def out_batches(sp: Spec):
    """(query batch, key batch) of every output batch element."""
    return [(b, b) for b in range(sp.B)] + [(sp.B - sp.dup + i, sp.B + i) for i in range(sp.dup)]


def _ints(rng, shape, small=0.7):
    """Integers in [-6, 6] (the 7s are planted): mostly -1, 0, 1 (close logits: weights spread over many keys), the rest uniform."""
    x = rng.integers(-6, 7, size=shape)
    s = rng.integers(-1, 2, size=shape)
    return np.where(rng.random(shape) < small, s, x).astype(np.float64)


@functools.lru_cache(maxsize=16)
def make_case(sp: Spec) -> Case:
    assert sp.family in ("grid", "onehot") and sp.N % D == 0 and sp.K >= sp.N and 1 <= sp.Nk <= SLOTS and 0 <= sp.dup <= sp.B
    B, H, Nq, Nk, nb = sp.B, sp.N // D, sp.Nq, sp.Nk, sp.B + sp.dup
    rows = SLOTS + 8
    rng = np.random.default_rng(1000 * Nk + sp.N + 7 * sp.dup + (17 if sp.family == "grid" else 0))
    t = np.arange(Nq)
    k = np.zeros((nb, rows, H, D))
    v = np.zeros((nb, rows, H, D))
    q = np.zeros((B, Nq, H, D))
    qi = np.stack([q_exponent(t, sp.imode)] * B)
    winner = None
    if sp.family == "grid":
        k[:, :Nk] = _ints(rng, (nb, Nk, H, D))
        v[:, :Nk] = rng.integers(1, 7, size=(nb, Nk, H, D)) * np.where(rng.random((nb, Nk, H, D)) < 0.5, 1.0, -1.0)  # no zero: A >= 2^j
        for h in range(H):
            k[:, :Nk, h, anti_channel(h)] = -sgn0(anti_channel(h), h) * (1 + np.arange(Nk) % 3)
            k[:, Nk:, h, :] = 7 * sgn0(np.arange(D), h)
        v[:, Nk:] = 7
        for h in range(H):
            d0 = (t + 11 * h) % D
            d1 = (d0 + 1 + (t // D) % 62) % D
            e = rng.integers(0, 4, size=(B, Nq)) * sgn0(d1, h)   # (signed like the padding row: 49 + 7 |e| there, <= 42 + 6 |e| on a real key)
            e[:, d0 == anti_channel(h)] = 0
            for b in range(B):
                q[b, t, h, d1] = e[b]
                q[b, t, h, d0] = 7 * sgn0(d0, h)
    else:
        kk = rng.integers(-7, 8, size=(nb, rows, H, D)).astype(np.float64)
        kk[..., 0] = 7 * np.where(rng.random((nb, rows, H)) < 0.5, 1.0, -1.0)   # every key row's maximum is 7: q = the row
        if sp.dup:  # the key sets a de-duplicated query meets hold the same rows, rotated by one key: it wins in both
            for i in range(sp.dup):
                kk[B + i, :Nk] = np.roll(kk[B - sp.dup + i, :Nk], 1, axis=0)
        k[:] = kk
        vv = rng.integers(1, 7, size=(nb, rows, H, D)) * np.where(rng.random((nb, rows, H, D)) < 0.5, 1.0, -1.0)
        v[:] = vv
        win = t % Nk
        winner = np.stack([win if kb < B else (win + 1) % Nk for _, kb in out_batches(sp)])
        winner = torch.from_numpy(winner)
    # the plants: +-7 in every (batch, head) of K and V among the real keys (not on the anti channel)
    for b in range(nb):
        for h in range(H):
            if sp.family == "grid":
                k[b, (h + b) % Nk, h, (anti_channel(h) + 1) % D] = 7
            v[b, (2 * h + b + 1) % Nk, h, (5 * h) % D] = -7
            k[b, :, h] *= 2.0 ** jk_of(b, h)
            v[b, :, h] *= 2.0 ** jv_of(b, h)
    if sp.family == "onehot":  # q is the unscaled winning row
        for b in range(B):
            for h in range(H):
                q[b, :, h] = k[b, t % Nk, h] * 2.0 ** -jk_of(b, h)
    q *= (2.0 ** qi)[:, :, None, None]
    # signed selection: row n of W has sigma(n) at column pi(n); a[pi(n)] = sigma(n) q[n], the columns W never selects hold other integers
    n = np.arange(sp.N)
    pi = (5 * n + 3) % sp.K
    sigma = np.where(n % 3 == 1, -1.0, 1.0)
    assert len(set(pi.tolist())) == sp.N and (pi != n).any()
    w = np.zeros((sp.N, sp.K))
    w[n, pi] = sigma
    a = rng.integers(-7, 8, size=(B, Nq, sp.K)).astype(np.float64)
    a[:, :, pi] = q.reshape(B, Nq, sp.N) * sigma
    case = Case(sp, *(torch.from_numpy(x) for x in (a, w, q, k, v)), torch.from_numpy(qi), winner)
    assert torch.equal(case.a @ case.w.T, case.q.reshape(B, Nq, sp.N))
    return case


# ---- float64 reference --------------------------------------------------------------------------------------------------------------

@dataclass
class Ref:
    out: torch.Tensor     # [B + dup, Nq, H * 64] float64
    A: torch.Tensor       # the softmax-weighted mean of |v|, same shape
    logits: torch.Tensor  # [B + dup, H, Nq, Nk] in exp2 units


def c_f32():
    """scale * log2(e) as the entry points form it, in fp32."""
    return np.float32(SCALE) * LOG2E_F32


def gather(case: Case, x_q, x_kv):
    """q-side / key-side tensors per output batch element."""
    qb = [p[0] for p in out_batches(case.spec)]
    kb = [p[1] for p in out_batches(case.spec)]
    return x_q[qb], x_kv[kb]


@functools.lru_cache(maxsize=16)
def _reference(sp: Spec) -> Ref:
    case = make_case(sp)
    q, k = gather(case, case.q, case.k)
    _, v = gather(case, case.q, case.v)
    k, v = k[:, :sp.Nk], v[:, :sp.Nk]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * float(c_f32())
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(len(q), sp.Nq, sp.N)
    A = torch.einsum("bhqk,bkhd->bqhd", p, v.abs()).reshape(len(q), sp.Nq, sp.N)
    return Ref(out, A, s)


def reference(case: Case) -> Ref:
    return _reference(case.spec)


def bar(ref: Ref):
    return BAR_REL * ref.out.abs() + BAR_ABS * ref.A


def worst_ratio(got: torch.Tensor, ref: Ref) -> float:
    """max |got - ref| / bar over the elements (NaN counts as infinite)."""
    r = (got.double() - ref.out).abs() / bar(ref)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def is_e4m3(x: torch.Tensor) -> bool:
    x = x.float()
    return bool(torch.equal(x.to(torch.float8_e4m3fn).float(), x))


def check_conditions(case: Case):
    """What makes float64 the exact answer on this case; raises AssertionError otherwise."""
    sp, H, nb = case.spec, case.H, case.spec.B + case.spec.dup
    assert float(c_f32()) == 1.0, "scale * log2(e) must be exactly 1.0f"
    assert case.rows >= SLOTS and case.k.shape == case.v.shape == (nb, case.rows, H, D)
    for name, x, jf in (("k", case.k, jk_of), ("v", case.v, jv_of)):
        assert torch.equal(x.bfloat16().double(), x), f"{name} is not bf16"
        for b in range(nb):
            for h in range(H):
                r = x[b, :sp.Nk, h] * 2.0 ** -jf(b, h)
                assert torch.equal(r, r.round()) and float(r.abs().max()) == 7.0, f"{name}[{b}, :, {h}]: integers in [-7, 7] with a 7"
                assert is_e4m3(x[b, :sp.Nk, h] * (448.0 / (7 * 2.0 ** jf(b, h))))
        assert jf(0, 0) != jf(0, 1) and jf(0, 0) != jf(1, 0)
    assert all(jk_of(b, h) != jv_of(b, h) for b in range(nb) for h in range(H))
    assert torch.equal(case.q.bfloat16().double(), case.q) and torch.equal(case.a.bfloat16().double(), case.a)
    am = case.q.abs().amax(-1)
    assert torch.equal(am, 7 * 2.0 ** case.qi.double()[:, :, None].expand_as(am)), "per token and head max |q| = 7 2^i"
    assert is_e4m3(case.q * (448.0 / am)[..., None])
    assert ((case.w != 0).sum(1) == 1).all() and (case.w.abs().sum(1) == 1).all() and ((case.w != 0).sum(0) <= 1).all()
    ref = reference(case)
    assert torch.equal(ref.logits, ref.logits.round()), "every logit is an integer number of exp2 units"
    qpad, kpad = gather(case, case.q, case.k)
    pad = torch.einsum("bqhd,bkhd->bhqk", qpad, kpad[:, sp.Nk:SLOTS]) * float(c_f32()) if sp.Nk < SLOTS else None
    top = ref.logits.amax(-1)
    if sp.family == "grid":
        nz = (case.q != 0).sum(-1)
        assert int(nz.max()) <= 2 and int(nz.min()) >= 1
        if sp.imode == "vary":
            i = case.qi[0]
            assert all(len(set(i[s:s + 32].tolist())) == 3 for s in range(0, sp.Nq - 31, 32))
            assert (i[:-32] != i[32:]).all(), "the token 32 rows on has another scale"
        for h in range(H):
            d0 = case.q[0, :, h].abs().argmax(-1)
            assert set(d0.tolist()) == set(range(D)) or sp.Nq < D
        assert (top < 0).any(), "rows whose every logit is negative (a zero padding key would win them)"
        if pad is not None:
            assert float((pad.amax(-1) > top).double().mean()) > 0.5, "the padding must beat the real keys of most tokens"
    else:
        second = ref.logits.clone()
        second.scatter_(-1, case.winner[:, None, :, None].expand(-1, H, -1, 1), float("-inf"))
        assert torch.equal(ref.logits.argmax(-1), case.winner[:, None, :].expand(-1, H, -1))
        assert float((top - second.amax(-1)).min()) >= 24 or sp.Nk == 1, "winner >= 24 units above every other key"
        if pad is not None:
            assert float((top - pad.amax(-1)).min()) >= 24, "winner >= 24 units above the padding"
        assert (case.v[:, :sp.Nk] != 0).all()
        assert set(case.winner[0].tolist()) == set(range(min(sp.Nk, sp.Nq)))


def onehot_target(case: Case) -> torch.Tensor:
    """[B + dup, Nq, N]: the winning key's v row."""
    _, v = gather(case, case.q, case.v)
    idx = case.winner[:, :, None, None].expand(-1, -1, case.H, D)
    return torch.gather(v, 1, idx).reshape(len(v), case.spec.Nq, case.spec.N)


# ---- the packed e4m3 image, restated from the comment above kv_pack_fp8_kernel -------------------------------------------------------

def _k_index():
    """[96, 64] -> channel held by physical byte `col` of key row `row`."""
    row, phys = np.meshgrid(np.arange(96), np.arange(64), indexing="ij")
    logical = (((phys >> 4) ^ ((row >> 2) & 3)) << 4) | (phys & 15)     # 16-byte chunks XOR (row >> 2) & 3
    hh, e = logical >> 5, logical & 31
    return np.where(e < 16, 16 * hh + e, 32 + 16 * hh + (e - 16))


def _v_index():
    """[64, 128] -> key held by physical byte `col` of channel row d (keys >= Nk are zero bytes)."""
    d, phys = np.meshgrid(np.arange(64), np.arange(128), indexing="ij")
    logical = (((phys >> 4) ^ ((d >> 1) & 7)) << 4) | (phys & 15)       # chunks XOR (d >> 1) & 7
    m, hh, e = logical >> 6, (logical >> 5) & 1, logical & 31
    return 32 * (2 * m + (e >> 4)) + (e & 3) + 8 * ((e & 15) >> 2) + 4 * hh


K_INDEX, V_INDEX = _k_index(), _v_index()


def quantise(x: torch.Tensor, nk: int):
    """x [nb, rows, H, 64] -> (e4m3 values as fp32 [nb, 96, H, 64] with rows >= nk zero, scales fp32 [nb, H]) as kv_pack_fp8_kernel forms
    them: scale = amax / 448 over the real keys (1 for an all-zero head), x * (1 / scale) rounded to e4m3."""
    x = x.float()
    amax = x[:, :nk].abs().amax((1, 3))
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    inv = (1.0 / scale)[:, None, :, None]
    y = torch.zeros(x.shape[0], SLOTS, x.shape[2], D)
    y[:, :nk] = (x[:, :nk] * inv).to(torch.float8_e4m3fn).float()
    return y, scale


def kv_image(k: torch.Tensor, v: torch.Tensor, nk: int):
    """(image uint8 [nb, H, 14336], scales fp32 [nb, H, 2]) of k, v [nb, rows, H, 64]."""
    k8, sk = quantise(k, nk)
    v8, sv = quantise(v, nk)
    nb, H = k8.shape[0], k8.shape[2]
    kb = k8.to(torch.float8_e4m3fn).view(torch.uint8).permute(0, 2, 1, 3)            # [nb, H, 96 keys, 64 channels]
    vb = torch.zeros(nb, H, D, 128, dtype=torch.uint8)
    vb[..., :SLOTS] = v8.to(torch.float8_e4m3fn).view(torch.uint8).permute(0, 2, 3, 1)  # [nb, H, 64 channels, key]
    ki = torch.from_numpy(K_INDEX).expand(nb, H, 96, 64)
    vi = torch.from_numpy(V_INDEX).expand(nb, H, 64, 128)
    img = torch.cat([torch.gather(kb, 3, ki).reshape(nb, H, -1), torch.gather(vb, 3, vi).reshape(nb, H, -1)], -1)
    assert img.shape[-1] == IMAGE_BYTES
    return img.contiguous(), torch.stack([sk, sv], -1).contiguous()


def decode_image(img: torch.Tensor):
    """image [nb, H, 14336] -> (k8, v8) fp32 values [nb, 96, H, 64]: the inverse of the layout."""
    nb, H = img.shape[:2]
    vals = img.view(torch.float8_e4m3fn).float()
    kp, vp = vals[..., :96 * 64].reshape(nb, H, 96, 64), vals[..., 96 * 64:].reshape(nb, H, 64, 128)
    k8 = torch.zeros(nb, H, 96, 64).scatter_(3, torch.from_numpy(K_INDEX).expand(nb, H, 96, 64), kp)
    v8 = torch.zeros(nb, H, 64, 128).scatter_(3, torch.from_numpy(V_INDEX).expand(nb, H, 64, 128), vp)
    return k8.permute(0, 2, 1, 3).contiguous(), v8[..., :SLOTS].permute(0, 3, 1, 2).contiguous()


# ---- fp32 emulations of the two pipelines, with the fault models ---------------------------------------------------------------------

FAULTS_BF16 = ("k_chan_swap", "v_key_perm", "pad_unmasked", "nk_round16", "dup_batch")
FAULTS_FP8 = FAULTS_BF16 + ("k_scale_head", "v_scale_head", "k_scale_batch", "v_scale_batch", "q_scale_32")


def faults_for(sp: Spec, route: str):
    """The fault models a case must expose on a route: "bf16", "fp8" (packed image, scales per batch and head, q scale per token) or
    "fp8core" (cd360_attn_fwd_fp8mfma_bf16: one scale per tensor, passed by the caller -- no slot to misread).  The one-hot family answers
    to what moves the winner's v row; a changed logit scale or two swapped channels leave its winner in place (that is what the grid
    family is for)."""
    fp8 = route == "fp8"
    f = ["v_key_perm"]
    if sp.dup:
        f.append("dup_batch")
    if fp8:
        f += ["v_scale_head", "v_scale_batch"]
    if sp.family == "grid":
        f.append("k_chan_swap")
        if sp.Nk % 32:
            f.append("pad_unmasked")
        if sp.Nk % 16:
            f.append("nk_round16")
        if fp8:
            f += ["k_scale_head", "k_scale_batch"]
            if sp.imode == "vary":
                f.append("q_scale_32")
    return f


def _faulty_kv(case: Case, fault):
    sp = case.spec
    k, v = case.k.float().clone(), case.v.float().clone()
    if fault == "k_chan_swap":      # two channels of one 16-channel chunk, in every key row
        k[..., [2, 3]] = k[..., [3, 2]]
        k[..., [17, 30]] = k[..., [30, 17]]
        for h in range(case.H):     # (and the pair the anti channel is in, so the rows that test the padding see it too)
            c = anti_channel(h)
            k[:, :, h, [c, c ^ 1]] = k[:, :, h, [c ^ 1, c]]
    if fault == "v_key_perm":       # keys rotated inside every complete group of four
        g = sp.Nk // 4 * 4
        if g:
            idx = torch.arange(g).view(-1, 4).roll(1, 1).reshape(-1)
            v[:, :g] = v[:, idx]
    return k, v


def _batches(case: Case, fault):
    ob = out_batches(case.spec)
    if fault == "dup_batch":
        ob = [(qb, qb) for qb, _ in ob]
    return [p[0] for p in ob], [p[1] for p in ob]


def emulate_bf16(case: Case, fault=None, round_out=True) -> torch.Tensor:
    """The bf16 epilogue in fp32 torch: q = bf16(a W^T), fp32 scores, p = exp2(c (s - max)), the row sum of the fp32 p, P rounded to bf16,
    fp32 P V, one bf16 rounding of o / l (round_out=False: the fp32 value in front of it)."""
    sp = case.spec
    nk = -(-sp.Nk // 16) * 16 if fault == "nk_round16" else sp.Nk
    slots = nk + 1 if fault == "pad_unmasked" else nk
    k, v = _faulty_kv(case, fault)
    qb, kb = _batches(case, fault)
    q = (case.a.float() @ case.w.float().T).bfloat16().float().reshape(sp.B, sp.Nq, case.H, D)[qb]
    k, v = k[kb][:, :slots], v[kb][:, :slots]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k)
    c = torch.tensor(c_f32())
    mx = s.amax(-1, keepdim=True)
    p = torch.exp2(s * c - mx * c)
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("bhqk,bkhd->bhqd", p.bfloat16().float(), v) / l
    o = o.permute(0, 2, 1, 3).reshape(len(qb), sp.Nq, sp.N)
    return o.bfloat16() if round_out else o


def emulate_fp8(case: Case, fault=None, per_tensor_amax=None, round_out=True) -> torch.Tensor:
    """The fp8 pipeline in fp32 torch: K, V quantised per (batch, head) and laid out / read back through the image, q per token and head
    (max -> 448), integer dot, exp2 with the scales folded in, P 2^8 to e4m3, the row sum of the fp32 p, o = P V * v scale / sum.
    per_tensor_amax = (q, k, v): the scales of cd360_attn_fwd_fp8mfma_bf16 instead (one per tensor, from the caller)."""
    sp, H = case.spec, case.H
    nk = -(-sp.Nk // 16) * 16 if fault == "nk_round16" else sp.Nk
    kf, vf = _faulty_kv(case, fault)
    qb, kb = _batches(case, fault)
    q = (case.a.float() @ case.w.float().T).reshape(sp.B, sp.Nq, H, D)
    if per_tensor_amax is None:
        k8, v8 = decode_image(kv_image(kf, vf, nk)[0])
        _, sk = quantise(kf, nk)
        _, sv = quantise(vf, nk)
        am = q.abs().amax(-1).clamp_min(1e-20)
        qs = am * float(np.float32(1.0 / 448.0))
        q8 = (q * (448.0 / am)[..., None]).to(torch.float8_e4m3fn).float()
    else:
        aq, ak, av = (np.float32(x) / np.float32(448.0) for x in per_tensor_amax)
        k8 = torch.zeros(kf.shape[0], SLOTS, H, D)
        v8 = torch.zeros_like(k8)
        k8[:, :nk] = (kf[:, :nk] * float(np.float32(1.0) / ak)).to(torch.float8_e4m3fn).float()
        v8[:, :nk] = (vf[:, :nk] * float(np.float32(1.0) / av)).to(torch.float8_e4m3fn).float()
        sk = torch.full((kf.shape[0], H), float(ak))
        sv = torch.full((kf.shape[0], H), float(av))
        qs = torch.full(q.shape[:3], float(aq))
        q8 = (q * float(np.float32(1.0) / aq)).to(torch.float8_e4m3fn).float()
    nb = kf.shape[0]
    if fault == "k_scale_head":
        sk = sk.roll(-1, 1)
    if fault == "v_scale_head":
        sv = sv.roll(-1, 1)
    if fault == "k_scale_batch":
        sk = sk.roll(-1, 0)
    if fault == "v_scale_batch":
        sv = sv.roll(-1, 0)
    if fault == "q_scale_32":
        qs = qs.roll(-32, 1)
    assert nb == sp.B + sp.dup
    q8, qs = q8[qb], qs[qb]
    k8, v8, sk, sv = k8[kb], v8[kb], sk[kb], sv[kb]
    s = torch.einsum("bqhd,bkhd->bhqk", q8, k8)                       # [ob, H, Nq, 96]
    masked = torch.arange(SLOTS) >= (nk + 1 if fault == "pad_unmasked" else nk)
    s = s + torch.zeros(SLOTS).masked_fill(masked, -1e30)
    cs = (torch.tensor(c_f32()) * qs.permute(0, 2, 1) * sk[:, :, None])[..., None]
    mc = -s.amax(-1, keepdim=True) * cs + 8.0
    p = torch.exp2(s * cs + mc)
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("bhqk,bkhd->bhqd", p.to(torch.float8_e4m3fn).float(), v8) * (1.0 / l) * sv[:, :, None, None]
    o = o.permute(0, 2, 1, 3).reshape(len(qb), sp.Nq, sp.N)
    return o.bfloat16() if round_out else o


# ---- the case lists of the GPU tests -------------------------------------------------------------------------------------------------

QCFGS = (1, 2, 3, 4)
WIDTHS = ((128, 192), (384, 384))      # (N, K): two heads behind a K = N + 64 selection; 256 + 128 columns behind a K = N one
NK_BF16 = (16, 17, 32, 33, 48, 64, 65, 77, 80, 81, 95, 96)
NK_KEYS16 = (65, 77, 80)
NK_FP8 = (65, 77, 80, 81, 96)
NK_CORE = (20, 32, 33, 64, 65, 77, 96)
NQ_CORE = (256, 200)
NK_PACK = (1, 31, 64, 77, 96)
FAMILIES = ("grid", "onehot")


def qproj_specs(nk, n, kdim, dup):
    return [Spec(f, n, kdim, nk, dup) for f in FAMILIES]


def core_specs(nk, nq):
    """The plain attention entries: q's i is one value per case (the fp8 form scales per tensor) and changes from case to case."""
    i = (NK_CORE.index(nk) + NQ_CORE.index(nq)) % 3
    return [Spec(f, 128, 128, nk, 0, nq, 2, i) for f in FAMILIES]


def core_amax(sp: Spec):
    """(max |q|, max |k|, max |v|) = (7 2^i, 7 2^j, 7 2^j) with j the largest exponent among the heads."""
    return (7.0 * 2.0 ** (1 + sp.imode), 7.0 * 2.0 ** max(J), 7.0 * 2.0 ** max(J))


def pack_spec(nk):
    return Spec("grid", 384, 384, nk, 1)


def all_specs():
    """(spec, runs on the bf16 route, runs on the fp8 route), every case the GPU file runs, once."""
    seen = {}
    for n, kdim in WIDTHS:
        for dup in (0, 1):
            for nk in NK_BF16:
                for sp in qproj_specs(nk, n, kdim, dup):
                    seen[sp] = (True, nk in NK_FP8)
    for nk in NK_CORE:
        for nq in NQ_CORE:
            for sp in core_specs(nk, nq):
                seen[sp] = (True, True)
    return [(sp, b, f) for sp, (b, f) in seen.items()]
