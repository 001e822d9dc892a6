"""Exact inputs for the thin kernels around the GEMM core -- cd360_out_conv4_bf16, cd360_unet_stage_in, cd360_vae_conv_in_f32,
cd360_vae_conv_out_bf16 / _u8, cd360_vae_enc_conv_out_bf16, cd360_rowdot1 / 4_bf16, cd360_rowdot4_bwd_bf16, cd360_concat_channels_bf16,
cd360_geglu_bf16 and its backward -- with float64 references.  CPU only: nothing here imports the HIP library.

The method is that of tests/gemm_cases.py (its rne, truncate and rounding_shares are used, not copied).  These kernels accumulate in fp32
with fp32 or bf16 operands; with small integer operands (or integers times one power of two) every product and every partial sum is a
multiple of that power of two below 2^24 of them, in any order -- taps, row bands, channel chunks staged through the LDS, K slices summed
through the LDS, statistics slabs.  So an fp32 output has exactly one right value, a bf16 output one rounding with one right answer, and
the uint8 image one truncation of an exact fp32 value.  The GPU tests compare with torch.equal.

Every builder asserts what its exactness rests on (`check_*`): operands representable in the dtype the kernel reads, the worst
sum |x||w| + |bias| below 2^24 (in units of the operands' common power of two), and for statistics sum |v| and sum v^2 of the STORED values
of a slab below 2^24.  Where the output is bf16 the builder walks a fixed seed sequence until at least 15 % of the outputs need rounding
and at least 5 % are exact ties.  `*_faults` restate the reference with one defect each -- (name, defective output, mask of positions the
change has to include or None); tests/test_thin_cases_cpu.py holds every case to detecting every defect that applies to it.

Layouts here: activations [B, H, W, C] float64 (channels last), convolution weights [Cout, Cin, 3, 3] as nn.Conv2d holds them, outputs
[B, H, W, Cout]; the GPU tests pack and permute through the cd360.ops helpers.  An output a defective kernel would not write is NaN (the
GPU tests pre-fill what they can with NaN).

GEGLU (an erf and an exp: no bit equality).  Reference in float64: y = x gelu(g), dx = dy gelu(g), dg = dy x gelu'(g).  Per element got is
accepted iff it lies in [bf16(want - delta), bf16(want + delta)], delta = c 2^-24 scale, scale = |x| max(|g|, 1) for y, |dy| max(|g|, 1)
for dx, |dy||x| max(|g|, 1) for dg.  c is four times the worst error, in units of 2^-24 scale, of a plain fp32 CPU evaluation of the same
formulas against float64 over the inputs of every case below (measured: y 2.37, dx 1.72, dg 2.63 -> GEGLU_C = 10.5 for all three; the
factor four covers libm differences between hosts).  tests/test_thin_cases_cpu.py measures again and holds the figure below c / 2."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Dict, Iterator, List, Optional, Tuple

import torch

from gemm_cases import BF, TWO24, _ints, _seed, exact_f32, is_bf16, rne, rounding_shares, truncate

MIN_INEXACT, MIN_TIES = 0.15, 0.05
NAN = float("nan")
Fault = Tuple[str, torch.Tensor, Optional[torch.Tensor]]


def is_f32(x64: torch.Tensor) -> bool:
    return torch.equal(x64.float().double(), x64)


def bf16_of(x64: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16 with ONE round-to-nearest-even, on the bits (torch's cast goes through fp32 and rounds twice); normal range."""
    bits = x64.contiguous().view(torch.int64)
    bits = (bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) & ~((1 << 45) - 1)
    return bits.view(torch.float64).to(BF)


def floors_met(pre: torch.Tensor) -> bool:
    inexact, ties, _ = rounding_shares(pre)
    return inexact >= MIN_INEXACT and ties >= MIN_TIES


def differs(bad: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Elementwise: a NaN in `bad` (an element left unwritten) differs from everything."""
    return bad.double() != want.double()


def with_nan(t: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    t = t.double().clone()
    t[mask.expand_as(t)] = NAN
    return t


# ---- 3 x 3 convolution, padding 1, as nine tap terms -------------------------------------------------------------------------------------
def tap_terms(x: torch.Tensor, w: torch.Tensor, wrap_cols: bool = False, wrap_rows: bool = False) -> torch.Tensor:
    """x [B, H, W, Cin], w [Cout, Cin, 3, 3] -> [9, B, H, W, Cout]: the contribution of tap 3 ky + kx to every output.
    wrap_cols: the column test is missing, the shifted read runs into the neighbouring image row (flat pixel index +- 1).
    wrap_rows: the row test is per batch, not per image: the first / last row reads the neighbouring image."""
    B, H, W, C = x.shape
    if wrap_rows:
        return tap_terms(x.reshape(1, B * H, W, C), w, wrap_cols).reshape(9, B, H, W, -1)
    flat = x.reshape(B, H * W, C)
    ys, xs = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    out = []
    for tap in range(9):
        sy, sx = ys + tap // 3 - 1, xs + tap % 3 - 1
        src = sy * W + sx
        ok = (sy >= 0) & (sy < H) & ((src >= 0) & (src < H * W) if wrap_cols else (sx >= 0) & (sx < W))
        g = flat[:, src.clamp(0, H * W - 1).reshape(-1)] * ok.reshape(1, -1, 1).double()
        out.append((g @ w[:, :, tap // 3, tap % 3].t()).reshape(B, H, W, -1))
    return torch.stack(out)


def conv3x3(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return tap_terms(x, w).sum(0)


def conv_bound(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> float:
    """The worst sum |x||w| + |bias| over the outputs."""
    return (conv3x3(x.abs(), w.abs()) + bias.abs()).max().item()


@dataclass(frozen=True)
class ConvCase:
    family: str
    key: tuple
    x: torch.Tensor      # [B, H, W, Cin] what the kernel multiplies (stage-in: bf16(c_in x_lat))
    w: torch.Tensor      # [Cout, Cin, 3, 3]
    bias: torch.Tensor   # [Cout]
    pre: torch.Tensor    # [B, H, W, Cout] exact, in front of the output's one rounding
    out: str             # "bf16" | "f32" | "u8"
    unit: float = 1.0    # the operands' common power of two: sums are multiples of it, and below 2^24 of it
    extra: Dict[str, object] = field(default_factory=dict)

    def final(self, pre: torch.Tensor) -> torch.Tensor:
        if self.out == "bf16":
            return rne(pre)
        if self.out == "u8":
            return image_bytes(pre)
        return exact_f32(pre).double()

    @property
    def want(self) -> torch.Tensor:
        return self.final(self.pre)


def image_bytes(f: torch.Tensor) -> torch.Tensor:
    """(clip(f 0.5 + 0.5, 0, 1) 255).to(uint8) in float64; exact in fp32 too when f is a multiple of 1/256 of small magnitude."""
    return ((f * 0.5 + 0.5).clamp(0.0, 1.0) * 255.0).floor().to(torch.uint8)


def check_conv(c: ConvCase, x_dtype: str, w_dtype: str) -> None:
    """Operands representable, sum |x||w| + |bias| < 2^24 units, the reference is what the operands give."""
    ux = c.extra.get("x_unit", 1.0)
    for t, dt, u, name in ((c.x, x_dtype, ux, "x"), (c.w, w_dtype, c.unit / ux, "w"), (c.bias, "f32", c.unit, "bias")):
        assert is_bf16(t) if dt == "bf16" else is_f32(t), f"{name} is not {dt}-representable"
        assert torch.equal((t / u).round() * u, t), f"{name} is no multiple of {u}"
    bound = conv_bound(c.x, c.w, c.bias) / c.unit
    assert bound < TWO24, f"sum |x||w| + |bias| = {bound} units reaches 2^24"
    assert torch.equal(c.pre, conv3x3(c.x, c.w) + c.bias)
    exact_f32(c.pre)


def chunk_term(c: ConvCase, c0: int, c1: int) -> torch.Tensor:
    return conv3x3(c.x[..., c0:c1], c.w[:, c0:c1])


def conv_faults(c: ConvCase, *, chunk: Optional[int] = None, band: Optional[int] = None, block: Optional[int] = None,
                bias_shift: int = 1) -> Iterator[Fault]:
    """The defects every 3 x 3 kernel here shares.  chunk: input channels per LDS stage; band: output rows per workgroup (halo rows
    above and below); block: output pixels per workgroup of a flat pixel grid (the ragged last one may be skipped)."""
    B, H, W, _ = c.x.shape
    T = tap_terms(c.x, c.w)
    col = torch.arange(W)[None, None, :, None]
    row = torch.arange(H)[None, :, None, None]
    img = torch.arange(B)[:, None, None, None]
    everywhere = torch.ones(B, H, W, 1, dtype=torch.bool)
    for tap in range(9):
        if T[tap].abs().sum() > 0:  # (a 1-row or 1-column image has taps that never land)
            yield f"tap-{tap}-dropped", c.final(c.pre - T[tap]), None
    if W > 1 and H > 1:  # (one image row: nothing to wrap into)
        Tw = tap_terms(c.x, c.w, wrap_cols=True)
        yield "column-shift-wraps-at-x=0", c.final(c.pre + (Tw - T)[[0, 3, 6]].sum(0)), (col == 0) & everywhere
        yield "column-shift-wraps-at-x=W-1", c.final(c.pre + (Tw - T)[[2, 5, 8]].sum(0)), (col == W - 1) & everywhere
    if band is not None and H > band:
        top = (row % band == 0) & (row > 0) & everywhere      # first row of an interior band: its upper halo row
        bot = (row % band == band - 1) & (row < H - 1) & everywhere
        yield "upper-halo-row-missing-at-interior-band-edges", c.final(c.pre - T[0:3].sum(0) * top), top
        yield "lower-halo-row-missing-at-interior-band-edges", c.final(c.pre - T[6:9].sum(0) * bot), bot
    if B > 1:
        Tr = tap_terms(c.x, c.w, wrap_rows=True)
        yield "first-band-halo-from-the-image-before", c.final(c.pre + (Tr - T)[0:3].sum(0)), (row == 0) & (img > 0) & everywhere
        yield "last-band-halo-from-the-image-after", c.final(c.pre + (Tr - T)[6:9].sum(0)), (row == H - 1) & (img < B - 1) & everywhere
    if chunk is not None:
        cin = c.x.shape[-1]
        for i, c0 in enumerate(range(0, cin, chunk)):
            t = chunk_term(c, c0, min(cin, c0 + chunk))
            tail = "-the-tail" if cin % chunk and c0 + chunk > cin else ""
            yield f"k-chunk-{i}{tail}-dropped", c.final(c.pre - t), None
            yield f"k-chunk-{i}{tail}-added-twice", c.final(c.pre + t), None
    if block is not None and (H * W) % block:
        p = (torch.arange(H * W) >= (H * W) // block * block).reshape(1, H, W, 1) & everywhere
        yield "ragged-last-pixel-block-skipped", with_nan(c.want, p), p
    if c.out == "bf16":
        yield "truncation", truncate(c.pre), None
    b = torch.roll(c.bias, -bias_shift)
    if not torch.equal(b, c.bias):
        yield f"bias-slice-shifted-{bias_shift}", c.final(c.pre - c.bias + b), None


def _walk(name: str, key: tuple, build, rounds: bool = True):
    for attempt in range(256):
        c = build(torch.Generator().manual_seed(_seed(name, *key) + attempt))
        if not rounds or floors_met(c.pre):
            return c
    raise AssertionError(f"no case of {name} {key} meets the rounding floors")


# ---- cd360_out_conv4_bf16 ----------------------------------------------------------------------------------------------------------------
OUT_CONV4 = dict(x=8, w=4, b=64)
OUT_CONV4_IMAGES, OUT_CONV4_HW, OUT_CONV4_CIN = (1, 3), [(2, 32), (6, 32), (4, 64), (6, 128)], (64, 128, 192, 320)


@functools.lru_cache(maxsize=None)
def out_conv4_case(images: int, H: int, W: int, cin: int) -> ConvCase:
    def build(g):
        x, w, b = _ints(g, (images, H, W, cin), OUT_CONV4["x"]), _ints(g, (4, cin, 3, 3), OUT_CONV4["w"]), _ints(g, (4,), OUT_CONV4["b"])
        return ConvCase("out_conv4", (images, H, W, cin), x, w, b, conv3x3(x, w) + b, "bf16")
    c = _walk("out_conv4", (images, H, W, cin), build)
    check_out_conv4(c)
    return c


def check_out_conv4(c: ConvCase) -> None:
    check_conv(c, "bf16", "bf16")
    assert c.x.shape[0] == 1 or not torch.equal(c.x[0], c.x[1])  # distinct data per image


def out_conv4_faults(c: ConvCase) -> Iterator[Fault]:
    """K chunks of 64 through a two-stage ring (one chunk: a single issue; two: both stages, no re-issue; three or more: issue(c + 2));
    bands of two rows; tap 8 = partial columns 32 .. 35, stored by the hh == 0 half wave alone."""
    yield from conv_faults(c, chunk=64, band=2)
    yield "tap-8-partial-columns-32..35-dropped", c.final(c.pre - tap_terms(c.x, c.w)[8]), None


def out_conv4_cases() -> List[tuple]:
    return [(n, H, W, cin) for n in OUT_CONV4_IMAGES for H, W in OUT_CONV4_HW for cin in OUT_CONV4_CIN]


# ---- cd360_unet_stage_in -----------------------------------------------------------------------------------------------------------------
STAGE = dict(w=8, b=64)
STAGE_HW = [(3, 5), (5, 64), (4, 96), (2, 128), (3, 130)]  # less than a tile; one tile; a ragged second; two tiles; a third of two pixels
STAGE_BS, STAGE_REP, STAGE_COUT, STAGE_E = (1, 2), (2, 3), (64, 320), (64, 1280)
STAGE_TABLES = {"exact": ((0.5, 0.25, 2.0), 32), "round": ((0.5, 1.0, 2.0), 600)}  # c_in per step row, |x|


@functools.lru_cache(maxsize=None)
def stage_in_case(kind: str, bs: int, rep: int, cout: int, H: int, W: int) -> ConvCase:
    cins, amp = STAGE_TABLES[kind]
    idx = 1 if kind == "round" else 1 + (bs + rep + H + cout // 64) % 2  # the device step index: 1 or 2, never row 0

    def build(g):
        lat = _ints(g, (bs, H, W, 4), amp)
        w, b = _ints(g, (cout, 4, 3, 3), STAGE["w"]), _ints(g, (cout,), STAGE["b"])
        tab = torch.tensor([[1.0 + r, 0.5 + r, ci, 0.0] for r, ci in enumerate(cins)], dtype=torch.float64)
        x = (lat * cins[idx]).to(BF).double()
        unit = min(1.0, cins[idx]) if kind == "exact" else 1.0
        return ConvCase("stage_in", (kind, bs, rep, cout, H, W), x, w, b, conv3x3(x, w) + b, "bf16", unit,
                        dict(lat=lat, tab=tab, idx=idx, rep=rep, kind=kind, x_unit=unit))
    c = _walk("stage_in", (kind, bs, rep, cout, H, W), build)
    check_stage_in(c)
    return c


def check_stage_in(c: ConvCase) -> None:
    check_conv(c, "bf16", "bf16")
    lat, tab, idx = c.extra["lat"], c.extra["tab"], c.extra["idx"]
    cins = tab[:, 2].tolist()
    assert tab.shape[0] >= 3 and idx in (1, 2) and len(set(cins)) == len(cins) and all(math.log2(v) == round(math.log2(v)) for v in cins)
    assert is_f32(lat) and is_f32(tab)
    scaled = lat * cins[idx]
    if c.extra["kind"] == "exact":
        assert torch.equal(c.x, scaled), "c_in x must be exact in bf16"
    else:
        assert cins[idx] == 1.0 and (c.x != scaled).double().mean().item() >= 0.15, "bf16(c_in x) must round"


def stage_full(c: ConvCase, t: torch.Tensor) -> torch.Tensor:
    """[bs, H, W, Cout] -> h [rep bs, H, W, Cout]: branch r of sample s is image r bs + s."""
    return t.repeat(c.extra["rep"], 1, 1, 1)


def stage_in_faults(c: ConvCase) -> Iterator[Fault]:
    """On h [rep bs, H, W, Cout].  A workgroup = 64 pixels of one image row with a halo of one row and one column."""
    rep, lat, tab, idx = c.extra["rep"], c.extra["lat"], c.extra["tab"], c.extra["idx"]
    bs, H, W, _ = c.x.shape
    for name, bad, where in conv_faults(c, band=1, bias_shift=8):
        yield name, stage_full(c, bad), None if where is None else stage_full(c, where)
    T = tap_terms(c.x, c.w)
    col = torch.arange(W)[None, None, :, None]
    for edge in (64, 128):
        if W > edge:
            left, right = (col == edge - 1).expand(bs, H, W, 1), (col == edge).expand(bs, H, W, 1)
            bad = c.pre - T[[2, 5, 8]].sum(0) * left - T[[0, 3, 6]].sum(0) * right
            yield f"tile-edge-halo-column-zero-at-x={edge}", stage_full(c, c.final(bad)), stage_full(c, left | right)
    if W % 64:
        p = (col >= W // 64 * 64).expand(bs, H, W, 1)
        yield "ragged-last-tile-skipped", stage_full(c, with_nan(c.want, p)), stage_full(c, p)

    def redo(x):
        return stage_full(c, rne(conv3x3(x, c.w) + c.bias))
    yield "c_in-from-row-0", redo((lat * tab[0, 2].item()).to(BF).double()), None
    if c.extra["kind"] == "round":
        yield "bf16-rounding-of-c_in-x-omitted", redo(lat * tab[idx, 2].item()), None
    full = stage_full(c, c.want)
    for r in range(1, rep):
        m = torch.zeros(rep * bs, 1, 1, 1, dtype=torch.bool)
        m[r * bs:(r + 1) * bs] = True
        yield f"branch-copy-{r}-not-written", with_nan(full, m), m.expand(rep * bs, H, W, 1)


def stage_in_cases() -> List[tuple]:
    return [(k, bs, rep, co, H, W) for k in STAGE_TABLES for bs in STAGE_BS for rep in STAGE_REP for co in STAGE_COUT for H, W in STAGE_HW]


@dataclass(frozen=True)
class EmbCase:
    bs: int
    rep: int
    E: int
    idx: int
    temb: torch.Tensor   # [3, E] bf16 values
    lab: torch.Tensor    # [rep bs, E]
    ssum: torch.Tensor   # [rep bs, E] bf16(temb[idx] + lab)
    want: torch.Tensor   # [rep bs, E] float64 silu(ssum)


def emb_launch(bs: int, rep: int) -> tuple:
    """The stage-in case an emb_act case is launched with (one launch serves both outputs; they share the device step index)."""
    return ("exact", bs, rep, 64, 3, 5)


def silu64(v: torch.Tensor) -> torch.Tensor:
    return v / (1.0 + torch.exp(-v))


def bf16_spacing(ref: torch.Tensor) -> torch.Tensor:
    """The distance between neighbouring bf16 values at |ref| (normal range)."""
    return 2.0 ** (torch.frexp(ref.abs().clamp_min(2.0 ** -100))[1].double() - 8)


@functools.lru_cache(maxsize=None)
def emb_case(bs: int, rep: int, E: int) -> EmbCase:
    g = torch.Generator().manual_seed(_seed("emb", bs, rep, E))
    temb = (torch.randn(3, E, generator=g, dtype=torch.float64) * 2).to(BF).double()
    lab = (torch.randn(rep * bs, E, generator=g, dtype=torch.float64) * 2).to(BF).double()
    idx = stage_in_case(*emb_launch(bs, rep)).extra["idx"]
    s = (temb[idx] + lab).to(BF).double()
    return EmbCase(bs, rep, E, idx, temb, lab, s, silu64(s))


def emb_accepts(c: EmbCase, got: torch.Tensor) -> torch.Tensor:
    """Per element: within one bf16 spacing of the float64 reference (the fp32 evaluation error is far below half a spacing: the kernel
    can land only on one of the reference's two bf16 neighbours).  A NaN is refused."""
    return (got.double().cpu() - c.want).abs() <= bf16_spacing(c.want)


def emb_faults(c: EmbCase) -> Iterator[Tuple[str, torch.Tensor]]:
    yield "temb-from-row-0", silu64((c.temb[0] + c.lab).to(BF).double()).to(BF)
    yield "lab-rows-rotated-by-one", silu64((c.temb[c.idx] + torch.roll(c.lab, 1, 0)).to(BF).double()).to(BF)
    yield "silu-left-out", c.ssum.to(BF)
    yield "last-row-not-written", with_nan(c.want.to(BF), (torch.arange(c.rep * c.bs) == c.rep * c.bs - 1)[:, None])


def emb_cases() -> List[tuple]:
    return [(bs, rep, E) for bs in STAGE_BS for rep in STAGE_REP for E in STAGE_E]


# ---- cd360_vae_conv_in_f32 ---------------------------------------------------------------------------------------------------------------
VAE_IN = {4: dict(z=16, w=8, b=64), 8: dict(z=12, w=8, b=64)}  # Cz = 8: z narrowed so that a 64-pixel slab's sum v^2 stays below 2^24
VAE_IN_B, VAE_IN_CZ, VAE_IN_COUT, VAE_IN_HW = (1, 2), (4, 8), (64, 128, 512), [(17, 23), (8, 8), (16, 12)]
CI_SLAB = 64


def pixel_slab_stats(stored: torch.Tensor, slab: int = CI_SLAB) -> torch.Tensor:
    """[B, H, W, C] -> [B, H W / slab, C, 2] float64 (sum, sum of squares) per slab of consecutive pixels."""
    B, H, W, C = stored.shape
    v = stored.double().reshape(B, H * W // slab, slab, C)
    return torch.stack([v.sum(2), (v * v).sum(2)], -1)


@functools.lru_cache(maxsize=None)
def vae_conv_in_case(B: int, cz: int, cout: int, H: int, W: int) -> ConvCase:
    r = VAE_IN[cz]

    def build(g):
        x, w, b = _ints(g, (B, H, W, cz), r["z"]), _ints(g, (cout, cz, 3, 3), r["w"]), _ints(g, (cout,), r["b"])
        return ConvCase("vae_conv_in", (B, cz, cout, H, W), x, w, b, conv3x3(x, w) + b, "bf16", 1.0, dict(stats=(H * W) % CI_SLAB == 0))
    c = _walk("vae_conv_in", (B, cz, cout, H, W), build)
    check_vae_conv_in(c)
    return c


def check_vae_conv_in(c: ConvCase) -> None:
    check_conv(c, "f32", "f32")
    if c.extra["stats"]:
        B, H, W, C = c.pre.shape
        v = c.want.double().reshape(B, H * W // CI_SLAB, CI_SLAB, C)
        worst_abs, worst_sq = v.abs().sum(2).max().item(), (v * v).sum(2).max().item()
        assert worst_abs < TWO24 and worst_sq < TWO24, f"slab statistics reach 2^24: sum |v| {worst_abs}, sum v^2 {worst_sq}"


def vae_conv_in_faults(c: ConvCase) -> Iterator[Fault]:
    yield from conv_faults(c, block=CI_SLAB, bias_shift=2)


def vae_conv_in_stats_faults(c: ConvCase) -> Iterator[Fault]:
    """(name, defective statistics, mask over [B, slabs, C, 2]); the right ones are pixel_slab_stats(c.want)."""
    if not c.extra["stats"]:
        return
    right = pixel_slab_stats(c.want)
    every = torch.ones_like(right, dtype=torch.bool)
    yield "statistics-of-the-unrounded-values", pixel_slab_stats(c.pre), None
    if right.shape[1] > 1:
        yield "statistics-slabs-shifted-by-one", torch.roll(right, 1, 1), every
    yield "sum-and-sum-of-squares-swapped", right.flip(-1), None


def vae_conv_in_cases() -> List[tuple]:
    return [(B, cz, co, H, W) for B in VAE_IN_B for cz in VAE_IN_CZ for co in VAE_IN_COUT for H, W in VAE_IN_HW]


# ---- cd360_vae_conv_out_bf16 / cd360_vae_conv_out_u8 -------------------------------------------------------------------------------------
VAE_OUT = dict(x=8, w=8, b=64)
VAE_OUT_U8 = dict(x=4, w=4, b=64)  # w and bias in units of 1 / 256
VAE_OUT_B, VAE_OUT_COUT, VAE_OUT_CIN, VAE_OUT_HW = (1, 2), (3, 4), (64, 256, 320, 512), [(1, 5), (16, 16), (17, 23)]
U8_MIN_DISTINCT = 128


@functools.lru_cache(maxsize=None)
def vae_conv_out_case(B: int, cout: int, cin: int, H: int, W: int, u8: bool = False) -> ConvCase:
    r = VAE_OUT_U8 if u8 else VAE_OUT
    unit = 1.0 / 256 if u8 else 1.0

    def build(g):
        x, w, b = _ints(g, (B, H, W, cin), r["x"]), _ints(g, (cout, cin, 3, 3), r["w"]) * unit, _ints(g, (cout,), r["b"]) * unit
        return ConvCase("vae_conv_out_u8" if u8 else "vae_conv_out", (B, cout, cin, H, W), x, w, b, conv3x3(x, w) + b, "u8" if u8 else "f32", unit)
    c = _walk("vae_conv_out_u8" if u8 else "vae_conv_out", (B, cout, cin, H, W), build, rounds=False)
    check_vae_conv_out(c)
    return c


def check_vae_conv_out(c: ConvCase) -> None:
    check_conv(c, "bf16", "f32")
    if c.out == "u8":
        t = c.pre * 0.5 + 0.5  # a multiple of 1 / 512 of magnitude < 2^24 / 512: exact in fp32, and so is clip(t) 255 (< 2^17 units of 1 / 512)
        assert is_f32(t) and is_f32(t.clamp(0, 1) * 255.0)
        if c.pre.numel() >= 512:  # (the 5-pixel images cannot show 128 values)
            vals = c.want.unique()
            assert vals.numel() >= U8_MIN_DISTINCT and vals[0] == 0 and vals[-1] == 255, f"{vals.numel()} byte values, {vals[0]} .. {vals[-1]}"


def vae_conv_out_faults(c: ConvCase) -> Iterator[Fault]:
    """Channel chunks of 256 through the LDS (Cin = 320: a tail of 64), 256 output pixels per workgroup."""
    yield from conv_faults(c, chunk=256, block=256)
    B, H, W, cout = c.pre.shape
    if cout < 4:  # the packed weight's columns >= Cout are zero: a fourth channel stored is bias-less 0 (byte 127) one element further on
        spill = 127 if c.out == "u8" else 0.0
        if c.out == "u8":   # [B, H, W, Cout] bytes: channel Cout of pixel p is channel 0 of pixel p + 1
            flat = c.want.clone().reshape(-1, cout)
            where = torch.zeros_like(flat, dtype=torch.bool)
            flat[1:, 0], where[1:, 0] = spill, True
            yield "output-channels->=Cout-written", flat.reshape(c.want.shape), where.reshape(c.want.shape)
        elif B > 1:         # [B, Cout, H, W] fp32: channel Cout of image b is channel 0 of image b + 1
            bad, where = c.want.clone(), torch.zeros_like(c.want, dtype=torch.bool)
            bad[1:, :, :, 0], where[1:, :, :, 0] = spill, True
            yield "output-channels->=Cout-written", bad, where


def vae_conv_out_cases() -> List[tuple]:
    return [(B, co, cin, H, W) for B in VAE_OUT_B for co in VAE_OUT_COUT for cin in VAE_OUT_CIN for H, W in VAE_OUT_HW]


# ---- cd360_vae_enc_conv_out_bf16 ---------------------------------------------------------------------------------------------------------
ENC_OUT = dict(x=8, w=8, b=64)
ENC_OUT_B, ENC_OUT_COUT, ENC_OUT_CIN, ENC_OUT_HW = (1, 3), (5, 8), (64, 128, 192, 512), [(1, 3), (4, 4), (17, 23)]
EO_SLICES, EO_CHUNK = 16, 128


@functools.lru_cache(maxsize=None)
def enc_conv_out_case(B: int, cout: int, cin: int, H: int, W: int) -> ConvCase:
    def build(g):
        x, w, b = _ints(g, (B, H, W, cin), ENC_OUT["x"]), _ints(g, (cout, cin, 3, 3), ENC_OUT["w"]), _ints(g, (cout,), ENC_OUT["b"])
        return ConvCase("vae_enc_conv_out", (B, cout, cin, H, W), x, w, b, conv3x3(x, w) + b, "f32")
    c = _walk("vae_enc_conv_out", (B, cout, cin, H, W), build, rounds=False)
    check_conv(c, "bf16", "f32")
    return c


def slice_weight(c: ConvCase, s: int) -> torch.Tensor:
    """The part of the weight K slice s of 16 multiplies: per chunk of 128 channels (groups = its 8-channel groups) the units
    u = tap groups + g with u % 16 == s."""
    cin = c.w.shape[1]
    m = torch.zeros(cin, 3, 3, dtype=torch.bool)
    for c0 in range(0, cin, EO_CHUNK):
        groups = min(EO_CHUNK, cin - c0) // 8
        for u in range(s, 9 * groups, EO_SLICES):
            tap, g = divmod(u, groups)
            m[c0 + 8 * g:c0 + 8 * g + 8, tap // 3, tap % 3] = True
    return c.w * m.double()


def enc_conv_out_faults(c: ConvCase) -> Iterator[Fault]:
    """Channel chunks of 128 (Cin = 192: a tail of 64), 16 pixels per workgroup, 16 K slices per pixel summed through the LDS."""
    yield from conv_faults(c, chunk=EO_CHUNK, block=16)
    for s in (0, 7, EO_SLICES - 1):
        yield f"k-slice-{s}-left-out-of-the-lds-sum", c.final(c.pre - conv3x3(c.x, slice_weight(c, s))), None
    B, H, W, cout = c.pre.shape
    if cout < 8 and B > 1:
        bad, where = c.want.clone(), torch.zeros_like(c.want, dtype=torch.bool)
        bad[1:, :, :, 0], where[1:, :, :, 0] = 0.0, True
        yield "output-channels->=Cout-written", bad, where


def enc_conv_out_cases() -> List[tuple]:
    return [(B, co, cin, H, W) for B in ENC_OUT_B for co in ENC_OUT_COUT for cin in ENC_OUT_CIN for H, W in ENC_OUT_HW]


# ---- cd360_rowdot1_bf16 / cd360_rowdot4_bf16 ---------------------------------------------------------------------------------------------
ROWDOT = dict(h=16, w=16)
# d in [-16, 16] leaves 4 .. 14 % of dh to round (four products of at most 256 each), below the floor of 15 %: every shape is built on
# that range (held to the exactness conditions and the fault models) AND on [-32, 32], which meets the floors (19 .. 50 % round, >= 15 % ties)
ROWDOT_BWD_D = (16, 32)
ROWDOT_MAX_WAVES = 3072
ROWDOT_SMALL = [(rows, C) for C in (8, 64, 504, 512, 520, 1024, 1032, 1536, 2048) for rows in (1, 37)]
ROWDOT_MULTI = [(rows, C) for C in (64, 520) for rows in (3072, 3073, 6149)]  # one row per wave; one wave with two; two each and a remainder


def rowdot_waves(rows: int) -> int:
    """Waves of a launch, restated from rowdot_pick: min(rows, 3072) rounded up to whole workgroups of four."""
    return -(-min(rows, ROWDOT_MAX_WAVES) // 4) * 4


@dataclass(frozen=True)
class RowdotCase:
    nw: int
    rows: int
    C: int
    h: torch.Tensor    # [rows, C]
    w: torch.Tensor    # [nw, C]
    out: torch.Tensor  # [rows, nw] float64, exact integers


def check_rowdot(c: RowdotCase) -> None:
    assert is_bf16(c.h) and is_f32(c.w)
    bound = (c.h.abs() @ c.w.abs().t()).max().item()
    assert bound < TWO24, f"sum |h||w| = {bound} reaches 2^24"
    assert torch.equal(c.out, c.h @ c.w.t())
    exact_f32(c.out)


@functools.lru_cache(maxsize=None)
def rowdot_case(nw: int, rows: int, C: int) -> RowdotCase:
    g = torch.Generator().manual_seed(_seed("rowdot", nw, rows, C))
    h, w = _ints(g, (rows, C), ROWDOT["h"]), _ints(g, (nw, C), ROWDOT["w"])
    c = RowdotCase(nw, rows, C, h, w, h @ w.t())
    check_rowdot(c)
    return c


def rowdot_faults(c: RowdotCase) -> Iterator[Fault]:
    nwaves = rowdot_waves(c.rows)
    later = (torch.arange(c.rows) >= nwaves)[:, None]
    if c.rows > nwaves:
        bad = c.out.clone()
        idx = torch.arange(c.rows)
        bad[nwaves:] = c.out[idx[nwaves:] % nwaves]
        yield "second-row-reuses-the-first-row's-data", bad, later.expand_as(bad)
        yield "second-row-skipped", with_nan(c.out, later), later.expand_as(c.out)
        bad = c.out.clone()  # the hand-over vn -> v one row late: every later row of a wave sees the row before it
        bad[2 * nwaves:] = c.out[nwaves:c.rows - nwaves]
        if c.rows > 2 * nwaves:
            yield "third-row-sees-the-second-row's-data", bad, (torch.arange(c.rows) >= 2 * nwaves)[:, None].expand_as(bad)
    pad = -(-c.C // 512) * 512 - c.C
    if pad and c.nw == 4 and c.rows > 1:  # lanes of the last 512-channel group at c >= C read on: the next row's head against the next weight row's
        hf = torch.cat([c.h.reshape(-1), torch.zeros(pad, dtype=torch.float64)])
        wf = torch.cat([c.w.reshape(-1), torch.zeros(pad, dtype=torch.float64)])
        hp = hf[(torch.arange(c.rows)[:, None] + 1) * c.C + torch.arange(pad)[None]]
        wp = wf[(torch.arange(c.nw)[:, None] + 1) * c.C + torch.arange(pad)[None]]
        yield "lane-of-the-last-group-reads-past-C", c.out + hp @ wp.t(), None
    yield "last-8-channels-dropped", c.out - c.h[:, -8:] @ c.w[:, -8:].t(), None


# ---- cd360_rowdot4_bwd_bf16 --------------------------------------------------------------------------------------------------------------
ROWDOT_BWD = [(rows, C) for rows in (1, 255, 256, 257, 1000) for C in (8, 64, 520, 1280)]
ROWDOT_BWD_BIG = (16400, 1024)  # 2,099,200 vectors of 8: above the 8192 x 256 threads of the dh grid
DH_GRID_VECTORS, DW_SLAB_ROWS = 8192 * 256, 256
ROWDOT_BWD_MIN_ROUNDING_OUTPUTS = 512  # truncation is held to changing bits from this many outputs on (fewer: a handful of ties)


@dataclass(frozen=True)
class RowdotBwdCase:
    rows: int
    C: int
    d: torch.Tensor    # [rows, 4] fp32 integers
    h: torch.Tensor    # [rows, C]
    w: torch.Tensor    # [4, C]
    dh_pre: torch.Tensor  # [rows, C] exact d w
    dw: torch.Tensor      # [4, C] exact d^T h

    @property
    def dh(self) -> torch.Tensor:
        return rne(self.dh_pre)


def check_rowdot_bwd(c: RowdotBwdCase) -> None:
    assert is_bf16(c.h) and is_f32(c.w) and is_f32(c.d)
    assert (c.d.abs() @ c.w.abs()).max().item() < TWO24
    bound = (c.d.abs().t() @ c.h.abs()).max().item()
    assert bound < TWO24, f"sum |d||h| = {bound} reaches 2^24"
    assert torch.equal(c.dh_pre, c.d @ c.w) and torch.equal(c.dw, c.d.t() @ c.h)
    exact_f32(c.dw)


@functools.lru_cache(maxsize=4)
def rowdot_bwd_case(rows: int, C: int, amp: int = 32) -> RowdotBwdCase:
    assert amp in ROWDOT_BWD_D
    for attempt in range(256):
        g = torch.Generator().manual_seed(_seed("rowdot_bwd", rows, C, amp) + attempt)
        d, h, w = _ints(g, (rows, 4), amp), _ints(g, (rows, C), ROWDOT["h"]), _ints(g, (4, C), ROWDOT["w"])
        c = RowdotBwdCase(rows, C, d, h, w, d @ w, d.t() @ h)
        if amp == 16 or floors_met(c.dh_pre):
            check_rowdot_bwd(c)
            return c
    raise AssertionError(f"no rowdot4_bwd case for {rows} x {C} meets the rounding floors")


def rowdot_bwd_faults(c: RowdotBwdCase) -> Iterator[Tuple[str, str, torch.Tensor, Optional[torch.Tensor]]]:
    """(name, which output: "dh" | "dw", defective output, mask)."""
    if c.rows * c.C >= ROWDOT_BWD_MIN_ROUNDING_OUTPUTS and rounding_shares(c.dh_pre)[2] > 0:
        yield "truncation", "dh", truncate(c.dh_pre), None
    j = int(c.d.abs().sum(0).argmax())  # (a column of zeros dropped is no defect: the one that carries most)
    yield "one-d-column-left-out", "dh", rne(c.dh_pre - c.d[:, j:j + 1] @ c.w[j:j + 1]), None
    if c.rows * c.C // 8 > DH_GRID_VECTORS:
        m = (torch.arange(c.rows * c.C) >= DH_GRID_VECTORS * 8).reshape(c.rows, c.C)
        yield "elements-beyond-the-first-grid-trip-unwritten", "dh", with_nan(c.dh, m), m
    r0 = (c.rows - 1) // DW_SLAB_ROWS * DW_SLAB_ROWS
    if r0 > 0:
        yield "last-slab-skipped", "dw", c.dw - c.d[r0:].t() @ c.h[r0:], None
    if c.rows >= 4:
        yield "fourth-wave's-rows-left-out-of-the-lds-sum", "dw", c.dw - c.d[3::4].t() @ c.h[3::4], None
    yield "last-row-dropped", "dw", c.dw - c.d[-1:].t() @ c.h[-1:], None


# ---- cd360_concat_channels_bf16 ----------------------------------------------------------------------------------------------------------
GRID_VECTORS = 4096 * 256  # the elementwise grid's cap: 1,048,576 vectors of 16 bytes per trip
CONCAT_SMALL = [(8, 8, 333), (64, 24, 200), (320, 640, 150)]
CONCAT_BIG = (320, 640, 8750)  # 1,050,000 vectors


def concat_fill(pixels: int, ch: int, salt: int) -> torch.Tensor:
    """[pixels, ch] int16 bit patterns.  bf16 has 65536 patterns, fewer than these tensors have elements, so what is distinct is the unit
    the kernel moves: every 8-element vector differs from every other vector of both inputs (its index in words 0 .. 2, the tensor in
    word 3), and the words of a vector differ from each other."""
    n = pixels * ch // 8
    i = torch.arange(n, dtype=torch.int64)
    words = [i & 0x7FFF, (i >> 15) & 0x7FFF, 0x4000 | (i % 8191), torch.full_like(i, 0x3000 + salt)] + [0x1000 * (e - 3) + (i * (2 * e + 1)) % 4093 for e in range(4, 8)]
    v = torch.stack(words, 1)
    v = torch.where(v >= 0x8000, v - 0x10000, v)
    return v.to(torch.int16).reshape(pixels, ch)


@functools.lru_cache(maxsize=2)
def concat_case(ca: int, cb: int, pixels: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(a [pixels, ca], b [pixels, cb], want [pixels, ca + cb]) int16 bit patterns of bf16 tensors."""
    a, b = concat_fill(pixels, ca, 1), concat_fill(pixels, cb, 2)
    return a, b, torch.cat([a, b], 1)


def check_concat(ca: int, cb: int, pixels: int) -> None:
    a, b, want = concat_case(ca, cb, pixels)
    vec = torch.cat([a.reshape(-1, 8), b.reshape(-1, 8)]).to(torch.int64) & 0xFFFF
    keys = vec[:, 0] | vec[:, 1] << 16 | vec[:, 3] << 32
    assert keys.unique().numel() == vec.shape[0], "two vectors agree"
    assert want.shape == (pixels, ca + cb)


def concat_faults(ca: int, cb: int, pixels: int) -> Iterator[Fault]:
    a, b, want = concat_case(ca, cb, pixels)
    w64 = want.double()
    if pixels * (ca + cb) // 8 > GRID_VECTORS:
        m = (torch.arange(want.numel()) >= GRID_VECTORS * 8).reshape(want.shape)
        yield "elements-beyond-the-first-grid-trip-unwritten", with_nan(w64, m), m
    if ca != cb:
        yield "b-read-at-a's-row-pitch", torch.cat([a, b.reshape(-1)[(torch.arange(pixels)[:, None] * ca + torch.arange(cb)[None]) % b.numel()]], 1).double(), None
    bad = w64.clone()  # the first vector behind the split taken from a (the next pixel's head), not from b
    bad[:, ca:ca + 8] = torch.roll(a, -1, 0)[:, :8].double()
    yield "split-one-vector-late", bad, None
    yield "last-pixel-not-written", with_nan(w64, (torch.arange(pixels) == pixels - 1)[:, None]), None


# ---- cd360_geglu_bf16 / cd360_geglu_bwd_bf16 ---------------------------------------------------------------------------------------------
GEGLU_SMALL = [(rows, inner) for rows in (1, 37) for inner in (8, 320)]
GEGLU_BIG = (4100, 2048)  # 1,049,600 vectors
GATE_GRID = (-8.0, -6.0, -4.0, -2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 4.0, 6.0, 8.0)
GEGLU_MEASURED = dict(y=2.37, dx=1.72, dg=2.63)  # worst fp32 CPU error in units of 2^-24 scale over every case below
GEGLU_C = 10.5                                   # four times the largest of them
U24 = 2.0 ** -24


@dataclass(frozen=True)
class GegluCase:
    rows: int
    inner: int
    x: torch.Tensor   # [rows, inner] bf16 values
    g: torch.Tensor
    dy: torch.Tensor

    @property
    def proj(self) -> torch.Tensor:
        return torch.cat([self.x, self.g], 1)


def gelu64(g: torch.Tensor) -> torch.Tensor:
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def dgelu64(g: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def geglu_reference(c: GegluCase) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """{"y" | "dx" | "dg": (want float64, scale)}"""
    m = c.g.abs().clamp_min(1.0)
    return dict(y=(c.x * gelu64(c.g), c.x.abs() * m), dx=(c.dy * gelu64(c.g), c.dy.abs() * m), dg=(c.dy * c.x * dgelu64(c.g), (c.dy * c.x).abs() * m))


def geglu_fp32(c: GegluCase) -> Dict[str, torch.Tensor]:
    """The same formulas evaluated plainly in fp32 on the CPU (the yardstick c is set by)."""
    x, g, dy = c.x.float(), c.g.float(), c.dy.float()
    cdf = 0.5 * (1.0 + torch.erf(g * 0.70710678118654752))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * g * g)
    return dict(y=x * (g * cdf), dx=dy * g * cdf, dg=dy * x * (cdf + g * pdf))


@functools.lru_cache(maxsize=2)
def geglu_case(rows: int, inner: int) -> GegluCase:
    gen = torch.Generator().manual_seed(_seed("geglu-thin", rows, inner))
    x, g, dy = [(torch.randn(rows, inner, generator=gen) * 2).to(BF).double() for _ in range(3)]
    grid = torch.tensor(GATE_GRID, dtype=torch.float64)
    flat = g.reshape(-1)
    at = torch.arange(0, flat.numel(), 3)
    flat[at] = grid[(at // 3) % len(GATE_GRID)]
    c = GegluCase(rows, inner, x, g, dy)
    check_geglu(c)
    return c


def check_geglu(c: GegluCase) -> None:
    assert is_bf16(c.x) and is_bf16(c.g) and is_bf16(c.dy)
    assert c.rows * c.inner < len(GATE_GRID) * 3 or set(GATE_GRID) <= set(c.g.unique().tolist()), "the gate grid is not in the case"


def band(want: torch.Tensor, scale: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lo, hi) bf16; works on any device."""
    delta = GEGLU_C * U24 * scale
    return bf16_of(want - delta), bf16_of(want + delta)


def band_accepts(got: torch.Tensor, want: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    lo, hi = band(want, scale)
    g = got.double()
    return (g >= lo.double()) & (g <= hi.double())


def band_error(got: torch.Tensor, want: torch.Tensor, scale: torch.Tensor) -> float:
    """Worst error / delta, the error of an element being the least |v - want| over the fp32 values v that round to the bf16 value
    seen (|got - want| minus half a bf16 step of got, at least 0), as gemm_cases.geglu_accepts measures it."""
    g = got.double()
    half = torch.where(g == 0, torch.zeros_like(g), 2.0 ** (torch.frexp(g)[1].double() - 9))
    err = ((g - want).abs() - half).clamp_min(0.0)
    delta = GEGLU_C * U24 * scale
    ratio = torch.where(delta > 0, err / delta.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return ratio.max().item()


def fp32_error_units(c: GegluCase) -> Dict[str, float]:
    """Worst |fp32 - float64| in units of 2^-24 scale, per output."""
    ref, got = geglu_reference(c), geglu_fp32(c)
    out = {}
    for k, (want, scale) in ref.items():
        live = scale > 0
        assert bool((got[k].double()[~live] == 0).all())
        out[k] = ((got[k].double() - want).abs()[live] / (U24 * scale[live])).max().item() if bool(live.any()) else 0.0
    return out


def geglu_faults(c: GegluCase) -> Iterator[Tuple[str, str, torch.Tensor]]:
    """(name, output, defective bf16 output)."""
    ref = geglu_reference(c)
    tanh = 0.5 * c.g * (1 + torch.tanh(math.sqrt(2 / math.pi) * (c.g + 0.044715 * c.g ** 3)))
    yield "tanh-form-gelu", "y", (c.x * tanh).to(BF)
    yield "tanh-form-gelu", "dx", (c.dy * tanh).to(BF)
    yield "value-and-gate-swapped", "y", (c.g * gelu64(c.x)).to(BF)
    yield "density-term-of-gelu'-left-out", "dg", (c.dy * c.x * 0.5 * (1.0 + torch.erf(c.g / math.sqrt(2.0)))).to(BF)
    yield "dx-and-dg-swapped", "dx", ref["dg"][0].to(BF)
    if c.inner >= 16:
        for k in ("y", "dx", "dg"):
            yield "columns-shifted-by-one-vector", k, torch.roll(ref[k][0], 8, 1).to(BF)
    if c.rows * c.inner // 8 > GRID_VECTORS:
        m = (torch.arange(c.rows * c.inner) >= GRID_VECTORS * 8).reshape(c.rows, c.inner)
        for k in ("y", "dx", "dg"):
            yield "elements-beyond-the-first-grid-trip-unwritten", k, with_nan(ref[k][0].to(BF), m).to(BF)


# ---- how many cases the GPU file builds, per family --------------------------------------------------------------------------------------
def case_counts() -> Dict[str, int]:
    n_out = len(vae_conv_out_cases())
    return dict(out_conv4=len(out_conv4_cases()), stage_in=len(stage_in_cases()), emb_act=len(emb_cases()), vae_conv_in=len(vae_conv_in_cases()),
                vae_conv_out=n_out, vae_conv_out_u8=n_out, vae_enc_conv_out=len(enc_conv_out_cases()),
                rowdot1=len(ROWDOT_SMALL + ROWDOT_MULTI), rowdot4=len(ROWDOT_SMALL + ROWDOT_MULTI), rowdot4_bwd=len(ROWDOT_BWD_D) * (len(ROWDOT_BWD) + 1),
                concat_channels=len(CONCAT_SMALL) + 1, geglu=len(GEGLU_SMALL) + 1, geglu_bwd=len(GEGLU_SMALL) + 1)
