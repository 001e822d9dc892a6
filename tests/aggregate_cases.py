"""Per-element cases for the fused FeatureNeRF render (csrc/nerf_fused.hip) and its backward (csrc/nerf_bwd.hip) through their C ABI
(ops.nerf_mlp_aggregate, ops.nerf_mlp_aggregate_bwd), where Y, zP, lv, cview, Wk and img_map are free inputs: inputs, a float64 reference
of the operator itself, an error model per output element, an fp32 emulation of the kernels' order, and fault models.  CPU only: nothing
here loads the HIP library.

THE REFERENCE is a float64 restatement of the operator on the fp32 geometry (render_cases.geometry: the chain of csrc/cd360_geom.h bit for
bit, which tests/test_aggregate_gpu.py asserts again for every shape here), for view i, sample p = ray * S + depth, channel c:
    z_i = zP_i(ray) + sum_c w_c Y[pix_c] + Wk . bf16(F(q_i))     a = softmax_i(cview_i + sum_c w_c lv[pix_c])     g = sum_i a_i silu(z_i)
x0, y0, tx, ty, mask, q are the fp32 chain's; the only fp32 product kept is w_c = (1 - tx)(1 - ty) etc., zero on corners outside the image.
F(q) is restated as far as it can be: the phase rev = fract(q 2^(kf - 9)) is a power-of-two scaling and a fract, exact on the fp32 q; the
sin / cos columns are sin / cos(2 pi rev) in float64, the raw columns bf16(q), the pad columns zero, the order nerf.xyz_k_columns'.
tests/test_aggregate_cpu.py ties this to oracle.pose_path.nerf_module at 1e-10 (tables built in float64 from FeatureNeRFEncoding weights),
in everything but one thing the kernels do on purpose: the oracle's frequency bands are a float32 tensor, 2^k fl32(pi) like the
reference's buffer, the kernels' period is exactly one revolution (4e-4 rad at the phases of `far`; features move by 1e-5: part of the
1e-2 budget of the render parity tests, not of this reference).  With grads the backward outputs come from float64 autograd through
the same restatement: dz, dlogit (gradients at z and at the logits), dY, dlv, dcview, dzP, dWk.

SHAPES (C, r, S, b, n), at most 1.11 M (view, sample, channel) triples:
  hostile8   ( 64,  8, 6, 1, 6)  the hostile cameras of render_cases.cameras; 12 whole tiles
  hostile12  (128, 12, 5, 2, 6)  hostile + ring, xy and depth jitter (xs != ys, t [hw, S]); 720 samples = two 512-sample workgroups and a
                                 ragged last tile of 16; views without a live corner beyond all four image borders; two channel slices
  n1         (192,  8, 3, 1, 1)  one view: the record pipeline's shortest form; three slices
  n2, n3     ( 64,  5, 7, 1, 2 | 3)  prologue / epilogue of "two views ahead"; odd r; ragged tile of 15; n2 with jitter
  ring7      ( 64,  6, 4, 1, 7)  the ring of synth.pose_batch, n = 7, jitter
  imgmap     ( 64,  8, 6, 2, 6)  img_map (2,0,2,1,1,0, 1,2,0,0,2,1): 3 table images for 12 (batch, view) pairs, the images 3 apart
Sample classes (render_cases.sample_classes) present: partial, behind, mask0, rest at hostile12 (`allmask0` needs r = 16 under these cameras).

INPUT FAMILIES (all eight on hostile8 and hostile12; `plain` and `index` on the other shapes):
  plain      Y, zP bf16 randn, lv 2 randn, cview randn, Wk = a FusedNerfWeights.Wk_f32 with unit rows (|z| <= 14)
  tables     Wk = 0: no encodings, the tightest bar
  index      Wk = 0; Y[img, pix, c], zP[img, ray, c] = integers / 4 that move by >= 1 / 4 when exactly one of pixel -> any of its eight
             neighbours, ray -> neighbour, 16-channel group, slice, table image changes
  input-a/b  Y = 0, zP small, Wk[c, :] = one +-2^j (j = -2 .. 1) at input kappa(c).  A slice has 64 channels and there are 99 live inputs,
             so ONE Wk cannot walk them all inside a slice: the two families together do, shifted by 37 from slice to slice.  Every sin /
             cos input and raw coordinate alone in a channel, for `far` (|q| = 37: phases of thousands of revolutions) and ordinary views
  onehot     planted winners, at least 200 natural-log units clear of every other view (their exp2 is exactly 0 in fp32), see
             _onehot_logits; zP of a (view, ray) that is no planted winner on that ray is +-2^10: the answer is silu(z_winner) and a leak is
             enormous.  Views without a live corner (logit = cview alone) win 1009 samples of hostile12.  "Every view in every tile" is out
             of reach under these cameras (check_builders says why); reached: every view wins in >= 74 % of its tiles, >= 3 winners per
             tile, 98 % of the samples have a clear winner, 16 - 21 changes of winner per 32-sample tile
  equal      lv = 0, cview equal: weights 1 / n
  far-apart  logits in [-60, 60] (+-50 per texel on a cview ramp of 20 that rises to the last view in batch element 0, falls in element
             1): differences up to 118, the maximum late (a rescale of the one-pass accumulator at every view before it) and early

ERROR MODEL, per element.  Units: EPS = 2^-19 (fp32 slack), DELTA_F = 2^-8 per generated sin / cos input (2^-9 its bf16 rounding, 2^-9 for
v_sin / v_cos and a rounding decision they flip), L_i = |cview_i| + sum_c w_c |lv_c|.
  z slack      dz_i = EPS (|zP_i| + sum_c w_c |Y_c| + sum_k |Wk_k F_k|) + DELTA_F sum_{k sin/cos} |Wk_k|   (raw columns: restated exactly)
  weight       rho_i = 2^-19 (L_i + max_j L_j): relative allowance of a softmax weight, + 2^-126 absolute (fp32 underflow)
  g            bf16(g) + 1.1 sum_i a_i dz_i + EPS sum_i a_i |silu(z_i)| + sum_i a_i rho_i |silu(z_i) - g|
  logits       2^-21 L_i (five fp32 roundings)
  lse          5.5e-7 * (max L + 1 | l (1 + sum_i a_i (L_i + max L))): four times the fp32 emulation's own worst (1.35e-7 in these units),
               the rule of tests/test_attn_tile_gpu.py
  dz           bf16(dz) + (a_i (EPS + rho_i) + 2^-126) |dg| |silu'(z_i)| + a_i |dg| 0.5 dz_i                     (|silu''| <= 0.5)
  dlogit       with e_i = <dg, silu(z_i)> over all channels, E_i = sum_c |dg_c| (EPS |silu(z_ic)| + 1.1 EPS zabs_ic)
               + 1.1 DELTA_F sum_k |sum_c dg_c silu'(z_ic) Wk_ck|  (one input's error reaches e_i through every channel at once, signs kept):
               a_i (E_i + sum_j a_j E_j) + da_i |e_i - mean| + a_i sum_j da_j |e_j|,  da = a (EPS + rho) + 2^-126
  dY, dlv      the float64 scatter of the contributions' own bars through the same weights + EPS sum |contribution| (atomics: any order);
               dY accumulates the fp32 dz, not the stored bf16 one, so no 2^-8 term
  dcview       sum over the samples of the dlogit bars + EPS sum |dlogit|
  dzP, dWk     (host reductions of grad.NerfAggregateFn on the stored bf16 dz; dWk one GEMM-TN with bf16 operands, fp32 accumulation) the
               operands' bars through the sums + EPS sum |term| + bf16(result)
  bf16(x)      2^-8 |x| + 2^-133: the project's bar for one bf16 rounding, and the spacing of bf16's subnormals
No element is excluded anywhere.

EPS is the smallest power of two for which emulate() / emulate_bwd() -- torch fp32 in the kernels' order: fma chains over the corners,
online or final-maximum softmax, g * (1 / l), the backward's chunked dlogit -- stay within a TENTH of the fp32 part of every bar (the bar
without bf16(.) and without DELTA_F, which the emulation does not incur: stricter than a tenth of the whole bar) on 100 % of the elements
of every case; the factor ten is the margin for v_exp_f32 / v_rcp_f32, which the emulation does not model.  Worst emulation err / bar at
2^-19: g 0.082 (hostile8 input-b; 0.164 at 2^-20), dz 0.071, dlogit 0.025, dY 0.044, dlv 0.016, dcview 0.002; logits 0.364 of their own bar.

CORRECTIONS to the first statement of the model (three terms for g: bf16 rounding, EPS slack, DELTA_F), each found by a failing check:
  1. rho.  The logits' own roundings move the softmax weights: logit * log2(e) and the subtraction of the maximum are rounded at the size
     of the logits, not of their differences.  Without rho the emulation reaches 0.29 of the fp32 bar of g and 1.6 (far-apart) / 54 (onehot)
     times that of dz.
  2. dlogit.  The deterministic kernel forms sum_j a_j e_j from the stored terms, so a weight's error reaches every view of the sample
     through |e_j|, not |e_j - mean| (onehot: 14 times the bar otherwise, with a_winner = 1 - 2e-3).
  3. Subnormals.  Where a view's weight is e^-90, dz = a dg silu'(z) is below 2^-126: v_exp_f32 returns zero for a weight below 2^-126
     (the 2^-126 in da), and the stored bf16 keeps fewer than eight bits (2^-133).  Found on the MI355X: four far-apart backward cases
     measured 6.3 and 12.8 bars at elements of 4e-41, which the CPU emulation rounded to bf16 reproduces to four digits; with the 2^-133
     the same cases measure 0.821 and 0.965, which the emulation reproduces once its exp2 flushes results below 2^-126.  The kernel's
     own multiplications and its stores keep subnormals.
EPS was not touched by any of them."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

import torch

import render_cases as RC
import weights as W
from oracle import pose_path as O

F64, F32 = torch.float64, torch.float32
KP = 112                  # the kernel's padded input count (cd360_nerf_k_padded)
TILE, WG_PTS = 32, 512    # samples per wave tile and per workgroup (nerf_fused.hip: 4 waves x TILES_PER_WAVE x 32)
EPS = 2.0 ** -19          # the fp32 slack unit of the error model (module docstring)
DELTA_F = 2.0 ** -8       # allowance per generated sin / cos input
TINY = 2.0 ** -126        # fp32 underflow: a softmax weight below it may come back as zero
RHO_UNIT = 2.0 ** -19     # relative allowance of a softmax weight per unit of |cview| + sum w |lv| (four times the logits' bar)
LSE_REL = 5.5e-7          # lse bar: LSE_REL * lse_scale, four times the fp32 emulation's own worst error (1.35e-7)
LOG2E = torch.tensor(1.4426950408889634, dtype=F32)
LN2 = torch.tensor(0.6931471805599453, dtype=F32)
bf = RC.bf


# ------------------------------------------------------------------------------------------------ shapes
@dataclass(frozen=True)
class Shape:
    name: str
    C: int
    r: int
    S: int
    b: int
    n: int
    cams: str                     # "hostile" (render_cases.cameras), "hostile:<views>" (a subset of its views), "ring" (synth.pose_batch)
    jitter: bool                  # stratified mode: xs != ys, t is [hw, S]
    img_map: Optional[Tuple[int, ...]] = None

    @property
    def hw(self):
        return self.r * self.r

    @property
    def P(self):
        return self.r * self.r * self.S


SHAPES = {s.name: s for s in (
    Shape("hostile8", 64, 8, 6, 1, 6, "hostile", False),
    Shape("hostile12", 128, 12, 5, 2, 6, "hostile", True),
    Shape("n1", 192, 8, 3, 1, 1, "ring", False),
    Shape("n2", 64, 5, 7, 1, 2, "hostile:skewed,far", True),
    Shape("n3", 64, 5, 7, 1, 3, "hostile:turned,skewed,far", False),
    Shape("ring7", 64, 6, 4, 1, 7, "ring", True),
    Shape("imgmap", 64, 8, 6, 2, 6, "hostile", False, img_map=(2, 0, 2, 1, 1, 0, 1, 2, 0, 0, 2, 1)),
)}
FAMILIES = ("plain", "tables", "index", "input-a", "input-b", "onehot", "equal", "far-apart")
# every family on the first two shapes; the others carry `plain` and `index` (the family that sees a wrong row, ray, view or image)
CASES = [(s, f) for s in ("hostile8", "hostile12") for f in FAMILIES] + [(s, f) for s in ("n1", "n2", "n3", "ring7", "imgmap") for f in ("plain", "index")]
GRAD_CASES = [c for c in CASES if c[0] in ("hostile8", "hostile12", "n1", "n3", "imgmap")]


def case_id(c) -> str:
    return f"{c[0]}-{c[1]}"


@functools.lru_cache(maxsize=None)
def cameras(name: str) -> torch.Tensor:
    sh = SHAPES[name]
    if sh.cams == "ring":
        from cd360 import synth
        from cd360.cameras import pack_cameras
        return pack_cameras(synth.pose_batch(sh.b, sh.n, seed=RC.CAM_SEED + sh.n)).float().contiguous()
    cams = RC.cameras(sh.b)
    if ":" in sh.cams:
        cams = cams[:, [0] + [1 + RC.VIEWS.index(v) for v in sh.cams.split(":")[1].split(",")]]
    assert cams.shape == (sh.b, sh.n + 1, 16)
    return cams.contiguous()


# ------------------------------------------------------------------------------------------------ geometry
@functools.lru_cache(maxsize=None)
def geometry(name: str, dtype=F32) -> SimpleNamespace:
    """The coordinate chain of oracle/pose_path.py (= csrc/cd360_geom.h bit for bit in fp32) on the shape's cameras, flattened to samples
    p = ray * S + depth: x0, y0, mask [b, n, P] integers, tx, ty [b, n, P] and q [b, n, P, 3] in `dtype`; xs, ys, t are the fp32 inputs."""
    sh = SHAPES[name]
    xy, dj = RC.jitter(sh.r, sh.S) if sh.jitter else (None, None)
    t = O.depth_samples(sh.S, RC.FAR, 0.0, dj, sh.hw)[0][0]
    t = (t if sh.jitter else t[0]).contiguous()
    geo = RC.geometry(cameras(name).to(dtype), sh.r, t, xy)
    x0, y0, tx, ty, mask = O.bilinear_corners(geo["grid"], sh.r)
    fl = lambda x: x.reshape(sh.b, sh.n, sh.P, *x.shape[4:])
    if sh.jitter:
        assert not torch.equal(geo["xs"], geo["ys"]) and t.shape == (sh.hw, sh.S)
    return SimpleNamespace(xs=geo["xs"].contiguous(), ys=geo["ys"].contiguous(), t=t, x0=fl(x0).long(), y0=fl(y0).long(), tx=fl(tx), ty=fl(ty),
                           mask=fl(mask).long(), q=fl(geo["q"]), grid=geo["grid"], points=geo["points"])


def corner_tables(sh: Shape, geo, img: torch.Tensor, masked: bool = True, swap_ne_sw: bool = False):
    """(pix [4] of [b, n, P] rows of the flattened tables, w [4] of [b, n, P] float64).  The weights are the products (1 - tx)(1 - ty) ...
    in the dtype of the geometry -- the one fp32 product the reference keeps -- and zero on corners outside the image."""
    r = sh.r
    wts = [(1 - geo.tx) * (1 - geo.ty), geo.tx * (1 - geo.ty), (1 - geo.tx) * geo.ty, geo.tx * geo.ty]
    pix, w = [], []
    for bit, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        idx = (geo.y0 + dy).clamp(0, r - 1) * r + (geo.x0 + dx).clamp(0, r - 1)
        pix.append(img[:, :, None] * sh.hw + idx)
        ok = ((geo.mask >> bit) & 1).bool()
        w.append((torch.where(ok, wts[bit], torch.zeros_like(wts[bit])) if masked else wts[bit]).double())
    if swap_ne_sw:
        pix[1], pix[2] = pix[2], pix[1]
    return pix, w


# ------------------------------------------------------------------------------------------------ the generated inputs F(q)
@functools.lru_cache(maxsize=None)
def columns():
    """Per kernel input k: (kind [KP]: 0 sin, 1 cos, 2 raw, 3 pad; comp [KP]; kf [KP]) from nerf.xyz_k_columns (reference column order
    [sin f0 (xyz) .. sin f15 (xyz) | cos f0 .. f15 | q])."""
    from cd360 import nerf
    kind, comp, kf = [], [], []
    for c in nerf.xyz_k_columns(0):
        if c < 0:
            kind.append(3), comp.append(0), kf.append(0)
        elif c < 96:
            kind.append(int(c >= 48)), comp.append(c % 3), kf.append((c % 48) // 3)
        else:
            kind.append(2), comp.append(c - 96), kf.append(0)
    assert len(kind) == KP and kind.count(0) == 48 and kind.count(1) == 48 and kind.count(2) == 3
    return torch.tensor(kind), torch.tensor(comp), torch.tensor(kf)


def live_inputs():
    return [k for k, kd in enumerate(columns()[0].tolist()) if kd != 3]


def encode(q: torch.Tensor, fault: Optional[str] = None, rounded: bool = True, oracle_pi: bool = False) -> torch.Tensor:
    """F(q) [..., KP] float64 for view-space points q [..., 3].  The phase rev = fract(q 2^(kf - 9)) is a power-of-two scaling (exact in the
    dtype of q) and a fract, sin / cos (2 pi rev) are float64, the raw columns are q, the pad columns zero; rounded: every column goes
    through bf16 as the kernel's B operand does.  fault (tests/test_aggregate_cpu.py): 'sincos' | 'xy' | 'freq' | 'half' | 'raw'."""
    kind, comp, kf = (x.clone() for x in columns())
    KF = 5  # the frequency the single-frequency faults hit
    if fault == "sincos":
        sel = (kf == KF) & (kind < 2)
        kind[sel] = 1 - kind[sel]
    elif fault == "xy":
        sel = (kf == KF) & (kind < 2) & (comp < 2)
        comp[sel] = 1 - comp[sel]
    elif fault == "freq":
        kf[(kf == KF) & (kind < 2)] = KF + 1
    elif fault == "half":
        kf[(kf % 2 == 1) & (kind < 2)] -= 1
    elif fault == "raw":
        kind[(kind == 2) & (comp == 2)] = 3
    else:
        assert fault is None, fault
    x = (q[..., comp] * (2.0 ** (kf - 9).to(q.dtype))).double()
    # oracle_pi: the oracle's own argument, x 2 fl32(pi) without a reduction -- its frequency bands are a float32 tensor, as the reference's
    # buffer is, so its pi is the fp32 one (2.8e-8 off: 4e-4 rad at the phases of `far`); the kernel's period is exactly one revolution
    arg = x * (2 * float(torch.tensor(math.pi, dtype=F32))) if oracle_pi else 2 * math.pi * (x - torch.floor(x))
    out = torch.where(kind == 0, torch.sin(arg), torch.cos(arg))
    out = torch.where(kind == 2, q[..., comp].double(), out)
    out = torch.where(kind == 3, torch.zeros((), dtype=F64), out)
    return bf(out.float()).double() if rounded else out


# ------------------------------------------------------------------------------------------------ inputs
@dataclass
class Inputs:
    Y: torch.Tensor       # [ntab, hw, C] fp32 holding bf16 values
    zP: torch.Tensor      # [b * n, hw, C] fp32 holding bf16 values
    lv: torch.Tensor      # [ntab, hw] fp32
    cview: torch.Tensor   # [b, n] fp32
    Wk: torch.Tensor      # [C, KP] fp32 holding bf16 values
    dg: torch.Tensor      # [b, P, C] fp32 holding bf16 values
    img_map: Optional[torch.Tensor]  # int32 [b * n] | None
    note: dict


@functools.lru_cache(maxsize=None)
def real_wk(C: int) -> torch.Tensor:
    """FusedNerfWeights.Wk_f32 of synthetic FeatureNeRFEncoding weights, rows scaled to unit norm: Wk . F is of order 1 on ordinary views
    and a few units on `far`, whose raw coordinates are around 37."""
    from cd360 import nerf
    shapes = {"plane_coefs.0.weight": (C, C + 198), "plane_coefs.0.bias": (C,), "plane_coefs.2.weight": (C, C), "plane_coefs.2.bias": (C,),
              "nviews.weight": (1, C + 198), "nviews.bias": (1,), "decoder.weight": (4, C)}
    w = W.synth_state_dict(shapes, C)
    wk = nerf.FusedNerfWeights(*(w[k] for k in RC.NERF_KEYS)).Wk_f32
    assert wk.shape == (C, KP)
    return bf(wk / wk.norm(dim=1, keepdim=True))


def images_of(sh: Shape) -> torch.Tensor:
    """[b, n] table image of every (batch, view)."""
    if sh.img_map is None:
        return torch.arange(sh.b * sh.n).reshape(sh.b, sh.n)
    return torch.tensor(sh.img_map).reshape(sh.b, sh.n)


def _index_tables(sh: Shape, ntab: int):
    """Y[img, pix, c] and zP[img, ray, c] as integers / 4, each the sum of a pixel code (x + 2 y) mod 5 (every one of the eight neighbours of
    a pixel differs), a code of the 16-channel group inside the slice, of the slice, of the channel inside its group (mod 2) and of the table
    image: changing exactly one of pixel -> neighbour, ray -> neighbour, group, slice, image moves the entry by at least 1 / 4."""
    r, C = sh.r, sh.C
    yy, xx = torch.meshgrid(torch.arange(r), torch.arange(r), indexing="ij")
    pixc = ((xx + 2 * yy) % 5).reshape(-1).double()
    c = torch.arange(C)
    grp, slc, par = ((c % 64) // 16).double(), (c // 64).double(), (c % 2).double()
    Y = (pixc[None, :, None] + grp[None, None, :] + slc[None, None, :] + (torch.arange(ntab) % 7).double()[:, None, None] - 6.0) / 4
    zP = (4 - pixc[None, :, None] + (3 - grp)[None, None, :] - slc[None, None, :] + par[None, None, :] + (torch.arange(sh.b * sh.n) % 5).double()[:, None, None]
          - 5.0) / 4
    for t in (Y, zP):
        nb = t.reshape(t.shape[0], r, r, C)
        assert (nb[:, :, 1:] - nb[:, :, :-1]).abs().min() >= 0.25 and (nb[:, 1:] - nb[:, :-1]).abs().min() >= 0.25
        assert (nb[:, 1:, 1:] - nb[:, :-1, :-1]).abs().min() >= 0.25 and (nb[:, 1:, :-1] - nb[:, :-1, 1:]).abs().min() >= 0.25
        assert (t[..., 16:64] - t[..., :48]).abs().min() >= 0.25 and (C == 64 or (t[..., 64:] - t[..., :-64]).abs().min() >= 0.25)
        assert t.shape[0] == 1 or (t[1:] - t[:-1]).abs().min() >= 0.25
        assert torch.equal(t * 4, torch.round(t * 4)) and t.abs().max() <= 4
    return Y.float(), zP.float()


def _one_input_wk(sh: Shape, half: int):
    """Wk[c, :] = one +-2^j at input kappa(c) = live[(c % 64 + 64 half + 37 slice) mod 99]: the families `input-a` (half 0) and `input-b`
    (half 1) together walk all 99 live inputs inside every 64-channel slice (a slice has 64 channels, so one Wk cannot)."""
    live = live_inputs()
    assert len(live) == 99
    Wk = torch.zeros(sh.C, KP)
    kappa = []
    for c in range(sh.C):
        k = live[(c % 64 + 64 * half + 37 * (c // 64)) % 99]
        kappa.append(k)
        Wk[c, k] = (-1.0) ** c * 2.0 ** (c % 4 - 2)
    return Wk, kappa


def _onehot_logits(sh: Shape, geo, img: torch.Tensor, ntab: int, seed: int):
    """lv, cview with planted winners, by construction.  A texel is HOT (lv = 300) or COLD (lv = -32768); the views of a batch element
    are ranked by how many different texels a 32-sample tile reaches in them (`far` reaches ONE quad per tile: it cannot change inside a
    tile, so it is lowest) and cview = 650 rank: a higher-ranked view that is hot, or has no live corner (logit = cview alone), beats
    every lower one by 350 or more, and loses only where its texels are cold.  In every tile every view gets a target sample, chosen
    greedily: the free texels of the view's corners there are pledged hot, those of every higher-ranked view cold, and the sample is taken if
    under ALL pledges so far the view is 300 natural-log units clear of every other (the margin is evaluated, not assumed: corners may be
    partly outside, or pledged already).  Pledges never change, so a margin checked once holds.  Texels nobody pledged are hot or cold at
    random: the winner of the other samples changes from sample to sample as well.
    -> (lv [ntab, hw], cview [b, n], winner [b, P] (-1 where no view is 200 natural-log units clear), target [b, P] (-1: not a target))."""
    b, n, P, hw = sh.b, sh.n, sh.P, sh.hw
    assert sh.img_map is None
    HOT, COLD, STEP = 300.0, -32768.0, 650.0
    pix, w = corner_tables(sh, geo, img)
    pixs, ws = torch.stack(pix, -1), torch.stack(w, -1)
    ntile = -(-P // TILE)
    agility = torch.tensor([[sum(len(set(map(tuple, pixs[bi, v, t0 * TILE:(t0 + 1) * TILE].tolist()))) for t0 in range(ntile)) for v in range(n)]
                            for bi in range(b)])
    rank = agility.argsort(dim=1, stable=True).argsort(dim=1)  # [b, n]: 0 = the view that moves least
    cview = (STEP * rank).float()
    rows = [[[[(r_, x) for r_, x in zip(pixs[bi, v, p].tolist(), ws[bi, v, p].tolist()) if x > 0] for p in range(P)] for v in range(n)] for bi in range(b)]
    cvl = cview.tolist()
    state = [0] * (ntab * hw)  # 1 hot, -1 cold, 0 free
    tgt = torch.full((b, P), -1, dtype=torch.long)

    def logit(bi, u, p, free):  # the logit of view u at p with free texels counted as `free`
        return cvl[bi][u] + sum(x * (HOT if (state[r_] or free) == 1 else COLD) for r_, x in rows[bi][u][p])

    def plant(bi, tile, order, shift):  # one greedy pass over a tile -> [(sample, view)]
        used, got = set(), []
        for v in order:
            for p in sorted(tile, key=lambda p: (p - tile[0] - shift * v) % TILE):
                # (a lower-ranked view loses even where it is hot: its free texels stay free)
                if p in used or any(logit(bi, v, p, 1) - logit(bi, u, p, -1 if cvl[bi][u] > cvl[bi][v] else 1) < 300.0 for u in range(n) if u != v):
                    continue
                for u in range(n):
                    for r_, _ in rows[bi][u][p]:
                        if state[r_] == 0 and cvl[bi][u] >= cvl[bi][v]:
                            state[r_] = 1 if u == v else -1
                used.add(p)
                got.append((p, v))
                break
        return got

    for bi in range(b):
        up = sorted(range(n), key=lambda v: cvl[bi][v])
        for p0 in range(0, P, TILE):
            tile = list(range(p0, min(p0 + TILE, P)))
            best = None  # the pass that plants most views: by rank upwards / downwards, candidate samples spread differently
            for order in (up, up[::-1]):
                for shift in (5, 1, 7, 11):
                    saved = list(state)
                    got = plant(bi, tile, order, shift)
                    if best is None or len(got) > len(best[0]):
                        best = (got, list(state))
                    state[:] = saved
                    if len(best[0]) == n:
                        break
            state[:] = best[1]
            for p, v in best[0]:
                tgt[bi, p] = v
    g = torch.Generator().manual_seed(seed)
    st = torch.tensor(state)
    st = torch.where(st == 0, (torch.rand(ntab * hw, generator=g) < 0.5).long() * 2 - 1, st)
    lv = torch.where(st.reshape(ntab, hw) == 1, torch.full((ntab, hw), HOT), torch.full((ntab, hw), COLD))
    lg =cview.double()[:, :, None] + sum(w[c] * lv.double().reshape(-1)[pix[c]] for c in range(4))
    top2 = lg.topk(min(2, n), dim=1)
    clear = (top2.values[:, 0] - top2.values[:, 1] >= 200.0) if n > 1 else torch.ones(b, P, dtype=torch.bool)
    winner = torch.where(clear, top2.indices[:, 0], torch.full_like(tgt, -1))
    sel = tgt >= 0
    assert bool((winner[sel] == tgt[sel]).all()), "one-hot logits: a planted winner is not 200 clear"
    return lv, cview, winner, tgt


@functools.lru_cache(maxsize=None)
def inputs(name: str, family: str) -> Inputs:
    sh = SHAPES[name]
    geo = geometry(name)
    b, n, hw, C, P = sh.b, sh.n, sh.hw, sh.C, sh.P
    img = images_of(sh)
    ntab = b * n if sh.img_map is None else max(sh.img_map) + 1
    g = torch.Generator().manual_seed(1000 * C + 10 * sh.r + FAMILIES.index(family))
    rn = lambda *s: torch.randn(*s, generator=g)
    Y, zP, lv, cview, Wk, dg = bf(rn(ntab, hw, C)), bf(rn(b * n, hw, C)), rn(ntab, hw) * 2, rn(b, n), real_wk(C), bf(rn(b, P, C))
    if sh.img_map is not None:
        Y = bf(Y + 3.0 * (torch.arange(ntab) - 1.0)[:, None, None])  # table images far from each other
        lv = lv + 3.0 * (torch.arange(ntab) - 1.0)[:, None]
    note = {}
    if family == "tables":
        Wk = torch.zeros(C, KP)
    elif family == "index":
        Wk = torch.zeros(C, KP)
        Y, zP = _index_tables(sh, ntab)
    elif family in ("input-a", "input-b"):
        Y, zP = torch.zeros(ntab, hw, C), bf(rn(b * n, hw, C) * 0.25)
        Wk, note["kappa"] = _one_input_wk(sh, int(family == "input-b"))
    elif family == "equal":
        lv, cview = torch.zeros(ntab, hw), torch.full((b, n), 0.3)
    elif family == "far-apart":
        # logits in [-60, 60]: +-50 per texel, on a cview that rises by 20 to the LAST view in batch element 0 and falls from the first in
        # element 1 -- the maximum comes late (a rescale at every view before it) or early (none), up to 120 above the smallest logit
        ramp = torch.linspace(-10, 10, n) if n > 1 else torch.zeros(1)
        cview = torch.stack([ramp if i % 2 == 0 else ramp.flip(0) for i in range(b)]).contiguous()
        lv = ((torch.rand(ntab, hw, generator=g) < 0.5).float() * 2 - 1) * 50
    elif family == "onehot":
        lv, cview, winner, tgt = _onehot_logits(sh, geo, img, ntab, seed=C + sh.r)
        # zP of (view, ray) is +-2^10 unless that view is the planted winner of one of the ray's samples; Y stays of order 1
        plant = torch.zeros(b, n, hw, dtype=torch.bool)
        bi, pi = torch.nonzero(tgt >= 0, as_tuple=True)
        plant[bi, tgt[bi, pi], pi // sh.S] = True
        big = torch.where(torch.rand(b, n, hw, C, generator=g) < 0.5, -1024.0, 1024.0)
        zP = torch.where(plant[..., None], zP.reshape(b, n, hw, C), big).reshape(b * n, hw, C)
        note.update(winner=winner, target=tgt, plant=plant)
    else:
        assert family == "plain", family
    im = None if sh.img_map is None else torch.tensor(sh.img_map, dtype=torch.int32)
    for x in (Y, zP, Wk, dg):
        assert torch.equal(bf(x), x)
    return Inputs(Y.contiguous(), zP.contiguous(), lv.float().contiguous(), cview.float().contiguous(), Wk.contiguous(), dg.contiguous(), im, note)


# ------------------------------------------------------------------------------------------------ the float64 restatement
def restate(sh: Shape, geo, inp: Inputs, grads: bool = False, fault: Optional[str] = None, fault_arg=None, rounded_F: bool = True,
            oracle_pi: bool = False) -> SimpleNamespace:
    """z_i = zP_i(ray) + sum_c w_c Y[pix_c] + Wk . bf16(F(q_i)),  a = softmax_i(cview_i + sum_c w_c lv[pix_c]),  g = sum_i a_i silu(z_i) in
    float64 on the geometry `geo` (fp32 chain: the reference of the kernels; float64 chain with rounded_F = False: what
    tests/test_aggregate_cpu.py ties to O.nerf_module).  grads: float64 autograd for the cotangent inp.dg -- dz, dlogit (gradients at the
    intermediates z, logits), dY, dzP, dlv, dcview, dWk.  fault: a wrong kernel, restated (tests/test_aggregate_cpu.py)."""
    b, n, P, hw, C, S = sh.b, sh.n, sh.P, sh.hw, sh.C, sh.S
    Y, zP, lv, cview, Wk = (x.double().requires_grad_(grads) for x in (inp.Y, inp.zP, inp.lv, inp.cview, inp.Wk))
    img = images_of(sh)
    ntab = Y.shape[0]
    if fault == "imgmap":
        img = torch.arange(b * n).reshape(b, n) % ntab
    pix, w = corner_tables(sh, geo, img, masked=fault != "mask", swap_ne_sw=fault == "corners")
    ypix = pix
    if fault == "late":  # the rows of view i - 1 (view 0: its own) under the weights of view i
        ypix = [torch.cat([p_[:, :1], p_[:, :-1]], 1) for p_ in pix]
    ray = torch.arange(P) // S
    zray = (ray + 1).clamp(max=hw - 1) if fault == "ray" else ray
    with torch.set_grad_enabled(grads):
        Fm = encode(geo.q, fault if fault in ("sincos", "xy", "freq", "half", "raw") else None, rounded_F, oracle_pi)
        enc = Fm @ Wk.t()
        if fault == "groups-enc":  # chan_pos: the encoding term of 16-channel group j lands on group (j + 1) mod 4 of its slice
            c = torch.arange(C)
            enc = enc[..., (c // 64) * 64 + (c % 64 + 48) % 64]
        Yf, lvf = Y.reshape(ntab * hw, C), lv.reshape(ntab * hw)
        blend = sum(w[c][..., None] * Yf[ypix[c]] for c in range(4))
        if fault == "groups-Y":
            c = torch.arange(C)
            blend = blend[..., (c // 64) * 64 + (c % 64 + 48) % 64]
        elif fault == "slices":
            blend = blend[..., (torch.arange(C) + 64) % C]
        zrow = zP.reshape(b, n, hw, C)[:, :, zray]
        z = zrow + blend + enc
        logits = cview[:, :, None] + sum(w[c] * lvf[pix[c]] for c in range(4))
        lg = logits
        if fault == "tile-view":  # view fault_arg[0] dropped for the samples of tile fault_arg[1]
            v, tl = fault_arg
            drop = torch.zeros(b, n, P, dtype=torch.bool)
            drop[:, v, tl * TILE:(tl + 1) * TILE] = True
            lg = torch.where(drop, torch.full_like(lg, -float("inf")), lg)
        elif fault == "log2e":
            lg = logits * math.log(2.0)
        a = torch.softmax(lg, 1)
        if fault == "neighbour-l":  # normalised by the next sample's sum
            m = lg.amax(1, keepdim=True)
            e = torch.exp(lg - m)
            l = e.sum(1, keepdim=True)
            l = torch.cat([l[..., 1:], l[..., -1:]], -1)
            a = e / l
        s = z * torch.sigmoid(z)
        gout = (a[..., None] * s).sum(1)
    m = logits.detach().amax(1)
    out = SimpleNamespace(g=gout.detach(), logits=logits.detach(), a=a.detach(), z=z.detach(), s=s.detach(), F=Fm.detach(), pix=pix, w=w, ray=ray,
                          lse=torch.stack([m, torch.exp(logits.detach() - m[:, None]).sum(1)], -1))
    if grads:
        dz, dlogit, dY, dzP, dlv, dcview, dWk = torch.autograd.grad(gout, (z, logits, Y, zP, lv, cview, Wk), inp.dg.double())
        out.__dict__.update(dz=dz, dlogit=dlogit, dY=dY, dzP=dzP, dlv=dlv, dcview=dcview, dWk=dWk)
    return out


_REFS = {}


def reference(name: str, family: str, grads: bool = False) -> SimpleNamespace:
    """The float64 reference of a case on the fp32 geometry; computed once, shared, never modified."""
    key = (name, family, grads)
    if key not in _REFS:
        ref = restate(SHAPES[name], geometry(name), inputs(name, family), grads=grads)
        for k, v in ref.__dict__.items():
            if isinstance(v, torch.Tensor):
                assert bool(torch.isfinite(v).all()), (key, k)
        _REFS[key] = ref
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ error model
def lse_scale(ref, L: torch.Tensor) -> torch.Tensor:
    """What the error of lse = (max, sum) scales with, [b, P, 2]: the maximum is a logit (L = |cview| + sum w |lv| of the largest), the sum
    moves with every logit's error in proportion to its weight.  The lse bar is LSE_REL times this."""
    Lmax = L.amax(1)
    return torch.stack([Lmax + 1.0, ref.lse[..., 1] * (1.0 + (ref.a * (L + Lmax[:, None])).sum(1))], -1)


def bf16_round(ref: torch.Tensor) -> torch.Tensor:
    """The bar of one rounding to bf16: 2^-8 |ref| (the project's bar for a normal number) + 2^-133, the spacing of bf16's subnormals --
    below 2^-126 a stored value keeps fewer than eight bits (dz = a dg silu'(z) gets there where a view's weight is e^-90)."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -133


_BARS = {}


def bars(name: str, family: str, grads: bool = False) -> SimpleNamespace:
    """Per-element bars of every output (module docstring), float64, in the outputs' shapes.  `fp32` holds the same bars WITHOUT the terms
    a correct fp32 emulation does not incur (the bf16 rounding of a stored output, the allowance delta_F per generated input): a tenth of
    those is what tests/test_aggregate_cpu.py holds the emulation to.  Computed once per case and shared."""
    key = (name, family, grads, EPS, RHO_UNIT)
    if key not in _BARS:
        _BARS[key] = _bars(name, family, grads)
    return _BARS[key]


def _bars(name: str, family: str, grads: bool) -> SimpleNamespace:
    sh, inp, ref = SHAPES[name], inputs(name, family), reference(name, family, grads)
    kind = columns()[0]
    Wa = inp.Wk.double().abs()
    tab = lambda T, c: T.reshape(-1, T.shape[-1])[ref.pix[c]]
    zabs = inp.zP.double().abs().reshape(sh.b, sh.n, sh.hw, sh.C)[:, :, ref.ray] + sum(ref.w[c][..., None] * tab(inp.Y.double().abs(), c) for c in range(4)) \
        + ref.F.abs() @ Wa.t()
    dz_round = EPS * zabs                                                   # fp32 slack of z [b, n, P, C]
    dz_enc = DELTA_F * Wa[:, kind < 2].sum(1).expand_as(zabs)               # allowance of the generated sin / cos inputs
    L = inp.cview.double().abs()[:, :, None] + sum(ref.w[c] * inp.lv.double().abs().reshape(-1)[ref.pix[c]] for c in range(4))
    rho = RHO_UNIT * (L + L.amax(1, keepdim=True))                         # relative allowance of a softmax weight
    a = ref.a[..., None]
    soft = (a * rho[..., None] * (ref.s - ref.g[:, None]).abs()).sum(1)
    g32 = (a * 1.1 * dz_round).sum(1) + EPS * (a * ref.s.abs()).sum(1) + soft + TINY * ref.s.abs().sum(1)
    out = SimpleNamespace(g=bf16_round(ref.g) + g32 + (a * 1.1 * dz_enc).sum(1), logits=2.0 ** -21 * L,
                          lse=LSE_REL * lse_scale(ref, L), rho=rho, fp32=SimpleNamespace(g=g32))
    if not grads:
        return out
    dg = inp.dg.double()[:, None]
    sig = torch.sigmoid(ref.z)
    sp = sig * (1 + ref.z * (1 - sig))
    core = a * dg.abs()
    da = ref.a * (EPS + rho) + TINY                                        # allowance of a softmax weight [b, n, P]
    dz32 = da[..., None] * dg.abs() * sp.abs() + core * 0.5 * dz_round
    dzenc = core * 0.5 * dz_enc
    out.dz = bf16_round(ref.dz) + dz32 + dzenc
    # dlogit_i = a_i (e_i - sum_j a_j e_j), e_i = <dg, silu(z_i)>: the kernel forms e_i and the mean separately, so the slack is on the terms
    E32 = (dg.abs() * (EPS * ref.s.abs() + 1.1 * dz_round)).sum(-1)         # [b, n, P]
    # the error of ONE generated input reaches e_i through every channel at once, with the signs of dg silu'(z) Wk: the sum over the channels
    # is taken inside the absolute value (first order in delta_F, a tenth on top for the second)
    Eenc = 1.1 * DELTA_F * ((dg * sp) @ inp.Wk.double()[:, kind < 2]).abs().sum(-1)
    e = (dg * ref.s).sum(-1)                                                # e_i [b, n, P]
    dev = (e - (ref.a * e).sum(1, keepdim=True)).abs()                      # |e_i - mean|
    spread = lambda E: ref.a * (E + (ref.a * E).sum(1, keepdim=True))
    # a weight's own error da_i acts on (e_i - mean) in its own row, and through the mean sum_j (a_j e_j), which the kernel adds up from
    # the stored terms, on every row of the sample: a_i sum_j da_j |e_j| (NOT |e_j - mean|: nothing cancels inside that sum)
    dl32 = spread(E32) + da * dev + ref.a * (da * e.abs()).sum(1, keepdim=True) + TINY * (dg.abs() * ref.s.abs()).sum(-1)
    out.dlogit = dl32 + spread(Eenc)
    # scatters and sums: the contributions' own bars (before any bf16 rounding) through the same weights, + EPS sum |contribution|
    ntab = inp.Y.shape[0]

    def scatter(vals, width):  # vals [4] of [b, n, P(, C)] -> [ntab * hw(, C)]
        acc = torch.zeros(ntab * sh.hw, *([width] if width else []), dtype=F64)
        for c in range(4):
            acc.index_add_(0, ref.pix[c].reshape(-1), vals[c].reshape(-1, *([width] if width else [])))
        return acc
    wz = [ref.w[c][..., None] for c in range(4)]
    dY32 = scatter([wz[c] * (dz32 + EPS * ref.dz.abs()) for c in range(4)], sh.C).reshape(ntab, sh.hw, sh.C)
    out.dY = dY32 + scatter([wz[c] * dzenc for c in range(4)], sh.C).reshape(ntab, sh.hw, sh.C)
    dlv32 = scatter([ref.w[c] * (dl32 + EPS * ref.dlogit.abs()) for c in range(4)], 0).reshape(ntab, sh.hw)
    out.dlv = dlv32 + scatter([ref.w[c] * spread(Eenc) for c in range(4)], 0).reshape(ntab, sh.hw)
    dc32 = (dl32 + EPS * ref.dlogit.abs()).sum(-1)
    out.dcview = dc32 + spread(Eenc).sum(-1)
    # host reductions of grad.NerfAggregateFn on the kernel's bf16 dz: dzP = sum_s dz (fp32 sum, bf16 result), dWk = dz^T F (one GEMM-TN with
    # bf16 operands, fp32 accumulation, bf16 result): the operands' bars through the sums + EPS sum |term| + the result's own rounding
    dzb = out.dz.reshape(sh.b * sh.n, sh.hw, sh.S, sh.C)
    out.dzP = bf16_round(ref.dzP) + dzb.sum(2) + EPS * ref.dz.abs().reshape(sh.b * sh.n, sh.hw, sh.S, sh.C).sum(2)
    Fa = ref.F.abs().reshape(-1, KP)
    Fbar = torch.where(kind < 2, DELTA_F, 0.0).double()
    out.dWk = bf16_round(ref.dWk) + out.dz.reshape(-1, sh.C).t() @ Fa + ref.dz.abs().reshape(-1, sh.C).t() @ (EPS * Fa + Fbar)
    out.fp32.__dict__.update(dz=dz32, dlogit=dl32, dY=dY32, dlv=dlv32, dcview=dc32)
    return out


def worst(got: torch.Tensor, want: torch.Tensor, bar: torch.Tensor, mask: Optional[torch.Tensor] = None) -> float:
    """max |got - want| / bar over every element (mask: over a class; empty: 0); a non-finite error counts as inf; 0 / 0 counts as 0."""
    err = (got.double() - want).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bar)
    q = torch.where(torch.isfinite(err), q, torch.full_like(q, float("inf")))
    if mask is not None:
        q = q[mask]
    return q.max().item() if q.numel() else 0.0


def sample_classes(name: str) -> dict:
    """render_cases.sample_classes on the fp32 geometry of the shape: class -> bool [b, P]."""
    geo = geometry(name)
    return RC.sample_classes(SimpleNamespace(mask=geo.mask, q=geo.q))


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels' order
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()  # one rounding (the products here are exact in float64)


def _geo32(sh, geo, img):
    pix, w = corner_tables(sh, geo, img)
    return pix, [x.float() for x in w]


def emulate(name: str, family: str, order: str = "online", fault: Optional[str] = None):
    """The forward in torch fp32 in the kernels' order: logit = fma chain over the corners from cview; z = (Wk . F, fp32 accumulation) + zP,
    then the fma chain over the corners; silu = z * (1 / (1 + exp2(-log2e z))); order 'online': the running maximum with rescales of
    nerf_fused_kernel / nerf_fused_line_kernel, 'final': exp2(lg - final maximum) of nerf_geom_kernel + nerf_fused_rec_kernel; g * (1 / l).
    F is bf16 of the float64 sin / cos: what v_sin / v_cos, v_exp and v_rcp add is not modelled.  -> (g fp32, NOT rounded to bf16; logits;
    lse).  fault 'max-view0': the maximum taken from view 0 alone."""
    sh, inp, geo = SHAPES[name], inputs(name, family), geometry(name)
    b, n, P, hw, C = sh.b, sh.n, sh.P, sh.hw, sh.C
    pix, w = _geo32(sh, geo, images_of(sh))
    Yf, lvf = inp.Y.reshape(-1, C), inp.lv.reshape(-1)
    Fb = encode(geo.q).float()
    ray = torch.arange(P) // sh.S
    logit = inp.cview[:, :, None].expand(b, n, P).contiguous()
    for c in range(4):
        logit = _fma(w[c], lvf[pix[c]], logit)
    lg = logit * LOG2E
    z = Fb @ inp.Wk.t() + inp.zP.reshape(b, n, hw, C)[:, :, ray]
    for c in range(4):
        z = _fma(w[c][..., None], Yf[pix[c]], z)
    s = z * (1.0 / (1.0 + torch.exp2(-LOG2E * z)))
    m_run, l_run = torch.full((b, P), -float("inf")), torch.zeros(b, P)
    g = torch.zeros(b, P, C)
    for i in range(n):
        m_new = lg[:, 0] if fault == "max-view0" else torch.maximum(m_run, lg[:, i])
        sc, a = torch.exp2(m_run - m_new), torch.exp2(lg[:, i] - m_new)
        l_run = _fma(l_run, sc, a)
        if order == "online":
            g = _fma(a[..., None], s[:, i], g * sc[..., None])
        m_run = m_new
    if order == "final":
        for i in range(n):
            g = _fma(torch.exp2(lg[:, i] - m_run)[..., None], s[:, i], g)
    else:
        assert order == "online", order
    return g * (1.0 / l_run)[..., None], logit, torch.stack([m_run * LN2, l_run], -1)


def emulate_bwd(name: str, family: str, g_in: Optional[torch.Tensor] = None, fault: Optional[str] = None):
    """nerf_bwd_kernel (deterministic dlogit) + nerf_dlogit_sum_kernel + nerf_logit_bwd_kernel in torch fp32, fed the float64 reference's
    lse rounded to fp32: a = exp2(logit log2e - m log2e) * (1 / l); dz = a dg silu'(z) (NOT rounded to bf16); per 64-channel chunk
    a <dg, silu(z)>, summed in chunk order, minus a times the sum over the views; dY / dlv fp32 scatters, dcview a fp32 sum.
    fault: 'sigmoid' (silu' -> sigmoid), 'saved-g' (dlogit against g_in, the atomic form), 'unmasked-dY', 'dlv-identity'."""
    sh, inp, geo, ref = SHAPES[name], inputs(name, family), geometry(name), reference(name, family, True)
    b, n, P, hw, C = sh.b, sh.n, sh.P, sh.hw, sh.C
    img = images_of(sh)
    pix, w = _geo32(sh, geo, img)
    Yf, lvf = inp.Y.reshape(-1, C), inp.lv.reshape(-1)
    ntab = inp.Y.shape[0]
    Fb = encode(geo.q).float()
    ray = torch.arange(P) // sh.S
    logit = inp.cview[:, :, None].expand(b, n, P).contiguous()
    for c in range(4):
        logit = _fma(w[c], lvf[pix[c]], logit)
    z = Fb @ inp.Wk.t() + inp.zP.reshape(b, n, hw, C)[:, :, ray]
    for c in range(4):
        z = _fma(w[c][..., None], Yf[pix[c]], z)
    lse = ref.lse.float()
    a = torch.exp2(logit * LOG2E - (lse[..., 0] * LOG2E)[:, None]) * (1.0 / lse[..., 1])[:, None]
    sg = 1.0 / (1.0 + torch.exp2(-LOG2E * z))
    dg = inp.dg[:, None]
    dz = a[..., None] * dg * (sg if fault == "sigmoid" else sg * (1.0 + z * (1.0 - sg)))
    term = z * sg
    if fault == "saved-g":
        term = term - g_in[:, None]
    parts = [a * (dg * term)[..., k:k + 64].sum(-1) for k in range(0, C, 64)]
    acc = parts[0]
    for p_ in parts[1:]:
        acc = acc + p_
    dlogit = acc if fault == "saved-g" else acc - a * acc.sum(1, keepdim=True)
    wy = corner_tables(sh, geo, img, masked=False)[1] if fault == "unmasked-dY" else w
    dY = torch.zeros(ntab * hw, C)
    for c in range(4):
        dY.index_add_(0, pix[c].reshape(-1), (wy[c].float()[..., None] * dz).reshape(-1, C))
    lpix = pix
    if fault == "dlv-identity":
        lpix = corner_tables(sh, geo, torch.arange(b * n).reshape(b, n) % ntab)[0]
    dlv = torch.zeros(ntab * hw)
    for c in range(4):
        dlv.index_add_(0, lpix[c].reshape(-1), (w[c] * dlogit).reshape(-1))
    return SimpleNamespace(dz=dz, dlogit=dlogit, dY=dY.reshape(ntab, hw, C), dlv=dlv.reshape(ntab, hw), dcview=dlogit.sum(-1), F=Fb)


# ------------------------------------------------------------------------------------------------ the builders' own conditions
def check_builders(name: str, family: str) -> dict:
    """The conditions the cases rest on, asserted (as tests/gemm_cases.py does); returns what it counted."""
    sh, geo, inp = SHAPES[name], geometry(name), inputs(name, family)
    P, n = sh.P, sh.n
    cls = {k: int(v.sum()) for k, v in sample_classes(name).items()}
    out = {"classes": cls, "tiles": -(-P // TILE), "ragged": P % TILE}
    if name == "hostile12":
        # (`allmask0` needs r = 16 under these cameras -- tests/render_cases.py -- and no shape here is that large)
        assert all(v > 0 for k, v in cls.items() if k != "allmask0"), cls
        assert P > WG_PTS and P % TILE == 16
        m0 = geo.mask == 0  # mask 0 on both sides of the image, in x and in y
        assert all(bool((m0 & sel).any()) for sel in (geo.x0 < 0, geo.x0 >= sh.r - 1, geo.y0 < 0, geo.y0 >= sh.r - 1))
    if name in ("hostile8", "imgmap", "n3"):
        assert cls["partial"] > 0 and cls["behind"] > 0, cls
    if name in ("n2", "n3", "ring7"):
        assert P % TILE != 0
    if name in ("hostile8", "hostile12"):
        assert float(geo.q[:, RC.VIEWS.index("far")].abs().max()) > 30.0
    if sh.img_map is not None:
        im = list(sh.img_map)
        assert len(im) == sh.b * n == 12 and len(set(im)) == 3 and im != sorted(im) and im != sorted(im, reverse=True)
        if family == "plain":  # table images 3 apart (`index`: 1 / 4 apart in every entry, asserted where they are built)
            assert float((inp.Y[1:].mean((1, 2)) - inp.Y[:-1].mean((1, 2))).abs().min()) >= 2.5
    if family in ("input-a", "input-b"):
        ka, kb = _one_input_wk(sh, 0)[1], _one_input_wk(sh, 1)[1]
        for s0 in range(0, sh.C, 64):
            assert set(ka[s0:s0 + 64]) | set(kb[s0:s0 + 64]) == set(live_inputs())
        assert bool(((inp.Wk != 0).sum(1) == 1).all())
        out["kappa"] = len(set(inp.note["kappa"]))
    if family == "onehot":
        win = inp.note["winner"]
        changes, tiles, cover = 0, 0, []
        for p0 in range(0, P, TILE):
            wt = win[:, p0:p0 + TILE]
            cover.append([[bool((wt[bi] == v).any()) for v in range(n)] for bi in range(sh.b)])
            changes += int((wt[:, 1:] != wt[:, :-1]).sum())
            tiles += sh.b
        cover = torch.tensor(cover)  # [tiles, b, n]
        out["cover"] = cover.float().mean(0).tolist()
        out["winners_per_tile_min"] = int(cover.sum(-1).min())
        ref = reference(name, family)
        m0win = (win >= 0) & (geo.mask.gather(1, win.clamp(min=0)[:, None])[:, 0] == 0)
        if name == "hostile12":
            assert bool(m0win.any())  # a view without a live corner (logit = cview alone) wins somewhere
        # where a view is 200 clear the others' exp2 is exactly 0 in fp32: the answer is silu(z_winner)
        zw = ref.z.gather(1, win.clamp(min=0)[:, None, :, None].expand(-1, 1, -1, sh.C))[:, 0]
        clear = win >= 0
        assert torch.allclose(ref.g[clear], (zw * torch.sigmoid(zw))[clear], rtol=1e-12, atol=1e-60)  # (e^-200 * 2^10 of a loser)
        assert float(inp.zP.abs().max()) == 1024.0
        out.update(clear=float(clear.float().mean()), winner_changes_per_tile=changes / tiles, mask0_winners=int(m0win.sum()))
        # Every view in EVERY tile is out of reach under these cameras (where `skewed` has no live corner over a whole tile its logit is
        # constant there, and so is that of `far`, which reaches one texel quad per tile: one of the two cannot win in that tile).  What
        # the planting reaches, and what is asked: every view wins, 200 clear, in at least 70 % of the tiles of its batch element, every
        # tile has three different winners or more, 95 % of all samples have a clear winner, and it changes 12 times per tile or more.
        assert float(cover.float().mean(0).min()) >= 0.7 and out["winners_per_tile_min"] >= 3, out
        assert out["clear"] >= 0.95 and out["winner_changes_per_tile"] >= 12, out
    if family == "equal":
        assert torch.allclose(reference(name, family).a, torch.full((), 1.0 / n, dtype=F64), rtol=1e-12)
    if family == "far-apart":
        lg = reference(name, family).logits
        top = lg.argmax(1)
        spread = lg.amax(1) - lg.amin(1)
        # (`far`, the last hostile view, reaches one texel quad per tile: its logit hardly moves, so the 100-unit case is asked of the last
        # two views and the last view itself only has to be the maximum somewhere, 50 above the smallest logit)
        assert bool(((top >= n - 2) & (spread >= 100)).any()) and bool(((top == n - 1) & (spread >= 50)).any())
        assert bool(((top == 0) & (spread >= 90)).any()) and float(spread.max()) <= 120.0
        out["spread"] = float(spread.max())
    if family == "index":
        assert float(inp.Wk.abs().max()) == 0.0
    return out
