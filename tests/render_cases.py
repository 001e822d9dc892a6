"""Deterministic inputs that reach the data-dependent paths of the render kernels (ray_project, feature_gather, the fused FeatureNeRF
forward variants and backward, volume rendering forward and backward), with float64 references.  CPU only: nothing here imports the
HIP library.

HOSTILE CAMERAS.  Rows are the packed layout of csrc/cd360_geom.h (R 9 | T 3 | focal 2 | principal point 2).  Batch element 0 is one
ring camera `tgt` of synth.pose_batch as the target view and six reference views derived from it:
  same     a copy of tgt: every sample projects onto its own ray's pixel;
  turned   R = R_tgt rot_y(pi), T = -T_tgt: every sample lies behind the camera (vz < 0), the projection flips;
  skewed   tgt with focal (0.7, 3.1) and principal point (0.35, -0.2);
  away     R = R_tgt rot_x(1.2): looks past the scene;
  inside   T = T_tgt + (0, 0, -1): the camera centre lies inside the sampled depth range, vz changes sign along a ray;
  far      R = R_tgt rot_z(0.5), T = 40 T_tgt: view-space coordinates around 37 (argument reduction of the positional encoding).
A second batch element (where b = 2) is a plain ring with n = 6: batch indexing, and ordinary samples that set the tensor scale.
The projection is clipped to +-1.2, so a sample with all four corners outside (mask 0) needs 0.1 (r - 1) > 1, r >= 12: the shapes are
(C, r, S, b) = (64, 16, 24, 2), (128, 12, 5, 1) -- the smallest r with mask 0 on both sides, stratified jitter on -- and (64, 8, 6, 1),
where an outside sample always keeps live corners.  DEPTH_ROW is an explicit depth list for ops.ray_project_index: 0, -0.5, 1e-20 and
1e6 next to ordinary depths (t = 0 puts the sample on the target's camera centre: vz of `same` is zero or next to it, the nan_to_num /
clip branch of grid_coord).

The reference features, the cotangent of the features and the two weight matrices that FusedNerfWeights keeps in bf16
(plane_coefs.0.weight, plane_coefs.2.weight) hold bf16 values, so that both sides start from the same inputs and only kernel error is
measured (the standard of tests/test_kernels_gpu.py); every other parameter is fp32 on both sides.

SAMPLE CLASSES of a fused-forward output element [b, hw, S] (from the float64 chain): `allmask0` every view mask 0, `partial` some view
with 1 - 3 live corners, `behind` some view with vz < 0, `rest` none of these -- and `mask0` (some view mask 0): under the hostile cameras
`same` is always in bounds, so `allmask0` occurs in the ring element only.  An error over a class is divided by that class's own max |want|.

TEXEL-CENTRE GRIDS for feature_gather: r = 9 and r = 17 (r - 1 a power of two, so ((g + 1) / 2) (r - 1) is exact in fp32), one point on
every texel centre g = -1 + 2 i / (r - 1) (the answer is the table row, bit for bit), for r = 17 the ring one texel outside (+-1.125:
exact zeros), and the points +-1 / +-1.2.

DENSITY FAMILIES for volume rendering, 32 whole rays each, interleaved in ONE tensor [2, 112, S, C] (ray i is of family i % 7) so that
tensor-wide scales are set by `plain`:
  plain randn * 2 | vanishing randn - 14 | thick randn + 3 | opaque-first sample 0 is 12 | overflow-mid sample S // 2 is 95 (expf -> inf)
  | wall-last all -20, the last 30 | underflow all -95.
dists in [0.04, 0.14], per ray [hw, S] or shared [S]; raw inputs or pre-activated ones (sigma = fp32 exp, rgb = fp32 sigmoid, as a caller
would hand them over: the pre-activated overflow density IS +inf); S in {1, 5, 24, 64} (64 = MAX_S fills the 64-lane scans of the
backward kernel); C = 8 for fp32, C = 64 with bf16-exact features for bf16.

ERROR MODEL of volume rendering (float64 reference w64, optical depth ahead of the sample cum64):
  bw = 2^-22 + 2^-18 max(1, cum64) w64     2^-22 = two ulps of 1: the absolute error 1 - exp(-dd) inherits from expf near 1 (the fp32
                                           reference shares it); 2^-18 = 64 * 2^-24: up to 64 sequential fp32 additions in cum64
  output  sum_s bw_s |x_s| + 2^-22 sum_s |w_s x_s|   (+ 2^-8 |want| where the output is rounded to bf16)
  alphas  2^-22 (the first term of bw: the same expf near 1, dd's three roundings weigh dd e^-dd * 3 * 2^-24 < 2^-24)

OUT OF SCOPE: inputs on which the reference itself is non-finite, e.g. dist = 0 next to an overflowing density (0 * inf): there
volrender_bwd_kernel deliberately returns zero where torch propagates NaN (its comment on the line that sets `dead`).  No case for it."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

import weights as W
from oracle import pose_path as O

VIEWS = ("same", "turned", "skewed", "away", "inside", "far")
NERF_KEYS = ("plane_coefs.0.weight", "plane_coefs.0.bias", "plane_coefs.2.weight", "plane_coefs.2.bias", "nviews.weight", "nviews.bias",
             "decoder.weight")
BF16_WEIGHTS = ("plane_coefs.0.weight", "plane_coefs.2.weight")  # what FusedNerfWeights keeps in bf16: bf16 values on both sides
RENDER_SHAPES = [(64, 16, 24, 2, False), (128, 12, 5, 1, True), (64, 8, 6, 1, False)]  # C, r, S, b, stratified jitter
BWD_SHAPES = RENDER_SHAPES[:2]
FAR = 2.0
DEPTH_ROW = torch.tensor([0.0, -0.5, 1e-20, 0.3, 0.9, 1.7, 2.0, 1e6], dtype=torch.float32)
CAM_SEED = 3
CLASSES = ("allmask0", "partial", "behind", "rest", "mask0")


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def shape_id(s) -> str:
    C, r, S, b, jit = s
    return f"C{C}-r{r}-S{S}-b{b}" + ("-jitter" if jit else "")


# ------------------------------------------------------------------------------------------------ cameras
def _rot(axis: str, a: float) -> torch.Tensor:
    c, s = math.cos(a), math.sin(a)
    return torch.tensor({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
                         "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def cameras(b: int) -> torch.Tensor:
    """[b, 7, 16] fp32: element 0 the hostile set (target + VIEWS), element 1 a plain ring."""
    from cd360 import synth
    from cd360.cameras import pack_cameras
    ring = pack_cameras(synth.pose_batch(2, 6, seed=CAM_SEED))
    tgt = ring[0, 0].double()
    R, T, f, c = tgt[:9].reshape(3, 3), tgt[9:12], tgt[12:14], tgt[14:16]

    def row(R_=R, T_=T, f_=f, c_=c):
        return torch.cat([R_.reshape(9), T_, f_, c_]).float()

    d = torch.float64
    views = {"same": row(), "turned": row(R @ _rot("y", math.pi), -T),
             "skewed": row(f_=torch.tensor([0.7, 3.1], dtype=d), c_=torch.tensor([0.35, -0.2], dtype=d)),
             "away": row(R @ _rot("x", 1.2)), "inside": row(T_=T + torch.tensor([0.0, 0.0, -1.0], dtype=d)),
             "far": row(R @ _rot("z", 0.5), 40.0 * T)}
    hostile = torch.stack([row()] + [views[v] for v in VIEWS])
    return torch.stack([hostile, ring[1]][:b]).contiguous()


def jitter(r: int, S: int):
    """(xy jitter (jx, jy), depth jitter [hw, S + 1]) of the stratified training mode."""
    return (W.uniform("jx", (r + 1,), seed=r), W.uniform("jy", (r + 1,), seed=r)), W.uniform("jd", (r * r, S + 1), seed=r)


def geometry(cams: torch.Tensor, r: int, t: torch.Tensor, xy=None):
    """The oracle's coordinate chain in the dtype of `cams` (xs / ys / t keep their fp32 VALUES): dict(rays, points, grid, x0, y0, mask,
    q [b, n, hw, S, 3] view-space points of the reference views).  t: [S] or [hw, S]."""
    xs, ys = O.patch_positions(r, None if xy is None else xy[0]), O.patch_positions(r, None if xy is None else xy[1])
    rays = O.patch_rays(cams, xs, ys)
    lengths = (t[None, None] if t.dim() == 1 else t[None]).to(cams.dtype)
    pts = O.ray_points(rays, lengths)
    grid = O.sample_grid(cams, pts)
    x0, y0, _, _, mask = O.bilinear_corners(grid, r)
    q = O.world_to_view(cams[:, 1:, None, None, :], pts[:, None])
    return dict(xs=xs, ys=ys, rays=rays, points=pts, grid=grid, x0=x0, y0=y0, mask=mask, q=q)


# ------------------------------------------------------------------------------------------------ fused render cases
@dataclass
class RenderCase:
    name: str
    C: int
    r: int
    S: int
    b: int
    cams: torch.Tensor            # [b, 7, 16] fp32
    xref: torch.Tensor            # [b, 6, r * r, C] fp32 holding bf16 values
    w: dict                       # FeatureNeRFEncoding parameters, fp32
    xy: Optional[Tuple[torch.Tensor, torch.Tensor]]
    dj: Optional[torch.Tensor]
    gf: torch.Tensor              # cotangents of (features, sigma_raw, rgb_raw)
    gs: torch.Tensor
    gr: torch.Tensor


@functools.lru_cache(maxsize=None)
def render_case(C: int, r: int, S: int, b: int, jit: bool) -> RenderCase:
    shapes = {"model.plane_coefs.0.weight": (C, C + 198), "model.plane_coefs.0.bias": (C,), "model.plane_coefs.2.weight": (C, C),
              "model.plane_coefs.2.bias": (C,), "model.nviews.weight": (1, C + 198), "model.nviews.bias": (1,), "model.decoder.weight": (4, C)}
    w = {k[len("model."):]: v for k, v in W.synth_state_dict(shapes, C + r).items()}
    for k in BF16_WEIGHTS:
        w[k] = bf(w[k])
    xy, dj = jitter(r, S) if jit else (None, None)
    n = len(VIEWS)
    g = torch.Generator().manual_seed(C + r)
    gf, gs, gr = bf(torch.randn(b, r * r, S, C, generator=g)), torch.randn(b, r * r, S, 1, generator=g), torch.randn(b, r * r, S, 3, generator=g)
    return RenderCase(shape_id((C, r, S, b, jit)), C, r, S, b, cameras(b), bf(W.tensor("xref", (b, n, r * r, C), seed=C + r)), w, xy, dj, gf, gs, gr)


@dataclass
class RenderRef:
    feats: torch.Tensor           # [b, hw, S, C]
    sigma: torch.Tensor           # [b, hw, S, 1]
    rgb: torch.Tensor             # [b, hw, S, 3]
    attn: torch.Tensor            # [b, n, hw, S, 1]
    grid: torch.Tensor            # [b, n, hw, S, 2]
    mask: torch.Tensor            # [b, n, hw, S] int32
    q: torch.Tensor               # [b, n, hw, S, 3]
    grads: Optional[tuple] = None  # d / d NERF_KEYS of <feats, gf> + <sigma, gs> + <rgb, gr>


_REFS = {}


def render_reference(case: RenderCase, dtype=torch.float64, grads: bool = False) -> RenderRef:
    """O.nerf_module in `dtype` on the case's values (float64: the reference; float32: the oracle, whose distance from the reference
    tests/test_render_cases_cpu.py holds to a tenth of every bar).  Computed once and shared; never modified."""
    key = (case.name, dtype, grads)
    if key in _REFS:
        return _REFS[key]
    w = {k: v.to(dtype).requires_grad_(grads) for k, v in case.w.items()}
    cams = case.cams.to(dtype)
    with torch.set_grad_enabled(grads):
        feats, sigma, _, attn, rgb, dbg = O.nerf_module(w, cams, case.xref.to(dtype), case.S, FAR, xy_jitter=case.xy, depth_jitter=case.dj)
        gr = None
        if grads:
            gr = torch.autograd.grad([feats, sigma, rgb], [w[k] for k in NERF_KEYS], [case.gf.to(dtype), case.gs.to(dtype), case.gr.to(dtype)])
    with torch.no_grad():
        grid = dbg["grid"].detach()
        mask = O.bilinear_corners(grid, case.r)[4]
        q = O.world_to_view(cams[:, 1:, None, None, :], dbg["points"][:, None])
    ref = RenderRef(feats.detach(), sigma.detach(), rgb.detach(), attn.detach(), grid, mask, q, gr)
    _REFS[key] = ref
    return ref


def sample_classes(ref: RenderRef) -> dict:
    """name -> bool [b, hw, S] (module docstring); view_classes: name -> bool [b, n, hw, S]."""
    m0, part, behind = ref.mask == 0, (ref.mask != 0) & (ref.mask != 15), ref.q[..., 2] < 0
    out = {"allmask0": m0.all(1), "partial": part.any(1), "behind": behind.any(1), "mask0": m0.any(1)}
    out["rest"] = ~(out["allmask0"] | out["partial"] | out["behind"] | out["mask0"])
    return out


def view_classes(ref: RenderRef) -> dict:
    m0, part, behind = ref.mask == 0, (ref.mask != 0) & (ref.mask != 15), ref.q[..., 2] < 0
    return {"mask0": m0, "partial": part, "behind": behind, "rest": ~(m0 | part | behind)}


def class_errors(got: torch.Tensor, want: torch.Tensor, classes: dict, lead: int) -> dict:
    """{'tensor': max |err| / max |want|, class: max |err| over the class / the class's own max |want| (None: empty class)}.  The class
    masks cover the first `lead` dimensions of the tensors.  A non-finite error counts as inf."""
    err = (got.double() - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    out = {"tensor": err.max().item() / want.abs().max().item()}
    e2, w2 = err.reshape(*err.shape[:lead], -1), want.abs().reshape(*want.shape[:lead], -1)
    for name, m in classes.items():
        out[name] = e2[m].max().item() / w2[m].max().item() if bool(m.any()) else None
    return out


def fmt(errs: dict) -> str:
    return " ".join(f"{k}={'-' if v is None else format(v, '.2e')}" for k, v in errs.items())


# ------------------------------------------------------------------------------------------------ texel-centre grids
@functools.lru_cache(maxsize=None)
def texel_case(r: int, C: int = 96, n_img: int = 3):
    """(xref [n_img, r * r, C] bf16 values, grid [n_img, P, 2], kinds): kinds = dict(centre = (slice of P, texel index of each point),
    ring = slice of the points one texel outside (r = 17 only, may be empty), edge = slice of the +-1 / +-1.2 points)."""
    g = torch.Generator().manual_seed(r)
    xref = bf(torch.randn(n_img, r * r, C, generator=g))
    c = -1.0 + 2.0 * torch.arange(r, dtype=torch.float32) / (r - 1)
    assert torch.equal(((c + 1) / 2) * (r - 1), torch.arange(r, dtype=torch.float32))
    yy, xx = torch.meshgrid(c, c, indexing="ij")
    centre = torch.stack([xx.reshape(-1), yy.reshape(-1)], -1)  # point y * r + x sits on texel y * r + x
    ring = torch.zeros(0, 2)
    if r == 17:
        o = torch.cat([torch.tensor([-1.125]), c, torch.tensor([1.125])])
        yo, xo = torch.meshgrid(o, o, indexing="ij")
        allp = torch.stack([xo.reshape(-1), yo.reshape(-1)], -1)
        ring = allp[(allp.abs() == 1.125).any(-1)]
    ev = torch.tensor([-1.2, -1.0, 0.0, 0.3, 1.0, 1.2])
    ye, xe = torch.meshgrid(ev, ev, indexing="ij")
    edge = torch.stack([xe.reshape(-1), ye.reshape(-1)], -1)
    grid = torch.cat([centre, ring, edge])[None].expand(n_img, -1, -1).contiguous()
    nc, nr = centre.shape[0], ring.shape[0]
    kinds = dict(centre=slice(0, nc), ring=slice(nc, nc + nr), edge=slice(nc + nr, grid.shape[1]))
    return xref, grid, kinds


# ------------------------------------------------------------------------------------------------ volume rendering
FAMILIES = ("plain", "vanishing", "thick", "opaque-first", "overflow-mid", "wall-last", "underflow")
RAYS = 32
VOL_B, VOL_HW = 2, len(FAMILIES) * RAYS // 2
VOL_S = (1, 5, 24, 64)
D_SIGMA_BAR = {False: 2e-4, True: 1e-2}  # by bf16: the bars of tests/test_backward_gpu.py test_volrender_backward
# (S, bf16, per_ray dists, raw inputs): every S with both dtypes; dists layout and activation alternate so that each S meets both of each
VOL_CASES = [(S, bf16, (i + j) % 2 == 0, raw) for i, S in enumerate(VOL_S) for j, bf16 in enumerate((False, True)) for raw in (True, False)]


def vol_id(v) -> str:
    S, bf16, per_ray, raw = v
    return f"S{S}-{'bf16' if bf16 else 'fp32'}-{'rays' if per_ray else 'shared'}-{'raw' if raw else 'activated'}"


@dataclass
class VolCase:
    name: str
    S: int
    C: int
    bf16: bool
    per_ray: bool
    raw: bool
    family: torch.Tensor          # [b, hw] int64 index into FAMILIES
    feats: torch.Tensor           # [b, hw, S, C] fp32 (bf16 values when bf16)
    sigma_raw: torch.Tensor       # [b, hw, S] fp32
    rgb_raw: torch.Tensor         # [b, hw, S, 3] fp32
    sigma_in: torch.Tensor        # what the kernel is handed: sigma_raw, or fp32 exp of it (raw = False)
    rgb_in: torch.Tensor
    dists: torch.Tensor           # [hw, S] or [S]
    g: tuple                      # cotangents of (rendered [b, hw, C], fg [b, hw, 1], alphas [b, hw, S, 1], rgb [b, hw, 3])

    def rays(self, fam: str) -> torch.Tensor:
        return self.family == FAMILIES.index(fam)

    def dists4(self, dtype) -> torch.Tensor:
        d = self.dists if self.per_ray else self.dists[None].expand(VOL_HW, self.S)
        return d[None, :, :, None].to(dtype)


@functools.lru_cache(maxsize=None)
def vol_case(S: int, bf16: bool, per_ray: bool, raw: bool) -> VolCase:
    name = vol_id((S, bf16, per_ray, raw))
    b, hw, C = VOL_B, VOL_HW, 64 if bf16 else 8
    g = torch.Generator().manual_seed(1000 * S + 2 * bf16 + per_ray)
    family = (torch.arange(b * hw) % len(FAMILIES)).reshape(b, hw)
    feats = torch.randn(b, hw, S, C, generator=g)
    z = torch.randn(b, hw, S, generator=g)
    sig = z * 2
    for i, fam in enumerate(FAMILIES):
        m = family == i
        if fam == "vanishing":
            sig[m] = z[m] - 14
        elif fam == "thick":
            sig[m] = z[m] + 3
        elif fam == "opaque-first":
            sig[m] = torch.cat([torch.full((int(m.sum()), 1), 12.0), sig[m][:, 1:]], 1)
        elif fam == "overflow-mid":
            row = sig[m]
            row[:, S // 2] = 95.0
            sig[m] = row
        elif fam == "wall-last":
            sig[m] = torch.cat([torch.full((int(m.sum()), S - 1), -20.0), torch.full((int(m.sum()), 1), 30.0)], 1)
        elif fam == "underflow":
            sig[m] = -95.0
    rgb_raw = torch.randn(b, hw, S, 3, generator=g)
    dists = (torch.rand(hw, S, generator=g) if per_ray else torch.rand(S, generator=g)) * 0.1 + 0.04
    gs = (torch.randn(b, hw, C, generator=g), torch.randn(b, hw, 1, generator=g), torch.randn(b, hw, S, 1, generator=g), torch.randn(b, hw, 3, generator=g))
    if bf16:
        feats, gs = bf(feats), (bf(gs[0]),) + gs[1:]
    sigma_in, rgb_in = (sig, rgb_raw) if raw else (torch.exp(sig), torch.sigmoid(rgb_raw))
    return VolCase(name, S, C, bf16, per_ray, raw, family, feats, sig, rgb_raw, sigma_in, rgb_in, dists, gs)


@dataclass
class VolRef:
    rendered: torch.Tensor
    fg: torch.Tensor
    alphas: torch.Tensor
    weights: torch.Tensor         # [b, hw, S, 1]
    rgb: torch.Tensor
    cum: torch.Tensor             # [b, hw, S, 1] optical depth ahead of the sample
    col: torch.Tensor             # [b, hw, S, 3] the colours that are weighted
    grads: Optional[tuple] = None  # (d_feats, d_sigma_in, d_rgb_in)


_VREFS = {}


def vol_reference(case: VolCase, dtype=torch.float64, grads: bool = False) -> VolRef:
    """O.trunc_exp + O.vol_render in `dtype` on the values the kernel is handed, and autograd gradients for the case's cotangents."""
    key = (case.name, dtype, grads)
    if key in _VREFS:
        return _VREFS[key]
    f, s, c = (t.to(dtype).requires_grad_(grads) for t in (case.feats, case.sigma_in, case.rgb_in))
    with torch.set_grad_enabled(grads):
        dens = O.trunc_exp(s) if case.raw else s
        col = torch.sigmoid(c) if case.raw else c
        d4 = case.dists4(dtype)
        rendered, fg, alphas, weights, rgb = O.vol_render(f, dens[..., None], d4, col)
        gr = None
        if grads:
            gr = torch.autograd.grad([rendered, fg, alphas, rgb], (f, s, c), [t.to(dtype) for t in case.g])
    with torch.no_grad():
        dd = d4 * dens.detach()[..., None]
        cum = torch.cumsum(torch.cat([torch.zeros_like(dd[..., :1, :]), dd[..., :-1, :]], -2), -2)  # (not inclusive - dd: inf - inf)
    ref = VolRef(rendered.detach(), fg.detach(), alphas.detach(), weights.detach(), rgb.detach(), cum, col.detach(), gr)
    _VREFS[key] = ref
    return ref


def weight_bar(ref: VolRef) -> torch.Tensor:
    """bw of the module docstring, [b, hw, S, 1] float64 (where w64 is 0 the second term is 0, whatever cum64)."""
    w = ref.weights
    return 2.0 ** -22 + torch.where(w > 0, 2.0 ** -18 * ref.cum.clamp(min=1.0) * w, torch.zeros_like(w))


def output_bar(ref: VolRef, x: torch.Tensor, want: torch.Tensor, bf16: bool = False) -> torch.Tensor:
    """Bar of sum_s w_s x_s for x [b, hw, S, K] float64."""
    bar = (weight_bar(ref) * x.abs()).sum(-2) + 2.0 ** -22 * (ref.weights * x).abs().sum(-2)
    return bar + (2.0 ** -8 * want.abs() if bf16 else 0.0)


def worst(err: torch.Tensor, bar: torch.Tensor) -> float:
    """max err / bar; a non-finite error counts as inf."""
    q = err / bar
    return torch.where(torch.isfinite(err), q, torch.full_like(q, float("inf"))).max().item()


def per_family(case: VolCase, err: torch.Tensor, bar: torch.Tensor) -> dict:
    """family -> worst err / bar over that family's rays (err, bar: [b, hw, ...])."""
    return {fam: worst(err[case.rays(fam)], bar[case.rays(fam)]) for fam in FAMILIES}


def per_ray_rel(got: torch.Tensor, want: torch.Tensor):
    """d_sigma_raw [b, hw, S]: (error over a ray / that ray's own max |want| [b, hw], rays whose float64 gradient is not all zero)."""
    err = (got.double() - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    scale = want.abs().amax(-1)
    live = scale > 0
    return err.amax(-1) / scale.clamp(min=1e-300), live
