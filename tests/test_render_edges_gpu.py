"""The forward render kernels on hostile cameras and saturated densities: the cases of tests/render_cases.py (reference views that see
samples behind them, past the scene, from inside the depth range, through an off-centre anisotropic lens and from 40 radii away; grid
points exactly on texel centres; density families from underflow to fp32 exp overflow) against the float64 oracle on the same values.
Needs an MI355X.

Bars (tests/test_render_cases_cpu.py holds the fp32 oracle inside each against the same reference):
  geometry        points, grid, x0, y0, mask of cd360_patch_rays / cd360_ray_project_index: bit-exact against the fp32 oracle chain;
  feature_gather  texel-centre points return the table row and the ring one texel outside returns zeros, bit for bit; everything else
                  max |got - want| / max |want| < 1e-6 (fp32), 8e-3 (bf16): the bars of tests/test_kernels_gpu.py;
  fused forward   features, sigma, rgb, view weights under cd360_tuning.nerf_kernel = 0, 1, 3, 4: tensor-wide 1e-2, unchanged, and the
                  same 1e-2 on the error over each sample class divided by that class's own max |want| (render_cases.sample_classes;
                  the view weights also by (view, sample) class);
  volume render   per element, the error model of render_cases (bw = 2^-22 + 2^-18 max(1, cum64) w64 per weight; sums
                  sum_s bw_s |x_s| + 2^-22 sum_s |w_s x_s|, + 2^-8 |want| for a bf16 output; alphas 2^-22); `opaque-first` and
                  `underflow` exactly; every output finite in every family.
Each test prints its figures (RENDER-EDGE ...) before it asserts.

Measured on an MI355X (worst over the cases; err / bar where the bar is per element):
  geometry        all eight cases bit-exact (rays, points, grid, x0, y0, mask); the depth row's t = 0 lands on vz = 0 exactly for `same`
                  (x / 0 -> clip to -1.2)
  feature_gather  centres and ring exact; tensor 4.9e-7 (fp32), 1.9e-3 (bf16)
  fused forward   the four variants give the same figures -- tensor-wide / worst class: features 5.8e-3 / 5.8e-3, sigma 7.4e-3 / 7.4e-3
                  (both at (64, 8, 6)), rgb 5.9e-3 / 5.9e-3, view weights 1.2e-5 / 2.2e-5; `mask0` classes at r = 16: features 4.7e-3,
                  sigma 5.5e-3.  Two-pass against one-pass: logits, the two pass-2 geometries and eight launches bit-identical, g within
                  2.7e-3 on < 1e-4 of the entries
  volume render   weights 0.17, alphas 0.32, fg 0.17, rgb 0.17, rendered 0.99 (the bf16 output's own rounding, 2^-8 |want|; fp32: 0.17);
                  by family the worst weights figure is plain 0.15, vanishing 0.17, thick 0.06, overflow-mid 0.12, the others 0;
                  `opaque-first` and `underflow` exact, everything finite

What these cases found: no kernel bug.  A float64 emulation of the design's bf16 roundings (tables Y / zP, the generated encodings and q,
g, h) reproduces the measured feature errors to three digits (4.58e-3, 3.58e-3, 7.39e-3 with fp32-valued weights), so what is left
is the sum of those roundings.  With fp32-VALUED weight matrices, which the library rounds to bf16 on its own, sigma at (64, 8, 6)
measured 1.14e-2 of its maximum, above the 1e-2 bar; the cases therefore carry bf16 values in the two matrices the library keeps in
bf16 (tests/render_cases.py), as the suite's other bf16 parity tests do with their inputs.

That the cases bite (scratch builds, not committed; arithmetic only, every index stays clamped):
  1. nerf_geom_kernel without `if (!((cr.mask >> c) & 1)) w[c] = 0.f;` -- caught by test_fused_forward_by_sample_class under
     nerf_kernel = 3 and 4 at all three shapes (features 2.2e-1 tensor-wide and 2.5e-1 on `mask0` at r = 16, view weights 5.2e-1; 4.6e-2
     at r = 8, where only partial masks exist), by test_two_pass_equals_one_pass_on_hostile_cameras (logits no longer identical, 85 % of g
     differs) and by all four fused backward cases (gradients up to 2.1e-1).  Variants 0 and 1 do not run that kernel and stay green.
  2. volrender_kernel with `cum = cum + dd` moved above w (inclusive transmittance) -- caught by all 16 cases of
     test_volrender_families_per_element: `opaque-first` no longer exact, weights 2.5e5 bars off in every family with weights above 1e-6.
"""
import pytest
import torch

import render_cases as RC
from oracle import pose_path as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ geometry
def check_geometry(label, cams, r, t_host, xs, ys, t_dev, xy):
    from cd360 import ops
    want = RC.geometry(cams, r, t_host, xy)  # the fp32 chain
    cd = cams.to(DEV)
    rays = ops.patch_rays(cd, xs, ys).cpu()
    res = {k: v.cpu() for k, v in ops.ray_project_index(cd, xs, ys, t_dev).items()}
    same = {"rays": torch.equal(rays, want["rays"])}
    for k in ("points", "grid", "x0", "y0", "mask"):
        same[k] = torch.equal(res[k], want[k])
    m = want["mask"]
    print(f"RENDER-EDGE geometry {label} bit-exact={same} mask0={(m == 0).float().mean().item():.3f} "
          f"partial={((m != 0) & (m != 15)).float().mean().item():.3f} behind={(want['q'][..., 2] < 0).float().mean().item():.3f}")
    assert all(torch.isfinite(res[k]).all() for k in ("points", "grid"))
    assert all(same.values()), same
    return want


@pytest.mark.parametrize("r,S,jit", [(16, 24, False), (16, 24, True), (12, 5, True), (12, 5, False), (8, 6, False), (8, 6, True)])
def test_geometry_bit_exact_on_hostile_cameras(r, S, jit):
    from cd360 import nerf
    cams = RC.cameras(2)
    xy, dj = RC.jitter(r, S) if jit else (None, None)
    t_host = O.depth_samples(S, RC.FAR, 0.0, dj, r * r)[0][0]
    t_host = t_host[0] if not jit else t_host
    jx, jy = xy if jit else (None, None)
    xs, ys = nerf.patch_positions(r, DEV, jx), nerf.patch_positions(r, DEV, jy)
    t_dev, _ = nerf.depth_samples(S, RC.FAR, 0.0, DEV, r * r, dj)
    want = check_geometry(f"r{r}-S{S}-jitter{int(jit)}", cams, r, t_host, xs, ys, t_dev, xy)
    assert bool(((want["mask"] != 15) & (want["mask"] != 0)).any()) and (r < 12 or bool((want["mask"] == 0).any()))


@pytest.mark.parametrize("r", [16, 8])
def test_geometry_bit_exact_on_the_explicit_depth_row(r):
    """t = 0, -0.5, 1e-20, 1e6 next to ordinary depths: with `same`, t = 0 puts vz on zero or next to it -- grid_coord's nan_to_num / clip."""
    from cd360 import nerf
    cams = RC.cameras(1)
    xs = nerf.patch_positions(r, DEV)
    want = check_geometry(f"r{r}-depth-row", cams, r, RC.DEPTH_ROW, xs, xs, RC.DEPTH_ROW.to(DEV), None)
    g = want["grid"][0, RC.VIEWS.index("same"), :, 0]  # t = 0
    assert bool((g.abs() == torch.tensor(1.2)).any()) or bool((g == 0).any())  # the clip or the nan_to_num branch was taken


# ------------------------------------------------------------------------------------------------ feature_gather
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("r", [9, 17])
def test_feature_gather_texel_centres(r, dtype):
    from cd360 import ops
    xref, grid, kinds = RC.texel_case(r)
    want = O.gather_bilinear(xref[:, None].double(), grid[:, None, :, None, :].double())[:, 0, :, 0]
    got = ops.feature_gather(xref.to(DEV, dtype), grid.to(DEV)).float().cpu()
    c, rg, e = kinds["centre"], kinds["ring"], kinds["edge"]
    centre_exact, ring_zero = torch.equal(got[:, c], xref), bool((got[:, rg] == 0).all())
    rel = (got.double() - want).abs().max().item() / want.abs().max().item()
    rel_edge = (got[:, e].double() - want[:, e]).abs().max().item() / want.abs().max().item()
    bar = 1e-6 if dtype == torch.float32 else 8e-3
    print(f"RENDER-EDGE feature_gather r{r}-{dtype} centre-exact={centre_exact} ring-zero={ring_zero} ({rg.stop - rg.start} points) "
          f"tensor={rel:.2e}/{bar:g} edge-points={rel_edge:.2e}/{bar:g}")
    assert torch.isfinite(got).all()
    assert centre_exact and ring_zero
    assert rel < bar and rel_edge < bar


# ------------------------------------------------------------------------------------------------ fused forward
def fused_weights(case, live=False):
    from cd360 import nerf
    wd = {k: v.to(DEV).requires_grad_(live) for k, v in case.w.items()}
    return nerf.FusedNerfWeights(*(wd[k] for k in RC.NERF_KEYS), live=live), wd


@pytest.mark.parametrize("variant", [0, 1, 3, 4])
@pytest.mark.parametrize("sh", RC.RENDER_SHAPES, ids=RC.shape_id)
def test_fused_forward_by_sample_class(sh, variant, tune):
    """nerf.fused_feature_nerf under every render kernel variant (0 register gathers, 1 full-line gathers, 3 / 4 two passes on 64 / 32
    channels per workgroup; 2 exists in probe builds only) against float64 O.nerf_module."""
    from cd360 import nerf
    case = RC.render_case(*sh)
    ref = RC.render_reference(case)
    fw, _ = fused_weights(case)
    tune(nerf_kernel=variant)
    with torch.no_grad():
        h, dec, _, vw = nerf.fused_feature_nerf(fw, case.cams.to(DEV), case.xref.to(DEV, BF), case.S, RC.FAR, xy_jitter=case.xy,
                                                depth_jitter=None if case.dj is None else case.dj.to(DEV), want_view_weights=True)
    sc, vc = RC.sample_classes(ref), RC.view_classes(ref)
    outs = {"features": (h.float().cpu(), ref.feats, sc, 3), "sigma": (dec[..., 3:].cpu(), ref.sigma, sc, 3), "rgb": (dec[..., :3].cpu(), ref.rgb, sc, 3),
            "view-weights": (vw.cpu().permute(0, 2, 3, 1, 4), ref.attn.permute(0, 2, 3, 1, 4), sc, 3),
            "view-weights-by-view": (vw.cpu(), ref.attn, vc, 4)}
    errs = {k: RC.class_errors(*v) for k, v in outs.items()}
    for k, e in errs.items():
        print(f"RENDER-EDGE fused-forward nerf_kernel={variant} {case.name} {k}: {RC.fmt(e)} (bar 1e-2)")
    for k, (got, _, _, _) in outs.items():
        assert torch.isfinite(got).all(), k
    for k, e in errs.items():
        assert all(x is None or x < 1e-2 for x in e.values()), (k, e)


@pytest.mark.parametrize("geometry", [3, 4])
@pytest.mark.parametrize("sh", RC.RENDER_SHAPES, ids=RC.shape_id)
def test_two_pass_equals_one_pass_on_hostile_cameras(sh, geometry, tune):
    """The relations of test_render_two_pass_equals_one_pass (tests/test_kernels_gpu.py) on the hostile cameras: view logits of the two-pass
    form bit-identical to the one-pass full-line kernel's, the two pass-2 geometries bit-identical to each other, eight launches
    bit-identical."""
    from cd360 import nerf, ops
    case = RC.render_case(*sh)
    fw, _ = fused_weights(case)
    cams = case.cams.to(DEV)
    xref = case.xref.to(DEV, BF)
    r, S, b, C, n = case.r, case.S, case.b, case.C, len(RC.VIEWS)
    xs = nerf.patch_positions(r, DEV, None if case.xy is None else case.xy[0])
    ys = nerf.patch_positions(r, DEV, None if case.xy is None else case.xy[1])
    t, _ = nerf.depth_samples(S, RC.FAR, 0.0, DEV, r * r, None if case.dj is None else case.dj.to(DEV))
    Y, lv = nerf.reference_tables(fw, xref)
    g = torch.Generator().manual_seed(C)
    zP = RC.bf(torch.randn(b * n, r * r, C, generator=g)).to(DEV, BF)
    cview = nerf.view_constants(fw, cams)
    tune(nerf_kernel=1)
    ref = ops.nerf_mlp_aggregate(cams, xs, ys, t, Y, zP, lv, cview, fw.Wk, want_logits=True)
    tune(nerf_kernel=7 - geometry)
    other = ops.nerf_mlp_aggregate(cams, xs, ys, t, Y, zP, lv, cview, fw.Wk, want_logits=True)
    tune(nerf_kernel=geometry)
    outs = [ops.nerf_mlp_aggregate(cams, xs, ys, t, Y, zP, lv, cview, fw.Wk, want_logits=True) for _ in range(8)]
    geometries = all(torch.equal(a, b_) for a, b_ in zip(other, outs[0]))
    logits = torch.equal(outs[0][1], ref[1])
    repeats = all(torch.equal(a, b_) for o in outs[1:] for a, b_ in zip(o, outs[0]))
    scale = ref[0].float().abs().max().item()
    gdiff = (outs[0][0].float() - ref[0].float()).abs().max().item() / scale
    flips = (outs[0][0] != ref[0]).float().mean().item()
    print(f"RENDER-EDGE two-pass nerf_kernel={geometry} {case.name} logits-identical={logits} geometries-identical={geometries} "
          f"repeats-identical={repeats} g-vs-one-pass={gdiff:.2e}/4e-3 differing={flips:.4f}/0.05")
    assert all(torch.isfinite(x.float()).all() for x in outs[0])
    assert geometries and logits and repeats
    assert torch.allclose(outs[0][2], ref[2], rtol=2e-6, atol=2e-6)
    assert gdiff < 4e-3 and flips < 0.05


# ------------------------------------------------------------------------------------------------ volume rendering
@pytest.mark.parametrize("v", RC.VOL_CASES, ids=RC.vol_id)
def test_volrender_families_per_element(v):
    from cd360 import ops
    case = RC.vol_case(*v)
    ref = RC.vol_reference(case)
    dtype = BF if case.bf16 else torch.float32
    got = ops.volrender(case.feats.to(DEV, dtype), case.sigma_in.to(DEV), case.dists.to(DEV), case.rgb_in.to(DEV), want_weights=True,
                        sigma_is_raw=case.raw, rgb_is_raw=case.raw)
    rendered, fg, alphas, weights, rgb = (t.float().cpu().double() for t in got)
    finite = all(bool(torch.isfinite(t).all()) for t in (rendered, fg, alphas, weights, rgb))
    bars = {"weights": (weights, ref.weights, RC.weight_bar(ref)),
            "alphas": (alphas, ref.alphas, torch.full_like(ref.alphas, 2.0 ** -22)),
            "rendered": (rendered, ref.rendered, RC.output_bar(ref, case.feats.double(), ref.rendered, case.bf16)),
            "fg": (fg, ref.fg, RC.output_bar(ref, torch.ones_like(ref.weights), ref.fg)),
            "rgb": (rgb, ref.rgb, RC.output_bar(ref, ref.col, ref.rgb))}
    figs = {k: RC.per_family(case, (g - w).abs(), bar) for k, (g, w, bar) in bars.items()}
    of, un = case.rays("opaque-first"), case.rays("underflow")
    onehot = torch.zeros_like(ref.weights[of])
    onehot[:, 0] = 1.0
    exact = {"opaque-first": torch.equal(rendered[of], case.feats[of][:, 0].double()) and bool((fg[of] == 1).all()) and torch.equal(weights[of], onehot),
             "underflow": all(bool((t[un] == 0).all()) for t in (rendered, fg, alphas, weights, rgb))}
    for k, f in figs.items():
        print(f"RENDER-EDGE volrender {case.name} {k} err/bar " + " ".join(f"{fam}={x:.2f}" for fam, x in f.items()))
    print(f"RENDER-EDGE volrender {case.name} finite={finite} exact={exact}")
    assert finite
    assert all(exact.values()), exact
    for k, f in figs.items():
        assert all(x <= 1.0 for x in f.values()), (k, f)
