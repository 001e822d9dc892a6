"""The backward render kernels on the cases of tests/render_cases.py: cd360_volrender_bwd on the density families (all four incoming
gradients: rendered, fg, alphas, rgb) and the fused FeatureNeRF backward on the hostile cameras, against float64 autograd through
O.trunc_exp + O.vol_render and through O.nerf_module.  Needs an MI355X.

Bars (tests/test_render_cases_cpu.py holds fp32 autograd inside each against the same reference):
  d_feats      per element bw_s |g| (+ 2^-8 |want| in bf16), bw the per-weight bar of render_cases; on `opaque-first`
               d_feats[..., 0, :] == d_rendered exactly and zero for the other samples;
  d_rgb_raw    per element bw_s |g sigmoid'(rgb_raw)| + 2^-20 |want|;
  d_sigma_raw  the bars of test_volrender_backward (2e-4 fp32, 1e-2 bf16) PER RAY for S >= 5: error over a ray divided by that ray's own
               max |want| (rays whose float64 gradient is exactly zero are skipped: none for S >= 5); S = 1: tensor-wide (a ray has one
               value and the two terms of d(dd) cancel).  fp32 autograd sits at <= 1.1e-6 per ray, 1.6e-7 tensor-wide at S = 1, so no
               case carries a bar of its own;
  fused        gradients of (features, rgb_raw, sigma_raw) with respect to the seven FeatureNeRFEncoding parameters through
               fused_feature_nerf(live=True), on the training route and on the precomputed-tables route (atomic dY / dlv scatter): the 3e-2 bars of test_fused_feature_nerf_backward, nviews.bias (mathematically zero) against
               the scale of nviews.weight's gradient; two backward passes within 1e-5 of each gradient's maximum (the dlv scatter uses
               atomics: bit-identity is not asked); on the tables route plane_coefs.0.weight within 2^-7: its dY is rounded to bf16
               after the atomic sums, and a last-bit flip of a dY element is one bf16 ulp.
Each test prints its figures (RENDER-EDGE ...) before it asserts.

Measured on an MI355X (worst over the 16 volume-render cases; err / bar where the bar is per element):
  d_feats      0.17 fp32, 0.99 bf16 (the output's own rounding); `opaque-first` exact          d_rgb_raw  0.41 (wall-last; plain 0.24)
  d_sigma_raw  per ray: plain 2.3e-6, vanishing 9.2e-7, thick 1.4e-6, opaque-first 1.8e-7, overflow-mid 9.2e-7, wall-last 3.0e-7,
               underflow 9.7e-7; tensor-wide 1.9e-7 (S = 1: 1.2e-7); no ray skipped for S >= 5; everything finite
  fused        both routes: parameter gradients 4.3e-3 at most, nviews.bias 5.2e-8 of nviews.weight's scale; forward features 4.8e-3 in
               every class.  Two passes: training route bit-identical; tables route plane_coefs.0.weight 4.4e-4 (2.2e-4 in another
               run), nviews.weight 9.8e-8, the rest identical.
No kernel bug found.  The scratch mutation of nerf_geom_kernel (tests/test_render_edges_gpu.py) moves these gradients by up to 2.1e-1.
"""
import pytest
import torch

import render_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.mark.parametrize("v", RC.VOL_CASES, ids=RC.vol_id)
def test_volrender_backward_families(v):
    from cd360 import ops
    case = RC.vol_case(*v)
    ref = RC.vol_reference(case, grads=True)
    dtype = BF if case.bf16 else torch.float32
    g_r, g_fg, g_al, g_rgb = case.g
    d_feats, d_sigma, d_rgb = ops.volrender_bwd(case.feats.to(DEV, dtype), case.sigma_in.to(DEV), case.dists.to(DEV), case.rgb_in.to(DEV),
                                                g_r.to(DEV, dtype), g_fg.to(DEV), g_al.to(DEV), None, g_rgb.to(DEV), sigma_is_raw=case.raw,
                                                rgb_is_raw=case.raw)
    d_feats, d_sigma, d_rgb = d_feats.float().cpu().double(), d_sigma.cpu().double(), d_rgb.cpu().double()
    want_f, want_s, want_c = ref.grads
    finite = all(bool(torch.isfinite(t).all()) for t in (d_feats, d_sigma, d_rgb))
    bw = RC.weight_bar(ref)
    dcol = ref.col * (1 - ref.col) if case.raw else torch.ones_like(ref.col)
    bar_f = bw * g_r.double()[:, :, None, :].abs() + (2.0 ** -8 * want_f.abs() if case.bf16 else 0.0)
    bar_c = bw * (g_rgb.double()[:, :, None, :] * dcol).abs() + 2.0 ** -20 * want_c.abs()
    fig_f = RC.per_family(case, (d_feats - want_f).abs(), bar_f.clamp(min=1e-300))
    fig_c = RC.per_family(case, (d_rgb - want_c).abs(), bar_c)
    of = case.rays("opaque-first")
    exact = torch.equal(d_feats[of][:, 0], g_r[of].double()) and bool((d_feats[of][:, 1:] == 0).all())
    bar_s = RC.D_SIGMA_BAR[case.bf16]
    tensor = (d_sigma - want_s).abs().max().item() / want_s.abs().max().item()
    rel, live = RC.per_ray_rel(d_sigma, want_s)
    fig_s = {fam: (rel[case.rays(fam) & live].max().item() if bool((case.rays(fam) & live).any()) else None) for fam in RC.FAMILIES}
    print(f"RENDER-EDGE volrender-bwd {case.name} d_feats err/bar " + " ".join(f"{k}={x:.2f}" for k, x in fig_f.items()))
    print(f"RENDER-EDGE volrender-bwd {case.name} d_rgb_raw err/bar " + " ".join(f"{k}={x:.2f}" for k, x in fig_c.items()))
    print(f"RENDER-EDGE volrender-bwd {case.name} d_sigma_raw tensor={tensor:.2e} per-ray " +
          " ".join(f"{k}={'-' if x is None else format(x, '.2e')}" for k, x in fig_s.items()) +
          f" (bar {bar_s:g}) skipped-rays={int((~live).sum())} finite={finite} opaque-first-exact={exact}")
    assert finite
    assert exact
    assert all(x <= 1.0 for x in fig_f.values()), fig_f
    assert all(x <= 1.0 for x in fig_c.values()), fig_c
    assert tensor < bar_s
    if case.S >= 5:
        assert all(x is not None and x < bar_s for x in fig_s.values()), fig_s


@pytest.mark.parametrize("route", ["gemm", "tables"])
@pytest.mark.parametrize("sh", RC.BWD_SHAPES, ids=RC.shape_id)
def test_fused_backward_on_hostile_cameras(sh, route):
    """route: `gemm` = grad.NerfRenderFn (the training path: weight gradients as GEMMs against gathered reference features, no scatter);
    `tables` = grad.NerfAggregateFn on precomputed tables: the backward kernel scatters into dY / dlv with fp32 atomics -- the route on
    which a fully masked view (mask 0) must add nothing to any table row."""
    from cd360 import nerf
    case = RC.render_case(*sh)
    ref = RC.render_reference(case, grads=True)
    cams, xref = case.cams.to(DEV), case.xref.to(DEV, BF)
    dj = None if case.dj is None else case.dj.to(DEV)
    gf, gdec = case.gf.to(DEV, BF), torch.cat([case.gr, case.gs], -1).to(DEV)

    def run():
        wd = {k: v.to(DEV).requires_grad_(True) for k, v in case.w.items()}
        fw = nerf.FusedNerfWeights(*(wd[k] for k in RC.NERF_KEYS), live=True)
        if route == "gemm":
            h, dec, _, _ = nerf.fused_feature_nerf(fw, cams, xref, case.S, RC.FAR, xy_jitter=case.xy, depth_jitter=dj)
        else:
            h, dec, _, _ = nerf.fused_feature_nerf(fw, cams, None, case.S, RC.FAR, xy_jitter=case.xy, depth_jitter=dj,
                                                   tables=nerf.reference_tables(fw, xref), dims=tuple(case.xref.shape))
        torch.autograd.backward([h, dec], [gf, gdec])
        return h.detach(), [wd[k].grad for k in RC.NERF_KEYS]

    h, grads = run()
    _, again = run()
    fwd = RC.class_errors(h.float().cpu(), ref.feats, RC.sample_classes(ref), 3)
    scale_v = ref.grads[RC.NERF_KEYS.index("nviews.weight")].abs().max().item()
    figs, rep = {}, {}
    for k, g, g2, want in zip(RC.NERF_KEYS, grads, again, ref.grads):
        assert g is not None, k
        g, g2 = g.float().cpu().double(), g2.float().cpu().double()
        e = (g - want).abs().max().item()
        figs[k] = (e if e == e else float("inf")) / (scale_v if k == "nviews.bias" else want.abs().max().item())
        rep[k] = (g - g2).abs().max().item() / max(scale_v if k == "nviews.bias" else want.abs().max().item(), 1e-300)
    print(f"RENDER-EDGE fused-backward {route} {case.name} forward features: {RC.fmt(fwd)} (bar 1e-2)")
    print(f"RENDER-EDGE fused-backward {route} {case.name} gradients (bar 3e-2) " + " ".join(f"{k}={x:.2e}" for k, x in figs.items()))
    print(f"RENDER-EDGE fused-backward {route} {case.name} two passes (bar 1e-5) " + " ".join(f"{k}={x:.2e}" for k, x in rep.items()))
    assert all(torch.isfinite(g).all() for g in grads)
    assert all(x is None or x < 1e-2 for x in fwd.values()), fwd
    assert all(x < 3e-2 for x in figs.values()), figs
    # tables route: dY is summed with fp32 atomics and then rounded to bf16 (grad.NerfAggregateFn), so the order of the additions can flip
    # the last bit of a dY element: one bf16 ulp, 2^-7 relative, is what two passes may differ by in the gradient that is formed from dY
    rep_bar = {k: (2.0 ** -7 if route == "tables" and k == "plane_coefs.0.weight" else 1e-5) for k in RC.NERF_KEYS}
    assert all(rep[k] < rep_bar[k] for k in RC.NERF_KEYS), rep
