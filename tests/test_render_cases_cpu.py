"""The claims of tests/render_cases.py, proved from its float64 reference alone: the shares of the sample classes under the hostile
cameras, that no sample sits on a discontinuity of the projection, the fp32 oracle's distance from the float64 reference (a tenth of
every max-normalised bar of tests/test_render_edges_gpu.py / test_render_edges_bwd_gpu.py, a quarter of the per-element weight bar),
the known answers of the crafted density families, and the exact structure of the texel-centre grids.

Measured (float64 chain; MKL_CBWR=COMPATIBLE as the suite sets it):
  hostile element, r = 16, share of (ray, sample) entries per view   same / turned / skewed / away / inside / far
      mask 0     0 / 0 / .25 / .46 / .59 / 0        partial  0 / 0 / .125 / .06 / .03 / 0
      vz < 0     0 / 1 / 0 / 0 / .54 / 0            |q| > 20 only `far`, all of it, max |q| 37.5
  r = 8: mask 0 nowhere (nor at r = 4), partial .375 / .58 in skewed / away; r = 12: mask 0 beyond all four image borders
  fp32 grid against float64 grid: 6.7e-6 at most (bar 1e-4)
  fp32 oracle against float64, worst of tensor-wide and every sample class, over the three shapes (bars 1e-2 forward, 3e-2 gradients):
      features 3.5e-5, sigma 6.9e-5, rgb 4.9e-5, view weights 2.2e-5, parameter gradients 7.8e-5
  fp32 volume-render oracle, worst err / bar over families and the 16 cases: weights 0.14 (claim 1 / 4); rendered 0.13, fg 0.13,
      rgb 0.13, alphas 0.31 (of 2^-22), d_feats 0.14, d_rgb_raw 0.39 (claim 1 / 2: the sums and gradients add roundings of their own)
  fp32 autograd d_sigma_raw: per ray 1.1e-6 at most for S >= 5 (3.2e-6 at S = 1) -- every family, `vanishing` and `wall-last` included; tensor-wide 1.9e-7
      (S = 1: 1.6e-7).  All below a tenth of the bars (2e-4 fp32, 1e-2 bf16), so no case carries a bar of its own.  At S = 1 the rays
      of `opaque-first`, `overflow-mid` and `wall-last` have a float64 gradient of exactly zero (their one sample is saturated)."""
import pytest
import torch

import render_cases as RC
from oracle import pose_path as O

BAR_FWD, BAR_GRAD = 1e-2, 3e-2


def share(m):
    return m.float().mean().item()


def hostile_geometry(r, S):
    return RC.geometry(RC.cameras(1).double(), r, O.depth_samples(S, RC.FAR)[0][0, 0])


def test_camera_classes_at_r16():
    g = hostile_geometry(16, 24)
    m, q = g["mask"][0], g["q"][0]  # [n, hw, S]
    rows = {"mask0": m == 0, "partial": (m != 0) & (m != 15), "behind": q[..., 2] < 0, "far": q.abs().amax(-1) > 20}
    per_view = {k: [share(v[i]) for i in range(len(RC.VIEWS))] for k, v in rows.items()}
    print("RENDER-CASE r16", {k: [round(x, 3) for x in v] for k, v in per_view.items()}, "max |q|", q.abs().max().item())
    for k, v in per_view.items():
        assert max(v) >= 0.05, (k, v)
    ix = {n: i for i, n in enumerate(RC.VIEWS)}
    assert per_view["behind"][ix["turned"]] == 1.0 and 0.3 < per_view["behind"][ix["inside"]] < 0.7  # vz changes sign along the rays
    assert min(per_view["mask0"][ix[v]] for v in ("skewed", "away", "inside")) >= 0.05 and per_view["partial"][ix["skewed"]] >= 0.05
    assert per_view["far"][ix["far"]] == 1.0 and q.abs().max().item() > 30.0
    assert torch.equal(m[ix["same"]], torch.full_like(m[0], 15))  # `same` sees every sample in its own pixel


def test_mask0_needs_r12():
    for r, S in ((8, 6), (4, 6)):
        assert not bool((hostile_geometry(r, S)["mask"] == 0).any())
    m = hostile_geometry(8, 6)["mask"][0]
    part = [share((m[RC.VIEWS.index(v)] != 0) & (m[RC.VIEWS.index(v)] != 15)) for v in ("skewed", "away")]
    print("RENDER-CASE r8 partial skewed / away", part)
    assert min(part) >= 0.30
    # r = 12: mask 0 is reached, on both sides of the image
    g = hostile_geometry(12, 5)
    m0 = g["mask"][0] == 0
    assert bool((m0 & (g["x0"][0] < 0)).any()) and bool((m0 & (g["x0"][0] >= 11)).any())
    assert bool((m0 & (g["y0"][0] < 0)).any()) and bool((m0 & (g["y0"][0] >= 11)).any())


@pytest.mark.parametrize("sh", RC.RENDER_SHAPES, ids=RC.shape_id)
def test_no_sample_on_a_discontinuity_and_fp32_oracle_within_a_tenth_of_every_bar(sh):
    case = RC.render_case(*sh)
    assert torch.equal(case.xref, RC.bf(case.xref)) and torch.equal(case.gf, RC.bf(case.gf)) and RC.render_case(*sh) is case
    ref, o32 = RC.render_reference(case), RC.render_reference(case, torch.float32)
    gd = (o32.grid.double() - ref.grid).abs().max().item()
    print(f"RENDER-CASE {case.name} fp32 grid - float64 grid {gd:.2e}")
    assert gd < 1e-4
    sc, vc = RC.sample_classes(ref), RC.view_classes(ref)
    if case.r >= 12:
        assert share(sc["mask0"]) >= 0.05 and share(sc["partial"]) >= 0.05 and share(sc["behind"]) >= 0.05
    if case.b == 2:  # the ring element: ordinary samples
        assert share(sc["rest"][1]) > 0.2
    for name, lead, cl in (("feats", 3, sc), ("sigma", 3, sc), ("rgb", 3, sc), ("attn", 3, sc), ("attn", 4, vc)):
        got, want = getattr(o32, name), getattr(ref, name)
        if name == "attn" and lead == 3:
            got, want = got.permute(0, 2, 3, 1, 4), want.permute(0, 2, 3, 1, 4)
        errs = RC.class_errors(got, want, cl, lead)
        print(f"RENDER-CASE {case.name} fp32 oracle {name}/{lead}: {RC.fmt(errs)}")
        assert all(e is None or e < BAR_FWD / 10 for e in errs.values()), (name, errs)


@pytest.mark.parametrize("sh", RC.BWD_SHAPES, ids=RC.shape_id)
def test_fp32_autograd_within_a_tenth_of_the_gradient_bar(sh):
    case = RC.render_case(*sh)
    ref, o32 = RC.render_reference(case, grads=True), RC.render_reference(case, torch.float32, grads=True)
    scale_v = ref.grads[RC.NERF_KEYS.index("nviews.weight")].abs().max().item()
    for k, g, w in zip(RC.NERF_KEYS, o32.grads, ref.grads):
        assert torch.isfinite(w).all()
        e = (g.double() - w).abs().max().item() / (scale_v if k == "nviews.bias" else w.abs().max().item())
        print(f"RENDER-CASE {case.name} fp32 autograd {k}: {e:.2e}")
        assert e < BAR_GRAD / 10, (k, e)


def test_texel_centre_grids_are_exact():
    for r in (9, 17):
        xref, grid, kinds = RC.texel_case(r)
        assert torch.equal(xref, RC.bf(xref))
        x0, y0, tx, ty, mask = O.bilinear_corners(grid, r)
        c = kinds["centre"]
        assert c.stop - c.start == r * r and bool((tx[:, c] == 0).all()) and bool((ty[:, c] == 0).all())
        assert torch.equal((y0[0, c] * r + x0[0, c]).long(), torch.arange(r * r)) and bool((mask[:, c] & 1 == 1).all())
        want = O.gather_bilinear(xref[:, None].double(), grid[:, None, :, None, :].double())[:, 0, :, 0]
        assert torch.equal(want[:, c], xref.double())
        rg = kinds["ring"]
        assert (rg.stop - rg.start) == (4 * 18 if r == 17 else 0)
        assert bool((want[:, rg] == 0).all())
        # every live corner of a ring point has weight zero, or there is none: the kernel's answer is an exact zero, too
        wts = torch.stack([(1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty], -1)[:, rg]
        live = torch.stack([(mask[:, rg] >> i) & 1 for i in range(4)], -1).bool()
        assert bool((wts[live] == 0).all())
        e = kinds["edge"]
        assert e.stop - e.start == 36 and set(grid[0, e].reshape(-1).tolist()) >= set(torch.tensor([-1.2, -1.0, 1.0, 1.2]).tolist())


@pytest.mark.parametrize("v", RC.VOL_CASES, ids=RC.vol_id)
def test_density_families_known_answers_and_fp32_oracle(v):
    case = RC.vol_case(*v)
    S = case.S
    assert RC.vol_case(*v) is case and all(int(case.rays(f).sum()) == RC.RAYS for f in RC.FAMILIES)
    assert 0.04 <= case.dists.min().item() and case.dists.max().item() <= 0.14 and case.dists.dim() == (2 if case.per_ray else 1)
    if case.bf16:
        assert torch.equal(case.feats, RC.bf(case.feats)) and torch.equal(case.g[0], RC.bf(case.g[0]))
    assert bool((case.sigma_raw[case.rays("overflow-mid")][:, S // 2] > 88.73).all())  # fp32 exp overflows
    assert case.raw or bool(torch.isinf(case.sigma_in[case.rays("overflow-mid")][:, S // 2]).all())
    ref, o32 = RC.vol_reference(case, grads=True), RC.vol_reference(case, torch.float32, grads=True)
    for t in (ref.rendered, ref.fg, ref.alphas, ref.weights, ref.rgb) + ref.grads:
        assert torch.isfinite(t).all()  # in scope: the reference itself is finite

    # known answers, in float64
    of, un, wl = case.rays("opaque-first"), case.rays("underflow"), case.rays("wall-last")
    onehot = torch.zeros(RC.RAYS, S, 1, dtype=torch.float64)
    onehot[:, 0] = 1.0
    assert torch.equal(ref.weights[of], onehot) and torch.equal(ref.fg[of], torch.ones(RC.RAYS, 1, dtype=torch.float64))
    assert torch.equal(ref.rendered[of], case.feats[of][:, 0].double())
    assert ref.weights[un].abs().max().item() < 1e-40 and ref.rendered[un].abs().max().item() < 1e-40 and ref.alphas[un].max().item() < 1e-40
    assert (ref.fg[wl] - 1).abs().max().item() < 1e-12
    if S > 1:
        assert ref.weights[wl][:, :-1].max().item() < 1e-8 and ref.weights[wl][:, -1].min().item() > 1 - 1e-7
    assert torch.equal(ref.grads[0][of][:, 0], case.g[0][of].double()) and (S == 1 or bool((ref.grads[0][of][:, 1:] == 0).all()))
    # the tensor-wide scales are set by `plain`, and `vanishing` rays would hide under them
    assert ref.weights[case.rays("plain")].max().item() > 0.5 and ref.weights[case.rays("vanishing")].max().item() < 1e-5
    if case.raw:  # d_sigma_raw carries the factor exp(sigma_raw)
        assert ref.grads[1][case.rays("vanishing")].abs().max().item() < 1e-4 * ref.grads[1][case.rays("plain")].abs().max().item()

    # the fp32 oracle against the error model: a quarter of the per-weight bar, half of every other per-element bar
    bw, g_r = RC.weight_bar(ref), case.g[0].double()
    col64 = ref.col
    dsig = torch.sigmoid(case.rgb_raw.double()) * (1 - torch.sigmoid(case.rgb_raw.double())) if case.raw else torch.ones_like(col64)
    figs = {"weights": RC.worst((o32.weights.double() - ref.weights).abs(), bw),
            "rendered": RC.worst((o32.rendered.double() - ref.rendered).abs(), RC.output_bar(ref, case.feats.double(), ref.rendered)),
            "fg": RC.worst((o32.fg.double() - ref.fg).abs(), RC.output_bar(ref, torch.ones_like(ref.weights), ref.fg)),
            "rgb": RC.worst((o32.rgb.double() - ref.rgb).abs(), RC.output_bar(ref, col64, ref.rgb)),
            "d_feats": RC.worst((o32.grads[0].double() - ref.grads[0]).abs(), bw * g_r[:, :, None, :].abs() + 1e-300),
            "d_rgb_raw": RC.worst((o32.grads[2].double() - ref.grads[2]).abs(),
                                  bw * (case.g[3].double()[:, :, None, :] * dsig).abs() + 2.0 ** -20 * ref.grads[2].abs())}
    alphas = RC.worst((o32.alphas.double() - ref.alphas).abs(), torch.full_like(ref.alphas, 2.0 ** -22))
    rel, live = RC.per_ray_rel(o32.grads[1], ref.grads[1])
    tensor = (o32.grads[1].double() - ref.grads[1]).abs().max().item() / ref.grads[1].abs().max().item()
    ray = rel[live].max().item()
    print(f"RENDER-CASE {case.name} fp32 oracle err/bar " + " ".join(f"{k}={x:.2f}" for k, x in figs.items()) +
          f" alphas={alphas:.2f} d_sigma tensor={tensor:.1e} per-ray={ray:.1e} zero-gradient rays={int((~live).sum())}")
    assert figs["weights"] <= 0.25 and all(x <= 0.5 for x in figs.values()), figs  # the sums and gradients add roundings of their own
    assert alphas <= 0.5
    bar = RC.D_SIGMA_BAR[False]  # the tighter of the two dtypes' bars
    assert tensor < bar / 10
    if S >= 5:
        assert ray < bar / 10 and bool(live.all())
    else:  # S = 1: the saturated families have one sample and no gradient at all
        assert set(f for f in RC.FAMILIES if not bool(live[case.rays(f)].any())) == {"opaque-first", "overflow-mid", "wall-last"}
