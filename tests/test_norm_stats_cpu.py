"""The yardstick of tests/test_norm_stats_gpu.py, checked without a GPU: torch's own fp32 normalisations sit inside the bound of
tests/norm_ref.py with the margin K was chosen for, the input builders deliver the conditioning they are asked for, and a one-pass
E[x^2] - mean^2 GroupNorm in fp32 leaves the bound where its cancellation sets in (so the bound can fire)."""
import pytest
import torch

import norm_ref as R


def _worst(got, ref, unit):
    return float(R.excess(got, ref, unit, store=0.0).max())


def _fp32_ratios():
    out = {}
    for (N, P, C, G), ratio in R.CASES_GN:
        x, gamma, beta, _ = R.gn_case(N, P, C, G, ratio)
        dy = R.group_scaled_noise(N, P, C, G)
        for eps in R.EPS:
            for silu in (False, True):
                out["gn", N, P, C, G, ratio, eps, silu] = _worst(R.gn_forward(x, gamma, beta, G, eps, silu, torch.float32), *R.gn_unit(x, gamma, beta, G, eps, silu))
        if (N, P, C, G) in R.GN_BWD_SHAPES and ratio in (0, 16, 64, 128):
            for silu in (False, True):
                out["gn_bwd", N, P, C, G, ratio, silu] = _worst(R.gn_backward(x, dy, gamma, beta, G, 1e-5, silu, torch.float32),
                                                                *R.gn_backward_unit(x, dy, gamma, beta, G, 1e-5, silu))
    for (rows, C), ratio in R.CASES_LN:
        a, b, gamma, beta, _ = R.ln_case(rows, C, ratio)
        for bb in (None, b):
            out["ln", rows, C, ratio, bb is not None] = _worst(R.ln_forward(a, bb, gamma, beta, 1e-5, torch.float32), *R.ln_unit(a, bb, gamma, beta, 1e-5))
        out["ln_bwd", rows, C, ratio] = _worst(R.ln_backward(a, gamma, b, None, 1e-5, torch.float32), *R.ln_backward_unit(a, gamma, b, None, 1e-5))
    for (M, N, K), ratio in R.CASES_FOLD:
        x, (w, b, gamma, beta), _ = R.fold_case(M, N, K, ratio)
        wp, _, cb = R.pack_ln_linear_cpu(w, b, gamma, beta)
        out["fold", M, N, K, ratio] = _worst(R.ln_linear(x, wp, cb, 1e-5, torch.float32), *R.ln_linear_unit(x, wp, cb, 1e-5))
    return out


def test_fp32_torch_reference_sits_inside_the_bound():
    """K = 8 x the worst fp32-torch error in units of 2^-24 unit: the fp32 reference must stay within K / 8 on every case, and the
    constant written in norm_ref.py must be the figure measured here (to the rounding it is written with)."""
    ratios = _fp32_ratios()
    worst_key = max(ratios, key=ratios.get)
    worst = ratios[worst_key]
    by_kind = {}
    for k, v in ratios.items():
        by_kind[k[0]] = max(by_kind.get(k[0], 0.0), v)
    print(f"fp32 torch against fp64, in units of 2^-24 unit: worst {worst:.3f} at {worst_key}; by kind {by_kind}; K_MEASURED = {R.K_MEASURED}, K = {R.K}")
    assert worst <= R.K / 8, (worst_key, worst)
    assert worst <= R.K_MEASURED <= 1.5 * worst + 0.5 and R.K == pytest.approx(8 * R.K_MEASURED), (worst, R.K_MEASURED, R.K)


def test_builders_deliver_the_requested_conditioning():
    for (N, P, C, G), ratio in R.CASES_GN:
        x, realised = R.offset_groups(N, P, C, G, ratio)
        assert x.dtype == torch.bfloat16 and realised.shape == (N, G)
        if ratio:
            assert (realised >= 0.7 * ratio).all() and (realised <= 1.3 * 1.25 * ratio).all(), (N, P, C, G, ratio, realised.min(), realised.max())
        else:
            assert (realised < 0.5).all()
    for (rows, C), ratio in R.CASES_LN:
        x, realised = R.offset_rows(rows, C, ratio)
        if ratio:
            assert (realised >= 0.7 * ratio).all() and (realised <= 1.3 * 1.25 * ratio).all(), (rows, C, ratio, realised.min(), realised.max())
        else:
            assert (realised < 0.5).all()
    for v in R.CONSTANTS:
        assert float(R.bfr(torch.tensor(v, dtype=torch.float64))) == v
        x, mask = R.constant_groups(2, 100, 320, 32, v)
        xg = x.double().view(2, 100, 32, 10)
        assert mask.any() and not mask.all()
        assert (xg.permute(0, 2, 1, 3)[mask] == v).all() and (xg.permute(0, 2, 1, 3)[~mask].std(-1) > 0).all()
        rr = R.group_ratio(x, 32)
        assert (rr[mask] == (float("inf") if v else 0.0)).all()
        xr, mr = R.constant_rows(37, 64, v)
        assert (xr.double()[mr] == v).all() and (xr.double()[~mr].std(-1) > 0).all()
    x, scale = R.wide_range(2, 256, 320, 32)
    s = x.double().view(2, 256, 32, 10).std((1, 3))
    assert float(scale.max() / scale.min()) == 2.0 ** 12 and ((s / scale).log2().abs() < 0.5).all()
    assert ((R.group_ratio(x, 32) > 5.6) & (R.group_ratio(x, 32) < 13)).all()


def test_one_pass_variance_in_fp32_leaves_the_bound():
    """The emulated E[x^2] - mean^2 GroupNorm: inside the bound at ratio 0, outside at ratio 128 (before AND after a bf16 store), so a
    kernel with that defect cannot pass the GPU file."""
    N, P, C, G = 2, 100, 320, 32
    for ratio, fails in ((0, False), (128, True)):
        x, gamma, beta, _ = R.gn_case(N, P, C, G, ratio)
        ref, unit = R.gn_unit(x, gamma, beta, G, 1e-5, False)
        y = R.onepass_group_norm_fp32(x, gamma, beta, G, 1e-5)
        w32 = float(R.excess(y, ref, unit, store=0.0).max())
        w16 = float(R.excess(R.bfr(y), ref, unit).max())
        print(f"one-pass fp32 GroupNorm at ratio {ratio}: {w32:.1f} (fp32 output) / {w16:.1f} (bf16 store) x 2^-24 unit, K = {R.K}")
        assert (w32 > R.K and w16 > R.K) == fails and (w32 <= R.K and w16 <= R.K) == (not fails), (ratio, w32, w16)
