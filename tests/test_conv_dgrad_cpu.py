"""The convolution data gradient on the host: the launches it makes, the route each takes, and the reference side of the GPU tests.

The data gradient of a frozen convolution (cd360.grad.ConvIgemmFn) is cd360_conv_igemm_bf16 launched on dy with swapped, re-padded channel
counts, so it reaches (tiling, halo form, Cout') combinations no forward launch reaches.  This file pins, against the built library,
the table of those launches (tests/conv_shapes.py) and the routes of the small shapes of tests/test_conv_dgrad_gpu.py; and it holds the
reference helpers of tests/conv_dgrad_ref.py, the bound term A and the impulse expectations to ConvIgemmFn.backward's recipe written out
in plain torch -- an fp32 convolution rounded once to bf16 must pass the very bar the kernels are held to, no element excused."""
import pytest
import torch

import conv_dgrad_ref as R
from conv_shapes import (BATCHES, DGRAD_BATCHES, DGRAD_ONLY_ROUTES, DGRAD_SCALES, UNET_1X1, UNET_3X3, UNET_DGRAD, UNET_DGRAD_ROUTES, UNET_DOWNSAMPLE, UNET_OUT_CONV,
                         UNET_UPSAMPLE_3X3, dgrad_channels, dgrad_product_launches)
from test_conv_routes_gpu import FORCED, _fp32_exact, assert_close, bfr

@pytest.fixture
def lib():
    from cd360 import _lib
    return _lib.load()


def route_of(lib, *shape, taps=9, stride=1):
    from cd360.ops import decode_conv_route
    return decode_conv_route(lib.cd360_conv_route(*shape, taps, stride))


def test_the_table_lists_every_differentiated_convolution():
    assert len(UNET_DGRAD) == len(UNET_3X3) + len(UNET_UPSAMPLE_3X3) + len(UNET_DOWNSAMPLE) + 1 + len(UNET_1X1)
    assert dgrad_channels(4, 320) == (320, 64) and dgrad_channels(320, 4) == (64, 320) and dgrad_channels(960, 320) == (320, 960)
    assert dgrad_channels(320, 48) == (64, 320) and dgrad_channels(2560, 1280) == (1280, 2560)
    assert (UNET_OUT_CONV[0], 64, 320, 9) in [e[:4] for e in UNET_DGRAD]
    assert {e[2] for e in UNET_DGRAD if e[3] == 9} == {64, 320, 640, 960, 1280, 1920, 2560}
    for h, ci, co, taps, what in UNET_DGRAD:
        assert ci % 64 == 0 and co % 64 == 0 and taps in (1, 9) and what.startswith("dgrad of"), (h, ci, co, taps, what)


def test_packed_conv_dgrad_pads_as_the_table_says(lib):
    """sgm...util.packed_conv_dgrad on host weights: [Cout', taps Cin'] with dgrad_channels' padding, holding -- read back through the
    documented K order (cd360_conv_k_order) -- the flipped, transposed, zero-padded weight."""
    import torch.nn as nn
    from sgm.modules.diffusionmodules.util import packed_conv_dgrad
    for cin, cout, k in ((4, 320, 3), (320, 4, 3), (192, 48, 3), (960, 64, 3), (128, 320, 1)):
        conv = nn.Conv2d(cin, cout, k, padding=k // 2)
        with torch.no_grad():
            conv.weight.copy_(bfr(torch.randn(conv.weight.shape, generator=torch.Generator().manual_seed(cin + cout))))
        cin_d, cout_d = dgrad_channels(cin, cout)
        wp = packed_conv_dgrad(conv)
        assert wp.shape == (cout_d, k * k * cin_d) and wp.dtype == torch.bfloat16
        g = lib.cd360_conv_k_order(cin_d, k * k)
        got = wp.float().reshape(cout_d, cin_d // (64 * g), k * k, g, 64).permute(0, 1, 3, 4, 2).reshape(cout_d, cin_d, k, k)
        want = torch.zeros(cout_d, cin_d, k, k)
        for ky in range(k):
            for kx in range(k):
                want[:cin, :cout, ky, kx] = conv.weight.detach()[:, :, k - 1 - ky, k - 1 - kx].t()
        assert torch.equal(got, want), (cin, cout, k)


def test_default_routes_of_the_gradient_launches(lib, tune):
    """UNET_DGRAD_ROUTES is the library's answer: every 3 x 3 gradient launch on the LDS-DMA core with the pinned (tiling, halo form,
    slab rows), every 1 x 1 launch on the GEMM entry, at every batch and both latent sizes."""
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    seen = {}
    for n in DGRAD_BATCHES:
        for scale in DGRAD_SCALES:
            for h, ci, co, taps, what in UNET_DGRAD:
                s = h // scale
                r = route_of(lib, n, s, s, ci, co, taps=taps)
                if taps == 1:
                    assert tuple(r) == ("gemm", 0, False, 0), (n, s, ci, co, what, r)
                    continue
                assert tuple(r) == ("dma",) + UNET_DGRAD_ROUTES[n, s][co], (n, s, ci, co, what, r)
                seen.setdefault((n, s), set()).add(co)
    assert {k: set(v) for k, v in UNET_DGRAD_ROUTES.items()} == seen  # (no stale rows in the table)


def test_the_gradient_reaches_routes_no_forward_launch_reaches(lib, tune):
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    forward = set()
    for n in DGRAD_BATCHES:
        for scale in DGRAD_SCALES:
            for h, cin, cout, _ in UNET_3X3:
                r = route_of(lib, n, h // scale, h // scale, cin, cout)
                forward.add((r.tiling, r.halo, cout))
    reached = {(t, halo, co) for d in UNET_DGRAD_ROUTES.values() for co, (t, halo, _) in d.items()}
    assert sorted(reached - forward) == sorted(DGRAD_ONLY_ROUTES)
    assert set(BATCHES) < set(DGRAD_BATCHES)
    # the product-size launch the GPU test runs for each of them is a launch of the table and takes that route
    for (n, s, ci, co, t, halo), want in zip(dgrad_product_launches(), DGRAD_ONLY_ROUTES):
        assert (t, halo, co) == want and any(e[1:4] == (ci, co, 9) and s in (e[0], e[0] // 2) for e in UNET_DGRAD), (n, s, ci, co)
        r = route_of(lib, n, s, s, ci, co)
        assert (r.family, r.tiling, r.halo) == ("dma", t, halo), (n, s, ci, co, r)


def test_default_routes_of_the_small_shapes(lib, tune):
    """The small shapes of tests/test_conv_dgrad_gpu.py: the default route of each gradient launch, among them the two kinds of image that
    are no whole number of slabs and stay on the register-staged kernel."""
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    assert len(R.SMALL_DEFAULT_ROUTES) == len(R.SMALL_3X3) + len(R.SMALL_1X1)
    for k, shapes in ((3, R.SMALL_3X3), (1, R.SMALL_1X1)):
        for s in shapes:
            assert tuple(route_of(lib, *R.dgrad_launch(*s), taps=k * k)) == R.SMALL_DEFAULT_ROUTES[s + (k,)], s
    tune(conv_dma=0)
    for k, shapes in ((3, R.SMALL_3X3), (1, R.SMALL_1X1)):
        for s in shapes:
            assert route_of(lib, *R.dgrad_launch(*s), taps=k * k).family == "register", s


def test_forced_routes_of_the_small_shapes(lib, tune):
    """Every forced (tiling, halo form) of the GPU matrix on every small 3 x 3 shape is either the route the query reports or ineligible for a
    stated reason; each of the new channel counts 960, 1920 and 2560 is reachable on every tiling and on the halo form, and the three
    forced routes of the impulse test are what they are named."""
    ran = set()
    for s in R.SMALL_3X3:
        launch = R.dgrad_launch(*s)
        for cfg, halo in FORCED[1:]:
            tune(conv_cfg=cfg, conv_halo=halo, conv_dma=-1)
            r = route_of(lib, *launch)
            if R.forced_route_mismatch(r, launch, cfg, halo) is None:
                assert (r.tiling, r.halo) == (cfg, bool(halo)), (s, cfg, halo, r)
                ran.add((cfg, bool(halo), launch[4]))
    for co in (960, 1920, 2560):
        assert {(cfg, h) for cfg, h, c in ran if c == co} == {(cfg, h) for cfg in range(1, 7) for h in (False, True)}, co
    assert {cfg for cfg, _, c in ran if c == 64} == {2, 3, 4}  # 64 and 128 output channels: not the 320-channel tilings
    for s in R.IMPULSE_SHAPES:
        launch = R.dgrad_launch(*s)
        for kw, want in ((dict(conv_halo=1), ("dma", 4, True, 64)), (dict(conv_cfg=3, conv_halo=0), ("dma", 3, False, 128)),
                         (dict(conv_dma=0), ("register", 0, False, 0))):
            tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
            tune(**kw)
            assert tuple(route_of(lib, *launch)) == want, (s, kw)


# ------------------------------------------------------------------------------------------------ the bar admits a correct kernel
@pytest.mark.parametrize("N,H,W,cin,cout,stride,k", [s + (3,) for s in R.SMALL_3X3] + [s + (1,) for s in R.SMALL_1X1])
def test_the_recipe_in_fp32_rounded_once_passes_the_bar(N, H, W, cin, cout, stride, k):
    """ConvIgemmFn.backward's recipe (flip, transpose, pad, zero-insert, stride-1 convolution, slice) as plain torch in fp32, rounded once
    to bf16, against the fp64 autograd reference under the GPU tests' bar |got - ref| <= 2^-8 |ref| + 1e-4 A, every element -- and exactly
    equal to it when computed in fp64, which pins the reference helpers against the recipe."""
    c = R.case(N, H, W, cin, cout, stride, k)
    assert c.dx.shape == (N, H * W, cin) and c.A.shape == c.dx.shape and (c.A >= c.dx.abs() * (1 - 1e-12)).all()
    exact = R.recipe_dx(c.w, c.dy, N, H, W, stride, torch.float64)
    assert (exact - c.dx).abs().max() <= 1e-12 * c.A.max()
    with _fp32_exact():
        got = R.recipe_dx(c.w, c.dy, N, H, W, stride, torch.float32).to(torch.bfloat16)
    assert_close(got.reshape(-1, cin), c.dx.reshape(-1, cin), c.A.reshape(-1, cin), f"recipe {c.shape}")
    if c.emb is not None:  # d_res = dy; d_emb = the fp32 sum over each image's pixels, rounded once
        assert torch.equal(c.d_res, c.dy)
        n = (H // stride) * (W // stride)
        d_emb = c.dy.float().reshape(N, n, cout).sum(1).to(torch.bfloat16).double()
        assert ((d_emb - c.d_emb).abs() <= 2.0 ** -8 * c.d_emb.abs() + n * 2.0 ** -24 * c.A_emb).all()
        assert torch.equal(c.A_emb, c.dy.abs().sum(1))


def test_the_bar_rejects_a_misplaced_tap_and_a_wrong_border():
    """What a global max-norm bar can let through and this one must not: one tap's weights exchanged with its mirror image, and an image
    whose rows are shifted by one pixel (wrong border columns)."""
    N, H, W, cin, cout, stride = 2, 16, 8, 128, 128, 2
    c = R.case(N, H, W, cin, cout, stride)
    w = c.w.clone()
    w[:, :, 0, 1], w[:, :, 2, 1] = c.w[:, :, 2, 1], c.w[:, :, 0, 1]
    with pytest.raises(AssertionError):
        assert_close(R.recipe_dx(w, c.dy, N, H, W, stride).to(torch.bfloat16).reshape(-1, cin), c.dx.reshape(-1, cin), c.A.reshape(-1, cin), "tap")
    shifted = R.recipe_dx(c.w, c.dy, N, H, W, stride).reshape(N, H, W, cin).roll(1, 2)  # every row one pixel to the right, wrapped round
    with pytest.raises(AssertionError):
        assert_close(shifted.to(torch.bfloat16).reshape(-1, cin), c.dx.reshape(-1, cin), c.A.reshape(-1, cin), "border")


@pytest.mark.parametrize("N,H,W,cin,cout,stride", R.IMPULSE_SHAPES)
def test_impulse_expectations_are_the_autograd_gradient(N, H, W, cin, cout, stride):
    """The expectation of the bit-exact impulse test: a one-hot dy gives exactly one weight slice placed round the pixel (single products
    with 1.0), which fp64 autograd and the recipe in fp32 / bf16 reproduce bit for bit."""
    w = R.impulse_weight(cout, cin)
    assert not torch.equal(w, w.flip(2)) and not torch.equal(w, w.flip(3)) and not torch.equal(w, w.transpose(2, 3))
    assert all(w[co].abs().unique().numel() == 9 * cin for co in (0, 7, cout - 1))
    ho, wo = H // stride, W // stride
    x = torch.zeros(N, H * W, cin, dtype=torch.float64)
    pos = R.impulse_positions(ho, wo)
    assert len(set(pos)) == 9 and all(0 <= y < ho and 0 <= x_ < wo for y, x_ in pos)
    for i, (yo, xo) in enumerate(pos):
        co = R.impulse_channel(i, cout)
        dy = R.impulse_dy(N, ho, wo, cout, 1, yo, xo, co)
        want = R.impulse_expected(w, N, H, W, stride, 1, yo, xo, co)
        _, dx, _, _ = R.autograd_reference(x, w, None, None, None, dy, N, H, W, stride)
        assert torch.equal(dx, want), (yo, xo, co)
        assert torch.equal(R.recipe_dx(w, dy, N, H, W, stride).to(torch.bfloat16).double(), want), (yo, xo, co)
        inside = sum(0 <= stride * yo + ky - 1 < H and 0 <= stride * xo + kx - 1 < W for ky in range(3) for kx in range(3))
        assert int((want != 0).sum()) == inside * cin and not want[0].any()
