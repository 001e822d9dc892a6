"""The convolution data gradient, element by element, on every route it takes.  Needs an MI355X.

A frozen convolution under autograd (sgm...util.conv_tokens -> cd360.grad.ConvIgemmFn) has no backward kernel of its own: dx is
cd360_conv_igemm_bf16 launched again on dy with the weight of packed_conv_dgrad (taps flipped, channels transposed, both channel counts
re-padded; dy zero-inserted for a stride-2 convolution), sliced back to cin.  Those launches run channel counts no forward launch runs
(Cout' = 64, 960, 1920, 2560 next to 320, 640, 1280: tests/conv_shapes.py), and the Python side has a flip, a transposition, two paddings
and a slice to get wrong.  Every case drives conv_tokens itself, asks ops.conv_route for the GRADIENT launch (N, H, W, Cin', Cout') first
and asserts that it is the route the case is named for (a forced route the shape cannot take is skipped, never tested under that name).

Reference: torch.autograd.grad through F.conv2d in fp64 on the host (tests/conv_dgrad_ref.py; tests/test_conv_dgrad_cpu.py holds it to the
recipe on the host), inputs bf16-valued on both sides.  With A the same gradient of |w| and |dy|, EVERY element of dx must satisfy the bar
of tests/test_conv_routes_gpu.py, |got - ref| <= 2^-8 |ref| + 1e-4 A.  d_res must be dy bit for bit, d_emb within
2^-8 |ref| + n 2^-24 A_emb (an fp32 sum of the image's n pixels, rounded once), two backward runs bit-identical."""
import functools

import pytest
import torch

import conv_dgrad_ref as R
from conv_shapes import UNET_DGRAD_ROUTES, dgrad_product_launches
from test_conv_routes_gpu import DEV, FORCED, REL_BAR, assert_close, gpu_case, run_and_check, to_dev

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ALL_3X3 = [s + (3,) for s in R.SMALL_3X3]
ALL_1X1 = [s + (1,) for s in R.SMALL_1X1]
SHAPE_ARGS = "N,H,W,cin,cout,stride,k"


def make_conv(w, bias, stride):
    """A frozen bf16 nn.Conv2d on the GPU holding the (bf16-valued) fp64 weight `w` and bias"""
    import torch.nn as nn
    cout, cin, k, _ = w.shape
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=bias is not None)
    with torch.no_grad():
        conv.weight.copy_(w)
        if bias is not None:
            conv.bias.copy_(bias)
    return conv.requires_grad_(False).to(DEV, BF)


@functools.lru_cache(maxsize=2)
def dev_case(N, H, W, cin, cout, stride, k):
    """the shape's reference (shared by its forced routes) + its module and operands on the GPU"""
    c = R.case(N, H, W, cin, cout, stride, k)
    d = lambda t: None if t is None else t.to(DEV, BF)  # noqa: E731
    return c, make_conv(c.w, c.bias, stride), d(c.x), d(c.emb), d(c.res), d(c.dy)


def run(conv, x, emb, res, dy, N, H, W, want_stats=False):
    """conv_tokens under autograd + backward -> (y, stats, dx, d_emb, d_res)"""
    from sgm.modules.diffusionmodules.util import conv_tokens
    leaf = lambda t: None if t is None else t.detach().clone().requires_grad_(True)  # noqa: E731
    x, emb, res = leaf(x), leaf(emb), leaf(res)
    out = conv_tokens(conv, x, N, H, W, emb=emb, res=res, want_stats=want_stats)
    y, stats = out if want_stats else (out, None)
    node = y.grad_fn  # the graph must be ConvIgemmFn's (below at most the slice of a padded channel count), not torch's own convolution
    while node is not None and "ConvIgemmFn" not in type(node).__name__:
        assert "Slice" in type(node).__name__ or "Alias" in type(node).__name__, type(node).__name__
        node = node.next_functions[0][0]
    assert node is not None, "conv_tokens did not go through ConvIgemmFn"
    y.backward(dy)
    g = lambda t: None if t is None else t.grad  # noqa: E731
    return y.detach(), stats, x.grad, g(emb), g(res)


def check(shape, what):
    """one shape under the tuning in force: forward, dx per element, d_emb, d_res, determinism"""
    N, H, W, cin, cout, stride, k = shape
    c, conv, x, emb, res, dy = dev_case(*shape)
    y, _, dx, d_emb, d_res = run(conv, x, emb, res, dy, N, H, W)
    assert dx.shape == x.shape and dx.dtype == BF and dx.is_contiguous()
    dev = lambda t: t.to(DEV).reshape(-1, t.shape[-1])  # noqa: E731
    assert_close(y, dev(c.y), dev(c.A_y), f"{what}: forward")
    assert_close(dx, dev(c.dx), dev(c.A), f"{what}: dx")
    if emb is not None:
        assert torch.equal(d_res, dy), f"{what}: d_res is not dy"
        n = (H // stride) * (W // stride)
        ref, a = c.d_emb.to(DEV), c.A_emb.to(DEV)
        err, bar = (d_emb.double() - ref).abs(), REL_BAR * ref.abs() + n * 2.0 ** -24 * a
        assert (err <= bar).all(), f"{what}: d_emb, worst {float((err / bar).max()):.3g} of the bar"
    again = run(conv, x, emb, res, dy, N, H, W)
    assert torch.equal(again[0], y) and torch.equal(again[2], dx), f"{what}: two runs differ"
    assert emb is None or (torch.equal(again[3], d_emb) and torch.equal(again[4], d_res)), f"{what}: two runs differ"
    return dx


# ------------------------------------------------------------------------------------------------ a. 3 x 3: default and forced routes
@pytest.mark.parametrize("cfg,halo", FORCED, ids=[f"cfg{c}-halo{h}" for c, h in FORCED])
@pytest.mark.parametrize(SHAPE_ARGS, ALL_3X3)
def test_data_gradient_on_the_dma_core_routes(cfg, halo, N, H, W, cin, cout, stride, k, tune):
    """cfg -1 / halo -1: the default route of the gradient launch, pinned in conv_dgrad_ref.SMALL_DEFAULT_ROUTES (the register-staged
    kernel for the 63- and 96-pixel images); else the forced (tiling, halo form)."""
    from cd360 import ops
    tune(conv_cfg=cfg, conv_halo=halo, conv_dma=-1)
    launch = R.dgrad_launch(N, H, W, cin, cout)
    r = ops.conv_route(*launch)
    if cfg < 0:
        assert tuple(r) == R.SMALL_DEFAULT_ROUTES[N, H, W, cin, cout, stride, k], r
    else:
        why = R.forced_route_mismatch(r, launch, cfg, halo)
        if why:
            pytest.skip(why)
        assert (r.family, r.tiling, r.halo) == ("dma", cfg, bool(halo)), r
    check((N, H, W, cin, cout, stride, k), f"launch {launch} {r}")


# ------------------------------------------------------------------------------------------------ b. the register-staged kernel, 1 x 1
@pytest.mark.parametrize(SHAPE_ARGS, ALL_3X3 + ALL_1X1)
def test_data_gradient_on_the_register_staged_kernel(N, H, W, cin, cout, stride, k, tune):
    from cd360 import ops
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=0)
    launch = R.dgrad_launch(N, H, W, cin, cout)
    r = ops.conv_route(*launch, k * k, 1)
    assert r.family == "register", r
    check((N, H, W, cin, cout, stride, k), f"launch {launch} {r}")


@pytest.mark.parametrize(SHAPE_ARGS, ALL_1X1)
def test_data_gradient_of_the_skip_connections_on_the_gemm_entry(N, H, W, cin, cout, stride, k, tune):
    """1 x 1: dx = dy W on cd360_gemm_bf16 with N' = 960 and 1920"""
    from cd360 import ops
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    launch = R.dgrad_launch(N, H, W, cin, cout)
    r = ops.conv_route(*launch, 1, 1)
    assert tuple(r) == R.SMALL_DEFAULT_ROUTES[N, H, W, cin, cout, stride, k] == ("gemm", 0, False, 0), r
    check((N, H, W, cin, cout, stride, k), f"launch {launch} {r}")


# ------------------------------------------------------------------------------------------------ c. product-size gradient launches
PRODUCT = dgrad_product_launches()


@pytest.mark.parametrize("N,S,ci,co,tiling,halo", PRODUCT, ids=[f"{n}x{s}x{s}-{ci}-{co}-cfg{t}-halo{int(h)}" for n, s, ci, co, t, h in PRODUCT])
def test_product_size_gradient_launches_on_routes_no_forward_launch_takes(N, S, ci, co, tiling, halo, tune):
    """For every (tiling, halo form, Cout') only the data gradient reaches at default tuning (conv_shapes.DGRAD_ONLY_ROUTES), the smallest
    UNet gradient launch that takes it, at its real size -- several rounds of workgroups, up to eight channel tiles on tiling 1 -- as
    ConvIgemmFn.backward launches it (no emb, no residual, no statistics); against nine fp32 GEMMs on the GPU, element by element."""
    from cd360 import ops
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    r = ops.conv_route(N, S, S, ci, co)
    assert tuple(r) == ("dma",) + UNET_DGRAD_ROUTES[N, S][co] and (r.tiling, r.halo) == (tiling, halo), r
    (x, w, bias, _, _), ref, A = gpu_case(N, S, S, ci, co, False)
    run_and_check("igemm", to_dev(x, w, bias, None, None), ref, A, N, S, S, ci, co, None, f"gradient launch {(N, S, S, ci, co)} {r}")


# ------------------------------------------------------------------------------------------------ d. statistics under autograd
@pytest.mark.parametrize(SHAPE_ARGS, [s for s in ALL_3X3 if R.with_extras(s[4]) and ((s[1] // s[5]) * (s[2] // s[5])) % 128 == 0])
def test_statistics_under_autograd_are_those_of_no_grad(N, H, W, cin, cout, stride, k, tune):
    """want_stats=True (the ResBlock call sites) under autograd: the output bits and statistics of the no_grad call, and the dx bits of the
    call without statistics."""
    from sgm.modules.diffusionmodules.util import conv_tokens
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    c, conv, x, emb, res, dy = dev_case(N, H, W, cin, cout, stride, k)
    with torch.no_grad():
        y0, st0 = conv_tokens(conv, x, N, H, W, emb=emb, res=res, want_stats=True)
    assert st0 is not None and st0.dtype == torch.float32 and st0.shape[0] == N and st0.shape[2:] == (cout, 2)
    y1, st1, dx1, de1, dr1 = run(conv, x, emb, res, dy, N, H, W, want_stats=True)
    assert st1 is not None and not st1.requires_grad
    assert torch.equal(y1, y0) and torch.equal(st1, st0)
    y2, _, dx2, de2, dr2 = run(conv, x, emb, res, dy, N, H, W)
    assert torch.equal(y2, y0) and torch.equal(dx1, dx2) and torch.equal(de1, de2) and torch.equal(dr1, dr2)
    assert_close(dx1, c.dx.to(DEV).reshape(-1, cin), c.A.to(DEV).reshape(-1, cin), "dx with statistics")


# ------------------------------------------------------------------------------------------------ e. impulse responses, bit exact
IMPULSE_ROUTES = [("default", {}, ("dma", 4, True, 64)), ("halo", dict(conv_halo=1), ("dma", 4, True, 64)),
                  ("tiling3", dict(conv_cfg=3, conv_halo=0), ("dma", 3, False, 128)), ("register", dict(conv_dma=0), ("register", 0, False, 0))]


@pytest.mark.parametrize("name,tuning,route", IMPULSE_ROUTES, ids=[r[0] for r in IMPULSE_ROUTES])
@pytest.mark.parametrize("N,H,W,cin,cout,stride", R.IMPULSE_SHAPES)
def test_impulse_response_is_one_weight_slice_bit_for_bit(name, tuning, route, N, H, W, cin, cout, stride, tune):
    """A one-hot dy at (image 1, pixel, output channel) -- corners, edges, interior -- gives exactly w[co, :, ky, kx] at the input pixels
    that output pixel read and exactly zero elsewhere (single products with 1.0): names the tap, channel or border that is wrong."""
    from cd360 import ops
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    tune(**tuning)
    assert tuple(ops.conv_route(*R.dgrad_launch(N, H, W, cin, cout))) == route
    w = R.impulse_weight(cout, cin)
    conv = make_conv(w, None, stride)
    x = torch.zeros(N, H * W, cin, dtype=BF, device=DEV)
    ho, wo = H // stride, W // stride
    for i, (yo, xo) in enumerate(R.impulse_positions(ho, wo)):
        co = R.impulse_channel(i, cout)
        dy = R.impulse_dy(N, ho, wo, cout, 1, yo, xo, co).to(DEV, BF)
        dx = run(conv, x, None, None, dy, N, H, W)[2]
        want = R.impulse_expected(w, N, H, W, stride, 1, yo, xo, co).to(DEV, BF)
        if not torch.equal(dx, want):
            bad = (dx != want).nonzero()
            n, p, ci = (int(v) for v in bad[0])
            raise AssertionError(f"{name}: impulse at pixel ({yo}, {xo}) channel {co}: {len(bad)} elements differ, first at image {n} pixel "
                                 f"({p // W}, {p % W}) channel {ci}: got {float(dx[n, p, ci])!r} want {float(want[n, p, ci])!r}")


# ------------------------------------------------------------------------------------------------ f. stale packs, the envelope
@pytest.mark.parametrize("how", ["copy_", "load_state_dict"])
def test_backward_uses_the_weight_as_changed_in_place(how, tune):
    """packed_conv and packed_conv_dgrad cache their packs on the module, keyed on the weight's _version: after an in-place change of the
    frozen weight (copy_ under no_grad, which is what load_state_dict does) forward and backward must use the new weight.  (A write through
    `weight.data` does not advance torch's version counter; like a raw-pointer write it is invisible to every cache of the package and
    needs torch.autograd.graph.increment_version, as cd360.finetune.MasterAdamW.bump_versions does.)"""
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    N, H, W, cin, cout, stride, k = 2, 16, 8, 960, 64, 1, 3
    c, _, x, emb, res, dy = dev_case(N, H, W, cin, cout, stride, k)
    conv = make_conv(c.w, c.bias, stride)  # (a module of this test's own: the shared one stays as it is)
    dev = lambda t: t.to(DEV).reshape(-1, t.shape[-1])  # noqa: E731
    y, _, dx, _, _ = run(conv, x, emb, res, dy, N, H, W)
    assert_close(y, dev(c.y), dev(c.A_y), "before: forward")
    assert_close(dx, dev(c.dx), dev(c.A), "before: dx")
    w2 = R.bfr(c.w.flip(0) * -0.75 + c.w * 0.5)  # another weight altogether (bf16-valued)
    if how == "copy_":
        with torch.no_grad():
            conv.weight.copy_(w2)
    else:
        conv.load_state_dict({"weight": w2.to(BF), "bias": c.bias.to(BF)})
    y2r, dx2r, _, _ = R.autograd_reference(c.x, w2, c.bias, c.emb, c.res, c.dy, N, H, W, stride)
    A_y2, A2, _, _ = R.autograd_reference(c.x.abs(), w2.abs(), c.bias.abs(), c.emb.abs(), c.res.abs(), c.dy.abs(), N, H, W, stride)
    y2, _, dx2, _, _ = run(conv, x, emb, res, dy, N, H, W)
    assert_close(y2, dev(y2r), dev(A_y2), f"after {how}: forward")
    assert_close(dx2, dev(dx2r), dev(A2), f"after {how}: dx")


@pytest.mark.parametrize("H,W", [(9, 8), (8, 9), (7, 7)])
@pytest.mark.parametrize("grad", [False, True])
def test_stride_2_on_an_odd_image_is_refused(grad, H, W):
    """F.conv2d would give ceil(H / 2) rows; the kernel's envelope is even H and W (Ho = H / 2), so the call must raise, not return a
    tensor of another size."""
    from cd360.ops import Cd360Error
    from sgm.modules.diffusionmodules.util import conv_tokens
    N, c = 2, 64
    conv = make_conv(R.bfr(torch.randn(c, c, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(H * 10 + W)) / 24), None, 2)
    x = torch.ones(N, H * W, c, dtype=BF, device=DEV).requires_grad_(grad)
    with pytest.raises(Cd360Error):
        if grad:
            conv_tokens(conv, x, N, H, W)
        else:
            with torch.no_grad():
                conv_tokens(conv, x, N, H, W)
