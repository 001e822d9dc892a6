"""Every route of the 3 x 3 convolution entry points against a high-precision reference, element by element.  Needs an MI355X.

cd360_conv_igemm_bf16 / cd360_conv3x3_dma_bf16 serve a 3 x 3 convolution with one of six tilings of the LDS-DMA core, its halo form or the
register-staged kernel; cd360_conv_up2x_bf16 with one of the six tilings.  Each case first asks the route query which kernel it will reach
and asserts that it is the one the case is named for (a forced tiling the shape cannot take is skipped, never tested under that name).

Comparison: inputs rounded to bf16 for both sides; the reference in fp64 on the host (small shapes) or fp32 on the GPU (product shapes,
nine fp32 GEMMs with TF32 off).  With A the same sum over absolute values, every element must satisfy
    |got - ref| <= 2^-8 |ref| + 1e-4 A
(one bf16 rounding plus fp32 summation slack).  Statistics: a buffer of TWICE the promised size, NaN-filled; every promised slab must hold
the fp64 sum / sum of squares of the returned bf16 output within 1e-5 of the slab's sum of |out| / out^2, the rest must stay NaN, and the
GroupNorm fed from them must match the GroupNorm with its own statistics pass."""
import functools
import math

import pytest
import torch

from conv_shapes import BATCHES, UNET_3X3, UNET_ROUTES, UNET_UP2X, UNET_UP2X_TILINGS, VAE_3X3, VAE_UP2X

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_BAR, ABS_SLACK = 2.0 ** -8, 1e-4
SLAB_OF_TILING = {1: 64, 2: 64, 3: 128, 4: 64, 5: 64, 6: 32}
NEEDS_320 = (1, 5, 6)


def _lib():
    from cd360 import _lib
    return _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def bfr(t):
    return t.to(torch.bfloat16).to(t.dtype)


def halo_fits(N, H, W, Cin):
    return W >= 8 and 128 % W == 0 and (H * W) % 128 == 0 and (128 // W + 2) * (W + 2) <= 9 * 32 and Cin >= 64


class _fp32_exact:
    """fp32 GEMMs without TF32 (the GPU reference)."""

    def __enter__(self):
        self.saved = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False

    def __exit__(self, *a):
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = self.saved
        return False


def conv_ref(x, w, bias=None, emb=None, res=None, stride=1, up=False):
    """x [N, H, W, Cin], w [Cout, Cin, k, k] (k = 3, pad 1, or 1) in x's dtype and device -> (ref, A), [N * Ho * Wo, Cout]: the
    convolution (of the nearest-2x image when `up`) + bias + emb[n] + res, and the same sum over absolute values."""
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    N, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[-1]
    Ho, Wo = H // stride, W // stride

    def run(x, w, bias, emb, res):
        xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1)) if k == 3 else x
        acc = torch.zeros(N * Ho * Wo, Cout, dtype=x.dtype, device=x.device)
        for ky in range(k):
            for kx in range(k):
                acc += xp[:, ky:ky + H:stride, kx:kx + W:stride, :].reshape(-1, Cin) @ w[:, :, ky, kx].t()
        if bias is not None:
            acc += bias
        if emb is not None:
            acc = (acc.view(N, Ho * Wo, Cout) + emb[:, None, :]).view(-1, Cout)
        if res is not None:
            acc += res.reshape(-1, Cout)
        return acc

    ab = lambda t: None if t is None else t.abs()  # noqa: E731
    with _fp32_exact():
        return run(x, w, bias, emb, res), run(x.abs(), w.abs(), ab(bias), ab(emb), ab(res))


def assert_close(got, ref, A, what):
    got = got.to(ref.device, ref.dtype).reshape(ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    bar = REL_BAR * ref.abs() + ABS_SLACK * A
    bad = err > bar
    if bad.any():
        i = int(torch.argmax(err / bar))
        r, c = divmod(i, ref.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements above the bar; worst pixel {r} channel {c}: got "
                             f"{got.view(-1)[i].item():.6g} ref {ref.view(-1)[i].item():.6g} bar {bar.view(-1)[i].item():.3g}")


def check_stats(out, buf, N, HW, Cout, rows, guard=True):
    """buf: the flat fp32 statistics of `out` ([N HW, Cout] bf16) in slabs of `rows` pixels, followed (guard) by as many NaNs."""
    promised = (N * HW // rows) * Cout * 2
    assert buf.numel() == (2 if guard else 1) * promised
    st = buf[:promised].view(-1, Cout, 2).double()
    assert torch.isfinite(st).all(), "a promised slab was not written"
    o = out.double().view(-1, rows, Cout)
    s, q, a = o.sum(1), (o * o).sum(1), o.abs().sum(1)
    assert ((st[..., 0] - s).abs() <= 1e-5 * a).all(), float(((st[..., 0] - s).abs() / a).max())
    assert ((st[..., 1] - q).abs() <= 1e-5 * q).all(), float(((st[..., 1] - q).abs() / q).max())
    if guard:
        assert torch.isnan(buf[promised:]).all(), "statistics written past the promised size"
    from cd360 import ops
    g = torch.Generator(device=DEV).manual_seed(Cout)
    gamma, beta = torch.randn(Cout, generator=g, device=DEV), torch.randn(Cout, generator=g, device=DEV)
    groups = 32 if Cout % 32 == 0 else 16
    x = out.view(N, HW, Cout)
    a_ = ops.gn_silu(x, gamma, beta, groups, 1e-5, True, tile_stats=buf[:promised].view(N, HW // rows, Cout, 2)).float()
    b_ = ops.gn_silu(x, gamma, beta, groups, 1e-5, True).float()
    assert (a_ - b_).abs().max().item() / b_.abs().max().item() < 4e-3, rows


def launch(entry, x, wp, bias, emb, res, N, H, W, Cin, Cout, stats_rows=None, taps=9, stride=1):
    """One call of the C entry point -> (out [N Ho Wo, Cout] bf16, statistics buffer of twice the promised size, or None)."""
    L = _lib()
    Ho, Wo = H // stride, W // stride
    out = torch.empty(N * Ho * Wo, Cout, dtype=torch.bfloat16, device=DEV)
    buf = None
    if stats_rows:
        buf = torch.full((2 * (N * Ho * Wo // stats_rows) * Cout * 2,), float("nan"), dtype=torch.float32, device=DEV)
    es = 0 if emb is None else emb.stride(0)
    s = torch.cuda.current_stream().cuda_stream
    if entry == "dma":
        rc = L.load().cd360_conv3x3_dma_bf16(_ptr(x), _ptr(wp), _ptr(bias), _ptr(emb), es, _ptr(res), _ptr(out), N, H, W, Cin, Cout, _ptr(buf), s)
    else:
        rc = L.load().cd360_conv_igemm_bf16(_ptr(x), _ptr(wp), _ptr(bias), _ptr(emb), es, _ptr(res), _ptr(out), N, H, W, Cin, Cout, taps, stride,
                                            _ptr(buf), s)
    L.check(rc, entry)
    return out, buf


def inputs(N, H, W, Cin, Cout, extras, device, dtype, seed, k=3, grid=False, stride=1):
    """bf16-valued x [N, H, W, Cin], w [Cout, Cin, k, k], fp32-valued bias, bf16-valued emb [N, Cout] / res [N Ho Wo, Cout] (extras).
    grid: weights on a 2^-j grid with at most 7 significant bits, so that the folded upsample phases (sums of up to four taps) are
    exact in bf16 and the reference's unfolded weights are the kernel's."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = bfr(torch.randn(N, H, W, Cin, generator=g, device=device, dtype=dtype))
    if grid:
        step = 2.0 ** -math.ceil(math.log2(64 * math.sqrt(k * k * Cin)))
        w = torch.randint(-64, 65, (Cout, Cin, k, k), generator=g, device=device).to(dtype) * step
    else:
        w = bfr(torch.randn(Cout, Cin, k, k, generator=g, device=device, dtype=dtype) / math.sqrt(k * k * Cin))
    bias = torch.randn(Cout, generator=g, device=device, dtype=dtype).float().to(dtype)
    emb = bfr(torch.randn(N, Cout, generator=g, device=device, dtype=dtype)) if extras else None
    res = bfr(torch.randn(N * (H // stride) * (W // stride), Cout, generator=g, device=device, dtype=dtype)) if extras else None
    return x, w, bias, emb, res


def to_dev(x, w, bias, emb, res, k=3):
    from cd360 import ops
    b16 = lambda t: None if t is None else t.to(DEV, torch.bfloat16).contiguous()  # noqa: E731
    wp = ops.pack_conv_weight(w.to(DEV, torch.float32) if k == 3 else w.to(DEV, torch.float32).reshape(w.shape[0], -1))
    return b16(x).view(-1, x.shape[-1]), wp, bias.to(DEV, torch.float32), b16(emb), b16(res)


@functools.lru_cache(maxsize=8)
def small_case(N, H, W, Cin, Cout, extras, stride=1, k=3):
    """inputs + fp64 host reference of a small convolution (shared by the parametrized cases of one shape)"""
    x, w, bias, emb, res = inputs(N, H, W, Cin, Cout, extras, "cpu", torch.float64, N * 1000 + H * 31 + W + Cin + Cout, k=k, stride=stride)
    ref, A = conv_ref(x, w, bias, emb, res, stride=stride)
    return to_dev(x, w, bias, emb, res, k=k), ref, A


def run_and_check(entry, dev_args, ref, A, N, H, W, Cin, Cout, rows, what, taps=9, stride=1):
    """launch with statistics (rows > 0) twice and without once: per-element output, statistics, determinism"""
    x, wp, bias, emb, res = dev_args
    out, buf = launch(entry, x, wp, bias, emb, res, N, H, W, Cin, Cout, rows, taps, stride)
    assert_close(out, ref, A, what)
    HW = (H // stride) * (W // stride)
    if rows:
        check_stats(out, buf, N, HW, Cout, rows)
        out2, buf2 = launch(entry, x, wp, bias, emb, res, N, H, W, Cin, Cout, rows, taps, stride)
        half = buf.numel() // 2
        assert torch.equal(out2, out) and torch.equal(buf2[:half], buf[:half]), "repeated launches differ"
    plain, _ = launch(entry, x, wp, bias, emb, res, N, H, W, Cin, Cout, None, taps, stride)
    assert torch.equal(plain, out), "the output depends on whether statistics were asked for"
    return out


# ------------------------------------------------------------------------------------------------ a. the LDS-DMA core, forced
FORCED = [(-1, -1)] + [(c, h) for c in range(1, 7) for h in (0, 1)]
EDGE_SHAPES = [  # (N, H, W, Cin, Cout, bias + emb + res, entry)
    (2, 9, 7, 128, 320, True, "dma"),     # 63-pixel images: a ragged last tile for every BM (128 / 192 / 256); the DMA entry, no statistics
    (3, 16, 8, 64, 320, False, "igemm"),  # 128-pixel images: 192 / 256-pixel tiles straddle images, 32 / 64 / 128-row slabs do not;
                                          # one 64-channel K chunk; W = 8 halo geometry
    (5, 16, 8, 128, 48, True, "igemm"),   # 640 pixels: ragged last tile for BM 192 and 256; 48 channels: ragged channel tile
    (1, 8, 16, 192, 80, True, "igemm"),   # W = 16 halo geometry, a tile that is exactly one image; 80 channels
    (2, 4, 32, 384, 640, True, "igemm"),  # W = 32, tile = one image; K = 3456 >= 3072: the K-split wave arrangement; 640 of 256 ragged
    (2, 2, 64, 64, 640, False, "igemm"),  # W = 64 halo geometry (two 64-pixel rows per tile)
]


@pytest.mark.parametrize("cfg,halo", FORCED, ids=[f"cfg{c}-halo{h}" for c, h in FORCED])
@pytest.mark.parametrize("N,H,W,Cin,Cout,extras,entry", EDGE_SHAPES)
def test_dma_core_forced_routes(cfg, halo, N, H, W, Cin, Cout, extras, entry, tune):
    from cd360 import ops
    tune(conv_cfg=cfg, conv_halo=halo, conv_dma=-1)
    r = ops.conv3x3_dma_route(N, H, W, Cin, Cout) if entry == "dma" else ops.conv_route(N, H, W, Cin, Cout)
    assert r.family == "dma", r
    if cfg > 0 and r.tiling != cfg:
        assert cfg in NEEDS_320 and Cout % 320, (cfg, r)
        pytest.skip(f"tiling {cfg} needs Cout % 320 == 0 (Cout = {Cout})")
    if halo == 1 and not r.halo:
        assert not halo_fits(N, H, W, Cin), r
        pytest.skip(f"the halo form does not fit {H} x {W} images")
    assert r.halo == (halo == 1 or (halo == -1 and r.tiling == 4 and halo_fits(N, H, W, Cin))), r
    assert r.slab_rows == (64 if r.halo else SLAB_OF_TILING[r.tiling]), r
    dev_args, ref, A = small_case(N, H, W, Cin, Cout, extras)
    rows = r.slab_rows if entry == "igemm" else None
    run_and_check(entry, dev_args, ref.to(DEV), A.to(DEV), N, H, W, Cin, Cout, rows, f"{r}")


@functools.lru_cache(maxsize=1)
def gpu_case(N, H, W, Cin, Cout, extras, up=False):
    """inputs on the GPU + fp32 GPU reference of a product-sized convolution (or folded upsample: grid weights, no emb / res)"""
    x, w, bias, emb, res = inputs(N, H, W, Cin, Cout, extras and not up, DEV, torch.float32, N * 7 + H + Cin * 3 + Cout, grid=up)
    ref, A = conv_ref(x, w, bias, emb, res, up=up)
    return (x, w, bias, emb, res), ref, A


@pytest.mark.parametrize("cfg,halo", [(3, 1), (6, 1), (3, 0), (-1, -1)])
def test_halo_form_under_every_slab_size_at_the_32x32_level(cfg, halo, tune):
    """M = 24576 pixels at 32^2, 1280 -> 1280 (the fine-tune step's 24 views; tiling 3 by default): the halo form combined with the
    128-row (tiling 3) and 32-row (tiling 6) tilings must write its own 64-row slabs into a buffer sized for them, and nothing past it."""
    from cd360 import ops
    N, H, W, Cin, Cout = 24, 32, 32, 1280, 1280
    tune(conv_cfg=cfg, conv_halo=halo, conv_dma=-1)
    r = ops.conv_route(N, H, W, Cin, Cout)
    want = ("dma", 3, False, 128) if cfg < 0 else ("dma", cfg, halo == 1, 64 if halo == 1 else SLAB_OF_TILING[cfg])  # (default: tiling 3)
    assert r == want, r
    (x, w, bias, emb, res), ref, A = gpu_case(N, H, W, Cin, Cout, True)
    run_and_check("igemm", to_dev(x, w, bias, emb, res), ref, A, N, H, W, Cin, Cout, r.slab_rows, f"{r}")


# ------------------------------------------------------------------------------------------------ b. product shapes, default tuning
PRODUCT = [(n, h, cin, cout, UNET_ROUTES[n, h], what) for n in BATCHES for h, cin, cout, what in UNET_3X3] + \
          [(1, h, cin, cout, route, "VAE " + what) for h, cin, cout, what, route in VAE_3X3]


@pytest.mark.parametrize("N,S,Cin,Cout,route,what", PRODUCT, ids=[f"{n}x{s}x{s}-{ci}-{co}" for n, s, ci, co, _, _ in PRODUCT])
def test_product_convolutions_at_default_tuning(N, S, Cin, Cout, route, what, tune):
    from cd360 import ops
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    r = ops.conv_route(N, S, S, Cin, Cout)
    assert tuple(r) == ("dma",) + route, (what, r)
    (x, w, bias, emb, res), ref, A = gpu_case(N, S, S, Cin, Cout, True)
    run_and_check("igemm", to_dev(x, w, bias, emb, res), ref, A, N, S, S, Cin, Cout, r.slab_rows, f"{what}: {r}")


UP_PRODUCT = [(n, s, c, UNET_UP2X_TILINGS[n, s]) for n in BATCHES for s, c in UNET_UP2X] + [(1, s, c, t) for s, c, t in VAE_UP2X]


@pytest.mark.parametrize("N,S,C,tiling", UP_PRODUCT, ids=[f"{n}x{s}x{s}-{c}" for n, s, c, _ in UP_PRODUCT])
def test_product_upsample_convolutions_at_default_tuning(N, S, C, tiling, tune):
    from cd360 import ops
    tune(conv_cfg=-1)
    assert ops.conv_up2x_tiling(N, S, S, C, C) == tiling
    (x, w, bias, _, _), ref, A = gpu_case(N, S, S, C, C, False, up=True)
    xt = x.to(torch.bfloat16).reshape(N, S * S, C).contiguous()
    wp = ops.pack_upsample_conv_weight(w)
    got = ops.conv_up2x(xt, wp, bias, N, S, S)
    assert_close(got, ref, A, f"up2x tiling {tiling}")
    assert torch.equal(got, ops.conv_up2x(xt, wp, bias, N, S, S))


# ------------------------------------------------------------------------------------------------ c. the folded upsample, forced
UP_SHAPES = [(2, 8, 8, 64, 320), (1, 5, 7, 128, 80), (2, 6, 10, 192, 640), (1, 3, 9, 64, 48)]


@functools.lru_cache(maxsize=4)
def small_up_case(N, H, W, Cin, Cout):
    x, w, bias, _, _ = inputs(N, H, W, Cin, Cout, False, "cpu", torch.float64, N + H * 5 + W + Cin + Cout, grid=True)
    ref, A = conv_ref(x, w, bias, up=True)
    return x, w, bias, ref, A


@pytest.mark.parametrize("cfg", [-1, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("N,H,W,Cin,Cout", UP_SHAPES)
def test_upsample_forced_tilings(cfg, N, H, W, Cin, Cout, tune):
    from cd360 import ops
    tune(conv_cfg=cfg)
    t = ops.conv_up2x_tiling(N, H, W, Cin, Cout)
    if cfg > 0 and t != cfg:
        assert cfg in NEEDS_320 and Cout % 320, (cfg, t)
        pytest.skip(f"tiling {cfg} needs Cout % 320 == 0 (Cout = {Cout})")
    x, w, bias, ref, A = small_up_case(N, H, W, Cin, Cout)
    xt = x.to(DEV, torch.bfloat16).reshape(N, H * W, Cin).contiguous()
    wp = ops.pack_upsample_conv_weight(w.to(DEV, torch.float32))
    got = ops.conv_up2x(xt, wp, bias.to(DEV, torch.float32), N, H, W)
    assert_close(got, ref.to(DEV), A.to(DEV), f"up2x tiling {t}")
    assert torch.equal(got, ops.conv_up2x(xt, wp, bias.to(DEV, torch.float32), N, H, W))


# ------------------------------------------------------------------------------------------------ d. the register-staged kernel, 1 x 1
@pytest.mark.parametrize("wide,wmajor,split", [(w, m, s) for w in (-1, 0) for m in (0, 1) for s in (1, 2)])
@pytest.mark.parametrize("N,H,W,Cin,Cout,stride", [(2, 16, 8, 128, 320, 1), (1, 16, 16, 192, 256, 1), (3, 8, 16, 64, 160, 1),
                                                   (2, 32, 32, 64, 128, 2), (1, 32, 16, 128, 320, 2)])
def test_register_staged_kernel_with_statistics(wide, wmajor, split, N, H, W, Cin, Cout, stride, tune):
    from cd360 import ops
    tune(conv_dma=0, conv_wide=wide, conv_wmajor=wmajor, conv_split=split)
    assert ops.conv_route(N, H, W, Cin, Cout, 9, stride).family == "register"
    L = _lib().load()
    rows = L.cd360_conv_stats_rows(N, H, W, Cin, Cout, 9, stride)
    assert rows == (32 if Cout % 160 == 0 and Cout % 128 and wide != 0 else 64), rows
    dev_args, ref, A = small_case(N, H, W, Cin, Cout, True, stride)
    run_and_check("igemm", dev_args, ref.to(DEV), A.to(DEV), N, H, W, Cin, Cout, rows, f"register wide {wide} wmajor {wmajor} split {split}",
                  stride=stride)


@pytest.mark.parametrize("dma", [-1, 0])
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 16, 16, 192, 256), (3, 8, 16, 640, 320)])
def test_pointwise_convolution_routes(dma, N, H, W, Cin, Cout, tune):
    """1 x 1 (the skip connections): the GEMM entry without emb / statistics, the register-staged kernel with statistics or conv_dma = 0"""
    from cd360 import ops
    tune(conv_dma=dma)
    r = ops.conv_route(N, H, W, Cin, Cout, 1, 1)
    assert r.family == ("gemm" if dma else "register"), r
    (x, wp, bias, emb, res), ref, A = small_case(N, H, W, Cin, Cout, True, 1, 1)
    ref, A = ref.to(DEV), A.to(DEV)
    # without emb: the GEMM entry (dma = -1); the reference is rebuilt without the per-image addend
    ref_noemb, A_noemb = ref - _emb_rows(emb, N, H * W), A - _emb_rows(emb, N, H * W).abs()
    run_and_check("igemm", (x, wp, bias, None, res), ref_noemb, A_noemb, N, H, W, Cin, Cout, None, f"1x1 {r}", taps=1)
    rows = _lib().load().cd360_conv_stats_rows(N, H, W, Cin, Cout, 1, 1)  # with statistics: the register-staged kernel's slabs
    run_and_check("igemm", (x, wp, bias, emb, res), ref, A, N, H, W, Cin, Cout, rows, "1x1 with statistics", taps=1)


def _emb_rows(emb, N, HW):
    return emb.double().repeat_interleave(HW, 0)


# ------------------------------------------------------------------------------------------------ e. per-stream tuning
def test_per_stream_tuning_sizes_and_fills_the_statistics(tune):
    """A side stream whose override gives tiling 6 (32-row slabs) while the process default gives tiling 3 (128-row slabs):
    ops.conv_igemm(want_stats=True) must size and fill the statistics of each launch for the stream it runs on."""
    from cd360 import ops
    N, H, W, Cin, Cout = 3, 16, 8, 64, 320
    tune(conv_cfg=3, conv_halo=0, conv_dma=-1)
    (x, wp, bias, emb, res), ref, A = small_case(N, H, W, Cin, Cout, True)
    ref, A = ref.to(DEV), A.to(DEV)
    side = torch.cuda.Stream()
    _lib().set_stream_tuning(side, conv_cfg=6)
    try:
        assert ops.conv_route(N, H, W, Cin, Cout) == ("dma", 3, False, 128)
        out, st = ops.conv_igemm(x, wp, bias, N, H, W, 9, emb, res, want_stats=True)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert ops.conv_route(N, H, W, Cin, Cout) == ("dma", 6, False, 32)
            out_s, st_s = ops.conv_igemm(x, wp, bias, N, H, W, 9, emb, res, want_stats=True)
        torch.cuda.current_stream().wait_stream(side)
        assert st.shape == (N, H * W // 128, Cout, 2) and st_s.shape == (N, H * W // 32, Cout, 2)
        for o, s, rows in ((out, st, 128), (out_s, st_s, 32)):
            assert_close(o, ref, A, f"{rows}-row slabs")
            check_stats(o.view(-1, Cout), s.view(-1), N, H * W, Cout, rows, guard=False)
    finally:
        _lib().clear_stream_tuning(side)
