"""GroupNorm / LayerNorm kernels on inputs whose mean is large next to their standard deviation, on constant groups and on group
scales spread over 2^12: every element against the fp64 reference of tests/norm_ref.py with its conditioning-aware bound
(|got - ref| <= 2^-8 |ref| + K 2^-24 unit; K comes from torch's fp32 CPU kernels, tests/test_norm_stats_cpu.py).  Needs an MI355X.

gn_silu and its gradient with their own statistics pass; gn_silu fed from the per-slab channel sums of every producer that writes them
(the offset injected through the producer's fp32 bias; reference = GroupNorm of the STORED output in fp64, never the kernel's other
path; the slab sums themselves against fp64 sums of the stored output); add_layernorm, its gradient and row_stats; the LayerNorm folded
into ops.gemm(ln=...) on every tiling family, statistics from ops.row_stats and from a producing GEMM's epilogue.  Each case also
asserts finite outputs and bit-identical repeated launches.  (cd360_conv_up2x_bf16 writes no statistics, so it is no producer here.)"""
import functools

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def twice(fn):
    """run fn twice -> the first result, after asserting the second is bit-identical"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert (x is None and y is None) or torch.equal(x, y), "repeated launches differ"
    return a


# ------------------------------------------------------------------------------------------------ gn_silu, own statistics
def _gn_check(x, gamma, beta, G, eps, silu, what):
    from cd360 import ops
    got = twice(lambda: ops.gn_silu(dev(x), dev(gamma), dev(beta), G, eps, silu))
    R.assert_within(got, *R.gn_unit(x, gamma, beta, G, eps, silu), what)


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape,ratio", R.CASES_GN, ids=[f"{'x'.join(map(str, s))}-r{r}" for s, r in R.CASES_GN])
def test_gn_silu_with_offset_groups(shape, ratio, silu, eps):
    N, P, C, G = shape
    x, gamma, beta, realised = R.gn_case(N, P, C, G, ratio)
    assert ratio == 0 or (realised >= 0.7 * ratio).all()
    _gn_check(x, gamma, beta, G, eps, silu, f"gn_silu {shape} ratio {ratio} silu {silu} eps {eps}")


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("value", R.CONSTANTS + ("all-zero",))
@pytest.mark.parametrize("shape", [(2, 100, 320, 32), (1, 256, 512, 32)])
def test_gn_silu_with_constant_groups(shape, value, eps):
    """groups holding one value (var = 0: the output is act(beta) there) next to groups of noise; and the all-zero tensor, the null
    reference image of the sampler's unconditional branch"""
    N, P, C, G = shape
    if value == "all-zero":
        x = torch.zeros(N, P, C, dtype=torch.bfloat16)
    else:
        x, _ = R.constant_groups(N, P, C, G, value)
    gamma, beta = R.affine(C)
    for silu in (False, True):
        _gn_check(x, gamma, beta, G, eps, silu, f"gn_silu {shape} constant {value} silu {silu} eps {eps}")


@pytest.mark.parametrize("silu", [False, True])
def test_gn_silu_with_group_scales_over_2_to_the_12(silu):
    N, P, C, G = 2, 256, 320, 32
    x, _ = R.wide_range(N, P, C, G)
    gamma, beta = R.affine(C)
    _gn_check(x, gamma, beta, G, 1e-5, silu, f"gn_silu wide range silu {silu}")


@pytest.mark.parametrize("silu", [False, True])
def test_gn_silu_where_the_statistics_change_form(silu):
    """gn_finalize_kernel keeps the raw E[x^2] - mean^2 up to |mean| / std = 8 and takes the centred merge beyond: offsets of
    7 x (1 .. 1.25) put groups on both sides of that threshold within one launch"""
    N, P, C, G = 2, 100, 320, 32
    x, gamma, beta, realised = R.gn_case(N, P, C, G, 7)
    assert (realised < 7.8).any() and (realised > 8.2).any()
    _gn_check(x, gamma, beta, G, 1e-5, silu, f"gn_silu around the raw / centred threshold silu {silu}")


def test_gn_silu_rejects_slabs_that_do_not_divide_the_image():
    """gn_finalize_kernel needs every slab's pixel count, so tile_stats must hold equal slabs: P % slabs != 0 is a shape error, raised
    before anything is launched"""
    from cd360 import ops
    from cd360._lib import Cd360Error
    N, P, C, G = 1, 100, 64, 32
    x, gamma, beta, _ = R.gn_case(N, P, C, G, 0)
    with pytest.raises(Cd360Error):
        ops.gn_silu(dev(x), dev(gamma), dev(beta), G, 1e-5, True, tile_stats=torch.zeros(N, 3, C, 2, device=DEV))
    torch.cuda.synchronize()


BWD_CASES = [(s, r) for s in R.GN_BWD_SHAPES for r in (0, 16, 128)]


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape,ratio", BWD_CASES, ids=[f"{'x'.join(map(str, s))}-r{r}" for s, r in BWD_CASES])
def test_gn_silu_bwd_with_offset_groups(shape, ratio, silu):
    from cd360 import ops
    N, P, C, G = shape
    x, gamma, beta, _ = R.gn_case(N, P, C, G, ratio)
    dy = R.group_scaled_noise(N, P, C, G)
    got = twice(lambda: ops.gn_silu_bwd(dev(x), dev(dy), dev(gamma), dev(beta), G, 1e-5, silu))
    R.assert_within(got, *R.gn_backward_unit(x, dy, gamma, beta, G, 1e-5, silu), f"gn_silu_bwd {shape} ratio {ratio} silu {silu}")


# ------------------------------------------------------------------------------------------------ producer statistics
def _group_bias(C, G, mag, seed):
    """fp32 [C]: one constant per group, magnitude mag (1 .. 1.25), random sign"""
    g = R._gen(C, G, seed, 37)
    return (R._offsets((G, 1), 1.0, g) * mag).expand(G, C // G).reshape(C).float()


def _check_producer(produce, C, G, ratio, what, eps=1e-5):
    """produce(bias fp32 [C] on the GPU) -> (out bf16 [N, P, C], tile_stats fp32 [N, slabs, C, 2]).  The bias-free output's standard
    deviation sets the scale of the per-group offsets; then the slab sums against fp64 sums of the stored output, and
    gn_silu(out, tile_stats=...) against the fp64 GroupNorm of the stored output."""
    from cd360 import ops
    out0, _ = produce(torch.zeros(C, device=DEV))
    std = float(out0.double().std())
    bias = dev(_group_bias(C, G, ratio * std, C + ratio))
    out, st = twice(lambda: produce(bias))
    N, P, _ = out.shape
    slabs = st.shape[1]
    assert st.shape == (N, slabs, C, 2) and P % slabs == 0
    rows = P // slabs
    realised = R.group_ratio(out.cpu(), G)
    assert ratio == 0 or (realised >= 0.7 * ratio).all(), (what, float(realised.min()))
    o = out.double().cpu().view(N, slabs, rows, C)
    s, q, sa = o.sum(2), (o * o).sum(2), o.abs().sum(2)
    std_ = st.double().cpu()
    es, eq = (std_[..., 0] - s).abs() / (rows * R.U32 * sa).clamp_min(1e-300), (std_[..., 1] - q).abs() / (rows * R.U32 * q).clamp_min(1e-300)
    print(f"{what}: slab sums off by {float(es.max()):.3g} / squares {float(eq.max()):.3g} of rows x 2^-24 x sum|x|")
    assert torch.isfinite(std_).all() and float(es.max()) <= 1.0 and float(eq.max()) <= 1.0, (what, float(es.max()), float(eq.max()))
    gamma, beta = R.affine(C)
    for silu in (False, True):
        got = twice(lambda: ops.gn_silu(out, dev(gamma), dev(beta), G, eps, silu, tile_stats=st))
        R.assert_within(got, *R.gn_unit(out.cpu(), gamma, beta, G, eps, silu), f"{what} -> gn_silu(tile_stats) silu {silu}")


@functools.lru_cache(maxsize=None)
def _conv_inputs(N, H, W, Cin, Cout, stride=1):
    from cd360 import ops
    g = R._gen(N, H, W, Cin, Cout, 41)
    x = R.bf16(torch.randn(N * H * W, Cin, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    return dev(x), ops.pack_conv_weight(dev(w))


PRODUCER_RATIOS = (0, 16, 128)


@pytest.mark.parametrize("ratio", PRODUCER_RATIOS)
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 16, 8, 128, 320), (1, 16, 16, 192, 256)])
def test_register_staged_convolution_statistics(N, H, W, Cin, Cout, split, ratio, tune):
    """ops.conv_igemm(want_stats=True) on the register-staged kernel: 160-channel tiles (Cout = 320) and 128-channel tiles (256),
    split K forced on and off"""
    from cd360 import ops
    tune(conv_dma=0, conv_split=split)
    assert ops.conv_route(N, H, W, Cin, Cout).family == "register"
    x, wp = _conv_inputs(N, H, W, Cin, Cout)
    _check_producer(lambda b: ops.conv_igemm(x, wp, b, N, H, W, want_stats=True), Cout, 32, ratio, f"register conv {Cout} split {split} ratio {ratio}")


@pytest.mark.parametrize("ratio", PRODUCER_RATIOS)
@pytest.mark.parametrize("halo", [0, 1])
def test_dma_convolution_statistics(halo, ratio, tune):
    """the LDS-DMA 3 x 3 route with and without the halo form"""
    from cd360 import ops
    N, H, W, Cin, Cout = 3, 16, 8, 64, 320
    tune(conv_dma=-1, conv_cfg=4, conv_halo=halo)
    r = ops.conv_route(N, H, W, Cin, Cout)
    assert r.family == "dma" and r.halo == bool(halo), r
    x, wp = _conv_inputs(N, H, W, Cin, Cout)
    _check_producer(lambda b: ops.conv_igemm(x, wp, b, N, H, W, want_stats=True), Cout, 32, ratio, f"dma conv halo {halo} ratio {ratio}")


@pytest.mark.parametrize("ratio", PRODUCER_RATIOS)
@pytest.mark.parametrize("M,N,K,rows", [(192, 64, 128, 32), (2048, 1280, 128, 64)])
def test_gemm_channel_statistics(M, N, K, rows, ratio, tune):
    """ops.gemm_cstats (proj_out + residual in front of a GroupNorm) at both slab heights"""
    from cd360 import ops
    assert ops._lib.load().cd360_gemm_cstats_rows(M, N) == rows
    g = R._gen(M, N, K, 43)
    a, w = dev(R.bf16(torch.randn(M, K, generator=g))), dev(R.bf16(torch.randn(N, K, generator=g) * K ** -0.5))
    res = dev(R.bf16(torch.randn(M, N, generator=g)))
    P = 64

    def produce(b):
        out, cst = ops.gemm_cstats(a, w, bias=b, res=res)
        assert cst is not None and cst.shape == (M // rows, N, 2)
        return out.view(M // P, P, N), cst.view(M // P, P // rows, N, 2)
    _check_producer(produce, N, 32, ratio, f"gemm_cstats {M}x{N}x{K} ratio {ratio}")


@pytest.mark.parametrize("ratio", PRODUCER_RATIOS)
def test_vae_conv_in_statistics(ratio):
    from cd360 import ops
    B, cz, H, W, cout = 2, 4, 16, 16, 512
    g = R._gen(B, cz, H, W, cout, 47)
    z = dev(torch.randn(B, cz, H, W, generator=g))
    wp = ops.pack_vae_conv_in_weight(dev(torch.randn(cout, cz, 3, 3, generator=g) * (9 * cz) ** -0.5))
    _check_producer(lambda b: ops.vae_conv_in(z, wp, b, want_stats=True), cout, 32, ratio, f"vae_conv_in ratio {ratio}", eps=1e-6)


@pytest.mark.parametrize("ratio", PRODUCER_RATIOS)
def test_vae_downsample_statistics(ratio):
    from cd360 import ops
    N, H, W, C = 1, 32, 32, 128
    assert ops.vae_downsample_stats_rows(N, H, W, C) > 0
    x, wp = _conv_inputs(N, H, W, C, C)
    _check_producer(lambda b: ops.vae_downsample(x.view(N, H * W, C), wp, b, N, H, W, want_stats=True), C, 32, ratio,
                    f"vae_downsample ratio {ratio}", eps=1e-6)


# ------------------------------------------------------------------------------------------------ add_layernorm, row_stats
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("shape,ratio", R.CASES_LN, ids=[f"{s[0]}x{s[1]}-r{r}" for s, r in R.CASES_LN])
def test_add_layernorm_forward_backward_and_row_stats(shape, ratio, with_b):
    rows, C = shape
    a, b, gamma, beta, realised = R.ln_case(rows, C, ratio)
    assert ratio == 0 or (realised >= 0.7 * ratio).all()
    _ln_check(a, b if with_b else None, gamma, beta, f"add_layernorm {shape} ratio {ratio} b {with_b}")
    if not with_b:
        _row_stats_check(a, f"row_stats {shape} ratio {ratio}")


@pytest.mark.parametrize("value", R.CONSTANTS)
@pytest.mark.parametrize("shape", R.LN_SHAPES)
def test_add_layernorm_with_constant_rows(shape, value):
    rows, C = shape
    a, _ = R.constant_rows(rows, C, value)
    gamma, beta = R.affine(C, dtype=torch.bfloat16)
    _ln_check(a, None, gamma, beta, f"add_layernorm {shape} constant {value}")
    _row_stats_check(a, f"row_stats {shape} constant {value}")


def _ln_check(a, b, gamma, beta, what, eps=1e-5):
    from cd360 import ops
    s, ln = twice(lambda: ops.add_layernorm(dev(a), dev(b), dev(gamma), dev(beta), eps))
    R.assert_within(ln, *R.ln_unit(a, b, gamma, beta, eps), what)
    if b is not None:
        want = a.double() + b.double()
        R.assert_within(s, want, want.abs(), what + " (sum)")
    x = a if b is None else s.cpu()
    d_ln = R.group_scaled_noise(1, a.shape[0], a.shape[1], 1)[0]
    d_sum = None if b is None else R.group_scaled_noise(1, a.shape[0], a.shape[1], 1, seed=1)[0]
    dx = twice(lambda: ops.add_layernorm_bwd(dev(x), dev(gamma), dev(d_ln), dev(d_sum), eps))
    R.assert_within(dx, *R.ln_backward_unit(x, gamma, d_ln, d_sum, eps), what + " (gradient)")


def _row_stats_check(a, what):
    """(sum, sum of squares) per row: |delta| <= C 2^-24 sum|x| (sum x^2), the worst case of a sequential fp32 sum"""
    from cd360 import ops
    st = twice(lambda: ops.row_stats(dev(a))).double().cpu()[:, 0]
    x = a.double()
    C = x.shape[1]
    es = (st[:, 0] - x.sum(1)).abs() / (C * R.U32 * x.abs().sum(1)).clamp_min(1e-300)
    eq = (st[:, 1] - (x * x).sum(1)).abs() / (C * R.U32 * (x * x).sum(1)).clamp_min(1e-300)
    assert torch.isfinite(st).all() and float(es.max()) <= 1.0 and float(eq.max()) <= 1.0, (what, float(es.max()), float(eq.max()))


# ------------------------------------------------------------------------------------------------ LayerNorm folded into a Linear
FOLD_CONFIGS = {"default": dict(gemm_cfg=-1), "128x128": dict(gemm_cfg=1), "256x256": dict(gemm_cfg=3), "ksplit": dict(gemm_cfg=4, gemm_ksplit=1)}
FOLD_CASES = [(s, c, False) for s in R.FOLD_SHAPES for c in FOLD_CONFIGS] + [(R.FOLD_SHAPES[2], "default", True)]


@pytest.mark.parametrize("producer", [False, True], ids=["row_stats", "gemm_stats"])
@pytest.mark.parametrize("ratio", R.RATIOS)
@pytest.mark.parametrize("shape,config,geglu", FOLD_CASES, ids=[f"{'x'.join(map(str, s))}-{c}{'-geglu' if g else ''}" for s, c, g in FOLD_CASES])
def test_layernorm_folded_into_gemm(shape, config, geglu, ratio, producer, tune):
    """producer: the rows come out of a GEMM that writes their (sum, sum of squares) per column tile (ln_parts > 1 when K > its tile
    width): an identity weight reproduces the offset rows exactly, so the reference is the same as with row_stats"""
    from cd360 import ops
    M, N, K = shape
    x, (w, b, gamma, beta), realised = R.fold_case(M, N, K, ratio)
    assert ratio == 0 or (realised >= 0.7 * ratio).all()
    wp, wsum, cb = ops.pack_ln_linear(dev(w), dev(b), dev(gamma), dev(beta))
    ref, unit = R.ln_linear_unit(x, wp.cpu(), cb.cpu(), 1e-5)
    xd = dev(x)
    tune(gemm_cfg=-1)
    if producer:
        eye = torch.eye(K, dtype=torch.bfloat16, device=DEV)
        xd2, st = ops.gemm(xd, eye, want_stats=True)
        assert torch.equal(xd2, xd) and st.shape[1] == -(-K // ops.gemm_tile_n(M, K))
        xd = xd2
    else:
        st = ops.row_stats(xd)
    kw = {}
    if geglu:
        perm = ops.geglu_row_order(N // 2, DEV)
        wp, wsum, cb = wp[perm].contiguous(), wsum[perm].contiguous(), cb[perm].contiguous()
        kw["geglu"] = True
        ref, unit = R.gelu_gate(ref, unit)
    tune(**FOLD_CONFIGS[config])
    got = twice(lambda: ops.gemm(xd, wp, bias=cb, ln=(st, wsum, 1e-5), **kw))
    R.assert_within(got, ref, unit, f"gemm(ln) {shape} {config} geglu {geglu} ratio {ratio} parts {st.shape[1]}")
