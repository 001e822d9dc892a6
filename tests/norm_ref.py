"""fp64 references, ill-conditioned inputs and a conditioning-aware error bound for the normalisation kernels.

The GroupNorm (csrc/gn_silu.hip), the stand-alone LayerNorm (csrc/elementwise.hip) and the LayerNorm folded in front of a Linear
(csrc/gemm8p.hip) take bf16 activations and compute in fp32.  Everything here is plain torch float64 on the CPU and takes the
bf16-rounded values the kernels see, so what a test measures is the kernel's own arithmetic.

Inputs: unit-variance noise on top of a per-group (per-row) constant `ratio` times as large -- the case in which a one-pass
E[x^2] - mean^2 variance cancels --, groups (rows) that hold one constant, and group scales spread over 2^-6 .. 2^6 inside one image.

Bound: for an output y = act(gamma (x - mu) r + beta), with mu and r = 1 / sqrt(var + eps) in fp64,

    |got - ref| <= 2^-8 |ref| + K 2^-24 unit,      unit = |gamma| (|x| + |mu|) r + |gamma (x - mu) r| + |ref|    (x 1.1 under SiLU),

i.e. one bf16 store plus K fp32 roundings of the quantities any fp32 evaluation of x - mu has to form: the first term of `unit` is
what ONE fp32 rounding of x or of mu does to the output, so the bound widens with |mean| / std exactly as fast as a correct fp32
kernel's error may -- linearly -- and not as fast as a one-pass variance's error does -- quadratically.  The gradient and the folded
Linear get the same construction from their own formulas (gn_backward, ln_linear).

K is NOT taken from the HIP kernels: tests/test_norm_stats_cpu.py measures torch's own fp32 CPU group_norm / layer_norm (outputs kept
in fp32) against `unit` over the whole case list below, and K is 8 times the worst ratio it finds (the margin is for another summation
order)."""
import functools

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24   # fp32 unit roundoff
UBF = 2.0 ** -8    # bf16 unit roundoff (the store)
# worst |fp32 torch - fp64| / (2^-24 unit) over every case of CASES_GN / CASES_LN / CASES_FOLD, forward and gradient
# (tests/test_norm_stats_cpu.py::test_fp32_torch_reference_sits_inside_the_bound prints and pins it), and K = 8 x that, rounded up
K_MEASURED = 12.0  # measured 11.81 (LayerNorm, 257 x 1280, ratio 0); GroupNorm 6.1, its gradient 3.6, LayerNorm gradient 7.9, folded Linear 3.1
K = 96.0

RATIOS = (0, 4, 16, 64, 128)   # 128: the last ratio at which bf16 inputs still carry a signal (std = 2 ulp of the mean)
CONSTANTS = (0.0, 1.0, -37.25, 240.0)  # exact in bf16
EPS = (1e-5, 1e-6)

# (N, P, C, G): channels per group 2, 10, 16, 30, 80, 4, 8; C / 8 > 256 (the `wide` branch); ragged slabs (P = 100); one slab (P = 16)
GN_SHAPES = [(2, 64, 64, 32), (2, 100, 320, 32), (1, 256, 512, 32), (2, 256, 960, 32), (1, 64, 2560, 32), (1, 1024, 128, 32), (2, 16, 64, 8)]
GN_BWD_SHAPES = GN_SHAPES[:3] + [(1, 64, 2560, 32)]
LN_SHAPES = [(37, 64), (130, 640), (5, 2048), (257, 1280)]
FOLD_SHAPES = [(300, 272, 192), (256, 256, 64), (512, 768, 320), (256, 1280, 1280)]  # (M, N, K)
CASES_GN = [(s, r) for s in GN_SHAPES[:3] for r in RATIOS] + [(s, 64) for s in GN_SHAPES[3:]]
CASES_LN = [(s, r) for s in LN_SHAPES for r in RATIOS]
CASES_FOLD = [(s, r) for s in FOLD_SHAPES for r in RATIOS]


def _gen(*seed):
    """a generator seeded by an arithmetic mix of the numbers given (no hash(): the same inputs on every interpreter)"""
    h = 17
    for s in seed:
        h = (h * 1000003 + (int(s * 64) if isinstance(s, float) else int(s))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def bf16(t):
    return t.to(torch.bfloat16)


def bfr(t):
    """round to bf16, keep the dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def _offsets(shape, ratio, g):
    mag = ratio * (1.0 + 0.25 * torch.rand(shape, generator=g, dtype=torch.float64))
    return mag * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def group_ratio(x, G):
    """x [N, P, C] -> realised |mean| / std per (image, group), [N, G] fp64 (inf for a constant non-zero group, 0 for a zero one)"""
    N, P, C = x.shape
    v = x.double().view(N, P, G, C // G).permute(0, 2, 1, 3).reshape(N, G, -1)
    m, s = v.mean(-1).abs(), v.std(-1, unbiased=False)
    return torch.where(s > 0, m / s, torch.where(m > 0, torch.full_like(m, float("inf")), torch.zeros_like(m)))


def row_ratio(x):
    return group_ratio(x.reshape(x.shape[0], 1, x.shape[-1]), 1)[:, 0]


def offset_groups(N, P, C, G, ratio, seed=0):
    """unit-variance noise + a constant per (image, group) of magnitude ratio (1 .. 1.25), random sign -> (x bf16 [N, P, C], realised
    |mean| / std [N, G])"""
    g = _gen(N, P, C, G, ratio, seed)
    x = torch.randn(N, P, C, generator=g, dtype=torch.float64)
    x = bf16(x + _offsets((N, 1, G, 1), ratio, g).expand(N, P, G, C // G).reshape(N, P, C))
    return x, group_ratio(x, G)


def offset_rows(rows, C, ratio, seed=0):
    g = _gen(rows, C, ratio, seed, 7)
    x = bf16(torch.randn(rows, C, generator=g, dtype=torch.float64) + _offsets((rows, 1), ratio, g))
    return x, row_ratio(x)


def constant_groups(N, P, C, G, value, seed=0, every=3):
    """noise, but every `every`-th (image, group) holds `value` everywhere -> (x bf16, mask [N, G] of the constant groups)"""
    g = _gen(N, P, C, G, value, seed, 11)
    x = torch.randn(N, P, G, C // G, generator=g, dtype=torch.float64)
    mask = (torch.arange(N * G).view(N, G) % every) == 0
    x = torch.where(mask[:, None, :, None], torch.full_like(x, value), x)
    return bf16(x.reshape(N, P, C)), mask


def constant_rows(rows, C, value, seed=0, every=3):
    g = _gen(rows, C, value, seed, 13)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64)
    mask = (torch.arange(rows) % every) == 0
    return bf16(torch.where(mask[:, None], torch.full_like(x, value), x)), mask


def wide_range(N, P, C, G, seed=0):
    """group scales 2^-6 .. 2^6 within one image (a metric normalised by the tensor's maximum sees the largest group only), each group
    with an offset of 8 standard deviations -> (x bf16, scale [G])"""
    g = _gen(N, P, C, G, seed, 17)
    scale = 2.0 ** (torch.arange(G, dtype=torch.float64) * 12.0 / (G - 1) - 6.0)[torch.randperm(G, generator=g)]
    x = torch.randn(N, P, G, C // G, generator=g, dtype=torch.float64) + _offsets((N, 1, G, 1), 8, g)
    return bf16((x * scale[None, None, :, None]).reshape(N, P, C)), scale


def affine(C, seed=0, dtype=torch.float32):
    """gamma around 1 with both signs of deviation, beta of a few tenths; in `dtype` (the kernel's), returned as that dtype"""
    g = _gen(C, seed, 19)
    return (1 + 0.3 * torch.randn(C, generator=g)).to(dtype), (0.3 * torch.randn(C, generator=g)).to(dtype)


def group_scaled_noise(N, P, C, G, seed=0):
    """a cotangent: unit noise times a per-group factor over 2^-4 .. 2^4, bf16"""
    g = _gen(N, P, C, G, seed, 23)
    s = 2.0 ** (torch.rand(N, 1, G, 1, generator=g, dtype=torch.float64) * 8 - 4)
    return bf16((torch.randn(N, P, G, C // G, generator=g, dtype=torch.float64) * s).reshape(N, P, C))


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def _gstats(x, G, eps):
    N, P, C = x.shape
    v = x.view(N, P, G, C // G)
    mu = v.mean((1, 3), keepdim=True)
    var = ((v - mu) ** 2).mean((1, 3), keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    return mu.expand_as(v).reshape(N, P, C), r.expand_as(v).reshape(N, P, C)


def _gmean(t, G):
    N, P, C = t.shape
    return t.view(N, P, G, C // G).mean((1, 3), keepdim=True).expand(N, P, G, C // G).reshape(N, P, C)


def gn_forward(x, gamma, beta, G, eps, silu, dtype=torch.float64):
    """x [N, P, C] (bf16-valued), gamma / beta [C] -> GroupNorm (+ SiLU) in `dtype` through torch's group_norm, [N, P, C]"""
    y = F.group_norm(x.to(dtype).transpose(1, 2), G, gamma.to(dtype), beta.to(dtype), eps).transpose(1, 2)
    return F.silu(y) if silu else y


def gn_unit(x, gamma, beta, G, eps, silu):
    """the fp64 reference and the error unit of the bound, [N, P, C] each"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mu, r = _gstats(x, G, eps)
    ref = gn_forward(x, gamma, beta, G, eps, silu)
    unit = gamma.abs() * (x.abs() + mu.abs()) * r + (gamma * (x - mu) * r).abs() + ref.abs()
    return ref, unit * (1.1 if silu else 1.0)


def gn_backward(x, dy, gamma, beta, G, eps, silu, dtype=torch.float64):
    """input gradient of gn_forward through autograd in `dtype`"""
    xx = x.to(dtype).clone().requires_grad_(True)
    gn_forward(xx, gamma, beta, G, eps, silu, dtype).backward(dy.to(dtype))
    return xx.grad


def _silu_d(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def gn_backward_unit(x, dy, gamma, beta, G, eps, silu):
    """dx = r (gh - m1 - xh m2), gh = dy act'(z) gamma, m1 = mean_g gh, m2 = mean_g (gh xh) (csrc/gn_silu.hip).  unit: the magnitudes
    of the three terms with the means taken over absolute values (an fp32 sum's error scales with the sum of magnitudes), plus what one
    fp32 rounding of x or mu -- e = (|x| + |mu|) r on xh -- does through xh m2, through mean_g(gh xh) and, under SiLU, through
    act'(z) (|act''| <= 1/2); plus |ref|."""
    x, dy, gamma, beta = x.double(), dy.double(), gamma.double(), beta.double()
    mu, r = _gstats(x, G, eps)
    xh = (x - mu) * r
    gh = dy * gamma
    e = (x.abs() + mu.abs()) * r
    d_gh = torch.zeros_like(gh)
    if silu:
        d_gh = 0.5 * (gh * gamma).abs() * e
        gh = gh * _silu_d(xh * gamma + beta)
    m2 = _gmean(gh * xh, G)
    ref = gn_backward(x, dy, gamma, beta, G, eps, silu)
    unit = r * (gh.abs() + _gmean(gh.abs(), G) + xh.abs() * _gmean((gh * xh).abs(), G)
                + e * m2.abs() + xh.abs() * _gmean(gh.abs() * e, G) + d_gh + _gmean(d_gh, G) + xh.abs() * _gmean(d_gh * xh.abs(), G)) + ref.abs()
    return ref, unit * (1.1 if silu else 1.0)


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def ln_forward(a, b, gamma, beta, eps, dtype=torch.float64):
    """LayerNorm(a + b) * gamma + beta over the last dim (b may be None)"""
    s = a.to(dtype) if b is None else a.to(dtype) + b.to(dtype)
    return F.layer_norm(s, (s.shape[-1],), gamma.to(dtype), beta.to(dtype), eps)


def ln_unit(a, b, gamma, beta, eps):
    s = a.double() if b is None else a.double() + b.double()
    ref, unit = gn_unit(s[:, None, :], gamma, beta, 1, eps, False)
    return ref[:, 0], unit[:, 0]


def ln_backward(x, gamma, d_ln, d_sum, eps, dtype=torch.float64):
    """gradient with respect to x = a + b of LayerNorm(x) * gamma (cotangent d_ln) plus the residual stream's own gradient d_sum"""
    xx = x.to(dtype).clone().requires_grad_(True)
    F.layer_norm(xx, (xx.shape[-1],), gamma.to(dtype), None, eps).backward(d_ln.to(dtype))
    return xx.grad if d_sum is None else xx.grad + d_sum.to(dtype)


def ln_backward_unit(x, gamma, d_ln, d_sum, eps):
    ref, unit = gn_backward_unit(x[:, None, :], d_ln[:, None, :], gamma, torch.zeros_like(gamma), 1, eps, False)
    ref, unit = ref[:, 0], unit[:, 0]
    if d_sum is not None:
        unit = unit - ref.abs() + d_sum.double().abs() + (ref + d_sum.double()).abs()
        ref = ref + d_sum.double()
    return ref, unit


# ------------------------------------------------------------------------------------------------------------------ LayerNorm -> Linear
def ln_linear(x, wp, cb, eps, dtype=torch.float64):
    """linear(layer_norm(x), wp, cb) with wp = the PACKED bf16 weight gamma o W and cb = W beta + b (ops.pack_ln_linear): the weight
    rounding is the kernel's, not counted as its error"""
    return F.linear(F.layer_norm(x.to(dtype), (x.shape[-1],), None, None, eps), wp.to(dtype), cb.to(dtype))


def ln_linear_unit(x, wp, cb, eps):
    """out_j = r (sum_k x_k w_jk - mu wsum_j) + cb_j: unit = r sum_k |x_k w_jk| + |mu wsum_j r| + |ref|"""
    x, wp, cb = x.double(), wp.double(), cb.double()
    mu = x.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    ref = ln_linear(x, wp, cb, eps)
    unit = r * (x.abs() @ wp.abs().t()) + (mu * r).abs() * wp.sum(1).abs()[None, :] + ref.abs()
    return ref, unit


def fold_weights(N, K, seed=0):
    """a Linear [N, K] behind a LayerNorm(gamma, beta): fp32 weight, bias, gamma, beta"""
    g = _gen(N, K, seed, 29)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    return w, 0.2 * torch.randn(N, generator=g), 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)


def gelu_gate(ref, unit):
    """GEGLU of [.., 2 I] (value | gate): value gelu(gate); |gelu| <= |g|, |gelu'| <= 1.13"""
    i = ref.shape[-1] // 2
    v, g = ref[..., :i], ref[..., i:]
    return v * F.gelu(g), unit[..., :i] * F.gelu(g).abs() + 1.13 * unit[..., i:] * v.abs() + (v * F.gelu(g)).abs()


# ------------------------------------------------------------------------------------------------------------------ the bound
def excess(got, ref, unit, store=UBF):
    """per element (|got - ref| - store |ref|) / (2^-24 unit): how many fp32 roundings of `unit` the error needs beyond the store's
    rounding.  A test asserts excess <= K (fp32 outputs: store = 0).  Elements with unit == 0 must be exact."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    err = (got - ref).abs() - store * ref.abs()
    return torch.where(unit > 0, err / (U32 * unit.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def assert_within(got, ref, unit, what, k=None, store=UBF):
    k = K if k is None else k
    g = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    ex = excess(g, ref, unit, store)
    worst = float(ex.max())
    print(f"{what}: worst error {worst:.3g} x 2^-24 unit beyond the bf16 store (K = {k})")
    if worst > k:
        i = int(ex.argmax())
        bad = int((ex > k).sum())
        raise AssertionError(f"{what}: {bad} of {ex.numel()} elements outside the bound, worst {worst:.4g} > K = {k} at flat index {i}: got "
                             f"{g.reshape(-1)[i].item():.8g} ref {ref.reshape(-1)[i].item():.8g} unit {unit.reshape(-1)[i].item():.4g}")
    return worst


@functools.lru_cache(maxsize=None)
def gn_case(N, P, C, G, ratio):
    x, realised = offset_groups(N, P, C, G, ratio)
    gamma, beta = affine(C)
    return x, gamma, beta, realised


@functools.lru_cache(maxsize=None)
def ln_case(rows, C, ratio):
    a, realised = offset_rows(rows, C, ratio)
    g = _gen(rows, C, ratio, 31)
    b = bf16(torch.randn(rows, C, generator=g))
    gamma, beta = affine(C, dtype=torch.bfloat16)
    return a, b, gamma, beta, realised


@functools.lru_cache(maxsize=None)
def fold_case(M, N, K, ratio):
    """-> x bf16 [M, K], (w, b, gamma, beta) fp32"""
    x, realised = offset_rows(M, K, ratio, seed=N)
    return x, fold_weights(N, K), realised


def pack_ln_linear_cpu(w, b, gamma, beta):
    """ops.pack_ln_linear on the CPU: (w' bf16 = w gamma, wsum of the rounded w', cb = w beta + b)"""
    wp = bf16(w.float() * gamma.float()[None, :])
    return wp, wp.float().sum(1), w.float() @ beta.float() + b.float()


def onepass_group_norm_fp32(x, gamma, beta, G, eps):
    """what the bound must catch: GroupNorm with var = E[x^2] - mean^2 from fp32 sums (an emulation, not any kernel's summation order)"""
    N, P, C = x.shape
    v = x.float().view(N, P, G, C // G)
    n = float(P * (C // G))
    mean = v.sum((1, 3), keepdim=True, dtype=torch.float32) / n
    var = ((v * v).sum((1, 3), keepdim=True, dtype=torch.float32) / n - mean * mean).clamp_min(0)
    y = (v - mean) * (1.0 / torch.sqrt(var + eps))
    return y.reshape(N, P, C) * gamma.float() + beta.float()
