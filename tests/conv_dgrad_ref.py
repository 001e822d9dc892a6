"""The reference side of the convolution data-gradient tests: shapes, inputs, the fp64 autograd reference and the impulse expectations.

Plain torch on the host, no library: tests/test_conv_dgrad_cpu.py holds these helpers (and the bar) to the recipe of
cd360.grad.ConvIgemmFn.backward written out in fp32, tests/test_conv_dgrad_gpu.py holds the kernels to them.

The product computes dx of a frozen convolution by launching cd360_conv_igemm_bf16 on dy with the weight of
sgm...util.packed_conv_dgrad (taps flipped, channels transposed, both channel counts re-padded; dy zero-inserted for stride 2) and slicing
the result back to cin.  The reference is torch.autograd.grad through F.conv2d in fp64, which shares none of that."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conv_shapes import dgrad_channels
from test_conv_routes_gpu import NEEDS_320, SLAB_OF_TILING, bfr, halo_fits  # (that module needs no GPU to import)

# Forward shapes (N, H, W, cin, cout, stride), 3 x 3 / pad 1, chosen for what their GRADIENT launch (N, H, W, Cin', Cout') exercises;
# non-square throughout, so that H and W cannot be exchanged unnoticed.
SMALL_3X3 = [
    (2, 16, 8, 960, 64, 1),    # Cout' = 960 (3.75 tiles of 256, three of 320), one 64-channel K chunk
    (2, 16, 8, 1920, 128, 1),  # Cout' = 1920 (7.5 tiles of 256, six of 320)
    (1, 8, 16, 1920, 128, 1),
    (2, 16, 8, 2560, 64, 1),   # Cout' = 2560 (eight tiles of 320)
    (1, 8, 16, 2560, 64, 1),
    (2, 4, 32, 1920, 640, 1),  # K' = 9 * 640 >= 3072: the K-split wave arrangement, at Cout' = 1920
    (2, 9, 7, 960, 128, 1),    # 63-pixel images: no whole slab of any tiling
    (3, 16, 8, 320, 48, 1),    # cout 48 -> Cin' 64 with sixteen zero channels
    (3, 16, 8, 320, 4, 1),     # the output convolution: cout 4 -> 16 (the output slice [..., :4]) -> Cin' 64
    (1, 8, 16, 4, 320, 1),     # the input convolution: cin 4 -> Cout' 64, dx sliced [..., :4]
    (2, 16, 8, 128, 128, 2),   # Downsample.op: dy zero-inserted from 8 x 4 to 16 x 8
    (1, 8, 12, 128, 160, 2),   # ... from 4 x 6 to 8 x 12 (96-pixel images)
]
SMALL_1X1 = [(2, 16, 8, 960, 320, 1), (2, 16, 8, 1920, 640, 1)]  # the skip connections: the GEMM entry with N' = 960 and 1920
# The default route of each shape's gradient launch, as cd360_conv_route of the built library answers on the host
# (tests/test_conv_dgrad_cpu.py pins it): forward shape + (k,) -> (family, tiling, halo form, slab rows)
SMALL_DEFAULT_ROUTES = {
    (2, 16, 8, 960, 64, 1, 3): ("dma", 4, True, 64),      # launch (2, 16, 8, 64, 960)
    (2, 16, 8, 1920, 128, 1, 3): ("dma", 4, True, 64),    # launch (2, 16, 8, 128, 1920)
    (1, 8, 16, 1920, 128, 1, 3): ("dma", 2, False, 64),   # launch (1, 8, 16, 128, 1920)
    (2, 16, 8, 2560, 64, 1, 3): ("dma", 4, True, 64),     # launch (2, 16, 8, 64, 2560)
    (1, 8, 16, 2560, 64, 1, 3): ("dma", 2, False, 64),    # launch (1, 8, 16, 64, 2560)
    (2, 4, 32, 1920, 640, 1, 3): ("dma", 4, True, 64),    # launch (2, 4, 32, 640, 1920)
    (2, 9, 7, 960, 128, 1, 3): ("register", 0, False, 0),  # launch (2, 9, 7, 128, 960): the dispatcher keeps images that are not whole slabs
                                                           # off the LDS-DMA core
    (3, 16, 8, 320, 48, 1, 3): ("dma", 4, True, 64),      # launch (3, 16, 8, 64, 320)
    (3, 16, 8, 320, 4, 1, 3): ("dma", 4, True, 64),       # launch (3, 16, 8, 64, 320)
    (1, 8, 16, 4, 320, 1, 3): ("dma", 2, False, 64),      # launch (1, 8, 16, 320, 64)
    (2, 16, 8, 128, 128, 2, 3): ("dma", 4, True, 64),     # launch (2, 16, 8, 128, 128)
    (1, 8, 12, 128, 160, 2, 3): ("register", 0, False, 0),  # launch (1, 8, 12, 192, 128): 96-pixel images
    (2, 16, 8, 960, 320, 1, 1): ("gemm", 0, False, 0),    # launch (2, 16, 8, 320, 960)
    (2, 16, 8, 1920, 640, 1, 1): ("gemm", 0, False, 0),   # launch (2, 16, 8, 640, 1920)
}


def with_extras(cout):
    """emb and res join the case wherever conv_tokens takes them (not with a padded output channel count)"""
    return cout % 16 == 0


def dgrad_launch(N, H, W, cin, cout, stride=1):
    """(N, H, W, Cin', Cout') of the gradient launch: stride 1 at the forward input's size, channels as packed_conv_dgrad pads them"""
    return (N, H, W) + dgrad_channels(cin, cout)


def forced_route_mismatch(r, launch, cfg, halo):
    """None when `r`, the route query's answer for the gradient `launch` (N, H, W, Cin', Cout') under forced (conv_cfg, conv_halo), is the
    route the case is named for; else the reason why the shape cannot take it (checked to be a genuine one)."""
    N, H, W, ci, co = launch
    if r.family != "dma":
        assert r.family == "register" and (H * W) % 128, r  # (every slab size divides 128)
        return f"{H * W}-pixel images are not whole slabs: the dispatcher gives the register-staged kernel"
    if cfg > 0 and r.tiling != cfg:
        assert cfg in NEEDS_320 and co % 320, (cfg, r)
        return f"tiling {cfg} needs Cout' % 320 == 0 (Cout' = {co})"
    if halo == 1 and not r.halo:
        assert not halo_fits(N, H, W, ci), r
        return f"the halo form does not fit {H} x {W} images"
    assert r.halo == (halo == 1 or (halo == -1 and r.tiling == 4 and halo_fits(N, H, W, ci))), r
    assert r.slab_rows == (64 if r.halo else SLAB_OF_TILING[r.tiling]), r
    return None


def _img(t, N, H, W):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _tok(t):
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], t.shape[2] * t.shape[3], t.shape[1])


def autograd_reference(x, w, bias, emb, res, dy, N, H, W, stride):
    """fp64 tokens x [N, H W, cin], w [cout, cin, k, k], bias [cout] | None, emb [N, cout] | None, res / dy [N, Ho Wo, cout] ->
    (y, dx, d_emb, d_res) of y = conv2d(x, w, bias, stride, pad k // 2) + emb[n] + res through torch.autograd.grad"""
    k = w.shape[-1]
    leaves = [x.clone().requires_grad_(True)] + [t.clone().requires_grad_(True) for t in (emb, res) if t is not None]
    y = _tok(F.conv2d(_img(leaves[0], N, H, W), w, bias, stride=stride, padding=k // 2))
    if emb is not None:
        y = y + leaves[1][:, None, :] + leaves[2]
    grads = torch.autograd.grad(y, leaves, dy)
    return (y.detach(), grads[0]) + (tuple(grads[1:]) if emb is not None else (None, None))


@functools.lru_cache(maxsize=2)
def case(N, H, W, cin, cout, stride, k=3):
    """bf16-valued fp64 inputs of one shape and its references, computed once: x, w, bias, emb, res, dy; y / A_y (forward and the same
    sum over absolute values), dx / A (data gradient; A = the same gradient with |w| and |dy|), d_emb / A_emb, d_res."""
    g = torch.Generator().manual_seed(N * 1000 + H * 31 + W + cin * 7 + cout + stride * 100000 + k)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    ho, wo = H // stride, W // stride
    c = SimpleNamespace(shape=(N, H, W, cin, cout, stride, k))
    c.x = bfr(rnd(N, H * W, cin))
    c.w = bfr(rnd(cout, cin, k, k) / math.sqrt(k * k * cin))
    c.bias = bfr(rnd(cout) * 0.1)
    extras = with_extras(cout)
    c.emb = bfr(rnd(N, cout)) if extras else None
    c.res = bfr(rnd(N, ho * wo, cout)) if extras else None
    c.dy = bfr(rnd(N, ho * wo, cout))
    c.y, c.dx, c.d_emb, c.d_res = autograd_reference(c.x, c.w, c.bias, c.emb, c.res, c.dy, N, H, W, stride)
    ab = lambda t: None if t is None else t.abs()  # noqa: E731
    c.A_y, c.A, c.A_emb, _ = autograd_reference(c.x.abs(), c.w.abs(), c.bias.abs(), ab(c.emb), ab(c.res), c.dy.abs(), N, H, W, stride)
    if not extras:
        c.A_emb = None
    return c


def recipe_dx(w, dy, N, H, W, stride, dtype=torch.float32):
    """ConvIgemmFn.backward + packed_conv_dgrad as plain torch in `dtype`: taps flipped, channels transposed, Cout padded to 16 then 64 as
    the input channels, Cin padded to 64 as the output channels, dy zero-inserted for stride 2, one stride-1 convolution, the slice back
    to cin.  w [cout, cin, k, k], dy [N, Ho Wo, cout] -> dx [N, H W, cin] (not yet rounded)."""
    cout, cin, k, _ = w.shape
    cin_d, cout_d = dgrad_channels(cin, cout)
    wd = F.pad(w.flip(2, 3).transpose(0, 1), (0, 0, 0, 0, 0, cin_d - cout, 0, cout_d - cin)).to(dtype)  # [Cout', Cin', k, k]
    g = dy.reshape(N, H // stride, W // stride, cout)
    if stride == 2:
        z = torch.zeros(N, H, W, cout, dtype=dy.dtype)
        z[:, ::2, ::2] = g
        g = z
    g = F.pad(g, (0, cin_d - cout)).to(dtype)
    return _tok(F.conv2d(g.permute(0, 3, 1, 2), wd, None, stride=1, padding=k // 2))[..., :cin]


# ------------------------------------------------------------------------------------------------ impulse responses
IMPULSE_SHAPES = [(2, 8, 16, 128, 64, 1), (2, 16, 8, 128, 128, 2)]  # forward (N, H, W, cin, cout, stride): H != W


def impulse_weight(cout, cin):
    """A 3 x 3 weight without symmetry, every value exact in bf16: 8-bit integer significands 128 .. 255 (one per input channel), one
    binary exponent per tap, shifted by nine per output channel, the sign alternating with ci + co.  More than 2^16 values cannot all
    differ in bf16: within an output channel all 9 * cin values differ in magnitude, between output channels less than 13 apart every value
    differs, and further apart the significands are permuted (an odd multiplier per group of 13)."""
    co, ci, tap = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(9), indexing="ij")
    sig = 128 + (ci * (2 * (co // 13) + 1)) % 128
    w = sig.double() * torch.exp2((tap + 9 * (co % 13) - 60).double()) * (1 - 2 * ((ci + co) % 2)).double()
    assert torch.equal(bfr(w), w)
    return w.reshape(cout, cin, 3, 3)


def impulse_positions(ho, wo):
    """(yo, xo) in the output image: the four corners, one pixel on each edge, one in the interior"""
    return [(0, 0), (0, wo - 1), (ho - 1, 0), (ho - 1, wo - 1), (0, wo // 2), (ho - 1, 1), (ho // 2, 0), (1, wo - 1), (ho // 2, wo // 2 - 1)]


def impulse_channel(i, cout):
    return (7 + 13 * i) % cout  # a different output channel at every position, spread over the channel tile


def impulse_dy(N, ho, wo, cout, n, yo, xo, co):
    dy = torch.zeros(N, ho, wo, cout, dtype=torch.float64)
    dy[n, yo, xo, co] = 1.0
    return dy.reshape(N, ho * wo, cout)


def impulse_expected(w, N, H, W, stride, n, yo, xo, co):
    """dx [N, H W, cin] of the one-hot dy: output pixel (yo, xo) read input pixel (stride yo + ky - 1, stride xo + kx - 1) through
    w[co, :, ky, kx], so that input pixel's gradient is that weight slice -- where it lies inside the image; everything else is zero."""
    dx = torch.zeros(N, H, W, w.shape[1], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            yi, xi = stride * yo + ky - 1, stride * xo + kx - 1
            if 0 <= yi < H and 0 <= xi < W:
                dx[n, yi, xi] = w[co, :, ky, kx]
    return dx.reshape(N, H * W, -1)
