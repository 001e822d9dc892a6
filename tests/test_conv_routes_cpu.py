"""The route contract of the convolution entry points, checked on the host (the dispatch decision needs no GPU).

cd360_conv_igemm_bf16 serves a 3 x 3 / stride 1 convolution with one of seven kernels of the LDS-DMA core: six tilings (cd360_tuning.conv_cfg)
or the halo form (conv_halo).  Each writes its GroupNorm statistics in slabs of NMB * 32 pixels, and the caller sizes `tile_stats` from
cd360_conv_stats_rows before the launch.  A query that names another kernel than the one that runs sizes the buffer wrongly: too small is
a write past the allocation, too large leaves slabs unwritten.  cd360_conv_route reports the decision the launch takes; this file holds
it, cd360_conv_dma_slab_rows and cd360_conv_stats_rows to the kernels' templates over the tuning space and the product shapes."""
import ctypes
import itertools

import pytest

from conv_shapes import (BATCHES, DGRAD_BATCHES, DGRAD_SCALES, UNET_3X3, UNET_DGRAD, UNET_ROUTES, UNET_UP2X, UNET_UP2X_TILINGS, VAE_3X3,
                         VAE_UP2X)

# pixels per statistics slab = 32 * the NMB template argument of each tiling's kernel (csrc/gemm8p.hip: launch_conv, launch_128x4)
SLAB_OF_TILING = {1: 64, 2: 64, 3: 128, 4: 64, 5: 64, 6: 32}
HALO_SLAB = 64  # launch_128x4: NMB = 2 in every wave arrangement
NEEDS_320 = (1, 5, 6)  # the 320-channel tilings

# (N, H, W, Cin, Cout): the product's convolutions (tests/conv_shapes.py) at the bench batches and the fine-tune step's 24 views
UNET = [(n, h, h, cin, cout) for n in BATCHES + (24,) for h, cin, cout, _ in UNET_3X3]
VAE = [(1, h, h, cin, cout) for h, cin, cout, _, _ in VAE_3X3]
EDGES = [(2, 9, 7, 128, 320), (3, 16, 8, 64, 320), (1, 16, 16, 64, 48), (2, 16, 24, 192, 1280), (2, 32, 32, 1280, 256), (1, 64, 64, 640, 80),
         (2, 8, 16, 192, 128), (1, 8, 8, 64, 640), (2, 4, 32, 384, 320), (1, 2, 64, 64, 640), (1, 16, 16, 64, 80), (24, 32, 32, 1280, 1280),
         (1, 1, 1, 64, 16), (3, 10, 10, 64, 320), (1, 8, 8, 32, 64)]
# the data-gradient launches of the same convolutions (cd360.grad.ConvIgemmFn: channel counts swapped, Cout' up to 2560), both latent sizes
DGRAD = sorted({(n, h // sc, h // sc, ci, co) for n in DGRAD_BATCHES for sc in DGRAD_SCALES for h, ci, co, taps, _ in UNET_DGRAD if taps == 9})
SHAPES = UNET + VAE + EDGES + [s for s in DGRAD if s not in UNET]


def halo_fits(N, H, W, Cin):
    """The halo form's geometry (gemm8p.hip: conv_halo_ok): image rows dividing the 128-pixel tile, whole tiles per image, a halo image of
    at most nine 32-row pieces."""
    return W >= 8 and 128 % W == 0 and (H * W) % 128 == 0 and (128 // W + 2) * (W + 2) <= 9 * 32 and Cin >= 64


def dma_fits(N, H, W, Cin, Cout):
    return Cin % 64 == 0 and Cout % 16 == 0 and N * H * W * Cin * 2 < 2 ** 31 and (Cout + 320) * 9 * Cin * 2 < 2 ** 32


@pytest.fixture
def lib():
    from cd360 import _lib
    return _lib.load()


def decode(route):
    from cd360.ops import decode_conv_route
    return decode_conv_route(route)


def route_of(lib, *shape, taps=9, stride=1):
    return decode(lib.cd360_conv_route(*shape, taps, stride))


def test_the_halo_form_reports_its_own_64_row_slabs(lib, tune):
    """The defect this file was written for: with conv_halo = 1 the halo form serves every shape it fits, whatever the tiling, but the
    slab query answered with the TILING's slab size -- 128 under tiling 3 (the kernel then wrote 64-row slabs into a buffer sized for
    half as many: a write past the allocation) and 32 under tiling 6 (half of the promised slabs never written)."""
    for cfg, shape in ((3, (24, 32, 32, 1280, 1280)), (3, (3, 64, 64, 640, 640)), (6, (3, 32, 32, 1280, 1280)), (6, (2, 16, 8, 64, 320))):
        tune(conv_halo=1, conv_cfg=cfg, conv_dma=-1)
        assert lib.cd360_conv_dma_slab_rows(*shape, 9, 1) == HALO_SLAB, (cfg, shape)
        assert lib.cd360_conv_stats_rows(*shape, 9, 1) == HALO_SLAB, (cfg, shape)


@pytest.mark.parametrize("dma", [-1, 0])
@pytest.mark.parametrize("halo", [-1, 0, 1])
@pytest.mark.parametrize("cfg", [-1, 1, 2, 3, 4, 5, 6])
def test_route_slab_rows_and_stats_rows_agree_with_the_kernel_that_runs(cfg, halo, dma, lib, tune):
    tune(conv_cfg=-1, conv_halo=halo, conv_dma=dma)
    fallback = {s: route_of(lib, *s).tiling for s in SHAPES}  # the measured default tiling of each shape (same halo / dma setting)
    tune(conv_cfg=cfg)
    for s in SHAPES:
        N, H, W, Cin, Cout = s
        r = route_of(lib, *s)
        rows = lib.cd360_conv_dma_slab_rows(*s, 9, 1)
        if dma == 0 or not dma_fits(*s):
            assert r.family == "register" and rows == 0, (s, r)
        else:
            if r.family == "register":  # the DMA core is only taken when every image is a whole number of its slabs
                assert rows == 0 and (H * W) % 128, (s, r)  # (every slab size divides 128)
                t = cfg if cfg > 0 and not (cfg in NEEDS_320 and Cout % 320) else None
                if t is not None:
                    halo_taken = halo_fits(N, H, W, Cin) and (halo == 1 or (halo == -1 and t == 4))
                    assert (H * W) % (HALO_SLAB if halo_taken else SLAB_OF_TILING[t]), (s, r, t)
            else:
                assert r.family == "dma", (s, r)
                if cfg > 0 and not (cfg in NEEDS_320 and Cout % 320):
                    assert r.tiling == cfg, (s, r)  # a forced tiling the shape can take is the tiling that runs
                elif fallback[s]:
                    assert r.tiling == fallback[s], (s, r)  # an ineligible forced tiling falls back to the measured default
                else:
                    assert r.tiling in SLAB_OF_TILING
                if cfg in NEEDS_320 and Cout % 320:
                    assert r.tiling not in NEEDS_320, (s, r)
                want_halo = halo_fits(N, H, W, Cin) and (halo == 1 or (halo == -1 and r.tiling == 4))
                assert r.halo == want_halo, (s, r)
                assert r.slab_rows == (HALO_SLAB if r.halo else SLAB_OF_TILING[r.tiling]), (s, r)
                assert rows == r.slab_rows and (H * W) % rows == 0, (s, r, rows)
        # the DMA entry itself (cd360_conv3x3_dma_bf16) also serves images that are not whole slabs: same decision, same slab rule
        d = decode(lib.cd360_conv3x3_dma_route(*s))
        if dma == 0 or not dma_fits(*s):
            assert d.family == "register", (s, d)
        else:
            assert d.family == "dma" and d.slab_rows == (HALO_SLAB if d.halo else SLAB_OF_TILING[d.tiling]), (s, d)
            assert d.halo == (halo_fits(N, H, W, Cin) and (halo == 1 or (halo == -1 and d.tiling == 4))), (s, d)
            if cfg > 0 and not (cfg in NEEDS_320 and Cout % 320):
                assert d.tiling == cfg, (s, d)
            assert r.family == "register" or d == r, (s, r, d)
        # what the caller sizes tile_stats from: the DMA core's slabs, else the register-staged kernel's 128 / slabs-per-tile
        want_stats_rows = rows if rows > 0 else 128 // lib.cd360_conv_stats_slabs(Cout)
        assert lib.cd360_conv_stats_rows(*s, 9, 1) == want_stats_rows, s


def test_default_routes_of_the_product_shapes(lib, tune):
    """Pins the default route of every product convolution (tests/conv_shapes.py): e.g. the 320-channel convolutions of the 128^2 level
    at the bench's CFG batch (N = 3) on tiling 6 (32-row slabs), the 32^2 level on the halo form, the VAE decoder's 256^2 and 512^2
    levels on tiling 3 (128-row slabs).  tests/test_conv_routes_gpu.py runs the same table on the card."""
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    for n in BATCHES:
        for h, cin, cout, what in UNET_3X3:
            assert tuple(route_of(lib, n, h, h, cin, cout)) == ("dma",) + UNET_ROUTES[n, h], (n, h, cin, cout, what)
            assert lib.cd360_conv_stats_rows(n, h, h, cin, cout, 9, 1) == UNET_ROUTES[n, h][2]
        for h, c in UNET_UP2X:
            assert lib.cd360_conv_up2x_route(n, h, h, c, c) == UNET_UP2X_TILINGS[n, h], (n, h, c)
    for h, cin, cout, what, want in VAE_3X3:
        assert tuple(route_of(lib, 1, h, h, cin, cout)) == ("dma",) + want, (h, cin, cout, what)
        assert lib.cd360_conv_stats_rows(1, h, h, cin, cout, 9, 1) == want[2]
    for h, c, want in VAE_UP2X:
        assert lib.cd360_conv_up2x_route(1, h, h, c, c) == want, (h, c)
    for s in UNET + VAE:  # (the 24-view batch of the fine-tune step included)
        r = route_of(lib, *s)
        assert r.family == "dma" and r.halo == (r.tiling == 4 and halo_fits(*s[:4])), (s, r)


def test_other_convolutions_report_their_kernel(lib, tune):
    tune(conv_cfg=-1, conv_halo=-1, conv_dma=-1)
    assert route_of(lib, 3, 32, 32, 2560, 1280, taps=1) == ("gemm", 0, False, 0)  # the 1 x 1 skip connections: GEMM entry
    assert route_of(lib, 3, 128, 128, 320, 320, stride=2) == ("register", 0, False, 0)  # Downsample
    assert route_of(lib, 2, 16, 16, 4, 320) == ("register", 0, False, 0)  # Cin % 64
    tune(conv_dma=0)
    assert route_of(lib, 3, 32, 32, 2560, 1280, taps=1).family == "register"
    assert route_of(lib, 3, 128, 128, 320, 320).family == "register"
    assert lib.cd360_conv_stats_rows(3, 128, 128, 320, 320, 9, 1) == 128 // lib.cd360_conv_stats_slabs(320)


@pytest.mark.parametrize("cfg", [-1, 1, 2, 3, 4, 5, 6])
def test_upsample_route(cfg, lib, tune):
    tune(conv_cfg=-1)
    shapes = [(n, h, h, c, c) for n in (1, 2, 3) for h, c in ((32, 1280), (64, 640))] + [(1, 128, 128, 512, 512), (1, 256, 256, 512, 512),
                                                                                          (1, 512, 512, 256, 256), (2, 16, 12, 192, 80), (1, 5, 7, 128, 320)]
    fallback = {s: lib.cd360_conv_up2x_route(*s) for s in shapes}
    tune(conv_cfg=cfg)
    for s in shapes:
        t = lib.cd360_conv_up2x_route(*s)
        forced_ok = cfg > 0 and not (cfg in NEEDS_320 and s[4] % 320)
        assert t == (cfg if forced_ok else fallback[s]) and t in SLAB_OF_TILING, (s, t)
    assert lib.cd360_conv_up2x_route(1, 8, 8, 32, 64) == -2  # Cin % 64: outside the envelope


def test_route_queries_follow_the_query_stream(lib, tune):
    """cd360_conv_route answers, like the other shape queries, for the stream named by the calling thread's last cd360_query_stream."""
    from cd360 import _lib
    tune(conv_cfg=3, conv_halo=0)
    h = 0x5150
    shape = (3, 128, 128, 320, 320)
    try:
        _lib.set_stream_tuning(h, conv_cfg=6)
        assert route_of(lib, *shape) == ("dma", 3, False, 128)
        lib.cd360_query_stream(ctypes.c_void_p(h))
        assert route_of(lib, *shape) == ("dma", 6, False, 32) and lib.cd360_conv_stats_rows(*shape, 9, 1) == 32
        assert lib.cd360_conv_up2x_route(3, 64, 64, 640, 640) == 6
        lib.cd360_query_stream(None)
        assert route_of(lib, *shape) == ("dma", 3, False, 128) and lib.cd360_conv_stats_rows(*shape, 9, 1) == 128
    finally:
        _lib.clear_stream_tuning(h)
        lib.cd360_query_stream(None)


def test_every_forced_case_of_the_gpu_matrix_is_reachable(lib, tune):
    """tests/test_conv_routes_gpu.py forces tilings on small shapes; each (tiling, halo) it names must be what the query reports."""
    for cfg, halo in itertools.product(range(1, 7), (0, 1)):
        tune(conv_cfg=cfg, conv_halo=halo)
        r = route_of(lib, 3, 16, 8, 64, 320)
        assert (r.tiling, r.halo) == (cfg, bool(halo)), (cfg, halo, r)
