"""The convolution shapes of the product and the route each takes at default tuning (cd360_conv_route / cd360_conv_up2x_route).

tests/test_conv_routes_cpu.py pins the routes on the host; tests/test_conv_routes_gpu.py runs every shape on the card against fp32.
A change of the picker's weights or of the halo rule shows up here first, as a deliberate edit of this table."""

# 3 x 3 / stride 1 convolutions of the SDXL UNet (cd360.configs.SDXL_NETWORK_CONFIG, latent 128^2; tools/probe/conv_census.py lists the
# launches of one denoise step) per level: (H = W, Cin, Cout, what).  ResBlock in_layers[2] (openaimodel.py ResBlock._forward) takes the
# per-image emb addend and writes GroupNorm statistics; out_layers[3] adds the skip connection and writes statistics.  input_blocks.0.0
# is 4 -> 320 with Cin zero-padded to 64 (util.packed_conv).
UNET_3X3 = [
    (128, 64, 320, "input_blocks.0.0"),
    (128, 320, 320, "input_blocks.1-2 in / out, output_blocks.6-8 out"),
    (128, 960, 320, "output_blocks.6 in"),
    (128, 640, 320, "output_blocks.7-8 in"),
    (64, 320, 640, "input_blocks.4 in"),
    (64, 640, 640, "input_blocks.4-5 out, input_blocks.5 in, output_blocks.3-5 out"),
    (64, 1920, 640, "output_blocks.3 in"),
    (64, 1280, 640, "output_blocks.4 in"),
    (64, 960, 640, "output_blocks.5 in"),
    (32, 640, 1280, "input_blocks.7 in"),
    (32, 1280, 1280, "input_blocks.7-8, middle_block, output_blocks.0-2 out"),
    (32, 2560, 1280, "output_blocks.0-1 in"),
    (32, 1920, 1280, "output_blocks.2 in"),
]
# Upsample convolutions folded into cd360_conv_up2x_bf16 (output_blocks.2.2: 32^2 -> 64^2, output_blocks.5.2: 64^2 -> 128^2): source
# (H = W, C)
UNET_UP2X = [(32, 1280), (64, 640)]
# The 1 x 1 skip connections (GEMM entry): (H = W, Cin, Cout)
UNET_1X1 = [(64, 320, 640), (64, 1920, 640), (64, 1280, 640), (64, 960, 640), (32, 640, 1280), (32, 2560, 1280), (32, 1920, 1280),
            (128, 960, 320), (128, 640, 320)]
BATCHES = (1, 2, 3)  # bench.py: one image / two / the 3-way CFG batch of the headline config

# default route (tiling, halo form, slab rows) of UNET_3X3 by batch and level; the tiling depends on N * H * W and Cout only
UNET_ROUTES = {
    (1, 128): (2, False, 64), (1, 64): (4, True, 64), (1, 32): (4, True, 64),
    (2, 128): (4, False, 64), (2, 64): (2, False, 64), (2, 32): (4, True, 64),
    (3, 128): (6, False, 32), (3, 64): (2, False, 64), (3, 32): (4, True, 64),
}
# default tiling of UNET_UP2X by (batch, source size)
UNET_UP2X_TILINGS = {(1, 32): 2, (2, 32): 4, (3, 32): 3, (1, 64): 4, (2, 64): 1, (3, 64): 2}

# ---- the data gradient (cd360.grad.ConvIgemmFn: BASELINE config 4, every frozen convolution differentiated with respect to its input).
# It has no kernel of its own: cd360_conv_igemm_bf16 runs again on dy (zero-inserted to the input's size for a stride-2 convolution) with
# the weight of sgm...util.packed_conv_dgrad -- so the channel counts SWAP and the launch is (N, H, W, Cin' = Cout padded to 16 then 64,
# Cout' = Cin padded to 64), stride 1, at the forward INPUT's size.
UNET_UPSAMPLE_3X3 = [  # Upsample.conv takes the unfolded path under autograd (the fold is forward only): a plain 3 x 3 at the OUTPUT size
    (64, 1280, 1280, "output_blocks.2.2 conv (unfolded under autograd)"),
    (128, 640, 640, "output_blocks.5.2 conv (unfolded under autograd)"),
]
UNET_DOWNSAMPLE = [(128, 320, 320, "input_blocks.3.0 op (stride 2)"), (64, 640, 640, "input_blocks.6.0 op (stride 2)")]  # (input H = W, ...)
UNET_OUT_CONV = (128, 320, 4, "out.2")


def dgrad_channels(cin, cout):
    """(Cin', Cout') of the data-gradient launch of a cin -> cout convolution (packed_conv pads Cin to 64 and Cout to 16,
    packed_conv_dgrad pads that Cout to 64 as its input channels)"""
    return -(-(-(-cout // 16) * 16) // 64) * 64, -(-cin // 64) * 64


# (level H = W of the launch, Cin', Cout', taps, what); input_blocks.0.0's entry is launched only when the latent itself wants a gradient
UNET_DGRAD = [(h, *dgrad_channels(cin, cout), 9, "dgrad of " + what) for h, cin, cout, what in UNET_3X3 + UNET_UPSAMPLE_3X3] + \
             [(h, *dgrad_channels(cin, cout), 9, "dgrad of " + what + ", zero-inserted dy") for h, cin, cout, what in UNET_DOWNSAMPLE] + \
             [(UNET_OUT_CONV[0], *dgrad_channels(*UNET_OUT_CONV[1:3]), 9, "dgrad of " + UNET_OUT_CONV[3])] + \
             [(h, *dgrad_channels(cin, cout), 1, f"dgrad of the {cin} -> {cout} skip connection") for h, cin, cout in UNET_1X1]
# the bench batches, the fine-tune step's own batch (tools/bench_train.py: 4) and its 24 views
DGRAD_BATCHES = BATCHES + (4, 24)
DGRAD_SCALES = (1, 2)  # level / 1 = the table's latent sizes (1024^2 images), level / 2 = 512^2 training

# Default route of the 3 x 3 data-gradient launches, as cd360_conv_route of the built library answers on the host
# (tests/test_conv_dgrad_cpu.py pins it): {(batch, H = W of the launch): {Cout': (tiling, halo form, slab rows)}}.  The tiling depends on
# N * H * W and Cout' only.  Every 1 x 1 launch takes the GEMM entry.
UNET_DGRAD_ROUTES = {
    (1, 16): {640: (4, True, 64), 1280: (4, True, 64), 1920: (4, True, 64), 2560: (4, True, 64)},
    (1, 32): {320: (4, True, 64), 640: (4, True, 64), 960: (4, True, 64), 1280: (4, True, 64), 1920: (4, True, 64), 2560: (4, True, 64)},
    (1, 64): {64: (4, True, 64), 320: (4, True, 64), 640: (4, True, 64), 960: (4, True, 64), 1280: (2, False, 64), 1920: (2, False, 64)},
    (1, 128): {64: (4, False, 64), 320: (2, False, 64), 640: (4, False, 64), 960: (3, False, 128)},
    (2, 16): {640: (4, True, 64), 1280: (4, True, 64), 1920: (4, True, 64), 2560: (4, True, 64)},
    (2, 32): {320: (4, True, 64), 640: (4, True, 64), 960: (4, True, 64), 1280: (4, True, 64), 1920: (4, True, 64), 2560: (2, False, 64)},
    (2, 64): {64: (4, True, 64), 320: (4, True, 64), 640: (2, False, 64), 960: (2, False, 64), 1280: (4, True, 64), 1920: (3, False, 128)},
    (2, 128): {64: (4, False, 64), 320: (4, False, 64), 640: (1, False, 64), 960: (3, False, 128)},
    (3, 16): {640: (4, True, 64), 1280: (4, True, 64), 1920: (4, True, 64), 2560: (4, True, 64)},
    (3, 32): {320: (4, True, 64), 640: (4, True, 64), 960: (4, True, 64), 1280: (4, True, 64), 1920: (2, False, 64), 2560: (2, False, 64)},
    (3, 64): {64: (4, True, 64), 320: (2, False, 64), 640: (2, False, 64), 960: (4, True, 64), 1280: (3, False, 128), 1920: (2, False, 64)},
    (3, 128): {64: (2, False, 64), 320: (6, False, 32), 640: (2, False, 64), 960: (3, False, 128)},
    (4, 16): {640: (4, True, 64), 1280: (4, True, 64), 1920: (4, True, 64), 2560: (4, True, 64)},
    (4, 32): {320: (4, True, 64), 640: (4, True, 64), 960: (4, True, 64), 1280: (2, False, 64), 1920: (2, False, 64), 2560: (4, True, 64)},
    (4, 64): {64: (4, True, 64), 320: (2, False, 64), 640: (4, True, 64), 960: (3, False, 128), 1280: (1, False, 64), 1920: (3, False, 128)},
    (4, 128): {64: (2, False, 64), 320: (1, False, 64), 640: (1, False, 64), 960: (1, False, 64)},
    (24, 16): {640: (4, True, 64), 1280: (2, False, 64), 1920: (4, True, 64), 2560: (3, False, 128)},
    (24, 32): {320: (4, True, 64), 640: (2, False, 64), 960: (2, False, 64), 1280: (3, False, 128), 1920: (3, False, 128), 2560: (1, False, 64)},
    (24, 64): {64: (4, True, 64), 320: (6, False, 32), 640: (1, False, 64), 960: (3, False, 128), 1280: (1, False, 64), 1920: (1, False, 64)},
    (24, 128): {64: (2, False, 64), 320: (1, False, 64), 640: (1, False, 64), 960: (1, False, 64)},
}

# (tiling, halo form, Cout') of data-gradient launches at default tuning that no forward launch of UNET_3X3 takes (same batches and
# sizes): tiling 1, "the 128^2 level, one channel tile", with up to eight channel tiles; tiling 3 with 3.75 and 7.5 tiles of 256 channels
DGRAD_ONLY_ROUTES = [
    (1, False, 960), (1, False, 1280), (1, False, 1920), (1, False, 2560),
    (2, False, 64), (2, False, 960), (2, False, 1920), (2, False, 2560),
    (3, False, 960), (3, False, 1920), (3, False, 2560),
    (4, False, 64), (4, False, 640),
    (4, True, 64), (4, True, 960), (4, True, 1920), (4, True, 2560),
]


def dgrad_product_launches():
    """For each of DGRAD_ONLY_ROUTES the smallest product launch (N, H = W, Cin', Cout') that takes it"""
    out = []
    for t, halo, co in DGRAD_ONLY_ROUTES:
        cands = [(n * s * s * ci, n, s, ci) for (n, s), d in UNET_DGRAD_ROUTES.items() if d.get(co, ())[:2] == (t, halo)
                 for h, ci, co2, taps, _ in UNET_DGRAD if taps == 9 and co2 == co and s in [h // sc for sc in DGRAD_SCALES]]
        _, n, s, ci = min(cands)
        out.append((n, s, ci, co, t, halo))
    return out


# The first-stage Decoder (SDXL ddconfig: ch 128, ch_mult 1 2 4 4, two ResBlocks + one per level in the decoder) for ONE 1024^2 image
# (Decoder.forward decodes one image per pass): (H = W, Cin, Cout, what, route).  conv1 of a ResnetBlock writes statistics, conv2 adds
# the shortcut.
VAE_3X3 = [
    (128, 512, 512, "mid.block_1-2, up.3.block conv1 / conv2", (2, False, 64)),
    (256, 512, 512, "up.2.block conv1 / conv2", (3, False, 128)),
    (512, 512, 256, "up.1.block.0 conv1", (3, False, 128)),
    (512, 256, 256, "up.1.block conv2, up.1.block.1-2 conv1", (3, False, 128)),
    (1024, 256, 128, "up.0.block.0 conv1", (2, False, 64)),
    (1024, 128, 128, "up.0.block conv2, up.0.block.1-2 conv1", (2, False, 64)),
]
# Decoder upsamples (up.3 .. up.1): source (H = W, C, default tiling)
VAE_UP2X = [(128, 512, 3), (256, 512, 3), (512, 256, 3)]
# nin_shortcut 1 x 1 convolutions and the mid attention's q|k|v / proj_out (GEMM entry): (H = W, Cin, Cout)
VAE_1X1 = [(512, 512, 256), (1024, 256, 128), (128, 512, 1536), (128, 512, 512)]
