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
