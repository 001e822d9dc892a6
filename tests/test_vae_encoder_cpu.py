"""The first stage's Encoder on the host: the fp32 restatement (tests/vae_enc_fp32.py) reproduces the reference's own outputs
(tests/golden/vae_encoder.npz), the encoder's conv_out weight packing matches its definition, the Downsample statistics-slab query keeps
its contract, and the calls the HIP modules do not serve raise."""
import os

import numpy as np
import pytest
import torch

import weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SDXL_DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                     ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
NARROW_DDCONFIG = dict(SDXL_DDCONFIG, resolution=64, ch=64, ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[16])


def _model():
    from sgm.modules.diffusionmodules import model
    return model


@pytest.mark.parametrize("case,cfg", [("sdxl", SDXL_DDCONFIG), ("narrow", NARROW_DDCONFIG), ("ragged", NARROW_DDCONFIG)])
def test_fp32_restatement_matches_the_golden_on_the_host(case, cfg):
    """tests/vae_enc_fp32.py (the GPU tests' full-size yardstick) reproduces the reference's own output (vae_encoder.npz) on the host."""
    import vae_enc_fp32
    d = np.load(os.path.join(GOLD, "vae_encoder.npz"))
    sd = W.synth_state_dict({k: v.shape for k, v in _model().Encoder(**cfg).state_dict().items()}, seed=3)
    with torch.no_grad():
        out = vae_enc_fp32.encode(sd, torch.from_numpy(d[f"x.{case}"]), cfg["ch_mult"], cfg["num_res_blocks"])
    want = torch.from_numpy(d[f"out.{case}"])
    assert out.shape == want.shape
    assert (out - want).abs().max().item() <= 1e-4 * want.abs().max().item()


@pytest.mark.parametrize("cout", [8, 5])
def test_enc_conv_out_weight_packing(cout):
    from cd360 import ops
    g = torch.Generator().manual_seed(cout)
    w = torch.randn(cout, 512, 3, 3, generator=g)
    p = ops.pack_vae_enc_conv_out_weight(w)
    assert p.shape == (9, 512, 8) and p.dtype == torch.float32 and p.is_contiguous()
    assert torch.all(p[:, :, cout:] == 0)
    for ky in range(3):
        for kx in range(3):
            assert torch.equal(p[3 * ky + kx, :, :cout], w[:, :, ky, kx].t())
    with pytest.raises(AssertionError):
        ops.pack_vae_enc_conv_out_weight(torch.zeros(9, 64, 3, 3))


@pytest.fixture
def lib():
    from cd360 import _lib
    return _lib.load()


def test_downsample_stats_rows_contract(lib):
    q = lib.cd360_vae_downsample_stats_rows
    # the SDXL encoder's three Downsamples at 512^2 and 1024^2 images: 64-pixel slabs (two per 128-pixel tile of the register-staged kernel)
    for n, h, c in [(1, 512, 128), (1, 256, 256), (1, 128, 512), (1, 1024, 128), (1, 512, 256), (1, 256, 512), (3, 128, 512)]:
        rows = q(n, h, h, c)
        assert rows == 64, (n, h, c)
        assert ((h // 2) ** 2) % rows == 0
    # odd sizes: 43 x 51 -> 21 x 25 and 21 x 25 -> 10 x 12 are not whole 128-pixel tiles; 257 x 256 -> 128 x 128 is
    assert q(1, 43, 51, 64) == 0
    assert q(1, 21, 25, 128) == 0
    assert q(1, 257, 256, 128) == 64
    # tiny and outside the envelope
    for n, h, w, c in [(1, 2, 2, 128), (1, 2, 3, 64), (1, 1, 8, 64), (1, 8, 1, 64), (0, 32, 32, 64), (1, 32, 32, 96), (1, 32, 32, 0)]:
        assert q(n, h, w, c) == 0, (n, h, w, c)


def test_unserved_calls_raise():
    m = _model()
    enc = m.Encoder(**dict(SDXL_DDCONFIG, ch=64, ch_mult=[1, 2]))
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            enc(torch.zeros(1, 3, 16, 16))  # a host tensor
        with pytest.raises(NotImplementedError):
            m.Downsample(64, with_conv=False)(torch.zeros(1, 64, 4, 4))
    # a call autograd would have to record
    with pytest.raises(NotImplementedError):
        enc(torch.zeros(1, 3, 16, 16))
    with pytest.raises(NotImplementedError):
        m.Downsample(64, with_conv=False)(torch.zeros(1, 64, 4, 4))


def test_pass_bytes_bounds_the_level_0_activation():
    enc = _model().Encoder(**SDXL_DDCONFIG)
    assert enc.pass_bytes(512, 512) == 512 * 512 * 128 * 2
    assert enc.pass_bytes(2048, 2048) == 2048 * 2048 * 128 * 2
    assert enc.pass_bytes(4096, 4096) >= 2 ** 31  # forward raises Cd360Error for this image


def test_downsample_stats_rows_follow_the_query_stream(lib):
    """Like cd360_conv_stats_rows, the query answers for the stream named by the calling thread's last cd360_query_stream: at C = 320 the
    160-channel tiling (four 32-pixel slabs per tile) serves the call unless that stream's tuning sets conv_wide = 0."""
    import ctypes
    from cd360 import _lib
    h = 0x5151
    try:
        _lib.set_stream_tuning(h, conv_wide=0)
        assert lib.cd360_vae_downsample_stats_rows(1, 64, 64, 320) == 32
        lib.cd360_query_stream(ctypes.c_void_p(h))
        assert lib.cd360_vae_downsample_stats_rows(1, 64, 64, 320) == 64
        lib.cd360_query_stream(None)
        assert lib.cd360_vae_downsample_stats_rows(1, 64, 64, 320) == 32
    finally:
        _lib.clear_stream_tuning(h)
        lib.cd360_query_stream(None)
