"""The first stage's Decoder / Encoder module tree (sgm.modules.diffusionmodules.model) on the host: it imports without xformers or
einops, has exactly the reference's state_dict keys and shapes (tests/golden/vae_*.keys.json.gz, written by make_golden_vae.py from the
reference's own module), rejects the options it does not serve, and its host-side weight packings match their definitions."""
import gzip
import importlib
import json
import os
import sys

import pytest
import torch

import weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SDXL_DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                     ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)


def _model():
    return importlib.import_module("sgm.modules.diffusionmodules.model")


def test_model_imports_without_xformers_or_einops():
    saved = {k: sys.modules.get(k) for k in ("xformers", "xformers.ops", "einops")}
    try:
        for k in saved:
            sys.modules[k] = None  # import of these names now raises ImportError
        sys.modules.pop("sgm.modules.diffusionmodules.model", None)
        m = importlib.import_module("sgm.modules.diffusionmodules.model")
        for name in ("nonlinearity", "Normalize", "Upsample", "Downsample", "ResnetBlock", "AttnBlock", "MemoryEfficientAttnBlock",
                     "make_attn", "Encoder", "Decoder"):
            assert hasattr(m, name), name
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@pytest.mark.parametrize("which", ["decoder", "encoder"])
def test_keys_and_shapes_match_the_reference(which):
    with gzip.open(os.path.join(GOLD, f"vae_{which}.keys.json.gz"), "rt") as f:
        want = json.load(f)
    cls = _model().Decoder if which == "decoder" else _model().Encoder
    got = {k: list(v.shape) for k, v in cls(**SDXL_DDCONFIG).state_dict().items()}
    assert got == want


def test_decoder_loads_a_synthetic_checkpoint_strictly():
    dec = _model().Decoder(**SDXL_DDCONFIG)
    sd = W.synth_state_dict({k: v.shape for k, v in dec.state_dict().items()}, seed=3)
    dec.load_state_dict(sd, strict=True)
    assert isinstance(dec.mid.attn_1, _model().MemoryEfficientAttnBlock)
    assert isinstance(_model().make_attn(64, "vanilla"), _model().AttnBlock)
    assert isinstance(_model().make_attn(64, "none"), torch.nn.Identity)


def test_unsupported_options_raise():
    m = _model()
    for t in ("linear", "memory-efficient-cross-attn"):
        with pytest.raises(NotImplementedError):
            m.make_attn(64, t)
    with pytest.raises(NotImplementedError):
        m.Decoder(**dict(SDXL_DDCONFIG, use_linear_attn=True))
    z = torch.zeros(1, 4, 8, 8)
    with torch.no_grad():
        for kw in ({"give_pre_end": True}, {"tanh_out": True}):
            with pytest.raises(NotImplementedError):
                m.Decoder(**dict(SDXL_DDCONFIG, ch=64, ch_mult=[1], **kw))(z)
        with pytest.raises(NotImplementedError):
            m.Encoder(**dict(SDXL_DDCONFIG, ch=64, ch_mult=[1]))(torch.zeros(1, 3, 8, 8))
        with pytest.raises(NotImplementedError):
            m.Upsample(64, with_conv=False)(torch.zeros(1, 64, 4, 4))
        rb = m.ResnetBlock(in_channels=64, out_channels=64, dropout=0.1, temb_channels=0).train()
        with pytest.raises(NotImplementedError):
            rb(torch.zeros(1, 64, 4, 4), None)
        with pytest.raises(NotImplementedError):
            rb.eval()(torch.zeros(1, 64, 4, 4), torch.zeros(1, 512))
    # a call autograd would have to record
    with pytest.raises(NotImplementedError):
        m.Decoder(**dict(SDXL_DDCONFIG, ch=64, ch_mult=[1]))(z)


def test_max_batch_at_1024():
    dec = _model().Decoder(**SDXL_DDCONFIG)
    # largest activation per image at a 128^2 latent: the 1024^2 x 256 Upsample output, 512 MiB -> three images per pass
    assert dec.max_batch(128, 128) == 3
    assert dec.max_batch(64, 64) == 15


def test_host_weight_packings():
    from cd360 import ops
    g = torch.Generator().manual_seed(0)
    w_in = torch.randn(512, 4, 3, 3, generator=g)
    p = ops.pack_vae_conv_in_weight(w_in)
    assert p.shape == (36, 512) and p.dtype == torch.float32
    for ci in range(4):
        for ky in range(3):
            for kx in range(3):
                assert torch.equal(p[ci * 9 + ky * 3 + kx], w_in[:, ci, ky, kx])
    w_out = torch.randn(3, 128, 3, 3, generator=g)
    p = ops.pack_vae_conv_out_weight(w_out)
    assert p.shape == (9, 128, 4) and p.dtype == torch.float32 and torch.all(p[:, :, 3] == 0)
    for ky in range(3):
        for kx in range(3):
            assert torch.equal(p[3 * ky + kx, :, :3], w_out[:, :, ky, kx].t())
    c = 128
    ws = [torch.randn(c, c, 1, 1, generator=g) for _ in range(3)]
    bs = [torch.randn(c, generator=g) for _ in range(3)]
    w, b = ops.pack_attn_qkv(ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])
    s = c ** -0.5 * 1.4426950408889634
    assert w.shape == (3 * c, c) and w.dtype == torch.bfloat16 and b.dtype == torch.float32
    assert torch.equal(w[:c], (ws[0].reshape(c, c) * s).to(torch.bfloat16))
    assert torch.equal(w[c:2 * c], ws[1].reshape(c, c).to(torch.bfloat16)) and torch.equal(w[2 * c:], ws[2].reshape(c, c).to(torch.bfloat16))
    assert torch.equal(b, torch.cat([bs[0] * s, bs[1], bs[2]]))


NARROW_DDCONFIG = dict(SDXL_DDCONFIG, resolution=64, ch=64, ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[16])


@pytest.mark.parametrize("case,cfg", [("sdxl", SDXL_DDCONFIG), ("narrow", NARROW_DDCONFIG), ("ragged", NARROW_DDCONFIG)])
def test_fp32_restatement_matches_the_golden_on_the_host(case, cfg):
    """tests/vae_fp32.py (the GPU tests' full-size yardstick) reproduces the reference's own output (vae_decoder.npz) on the host."""
    import numpy as np
    import vae_fp32
    d = np.load(os.path.join(GOLD, "vae_decoder.npz"))
    sd = W.synth_state_dict({k: v.shape for k, v in _model().Decoder(**cfg).state_dict().items()}, seed=3)
    with torch.no_grad():
        out = vae_fp32.decode(sd, torch.from_numpy(d[f"z.{case}"]), cfg["ch_mult"], cfg["num_res_blocks"])
    want = torch.from_numpy(d[f"out.{case}"])
    assert (out - want).abs().max().item() <= 1e-4 * want.abs().max().item()
