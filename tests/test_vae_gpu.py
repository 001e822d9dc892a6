"""The first stage's Decoder on the HIP kernels (sgm.modules.diffusionmodules.model, cd360_attn_single_bf16, cd360_vae_conv_in_f32,
cd360_vae_conv_out_bf16) against fp32: the reference's own outputs (tests/golden/vae_decoder.npz) at small sizes, and the fp32
framework restatement tests/vae_fp32.py on the same weights at full size.  Bars are fixed: a measurement above one is a finding."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_fp32
import weights as W
from cd360 import ops

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_ATTN = 1e-2  # the existing attention bar
TOL = 2.5e-2     # the module bar of test_modules_gpu.py
SDXL_DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                     ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
NARROW_DDCONFIG = dict(SDXL_DDCONFIG, resolution=64, ch=64, ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[16])
DEV = torch.device("cuda:0")


def _rel(got, want):
    return (got.float() - want.float()).abs().max().item() / want.float().abs().max().item()


def _decoder(cfg, seed=3, dtype=torch.float32):
    from sgm.modules.diffusionmodules.model import Decoder
    dec = Decoder(**cfg).eval()
    sd = W.load_into(dec, seed)
    for p in dec.parameters():
        p.requires_grad_(False)
    return dec.to(DEV, dtype), sd


# key splits per query block the host picks (cd360_attn_single_splits, from N alone); N % 32 != 0 puts a ragged, masked last key tile
# in the last split: N = 1 and 33 on the single-launch path, 500 (2 splits, the second ending 20 keys into its last tile) and 4100
# (15 splits) on the key-split path
SPLITS = {1: 1, 33: 1, 256: 1, 480: 1, 500: 2, 4096: 16, 4100: 15, 16384: 4}


@pytest.mark.parametrize("n", sorted(SPLITS))
@pytest.mark.parametrize("b", [1, 2])
def test_attn_single_against_fp32(n, b):
    c = 512
    g = torch.Generator(device=DEV).manual_seed(n + b)
    # q carries the softmax scale: logits of std ~ 3 (neither uniform nor one-hot)
    qkv = torch.randn(b * n, 3 * c, generator=g, device=DEV)
    qkv[:, :c] *= 3.0 / c ** 0.5
    qkv = qkv.to(torch.bfloat16).view(b, n, 3 * c)
    q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    with torch.no_grad():
        out = ops.attention_single(q, k, v)
    torch.cuda.synchronize()
    assert ops.attention_single_splits(b, n) == SPLITS[n]
    qf, kf, vf = (t.float() for t in (q, k, v))
    for i in range(0, n, 1024):
        s = torch.matmul(qf[:, i:i + 1024], kf.transpose(1, 2)) * 0.6931471805599453  # base-2 logits -> natural
        p = torch.softmax(s, -1)
        if i == 0 and n >= 256:
            assert 0.01 < p.amax(-1).mean().item() < 0.9  # not one-hot, not uniform
        want = torch.matmul(p, vf)
        assert _rel(out[:, i:i + 1024], want) < TOL_ATTN, (n, b, i)


def test_memory_efficient_attention_routes_head_dim_512():
    g = torch.Generator(device=DEV).manual_seed(5)
    q, k, v = (torch.randn(2, 480, 512, generator=g, device=DEV) for _ in range(3))
    with torch.no_grad():
        out = ops.memory_efficient_attention(q, k, v)
    assert out.dtype == torch.float32 and out.shape == q.shape
    qb, kb, vb = (t.to(torch.bfloat16).float() for t in (q, k, v))
    want = torch.softmax(torch.matmul(qb, kb.transpose(1, 2)) * 512 ** -0.5, -1) @ vb
    assert _rel(out, want) < TOL_ATTN


@pytest.mark.parametrize("h,w", [(17, 23), (128, 128)])
def test_conv_in_against_conv2d(h, w):
    g = torch.Generator(device=DEV).manual_seed(h)
    z = torch.randn(2, 4, h, w, generator=g, device=DEV)
    wt = torch.randn(512, 4, 3, 3, generator=g, device=DEV) / 6
    b = torch.randn(512, generator=g, device=DEV) * 0.05
    with torch.no_grad():
        got = ops.vae_conv_in(z, ops.pack_vae_conv_in_weight(wt), b)
    want = F.conv2d(z, wt, b, padding=1).permute(0, 2, 3, 1).reshape(2, h * w, 512)
    # one bf16 rounding (2^-8 relative) + fp32 summation slack
    assert ((got.float() - want).abs() <= want.abs() * 2 ** -8 + 1e-5).all()
    if (h * w) % 64 == 0:
        _, st = ops.vae_conv_in(z, ops.pack_vae_conv_in_weight(wt), b, want_stats=True)
        gf = got.float().view(2, -1, 64, 512)
        assert torch.allclose(st[..., 0], gf.sum(2), rtol=1e-4, atol=1e-3)
        assert torch.allclose(st[..., 1], (gf * gf).sum(2), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("h,w,cin", [(17, 23, 128), (1024, 1024, 128), (33, 40, 320)])
def test_conv_out_against_conv2d(h, w, cin):
    g = torch.Generator(device=DEV).manual_seed(w)
    x = torch.randn(1, h * w, cin, generator=g, device=DEV).to(torch.bfloat16)
    wt = torch.randn(3, cin, 3, 3, generator=g, device=DEV) / (9 * cin) ** 0.5
    b = torch.randn(3, generator=g, device=DEV) * 0.05
    with torch.no_grad():
        got = ops.vae_conv_out(x, ops.pack_vae_conv_out_weight(wt), b, 1, h, w, 3)
    xin = x.float().view(1, h, w, cin).permute(0, 3, 1, 2)
    want = F.conv2d(xin, wt, b, padding=1)
    assert got.shape == (1, 3, h, w) and got.dtype == torch.float32
    # fp32 on both sides: summation-order slack only
    bound = F.conv2d(xin.abs(), wt.abs(), b.abs(), padding=1) * 1e-5 + 1e-6
    assert ((got - want).abs() <= bound).all()


@pytest.mark.parametrize("case,cfg", [("sdxl", SDXL_DDCONFIG), ("narrow", NARROW_DDCONFIG), ("ragged", NARROW_DDCONFIG)])
def test_decoder_against_reference_golden(case, cfg):
    d = np.load(os.path.join(GOLD, "vae_decoder.npz"))
    dec, _ = _decoder(cfg)
    with torch.no_grad():
        out = dec(torch.from_numpy(d[f"z.{case}"]).to(DEV))
    want = torch.from_numpy(d[f"out.{case}"])
    assert out.shape == want.shape and out.dtype == torch.float32
    assert torch.isfinite(out).all()
    assert _rel(out.cpu(), want) < TOL, case


@pytest.fixture(scope="module")
def sdxl():
    dec, sd = _decoder(SDXL_DDCONFIG)
    return dec, {k: v.to(DEV) for k, v in sd.items()}


@pytest.mark.parametrize("hw", [64, 128])
def test_decoder_full_size_against_fp32_restatement(sdxl, hw):
    dec, sd = sdxl
    z = W.tensor(f"z{hw}", (2, 4, hw, hw), seed=1).to(DEV)
    with torch.no_grad():
        one = [dec(z[i:i + 1]) for i in range(2 if hw == 128 else 1)]
        wants = []
        for i, o in enumerate(one):
            wants.append(vae_fp32.decode(sd, z[i:i + 1], SDXL_DDCONFIG["ch_mult"], 2))
            assert torch.isfinite(o).all()
            assert _rel(o, wants[i]) < TOL, (hw, i)
        if hw == 128:
            # Decoder.forward decodes one image per pass: a batch gives each image's own decode, bit for bit
            both = dec(z)
            assert torch.isfinite(both).all()
            for i in range(2):
                assert torch.equal(both[i], one[i][0])
            # the batch-folded pass (what forward would run for the whole batch) is as close to fp32 as the per-image one
            folded = dec._decode_pass(z)
            assert torch.isfinite(folded).all()
            for i in range(2):
                assert _rel(folded[i], wants[i][0]) < TOL, ("folded", i)


def test_bf16_parameters_and_stale_pack(sdxl):
    _, sd = sdxl
    dec, _ = _decoder(SDXL_DDCONFIG, dtype=torch.bfloat16)
    sd16 = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    z = W.tensor("z32", (1, 4, 32, 32), seed=2).to(DEV)
    with torch.no_grad():
        out = dec(z)
        assert out.dtype == torch.bfloat16
        want = vae_fp32.decode(sd16, z, SDXL_DDCONFIG["ch_mult"], 2)
        assert _rel(out, want) < TOL
        before = dec(z).float()
        dec.up[0].block[0].conv2.weight.copy_(dec.up[0].block[0].conv2.weight * 0.5)  # bumps _version, as load_state_dict does
        after = dec(z).float()
    assert (after - before).abs().max().item() > 1e-2


def test_forward_hook_sees_real_values(sdxl):
    dec, _ = sdxl
    seen = []
    hk = dec.mid.attn_1.register_forward_hook(lambda m, i, o: seen.append((tuple(o.shape), o.float().abs().max().item())))
    try:
        with torch.no_grad():
            dec(W.tensor("zh", (2, 4, 16, 16), seed=4).to(DEV))
    finally:
        hk.remove()
    # Decoder.forward decodes one image per pass (batch-invariant output): the hook fires once per image
    assert len(seen) == 2 and all(s[0] == (1, 512, 16, 16) and 0 < s[1] < float("inf") for s in seen)


def test_autoencoder_decode_call_shape():
    """AutoencoderKL.decode: post_quant_conv (a framework 1x1 conv) then the Decoder, on z / scale_factor (diffusion.py:208-212)."""
    dec, sd = _decoder(dict(SDXL_DDCONFIG))
    pqc = torch.nn.Conv2d(4, 4, 1).to(DEV)
    with torch.no_grad():
        pqc.weight.copy_(W.tensor("pqc.w", (4, 4, 1, 1), seed=3).to(DEV) * 0.5)
        pqc.bias.copy_(W.tensor("pqc.b", (4,), seed=3).to(DEV) * 0.05)
        z = W.tensor("zs", (1, 4, 25, 19), seed=5).to(DEV)  # N = 475: a ragged last key tile in mid.attn_1
        out = dec(pqc(z / 0.13025))
        want = vae_fp32.decode({k: v.to(DEV) for k, v in sd.items()}, pqc(z / 0.13025), SDXL_DDCONFIG["ch_mult"], 2)
    assert out.shape == (1, 3, 200, 152) and torch.isfinite(out).all()
    assert _rel(out, want) < TOL
