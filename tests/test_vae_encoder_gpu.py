"""The first stage's Encoder on the HIP kernels (sgm.modules.diffusionmodules.model.Encoder: cd360_vae_conv_in_f32, the decoder's blocks,
cd360_vae_downsample_bf16, cd360_vae_enc_conv_out_bf16) against fp32: the two new kernels against F.conv2d element by element, the
module against the reference's own outputs (tests/golden/vae_encoder.npz) at small sizes and against the fp32 restatement
tests/vae_enc_fp32.py on the same weights at 512^2 and 1024^2.  Bars are fixed: a measurement above one is a finding."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_enc_fp32
import weights as W
from cd360 import ops

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 2.5e-2  # the module bar of test_modules_gpu.py
REL_BAR, ABS_SLACK = 2.0 ** -8, 1e-4  # one bf16 rounding + fp32 summation slack (test_conv_routes_gpu.py)
SDXL_DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                     ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
NARROW_DDCONFIG = dict(SDXL_DDCONFIG, resolution=64, ch=64, ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[16])
DEV = torch.device("cuda:0")


class _fp32_exact:
    """fp32 convolutions / GEMMs without TF32 (the GPU reference)."""

    def __enter__(self):
        self.saved = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False

    def __exit__(self, *a):
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = self.saved
        return False


def _rel(got, want):
    return (got.float() - want.float()).abs().max().item() / want.float().abs().max().item()


def _encoder(cfg, seed=3, dtype=torch.float32):
    from sgm.modules.diffusionmodules.model import Encoder
    enc = Encoder(**cfg).eval()
    sd = W.load_into(enc, seed)
    for p in enc.parameters():
        p.requires_grad_(False)
    return enc.to(DEV, dtype), sd


def _down_ref(x_nchw, w, b):
    """The reference's Downsample in fp32 and the same over absolute values."""
    with _fp32_exact():
        ref = F.conv2d(F.pad(x_nchw, (0, 1, 0, 1)), w, b, stride=2)
        a = F.conv2d(F.pad(x_nchw.abs(), (0, 1, 0, 1)), w.abs(), b.abs(), stride=2)
    return ref, a


def _assert_close(got, ref, A, what):
    assert torch.isfinite(got).all(), what
    err = (got.float() - ref).abs()
    bar = REL_BAR * ref.abs() + ABS_SLACK * A
    bad = err > bar
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements above the bar, worst {float((err / bar).max()):.3g} x the bar"


# ----------------------------------------------------------------------------------------------- Downsample kernel
@pytest.mark.parametrize("n,h,w,c", [(1, 512, 512, 128), (1, 256, 256, 256), (1, 128, 128, 512), (1, 21, 25, 256), (1, 2, 3, 128),
                                     (3, 64, 64, 512), (3, 43, 51, 64)])
def test_downsample_against_conv2d(n, h, w, c):
    from cd360 import _lib
    g = torch.Generator(device=DEV).manual_seed(h * w + c)
    x = torch.randn(n, h * w, c, generator=g, device=DEV).to(torch.bfloat16)
    wt = (torch.randn(c, c, 3, 3, generator=g, device=DEV) / (9 * c) ** 0.5).to(torch.bfloat16).float()
    b = torch.randn(c, generator=g, device=DEV) * 0.05
    wp = ops.pack_conv_weight(wt)
    ho, wo = h // 2, w // 2
    rows = ops.vae_downsample_stats_rows(n, h, w, c)
    assert rows == (64 if (ho * wo) % 128 == 0 else 0)
    # the entry point itself, statistics into a NaN-filled buffer of twice the promised size
    out = torch.empty(n * ho * wo, c, dtype=torch.bfloat16, device=DEV)
    buf = torch.full((2 * (n * ho * wo // rows) * c * 2,), float("nan"), device=DEV) if rows else None
    with torch.no_grad():
        rc = _lib.load().cd360_vae_downsample_bf16(x.data_ptr(), wp.data_ptr(), b.data_ptr(), out.data_ptr(),
                                                   None if buf is None else buf.data_ptr(), n, h, w, c, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        got, st = ops.vae_downsample(x, wp, b, n, h, w)
    torch.cuda.synchronize()
    assert torch.equal(got.view(-1, c), out)
    ref, A = _down_ref(x.float().view(n, h, w, c).permute(0, 3, 1, 2), wt, b)
    _assert_close(out.view(n, ho, wo, c).permute(0, 3, 1, 2), ref, A, (n, h, w, c))
    if rows:
        promised = (n * ho * wo // rows) * c * 2
        assert st.shape == (n, ho * wo // rows, c, 2) and torch.equal(st.view(-1), buf[:promised])
        assert torch.isnan(buf[promised:]).all(), "statistics written past the promised size"
        s = buf[:promised].view(-1, c, 2).double()
        o = out.double().view(-1, rows, c)
        assert ((s[..., 0] - o.sum(1)).abs() <= 1e-5 * o.abs().sum(1)).all()
        assert ((s[..., 1] - (o * o).sum(1)).abs() <= 1e-5 * (o * o).sum(1)).all()
    else:
        assert st is None


# ----------------------------------------------------------------------------------------------- Encoder conv_out kernel
@pytest.mark.parametrize("h,w", [(64, 64), (128, 128), (17, 23)])
@pytest.mark.parametrize("cin,cout", [(128, 8), (512, 8), (128, 5), (512, 5)])
@pytest.mark.parametrize("b", [1, 3])
def test_enc_conv_out_against_conv2d(h, w, cin, cout, b):
    g = torch.Generator(device=DEV).manual_seed(h * cin + cout + b)
    x = torch.randn(b, h * w, cin, generator=g, device=DEV).to(torch.bfloat16)
    wt = torch.randn(cout, cin, 3, 3, generator=g, device=DEV) / (9 * cin) ** 0.5
    bias = torch.randn(cout, generator=g, device=DEV) * 0.05
    with torch.no_grad():
        got = ops.vae_enc_conv_out(x, ops.pack_vae_enc_conv_out_weight(wt), ops.bias_f32(bias), b, h, w, cout)
        one = ops.vae_enc_conv_out(x[-1:].contiguous(), ops.pack_vae_enc_conv_out_weight(wt), ops.bias_f32(bias), 1, h, w, cout)
    xin = x.float().view(b, h, w, cin).permute(0, 3, 1, 2)
    with _fp32_exact():
        want = F.conv2d(xin, wt, bias, padding=1)
        bound = F.conv2d(xin.abs(), wt.abs(), bias.abs(), padding=1) * 1e-5 + 1e-6
    assert got.shape == (b, cout, h, w) and got.dtype == torch.float32
    assert ((got - want).abs() <= bound).all()
    assert torch.equal(got[-1:], one)  # an image's output does not depend on the batch


# ----------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("case,cfg", [("sdxl", SDXL_DDCONFIG), ("narrow", NARROW_DDCONFIG), ("ragged", NARROW_DDCONFIG)])
def test_encoder_against_reference_golden(case, cfg):
    d = np.load(os.path.join(GOLD, "vae_encoder.npz"))
    enc, _ = _encoder(cfg)
    with torch.no_grad():
        out = enc(torch.from_numpy(d[f"x.{case}"]).to(DEV))
    want = torch.from_numpy(d[f"out.{case}"])
    assert out.shape == want.shape and out.dtype == torch.float32
    assert torch.isfinite(out).all()
    assert _rel(out.cpu(), want) < TOL, case


@pytest.fixture(scope="module")
def sdxl():
    enc, sd = _encoder(SDXL_DDCONFIG)
    return enc, {k: v.to(DEV) for k, v in sd.items()}


@pytest.mark.parametrize("hw", [512, 1024])
def test_encoder_full_size_against_fp32_restatement(sdxl, hw):
    enc, sd = sdxl
    x = W.tensor(f"x{hw}", (1, 3, hw, hw), seed=1).to(DEV)
    with torch.no_grad():
        out = enc(x)
        with _fp32_exact():
            want = vae_enc_fp32.encode(sd, x, SDXL_DDCONFIG["ch_mult"], 2)
    assert out.shape == (1, 8, hw // 8, hw // 8) and torch.isfinite(out).all()
    rel = _rel(out, want)
    print(f"encoder {hw}^2: max relative error against fp32 {rel:.3e}")
    assert rel < TOL, hw


def test_batch_of_three_equals_each_image_alone(sdxl):
    enc, _ = sdxl
    x = W.tensor("xb", (3, 3, 256, 256), seed=2).to(DEV)
    with torch.no_grad():
        both = enc(x)
        for i in range(3):
            assert torch.equal(both[i:i + 1], enc(x[i:i + 1])), i


def test_bf16_parameters_and_stale_pack(sdxl):
    _, sd = sdxl
    enc, _ = _encoder(SDXL_DDCONFIG, dtype=torch.bfloat16)
    sd16 = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
    x = W.tensor("x256", (1, 3, 256, 256), seed=3).to(DEV)
    with torch.no_grad():
        out = enc(x.to(torch.bfloat16))
        assert out.dtype == torch.bfloat16 and out.shape == (1, 8, 32, 32)
        with _fp32_exact():
            want = vae_enc_fp32.encode(sd16, x.to(torch.bfloat16).float(), SDXL_DDCONFIG["ch_mult"], 2)
        assert _rel(out, want) < TOL
        before = enc(x).float()
        w = enc.down[1].downsample.conv.weight
        w.copy_(w * 0.5)  # bumps _version, as load_state_dict does
        after = enc(x).float()
    assert (after - before).abs().max().item() > 1e-2


def test_forward_hook_sees_real_values(sdxl):
    enc, _ = sdxl
    seen = []
    conv = enc.down[1].downsample.conv
    hk = enc.down[1].downsample.register_forward_hook(lambda m, i, o: seen.append((i[0].float().clone(), o.float().clone())))
    try:
        with torch.no_grad():
            enc(W.tensor("xh", (2, 3, 128, 128), seed=4).to(DEV))
    finally:
        hk.remove()
    # one image per pass: the hook fires once per image, on the level-1 activation (256 channels at 64^2) and its downsampled output
    assert len(seen) == 2
    for inp, out in seen:
        assert inp.shape == (1, 256, 64, 64) and out.shape == (1, 256, 32, 32)
        assert 0 < inp.abs().max().item() < float("inf")
        ref, A = _down_ref(inp, conv.weight.to(torch.bfloat16).float(), conv.bias.float())
        _assert_close(out, ref, A, "hooked Downsample")


def test_autoencoder_encode_call_shape(sdxl):
    """AutoencoderKL.encode: the Encoder, then quant_conv (a framework 1x1 conv 8 -> 8), then the posterior's moments chunk(2, 1)."""
    enc, sd = sdxl
    qc = torch.nn.Conv2d(8, 8, 1).to(DEV)
    with torch.no_grad():
        qc.weight.copy_(W.tensor("qc.w", (8, 8, 1, 1), seed=3).to(DEV) * 0.5)
        qc.bias.copy_(W.tensor("qc.b", (8,), seed=3).to(DEV) * 0.05)
        x = W.tensor("xe", (1, 3, 512, 384), seed=5).to(DEV)
        mean, logvar = qc(enc(x)).chunk(2, 1)
        with _fp32_exact():
            want_mean, want_logvar = qc(vae_enc_fp32.encode(sd, x, SDXL_DDCONFIG["ch_mult"], 2)).chunk(2, 1)
    assert mean.shape == (1, 4, 64, 48) and logvar.shape == (1, 4, 64, 48)
    assert torch.isfinite(mean).all() and torch.isfinite(logvar).all()
    assert _rel(mean, want_mean) < TOL and _rel(logvar, want_logvar) < TOL


def test_image_beyond_32_bit_offsets_raises(sdxl):
    enc, _ = sdxl
    x = torch.zeros(1, 3, 4096, 4096, device=DEV)  # level-0 activation 4096^2 x 128 x 2 bytes = 4 GiB
    with torch.no_grad(), pytest.raises(ops.Cd360Error):
        enc(x)
