"""From a sampling job to images on the HIP kernels of include/cd360_image.h: the start noise and the posterior sample against their float64
restatements (tests/image_cases.py), the two affine parts and the uint8 epilogue bit for bit against torch restatements, `FirstStage` on
the narrow first stage, the `sample_images` job, and every entry point under tests/guarded.py.  Needs an MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as G
import image_cases as IC
import sampler_cases as SC
import weights as W
from sampler_cases import BF, DEV, LATENT, POSES, SEED, STEPS, R, seed_t, step_t, streams_t

BIG_SEED = 2 ** 63 + 12345
TOL = 2.5e-2  # the module bar of test_vae_gpu.py
SDXL_DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                     ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
NARROW_DDCONFIG = dict(SDXL_DDCONFIG, resolution=64, ch=64, ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[16])
SF32 = np.float32(IC.SCALE_FACTOR)  # scale_factor as the kernel receives it


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _start_scale():
    """sqrt(1 + sigma_0^2) of the 50-step LegacyDDPM schedule, by torch exactly as sampling.py:50 computes it: a 1-element fp32 tensor."""
    from cd360 import sampler as S
    sig = S.LegacyDDPMDiscretization()(50)
    return torch.sqrt(1.0 + sig[0] ** 2.0).reshape(1).to(DEV)


# ================================================================================================ 1: start noise
@pytest.mark.gpu
@pytest.mark.parametrize("H,Wd", [(5, 7), (16, 16)])
def test_start_noise_equals_the_float64_restatement(H, Wd):
    """cd360_start_noise_f32 at bs = 2 against image_cases.start_noise in float64 (counter (px, 0, stream, 1), z * scale): seeds 30 and
    2^63 + 12345, streams null and [0, 3].  Bar, by the rule of test_noise_kernel_equals_the_float64_restatement: 4 x what the SAME
    expression evaluated in float32 by numpy gives against float64 on the same inputs.  Rows of equal stream id are bit-equal, rows of
    different ids differ, a row does not depend on bs, and the draw is not the step noise of the same seed (domain 0)."""
    from cd360 import ops
    bs, hw = 2, H * Wd
    scale = _start_scale()
    sc = np.float32(scale.item())
    assert 14.0 < float(sc) < 15.0
    for seed in (30, BIG_SEED):
        for ids in (None, [0, 3]):
            got = ops.start_noise(seed_t(seed), streams_t(ids), scale, bs, H, Wd)
            assert got.shape == (bs, 4, H, Wd) and got.dtype == torch.float32
            rows = [0] * bs if ids is None else ids
            want = IC.start_noise(seed, rows, hw, sc)
            bar = 4 * float(np.abs(IC.start_noise(seed, rows, hw, sc, np.float32) - want).max())
            err = float(np.abs(_np64(got).reshape(bs, 4, hw) - want).max())
            print(f"start noise {bs}x4x{H}x{Wd} seed {seed} streams {ids}: max |kernel - float64| {err:.3e} | bar {bar:.3e}")
            assert err <= bar, (seed, ids, err, bar)
            assert torch.equal(got[0], got[1]) == (rows[0] == rows[1]), (seed, ids)
            for r in range(bs):  # the matching row of bs = 1 and of bs = 3
                one = ops.start_noise(seed_t(seed), streams_t([rows[r]]), scale, 1, H, Wd)
                three = ops.start_noise(seed_t(seed), streams_t([7, rows[r], 9]), scale, 3, H, Wd)
                assert torch.equal(one[0], got[r]) and torch.equal(three[1], got[r]), (seed, ids, r)
            step = ops.sampler_noise(seed_t(seed), streams_t(ids), step_t(0), bs, H, Wd) * scale
            assert not torch.equal(step, got)
    assert not torch.equal(ops.start_noise(seed_t(30), None, scale, bs, H, Wd), ops.start_noise(seed_t(31), None, scale, bs, H, Wd))


# ================================================================================================ 2: post-quant
def _affine(t, w, b):
    """One 1 x 1 convolution in the kernels' order, one fp32 rounding per operation (torch's elementwise kernels do not contract):
    t [B, N, H, W], w [O, N], b [O] -> [B, O, H, W]."""
    rows = []
    for o in range(w.shape[0]):
        acc = w[o, 0] * t[:, 0]
        for i in range(1, w.shape[1]):
            acc = acc + w[o, i] * t[:, i]
        rows.append(acc + b[o])
    return torch.stack(rows, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (1, 4, 16, 16)])
def test_post_quant_equals_a_torch_restatement_in_the_kernels_order(shape):
    """cd360_post_quant_f32: bit-equal to t = z * inv_scale, out_o = (((w_o0 t_0 + w_o1 t_1) + w_o2 t_2) + w_o3 t_3) + b_o evaluated
    operation by operation in fp32, and within fp32 summation slack of F.conv2d(z * (1 / 0.13025), w, b): the conv2d of the absolute
    values x 1e-5 + 1e-6, the bound of test_conv_out_against_conv2d."""
    from cd360 import ops
    z = R(*shape, seed=shape[2])
    w, b = R(4, 4, seed=2) * 0.5, R(4, seed=3) * 0.05
    inv = 1 / 0.13025
    got = ops.post_quant(z, w, b, inv)
    assert got.shape == z.shape and got.dtype == torch.float32
    want = _affine(z * inv, w, b)
    assert torch.equal(got, want), float((got - want).abs().max())
    zin = z * inv
    ref = F.conv2d(zin, w.reshape(4, 4, 1, 1), b)
    bound = F.conv2d(zin.abs(), w.abs().reshape(4, 4, 1, 1), b.abs()) * 1e-5 + 1e-6
    assert ((got - ref).abs() <= bound).all(), float(((got - ref).abs() / bound).max())
    into = torch.full_like(z, float("nan"))
    assert ops.post_quant(z, w, b, inv, out=into) is into and torch.equal(into, want)


# ================================================================================================ 3: posterior
def _posterior_inputs(shape):
    """Moments whose logvar rows m_4..7 spread at a standard deviation of about 15: some below -30, some above 20, most between."""
    mom = R(*shape, seed=shape[2] + 1)
    w = R(8, 8, seed=5) * 0.35
    b = R(8, seed=6) * 0.05
    w[4:] *= 15.0
    return mom, w, b


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 8, 5, 7), (1, 8, 16, 16)])
def test_posterior_sample_equals_the_float64_restatement(shape):
    """cd360_posterior_sample_f32 against image_cases.posterior in float64 on the float64 restated noise (counter (px, draw, stream, 2)).
    Bar: 4 x what the SAME expression evaluated in float32 by numpy gives against float64 on the same inputs, computed here and printed.
    The logvar rows hold all three classes (below -30, above 20, between).  The affine part is compared bit for bit through the mode()
    form against a torch restatement in the stated order.  draw 0 and 1 differ; a NULL seed ignores streams and draw."""
    from cd360 import ops
    B, _, H, Wd = shape
    hw = H * Wd
    mom, w, b = _posterior_inputs(shape)
    m = _affine(mom, w, b)
    lv = m[:, 4:]
    n_lo, n_hi, n_mid = int((lv < -30).sum()), int((lv > 20).sum()), int(((lv >= -30) & (lv <= 20)).sum())
    print(f"posterior {shape}: logvar rows below -30: {n_lo}, above 20: {n_hi}, between: {n_mid}")
    assert n_lo > 0 and n_hi > 0 and n_mid > n_lo + n_hi, (n_lo, n_hi, n_mid)
    mode = ops.posterior_sample(mom, w, b, None, None, None, float(SF32))
    assert mode.shape == (B, 4, H, Wd) and torch.equal(mode, m[:, :4] * float(SF32)), float((mode - m[:, :4] * float(SF32)).abs().max())
    junk = torch.tensor([123], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.posterior_sample(mom, w, b, None, streams_t([5] * B), junk, float(SF32)), mode)
    mom_n, w_n, b_n = (t.cpu().numpy() for t in (mom.reshape(B, 8, hw), w, b))
    for seed in (30, BIG_SEED):
        for ids in (None, list(range(2, 2 + B))):
            rows = [0] * B if ids is None else ids
            res = {}
            for draw in (0, 1):
                got = ops.posterior_sample(mom, w, b, seed_t(seed), streams_t(ids), step_t(draw), float(SF32))
                want, _ = IC.posterior(mom_n, w_n, b_n, seed, rows, draw, SF32)
                bar = 4 * float(np.abs(IC.posterior(mom_n, w_n, b_n, seed, rows, draw, SF32, np.float32)[0] - want).max())
                err = float(np.abs(_np64(got).reshape(B, 4, hw) - want).max())
                print(f"posterior {shape} seed {seed} streams {ids} draw {draw}: max |kernel - float64| {err:.3e} | bar {bar:.3e} | max |value| {np.abs(want).max():.3e}")
                assert torch.isfinite(got).all() and err <= bar, (seed, ids, draw, err, bar)
                res[draw] = got
            assert not torch.equal(res[0], res[1]) and not torch.equal(res[0], mode)
            if B == 2:
                for r in range(B):  # an image's sample depends on its stream id, not on the batch
                    one = ops.posterior_sample(mom[r:r + 1].contiguous(), w, b, seed_t(seed), streams_t([rows[r]]), step_t(0), float(SF32))
                    assert torch.equal(one[0], res[0][r]), (seed, ids, r)


# ================================================================================================ 4: uint8 out
U8_SHAPES = [(1, 17, 23, 128, 3), (2, 33, 40, 320, 3), (1, 17, 23, 128, 4)]  # ragged last workgroup | two weight chunks + the batch | cout 4


def _u8_inputs(n, h, w, cin, cout):
    x = R(n, h * w, cin, seed=w + cout, dtype=BF)
    wt = R(cout, cin, 3, 3, seed=h) * (1.3 / (9 * cin) ** 0.5)  # outputs of standard deviation ~ 1.3: well beyond [-1, 1] both ways
    b = R(cout, seed=cin) * 0.05
    return x, wt, b


def _image_chain(f):
    """sample.py:346 on the fp32 NCHW output, as torch evaluates it -> uint8 NHWC."""
    return (torch.clip(f * 0.5 + 0.5, 0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,cin,cout", U8_SHAPES)
def test_conv_out_u8_is_exactly_the_image_chain_of_the_fp32_output(n, h, w, cin, cout):
    """cd360_vae_conv_out_u8 == (torch.clip(f * 0.5 + 0.5, 0, 1) * 255).to(torch.uint8), permuted to HWC, of the fp32 output f that
    cd360_vae_conv_out_bf16 writes on the same inputs -- exactly.  f spans beyond [-1, 1]: values < -1, > 1 and inside (-1, 1) each make
    up at least a tenth."""
    from cd360 import ops
    x, wt, b = _u8_inputs(n, h, w, cin, cout)
    wp = ops.pack_vae_conv_out_weight(wt)
    f = ops.vae_conv_out(x, wp, b, n, h, w, cout)
    frac = [float((f < -1).float().mean()), float((f > 1).float().mean()), float(((f > -1) & (f < 1)).float().mean())]
    print(f"u8 {n}x{h}x{w}x{cin} -> {cout}: share of f below -1 / above 1 / inside: {frac[0]:.3f} / {frac[1]:.3f} / {frac[2]:.3f}")
    assert min(frac) >= 0.1, frac
    got = ops.vae_conv_out_u8(x, wp, b, n, h, w, cout)
    want = _image_chain(f)
    assert got.shape == (n, h, w, cout) and got.dtype == torch.uint8 and got.is_contiguous()
    assert torch.equal(got, want), int((got != want).sum())
    assert int((got == 0).sum()) > 0 and int((got == 255).sum()) > 0 and int(((got > 0) & (got < 255)).sum()) > 0
    nob = ops.vae_conv_out_u8(x, wp, None, n, h, w, cout)  # bias is optional, as for the fp32 form
    assert torch.equal(nob, _image_chain(ops.vae_conv_out(x, wp, None, n, h, w, cout)))


@pytest.mark.gpu
def test_conv_out_u8_writes_zero_for_a_nan_and_leaves_the_rest():
    """One NaN input pixel makes the fp32 output NaN at the 3 x 3 output pixels that read it (NaN * w, whatever w).  Those write 0 in every
    channel; every other byte is the clean run's."""
    from cd360 import ops
    n, h, w, cin, cout = 1, 17, 23, 128, 3
    x, wt, b = _u8_inputs(n, h, w, cin, cout)
    wp = ops.pack_vae_conv_out_weight(wt)
    clean = ops.vae_conv_out_u8(x, wp, b, n, h, w, cout)
    py, px = 9, 11
    xn = x.clone()
    xn[0, py * w + px, 5] = float("nan")
    f = ops.vae_conv_out(xn, wp, b, n, h, w, cout)
    bad = torch.isnan(f).permute(0, 2, 3, 1)
    assert int(bad.sum()) == 9 * cout and bool(bad[0, py - 1:py + 2, px - 1:px + 2].all())
    got = ops.vae_conv_out_u8(xn, wp, b, n, h, w, cout)
    assert bool((got[bad] == 0).all()) and int((clean[bad] != 0).sum()) > 0
    assert torch.equal(got[~bad], clean[~bad])


# ================================================================================================ 5: FirstStage
def _first_stage():
    """FirstStage on the narrow first stage with tests/golden/weights.py weights and fp32 parameters."""
    from cd360 import images
    from sgm.modules.diffusionmodules.model import Decoder, Encoder
    enc, dec = Encoder(**NARROW_DDCONFIG).eval(), Decoder(**NARROW_DDCONFIG).eval()
    W.load_into(enc, 3)
    W.load_into(dec, 3)
    qc, pqc = torch.nn.Conv2d(8, 8, 1), torch.nn.Conv2d(4, 4, 1)
    with torch.no_grad():
        qc.weight.copy_(W.tensor("qc.w", (8, 8, 1, 1), seed=3) * 0.35)
        qc.bias.copy_(W.tensor("qc.b", (8,), seed=3) * 0.05)
        pqc.weight.copy_(W.tensor("pqc.w", (4, 4, 1, 1), seed=3) * 0.5)
        pqc.bias.copy_(W.tensor("pqc.b", (4,), seed=3) * 0.05)
    mods = [m.to(DEV) for m in (enc, dec, qc, pqc)]
    for m in mods:
        for p in m.parameters():
            p.requires_grad_(False)
    return images.FirstStage(*mods), mods


@pytest.fixture(scope="module")
def first_stage():
    return _first_stage()


def _rel(got, want):
    return (got.float() - want.float()).abs().max().item() / want.float().abs().max().item()


@pytest.mark.gpu
@torch.no_grad()
def test_first_stage_decode_and_decode_u8(first_stage):
    """decode(z) against dec(pqc(z / 0.13025)) -- the call shape of test_autoencoder_decode_call_shape, post_quant_conv a framework
    convolution -- at the module bar TOL, on that file's ragged latent [1, 4, 25, 19]; decode_u8(z) is exactly the torch chain applied to
    decode(z); a batch of 2 gives each image the bits it gets alone."""
    fs, (enc, dec, qc, pqc) = first_stage
    z = W.tensor("zs", (2, 4, 25, 19), seed=5).to(DEV)
    img = fs.decode(z[:1])
    want = dec(pqc(z[:1] / 0.13025))
    assert img.shape == (1, 3, 100, 76) and img.dtype == torch.float32 and torch.isfinite(img).all()
    rel = _rel(img, want)
    print("FirstStage.decode vs dec(pqc(z / 0.13025)): max rel", rel, "| bar", TOL, "| image range", float(img.min()), float(img.max()))
    assert rel < TOL
    u8 = fs.decode_u8(z[:1])
    assert u8.shape == (1, 100, 76, 3) and u8.dtype == torch.uint8 and torch.equal(u8, _image_chain(img))
    assert int((u8 > 0).sum()) > 0 and int((u8 < 255).sum()) > 0
    both, both_u8 = fs.decode(z), fs.decode_u8(z)
    other, other_u8 = fs.decode(z[1:]), fs.decode_u8(z[1:])
    assert torch.equal(both[0], img[0]) and torch.equal(both[1], other[0]) and not torch.equal(both[0], both[1])
    assert torch.equal(both_u8[0], u8[0]) and torch.equal(both_u8[1], other_u8[0]) and torch.equal(both_u8, _image_chain(both))


@pytest.mark.gpu
@torch.no_grad()
def test_first_stage_encode(first_stage):
    """encode(x, seed, draw, streams) against (mean + std * z_restated) * 0.13025 in float64 from the Encoder's own moments output, at the
    posterior bar (4 x the numpy float32 evaluation of the same expression); encode_mode is the mean; a batch of 2 gives each image the
    bits it gets alone; draw and seed change the sample."""
    fs, (enc, dec, qc, pqc) = first_stage
    x = W.tensor("img", (2, 3, 64, 64), seed=7).to(DEV)
    moments = enc(x).float()
    B, _, h, w = moments.shape
    assert (B, h, w) == (2, 16, 16)
    mom_n = moments.cpu().numpy().reshape(B, 8, h * w)
    w_n, b_n = qc.weight.detach().cpu().numpy().reshape(8, 8), qc.bias.detach().cpu().numpy()
    seed, draw, ids = BIG_SEED, 4, [1, 6]
    got = fs.encode(x, seed, draw, ids)
    want, _ = IC.posterior(mom_n, w_n, b_n, seed, ids, draw, SF32)
    bar = 4 * float(np.abs(IC.posterior(mom_n, w_n, b_n, seed, ids, draw, SF32, np.float32)[0] - want).max())
    err = float(np.abs(_np64(got).reshape(B, 4, h * w) - want).max())
    print(f"FirstStage.encode vs float64 on the Encoder's moments: max abs {err:.3e} | bar {bar:.3e} | max |value| {np.abs(want).max():.3e}")
    assert got.shape == (B, 4, h, w) and got.dtype == torch.float32 and err <= bar, (err, bar)
    mode = fs.encode_mode(x)
    assert torch.equal(mode, _affine(moments, qc.weight.reshape(8, 8), qc.bias)[:, :4] * float(SF32))
    for r in range(B):
        assert torch.equal(fs.encode(x[r:r + 1], seed, draw, [ids[r]])[0], got[r]) and torch.equal(fs.encode_mode(x[r:r + 1])[0], mode[r])
    assert not torch.equal(fs.encode(x, seed, draw + 1, ids), got) and not torch.equal(fs.encode(x, seed + 1, draw, ids), got)
    assert torch.equal(fs.encode(x, seed, draw), fs.encode(x, seed, draw, [0, 0]))  # default: stream 0 for every image


# ================================================================================================ 6: the job
@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_job():
    yield
    SC.release()


@pytest.mark.gpu
@torch.no_grad()
def test_sample_images_is_the_decode_of_sample_poses_from_the_start_latent(first_stage):
    """The tiny UNet and poses of sampler_cases, 3 poses, 4 steps, world 1, the narrow decoder: sample_images (x0 = None: the start
    latent drawn on the device from the seed) is exactly decode_u8 of sample_poses run from start_latent's x0; a second call with the
    same seed gives the same bytes after torch.manual_seed was changed in between; another seed gives other bytes.  One captured sampler
    serves every call (Euler keeps nothing between images)."""
    from cd360 import job as J
    fs, _ = first_stage
    held = {}

    def make_sampler(pose, ctx, y):
        if "smp" not in held:
            held["smp"] = SC.sampler(pose, ctx, y)
        else:
            held["smp"].retarget(pose, ctx, y)
        return held["smp"]

    no_x0 = lambda p: SC.job(p)[:3] + (None,)  # noqa: E731
    torch.manual_seed(1)
    images, mine = J.sample_images(make_sampler, no_x0, POSES, STEPS, fs, seed=SEED, latent_hw=(LATENT, LATENT))
    assert mine == list(range(POSES)) and images.shape == (POSES, 4 * LATENT, 4 * LATENT, 3) and images.dtype == torch.uint8
    x0 = J.start_latent(held["smp"], LATENT, LATENT, SEED)
    assert x0.shape == (1, 4, LATENT, LATENT) and 10.0 < float(x0.std()) < 20.0  # randn * sqrt(1 + sigma_0^2), sigma_0 = 14.6
    latents, _ = J.sample_poses(make_sampler, lambda p: SC.job(p)[:3] + (x0,), POSES, STEPS)
    assert torch.isfinite(latents).all()
    want = fs.decode_u8(latents)
    assert torch.equal(images, want), int((images != want).sum())
    assert not torch.equal(images[0], images[1]) and int((images > 0).sum()) > 0 and int((images < 255).sum()) > 0
    torch.manual_seed(2)
    torch.randn(7, device=DEV)
    again, _ = J.sample_images(make_sampler, no_x0, POSES, STEPS, fs, seed=SEED, latent_hw=(LATENT, LATENT))
    assert torch.equal(again, images)
    other, _ = J.sample_images(make_sampler, no_x0, POSES, STEPS, fs, seed=SEED + 1, latent_hw=(LATENT, LATENT))
    assert not torch.equal(other, images)
    assert torch.equal(J.start_latent(held["smp"], LATENT, LATENT, SEED, streams=[0]), x0)
    assert not torch.equal(J.start_latent(held["smp"], LATENT, LATENT, SEED, streams=[1]), x0)


# ================================================================================================ 7: guarded runs
GUARDED = [  # (id, declares, kind, shape): what test_every_image_entry_point_has_a_guarded_case reads
    ("start-noise-2x4x5x7", ["cd360_start_noise_f32"], "start", (2, 5, 7)),
    ("start-noise-1x4x16x16", ["cd360_start_noise_f32"], "start", (1, 16, 16)),
    ("posterior-2x8x5x7", ["cd360_posterior_sample_f32"], "posterior", (2, 8, 5, 7)),
    ("posterior-1x8x16x16", ["cd360_posterior_sample_f32"], "posterior", (1, 8, 16, 16)),
    ("post-quant-2x4x5x7", ["cd360_post_quant_f32"], "post_quant", (2, 4, 5, 7)),
    ("post-quant-1x4x16x16", ["cd360_post_quant_f32"], "post_quant", (1, 4, 16, 16)),
    ("u8-ragged-1x17x23x128-cout3", ["cd360_vae_conv_out_u8"], "u8", (1, 17, 23, 128, 3)),
    ("u8-2x33x40x320-cout3", ["cd360_vae_conv_out_u8"], "u8", (2, 33, 40, 320, 3)),
    ("u8-ragged-1x17x23x128-cout4", ["cd360_vae_conv_out_u8"], "u8", (1, 17, 23, 128, 4)),
]


def _arena_copy(guard, t):
    """t's values in an arena block between canaries (an operand the kernel must not write, and must not read beyond)."""
    g = guard.torch.empty(tuple(t.shape), dtype=t.dtype, device=t.device)
    g.copy_(t)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("declares,kind,shape", [c[1:] for c in GUARDED], ids=[c[0] for c in GUARDED])
def test_image_entry_points_write_their_outputs_only(declares, kind, shape):
    """Every launching entry point of include/cd360_image.h under tests/guarded.py, both poison patterns: operands and outputs live in
    arena blocks between canaries.  No guard byte changes (the 3-byte pixel pitch of the ragged uint8 shape is where a stray dword store
    would show); every output is fully written (bit-equal between the poisons, finite where it is a float); every operand is unchanged."""
    from cd360 import ops
    if kind == "start":
        bs, H, Wd = shape
        d = dict(seed=seed_t(BIG_SEED), streams=streams_t(list(range(1, bs + 1))), scale=_start_scale())

        @SC.guardfn
        def fn(seed, streams, scale, guard):
            return ops.start_noise(_arena_copy(guard, seed), _arena_copy(guard, streams), _arena_copy(guard, scale), bs, H, Wd)

        out, _ = G.run_twice(fn, d, declares=declares)
        assert out.shape == (bs, 4, H, Wd) and float(out.abs().max()) > 1.0
    elif kind == "posterior":
        mom, w, b = _posterior_inputs(shape)
        B = shape[0]
        d = dict(mom=mom, w=w, b=b, seed=seed_t(30), streams=streams_t(list(range(B))), draw=step_t(2))

        @SC.guardfn
        def fn(mom, w, b, seed, streams, draw, guard):
            gm, gw, gb = (_arena_copy(guard, t) for t in (mom, w, b))
            gs, gst, gd = (_arena_copy(guard, t) for t in (seed, streams, draw))
            smp = ops.posterior_sample(gm, gw, gb, gs, gst, gd, float(SF32))
            mode = ops.posterior_sample(gm, gw, gb, None, None, None, float(SF32))
            assert torch.equal(gm, mom) and torch.equal(gw, w) and torch.equal(gb, b), "an operand was written"
            return smp, mode

        (smp, mode), _ = G.run_twice(fn, d, declares=declares)
        assert torch.equal(mode, _affine(mom, w, b)[:, :4] * float(SF32)) and not torch.equal(smp, mode)
    elif kind == "post_quant":
        z, w, b = R(*shape, seed=1), R(4, 4, seed=2) * 0.5, R(4, seed=3) * 0.05
        d = dict(z=z, w=w, b=b)

        @SC.guardfn
        def fn(z, w, b, guard):
            gz, gw, gb = (_arena_copy(guard, t) for t in (z, w, b))
            out = ops.post_quant(gz, gw, gb, 1 / 0.13025)
            assert torch.equal(gz, z) and torch.equal(gw, w) and torch.equal(gb, b), "an operand was written"
            return out

        out, _ = G.run_twice(fn, d, declares=declares)
        assert torch.equal(out, _affine(z * (1 / 0.13025), w, b))
    else:
        n, h, wd, cin, cout = shape
        x, wt, b = _u8_inputs(n, h, wd, cin, cout)
        wp = ops.pack_vae_conv_out_weight(wt)
        d = dict(x=x, wp=wp, b=b)

        @SC.guardfn
        def fn(x, wp, b, guard):
            gx, gw, gb = (_arena_copy(guard, t) for t in (x, wp, b))
            out = ops.vae_conv_out_u8(gx, gw, gb, n, h, wd, cout)
            assert torch.equal(gx, x) and torch.equal(gw, wp) and torch.equal(gb, b), "an operand was written"
            return out

        out, _ = G.run_twice(fn, d, declares=declares)
        assert out.dtype == torch.uint8 and torch.equal(out, _image_chain(ops.vae_conv_out(x, wp, b, n, h, wd, cout)))


def test_every_image_entry_point_has_a_guarded_case():
    """The twin of test_every_stochastic_entry_point_has_a_guarded_case for include/cd360_image.h (runs without a GPU): every
    `int cd360_...(` the header declares is in some guarded case's `declares` in this file, and is typed in IMAGE_SIGNATURES."""
    from cd360 import _lib
    untyped, unknown, uncovered = SC.check_guarded_cover("cd360_image.h", _lib.IMAGE_SIGNATURES, GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"
