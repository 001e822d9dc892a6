"""From a sampling job to images, the parts that need no GPU: include/cd360_image.h against its signature table, the numpy restatement of
the two new noise counters, the `sample_images` job over gloo with stand-ins, and the host-side refusals of the four ops wrappers."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import image_cases as IC
import philox_ref as P
import sampler_cases as SC


# ================================================================================================ 1: header and table
def test_image_header_matches_the_sixth_signature_table():
    """include/cd360_image.h <=> cd360._lib.IMAGE_SIGNATURES by the rule of test_library_exports_every_declared_symbol (every `cd360_...(`
    word, comments included); the library exports the four symbols, typed; no older table holds the new names and no older header names
    them; null pointers are refused on the host."""
    from cd360 import _lib
    mismatch, in_tables, in_headers, mistyped, lib = SC.check_header_matches_table("cd360_image.h", _lib.IMAGE_SIGNATURES, IC.NEW, IC.OLDER)
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    assert list(_lib.ABI)[-1] == "cd360_image.h" and tuple(list(_lib.ABI)[:-1]) == IC.OLDER
    nul = ctypes.c_void_p(None)
    assert lib.cd360_start_noise_f32(nul, nul, nul, nul, 1, 16, nul) == -1
    assert lib.cd360_posterior_sample_f32(nul, nul, nul, nul, nul, nul, 0.13025, nul, 1, 16, nul) == -1
    assert lib.cd360_post_quant_f32(nul, nul, nul, 1.0, nul, 1, 16, nul) == -1
    assert lib.cd360_vae_conv_out_u8(nul, nul, nul, nul, 1, 4, 4, 64, 3, nul) == -1


# ================================================================================================ 2: the two new counters
def test_domain_words_give_unrelated_draws_with_sound_statistics():
    """Domain 0 of image_cases.normals is philox_ref.normals (the step noise, unchanged).  For the same (seed, stream, step) the domains 0,
    1 and 2 give different Philox words at every pixel and uncorrelated normals, and the normals of domains 1 and 2 pass
    philox_ref.check_statistics: moments at five standard errors, no correlation between steps, streams, neighbouring seeds, channels and
    pixels.  The known answer: counter (0, 0, 0, 1) under key 0 is not the all-zero counter's output."""
    hw = 257
    for seed in (30, 2 ** 63 + 12345):
        for stream, step in ((0, 0), (3, 2)):
            assert np.array_equal(IC.normals(seed, stream, step, hw, IC.DOMAIN_STEP), P.normals(seed, stream, step, hw))
            w = [np.stack(IC.words(seed, stream, step, hw, d)) for d in (0, 1, 2)]
            for a in range(3):
                for b in range(a + 1, 3):
                    assert not (w[a] == w[b]).all(0).any(), (seed, stream, step, a, b)  # no pixel draws the same four words
    assert tuple(int(v[0]) for v in IC.words(0, 0, 0, 1, 0)) == P.KAT[0][2]
    assert tuple(int(v[0]) for v in IC.words(0, 0, 0, 1, 1)) != P.KAT[0][2]
    for domain in (IC.DOMAIN_START, IC.DOMAIN_POSTERIOR):
        worst = P.check_statistics(lambda seed, stream, step: IC.normals(seed, stream, step, P.STAT_HW, domain))
        print("domain %d, worst figures: mean %.2e var %.2e m4 %.3f, correlation %.2f standard errors"
              % (domain, worst["mean"], worst["var"], worst["m4"], worst["corr"]))
    z = [IC.normals(30, 0, 0, P.STAT_HW, d) for d in (0, 1, 2)]
    for a in range(3):
        for b in range(a + 1, 3):
            assert abs(P.corr(z[a], z[b])) <= 5.0 / np.sqrt(z[a].size), (a, b)


def test_restated_start_noise_and_posterior():
    """The two expressions on the counters: the start latent is z * scale in domain 1 at step word 0, equal rows for equal stream ids; the
    posterior is (mean + exp(0.5 clamp(lv, -30, 20)) z) * scale_factor in domain 2 with the step word = draw, and mean * scale_factor
    without a seed."""
    hw = 35
    sc = np.float32(14.6146)
    x = IC.start_noise(30, [0, 3, 0], hw, sc)
    assert x.shape == (3, 4, hw) and np.array_equal(x[0], x[2]) and not np.array_equal(x[0], x[1])
    assert np.array_equal(x[1], IC.normals(30, 3, 0, hw, IC.DOMAIN_START) * float(sc))
    g = np.random.default_rng(5)
    mom = g.standard_normal((2, 8, hw)).astype(np.float32)
    w = np.eye(8, dtype=np.float32)
    b = np.zeros(8, np.float32)
    mom[:, 4:, :5], mom[:, 4:, 5:9] = -40.0, 25.0
    sf = np.float32(IC.SCALE_FACTOR)
    mode, lv = IC.posterior(mom, w, b, None, None, None, sf)
    assert np.array_equal(mode, mom[:, :4].astype(np.float64) * float(sf)) and np.array_equal(lv, mom[:, 4:].astype(np.float64))
    s0, _ = IC.posterior(mom, w, b, 30, [0, 1], 0, sf)
    s1, _ = IC.posterior(mom, w, b, 30, [0, 1], 1, sf)
    assert not np.array_equal(s0, s1)
    z = IC.normals(30, 1, 0, hw, IC.DOMAIN_POSTERIOR)
    std = np.exp(0.5 * np.clip(mom[1, 4:].astype(np.float64), -30, 20))
    assert np.allclose(s0[1], (mom[1, :4] + std * z) * float(sf), rtol=1e-15, atol=0)
    assert np.allclose(std[:, :5], np.exp(-15.0)) and np.allclose(std[:, 5:9], np.exp(10.0))


# ================================================================================================ 3: the job over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _CpuSampler:
    """Stand-in with the Sampler protocol of cd360/job.py (retarget / step) on CPU tensors, as in tests/test_shard_gloo.py."""

    def __init__(self, pose, ctx, y):
        self.retarget(pose, ctx, y)

    def retarget(self, pose, ctx, y):
        self.k = float(pose) + float(ctx.sum()) * 1e-3 + float(y.sum()) * 1e-4

    def step(self, x, i):
        return x * 0.5 + self.k * 0.1 + 0.01 * i


class _CpuFirstStage:
    """Stand-in first stage: a 2 x nearest 'decoder' on three of the four channels with the image epilogue of sample.py:346."""

    def decode_u8(self, z):
        img = torch.nn.functional.interpolate(z[:, :3] * 0.7 - z[:, 3:4] * 0.2, scale_factor=2, mode="nearest")
        return (torch.clip(img * 0.5 + 0.5, 0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _job_of(p):
    g = torch.Generator().manual_seed(50 + p)
    return (p, torch.randn(3, 7, generator=g), torch.randn(3, 5, generator=g), torch.randn(1, 4, 8, 8, generator=g))


def _job_worker(rank, world, port, num_poses, steps, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "custom-diffusion360_amd"))
    from cd360 import job
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    images, mine = job.sample_images(_CpuSampler, _job_of, num_poses, steps, _CpuFirstStage(), world, rank)
    try:  # fewer poses than ranks: refused from the arguments alone, so on EVERY rank and before any collective
        job.sample_images(_CpuSampler, _job_of, world - 1, steps, _CpuFirstStage(), world, rank)
        refused = False
    except ValueError:
        refused = True
    q.put((rank, mine, images, refused))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sample_images_job_gathers_identical_uint8_images_on_every_rank(world):
    """cd360.job.sample_images with a CPU stand-in sampler and first stage over gloo, 4 poses on 2 ranks (2 + 2) and on 3 ranks (2 + 1 + 1:
    the per-rank counts differ, so the all-gather pads): every rank ends with the uint8 images of ALL poses in pose order, equal to the
    world-1 run; num_poses < world raises on every rank."""
    from cd360 import job
    num_poses, steps = 4, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_job_worker, args=(r, world, port, num_poses, steps, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want, all_mine = job.sample_images(_CpuSampler, _job_of, num_poses, steps, _CpuFirstStage())
    assert all_mine == list(range(num_poses)) and want.shape == (num_poses, 16, 16, 3) and want.dtype == torch.uint8
    assert len({bytes(want[p].numpy().tobytes()) for p in range(num_poses)}) == num_poses  # the poses' images differ
    assert 0 < int((want > 0).sum()) and int((want == 255).sum()) < want.numel()  # not saturated either way
    assert sum((m for _, m, _, _ in res), []) == list(range(num_poses))
    assert len({len(m) for _, m, _, _ in res}) == (1 if num_poses % world == 0 else 2)
    for rank, _, images, refused in res:
        assert images.dtype == torch.uint8 and images.shape == want.shape and torch.equal(images, want), rank
        assert refused, rank
    with pytest.raises(ValueError):
        job.sample_images(_CpuSampler, _job_of, 1, steps, _CpuFirstStage(), world=2, rank=1)
    with pytest.raises(ValueError):  # x0 = None needs the latent's size
        job.sample_images(_CpuSampler, lambda p: _job_of(p)[:3] + (None,), 2, steps, _CpuFirstStage())


# ================================================================================================ 4: host-side refusals
@pytest.fixture
def no_library(monkeypatch):
    """The refusals below happen before the library is touched: loading it fails the test."""
    from cd360 import _lib

    def load(check_symbols=True):
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "load", load)


def _f(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def test_start_noise_refuses_bad_arguments(no_library):
    from cd360 import ops
    seed, scale, streams = torch.zeros(1, dtype=torch.int64), _f(1), torch.zeros(2, dtype=torch.int32)
    for kw in (dict(seed=seed.int()), dict(seed=torch.zeros(2, dtype=torch.int64)), dict(scale=scale.double()), dict(scale=_f(2)),
               dict(streams=streams.long()), dict(streams=torch.zeros(3, dtype=torch.int32)), dict(bs=0), dict(H=0), dict(W=-1)):
        args = dict(dict(seed=seed, streams=streams, scale=scale, bs=2, H=5, W=7), **kw)
        with pytest.raises(ValueError):
            ops.start_noise(**args)
    with pytest.raises(ops.Cd360Error):  # sound arguments on the host: no CPU implementation
        ops.start_noise(seed, streams, scale, 2, 5, 7)


def test_posterior_sample_refuses_bad_arguments(no_library):
    from cd360 import ops
    mom, w, b = _f(2, 8, 5, 7), _f(8, 8), _f(8)
    seed, draw, streams = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    buf = _f(2 * 12 * 35)
    over_m, over_o = buf[:2 * 8 * 35].view(2, 8, 5, 7), buf[2 * 8 * 35 - 4:2 * 8 * 35 - 4 + 2 * 4 * 35].view(2, 4, 5, 7)
    bad = (dict(moments=_f(2, 4, 5, 7)), dict(moments=_f(2, 16, 5, 7)), dict(moments=_f(8, 5, 7)), dict(moments=mom.double()),
           dict(moments=mom.half()), dict(moments=_f(2, 8, 7, 5).transpose(2, 3)), dict(w=_f(4, 8)), dict(w=_f(8, 8, 1, 1)), dict(w=w.double()),
           dict(bias=_f(4)), dict(bias=b.half()), dict(seed=seed.int()), dict(draw=None), dict(draw=draw.long()),
           dict(streams=torch.zeros(3, dtype=torch.int32)), dict(streams=streams.long()), dict(out=_f(2, 8, 5, 7)), dict(out=_f(2, 4, 5, 7).double()),
           dict(out=_f(2, 4, 7, 5)), dict(moments=over_m, out=over_o), dict(moments=mom, out=mom[:1].view(2, 4, 5, 7)))
    for kw in bad:
        args = dict(dict(moments=mom, w=w, bias=b, seed=seed, streams=streams, draw=draw, scale_factor=0.13025), **kw)
        with pytest.raises(ValueError):
            ops.posterior_sample(**args)
    for seed_ in (seed, None):
        with pytest.raises(ops.Cd360Error):
            ops.posterior_sample(mom, w, b, seed_, None, draw, 0.13025)


def test_post_quant_refuses_bad_arguments(no_library):
    from cd360 import ops
    z, w, b = _f(2, 4, 5, 7), _f(4, 4), _f(4)
    buf = _f(2 * 2 * 4 * 35)
    over_z, over_o = buf[:2 * 4 * 35].view(2, 4, 5, 7), buf[2 * 4 * 35 - 1:4 * 4 * 35 - 1].view(2, 4, 5, 7)
    bad = (dict(z=_f(2, 8, 5, 7)), dict(z=_f(2, 3, 5, 7)), dict(z=_f(4, 5, 7)), dict(z=z.double()), dict(z=z.bfloat16()),
           dict(z=_f(2, 4, 7, 5).transpose(2, 3)), dict(w=_f(8, 8)), dict(w=_f(4, 4, 1, 1)), dict(w=w.half()), dict(bias=_f(8)), dict(bias=b.double()),
           dict(out=z), dict(out=_f(2, 4, 5, 8)), dict(out=_f(2, 4, 5, 7).half()), dict(z=over_z, out=over_o))
    for kw in bad:
        args = dict(dict(z=z, w=w, bias=b, inv_scale=1 / 0.13025), **kw)
        with pytest.raises(ValueError):
            ops.post_quant(**args)
    with pytest.raises(ops.Cd360Error):
        ops.post_quant(z, w, b, 1 / 0.13025)


def test_vae_conv_out_u8_refuses_bad_arguments(no_library):
    from cd360 import ops
    n, h, wd, cin = 1, 5, 7, 64
    x = torch.zeros(n, h * wd, cin, dtype=torch.bfloat16)
    wp, b = _f(9, cin, 4), _f(3)
    raw = torch.zeros(n * h * wd * cin * 2, dtype=torch.uint8)
    over_x, over_o = raw.view(torch.bfloat16).view(n, h * wd, cin), raw[8:8 + n * h * wd * 3].view(n, h, wd, 3)
    bad = (dict(cout=0), dict(cout=5), dict(cout=4), dict(x=x.float()), dict(x=torch.zeros(n, h * wd, 96, dtype=torch.bfloat16)),
           dict(x=torch.zeros(n, h * wd + 1, cin, dtype=torch.bfloat16)), dict(w_packed=_f(9, cin, 3)), dict(w_packed=_f(9, 128, 4)),
           dict(w_packed=wp.half()), dict(bias=_f(4)), dict(bias=b.double()), dict(N=0), dict(H=0),
           dict(out=torch.zeros(n, 3, h, wd, dtype=torch.uint8)), dict(out=torch.zeros(n, h, wd, 3, dtype=torch.int8)),
           dict(out=torch.zeros(n, h, wd, 3)), dict(x=over_x, out=over_o))
    for kw in bad:
        args = dict(dict(x=x, w_packed=wp, bias=b, N=n, H=h, W=wd, cout=3), **kw)
        with pytest.raises(ValueError):
            ops.vae_conv_out_u8(**args)
    with pytest.raises(ops.Cd360Error):
        ops.vae_conv_out_u8(x, wp, b, n, h, wd, 3)


def test_first_stage_refuses_other_convolutions_and_host_tensors():
    """FirstStage takes the reference's two 1 x 1 nn.Conv2d modules (8 -> 8 and 4 -> 4); anything else is refused when it is built.  A host
    tensor raises, as in sgm.modules.diffusionmodules.model."""
    from cd360 import images, ops
    qc, pqc = torch.nn.Conv2d(8, 8, 1), torch.nn.Conv2d(4, 4, 1)
    for bad_q, bad_p in ((torch.nn.Conv2d(8, 8, 3, padding=1), pqc), (torch.nn.Conv2d(6, 6, 1), pqc), (qc, torch.nn.Conv2d(4, 3, 1)),
                         (qc, torch.nn.Linear(4, 4))):
        with pytest.raises(ValueError):
            images.FirstStage(None, None, bad_q, bad_p)
    fs = images.FirstStage(None, None, qc, pqc)
    assert fs.scale_factor == 0.13025
    w, b = images._conv1x1_pack(qc, 8, 8)
    assert w.shape == (8, 8) and w.dtype == torch.float32 and images._conv1x1_pack(qc, 8, 8)[0] is w  # packed once
    with torch.no_grad():
        qc.weight.mul_(2.0)
    assert images._conv1x1_pack(qc, 8, 8)[0] is not w  # an in-place edit repacks
    for call in (lambda: fs.decode(torch.zeros(1, 4, 8, 8)), lambda: fs.decode_u8(torch.zeros(1, 4, 8, 8)),
                 lambda: fs.encode(torch.zeros(1, 3, 64, 64), 0, 0), lambda: fs.encode_mode(torch.zeros(1, 3, 64, 64))):
        with pytest.raises(ops.Cd360Error):
            call()
