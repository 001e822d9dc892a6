"""Masked and image-to-image sampling without a GPU: the second library's header <=> table <=> exports, counter domain 3, the plain-torch
blend against numpy fp32, the sampler classes honouring `mask` / `init_im`, the host-side refusals and the partial walk of the job."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import edit_cases as EC
import image_cases as IC
import philox_ref as P
import sampler_cases as SC


# ================================================================================================ 1: header, table, library
def test_edit_header_matches_its_table_and_the_first_library_is_closed():
    """include/edit/cd360_edit.h <=> cd360._edit.EDIT_SIGNATURES <=> libcd360_edit.so (every `cd360_...(` word, comments included); neither
    name is in a table of cd360._lib.ABI, in a header of include/*.h or exported by libcd360_hip.so; _lib.ABI is the six headers it was,
    each table holding exactly its header's names; null pointers and a mask of 2 rows for 3 samples are refused on the host."""
    from cd360 import _edit, _lib
    mismatch, in_tables, in_headers, mistyped, lib = SC.check_library_matches_table(EC.LIBRARY)
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    assert tuple(_lib.ABI) == IC.OLDER + ("cd360_image.h",)
    for header, table in _lib.ABI.items():
        assert set(re.findall(r"\b(cd360_[a-z0-9_]+)\s*\(", SC.header_text(header))) == set(table), header
    assert "EDIT_SIGNATURES" not in vars(_lib)
    first = _lib.load(check_symbols=True)
    for name in EC.NEW:
        assert not hasattr(first, name), name
    src = open(_edit.__file__).read()
    assert "os.environ" not in src and "getenv" not in src  # the binding reads no environment variable
    nul, p = ctypes.c_void_p(None), [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(7)]
    assert lib.cd360_edit_noise_f32(nul, nul, nul, nul, 1, 16, nul) == -1
    assert lib.cd360_mask_blend_f32(nul, nul, nul, 1, nul, 0, nul, nul, nul, 1, 16, nul) == -1
    x, known, mask, sig, step, seed, streams = p
    for missing in range(6):  # streams may be null: never reached, an earlier argument is
        args = [nul if i == missing else v for i, v in enumerate((x, known, mask, sig, step, seed))]
        assert lib.cd360_mask_blend_f32(args[0], args[1], args[2], 1, args[3], 0, args[4], args[5], nul, 1, 16, nul) == -1, missing
    assert lib.cd360_mask_blend_f32(x, known, mask, 2, sig, 0, step, seed, streams, 3, 16, nul) == -1  # mask_rows outside {1, bs}
    assert lib.cd360_mask_blend_f32(x, known, mask, 1, sig, -4, step, seed, streams, 3, 16, nul) == -1
    assert lib.cd360_mask_blend_f32(x, known, mask, 1, sig, 0, step, seed, streams, 0, 16, nul) == -1
    assert lib.cd360_mask_blend_f32(x, known, mask, 1, sig, 0, step, seed, streams, 1, 2 ** 32 + 1, nul) == -1
    assert lib.cd360_mask_blend_f32(x, x, mask, 1, sig, 0, step, seed, streams, 1, 16, nul) == -1  # x overlapping known
    assert lib.cd360_mask_blend_f32(x, known, ctypes.c_void_p(0x10000 + 64), 1, sig, 0, step, seed, streams, 1, 16, nul) == -1  # ... mask


def test_edit_kernels_are_recorded_without_scratch():
    """build() leaves the new object's resource record where test_no_kernel_keeps_a_stack_object_in_scratch_memory reads it: both kernels,
    no scratch, no spill."""
    import json
    rec = json.load(open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "lib", "obj", "mask_blend.o.resources.json")))
    assert len(rec) == 2 and any("mask_blend_kernel" in k for k in rec) and any("edit_noise_kernel" in k for k in rec), sorted(rec)
    for name, r in rec.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


# ================================================================================================ 2: counter domain 3
def test_domain_3_is_unrelated_to_the_older_domains_with_sound_statistics():
    """For the same (seed, stream, step) domain 3 shares no pixel's four Philox words with domains 0, 1 and 2, its normals pass
    philox_ref.check_statistics and are uncorrelated with theirs at five standard errors (the bar of test_images_cpu.py)."""
    hw = 257
    for seed in (30, 2 ** 63 + 12345):
        for stream, step in ((0, 0), (3, 2)):
            w3 = np.stack(IC.words(seed, stream, step, hw, EC.DOMAIN_EDIT))
            for d in (0, 1, 2):
                assert not (w3 == np.stack(IC.words(seed, stream, step, hw, d))).all(0).any(), (seed, stream, step, d)
    worst = P.check_statistics(lambda seed, stream, step: EC.normals(seed, stream, step, P.STAT_HW))
    print("domain 3, worst figures: mean %.2e var %.2e m4 %.3f, correlation %.2f standard errors"
          % (worst["mean"], worst["var"], worst["m4"], worst["corr"]))
    z3 = EC.normals(30, 0, 0, P.STAT_HW)
    for d in (0, 1, 2):
        assert abs(P.corr(z3, IC.normals(30, 0, 0, P.STAT_HW, d))) <= 5.0 / np.sqrt(z3.size), d


# ================================================================================================ 3: the blend in plain torch
@pytest.mark.parametrize("hw", [1, 35, 257])
@pytest.mark.parametrize("bs,rows", [(1, 1), (3, 1), (3, 3)])
def test_masked_blend_equals_the_numpy_fp32_expression(hw, bs, rows):
    """cd360.sampler.masked_blend on CPU: m = 1 returns x, m = 0 returns known + noise sigma_next, sigma_next = 0 adds no noise term, and a
    fractional mask is bit-equal to the numpy fp32 expression of include/edit/cd360_edit.h."""
    from cd360.sampler import masked_blend
    g = torch.Generator().manual_seed(hw * 10 + bs + rows)
    x, known, z = (torch.randn(bs, 4, 1, hw, generator=g) for _ in range(3))
    m = torch.rand(rows, 1, 1, hw, generator=g)
    s = torch.tensor(2.7182817)
    nx, nk, nz = (t.numpy().reshape(bs, 4, hw) for t in (x, known, z))

    def np_of(t):
        return t.numpy().reshape(t.shape[0], t.shape[1], hw)

    assert torch.equal(masked_blend(x, known, torch.ones_like(m), s, z), x)
    kn = masked_blend(x, known, torch.zeros_like(m), s, z)
    assert np.array_equal(np_of(kn), (nk + (nz * np.float32(s)).astype(np.float32)).astype(np.float32))
    assert torch.equal(masked_blend(x, known, torch.zeros_like(m), torch.tensor(0.0), z), known)
    got0 = masked_blend(x, known, m, torch.zeros(1), torch.full_like(z, float("nan")))  # the noise is not read into the result
    assert np.array_equal(np_of(got0), EC.blend(nx, nk, np_of(m), 0.0, nz))
    for sig in (s, s.reshape(1), s.expand(bs)):
        assert np.array_equal(np_of(masked_blend(x, known, m, sig, z)), EC.blend(nx, nk, np_of(m), float(s), nz))


# ================================================================================================ 4: the sampler classes
def _network(x_in, c_noise, cond, **kw):
    pred = 0.3 * torch.tanh(x_in) + 0.0001 * c_noise.float().view(-1, 1, 1, 1) + 0.1 * cond["crossattn"].float().mean((1, 2)).view(-1, 1, 1, 1)
    return pred, [], [], [torch.zeros(x_in.shape[0], 4, 3)]


def _stand_in(cls, steps=6):
    from cd360 import sampler as S
    den = S.DiscreteDenoiser()
    smp = getattr(S, cls)(num_steps=steps, device="cpu")
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 4, 6, 5, generator=g)
    init = torch.randn(2, 4, 6, 5, generator=g)
    cond = {"crossattn": torch.randn(2, 3, 8, generator=g), "vector": torch.randn(2, 7, generator=g)}
    return smp, (lambda inp, s, cc: den(_network, inp, s, cc)), x, init, cond


def _as_before(smp, denoiser, x, cond):
    """EulerEDMSampler.__call__ as it was before it read `mask` / `init_im`."""
    x, s_in, sigmas, num_sigmas, cond, uc = smp.prepare_sampling_loop(x, cond, None, None)
    for i in range(num_sigmas - 1):
        x, _ = smp.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc, smp.gamma_of(sigmas[i], num_sigmas - 1))
    return x


@pytest.mark.parametrize("cls", ["EulerEDMSampler", "HeunEDMSampler"])
def test_sampler_classes_honour_mask_and_init_im(cls):
    """mask=None walks the trajectory it walked; a mask of ones (under one manual seed) is bit-equal to it; with a half mask the kept
    half ends as init_im exactly (the last sigma_next is 0) and the generated half is not init_im; a mask without init_im, or the reverse,
    or of another shape, raises."""
    smp, denoiser, x, init, cond = _stand_in(cls)
    want = _as_before(smp, denoiser, x.clone(), cond)
    plain, _ = smp(denoiser, x.clone(), cond)
    assert torch.equal(plain, want)
    ones = torch.ones(1, 1, 6, 5)
    torch.manual_seed(3)
    full, _ = smp(denoiser, x.clone(), cond, mask=ones, init_im=init)
    assert torch.equal(full, want)
    half = ones.clone()
    half[..., :3, :] = 0.0
    torch.manual_seed(3)
    got, _ = smp(denoiser, x.clone(), cond, mask=half, init_im=init)
    assert torch.equal(got[..., :3, :], init[..., :3, :])
    assert not torch.equal(got[..., 3:, :], init[..., 3:, :]) and torch.isfinite(got).all()
    assert torch.equal(got[..., 3:, :], want[..., 3:, :])  # (the stand-in network is pointwise: the generated half is the unmasked run's)
    per_sample = half.expand(2, 1, 6, 5).contiguous()
    torch.manual_seed(3)
    assert torch.equal(smp(denoiser, x.clone(), cond, mask=per_sample, init_im=init)[0], got)
    for kw in (dict(mask=half), dict(init_im=init), dict(mask=half[..., :2], init_im=init), dict(mask=half, init_im=init[:, :3])):
        with pytest.raises(ValueError):
            smp(denoiser, x.clone(), cond, **kw)
    seeded = type(smp)(num_steps=6, device="cpu", seed=5)
    with pytest.raises(Exception, match="HIP kernel"):  # seed=<int>: the library's generator, GPU tensors only
        seeded(denoiser, x.clone(), cond, mask=half, init_im=init)


# ================================================================================================ 5: host-side refusals
@pytest.fixture
def no_library(monkeypatch):
    """The refusals below happen before either library is touched: loading one fails the test."""
    from cd360 import _edit, _lib

    def load(*a, **kw):
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "load", load)
    monkeypatch.setattr(_edit, "load", load)


def _f(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def test_ops_refuse_bad_arguments(no_library):
    from cd360 import ops
    seed, step = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    good = dict(x=_f(3, 4, 5, 7), known=_f(3, 4, 5, 7), mask=_f(3, 1, 5, 7), sigma_next=_f(4, 4), step=step, seed=seed, streams=None)
    x = _f(3, 4, 5, 7)
    bad = [dict(x=_f(3, 3, 5, 7)), dict(x=x.double()), dict(x=_f(3, 4, 7, 5).transpose(2, 3)), dict(known=_f(3, 4, 5, 8)), dict(known=_f(3, 4, 5, 7).half()),
           dict(mask=_f(2, 1, 5, 7)), dict(mask=_f(3, 4, 5, 7)), dict(mask=_f(3, 1, 5, 7).bool()), dict(sigma_next=_f(4, 3)), dict(sigma_next=_f(2)),
           dict(sigma_next=_f(1).double()), dict(step=step.long()), dict(seed=seed.int()), dict(streams=torch.zeros(2, dtype=torch.int32)),
           dict(streams=torch.zeros(3, dtype=torch.int64)), dict(x=x, known=x), dict(x=x, mask=x[:, :1])]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.mask_blend(**dict(good, **kw))
    for args in ((seed, None, step, 0, 5, 7), (seed.int(), None, step, 1, 5, 7), (seed, None, step.long(), 1, 5, 7),
                 (seed, torch.zeros(2, dtype=torch.int32), step, 1, 5, 7)):
        with pytest.raises(ValueError):
            ops.edit_noise(*args)
    with pytest.raises(ops.Cd360Error):  # everything else in order: a CPU tensor is refused by the device check
        ops.mask_blend(**good)
    with pytest.raises(ops.Cd360Error):
        ops.edit_noise(seed, None, step, 1, 5, 7)


class _Schedule:
    def __init__(self, n, solver=None):
        self.sigmas, self.bs, self.solver = torch.linspace(10.0, 0.0, n + 1), 1, solver


def test_job_refuses_bad_arguments(no_library):
    """The argument checks of Sampler(known=, mask=) / set_known, of a partial start and of start_from, on the host."""
    from cd360 import job
    known, mask = _f(2, 4, 5, 7), _f(2, 1, 5, 7)
    job.check_known(2, None, None)
    job.check_known(2, known, mask)
    job.check_known(2, known, mask[:1], (2, 4, 5, 7))
    for k, m, shape in ((known, None, None), (None, mask, None), (_f(3, 4, 5, 7), mask, None), (_f(2, 3, 5, 7), mask, None), (known.double(), mask, None),
                        (known, _f(2, 1, 5, 8), None), (known, _f(2, 4, 5, 7), None), (known, mask.bool(), None), (known, _f(3, 1, 5, 7), None),
                        (known, mask, (2, 4, 6, 7)), (known[0], mask, None)):
        with pytest.raises(ValueError):
            job.check_known(2, k, m, shape)
    assert job.Sampler.PARTIAL_START == ("euler", "heun", "euler_a", "dpmpp2s_a")
    for solver in job.Sampler.PARTIAL_START + (None,):
        job.check_first_step(solver, 2, 4)
    for solver in ("dpmpp2m", "lms"):
        job.check_first_step(solver, 0, 4)
        with pytest.raises(ValueError) as e:
            job.check_first_step(solver, 2, 4)
        assert all(name in str(e.value) for name in job.Sampler.PARTIAL_START) and "churn" in str(e.value)
        with pytest.raises(ValueError):
            job.sample_assigned(_Schedule(4, solver), [], 4, first_step=2)
    for row in (-1, 4, True, 1.0):
        with pytest.raises(ValueError):
            job.check_first_step("euler", row, 4)
    for k in (0, 4, -1, True):
        with pytest.raises(ValueError):
            job.start_from(_Schedule(4), _f(1, 4, 5, 7), k, seed=1)
    with pytest.raises(ValueError):
        job.start_from(_Schedule(4), _f(1, 3, 5, 7), 2, seed=1)
    with pytest.raises(ValueError):
        job.start_from(_Schedule(4), _f(1, 4, 5, 7), 2, seed=1, streams=[0, 1])
    fs = type("FS", (), {"decode_u8": staticmethod(lambda z: z)})()
    for kw in (dict(masks=_f(1, 1, 8, 8)), dict(init_latents=_f(3, 4, 8, 8), masks=_f(1, 1, 8, 8)), dict(init_latents=_f(1, 4, 8, 8), masks=_f(3, 1, 8, 8)),
               dict(first_step=4), dict(first_step=2)):  # (the last: x0 = None and nothing to start from)
        with pytest.raises(ValueError):
            job.sample_images(lambda *a: _Schedule(4), lambda p: (p, None, None, None), 2, 4, fs, **kw)


def test_latent_mask_is_the_area_average():
    from cd360.images import latent_mask
    m = torch.zeros(2, 1, 16, 24, dtype=torch.bool)
    m[0, 0, :8, :12] = True  # latent pixels (0, 0) whole, (0, 1) half
    m[1] = True
    for form in (m, m.to(torch.uint8) * 255, m.float(), m[:, 0], m[:, 0].to(torch.uint8)):
        got = latent_mask(form)
        assert got.shape == (2, 1, 2, 3) and got.dtype == torch.float32 and got.is_contiguous()
        assert got[0, 0].tolist() == [[1.0, 0.5, 0.0], [0.0, 0.0, 0.0]] and bool((got[1] == 1.0).all())
    assert latent_mask(torch.full((1, 1, 4, 4), 0.25), factor=4).item() == 0.25
    for bad in (torch.zeros(2, 3, 16, 16), torch.zeros(16, 16), torch.zeros(1, 1, 12, 16)):
        with pytest.raises(ValueError):
            latent_mask(bad)


# ================================================================================================ 6: the partial walk over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _CpuSampler:
    """Stand-in with the Sampler protocol of cd360/job.py (retarget / step) on CPU tensors, as in tests/test_images_cpu.py; it notes the rows
    it is asked for."""
    rows = []

    def __init__(self, pose, ctx, y):
        self.retarget(pose, ctx, y)

    def retarget(self, pose, ctx, y):
        self.k = float(pose) + float(ctx.sum()) * 1e-3 + float(y.sum()) * 1e-4

    def step(self, x, i):
        _CpuSampler.rows.append(i)
        return x * 0.5 + self.k * 0.1 + 0.01 * (i + 1) ** 2


class _CpuFirstStage:
    def decode_u8(self, z):
        img = torch.nn.functional.interpolate(z[:, :3] * 0.7 - z[:, 3:4] * 0.2, scale_factor=2, mode="nearest")
        return (torch.clip(img * 0.5 + 0.5, 0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _job_of(p):
    g = torch.Generator().manual_seed(50 + p)
    return (p, torch.randn(3, 7, generator=g), torch.randn(3, 5, generator=g), torch.randn(1, 4, 8, 8, generator=g))


def _job_worker(rank, world, port, num_poses, steps, first_step, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "custom-diffusion360_amd"))
    from cd360 import job
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    images, mine = job.sample_images(_CpuSampler, _job_of, num_poses, steps, _CpuFirstStage(), world, rank, first_step=first_step)
    q.put((rank, mine, images, list(_CpuSampler.rows)))
    dist.barrier()
    dist.destroy_process_group()


def test_sample_images_walks_the_rows_from_first_step_only():
    """cd360.job.sample_images(first_step=2) with a CPU stand-in over gloo, 3 poses on 2 ranks, 4 steps: every pose is stepped through rows
    2 and 3 and no other, and every rank ends with the images of rows 2, 3 applied by hand to each pose's start latent."""
    from cd360 import job
    num_poses, steps, first_step, world = 3, 4, 2, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_job_worker, args=(r, world, port, num_poses, steps, first_step, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    finals = []
    for p in range(num_poses):
        pose, c, y, x = _job_of(p)
        smp = _CpuSampler(pose, c, y)
        for i in (2, 3):
            x = smp.step(x, i)
        finals.append(x)
    want = torch.cat([_CpuFirstStage().decode_u8(x) for x in finals], 0)
    _CpuSampler.rows.clear()
    whole, _ = job.sample_images(_CpuSampler, _job_of, num_poses, steps, _CpuFirstStage())
    assert _CpuSampler.rows == [0, 1, 2, 3] * num_poses and not torch.equal(whole, want)
    _CpuSampler.rows.clear()
    one, mine = job.sample_images(_CpuSampler, _job_of, num_poses, steps, _CpuFirstStage(), first_step=first_step)
    assert mine == list(range(num_poses)) and _CpuSampler.rows == [2, 3] * num_poses and torch.equal(one, want)
    assert sum((m for _, m, _, _ in res), []) == list(range(num_poses))
    for rank, mine, images, rows in res:
        assert rows == [2, 3] * len(mine), (rank, rows)
        assert images.dtype == torch.uint8 and torch.equal(images, want), rank
    latents, _ = job.sample_poses(_CpuSampler, _job_of, num_poses, steps, first_step=first_step)
    assert torch.equal(latents, torch.cat(finals, 0))
