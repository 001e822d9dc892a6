"""What tests/test_train_stage_cpu.py, tests/test_train_stage_gpu.py and tests/golden/make_train_stage_golden.py share (plain helper module,
like textgrad_cases.py; no tests, no fixtures): the names include/train/cd360_train.h adds, and a numpy restatement of its four entry
points -- every operation in the header's order, once, in the dtype the caller names: np.float64 is the yardstick of the kernels,
np.float32 the same expression in the kernels' precision on the host, which sizes their bars and reproduces the reference's own fp32
arithmetic (tests/golden/train_stage.npz).  Built on philox_ref.philox4x32_10 / box_muller with the counter's domain word passed in.

Indices are integers defined by fp32 arithmetic (the cubic index, the nearest table entry): they are formed in fp32 whatever `dtype` is."""
import os

import numpy as np

import philox_ref as PR

HEADER = os.path.join("train", "cd360_train.h")
NEW = ["cd360_train_sigmas_f32", "cd360_train_noise_f32", "cd360_train_l2_f32", "cd360_train_l2_bwd_f32"]
KERNELS = ("train_sigmas_kernel", "train_noise_kernel", "train_l2_kernel", "train_l2_bwd_kernel")
BUILD_ROW = ("libcd360_train.so", "csrc_train", ["train_stage.hip"], "_train")
# the guarded cases of tests/test_train_stage_gpu.py::test_train_entry_points_write_their_outputs_only: (id, entry points the case must reach)
GUARDED = [("sigmas", ["cd360_train_sigmas_f32"]), ("noise-both-dtypes", ["cd360_train_sigmas_f32", "cd360_train_noise_f32"]),
           ("l2-forward-backward", ["cd360_train_l2_f32", "cd360_train_l2_bwd_f32"])]
ROW = 12
SIGMA, W, C_SKIP, C_OUT, C_IN, SIGMA_REF, C_IN_REF, OFF_TGT, OFF_REF = range(9)
CUBIC, DISCRETE = 0, 1
DOMAIN_SIGMA, DOMAIN_TARGET, DOMAIN_REF_A, DOMAIN_REF_B = 4, 5, 6, 7
F32 = np.float32


def legacy_table(n):
    """LegacyDDPMDiscretization()(n, do_append_zero=False, flip=True) as fp32 numpy: the table of the shipped samplers and denoiser."""
    from cd360 import sampler as S
    return S.LegacyDDPMDiscretization()(n, do_append_zero=False, flip=True).numpy().astype(F32)


def words(seed, streams, step, B):
    """[B, 4] uint32: the domain-4 draw of every row, counter (0, step, stream, 4)."""
    streams = [0] * B if streams is None else list(streams)
    r = PR.philox4x32_10((0, int(step) & PR.MASK, np.asarray(streams, np.int64) & PR.MASK, DOMAIN_SIGMA), PR.key_of(seed))
    return np.stack([np.broadcast_to(v, (B,)) for v in r], 1)


def uniform24(r):
    """(r >> 8) 2^-24 in [0, 1): exact in fp32 -- the value torch.rand would have to return."""
    return ((np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(F32)


def sample_index(kind, r, num_idx, start):
    r = np.asarray(r, np.uint32)
    if kind == CUBIC:
        u = uniform24(r)
        return ((F32(1.0) - u * u * u) * F32(num_idx - 1)).astype(np.int64)
    return start + (r.astype(np.int64) % (num_idx - start))


def sigma_to_idx(sigma, table):
    """DiscreteDenoiser.sigma_to_idx in fp32: the first minimum of |sigma - table|."""
    return np.abs(np.asarray(sigma, F32)[None, :] - np.asarray(table, F32)[:, None]).argmin(0).astype(np.int64)


def normals4(seed, stream, step, word, domain, dtype):
    """[4, len(word)]: the four channels' normals at pixel words `word` of one noise stream."""
    r = PR.philox4x32_10((np.asarray(word, np.uint64), int(step) & PR.MASK, int(stream) & PR.MASK, domain), PR.key_of(seed))
    z0, z1 = PR.box_muller(r[0], r[1], dtype)
    z2, z3 = PR.box_muller(r[2], r[3], dtype)
    return np.stack([z0, z1, z2, z3])


def restate(dtype, *, seed, streams, step, table, tgt_table, tgt_kind, tgt_start, ref_table, ref_kind, ref_start, level, x0, xr=None, drop=None,
            eps=None, mask=None, g=None):
    """(a)-(d) of include/train/cd360_train.h in `dtype`, in the header's order -> dict.  x0 [B, 4, H, W]; xr [B, n, 4, H, W] | None; drop [B] |
    None; eps [B, 4, H, W] | None (then no loss); mask [B, 1, H, W] | None; g [B] | None (the gradient of the loss; then d_eps too).
    Inputs are fp32 values (eps possibly bf16-rounded ones) converted to `dtype`; nothing is rounded to bf16 here."""
    dt = np.dtype(dtype).type
    x0 = np.asarray(x0, F32)
    B, _, H, Wd = x0.shape
    HW = H * Wd
    strm = [0] * B if streams is None else [int(s) for s in streams]
    # ---- a) the scalars
    r = words(seed, strm, step, B)
    tgt_idx = sample_index(tgt_kind, r[:, 0], len(tgt_table), tgt_start)
    ref_idx = sample_index(ref_kind, r[:, 1], len(ref_table), ref_start)
    sigma32, sigma_ref32 = np.asarray(tgt_table, F32)[tgt_idx], np.asarray(ref_table, F32)[ref_idx]
    sigma, sigma_ref = sigma32.astype(dt), sigma_ref32.astype(dt)
    off_tgt, off_ref = PR.box_muller(r[:, 2], r[:, 3], dtype)
    rows = np.zeros((B, ROW), dt)
    rows[:, SIGMA], rows[:, W], rows[:, C_SKIP], rows[:, C_OUT] = sigma, dt(1.0) / (sigma * sigma), dt(1.0), -sigma
    rows[:, C_IN] = dt(1.0) / np.sqrt(sigma * sigma + dt(1.0))
    rows[:, SIGMA_REF], rows[:, C_IN_REF] = sigma_ref, dt(1.0) / np.sqrt(sigma_ref * sigma_ref + dt(1.0))
    rows[:, OFF_TGT], rows[:, OFF_REF] = off_tgt, off_ref
    out = dict(rows=rows, tgt_idx=tgt_idx, ref_sampler_idx=ref_idx, timesteps=sigma_to_idx(sigma32, table), sigmas_ref_idx=sigma_to_idx(sigma_ref32, table),
               step_used=np.int64(step), u=uniform24(r[:, 0]), words=r)
    # ---- b) the bulk pass
    lv = dt(level)
    bc = lambda v: v.reshape(B, 1, 1, 1)
    z = np.stack([normals4(seed, strm[b], step, np.arange(HW), DOMAIN_TARGET, dtype) for b in range(B)]).reshape(B, 4, H, Wd)
    zp = z + lv * bc(off_tgt) if level > 0 else z
    x_t = x0.astype(dt) + zp * bc(sigma)
    out.update(z=z, x_t=x_t, x_in=x_t * bc(rows[:, C_IN]))
    if xr is not None:
        xr = np.asarray(xr, F32).astype(dt)
        n = xr.shape[1]
        za, zb = (np.stack([normals4(seed, strm[b], step, np.arange(n * HW), d, dtype).reshape(4, n, H, Wd).transpose(1, 0, 2, 3) for b in range(B)])
                  for d in (DOMAIN_REF_A, DOMAIN_REF_B))
        b5 = lambda v: v.reshape(B, 1, 1, 1, 1)
        xr0 = b5(np.asarray(drop, F32).astype(dt)) * xr if drop is not None else xr
        zap = za + lv * b5(off_ref) if level > 0 else za
        xr1 = xr0 + zap * b5(sigma_ref)
        xr2 = xr1 + zb * b5(sigma_ref)
        out.update(z_a=za, z_b=zb, xr_in=xr2 * b5(rows[:, C_IN_REF]))
    # ---- c), d) the l2 term and its gradient
    if eps is not None:
        e = np.asarray(eps, F32).astype(dt)
        err = (e * bc(rows[:, C_OUT]) + x_t * bc(rows[:, C_SKIP])) - x0.astype(dt)
        t = bc(rows[:, W]) * (err * err)
        if mask is not None:
            m = np.asarray(mask, F32).astype(dt)
            t = t * m
            den = m.reshape(B, -1).sum(1, dtype=dt) + dt(1e-6)
        else:
            m, den = None, np.full((B,), 4 * HW, dt)
        out.update(err=err, den=den, loss=t.reshape(B, -1).sum(1, dtype=dt) / den)
        if g is not None:
            d = (dt(2.0) * bc(rows[:, W])) * err
            d = d * bc(rows[:, C_OUT])
            if m is not None:
                d = d * m
            d = d / bc(den)
            gb = bc(np.asarray(g, F32).astype(dt))
            out["d_eps"] = np.where(gb == 0, dt(0.0), gb * d)
    return out


def shipped(level=0.0):
    """The samplers and the denoiser table of the shipped config (configs/train_co3d_concept.yaml:119-134): CubicSampling over the 1000-entry
    legacy table, DiscreteSampling over its 50-entry one, DiscreteDenoiser on the 1000-entry one."""
    t1000, t50 = legacy_table(1000), legacy_table(50)
    return dict(table=t1000, tgt_table=t1000, tgt_kind=CUBIC, tgt_start=0, ref_table=t50, ref_kind=DISCRETE, ref_start=0, level=level)


def ulps(a, b):
    """The largest distance between fp32 arrays a and b in units in the last place of b."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)).max()) if a.size else 0.0
