"""What tests/test_images_cpu.py and tests/test_images_gpu.py share (plain helper module, like philox_ref.py and sampler_cases.py; no
tests, no fixtures): the numpy restatement of the two noise counters include/cd360_image.h adds (domain word 1 = the start of a trajectory,
2 = the posterior sample) on tests/philox_ref.py's Philox and Box-Muller, and of the two expressions built on them, in any precision."""
import numpy as np

import philox_ref as P

NEW = ["cd360_start_noise_f32", "cd360_posterior_sample_f32", "cd360_post_quant_f32", "cd360_vae_conv_out_u8"]
OLDER = ("cd360_hip.h", "cd360_solvers.h", "cd360_stochastic.h", "cd360_edm.h", "cd360_highorder.h")
DOMAIN_STEP, DOMAIN_START, DOMAIN_POSTERIOR = 0, 1, 2
SCALE_FACTOR = 0.13025


def words(seed, stream, step, hw, domain):
    """The four Philox output words of every pixel at counter (px, step, stream, domain)."""
    return P.philox4x32_10((np.arange(hw, dtype=np.uint64), step, stream, domain), P.key_of(seed))


def normals(seed, stream, step, hw, domain, dtype=np.float64):
    """[4, hw]: philox_ref.normals with the counter's last word = `domain` (philox_ref.normals itself fixes it at 0)."""
    r = words(seed, stream, step, hw, domain)
    z0, z1 = P.box_muller(r[0], r[1], dtype)
    z2, z3 = P.box_muller(r[2], r[3], dtype)
    return np.stack([z0, z1, z2, z3])


def start_noise(seed, streams, hw, scale, dtype=np.float64):
    """[bs, 4, hw] = z * scale at counter (px, 0, streams[row], 1): what cd360_start_noise_f32 writes.  `scale` is the fp32 value the
    kernel reads, every operation in `dtype`."""
    dt = np.dtype(dtype).type
    return np.stack([normals(seed, s, 0, hw, DOMAIN_START, dtype) * dt(scale) for s in streams])


def posterior(moments, w, bias, seed, streams, draw, scale_factor, dtype=np.float64):
    """moments [B, 8, hw], w [8, 8], bias [8] (the fp32 values the kernel reads) -> [B, 4, hw] = (mean + exp(0.5 clamp(lv)) z) *
    scale_factor in the kernel's order with z at counter (px, draw, streams[b], 2); every operation in `dtype`.  seed None: mean *
    scale_factor.  Also returns the logvar rows before the clamp (the test asserts all three classes are present)."""
    dt = np.dtype(dtype).type
    t = moments.astype(dt)
    wv, bv = w.astype(dt), bias.astype(dt)
    m = []
    for o in range(8):
        acc = wv[o, 0] * t[:, 0]
        for i in range(1, 8):
            acc = acc + wv[o, i] * t[:, i]
        m.append(acc + bv[o])
    m = np.stack(m, 1)  # [B, 8, hw]
    mean, lv = m[:, :4], np.minimum(np.maximum(m[:, 4:], dt(-30.0)), dt(20.0))
    if seed is None:
        return mean * dt(scale_factor), m[:, 4:]
    hw = moments.shape[-1]
    z = np.stack([normals(seed, s, draw, hw, DOMAIN_POSTERIOR, dtype) for s in streams])
    return (mean + np.exp(dt(0.5) * lv) * z) * dt(scale_factor), m[:, 4:]
