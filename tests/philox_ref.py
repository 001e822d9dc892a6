"""numpy restatement of the library's device noise (include/cd360_stochastic.h; plain helper module, like guarded.py): Philox4x32-10 as
published in Random123, the two uniforms per word pair, Box-Muller.  `normals(..., dtype=np.float64)` is the yardstick of the noise
kernel; `dtype=np.float32` evaluates the same expression in the kernel's precision on the host, which sizes the kernel's bar.

Known answers (Random123, kat_vectors, philox4x32 10 rounds), asserted in tests/test_euler_a_cpu.py: KAT below."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
TWO_PI_F32 = np.float32(6.2831855)

# (counter, key) -> output words
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) that broadcast against each other, key: two ints -> four uint32 arrays r0..r3."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def key_of(seed: int):
    """(low, high) 32-bit words of the seed's low 64 bits -- what the kernels read from the device int64."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & MASK, s >> 32


def box_muller(ra, rb, dtype=np.float64):
    """u1 = ((ra >> 8) + 1) 2^-24 in (0, 1], u2 = (rb >> 8) 2^-24 in [0, 1): both exact in fp32.  rad = sqrt(-2 log u1), angle =
    6.2831855f u2 (the fp32 constant), -> (rad cos, rad sin), every operation in `dtype`."""
    dt = np.dtype(dtype).type
    u1 = ((ra >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (rb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    u1, u2 = u1.astype(dt), u2.astype(dt)
    rad = np.sqrt(dt(-2.0) * np.log(u1))
    ang = dt(TWO_PI_F32) * u2
    return rad * np.cos(ang), rad * np.sin(ang)


def normals(seed: int, stream: int, step: int, hw: int, dtype=np.float64):
    """[4, hw]: z[c, px] = the noise of channel c of pixel px in noise stream `stream` at step `step` under `seed`."""
    r = philox4x32_10((np.arange(hw, dtype=np.uint64), step, stream, 0), key_of(seed))
    z0, z1 = box_muller(r[0], r[1], dtype)
    z2, z3 = box_muller(r[2], r[3], dtype)
    return np.stack([z0, z1, z2, z3])


def batch(seed: int, streams, step: int, hw: int, dtype=np.float64):
    """[bs, 4, hw] for one stream id per row: what cd360_sampler_noise_f32 writes."""
    return np.stack([normals(seed, s, step, hw, dtype) for s in streams])


def corr(a, b) -> float:
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def moments(z):
    """(|mean|, |var - 1|, |m4 - 3|) of all values of z."""
    z = np.asarray(z, np.float64).ravel()
    return abs(float(z.mean())), abs(float(z.var()) - 1.0), abs(float((z ** 4).mean()) - 3.0)


# bounds of tests/test_euler_a_cpu.py test 6 at N = 65 536 values per seed (five standard errors: 5 / sqrt(N) = 0.0195, 5 sqrt(2 / N) =
# 0.0276, 5 sqrt(96 / N) = 0.191)
BOUND_MEAN, BOUND_VAR, BOUND_M4 = 0.020, 0.028, 0.19
STAT_SEEDS, STAT_HW, STAT_STEPS = (30, 0, 2 ** 63 + 12345), 4096, (0, 1, 2, 3)


def check_statistics(draw):
    """The conditions of test 6, on any generator `draw(seed, stream, step) -> [4, STAT_HW]` (the restatement on the CPU, the kernel on the
    GPU); returns the worst figures."""
    worst = dict(mean=0.0, var=0.0, m4=0.0, corr=0.0)
    for seed in STAT_SEEDS:
        z = {st: np.asarray(draw(seed, 0, st), np.float64) for st in STAT_STEPS}
        m = moments(np.stack([z[st] for st in STAT_STEPS]))  # N = 4 steps x 4 channels x 4096 pixels
        assert m[0] <= BOUND_MEAN and m[1] <= BOUND_VAR and m[2] <= BOUND_M4, (seed, m)
        pairs = {"steps 0 / 1": (z[0], z[1]), "streams 0 / 1": (z[0], draw(seed, 1, 0)), "seeds s / s + 1": (z[0], draw(seed + 1, 0, 0)),
                 "neighbouring pixels": (z[0][:, :-1], z[0][:, 1:])}
        for a in range(4):
            for b in range(a + 1, 4):
                pairs[f"channels {a} / {b}"] = (z[0][a], z[0][b])
        for what, (a, b) in pairs.items():
            n = np.asarray(a).size
            c = abs(corr(a, b))
            assert c <= 5.0 / np.sqrt(n), (seed, what, c, n)
            worst["corr"] = max(worst["corr"], c * np.sqrt(n))  # in standard errors
        for k, v in zip(("mean", "var", "m4"), m):
            worst[k] = max(worst[k], v)
    return worst
