// The library's device noise, shared by sampler_stage.hip (the noise drawn inside a sampling step) and image_stage.hip (the start latent,
// the first stage's posterior sample).  Standard normals as a PURE FUNCTION of (seed, domain, noise stream, step index, channel, pixel):
// Philox4x32-10 as published in Random123 (key = the two halves of the seed, counter = (pixel, step, stream id, domain)), then Box-Muller
// on the four output words.  One Philox call serves the four latent channels of a pixel.  Nothing here depends on the grid, on bs or on
// where a row sits in the batch, so a graph replay, an eager launch, a fresh sampler and the un-staged route draw the same bits
// (include/cd360_stochastic.h, include/cd360_image.h).
// Precise logf / sinf / cosf / sqrtf: the float64 restatement in tests/philox_ref.py is the yardstick.
#pragma once
#include "cd360_common.h"

#include <cmath>

// the counter's last word: which consumer draws.  A trajectory's start latent and the posterior sample never meet a step's noise.
constexpr uint32_t CD360_NOISE_STEP = 0u;       // inside a sampling step (include/cd360_stochastic.h, cd360_edm.h, cd360_highorder.h)
constexpr uint32_t CD360_NOISE_START = 1u;      // the start of a trajectory (cd360_start_noise_f32)
constexpr uint32_t CD360_NOISE_POSTERIOR = 2u;  // DiagonalGaussianDistribution.sample (cd360_posterior_sample_f32)
constexpr uint32_t CD360_NOISE_EDIT = 3u;       // the known region of a masked step (csrc_edit/mask_blend.hip, include/edit/cd360_edit.h)
// a training step (csrc_train/train_stage.hip, include/train/cd360_train.h)
constexpr uint32_t CD360_NOISE_TRAIN_SIGMA = 4u;   // the per-sample draws: sigma indices, offset noise
constexpr uint32_t CD360_NOISE_TRAIN_TARGET = 5u;  // the noise added to the target latent
constexpr uint32_t CD360_NOISE_TRAIN_REF_A = 6u;   // the reference views, noised by the loss
constexpr uint32_t CD360_NOISE_TRAIN_REF_B = 7u;   // the reference views, noised again by the denoiser

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& za, float& zb) {
  const float u1 = (float)((ra >> 8) + 1u) * 0x1p-24f;  // (0, 1]: exact in fp32
  const float u2 = (float)(rb >> 8) * 0x1p-24f;         // [0, 1)
  const float rad = sqrtf(-2.f * logf(u1));
  const float ang = 6.2831855f * u2;
  za = rad * cosf(ang);
  zb = rad * sinf(ang);
}

// z[c] = the noise of channel c of pixel px in noise stream `strm` at step `step` of domain `domain`
__device__ __forceinline__ void noise4(uint32_t px, uint32_t step, uint32_t strm, uint32_t domain, uint32_t k0, uint32_t k1, float z[4]) {
  uint32_t r[4];
  philox4x32_10(px, step, strm, domain, k0, k1, r);
  box_muller(r[0], r[1], z[0], z[1]);
  box_muller(r[2], r[3], z[2], z[3]);
}

// what every user of the generator asks: seed a device int64, step / streams device int32 (streams may be null), HW <= 2^32: the pixel is
// one 32-bit counter word
inline bool noise_args_ok(const void* seed, const void* streams, const void* step, int64_t HW) {
  return seed && step && (uintptr_t)seed % 8 == 0 && ((uintptr_t)step | (uintptr_t)streams) % 4 == 0 && HW <= ((int64_t)1 << 32);
}
