// Decoder.conv_out's accumulation (model.py:699-701, :733), shared by its two epilogues: vae_conv_out_kernel (vae.hip: fp32 NCHW) and
// vae_conv_out_u8_kernel (image_stage.hip: the uint8 image).  One function, so both see the same fp32 value before their epilogue.
#pragma once
#include "cd360_common.h"

constexpr int CO_CHUNK = 256;  // input channels whose weights sit in the LDS at a time

// x [B][H W][Cin] bf16; w [9][Cin][4] fp32 (tap 3 ky + kx, channel, output channel; columns >= Cout zero); wl: 9 * CO_CHUNK * 4 floats of
// LDS, 16-byte aligned.  Called by ALL 256 threads of a workgroup (it synchronises); thread = output pixel p of image b, `live` = p < H W.
// -> the four output channels' sums, bias not added.
__device__ __forceinline__ f32x4 vae_conv_out_accumulate(const uint16_t* __restrict__ x, const float* __restrict__ w, float* wl, int b, long p,
                                                         bool live, int H, int W, int Cin) {
  const long HW = (long)H * W;
  const int y = live ? (int)(p / W) : 0, xq = live ? (int)(p - (long)y * W) : 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < Cin; c0 += CO_CHUNK) {
    const int cn = min(CO_CHUNK, Cin - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < 9 * cn; i += 256) {
      const int tap = i / cn, ci = i - tap * cn;
      *reinterpret_cast<f32x4*>(wl + (tap * CO_CHUNK + ci) * 4) = *reinterpret_cast<const f32x4*>(w + ((long)tap * Cin + c0 + ci) * 4);
    }
    __syncthreads();
    if (!live) continue;
    for (int tap = 0; tap < 9; ++tap) {
      const int yy = y + tap / 3 - 1, xx = xq + tap % 3 - 1;
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const uint16_t* xp = x + ((long)b * HW + (long)yy * W + xx) * Cin + c0;
      const float* wt = wl + tap * CO_CHUNK * 4;
      for (int c8 = 0; c8 < cn; c8 += 8) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(xp + c8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wt + (c8 + 2 * e) * 4);
          const f32x4 w1 = *reinterpret_cast<const f32x4*>(wt + (c8 + 2 * e + 1) * 4);
          acc += bf16lo_to_f32(v[e]) * w0;
          acc += bf16hi_to_f32(v[e]) * w1;
        }
      }
    }
  }
  return acc;
}
