// libcd360_edit.so (include/edit/cd360_edit.h): the blend that ends a masked sampling step, and the noise it adds to the known latent.
// After a solver's whole step to the noise level s' the region to keep is replaced by the known latent at that level:
//   kn = (s' == 0) ? known : known + z * s'         z = the generator of ../csrc/cd360_philox.h in counter domain 3
//   x' = m * x + (1 - m) * kn                       m = the pixel's mask value, 1 = generate, 0 = keep
// One fp32 rounding per operation (the build passes -ffp-contract=off).  Memory-bound and elementwise: a thread owns one pixel of one
// sample, so one Philox call serves its four channels and every channel plane is read and written along consecutive lanes.
#include "../csrc/cd360_philox.h"

namespace {

// z[c] = the domain-3 noise of channel c of pixel px in noise stream `strm` at step `step`
__device__ __forceinline__ void edit_noise4(uint32_t px, uint32_t step, uint32_t strm, uint32_t k0, uint32_t k1, float z[4]) {
  noise4(px, step, strm, CD360_NOISE_EDIT, k0, k1, z);
}

// out [bs, 4, HW] fp32; seed: device int64 read as (low, high) 32-bit words; streams [bs] int32 or null (stream 0 for every row)
__global__ __launch_bounds__(256) void edit_noise_kernel(float* __restrict__ out, const uint32_t* __restrict__ seed, const int* __restrict__ streams,
                                                         const int* __restrict__ step, int bs, long HW) {
  const uint32_t k0 = seed[0], k1 = seed[1], st = (uint32_t)*step;
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    float z[4];
    edit_noise4((uint32_t)px, st, streams ? (uint32_t)streams[smp] : 0u, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) out[(smp * 4 + c) * HW + px] = z[c];
  }
}

// x [bs, 4, HW] fp32 IN PLACE; known [bs, 4, HW]; mask [mask_rows, HW], mask_rows in {1, bs} (mask_stride = 0 or HW: the row of sample smp
// starts at smp * mask_stride); s' = sigma_next[step * sigma_stride].  s' is one scalar, uniform over the launch: no Philox work on an
// s' == 0 row.
__global__ __launch_bounds__(256) void mask_blend_kernel(float* __restrict__ x, const float* __restrict__ known, const float* __restrict__ mask,
                                                         long mask_stride, const float* __restrict__ sigma_next, int sigma_stride,
                                                         const int* __restrict__ step, const uint32_t* __restrict__ seed,
                                                         const int* __restrict__ streams, int bs, long HW) {
  const int idx = *step;
  const float sn = sigma_next[(long)idx * sigma_stride];
  const bool noisy = sn != 0.f;
  const uint32_t k0 = seed[0], k1 = seed[1];
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    const float m = mask[smp * mask_stride + px], keep = 1.f - m;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) edit_noise4((uint32_t)px, (uint32_t)idx, streams ? (uint32_t)streams[smp] : 0u, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      const float kv = known[at];
      const float kn = noisy ? kv + z[c] * sn : kv;
      x[at] = m * x[at] + keep * kn;
    }
  }
}

inline unsigned tail_grid(long total) {  // grid-stride kernels: one thread per element up to 65536 workgroups
  const long g = (total + 255) / 256;
  return (unsigned)(g < 65536 ? g : 65536);
}

inline bool overlap(const void* a, long bytes_a, const void* b, long bytes_b) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

}  // namespace

// out [bs, 4, HW] fp32 standard normals of domain 3; seed: device int64[1]; streams: device int32[bs] or null; step: device int32[1]
// (noise_args_ok)
extern "C" int cd360_edit_noise_f32(void* out, const void* seed, const void* streams, const void* step, int bs, int64_t HW, void* stream) {
  if (!out || bs <= 0 || HW <= 0 || !noise_args_ok(seed, streams, step, HW) || (uintptr_t)out % 4) return CD360_ERR_ARG;
  hipLaunchKernelGGL(edit_noise_kernel, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream, (float*)out, (const uint32_t*)seed,
                     (const int*)streams, (const int*)step, bs, (long)HW);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [bs, 4, HW] fp32 IN PLACE; known [bs, 4, HW]; mask [mask_rows, HW]; sigma_next / sigma_stride: column 1 of a step table with stride 4,
// or a device scalar with stride 0; step = the index of sigma_next AND the noise counter's step word
extern "C" int cd360_mask_blend_f32(void* x, const void* known, const void* mask, int mask_rows, const void* sigma_next, int sigma_stride,
                                    const void* step, const void* seed, const void* streams, int bs, int64_t HW, void* stream) {
  if (!x || !known || !mask || !sigma_next || bs <= 0 || HW <= 0 || !noise_args_ok(seed, streams, step, HW)) return CD360_ERR_ARG;
  if ((mask_rows != 1 && mask_rows != bs) || sigma_stride < 0) return CD360_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)known | (uintptr_t)mask | (uintptr_t)sigma_next) % 4) return CD360_ERR_ARG;
  const long bytes = (long)bs * 4 * HW * (long)sizeof(float);
  if (overlap(x, bytes, known, bytes) || overlap(x, bytes, mask, (long)mask_rows * HW * (long)sizeof(float))) return CD360_ERR_ARG;
  hipLaunchKernelGGL(mask_blend_kernel, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream, (float*)x, (const float*)known,
                     (const float*)mask, mask_rows == 1 ? 0L : (long)HW, (const float*)sigma_next, sigma_stride, (const int*)step,
                     (const uint32_t*)seed, (const int*)streams, bs, (long)HW);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
