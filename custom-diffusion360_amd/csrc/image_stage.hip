// The joints between the sampler and the first stage (include/cd360_image.h): what ran as short stretches of framework kernels between the
// HIP denoise step, the HIP Decoder and the HIP Encoder.
//
//   cd360_start_noise_f32        the start latent of a trajectory: randn * sqrt(1 + sigma_0^2) (sampling.py:50, sample.py:290-292)
//   cd360_posterior_sample_f32   quant_conv (8 -> 8, 1 x 1) + DiagonalGaussianDistribution.sample() / .mode() + scale_factor * z
//                                (autoencoder.py:304-311, distributions.py:24-41, diffusion.py:214-219)
//   cd360_post_quant_f32         1 / scale_factor * z + post_quant_conv (4 -> 4, 1 x 1) (diffusion.py:208-212, autoencoder.py:313-316)
//   cd360_vae_conv_out_u8        Decoder.conv_out with the image epilogue clip(x * 0.5 + 0.5, 0, 1) * 255 -> uint8 HWC (sample.py:346)
//
// All four are memory-bound elementwise kernels: one thread per pixel, the channel planes read and written with consecutive lanes on
// consecutive addresses.  -ffp-contract=off: one fp32 rounding per operation, in the order the header states (tests/test_images_gpu.py holds
// the affine parts and the image epilogue to it bit for bit).  The noise is cd360_philox.h's, in domains 1 and 2 of its counter.
#include "cd360_common.h"
#include "cd360_philox.h"
#include "vae_conv_out.h"

namespace {

// out [bs, 4, HW] fp32 = z * scale[0], z = noise4 at counter (px, 0, streams[smp], 1)
__global__ __launch_bounds__(256) void start_noise_kernel(float* __restrict__ out, const uint32_t* __restrict__ seed, const int* __restrict__ streams,
                                                          const float* __restrict__ scale, int bs, long HW) {
  const uint32_t k0 = seed[0], k1 = seed[1];
  const float sc = *scale;
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    float z[4];
    noise4((uint32_t)px, 0u, streams ? (uint32_t)streams[smp] : 0u, CD360_NOISE_START, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) out[(smp * 4 + c) * HW + px] = z[c] * sc;
  }
}

// one output channel of a 1 x 1 convolution over N inputs: ((w_0 t_0 + w_1 t_1) + ... + w_(N-1) t_(N-1)) + bias
template <int N>
__device__ __forceinline__ float affine_row(const float (&w)[N], const float (&t)[N], float bias) {
  float m = w[0] * t[0];
#pragma unroll
  for (int i = 1; i < N; ++i) m = m + w[i] * t[i];
  return m + bias;
}

// moments [B, 8, HW] fp32; w [8][8], bias [8] fp32; out [B, 4, HW] fp32.  SAMPLE: out = (mean + exp(0.5 clamp(logvar)) z) scale_factor with
// z = noise4 at counter (px, draw[0], streams[b], 2); else out = mean * scale_factor and seed / streams / draw are not read.
template <bool SAMPLE>
__global__ __launch_bounds__(256) void posterior_sample_kernel(const float* __restrict__ moments, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const uint32_t* __restrict__ seed,
                                                               const int* __restrict__ streams, const int* __restrict__ draw, float scale_factor,
                                                               float* __restrict__ out, int B, long HW) {
  constexpr int NO = SAMPLE ? 8 : 4;  // mode() needs the mean rows alone
  float wr[NO][8], br[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    br[o] = bias[o];
#pragma unroll
    for (int i = 0; i < 8; ++i) wr[o][i] = w[o * 8 + i];
  }
  uint32_t k0 = 0u, k1 = 0u, dr = 0u;
  if constexpr (SAMPLE) k0 = seed[0], k1 = seed[1], dr = (uint32_t)*draw;
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / HW, px = i - b * HW;
    float t[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) t[c] = moments[(b * 8 + c) * HW + px];
    float m[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) m[o] = affine_row<8>(wr[o], t, br[o]);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SAMPLE) noise4((uint32_t)px, dr, streams ? (uint32_t)streams[b] : 0u, CD360_NOISE_POSTERIOR, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = m[c];
      if constexpr (SAMPLE) {
        const float lv = m[4 + c] < -30.f ? -30.f : (m[4 + c] > 20.f ? 20.f : m[4 + c]);  // torch.clamp: a NaN stays a NaN
        v = v + expf(0.5f * lv) * z[c];
      }
      out[(b * 4 + c) * HW + px] = v * scale_factor;
    }
  }
}

// z [B, 4, HW] fp32; w [4][4], bias [4] fp32; out [B, 4, HW] fp32 = post_quant_conv(z * inv_scale)
__global__ __launch_bounds__(256) void post_quant_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float inv_scale, float* __restrict__ out, int B, long HW) {
  float wr[4][4], br[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    br[o] = bias[o];
#pragma unroll
    for (int i = 0; i < 4; ++i) wr[o][i] = w[o * 4 + i];
  }
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / HW, px = i - b * HW;
    float t[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] = z[(b * 4 + c) * HW + px] * inv_scale;
#pragma unroll
    for (int o = 0; o < 4; ++o) out[(b * 4 + o) * HW + px] = affine_row<4>(wr[o], t, br[o]);
  }
}

// clip(v * 0.5 + 0.5, 0, 1) * 255, truncated; a NaN gives 0
__device__ __forceinline__ uint32_t image_byte(float v) {
  float t = v * 0.5f + 0.5f;
  t = t > 0.f ? t : 0.f;  // (false for a NaN)
  t = t < 1.f ? t : 1.f;
  return (uint32_t)(t * 255.f);
}

// x, w as for vae_conv_out_kernel (vae.hip); out [B][H][W][Cout] uint8.  Grid (ceil(H W / 256), B); thread = one output pixel.  A
// workgroup's pixels are one contiguous run of npx * Cout <= 1024 bytes of the image: the bytes are laid out in the LDS, then written as
// whole dwords from the first 4-byte boundary on, and as single bytes in front of it and behind the last whole dword (an image row is
// 3 W bytes, so neither end of a run need be aligned).  No store reaches outside [run, run + npx * Cout).
__global__ __launch_bounds__(256) void vae_conv_out_u8_kernel(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, uint8_t* __restrict__ out, int H, int W, int Cin,
                                                              int Cout) {
  __shared__ __attribute__((aligned(16))) float wl[9 * CO_CHUNK * 4];
  __shared__ __attribute__((aligned(4))) uint8_t ob[256 * 4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long HW = (long)H * W, p0 = (long)blockIdx.x * 256, p = p0 + tid;
  const bool live = p < HW;
  const f32x4 acc = vae_conv_out_accumulate(x, w, wl, b, p, live, H, W, Cin);
  if (live) {
#pragma unroll
    for (int co = 0; co < 4; ++co)
      if (co < Cout) ob[tid * Cout + co] = (uint8_t)image_byte(acc[co] + (bias ? bias[co] : 0.f));
  }
  __syncthreads();
  const int npx = (int)min((long)256, HW - p0), nbytes = npx * Cout;
  uint8_t* const run = out + ((long)b * HW + p0) * Cout;
  const int head = min((int)((4 - ((uintptr_t)run & 3)) & 3), nbytes);  // bytes in front of the first 4-byte boundary
  const int ndw = (nbytes - head) >> 2;                                // whole dwords behind them
  if (tid < ndw) {
    const uint8_t* s = ob + head + 4 * tid;
    *reinterpret_cast<uint32_t*>(run + head + 4 * tid) = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
  }
  const int tail0 = head + 4 * ndw;  // the at most 3 bytes behind the last whole dword
  if (tid < head) run[tid] = ob[tid];
  if (tid >= 64 && tid - 64 < nbytes - tail0) run[tail0 + tid - 64] = ob[tail0 + tid - 64];
}

inline unsigned stride_grid(long total) {  // grid-stride kernels: one thread per pixel up to 65536 workgroups
  const long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

inline bool overlap(const void* a, long bytes_a, const void* b, long bytes_b) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

inline bool f32_ok(const void* p) { return p && (uintptr_t)p % 4 == 0; }

}  // namespace

extern "C" int cd360_start_noise_f32(void* out, const void* seed, const void* streams, const void* scale, int bs, int64_t HW, void* stream) {
  if (!f32_ok(out) || !f32_ok(scale) || bs <= 0 || HW <= 0 || !noise_args_ok(seed, streams, scale, HW)) return CD360_ERR_ARG;
  hipLaunchKernelGGL(start_noise_kernel, dim3(stride_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream, (float*)out, (const uint32_t*)seed,
                     (const int*)streams, (const float*)scale, bs, (long)HW);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_posterior_sample_f32(const void* moments, const void* w, const void* bias, const void* seed, const void* streams,
                                          const void* draw, float scale_factor, void* out, int B, int64_t HW, void* stream) {
  if (!f32_ok(moments) || !f32_ok(w) || !f32_ok(bias) || !f32_ok(out) || B <= 0 || HW <= 0 || HW > ((int64_t)1 << 32)) return CD360_ERR_ARG;
  if (seed && !noise_args_ok(seed, streams, draw, HW)) return CD360_ERR_ARG;
  if (overlap(out, (long)B * 4 * HW * 4, moments, (long)B * 8 * HW * 4)) return CD360_ERR_ARG;
  const dim3 grid(stride_grid((long)B * HW));
  if (seed)
    hipLaunchKernelGGL(posterior_sample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)moments, (const float*)w,
                       (const float*)bias, (const uint32_t*)seed, (const int*)streams, (const int*)draw, scale_factor, (float*)out, B, (long)HW);
  else
    hipLaunchKernelGGL(posterior_sample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)moments, (const float*)w,
                       (const float*)bias, (const uint32_t*)nullptr, (const int*)nullptr, (const int*)nullptr, scale_factor, (float*)out, B,
                       (long)HW);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_post_quant_f32(const void* z, const void* w, const void* bias, float inv_scale, void* out, int B, int64_t HW, void* stream) {
  if (!f32_ok(z) || !f32_ok(w) || !f32_ok(bias) || !f32_ok(out) || B <= 0 || HW <= 0) return CD360_ERR_ARG;
  if (overlap(out, (long)B * 4 * HW * 4, z, (long)B * 4 * HW * 4)) return CD360_ERR_ARG;
  hipLaunchKernelGGL(post_quant_kernel, dim3(stride_grid((long)B * HW)), dim3(256), 0, (hipStream_t)stream, (const float*)z, (const float*)w,
                     (const float*)bias, inv_scale, (float*)out, B, (long)HW);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_vae_conv_out_u8(const void* x, const void* w, const void* bias, void* out, int B, int H, int W, int Cin, int Cout,
                                     void* stream) {
  if (!x || !w || !out || B <= 0 || H <= 0 || W <= 0) return CD360_ERR_ARG;
  if (Cin % 64 || Cin <= 0 || Cout < 1 || Cout > 4 || B > 65535) return CD360_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)w) % 16) return CD360_ERR_ARG;
  const dim3 grid((unsigned)(((long)H * W + 255) / 256), B);
  vae_conv_out_u8_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const uint16_t*)x, (const float*)w, (const float*)bias, (uint8_t*)out, H, W, Cin,
                                                               Cout);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
