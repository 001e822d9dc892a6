// The two ends of one captured denoise step (sample.py:331-349 through EulerEDMSampler.sampler_step,
// sampling.py:85-136, DiscreteDenoiser.network_inputs, denoiser.py:47-79, and UNetModel.forward's first lines, openaimodel.py:1006-1030):
//
//   stage-in   x3 = [x | x | x];  h0 = conv3x3(bf16(c_in x3), 4 -> 320) + b        the UNet's input convolution on the scaled latent
//              emb_act = silu(time_embed(t_emb(idx(sigma))) + label_emb(y))        the input of every ResBlock's emb_layers Linear
//   step-out   x <- x + (x - d0) / sigma (sigma' - sigma),  d0 = the 3-way CFG combine of x - sigma eps_b
//
// Everything that depends on the STEP only -- sigma, sigma', c_in, the time-embedding row -- is a row of two tables the sampler fills
// once per schedule (cd360/job.py: Sampler.prepare); the kernels pick their row through a device-side step index, so a captured step
// holds no scalar arithmetic at all: round 5's graph spent ~45 torch-issued micro-kernels per step on it (sub / abs / argmin / index /
// pow / sqrt / reciprocal / arange / exp / sin / cos / cat / silu / casts / the 4 -> 64 channel pad of the input convolution).
// The input convolution is computed ONCE per diffusion sample and written to its three CFG branches (their inputs are identical).
#include "cd360_common.h"
#include "cd360_philox.h"

#include <cmath>
#include <type_traits>

namespace {

constexpr int TP = 64;  // pixels of one image row per workgroup

// x [bs, 4, H, W] fp32 (NCHW); tab [nsteps, 4] fp32 = (sigma, sigma_next, c_in, -); step: device int32; w [36][Cout] fp32 (k = tap * 4 + ci,
// values already rounded to bf16); bias [Cout] fp32; h [rep * bs, H * W, Cout] bf16 (branch r of sample s = image r * bs + s);
// temb [nsteps, E] bf16, lab [rep * bs, E] bf16, emb_act [rep * bs, E] bf16.  Blocks [0, nconv) convolve, the rest build emb_act.
__global__ __launch_bounds__(256) void unet_stage_in_kernel(const float* __restrict__ x, const float* __restrict__ tab, const int* __restrict__ step,
                                                            const float* __restrict__ w, const float* __restrict__ bias, uint16_t* __restrict__ h,
                                                            const uint16_t* __restrict__ temb, const uint16_t* __restrict__ lab,
                                                            uint16_t* __restrict__ emb_act, int bs, int rep, int H, int W, int Cout, int E, int nconv) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int idx = *step;
  if ((int)blockIdx.x >= nconv) {  // ---- emb_act rows: 8 values per thread ----
    const long total = (long)rep * bs * (E >> 3);
    for (long i = (long)(blockIdx.x - nconv) * 256 + tid; i < total; i += (long)(gridDim.x - nconv) * 256) {
      const long row = i / (E >> 3);
      const int c8 = (int)(i - row * (E >> 3));
      const u32x4 a = *reinterpret_cast<const u32x4*>(temb + (long)idx * E + c8 * 8);
      const u32x4 b = *reinterpret_cast<const u32x4*>(lab + row * E + c8 * 8);
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // emb = time_embed(..) + label_emb(y) is a bf16 tensor in the module path: round the sum, then SiLU of the rounded value
        const uint32_t s = pack_bf16x2(bf16lo_to_f32(a[e]) + bf16lo_to_f32(b[e]), bf16hi_to_f32(a[e]) + bf16hi_to_f32(b[e]));
        const float v0 = bf16lo_to_f32(s), v1 = bf16hi_to_f32(s);
        o[e] = pack_bf16x2(v0 / (1.f + __expf(-v0)), v1 / (1.f + __expf(-v1)));
      }
      *reinterpret_cast<u32x4*>(emb_act + row * E + c8 * 8) = o;
    }
    return;
  }
  float* const wl = reinterpret_cast<float*>(smem);               // [36][Cout]
  float* const xs = wl + 36 * Cout;                               // [3][TP + 2][4]: the row band with its halo, scaled and bf16-rounded
  const int tiles_w = (W + TP - 1) / TP;
  const int tw = blockIdx.x % tiles_w, y = (blockIdx.x / tiles_w) % H, s = blockIdx.x / (tiles_w * H);
  const int x0 = tw * TP;
  const float c_in = tab[idx * 4 + 2];
  for (int i = tid; i < 36 * Cout; i += 256) wl[i] = w[i];
  for (int i = tid; i < 3 * (TP + 2) * 4; i += 256) {
    const int ci = i & 3, px = (i >> 2) % (TP + 2), ry = (i >> 2) / (TP + 2);
    const int yy = y + ry - 1, xx = x0 + px - 1;
    float v = 0.f;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = bf16_to_f32(f32_to_bf16(x[(((long)s * 4 + ci) * H + yy) * W + xx] * c_in));
    xs[i] = v;
  }
  __syncthreads();
  const int chunks = Cout >> 3;
  const long HW = (long)H * W;
  for (int item = tid; item < TP * chunks; item += 256) {
    const int px = item / chunks, ch = item - px * chunks;
    if (x0 + px >= W) continue;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = bias[ch * 8 + e];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const f32x4 xin = *reinterpret_cast<const f32x4*>(xs + ((tap / 3) * (TP + 2) + px + tap % 3) * 4);
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const float* wk = wl + (tap * 4 + ci) * Cout + ch * 8;
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wk), w1 = *reinterpret_cast<const f32x4*>(wk + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[e] = fmaf(xin[ci], w0[e], acc[e]);
          acc[4 + e] = fmaf(xin[ci], w1[e], acc[4 + e]);
        }
      }
    }
    const u32x4 o = {pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]), pack_bf16x2(acc[4], acc[5]), pack_bf16x2(acc[6], acc[7])};
    for (int r = 0; r < rep; ++r)
      *reinterpret_cast<u32x4*>(h + (((long)r * bs + s) * HW + (long)y * W + x0 + px) * Cout + ch * 8) = o;
  }
}


// ---- the tails of one CFG sampling step: EpsScaling c_out (denoiser.py:41-44, denoiser_scaling.py:26-32), the guider's
// combine -- ScheduledCFGImgTextRef (guiders.py:111-114, NB = 3: u | ic | c) or VanillaCFGImgRef (guiders.py:144-147, NB = 2: u | c) --,
// then the solver's update.  Every solver has two kernels: the `_cl` form a captured step ends on (x in place, eps = the output convolution's
// bf16 channels-last rows, per-step scalars from tables through the device-side step index) and the un-staged flat fp32 form.  They share
// the combine and the eps loads below and differ in one short update function per solver.
// -ffp-contract=off: one fp32 rounding per operation, in the order written (tests/test_cfg2_gpu.py, test_dpmpp2m_gpu.py and
// test_euler_a_gpu.py hold every kernel to it bit for bit).

// den_b = x - s eps_b;  d0 = the guider's combine.  NB = 2 is the NB = 3 expression without the image term.
template <int NB>
__device__ __forceinline__ float cfg_combine(float xv, float s, float e_u, float e_i, float e_c, float scale, float scale_im) {
  static_assert(NB == 2 || NB == 3, "two or three CFG branches");
  if constexpr (NB == 3) {
    const float du = xv - s * e_u, dic = xv - s * e_i, dc = xv - s * e_c;
    return du + scale * (dc - dic) + scale_im * (dic - du);
  } else {
    const float du = xv - s * e_u, dc = xv - s * e_c;
    return du + scale * (dc - du);
  }
}

// flat eps [NB n] fp32: branch b of element i at eps[b n + i]
template <int NB>
__device__ __forceinline__ float cfg_combine_flat(const float* __restrict__ eps, long n, long i, float xv, float s, float scale, float scale_im) {
  return cfg_combine<NB>(xv, s, eps[i], NB == 3 ? eps[n + i] : 0.f, eps[(NB - 1) * n + i], scale, scale_im);
}

// eps [NB bs, HW, ld] bf16 channels-last (channels 0..3 of each pixel row; NB = 3: u | ic | c thirds, NB = 2: u | c halves -- no row past
// image 2 bs - 1 is read): one pixel's four channels of every branch, as they lie (two bf16 pairs per branch)
struct EpsRow {
  u32x2 u, i, c;  // (NB = 2: i = u, unused)
};

template <int NB>
__device__ __forceinline__ EpsRow load_eps_row(const uint16_t* __restrict__ eps, int bs, long HW, int ld, long smp, long px) {
  EpsRow r;
  r.u = *reinterpret_cast<const u32x2*>(eps + ((0 * bs + smp) * HW + px) * ld);
  r.i = r.u;
  if constexpr (NB == 3) r.i = *reinterpret_cast<const u32x2*>(eps + ((1 * bs + smp) * HW + px) * ld);
  r.c = *reinterpret_cast<const u32x2*>(eps + (((NB - 1) * bs + smp) * HW + px) * ld);
  return r;
}

__device__ __forceinline__ float bf16_of(u32x2 v, int c) { return (c & 1) ? bf16hi_to_f32(v[c >> 1]) : bf16lo_to_f32(v[c >> 1]); }

template <int NB>
__device__ __forceinline__ float cfg_combine_cl(const EpsRow& r, int c, float xv, float s, float scale, float scale_im) {
  return cfg_combine<NB>(xv, s, bf16_of(r.u, c), bf16_of(r.i, c), bf16_of(r.c, c), scale, scale_im);
}

// ---- Euler (sampling.py:101-106, sampling_utils.py:39-40: to_d, then the step to sigma_next) ----
__device__ __forceinline__ float euler_update(float xv, float d0, float s, float sn) { return xv + (xv - d0) / s * (sn - s); }

// x [bs, 4, HW] fp32, updated IN PLACE; eps: see load_eps_row; tab [nsteps, 4] = (sigma, sigma_next, c_in, -)
template <int NB>
__global__ __launch_bounds__(256) void cfg_euler_step_cl_kernel(float* __restrict__ x, const uint16_t* __restrict__ eps, const float* __restrict__ tab,
                                                                const int* __restrict__ step, float scale, float scale_im, int bs, long HW, int ld) {
  const int idx = *step;
  const float s = tab[idx * 4], sn = tab[idx * 4 + 1];
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    const EpsRow e = load_eps_row<NB>(eps, bs, HW, ld, smp, px);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float* xp = x + (smp * 4 + c) * HW + px;
      const float xv = *xp;
      *xp = euler_update(xv, cfg_combine_cl<NB>(e, c, xv, s, scale, scale_im), s, sn);
    }
  }
}

// the un-staged form: x [n] fp32, eps [NB n] fp32, sigma / sigma_next device scalars -> out [n]
template <int NB>
__global__ __launch_bounds__(256) void cfg_euler_step_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ sigma,
                                                             const float* __restrict__ sigma_next, float scale, float scale_im,
                                                             float* __restrict__ out, long n) {
  const float s = *sigma, sn = *sigma_next;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float xv = x[i];
    out[i] = euler_update(xv, cfg_combine_flat<NB>(eps, n, i, xv, s, scale, scale_im), s, sn);
  }
}

// ---- DPM++ 2M (sampling.py:390-465, DPMPP2MSampler.sampler_step): the second-order multistep update in table form.
// Per element, with s = sigma of the step and (m1, m2, m3, m4) one row of a per-schedule multiplier table (cd360/sampler.py::dpmpp2m_multipliers:
// get_variables / get_mult evaluated once per schedule on the host, (m3, m4) = (1, 0) for the first step and for sigma_next = 0):
//   d0    = cfg_combine<NB>
//   dd    = (m4 == 0) ? d0 : m3 d0 - m4 old          `old` (the previous step's d0) is NOT read when m4 == 0: on the first step of an image it holds
//                                                    the previous image's value or uninitialised memory, and 0 * NaN must not reach x
//   x'    = m1 x - m2 dd;  old' = d0
__device__ __forceinline__ float dpmpp2m_update(float xv, float d0, float ov, float m1, float m2, float m3, float m4, bool multi) {
  const float dd = multi ? m3 * d0 - m4 * ov : d0;
  return m1 * xv - m2 * dd;
}

// x, old [bs, 4, HW] fp32, both updated IN PLACE; eps as for cfg_euler_step_cl_kernel; tab [nsteps, 4] (column 0 = sigma), mult [nsteps, 4]
template <int NB>
__global__ __launch_bounds__(256) void cfg_dpmpp2m_step_cl_kernel(float* __restrict__ x, float* __restrict__ old, const uint16_t* __restrict__ eps,
                                                                  const float* __restrict__ tab, const float* __restrict__ mult,
                                                                  const int* __restrict__ step, float scale, float scale_im, int bs, long HW, int ld) {
  const int idx = *step;
  const float s = tab[idx * 4];
  const float m1 = mult[idx * 4], m2 = mult[idx * 4 + 1], m3 = mult[idx * 4 + 2], m4 = mult[idx * 4 + 3];
  const bool multi = m4 != 0.f;  // one table scalar: uniform over the launch
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    const EpsRow e = load_eps_row<NB>(eps, bs, HW, ld, smp, px);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      const float xv = x[at];
      const float ov = multi ? old[at] : 0.f;
      const float d0 = cfg_combine_cl<NB>(e, c, xv, s, scale, scale_im);
      x[at] = dpmpp2m_update(xv, d0, ov, m1, m2, m3, m4, multi);
      old[at] = d0;
    }
  }
}

// the un-staged form: x, old [n] fp32, eps [NB n] fp32, sigma [1], mult [4] device tensors -> out, old_out [n]
template <int NB>
__global__ __launch_bounds__(256) void cfg_dpmpp2m_step_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ old,
                                                               const float* __restrict__ sigma, const float* __restrict__ mult, float scale,
                                                               float scale_im, float* __restrict__ out, float* __restrict__ old_out, long n) {
  const float s = *sigma;
  const float m1 = mult[0], m2 = mult[1], m3 = mult[2], m4 = mult[3];
  const bool multi = m4 != 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float xv = x[i];
    const float ov = multi ? old[i] : 0.f;
    const float d0 = cfg_combine_flat<NB>(eps, n, i, xv, s, scale, scale_im);
    out[i] = dpmpp2m_update(xv, d0, ov, m1, m2, m3, m4, multi);
    old_out[i] = d0;
  }
}

// ---- device noise + ancestral Euler (sampling.py:236-273, 340-347: AncestralSampler / EulerAncestralSampler.sampler_step) --------------------
// The generator itself (Philox4x32-10 + Box-Muller, counter = (pixel, step, stream id, domain)) is cd360_philox.h, shared with
// image_stage.hip.  A step's noise is domain 0 (include/cd360_stochastic.h).

// z[c] = the noise of channel c of pixel px in noise stream `strm` at step `step`
__device__ __forceinline__ void sampler_noise4(uint32_t px, uint32_t step, uint32_t strm, uint32_t k0, uint32_t k1, float z[4]) {
  noise4(px, step, strm, CD360_NOISE_STEP, k0, k1, z);
}

// out [bs, 4, HW] fp32; seed: device int64 read as (low, high) 32-bit words; streams [bs] int32 or null (stream 0 for every row)
__global__ __launch_bounds__(256) void sampler_noise_kernel(float* __restrict__ out, const uint32_t* __restrict__ seed, const int* __restrict__ streams,
                                                            const int* __restrict__ step, int bs, long HW) {
  const uint32_t k0 = seed[0], k1 = seed[1], st = (uint32_t)*step;
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    float z[4];
    sampler_noise4((uint32_t)px, st, streams ? (uint32_t)streams[smp] : 0u, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) out[(smp * 4 + c) * HW + px] = z[c];
  }
}

// Per element, s = sigma of the step, (sd, su, s_noise, -) one row of cd360/sampler.py::euler_ancestral_table (get_ancestral_step evaluated
// once per schedule on the host):
//   d0  = cfg_combine<NB>                              x_e = the Euler step to sd: x + (x - d0) / s * (sd - s)   sampling.py:244-248
//   x'  = (su == 0) ? x_e : x_e + (z * s_noise) * su                                                             sampling.py:250-256
// su is one table scalar, uniform over the launch; no Philox work on a su == 0 row (the last row, and every row for eta = 0).
__device__ __forceinline__ float euler_ancestral_update(float xv, float d0, float s, float sd, float su, float s_noise, float z, bool noisy) {
  const float xe = euler_update(xv, d0, s, sd);
  return noisy ? xe + (z * s_noise) * su : xe;
}

// x [bs, 4, HW] fp32 IN PLACE; eps as for cfg_euler_step_cl_kernel; tab [nsteps, 4] (column 0 = sigma), anc [nsteps, 4] = (sd, su, s_noise, -)
template <int NB>
__global__ __launch_bounds__(256) void cfg_euler_ancestral_step_cl_kernel(float* __restrict__ x, const uint16_t* __restrict__ eps,
                                                                          const float* __restrict__ tab, const float* __restrict__ anc,
                                                                          const int* __restrict__ step, const uint32_t* __restrict__ seed,
                                                                          const int* __restrict__ streams, float scale, float scale_im, int bs,
                                                                          long HW, int ld) {
  const int idx = *step;
  const float s = tab[idx * 4];
  const float sd = anc[idx * 4], su = anc[idx * 4 + 1], s_noise = anc[idx * 4 + 2];
  const bool noisy = su != 0.f;
  const uint32_t k0 = seed[0], k1 = seed[1];
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    const EpsRow e = load_eps_row<NB>(eps, bs, HW, ld, smp, px);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) sampler_noise4((uint32_t)px, (uint32_t)idx, streams ? (uint32_t)streams[smp] : 0u, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      const float xv = x[at];
      x[at] = euler_ancestral_update(xv, cfg_combine_cl<NB>(e, c, xv, s, scale, scale_im), s, sd, su, s_noise, z[c], noisy);
    }
  }
}

// the un-staged form: x [bs, 4, HW] fp32, eps [NB bs, 4, HW] fp32, sigma [1], anc [4] device tensors -> out [bs, 4, HW]
template <int NB>
__global__ __launch_bounds__(256) void cfg_euler_ancestral_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                                       const float* __restrict__ sigma, const float* __restrict__ anc,
                                                                       const uint32_t* __restrict__ seed, const int* __restrict__ streams,
                                                                       const int* __restrict__ step, float scale, float scale_im,
                                                                       float* __restrict__ out, int bs, long HW) {
  const float s = *sigma;
  const float sd = anc[0], su = anc[1], s_noise = anc[2];
  const bool noisy = su != 0.f;
  const uint32_t k0 = seed[0], k1 = seed[1], st = (uint32_t)*step;
  const long total = (long)bs * HW, n = total * 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) sampler_noise4((uint32_t)px, st, streams ? (uint32_t)streams[smp] : 0u, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      const float xv = x[at];
      out[at] = euler_ancestral_update(xv, cfg_combine_flat<NB>(eps, n, at, xv, s, scale, scale_im), s, sd, su, s_noise, z[c], noisy);
    }
  }
}

// ---- the EDM family with churn, and Heun (sampling.py:85-136, 314-337: EDMSampler.sampler_step, HeunEDMSampler.possible_correction_step) ----
// include/cd360_edm.h.  A churned step evaluates the network at sigma_hat = sigma (1 + gamma), which is not on the denoiser's grid:
// DiscreteDenoiser snaps it, so c_out (and c_in, and the time-embedding row) come from sq = q(sigma_hat) while to_d and dt keep the
// un-snapped sigma_hat.  edm [nsteps, 4] = (sigma_hat, sigma_next, c_in(sq), sq); corr [nsteps, 4] = the same for the corrector's evaluation
// at sigma_next; churn [nsteps, 4] = (gamma, noise_std, s_noise, 0)  (cd360/sampler.py::edm_tables).

// x [bs, 4, HW] fp32 IN PLACE: x <- x + (z * s_noise) * noise_std, z = sampler_noise4 of (pixel, step, the row's stream).  noise_std is one
// table scalar, uniform over the launch: a noise_std == 0 row returns before x is touched.
__global__ __launch_bounds__(256) void edm_churn_kernel(float* __restrict__ x, const float* __restrict__ churn, const int* __restrict__ step,
                                                        const uint32_t* __restrict__ seed, const int* __restrict__ streams, int bs, long HW) {
  const int idx = *step;
  const float noise_std = churn[idx * 4 + 1], s_noise = churn[idx * 4 + 2];
  if (noise_std == 0.f) return;
  const uint32_t k0 = seed[0], k1 = seed[1];
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    float z[4];
    sampler_noise4((uint32_t)px, (uint32_t)idx, streams ? (uint32_t)streams[smp] : 0u, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      x[at] = x[at] + (z[c] * s_noise) * noise_std;
    }
  }
}

// the predictor: d = to_d(x, sigma_hat, d0), x_e = the Euler step to sigma_next (euler_update's expression, d kept)
__device__ __forceinline__ float edm_predict(float xv, float d0, float sh, float sn, float& d) {
  d = (xv - d0) / sh;
  return xv + d * (sn - sh);
}

// the corrector: d_new = to_d(x_e, sigma_next, d0'), d' = (d + d_new) / 2, x' = x + d' dt
__device__ __forceinline__ float edm_correct(float xv, float xev, float dv, float d0n, float sh, float sn) {
  const float dnew = (xev - d0n) / sn;
  const float dp = (dv + dnew) / 2.0f;
  return xv + dp * (sn - sh);
}

// x, xe, dir [bs, 4, HW] fp32; xe == x is allowed (same index, elementwise), dir may be null; eps as for cfg_euler_step_cl_kernel
template <int NB>
__global__ __launch_bounds__(256) void cfg_edm_predict_cl_kernel(const float* x, const uint16_t* __restrict__ eps, const float* __restrict__ tab,
                                                                 const int* __restrict__ step, float scale, float scale_im, float* xe,
                                                                 float* __restrict__ dir, int bs, long HW, int ld) {
  const int idx = *step;
  const float sh = tab[idx * 4], sn = tab[idx * 4 + 1], sq = tab[idx * 4 + 3];
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    const EpsRow e = load_eps_row<NB>(eps, bs, HW, ld, smp, px);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      const float xv = x[at];
      float d;
      xe[at] = edm_predict(xv, cfg_combine_cl<NB>(e, c, xv, sq, scale, scale_im), sh, sn, d);
      if (dir) dir[at] = d;
    }
  }
}

// the un-staged form: x [n] fp32, eps [NB n] fp32, row [4] = one row of edm -> xe [n], dir [n] or null
template <int NB>
__global__ __launch_bounds__(256) void cfg_edm_predict_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ row,
                                                              float scale, float scale_im, float* __restrict__ xe, float* __restrict__ dir, long n) {
  const float sh = row[0], sn = row[1], sq = row[3];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float xv = x[i];
    float d;
    xe[i] = edm_predict(xv, cfg_combine_flat<NB>(eps, n, i, xv, sq, scale, scale_im), sh, sn, d);
    if (dir) dir[i] = d;
  }
}

// x [bs, 4, HW] fp32 IN PLACE (it holds x_hat); xe, dir read; eps2 = the network's output at (x_e, sigma_next).  sigma_next is one table
// scalar, uniform over the launch: where it is not > 0 the row is x <- xe and neither eps2 nor dir is read (sampling.py:334-336)
template <int NB>
__global__ __launch_bounds__(256) void cfg_edm_correct_cl_kernel(float* __restrict__ x, const float* __restrict__ xe, const float* __restrict__ dir,
                                                                 const uint16_t* __restrict__ eps, const float* __restrict__ tab,
                                                                 const float* __restrict__ corr, const int* __restrict__ step, float scale,
                                                                 float scale_im, int bs, long HW, int ld) {
  const int idx = *step;
  const float sh = tab[idx * 4], sn = tab[idx * 4 + 1], sqn = corr[idx * 4 + 3];
  const bool correct = sn > 0.f;
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    if (!correct) {
#pragma unroll
      for (int c = 0; c < 4; ++c) x[(smp * 4 + c) * HW + px] = xe[(smp * 4 + c) * HW + px];
      continue;
    }
    const EpsRow e = load_eps_row<NB>(eps, bs, HW, ld, smp, px);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      const float xev = xe[at];
      x[at] = edm_correct(x[at], xev, dir[at], cfg_combine_cl<NB>(e, c, xev, sqn, scale, scale_im), sh, sn);
    }
  }
}

// the un-staged form: x, xe, dir [n] fp32, eps [NB n] fp32, row / crow [4] = one row of edm / corr -> out [n]
template <int NB>
__global__ __launch_bounds__(256) void cfg_edm_correct_kernel(const float* __restrict__ x, const float* __restrict__ xe, const float* __restrict__ dir,
                                                              const float* __restrict__ eps, const float* __restrict__ row,
                                                              const float* __restrict__ crow, float scale, float scale_im, float* __restrict__ out,
                                                              long n) {
  const float sh = row[0], sn = row[1], sqn = crow[3];
  const bool correct = sn > 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float xev = xe[i];
    if (correct)
      out[i] = edm_correct(x[i], xev, dir[i], cfg_combine_flat<NB>(eps, n, i, xev, sqn, scale, scale_im), sh, sn);
    else
      out[i] = xev;
  }
}

// ---- DPM++ 2S ancestral and linear multistep (sampling.py:350-387, 276-311) -------------------------------------------------------------
// include/cd360_highorder.h.  DPM++ 2S evaluates the network twice per step: at (x, sigma) and at (x2, to_sigma(s)), the midpoint in
// -log sigma between sigma and sigma_down, which is NOT on the denoiser's grid: c_out of the second evaluation is sq_mid = q(sigma_mid).
// mid [nsteps, 4] = (sigma_mid, sigma_down, c_in(sq_mid), sq_mid); m2s [nsteps, 4] = (m1, m2, m3, m4) of get_mult; anc as above
// (cd360/sampler.py::dpmpp2s_tables).  Rows with sigma_down = 0 run the ancestral Euler tail above instead (one evaluation).
__device__ __forceinline__ float dpmpp2s_mix(float xv, float d0, float ma, float mb) { return ma * xv - mb * d0; }

// x [bs, 4, HW] fp32 READ; x2 [bs, 4, HW] fp32 written; eps as for cfg_euler_step_cl_kernel; tab [nsteps, 4] (column 0 = sigma)
template <int NB>
__global__ __launch_bounds__(256) void cfg_dpmpp2s_mid_cl_kernel(const float* __restrict__ x, const uint16_t* __restrict__ eps,
                                                                 const float* __restrict__ tab, const float* __restrict__ m2s,
                                                                 const int* __restrict__ step, float scale, float scale_im, float* __restrict__ x2,
                                                                 int bs, long HW, int ld) {
  const int idx = *step;
  const float s = tab[idx * 4], m1 = m2s[idx * 4], m2 = m2s[idx * 4 + 1];
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    const EpsRow e = load_eps_row<NB>(eps, bs, HW, ld, smp, px);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      const float xv = x[at];
      x2[at] = dpmpp2s_mix(xv, cfg_combine_cl<NB>(e, c, xv, s, scale, scale_im), m1, m2);
    }
  }
}

// the un-staged form: x [n] fp32, eps [NB n] fp32, sigma [1], mult [4] = one row of m2s -> x2 [n]
template <int NB>
__global__ __launch_bounds__(256) void cfg_dpmpp2s_mid_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ sigma,
                                                              const float* __restrict__ mult, float scale, float scale_im, float* __restrict__ x2,
                                                              long n) {
  const float s = *sigma, m1 = mult[0], m2 = mult[1];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float xv = x[i];
    x2[i] = dpmpp2s_mix(xv, cfg_combine_flat<NB>(eps, n, i, xv, s, scale, scale_im), m1, m2);
  }
}

// x' = m3 x - m4 d0', d0' combined from x2 at sq_mid; then the ancestral noise where sigma_up != 0 (euler_ancestral_update's last line)
__device__ __forceinline__ float dpmpp2s_update(float xv, float d0n, float m3, float m4, float su, float s_noise, float z, bool noisy) {
  const float xn = dpmpp2s_mix(xv, d0n, m3, m4);
  return noisy ? xn + (z * s_noise) * su : xn;
}

// x [bs, 4, HW] fp32 IN PLACE; x2 read; eps = the network's output at (x2, sigma_mid)
template <int NB>
__global__ __launch_bounds__(256) void cfg_dpmpp2s_step_cl_kernel(float* __restrict__ x, const float* __restrict__ x2, const uint16_t* __restrict__ eps,
                                                                  const float* __restrict__ mid, const float* __restrict__ m2s,
                                                                  const float* __restrict__ anc, const int* __restrict__ step,
                                                                  const uint32_t* __restrict__ seed, const int* __restrict__ streams, float scale,
                                                                  float scale_im, int bs, long HW, int ld) {
  const int idx = *step;
  const float sqm = mid[idx * 4 + 3], m3 = m2s[idx * 4 + 2], m4 = m2s[idx * 4 + 3];
  const float su = anc[idx * 4 + 1], s_noise = anc[idx * 4 + 2];
  const bool noisy = su != 0.f;
  const uint32_t k0 = seed[0], k1 = seed[1];
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    const EpsRow e = load_eps_row<NB>(eps, bs, HW, ld, smp, px);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) sampler_noise4((uint32_t)px, (uint32_t)idx, streams ? (uint32_t)streams[smp] : 0u, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      x[at] = dpmpp2s_update(x[at], cfg_combine_cl<NB>(e, c, x2[at], sqm, scale, scale_im), m3, m4, su, s_noise, z[c], noisy);
    }
  }
}

// the un-staged form: x, x2 [bs, 4, HW] fp32, eps [NB bs, 4, HW] fp32, midrow / mult / ancrow [4] = one row of mid / m2s / anc -> out
template <int NB>
__global__ __launch_bounds__(256) void cfg_dpmpp2s_step_kernel(const float* __restrict__ x, const float* __restrict__ x2, const float* __restrict__ eps,
                                                               const float* __restrict__ midrow, const float* __restrict__ mult,
                                                               const float* __restrict__ ancrow, const uint32_t* __restrict__ seed,
                                                               const int* __restrict__ streams, const int* __restrict__ step, float scale,
                                                               float scale_im, float* __restrict__ out, int bs, long HW) {
  const float sqm = midrow[3], m3 = mult[2], m4 = mult[3];
  const float su = ancrow[1], s_noise = ancrow[2];
  const bool noisy = su != 0.f;
  const uint32_t k0 = seed[0], k1 = seed[1], st = (uint32_t)*step;
  const long total = (long)bs * HW, n = total * 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) sampler_noise4((uint32_t)px, st, streams ? (uint32_t)streams[smp] : 0u, k0, k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      out[at] = dpmpp2s_update(x[at], cfg_combine_flat<NB>(eps, n, at, x2[at], sqm, scale, scale_im), m3, m4, su, s_noise, z[c], noisy);
    }
  }
}

// Linear multistep: d = to_d(x, sigma, d0) goes into slot step % order of a ring of the last `order` directions; x' = x + sum_j c_j d_(step - j)
// over j < min(step + 1, order), newest first, the sum formed before it is added (sampling.py:300-309).  coef = (c_0 .. c_3) of the step,
// zero-padded (cd360/sampler.py::lms_coefficients).  Slots with j >= min(step + 1, order) are NOT read: on the first steps of an image they
// hold the previous image's directions or uninitialised memory, and 0 * NaN must not reach x.  Element `at` of every slot belongs to the
// thread that owns element `at` of x: no thread reads what another writes.
__device__ __forceinline__ float lms_update(float xv, float d0, float s, const float coef[4], float* __restrict__ ring, long slot_elems, long at,
                                            int idx, int order) {
  const float d = (xv - d0) / s;
  ring[(long)(idx % order) * slot_elems + at] = d;
  const int cur = idx + 1 < order ? idx + 1 : order;
  float acc = coef[0] * d;
  for (int j = 1; j < cur; ++j) acc += coef[j] * ring[(long)((idx - j) % order) * slot_elems + at];
  return xv + acc;
}

// x [bs, 4, HW] fp32 IN PLACE; ring [order, bs, 4, HW] fp32; eps as for cfg_euler_step_cl_kernel; tab [nsteps, 4] (column 0 = sigma);
// lms [nsteps, 4]
template <int NB>
__global__ __launch_bounds__(256) void cfg_lms_step_cl_kernel(float* __restrict__ x, float* __restrict__ ring, const uint16_t* __restrict__ eps,
                                                              const float* __restrict__ tab, const float* __restrict__ lms,
                                                              const int* __restrict__ step, float scale, float scale_im, int order, int bs, long HW,
                                                              int ld) {
  const int idx = *step;
  const float s = tab[idx * 4];
  const float coef[4] = {lms[idx * 4], lms[idx * 4 + 1], lms[idx * 4 + 2], lms[idx * 4 + 3]};
  const long total = (long)bs * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long smp = i / HW, px = i - smp * HW;
    const EpsRow e = load_eps_row<NB>(eps, bs, HW, ld, smp, px);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = (smp * 4 + c) * HW + px;
      const float xv = x[at];
      x[at] = lms_update(xv, cfg_combine_cl<NB>(e, c, xv, s, scale, scale_im), s, coef, ring, total * 4, at, idx, order);
    }
  }
}

// the un-staged form: x [n] fp32, eps [NB n] fp32, ring [order, n] fp32 (slot step % order written), sigma [1], row [4] = one row of lms,
// step: device int32 -> out [n]
template <int NB>
__global__ __launch_bounds__(256) void cfg_lms_step_kernel(const float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ ring,
                                                           const float* __restrict__ sigma, const float* __restrict__ row,
                                                           const int* __restrict__ step, float scale, float scale_im, int order,
                                                           float* __restrict__ out, long n) {
  const int idx = *step;
  const float s = *sigma;
  const float coef[4] = {row[0], row[1], row[2], row[3]};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float xv = x[i];
    out[i] = lms_update(xv, cfg_combine_flat<NB>(eps, n, i, xv, s, scale, scale_im), s, coef, ring, n, i, idx, order);
  }
}

// ---- host side of the tails ----
inline unsigned tail_grid(long total) {  // grid-stride kernels: one thread per element up to 65536 workgroups
  const long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

inline bool overlap(const void* a, const void* b, long bytes_a, long bytes_b) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

inline bool overlap(const void* a, const void* b, long bytes) { return overlap(a, b, bytes, bytes); }

// The C ABI takes the two-branch request as a NaN scale_im (include/cd360_hip.h).  It is tested here, on the host: `launch` receives the
// branch count as a compile-time constant and the scale_im its kernel is to see (0.f for two branches), so no kernel ever sees the NaN.
template <class Launch>
inline void launch_for_branches(float scale_im, Launch&& launch) {
  if (std::isnan(scale_im))
    launch(std::integral_constant<int, 2>{}, 0.f);
  else
    launch(std::integral_constant<int, 3>{}, scale_im);
}

// what every `_cl` tail asks of its arguments: eps rows of ld >= 4 channels, ld % 4 == 0 (the 320 -> 4 output convolution writes 16-channel
// rows), 8-byte aligned for the u32x2 loads
inline bool cl_args_ok(const void* x, const void* eps, const void* step_tab, const void* step, int bs, int64_t HW, int ld) {
  return x && eps && step_tab && step && bs > 0 && HW > 0 && ld >= 4 && ld % 4 == 0 && (uintptr_t)eps % 8 == 0;
}

}  // namespace

// See the kernel for layouts.  Cout % 8 == 0, E % 8 == 0; w_k36 = the input convolution's weight as [36, Cout] fp32 (k = (ky * 3 + kx) * 4 + ci).
extern "C" int cd360_unet_stage_in(const void* x, const void* step_tab, const void* step, const void* w_k36, const void* bias, void* h,
                                   const void* temb_tab, const void* lab, void* emb_act, int bs, int rep, int H, int W, int Cout, int E,
                                   void* stream) {
  if (!x || !step_tab || !step || !w_k36 || !bias || !h || !temb_tab || !lab || !emb_act) return CD360_ERR_ARG;
  if (bs <= 0 || rep <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout % 8 || E <= 0 || E % 8) return CD360_ERR_SHAPE;
  if (((uintptr_t)h | (uintptr_t)temb_tab | (uintptr_t)lab | (uintptr_t)emb_act | (uintptr_t)w_k36) % 16) return CD360_ERR_ARG;
  const int lds = (36 * Cout + 3 * (TP + 2) * 4) * 4;
  if (lds > 64 * 1024) return CD360_ERR_SHAPE;
  const int nconv = bs * H * ((W + TP - 1) / TP);
  const int nemb = (int)(((long)rep * bs * (E >> 3) + 255) / 256);
  hipLaunchKernelGGL(unet_stage_in_kernel, dim3((unsigned)(nconv + nemb)), dim3(256), lds, (hipStream_t)stream, (const float*)x,
                     (const float*)step_tab, (const int*)step, (const float*)w_k36, (const float*)bias, (uint16_t*)h, (const uint16_t*)temb_tab,
                     (const uint16_t*)lab, (uint16_t*)emb_act, bs, rep, H, W, Cout, E, nconv);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [n] fp32 latent, sigma / sigma_next: device scalars; eps [3n] fp32 network output (uncond | image-cond | image+text-cond), or, when
// scale_im is NaN, eps [2n] (uncond | image+text-cond); out [n]
extern "C" int cd360_cfg_euler_step_f32(const void* x, const void* eps, const void* sigma, const void* sigma_next, float scale,
                                        float scale_im, void* out, int64_t n, void* stream) {
  if (!x || !eps || !sigma || !sigma_next || !out || n <= 0) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_euler_step_kernel<decltype(nb)::value>, dim3(tail_grid(n)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)eps, (const float*)sigma, (const float*)sigma_next, scale, sim, (float*)out, (long)n);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [bs, 4, HW] fp32 in place; eps [3 bs, HW, ld] bf16, or eps [2 bs, HW, ld] when scale_im is NaN (cl_args_ok)
extern "C" int cd360_cfg_euler_step_cl(void* x, const void* eps, const void* step_tab, const void* step, float scale, float scale_im, int bs,
                                       int64_t HW, int ld, void* stream) {
  if (!cl_args_ok(x, eps, step_tab, step, bs, HW, ld)) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_euler_step_cl_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream,
                       (float*)x, (const uint16_t*)eps, (const float*)step_tab, (const int*)step, scale, sim, bs, (long)HW, ld);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// include/cd360_solvers.h.  x, old [bs, 4, HW] fp32 IN PLACE (distinct buffers); eps, ld and the NaN scale_im as for cd360_cfg_euler_step_cl;
// step_tab [nsteps, 4] (sigma = column 0), mult_tab [nsteps, 4] = (m1, m2, m3, m4)
extern "C" int cd360_cfg_dpmpp2m_step_cl(void* x, void* old, const void* eps, const void* step_tab, const void* mult_tab, const void* step, float scale,
                                         float scale_im, int bs, int64_t HW, int ld, void* stream) {
  if (!cl_args_ok(x, eps, step_tab, step, bs, HW, ld) || !old || !mult_tab || ((uintptr_t)x | (uintptr_t)old) % 4) return CD360_ERR_ARG;
  const long total = (long)bs * HW;
  if (overlap(x, old, total * 4 * (long)sizeof(float))) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_dpmpp2m_step_cl_kernel<decltype(nb)::value>, dim3(tail_grid(total)), dim3(256), 0, (hipStream_t)stream, (float*)x,
                       (float*)old, (const uint16_t*)eps, (const float*)step_tab, (const float*)mult_tab, (const int*)step, scale, sim, bs,
                       (long)HW, ld);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x, old [n] fp32, eps [3n] fp32 (u | ic | c) or, for a NaN scale_im, [2n] (u | c); sigma [1], mult [4] device tensors; out, old_out [n]: buffers of
// their own (neither an input, nor each other)
extern "C" int cd360_cfg_dpmpp2m_step_f32(const void* x, const void* eps, const void* old, const void* sigma, const void* mult, float scale,
                                          float scale_im, void* out, void* old_out, int64_t n, void* stream) {
  if (!x || !eps || !old || !sigma || !mult || !out || !old_out || n <= 0) return CD360_ERR_ARG;
  const long bytes = (long)n * (long)sizeof(float);
  if (overlap(x, old, bytes) || overlap(out, old_out, bytes) || overlap(out, x, bytes) || overlap(out, old, bytes) || overlap(old_out, x, bytes) ||
      overlap(old_out, old, bytes))
    return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_dpmpp2m_step_kernel<decltype(nb)::value>, dim3(tail_grid(n)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)eps, (const float*)old, (const float*)sigma, (const float*)mult, scale, sim, (float*)out, (float*)old_out,
                       (long)n);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// include/cd360_stochastic.h.  out [bs, 4, HW] fp32 standard normals; seed: device int64[1]; streams: device int32[bs] or null; step: device
// int32[1] (noise_args_ok)
extern "C" int cd360_sampler_noise_f32(void* out, const void* seed, const void* streams, const void* step, int bs, int64_t HW, void* stream) {
  if (!out || bs <= 0 || HW <= 0 || !noise_args_ok(seed, streams, step, HW) || (uintptr_t)out % 4) return CD360_ERR_ARG;
  hipLaunchKernelGGL(sampler_noise_kernel, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream, (float*)out, (const uint32_t*)seed,
                     (const int*)streams, (const int*)step, bs, (long)HW);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [bs, 4, HW] fp32, eps [3 bs, 4, HW] fp32 (u | ic | c) or, for a NaN scale_im, [2 bs, 4, HW] (u | c); sigma [1], anc [4] = (sigma_down,
// sigma_up, s_noise, 0) device tensors; out [bs, 4, HW]: a buffer of its own
extern "C" int cd360_cfg_euler_ancestral_step_f32(const void* x, const void* eps, const void* sigma, const void* anc, const void* seed,
                                                  const void* streams, const void* step, float scale, float scale_im, void* out, int bs,
                                                  int64_t HW, void* stream) {
  if (!x || !eps || !sigma || !anc || !out || bs <= 0 || HW <= 0 || !noise_args_ok(seed, streams, step, HW)) return CD360_ERR_ARG;
  const long bytes = (long)bs * 4 * HW * (long)sizeof(float);
  if (overlap(out, x, bytes) || overlap(out, eps, bytes, bytes * (std::isnan(scale_im) ? 2 : 3))) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_euler_ancestral_step_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)x, (const float*)eps, (const float*)sigma, (const float*)anc, (const uint32_t*)seed, (const int*)streams,
                       (const int*)step, scale, sim, (float*)out, bs, (long)HW);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [bs, 4, HW] fp32 IN PLACE; eps, ld and the NaN scale_im as for cd360_cfg_euler_step_cl; step_tab [nsteps, 4] (sigma = column 0),
// anc_tab [nsteps, 4] = (sigma_down, sigma_up, s_noise, 0); step = the row of both tables AND the noise counter's step word
extern "C" int cd360_cfg_euler_ancestral_step_cl(void* x, const void* eps, const void* step_tab, const void* anc_tab, const void* step,
                                                 const void* seed, const void* streams, float scale, float scale_im, int bs, int64_t HW, int ld,
                                                 void* stream) {
  if (!cl_args_ok(x, eps, step_tab, step, bs, HW, ld) || !anc_tab || !noise_args_ok(seed, streams, step, HW) || (uintptr_t)x % 4)
    return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_euler_ancestral_step_cl_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream,
                       (float*)x, (const uint16_t*)eps, (const float*)step_tab, (const float*)anc_tab, (const int*)step, (const uint32_t*)seed,
                       (const int*)streams, scale, sim, bs, (long)HW, ld);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// include/cd360_edm.h.  x [bs, 4, HW] fp32 IN PLACE; churn_tab [nsteps, 4] fp32 = (gamma, noise_std, s_noise, 0); step: device int32, the row
// of the table AND the noise counter's step word; seed / streams as for cd360_sampler_noise_f32 (noise_args_ok)
extern "C" int cd360_edm_churn_f32(void* x, const void* churn_tab, const void* step, const void* seed, const void* streams, int bs, int64_t HW,
                                   void* stream) {
  if (!x || !churn_tab || bs <= 0 || HW <= 0 || !noise_args_ok(seed, streams, step, HW) || ((uintptr_t)x | (uintptr_t)churn_tab) % 4)
    return CD360_ERR_ARG;
  hipLaunchKernelGGL(edm_churn_kernel, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream, (float*)x, (const float*)churn_tab,
                     (const int*)step, (const uint32_t*)seed, (const int*)streams, bs, (long)HW);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x, xe, dir [bs, 4, HW] fp32: xe == x (the in-place form) or a buffer of its own; dir null or a buffer of its own; eps, ld and the NaN
// scale_im as for cd360_cfg_euler_step_cl; edm_tab [nsteps, 4] = (sigma_hat, sigma_next, c_in(sq), sq)
extern "C" int cd360_cfg_edm_predict_cl(const void* x, const void* eps, const void* edm_tab, const void* step, float scale, float scale_im, void* xe,
                                        void* dir, int bs, int64_t HW, int ld, void* stream) {
  if (!cl_args_ok(x, eps, edm_tab, step, bs, HW, ld) || !xe || ((uintptr_t)x | (uintptr_t)xe | (uintptr_t)dir) % 4) return CD360_ERR_ARG;
  const long bytes = (long)bs * 4 * HW * (long)sizeof(float);
  if ((xe != x && overlap(xe, x, bytes)) || (dir && (overlap(dir, x, bytes) || overlap(dir, xe, bytes)))) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_edm_predict_cl_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)x, (const uint16_t*)eps, (const float*)edm_tab, (const int*)step, scale, sim, (float*)xe, (float*)dir, bs,
                       (long)HW, ld);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [n] fp32, eps [3n] fp32 (u | ic | c) or, for a NaN scale_im, [2n] (u | c); row [4] = one row of edm_tab, a device tensor; xe [n] and
// dir [n] (or null): buffers of their own (neither an input, nor each other)
extern "C" int cd360_cfg_edm_predict_f32(const void* x, const void* eps, const void* row, float scale, float scale_im, void* xe, void* dir,
                                         int64_t n, void* stream) {
  if (!x || !eps || !row || !xe || n <= 0) return CD360_ERR_ARG;
  const long bytes = (long)n * (long)sizeof(float), ebytes = bytes * (std::isnan(scale_im) ? 2 : 3);
  if (overlap(xe, x, bytes) || overlap(xe, eps, bytes, ebytes)) return CD360_ERR_ARG;
  if (dir && (overlap(dir, x, bytes) || overlap(dir, eps, bytes, ebytes) || overlap(dir, xe, bytes))) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_edm_predict_kernel<decltype(nb)::value>, dim3(tail_grid(n)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)eps, (const float*)row, scale, sim, (float*)xe, (float*)dir, (long)n);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [bs, 4, HW] fp32 IN PLACE; xe, dir [bs, 4, HW] fp32, read: three distinct buffers; eps2, ld and the NaN scale_im as for
// cd360_cfg_euler_step_cl; edm_tab as above, corr_tab [nsteps, 4] = (sigma_next, sigma_next, c_in(sq'), sq') with sq' = q(sigma_next)
extern "C" int cd360_cfg_edm_correct_cl(void* x, const void* xe, const void* dir, const void* eps2, const void* edm_tab, const void* corr_tab,
                                        const void* step, float scale, float scale_im, int bs, int64_t HW, int ld, void* stream) {
  if (!cl_args_ok(x, eps2, edm_tab, step, bs, HW, ld) || !xe || !dir || !corr_tab || ((uintptr_t)x | (uintptr_t)xe | (uintptr_t)dir) % 4)
    return CD360_ERR_ARG;
  const long bytes = (long)bs * 4 * HW * (long)sizeof(float);
  if (overlap(x, xe, bytes) || overlap(x, dir, bytes) || overlap(xe, dir, bytes)) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_edm_correct_cl_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream, (float*)x,
                       (const float*)xe, (const float*)dir, (const uint16_t*)eps2, (const float*)edm_tab, (const float*)corr_tab, (const int*)step,
                       scale, sim, bs, (long)HW, ld);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x, xe, dir [n] fp32, eps2 [3n] fp32 or, for a NaN scale_im, [2n]; row / corr_row [4] = one row of edm_tab / corr_tab, device tensors; out [n]: a
// buffer of its own
extern "C" int cd360_cfg_edm_correct_f32(const void* x, const void* xe, const void* dir, const void* eps2, const void* row, const void* corr_row,
                                         float scale, float scale_im, void* out, int64_t n, void* stream) {
  if (!x || !xe || !dir || !eps2 || !row || !corr_row || !out || n <= 0) return CD360_ERR_ARG;
  const long bytes = (long)n * (long)sizeof(float);
  if (overlap(out, x, bytes) || overlap(out, xe, bytes) || overlap(out, dir, bytes) || overlap(out, eps2, bytes, bytes * (std::isnan(scale_im) ? 2 : 3)))
    return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_edm_correct_kernel<decltype(nb)::value>, dim3(tail_grid(n)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)xe, (const float*)dir, (const float*)eps2, (const float*)row, (const float*)corr_row, scale, sim, (float*)out,
                       (long)n);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// include/cd360_highorder.h.  x [bs, 4, HW] fp32, read; x2 [bs, 4, HW] fp32: a buffer of its own; eps, ld and the NaN scale_im as for
// cd360_cfg_euler_step_cl; step_tab [nsteps, 4] (sigma = column 0), mult2s_tab [nsteps, 4] = (m1, m2, m3, m4)
extern "C" int cd360_cfg_dpmpp2s_mid_cl(const void* x, const void* eps, const void* step_tab, const void* mult2s_tab, const void* step, float scale,
                                        float scale_im, void* x2, int bs, int64_t HW, int ld, void* stream) {
  if (!cl_args_ok(x, eps, step_tab, step, bs, HW, ld) || !mult2s_tab || !x2 || ((uintptr_t)x | (uintptr_t)x2) % 4) return CD360_ERR_ARG;
  if (overlap(x, x2, (long)bs * 4 * HW * (long)sizeof(float))) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_dpmpp2s_mid_cl_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)x, (const uint16_t*)eps, (const float*)step_tab, (const float*)mult2s_tab, (const int*)step, scale, sim,
                       (float*)x2, bs, (long)HW, ld);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [n] fp32, eps [3n] fp32 (u | ic | c) or, for a NaN scale_im, [2n] (u | c); sigma [1], mult [4] = one row of mult2s_tab, device tensors; x2 [n]:
// a buffer of its own
extern "C" int cd360_cfg_dpmpp2s_mid_f32(const void* x, const void* eps, const void* sigma, const void* mult, float scale, float scale_im, void* x2,
                                         int64_t n, void* stream) {
  if (!x || !eps || !sigma || !mult || !x2 || n <= 0) return CD360_ERR_ARG;
  const long bytes = (long)n * (long)sizeof(float);
  if (overlap(x2, x, bytes) || overlap(x2, eps, bytes, bytes * (std::isnan(scale_im) ? 2 : 3))) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_dpmpp2s_mid_kernel<decltype(nb)::value>, dim3(tail_grid(n)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)eps, (const float*)sigma, (const float*)mult, scale, sim, (float*)x2, (long)n);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [bs, 4, HW] fp32 IN PLACE; x2 [bs, 4, HW] fp32, read: distinct buffers; eps2, ld and the NaN scale_im as for cd360_cfg_euler_step_cl;
// mid_tab [nsteps, 4] = (sigma_mid, sigma_down, c_in(sq_mid), sq_mid), mult2s_tab as above, anc_tab [nsteps, 4] = (sigma_down, sigma_up,
// s_noise, 0); step = the row of the three tables AND the noise counter's step word
extern "C" int cd360_cfg_dpmpp2s_step_cl(void* x, const void* x2, const void* eps2, const void* mid_tab, const void* mult2s_tab, const void* anc_tab,
                                         const void* step, const void* seed, const void* streams, float scale, float scale_im, int bs, int64_t HW,
                                         int ld, void* stream) {
  if (!cl_args_ok(x, eps2, mid_tab, step, bs, HW, ld) || !x2 || !mult2s_tab || !anc_tab || !noise_args_ok(seed, streams, step, HW) ||
      ((uintptr_t)x | (uintptr_t)x2) % 4)
    return CD360_ERR_ARG;
  if (overlap(x, x2, (long)bs * 4 * HW * (long)sizeof(float))) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_dpmpp2s_step_cl_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream, (float*)x,
                       (const float*)x2, (const uint16_t*)eps2, (const float*)mid_tab, (const float*)mult2s_tab, (const float*)anc_tab,
                       (const int*)step, (const uint32_t*)seed, (const int*)streams, scale, sim, bs, (long)HW, ld);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x, x2 [bs, 4, HW] fp32, eps2 [3 bs, 4, HW] fp32 or, for a NaN scale_im, [2 bs, 4, HW]; mid_row / mult / anc [4] = one row of mid_tab /
// mult2s_tab / anc_tab, device tensors; out [bs, 4, HW]: a buffer of its own
extern "C" int cd360_cfg_dpmpp2s_step_f32(const void* x, const void* x2, const void* eps2, const void* mid_row, const void* mult, const void* anc,
                                          const void* seed, const void* streams, const void* step, float scale, float scale_im, void* out, int bs,
                                          int64_t HW, void* stream) {
  if (!x || !x2 || !eps2 || !mid_row || !mult || !anc || !out || bs <= 0 || HW <= 0 || !noise_args_ok(seed, streams, step, HW)) return CD360_ERR_ARG;
  const long bytes = (long)bs * 4 * HW * (long)sizeof(float);
  if (overlap(out, x, bytes) || overlap(out, x2, bytes) || overlap(out, eps2, bytes, bytes * (std::isnan(scale_im) ? 2 : 3))) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_dpmpp2s_step_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)x, (const float*)x2, (const float*)eps2, (const float*)mid_row, (const float*)mult, (const float*)anc,
                       (const uint32_t*)seed, (const int*)streams, (const int*)step, scale, sim, (float*)out, bs, (long)HW);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [bs, 4, HW] fp32 IN PLACE; ring [order, bs, 4, HW] fp32: slot step % order written, the min(step + 1, order) - 1 slots before it read; eps,
// ld and the NaN scale_im as for cd360_cfg_euler_step_cl; step_tab [nsteps, 4] (sigma = column 0), lms_tab [nsteps, 4] = (c_0 .. c_3); order 1..4
extern "C" int cd360_cfg_lms_step_cl(void* x, void* ring, const void* eps, const void* step_tab, const void* lms_tab, const void* step, float scale,
                                     float scale_im, int order, int bs, int64_t HW, int ld, void* stream) {
  if (!cl_args_ok(x, eps, step_tab, step, bs, HW, ld) || !ring || !lms_tab || order < 1 || order > 4 || ((uintptr_t)x | (uintptr_t)ring) % 4)
    return CD360_ERR_ARG;
  const long bytes = (long)bs * 4 * HW * (long)sizeof(float);
  if (overlap(x, ring, bytes, bytes * order)) return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_lms_step_cl_kernel<decltype(nb)::value>, dim3(tail_grid((long)bs * HW)), dim3(256), 0, (hipStream_t)stream, (float*)x,
                       (float*)ring, (const uint16_t*)eps, (const float*)step_tab, (const float*)lms_tab, (const int*)step, scale, sim, order, bs,
                       (long)HW, ld);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

// x [n] fp32, eps [3n] fp32 or, for a NaN scale_im, [2n]; ring [order, n] fp32, slot step % order written; sigma [1], row [4] = one row of
// lms_tab, step [1] int32: device tensors; out [n]: a buffer of its own (neither an input nor the ring)
extern "C" int cd360_cfg_lms_step_f32(const void* x, const void* eps, void* ring, const void* sigma, const void* row, const void* step, float scale,
                                      float scale_im, int order, void* out, int64_t n, void* stream) {
  if (!x || !eps || !ring || !sigma || !row || !step || !out || n <= 0 || order < 1 || order > 4) return CD360_ERR_ARG;
  const long bytes = (long)n * (long)sizeof(float), ebytes = bytes * (std::isnan(scale_im) ? 2 : 3);
  if (overlap(out, x, bytes) || overlap(out, eps, bytes, ebytes) || overlap(out, ring, bytes, bytes * order) || overlap(ring, x, bytes * order, bytes) ||
      overlap(ring, eps, bytes * order, ebytes))
    return CD360_ERR_ARG;
  launch_for_branches(scale_im, [&](auto nb, float sim) {
    hipLaunchKernelGGL(cfg_lms_step_kernel<decltype(nb)::value>, dim3(tail_grid(n)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)eps, (float*)ring, (const float*)sigma, (const float*)row, (const int*)step, scale, sim, order, (float*)out,
                       (long)n);
  });
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
