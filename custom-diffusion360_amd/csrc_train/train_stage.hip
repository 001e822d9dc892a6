// libcd360_train.so (include/train/cd360_train.h): the two ends of a captured fine-tuning step.
//   train_sigmas_kernel   the per-sample draws of StandardDiffusionLossImgRef.__call__ and the scalars DiscreteDenoiser derives from them
//   train_noise_kernel    x_t = x0 + z' sigma, x_in = x_t c_in, and the twice-noised, scaled reference views
//   train_l2_kernel       loss[b] = sum w (eps c_out + x_t c_skip - x0)^2 [mask] / den[b]
//   train_l2_bwd_kernel   its gradient with respect to eps, in eps's dtype and layout
// Every random number is the generator of ../csrc/cd360_philox.h in counter domains 4-7: a pure function of (seed, stream, step, channel,
// pixel), whatever the grid, the batch size or the row's place in the batch.  One fp32 rounding per operation, in the header's order (the
// build passes -ffp-contract=off).  All four are memory-bound or tiny: a thread owns four neighbouring pixels of one image, so every
// channel plane is read and written as 16-byte vectors along consecutive lanes; sizes that do not allow that take the scalar form of the
// same loop; a bf16 plane is 8 bytes per four pixels, so the bulk pass takes eight pixels per thread where it writes bf16.  The sum of c) is formed by one workgroup per sample in a fixed order; there is no cross-workgroup accumulation anywhere.
#include "../csrc/cd360_philox.h"

// as include/train/cd360_train.h defines them (tests/test_train_stage_cpu.py holds the two together)
#define CD360_TRAIN_ROW 12
#define CD360_TRAIN_CUBIC 0
#define CD360_TRAIN_DISCRETE 1

namespace {

constexpr int ROW = CD360_TRAIN_ROW;
constexpr int L2_THREADS = 1024;

// ------------------------------------------------------------------------------------------------ a) scalars
__device__ __forceinline__ long sample_index(int kind, uint32_t r, int num_idx, int start) {
  long idx;
  if (kind == CD360_TRAIN_CUBIC) {
    const float u = (float)(r >> 8) * 0x1p-24f;
    idx = (long)((1.0f - u * u * u) * (float)(num_idx - 1));
  } else {
    idx = (long)start + (long)(r % (uint32_t)(num_idx - start));
  }
  return idx < 0 ? 0 : (idx > num_idx - 1 ? num_idx - 1 : idx);  // no effect on a valid draw: the table is never read out of bounds
}

__device__ __forceinline__ void take_nearer(float& d, int& i, float od, int oi) {
  if (od < d || (od == d && oi < i)) d = od, i = oi;
}

// one workgroup for the whole batch: every thread reads *step before thread 0 rewrites it
__global__ __launch_bounds__(256) void train_sigmas_kernel(const float* __restrict__ table, int n_table, const float* __restrict__ tgt, int n_tgt,
                                                           int tgt_kind, int tgt_start, const float* __restrict__ ref, int n_ref, int ref_kind,
                                                           int ref_start, const uint32_t* __restrict__ seed, const int* __restrict__ streams,
                                                           uint32_t* step, int advance, float* __restrict__ rows,
                                                           long long* __restrict__ timesteps, long long* __restrict__ ref_idx,
                                                           uint32_t* __restrict__ step_used, int B) {
  __shared__ float s_d[2][256];
  __shared__ int s_i[2][256];
  const int tid = threadIdx.x;
  const uint32_t st = *step;
  const uint32_t k0 = seed[0], k1 = seed[1];
  __syncthreads();
  if (tid == 0) {
    *step_used = st;
    if (advance) *step = st + 1u;
  }
  for (int b = 0; b < B; ++b) {
    uint32_t r[4];
    philox4x32_10(0u, st, streams ? (uint32_t)streams[b] : 0u, CD360_NOISE_TRAIN_SIGMA, k0, k1, r);
    const float sigma = tgt[sample_index(tgt_kind, r[0], n_tgt, tgt_start)];
    const float sigma_ref = ref[sample_index(ref_kind, r[1], n_ref, ref_start)];
    float d0 = INFINITY, d1 = INFINITY;
    int i0 = 0, i1 = 0;
    for (int i = tid; i < n_table; i += 256) {
      const float t = table[i];
      const float e0 = fabsf(sigma - t), e1 = fabsf(sigma_ref - t);
      if (e0 < d0) d0 = e0, i0 = i;
      if (e1 < d1) d1 = e1, i1 = i;
    }
    s_d[0][tid] = d0, s_i[0][tid] = i0, s_d[1][tid] = d1, s_i[1][tid] = i1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        take_nearer(s_d[0][tid], s_i[0][tid], s_d[0][tid + s], s_i[0][tid + s]);
        take_nearer(s_d[1][tid], s_i[1][tid], s_d[1][tid + s], s_i[1][tid + s]);
      }
      __syncthreads();
    }
    if (tid == 0) {
      float off_tgt, off_ref;
      box_muller(r[2], r[3], off_tgt, off_ref);
      float* row = rows + (long)b * ROW;
      row[0] = sigma;
      row[1] = 1.0f / (sigma * sigma);
      row[2] = 1.0f;
      row[3] = -sigma;
      row[4] = 1.0f / sqrtf(sigma * sigma + 1.0f);
      row[5] = sigma_ref;
      row[6] = 1.0f / sqrtf(sigma_ref * sigma_ref + 1.0f);
      row[7] = off_tgt;
      row[8] = off_ref;
      row[9] = row[10] = row[11] = 0.0f;
      timesteps[b] = s_i[0][0];
      ref_idx[b] = s_i[1][0];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ four neighbouring values of a plane
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, long at, int cnt, float v[4]) {
  if (VEC) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(p + at);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[at + j] : 0.0f;
  }
}

template <bool VEC, bool BF>
__device__ __forceinline__ void store4(void* __restrict__ p, long at, int cnt, const float v[4]) {
  if (BF) {
    uint16_t* q = reinterpret_cast<uint16_t*>(p) + at;
    if (VEC) {
      const u32x2 w = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
      *reinterpret_cast<u32x2*>(q) = w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) q[j] = f32_to_bf16(v[j]);
    }
  } else {
    float* q = reinterpret_cast<float*>(p) + at;
    if (VEC) {
      const f32x4 w = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(q) = w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) q[j] = v[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------ b) the bulk pass
// what a unit needs of its image: the same for a target and for a reference view
struct NoiseUnit {
  const float* src;  // x0 or xr
  long img;          // b, or b n + view: the image's index among the [4, HW] images of src
  float s, cc, off, keep;
  bool is_ref, scale;
  uint32_t strm, word0;  // the pixel word of the image's first pixel: view * HW
};

// four neighbouring pixels from px0: y = src [* keep] + za' s; a target stores y as x_t and hands back y c, a view hands back (y + zb s) c
template <bool VEC>
__device__ __forceinline__ void noise_quad(const NoiseUnit& q, long px0, int cnt, long HW, uint32_t st, uint32_t k0, uint32_t k1, float level,
                                           float* __restrict__ x_t, float out[4][4]) {
  const bool offset = level > 0.0f;
  float za[4][4], zb[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < cnt) {
      const uint32_t word = q.word0 + (uint32_t)(px0 + j);  // n HW <= 2^32: checked on the host
      noise4(word, st, q.strm, q.is_ref ? CD360_NOISE_TRAIN_REF_A : CD360_NOISE_TRAIN_TARGET, k0, k1, za[j]);
      if (q.is_ref) noise4(word, st, q.strm, CD360_NOISE_TRAIN_REF_B, k0, k1, zb[j]);
    }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const long at = (q.img * 4 + c) * HW + px0;
    float v[4], y[4];
    load4<VEC>(q.src, at, cnt, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = j < cnt ? za[j][c] : 0.0f;
      if (offset) a = a + level * q.off;
      const float base = q.scale ? q.keep * v[j] : v[j];
      y[j] = base + a * q.s;
      float last = y[j];
      if (q.is_ref) last = y[j] + (j < cnt ? zb[j][c] : 0.0f) * q.s;
      out[c][j] = last * q.cc;
    }
    if (!q.is_ref) store4<VEC, false>(x_t, at, cnt, y);
  }
}

// a unit = PX neighbouring pixels (G = ceil(HW / PX) units per image) of a target image (units [0, B G)) or of a reference view (the
// rest).  PX = 4: fp32 planes go as 16-byte vectors (VEC: HW % 4 == 0, every base pointer aligned for its vector), bf16 output as 8-byte
// ones.  PX = 8 (bf16 output, HW % 8 == 0, 16-byte aligned outputs): two quads, so that the bf16 planes too are written 16 bytes at a time.
template <int PX, bool VEC, bool BF>
__global__ __launch_bounds__(256) void train_noise_kernel(const float* __restrict__ x0, const float* __restrict__ xr, const float* __restrict__ drop,
                                                          const float* __restrict__ rows, const uint32_t* __restrict__ seed,
                                                          const int* __restrict__ streams, const uint32_t* __restrict__ step_used, float level,
                                                          float* __restrict__ x_t, void* __restrict__ x_in, void* __restrict__ xr_in, int B, int n,
                                                          long HW, long G) {
  static_assert(PX == 4 || (PX == 8 && VEC && BF), "eight pixels per unit: the vector form with bf16 output only");
  const uint32_t k0 = seed[0], k1 = seed[1], st = *step_used;
  const long tgt_units = (long)B * G, total = tgt_units * (1 + (xr ? n : 0));
  for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long)gridDim.x * blockDim.x) {
    NoiseUnit q;
    q.is_ref = u >= tgt_units;
    const long v0 = q.is_ref ? u - tgt_units : u;
    q.img = v0 / G;
    const long px0 = (v0 - q.img * G) * PX;
    const long b = q.is_ref ? q.img / n : q.img, view = q.is_ref ? q.img - b * n : 0;
    const float* row = rows + b * ROW;
    q.s = q.is_ref ? row[5] : row[0], q.cc = q.is_ref ? row[6] : row[4], q.off = q.is_ref ? row[8] : row[7];
    q.scale = q.is_ref && drop;
    q.keep = q.scale ? drop[b] : 1.0f;
    q.strm = streams ? (uint32_t)streams[b] : 0u;
    q.word0 = (uint32_t)(view * HW);
    q.src = q.is_ref ? xr : x0;
    void* dst = q.is_ref ? xr_in : x_in;
    if (PX == 8) {
      float lo[4][4], hi[4][4];
      noise_quad<true>(q, px0, 4, HW, st, k0, k1, level, x_t, lo);
      noise_quad<true>(q, px0 + 4, 4, HW, st, k0, k1, level, x_t, hi);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const u32x4 w = {pack_bf16x2(lo[c][0], lo[c][1]), pack_bf16x2(lo[c][2], lo[c][3]), pack_bf16x2(hi[c][0], hi[c][1]), pack_bf16x2(hi[c][2], hi[c][3])};
        *reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(dst) + (q.img * 4 + c) * HW + px0) = w;
      }
    } else {
      const int cnt = HW - px0 < 4 ? (int)(HW - px0) : 4;
      float out[4][4];
      noise_quad<VEC>(q, px0, cnt, HW, st, k0, k1, level, x_t, out);
#pragma unroll
      for (int c = 0; c < 4; ++c) store4<VEC, BF>(dst, (q.img * 4 + c) * HW + px0, cnt, out[c]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ c), d) the l2 term
// how the 16 values (4 channels x 4 neighbouring pixels) of a unit of eps are reached
enum { EPS_STRIDED = 0, EPS_PLANES = 1, EPS_CHANNELS_LAST = 2 };  // scalar by strides | [B, 4, HW] dense | [B, HW, 4] dense; 1, 2: vectors

struct Strides {
  long b, c, h, w;
};

template <bool BF>
__device__ __forceinline__ float eps_at(const void* __restrict__ p, long at) {
  return BF ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p)[at]) : reinterpret_cast<const float*>(p)[at];
}

// e[c][j] = eps[b, c, px0 + j]
template <int MODE, bool BF>
__device__ __forceinline__ void load_eps(const void* __restrict__ eps, Strides s, long b, long px0, int cnt, int W, float e[4][4]) {
  if (MODE == EPS_CHANNELS_LAST && BF) {  // a pixel's four channels are 8 bytes: two pixels per 16-byte vector
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(eps) + b * s.b + (px0 + j) * 4);
      e[0][j] = bf16lo_to_f32(w.x), e[1][j] = bf16hi_to_f32(w.x), e[2][j] = bf16lo_to_f32(w.y), e[3][j] = bf16hi_to_f32(w.y);
      e[0][j + 1] = bf16lo_to_f32(w.z), e[1][j + 1] = bf16hi_to_f32(w.z), e[2][j + 1] = bf16lo_to_f32(w.w), e[3][j + 1] = bf16hi_to_f32(w.w);
    }
  } else if (MODE == EPS_CHANNELS_LAST) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(eps) + b * s.b + (px0 + j) * 4);
      e[0][j] = w.x, e[1][j] = w.y, e[2][j] = w.z, e[3][j] = w.w;
    }
  } else if (MODE == EPS_PLANES) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long at = b * s.b + c * s.c + px0;
      if (BF) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(eps) + at);
        e[c][0] = bf16lo_to_f32(w.x), e[c][1] = bf16hi_to_f32(w.x), e[c][2] = bf16lo_to_f32(w.y), e[c][3] = bf16hi_to_f32(w.y);
      } else {
        const f32x4 w = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(eps) + at);
        e[c][0] = w.x, e[c][1] = w.y, e[c][2] = w.z, e[c][3] = w.w;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long px = px0 + j, h = px / W, w = px - h * W;
#pragma unroll
      for (int c = 0; c < 4; ++c) e[c][j] = j < cnt ? eps_at<BF>(eps, b * s.b + c * s.c + h * s.h + w * s.w) : 0.0f;
    }
  }
}

template <int MODE, bool BF>
__device__ __forceinline__ void store_eps(void* __restrict__ out, Strides s, long b, long px0, int cnt, int W, const float e[4][4]) {
  if (MODE == EPS_CHANNELS_LAST && BF) {
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
      const u32x4 w = {pack_bf16x2(e[0][j], e[1][j]), pack_bf16x2(e[2][j], e[3][j]), pack_bf16x2(e[0][j + 1], e[1][j + 1]), pack_bf16x2(e[2][j + 1], e[3][j + 1])};
      *reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(out) + b * s.b + (px0 + j) * 4) = w;
    }
  } else if (MODE == EPS_CHANNELS_LAST) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v[4] = {e[0][j], e[1][j], e[2][j], e[3][j]};
      store4<true, false>(out, b * s.b + (px0 + j) * 4, 4, v);
    }
  } else if (MODE == EPS_PLANES) {
#pragma unroll
    for (int c = 0; c < 4; ++c) store4<true, BF>(out, b * s.b + c * s.c + px0, 4, e[c]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long px = px0 + j, h = px / W, w = px - h * W;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (j < cnt) {
          const long at = b * s.b + c * s.c + h * s.h + w * s.w;
          if (BF)
            reinterpret_cast<uint16_t*>(out)[at] = f32_to_bf16(e[c][j]);
          else
            reinterpret_cast<float*>(out)[at] = e[c][j];
        }
    }
  }
}

// err[c][j] of a unit and its mask values m[j] (1 without a mask)
template <int MODE, bool BF>
__device__ __forceinline__ void unit_err(const void* __restrict__ eps, Strides s, const float* __restrict__ x_t, const float* __restrict__ x0,
                                         const float* __restrict__ mask, float c_out, float c_skip, long b, long px0, int cnt, long HW, int W,
                                         float err[4][4], float m[4]) {
  constexpr bool VEC = MODE != EPS_STRIDED;
  float e[4][4];
  load_eps<MODE, BF>(eps, s, b, px0, cnt, W, e);
  if (mask) {
    load4<VEC>(mask, b * HW + px0, cnt, m);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = 1.0f;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float xt[4], xz[4];
    load4<VEC>(x_t, (b * 4 + c) * HW + px0, cnt, xt);
    load4<VEC>(x0, (b * 4 + c) * HW + px0, cnt, xz);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float D = e[c][j] * c_out + xt[j] * c_skip;
      err[c][j] = D - xz[j];
    }
  }
}

// one workgroup per sample; thread t sums units t, t + 1024, ... in rising order, then a fixed tree: lanes of a wave, then the 16 waves
template <int MODE, bool BF>
__global__ __launch_bounds__(L2_THREADS) void train_l2_kernel(const void* __restrict__ eps, Strides s, const float* __restrict__ x_t,
                                                              const float* __restrict__ x0, const float* __restrict__ rows,
                                                              const float* __restrict__ mask, float* __restrict__ loss, float* __restrict__ den,
                                                              long HW, int W, long G) {
  __shared__ float s_sum[L2_THREADS / 64], s_msk[L2_THREADS / 64];
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* row = rows + b * ROW;
  const float w = row[1], c_skip = row[2], c_out = row[3];
  float sum = 0.0f, msum = 0.0f;
  for (long g = tid; g < G; g += L2_THREADS) {
    const long px0 = g * 4;
    const int cnt = HW - px0 < 4 ? (int)(HW - px0) : 4;
    float err[4][4], m[4];
    unit_err<MODE, BF>(eps, s, x_t, x0, mask, c_out, c_skip, b, px0, cnt, HW, W, err, m);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float t = err[c][j] * err[c][j];
          t = w * t;
          if (mask) t = t * m[j];
          sum = sum + t;
        }
        msum = msum + m[j];
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum = sum + __shfl_down(sum, o, 64);
    msum = msum + __shfl_down(msum, o, 64);
  }
  if ((tid & 63) == 0) s_sum[tid >> 6] = sum, s_msk[tid >> 6] = msum;
  __syncthreads();
  if (tid == 0) {
    float total = 0.0f, mtotal = 0.0f;
    for (int i = 0; i < L2_THREADS / 64; ++i) total = total + s_sum[i], mtotal = mtotal + s_msk[i];
    const float d = mask ? mtotal + 1e-6f : (float)(4 * HW);
    den[b] = d;
    loss[b] = total / d;
  }
}

template <int MODE, bool BF>
__global__ __launch_bounds__(256) void train_l2_bwd_kernel(const void* __restrict__ eps, Strides s, const float* __restrict__ x_t,
                                                           const float* __restrict__ x0, const float* __restrict__ rows,
                                                           const float* __restrict__ mask, const float* __restrict__ den,
                                                           const float* __restrict__ gr, void* __restrict__ d_eps, Strides ds, int B, long HW, int W,
                                                           long G) {
  const long total = (long)B * G;
  for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long)gridDim.x * blockDim.x) {
    const long b = u / G, px0 = (u - b * G) * 4;
    const int cnt = HW - px0 < 4 ? (int)(HW - px0) : 4;
    const float* row = rows + b * ROW;
    const float w2 = 2.0f * row[1], c_skip = row[2], c_out = row[3], d = den[b], gb = gr[b];
    float err[4][4], m[4];
    unit_err<MODE, BF>(eps, s, x_t, x0, mask, c_out, c_skip, b, px0, cnt, HW, W, err, m);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = w2 * err[c][j];
        t = t * c_out;
        if (mask) t = t * m[j];
        t = t / d;
        err[c][j] = gb == 0.0f ? 0.0f : gb * t;
      }
    store_eps<MODE, BF>(d_eps, ds, b, px0, cnt, W, err);
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline unsigned stride_grid(long total) {  // grid-stride kernels: one thread per unit up to 65536 workgroups
  const long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g < 65536 ? g : 65536));
}

inline bool overlap(const void* a, long bytes_a, const void* b, long bytes_b) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

inline bool aligned(const void* p, uintptr_t to) { return (uintptr_t)p % to == 0; }

inline bool sampler_args_bad(int kind) { return kind != CD360_TRAIN_CUBIC && kind != CD360_TRAIN_DISCRETE; }

inline bool sampler_shape_bad(int kind, int num_idx, int start) {
  return kind == CD360_TRAIN_DISCRETE ? (start < 0 || start >= num_idx) : num_idx > (1 << 24);
}

// the vector form eps (and d_eps) allows, EPS_STRIDED if none: the strides of a dense layout, HW % 4 == 0, and the base pointer and every
// image on a 16-byte boundary (fp32: a vector of four values; bf16 channels-last: of two pixels; bf16 planes are read 8 bytes at a time)
inline int eps_mode(const void* p, const int64_t* s, int elem, int H, int W) {
  const long HW = (long)H * W;
  if (HW % 4 != 0 || !aligned(p, 16) || (s[0] * elem) % 16 != 0) return EPS_STRIDED;
  if (s[1] == 1 && s[3] == 4 && s[2] == 4L * W) return EPS_CHANNELS_LAST;
  if (s[3] == 1 && s[2] == W && s[1] == HW) return EPS_PLANES;
  return EPS_STRIDED;
}

inline Strides strides_of(const int64_t* s) { return Strides{(long)s[0], (long)s[1], (long)s[2], (long)s[3]}; }

inline int l2_args(const void* eps, int eps_dtype, const int64_t* st, const void* x_t, const void* x0, const void* rows, const void* mask, int B,
                   int H, int W) {
  if (!eps || !st || !x_t || !x0 || !rows || B <= 0 || H <= 0 || W <= 0 || (eps_dtype != 0 && eps_dtype != 1)) return CD360_ERR_ARG;
  if (!aligned(eps, eps_dtype ? 2 : 4) || !aligned(x_t, 4) || !aligned(x0, 4) || !aligned(rows, 4) || !aligned(mask, 4)) return CD360_ERR_ARG;
  if (st[0] < 0 || st[1] < 0 || st[2] < 0 || st[3] < 0 || (long)H * W > (1L << 28)) return CD360_ERR_SHAPE;
  return CD360_OK;
}

}  // namespace

extern "C" int cd360_train_sigmas_f32(const void* table, int n_table, const void* tgt_table, int n_tgt, int tgt_kind, int tgt_start,
                                      const void* ref_table, int n_ref, int ref_kind, int ref_start, const void* seed, const void* streams,
                                      void* step, int advance, void* rows, void* timesteps, void* sigmas_ref_idx, void* step_used, int B,
                                      void* stream) {
  if (!table || !tgt_table || !ref_table || !rows || !timesteps || !sigmas_ref_idx || !step_used || B <= 0) return CD360_ERR_ARG;
  if (n_table <= 0 || n_tgt <= 0 || n_ref <= 0 || sampler_args_bad(tgt_kind) || sampler_args_bad(ref_kind)) return CD360_ERR_ARG;
  if (!noise_args_ok(seed, streams, step, 1)) return CD360_ERR_ARG;
  if (!aligned(table, 4) || !aligned(tgt_table, 4) || !aligned(ref_table, 4) || !aligned(rows, 4) || !aligned(step_used, 4) ||
      !aligned(timesteps, 8) || !aligned(sigmas_ref_idx, 8))
    return CD360_ERR_ARG;
  if (overlap(step, 4, step_used, 4) || overlap(step, 4, rows, (long)B * ROW * 4) || overlap(step, 4, timesteps, (long)B * 8) ||
      overlap(step, 4, sigmas_ref_idx, (long)B * 8) || overlap(step, 4, seed, 8) || overlap(step, 4, streams ? streams : step_used, streams ? (long)B * 4 : 4))
    return CD360_ERR_ARG;
  if (sampler_shape_bad(tgt_kind, n_tgt, tgt_start) || sampler_shape_bad(ref_kind, n_ref, ref_start)) return CD360_ERR_SHAPE;
  hipLaunchKernelGGL(train_sigmas_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)table, n_table, (const float*)tgt_table, n_tgt,
                     tgt_kind, tgt_start, (const float*)ref_table, n_ref, ref_kind, ref_start, (const uint32_t*)seed, (const int*)streams,
                     (uint32_t*)step, advance, (float*)rows, (long long*)timesteps, (long long*)sigmas_ref_idx, (uint32_t*)step_used, B);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_train_noise_f32(const void* x0, const void* xr, const void* drop_im, const void* rows, const void* seed, const void* streams,
                                     const void* step_used, float level, void* x_t, void* x_in, void* xr_in, int out_dtype, int B, int n,
                                     int64_t HW, void* stream) {
  if (!x0 || !rows || !x_t || !x_in || B <= 0 || HW <= 0 || (out_dtype != 0 && out_dtype != 1)) return CD360_ERR_ARG;
  if (xr && (!xr_in || n <= 0)) return CD360_ERR_ARG;
  if (!(level >= 0.0f) || !(level < INFINITY)) return CD360_ERR_ARG;
  if (!seed || !step_used || !aligned(seed, 8) || !aligned(step_used, 4) || !aligned(streams, 4)) return CD360_ERR_ARG;
  const uintptr_t oa = out_dtype ? 2 : 4;
  if (!aligned(x0, 4) || !aligned(xr, 4) || !aligned(drop_im, 4) || !aligned(rows, 4) || !aligned(x_t, 4) || !aligned(x_in, oa) ||
      (xr && !aligned(xr_in, oa)))
    return CD360_ERR_ARG;
  if (HW > ((int64_t)1 << 32) || (xr && (int64_t)n * HW > ((int64_t)1 << 32))) return CD360_ERR_SHAPE;
  const long img = (long)B * 4 * HW, ob = (long)oa;
  if (overlap(x_t, img * 4, x0, img * 4) || overlap(x_in, img * ob, x0, img * 4) || overlap(x_in, img * ob, x_t, img * 4)) return CD360_ERR_ARG;
  if (xr) {
    const long refs = img * n;
    if (overlap(xr_in, refs * ob, xr, refs * 4) || overlap(xr_in, refs * ob, x0, img * 4) || overlap(xr_in, refs * ob, x_t, img * 4) ||
        overlap(xr_in, refs * ob, x_in, img * ob) || overlap(x_t, img * 4, xr, refs * 4) || overlap(x_in, img * ob, xr, refs * 4))
      return CD360_ERR_ARG;
  }
  const bool vec = HW % 4 == 0 && aligned(x0, 16) && aligned(xr, 16) && aligned(x_t, 16) && aligned(x_in, 4 * oa) && (!xr || aligned(xr_in, 4 * oa));
  const bool wide = vec && out_dtype && HW % 8 == 0 && aligned(x_in, 16) && (!xr || aligned(xr_in, 16));  // bf16 planes 16 bytes at a time
  const int px = wide ? 8 : 4;
  const long G = (long)((HW + px - 1) / px), total = (long)B * G * (1 + (xr ? n : 0));
#define CD360_TRAIN_NOISE(PX, VEC, BF)                                                                                                          \
  hipLaunchKernelGGL((train_noise_kernel<PX, VEC, BF>), dim3(stride_grid(total)), dim3(256), 0, (hipStream_t)stream, (const float*)x0,          \
                     (const float*)xr, (const float*)drop_im, (const float*)rows, (const uint32_t*)seed, (const int*)streams,                  \
                     (const uint32_t*)step_used, level, (float*)x_t, x_in, xr_in, B, n, (long)HW, G)
  if (wide) CD360_TRAIN_NOISE(8, true, true);
  else if (vec && out_dtype) CD360_TRAIN_NOISE(4, true, true);
  else if (vec) CD360_TRAIN_NOISE(4, true, false);
  else if (out_dtype) CD360_TRAIN_NOISE(4, false, true);
  else CD360_TRAIN_NOISE(4, false, false);
#undef CD360_TRAIN_NOISE
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

#define CD360_TRAIN_BY_MODE(LAUNCH)                        \
  do {                                                     \
    if (mode == EPS_CHANNELS_LAST) {                       \
      if (eps_dtype) LAUNCH(EPS_CHANNELS_LAST, true);      \
      else LAUNCH(EPS_CHANNELS_LAST, false);               \
    } else if (mode == EPS_PLANES) {                       \
      if (eps_dtype) LAUNCH(EPS_PLANES, true);             \
      else LAUNCH(EPS_PLANES, false);                      \
    } else {                                               \
      if (eps_dtype) LAUNCH(EPS_STRIDED, true);            \
      else LAUNCH(EPS_STRIDED, false);                     \
    }                                                      \
  } while (0)

extern "C" int cd360_train_l2_f32(const void* eps, int eps_dtype, const int64_t* eps_strides, const void* x_t, const void* x0, const void* rows,
                                  const void* mask, void* loss, void* den, int B, int H, int W, void* stream) {
  if (!loss || !den || !aligned(loss, 4) || !aligned(den, 4)) return CD360_ERR_ARG;
  const int bad = l2_args(eps, eps_dtype, eps_strides, x_t, x0, rows, mask, B, H, W);
  if (bad) return bad;
  const long HW = (long)H * W, G = (HW + 3) / 4;
  int mode = eps_mode(eps, eps_strides, eps_dtype ? 2 : 4, H, W);
  if (!aligned(x_t, 16) || !aligned(x0, 16) || !aligned(mask, 16)) mode = EPS_STRIDED;
  const Strides s = strides_of(eps_strides);
#define CD360_TRAIN_L2(MODE, BF)                                                                                                            \
  hipLaunchKernelGGL((train_l2_kernel<MODE, BF>), dim3(B), dim3(L2_THREADS), 0, (hipStream_t)stream, eps, s, (const float*)x_t, (const float*)x0, \
                     (const float*)rows, (const float*)mask, (float*)loss, (float*)den, HW, W, G)
  CD360_TRAIN_BY_MODE(CD360_TRAIN_L2);
#undef CD360_TRAIN_L2
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_train_l2_bwd_f32(const void* eps, int eps_dtype, const int64_t* eps_strides, const void* x_t, const void* x0, const void* rows,
                                      const void* mask, const void* den, const void* g, void* d_eps, const int64_t* d_strides, int B, int H,
                                      int W, void* stream) {
  if (!den || !g || !d_eps || !d_strides || !aligned(den, 4) || !aligned(g, 4) || !aligned(d_eps, eps_dtype == 1 ? 2 : 4)) return CD360_ERR_ARG;
  const int bad = l2_args(eps, eps_dtype, eps_strides, x_t, x0, rows, mask, B, H, W);
  if (bad) return bad;
  if (d_strides[0] < 0 || d_strides[1] < 0 || d_strides[2] < 0 || d_strides[3] < 0) return CD360_ERR_SHAPE;
  const long HW = (long)H * W, G = (HW + 3) / 4;
  const int elem = eps_dtype ? 2 : 4;
  int mode = eps_mode(eps, eps_strides, elem, H, W);
  if (mode != eps_mode(d_eps, d_strides, elem, H, W) || !aligned(x_t, 16) || !aligned(x0, 16) || !aligned(mask, 16)) mode = EPS_STRIDED;
  const Strides s = strides_of(eps_strides), ds = strides_of(d_strides);
#define CD360_TRAIN_L2_BWD(MODE, BF)                                                                                                          \
  hipLaunchKernelGGL((train_l2_bwd_kernel<MODE, BF>), dim3(stride_grid((long)B * G)), dim3(256), 0, (hipStream_t)stream, eps, s, (const float*)x_t, \
                     (const float*)x0, (const float*)rows, (const float*)mask, (const float*)den, (const float*)g, d_eps, ds, B, HW, W, G)
  CD360_TRAIN_BY_MODE(CD360_TRAIN_L2_BWD);
#undef CD360_TRAIN_L2_BWD
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
