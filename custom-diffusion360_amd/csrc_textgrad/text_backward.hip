// libcd360_textgrad.so (include/textgrad/cd360_textgrad.h): the backward of the prompt encoders beside the Linear layers and LayerNorms.
// Four kernels:
//   textgrad_causal_attn_bwd_kernel  one workgroup per (batch, head): q, k, v, dO in LDS; a quad per query row for (max, sum, D) and dq,
//                                    then a quad per key row for dk and dv; P recomputed in fp32, no atomics
//   textgrad_act_bwd_kernel          dy * f'(x) for QuickGELU / exact GELU, 8 values per thread and trip
//   textgrad_eot_scatter_kernel      one workgroup per prompt: argmax of the ids (lowest index on ties), then the row add
//   textgrad_token_rows_kernel       one thread per eight columns of one modifier row: a walk over all ids in rising order
// The attention is bound by its launch latency (at most 128 tokens per head), the others by memory.  One fp32 rounding per operation (the
// build passes -ffp-contract=off), one rounding to bf16 at every store.
#include "../csrc/cd360_common.h"

#define CD360_TEXT_MAX_TOKENS 128         // include/text/cd360_text.h
#define CD360_TEXTGRAD_MAX_MODIFIERS 3    // include/textgrad/cd360_textgrad.h

namespace {

constexpr int kWave = 64;
constexpr int kHeadDim = 64;
constexpr int kLanesPerRow = 4;                     // lanes that share a row
constexpr int kChan = kHeadDim / kLanesPerRow;      // 16 channels per lane
constexpr int kRowsPerWave = kWave / kLanesPerRow;  // 16
static_assert(kChan == 16, "two 16-byte LDS reads per row and lane");

__device__ __forceinline__ void unpack8(const u32x4 q, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = bf16lo_to_f32(q[e]);
    f[2 * e + 1] = bf16hi_to_f32(q[e]);
  }
}

__device__ __forceinline__ void load16(const uint16_t* p, float* f) {
  unpack8(*reinterpret_cast<const u32x4*>(p), f);
  unpack8(*reinterpret_cast<const u32x4*>(p + 8), f + 8);
}

__device__ __forceinline__ void store16(uint16_t* p, const float* f) {
  u32x4 a, b;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = pack_bf16x2(f[2 * e], f[2 * e + 1]);
    b[e] = pack_bf16x2(f[8 + 2 * e], f[8 + 2 * e + 1]);
  }
  *reinterpret_cast<u32x4*>(p) = a;
  *reinterpret_cast<u32x4*>(p + 8) = b;
}

// a fixed tree over the lane's 16 products, then over the four lanes of the row: every lane of a quad ends with the same bits, and both
// phases of the attention backward build s and dP by exactly these operations (a * b == b * a)
__device__ __forceinline__ float quad_dot(const float* a, const float* b) {
  float d[kChan];
#pragma unroll
  for (int e = 0; e < kChan; ++e) d[e] = a[e] * b[e];
  float s = (((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]))) + (((d[8] + d[9]) + (d[10] + d[11])) + ((d[12] + d[13]) + (d[14] + d[15])));
  s = s + __shfl_xor(s, 1, kWave);
  s = s + __shfl_xor(s, 2, kWave);
  return s;
}

// ---------------------------------------------------------------------------------------------------------------- causal attention backward
struct AttnBwdParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const uint16_t* d_o;
  uint16_t* dq;
  uint16_t* dk;
  uint16_t* dv;
  long qs[3], ks[3], vs[3], dos[3], dqs[3], dks[3], dvs[3];
  int H, N;
  float scale;
};

// blockDim = 4 N rounded up to whole waves (<= 512).  Thread t: row t / 4, channels [16 (t % 4), 16 (t % 4) + 16).  A wave holds 16
// consecutive rows.  The shuffles of quad_dot run outside every divergent branch: all 64 lanes of a wave walk the same trip count.
__global__ __launch_bounds__(512) void textgrad_causal_attn_bwd_kernel(const AttnBwdParams p) {
  __shared__ __attribute__((aligned(16))) uint16_t sq[CD360_TEXT_MAX_TOKENS * kHeadDim];
  __shared__ __attribute__((aligned(16))) uint16_t sk[CD360_TEXT_MAX_TOKENS * kHeadDim];
  __shared__ __attribute__((aligned(16))) uint16_t sv[CD360_TEXT_MAX_TOKENS * kHeadDim];
  __shared__ __attribute__((aligned(16))) uint16_t sdo[CD360_TEXT_MAX_TOKENS * kHeadDim];
  __shared__ float smax[CD360_TEXT_MAX_TOKENS], sinv[CD360_TEXT_MAX_TOKENS], sdd[CD360_TEXT_MAX_TOKENS];
  const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int N = p.N;
  const uint16_t* qb = p.q + b * p.qs[0] + h * p.qs[1];
  const uint16_t* kb = p.k + b * p.ks[0] + h * p.ks[1];
  const uint16_t* vb = p.v + b * p.vs[0] + h * p.vs[1];
  const uint16_t* gb = p.d_o + b * p.dos[0] + h * p.dos[1];
  // rows 0 .. N - 1 of the four operands, eight 16-byte vectors each; rows >= N are neither read from memory nor from LDS
  for (int idx = threadIdx.x; idx < N * 8; idx += blockDim.x) {
    const int r = idx >> 3, c = (idx & 7) * 8;
    *reinterpret_cast<u32x4*>(sq + r * kHeadDim + c) = *reinterpret_cast<const u32x4*>(qb + r * p.qs[2] + c);
    *reinterpret_cast<u32x4*>(sk + r * kHeadDim + c) = *reinterpret_cast<const u32x4*>(kb + r * p.ks[2] + c);
    *reinterpret_cast<u32x4*>(sv + r * kHeadDim + c) = *reinterpret_cast<const u32x4*>(vb + r * p.vs[2] + c);
    *reinterpret_cast<u32x4*>(sdo + r * kHeadDim + c) = *reinterpret_cast<const u32x4*>(gb + r * p.dos[2] + c);
  }
  __syncthreads();
  const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
  const bool live = row < N;
  const int wave_first = (threadIdx.x >> 6) * kRowsPerWave;
  const int wave_last = wave_first + kRowsPerWave - 1;
  const int lrow = live ? row : 0;  // a lane behind the last row reads row 0 of LDS and discards what it computes

  // ---- phase 1: this quad's QUERY row i = row
  {
    float qf[kChan], gf[kChan], acc[kChan];
    load16(sq + lrow * kHeadDim + part * kChan, qf);
    load16(sdo + lrow * kHeadDim + part * kChan, gf);
    const int jend = wave_last < N - 1 ? wave_last : N - 1;
    float m = -INFINITY, l = 0.f, dd = 0.f;
    for (int j = 0; j <= jend; ++j) {
      float kf[kChan], vf[kChan];
      load16(sk + j * kHeadDim + part * kChan, kf);
      load16(sv + j * kHeadDim + part * kChan, vf);
      float s = quad_dot(qf, kf);
      const float dp = quad_dot(gf, vf);
      if (live && j <= row) {
        s = s * p.scale;
        const float mn = s > m ? s : m;
        const float alpha = expf(m - mn);  // first key: exp(-inf) = 0 on sums that are 0
        const float pj = expf(s - mn);
        l = l * alpha + pj;
        dd = dd * alpha + pj * dp;
        m = mn;
      }
    }
    const float inv = 1.f / l;  // (l >= 1 on a live row: the maximum's own term is 1)
    dd = dd * inv;
#pragma unroll
    for (int e = 0; e < kChan; ++e) acc[e] = 0.f;
    for (int j = 0; j <= jend; ++j) {
      float kf[kChan], vf[kChan];
      load16(sk + j * kHeadDim + part * kChan, kf);
      load16(sv + j * kHeadDim + part * kChan, vf);
      float s = quad_dot(qf, kf);
      const float dp = quad_dot(gf, vf);
      if (live && j <= row) {
        s = s * p.scale;
        const float pj = expf(s - m) * inv;
        const float ds = pj * (dp - dd);
#pragma unroll
        for (int e = 0; e < kChan; ++e) acc[e] = acc[e] + ds * kf[e];
      }
    }
    if (live) {
      if (part == 0) {
        smax[row] = m;
        sinv[row] = inv;
        sdd[row] = dd;
      }
#pragma unroll
      for (int e = 0; e < kChan; ++e) acc[e] = acc[e] * p.scale;
      store16(p.dq + b * p.dqs[0] + h * p.dqs[1] + row * p.dqs[2] + part * kChan, acc);
    }
  }
  __syncthreads();

  // ---- phase 2: this quad's KEY row j = row, the queries wave_first .. N - 1 in rising order (those before j are skipped)
  {
    float kf[kChan], vf[kChan], dk[kChan], dv[kChan];
    load16(sk + lrow * kHeadDim + part * kChan, kf);
    load16(sv + lrow * kHeadDim + part * kChan, vf);
#pragma unroll
    for (int e = 0; e < kChan; ++e) {
      dk[e] = 0.f;
      dv[e] = 0.f;
    }
    for (int i = wave_first; i < N; ++i) {
      float qf[kChan], gf[kChan];
      load16(sq + i * kHeadDim + part * kChan, qf);
      load16(sdo + i * kHeadDim + part * kChan, gf);
      float s = quad_dot(qf, kf);
      const float dp = quad_dot(gf, vf);
      if (live && i >= row) {
        s = s * p.scale;
        const float pj = expf(s - smax[i]) * sinv[i];
        const float ds = pj * (dp - sdd[i]);
#pragma unroll
        for (int e = 0; e < kChan; ++e) {
          dk[e] = dk[e] + ds * qf[e];
          dv[e] = dv[e] + pj * gf[e];
        }
      }
    }
    if (live) {
#pragma unroll
      for (int e = 0; e < kChan; ++e) dk[e] = dk[e] * p.scale;
      store16(p.dk + b * p.dks[0] + h * p.dks[1] + row * p.dks[2] + part * kChan, dk);
      store16(p.dv + b * p.dvs[0] + h * p.dvs[1] + row * p.dvs[2] + part * kChan, dv);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- activation backward
__device__ __forceinline__ float quick_gelu_grad(float x) {
  const float s = 1.f / (1.f + expf(-1.702f * x));  // x -> -inf: 1 / inf = 0; x -> +inf: 1
  return s * (1.f + (1.702f * x) * (1.f - s));
}
__device__ __forceinline__ float gelu_erf_grad(float x) {
  const float cdf = 0.5f * erfcf(-x * 0.70710678118654752440f);
  const float pdf = 0.39894228040143267794f * expf(-0.5f * (x * x));
  return cdf + x * pdf;
}

template <int KIND>
__global__ __launch_bounds__(256) void textgrad_act_bwd_kernel(const uint16_t* __restrict__ x, const uint16_t* dy, uint16_t* dx, long rows,
                                                               int vecs_per_row, long ld_x, long ld_dy, long ld_dx) {
  const long total = rows * vecs_per_row;
  for (long vid = (long)blockIdx.x * blockDim.x + threadIdx.x; vid < total; vid += (long)gridDim.x * blockDim.x) {
    const long r = vid / vecs_per_row;
    const int c = (int)(vid - r * vecs_per_row) * 8;
    float f[8], g[8];
    unpack8(*reinterpret_cast<const u32x4*>(x + r * ld_x + c), f);
    unpack8(*reinterpret_cast<const u32x4*>(dy + r * ld_dy + c), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = g[e] * (KIND == 0 ? quick_gelu_grad(f[e]) : gelu_erf_grad(f[e]));
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pack_bf16x2(f[2 * e], f[2 * e + 1]);
    *reinterpret_cast<u32x4*>(dx + r * ld_dx + c) = w;
  }
}

// ---------------------------------------------------------------------------------------------------------------- EOT scatter
// blockDim = 256, block b = prompt b.  The argmax is the forward's: every wave finds it on its own, lane l scans ids l, l + 64, ... in
// rising order and keeps the first maximum, the butterfly keeps the larger id and, among equal ids, the lower index.
__global__ __launch_bounds__(256) void textgrad_eot_scatter_kernel(const uint16_t* __restrict__ dp, const int64_t* __restrict__ ids, uint16_t* dx,
                                                                   int N, int D, long ld_dp, long ld_dx) {
  const int b = blockIdx.x, lane = threadIdx.x & 63;
  const int64_t* row = ids + (long)b * N;
  long long best = INT64_MIN;
  int at = 0x7fffffff;
  for (int n = lane; n < N; n += kWave) {
    const long long v = row[n];
    if (at == 0x7fffffff || v > best) {
      best = v;
      at = n;
    }
  }
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) {
    const long long ob = __shfl_xor(best, s, kWave);
    const int oa = __shfl_xor(at, s, kWave);
    // a lane without any id (N < 64) carries at = INT_MAX and loses to every lane that has one
    const bool take = oa != 0x7fffffff && (at == 0x7fffffff || ob > best || (ob == best && oa < at));
    if (take) {
      best = ob;
      at = oa;
    }
  }
  const uint16_t* src = dp + (long)b * ld_dp;
  uint16_t* dst = dx + ((long)b * N + at) * ld_dx;
  for (int c = threadIdx.x * 8; c < D; c += blockDim.x * 8) {
    float a[8], g[8];
    unpack8(*reinterpret_cast<const u32x4*>(dst + c), a);
    unpack8(*reinterpret_cast<const u32x4*>(src + c), g);
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pack_bf16x2(a[2 * e] + g[2 * e], a[2 * e + 1] + g[2 * e + 1]);
    *reinterpret_cast<u32x4*>(dst + c) = w;
  }
}

// ---------------------------------------------------------------------------------------------------------------- modifier rows
struct ModIds {
  long long id[CD360_TEXTGRAD_MAX_MODIFIERS];
};

// grid (ceil(D / 8 / 256), k), blockDim = 256: thread t of block (x, m) owns columns [8 (256 x + t), + 8) of modifier m.  The ids are the
// same for every lane (a uniform branch); the adds run in rising (b, n) order whatever the grid.
__global__ __launch_bounds__(256) void textgrad_token_rows_kernel(const uint16_t* __restrict__ dx, const int64_t* __restrict__ ids, const ModIds mods,
                                                                  float* __restrict__ out, long rows, int D, long ld_dx) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (c >= D) return;
  const int m = blockIdx.y;
  const long long want = m == 0 ? mods.id[0] : (m == 1 ? mods.id[1] : mods.id[2]);
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (long r = 0; r < rows; ++r) {
    if (ids[r] != want) continue;
    float f[8];
    unpack8(*reinterpret_cast<const u32x4*>(dx + r * ld_dx + c), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = acc[e] + f[e];
  }
  float* o = out + (long)m * D + c;
  f32x4 lo = {acc[0], acc[1], acc[2], acc[3]}, hi = {acc[4], acc[5], acc[6], acc[7]};
  *reinterpret_cast<f32x4*>(o) = lo;
  *reinterpret_cast<f32x4*>(o + 4) = hi;
}

inline bool misaligned(const void* p, unsigned a) { return ((uintptr_t)p % a) != 0; }

}  // namespace

extern "C" int cd360_textgrad_causal_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* d_o, void* dq, void* dk, void* dv, int B,
                                                   int H, int N, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                                   const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides,
                                                   const int64_t* dv_strides, float scale, void* stream) {
  if (!q || !k || !v || !d_o || !dq || !dk || !dv || B <= 0 || H <= 0) return CD360_ERR_ARG;
  if (!q_strides || !k_strides || !v_strides || !do_strides || !dq_strides || !dk_strides || !dv_strides) return CD360_ERR_ARG;
  if (misaligned(q, 16) || misaligned(k, 16) || misaligned(v, 16) || misaligned(d_o, 16) || misaligned(dq, 16) || misaligned(dk, 16) ||
      misaligned(dv, 16))
    return CD360_ERR_ARG;
  if (!(scale == scale) || scale - scale != 0.f) return CD360_ERR_ARG;  // NaN or infinite
  if (N < 1 || N > CD360_TEXT_MAX_TOKENS) return CD360_ERR_SHAPE;
  if ((long)B * H > 0x7fffffffL) return CD360_ERR_SHAPE;
  AttnBwdParams p;
  const int64_t* in[7] = {q_strides, k_strides, v_strides, do_strides, dq_strides, dk_strides, dv_strides};
  long* out[7] = {p.qs, p.ks, p.vs, p.dos, p.dqs, p.dks, p.dvs};
  for (int a = 0; a < 7; ++a)
    for (int d = 0; d < 3; ++d) {
      if (in[a][d] < 0 || in[a][d] % 8) return CD360_ERR_SHAPE;
      out[a][d] = in[a][d];
    }
  p.q = (const uint16_t*)q; p.k = (const uint16_t*)k; p.v = (const uint16_t*)v; p.d_o = (const uint16_t*)d_o;
  p.dq = (uint16_t*)dq; p.dk = (uint16_t*)dk; p.dv = (uint16_t*)dv;
  p.H = H; p.N = N; p.scale = scale;
  const int threads = (N * kLanesPerRow + kWave - 1) / kWave * kWave;
  hipLaunchKernelGGL(textgrad_causal_attn_bwd_kernel, dim3((unsigned)(B * H)), dim3(threads), 0, (hipStream_t)stream, p);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_textgrad_act_bwd_bf16(const void* x, const void* dy, void* dx, int64_t rows, int n, int64_t ld_x, int64_t ld_dy, int64_t ld_dx,
                                           int kind, void* stream) {
  if (!x || !dy || !dx || rows <= 0 || n <= 0 || (kind != 0 && kind != 1)) return CD360_ERR_ARG;
  if (misaligned(x, 16) || misaligned(dy, 16) || misaligned(dx, 16)) return CD360_ERR_ARG;
  if (n % 8 || ld_x % 8 || ld_dy % 8 || ld_dx % 8 || ld_x < n || ld_dy < n || ld_dx < n) return CD360_ERR_SHAPE;
  const long vecs = rows * (n / 8);
  const long blocks = (vecs + 255) / 256;
  const dim3 grid((unsigned)(blocks > 256L * 8 ? 256L * 8 : blocks));
  if (kind == 0)
    hipLaunchKernelGGL(textgrad_act_bwd_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (const uint16_t*)dy, (uint16_t*)dx,
                       (long)rows, n / 8, (long)ld_x, (long)ld_dy, (long)ld_dx);
  else
    hipLaunchKernelGGL(textgrad_act_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (const uint16_t*)dy, (uint16_t*)dx,
                       (long)rows, n / 8, (long)ld_x, (long)ld_dy, (long)ld_dx);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_textgrad_eot_scatter_bf16(const void* d_pooled, const void* ids, void* dx, int B, int N, int D, int64_t ld_dp, int64_t ld_dx,
                                               void* stream) {
  if (!d_pooled || !ids || !dx || B <= 0 || N <= 0 || D <= 0) return CD360_ERR_ARG;
  if (misaligned(d_pooled, 16) || misaligned(dx, 16) || misaligned(ids, 8)) return CD360_ERR_ARG;
  if (D % 8 || ld_dp % 8 || ld_dx % 8 || ld_dp < D || ld_dx < D) return CD360_ERR_SHAPE;
  if ((long)B * N > 0x7fffffffL) return CD360_ERR_SHAPE;
  hipLaunchKernelGGL(textgrad_eot_scatter_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)d_pooled,
                     (const int64_t*)ids, (uint16_t*)dx, N, D, (long)ld_dp, (long)ld_dx);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_textgrad_token_rows_f32(const void* d_x0, const void* ids, const int64_t* mod_ids, void* out, int B, int N, int D, int k,
                                             int64_t ld_dx, void* stream) {
  if (!d_x0 || !ids || !mod_ids || !out || B <= 0 || N <= 0 || D <= 0) return CD360_ERR_ARG;
  if (misaligned(d_x0, 16) || misaligned(out, 16) || misaligned(ids, 8)) return CD360_ERR_ARG;
  if (k < 1 || k > CD360_TEXTGRAD_MAX_MODIFIERS) return CD360_ERR_SHAPE;
  if (D % 8 || ld_dx % 8 || ld_dx < D) return CD360_ERR_SHAPE;
  if ((long)B * N > 0x7fffffffL) return CD360_ERR_SHAPE;
  ModIds mods;
  for (int m = 0; m < CD360_TEXTGRAD_MAX_MODIFIERS; ++m) mods.id[m] = m < k ? (long long)mod_ids[m] : 0;
  hipLaunchKernelGGL(textgrad_token_rows_kernel, dim3((unsigned)((D / 8 + 255) / 256), (unsigned)k), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)d_x0, (const int64_t*)ids, mods, (float*)out, (long)B * N, D, (long)ld_dx);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
