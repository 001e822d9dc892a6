// libcd360_text.so (include/text/cd360_text.h): what the prompt encoders of the conditioner need beside the Linear layers.  Four kernels:
//   text_embed_kernel        one wave per token: bf16(fp32(tok[id]) + fp32(pos[n])), optionally the row's (sum, sum of squares)
//   text_causal_attn_kernel  one workgroup per (batch, head): K and V in LDS, four lanes per query row, online softmax over keys 0 .. i
//   text_act_kernel          QuickGELU / exact GELU, 8 values per thread and trip
//   text_eot_pool_kernel     one workgroup per prompt: argmax of the ids (lowest index on ties), then the row copy
// The embedding, the activation and the pooling are bound by memory, the attention by its launch latency (at most 128 tokens per head).
// One fp32 rounding per operation (the build passes -ffp-contract=off), one rounding to bf16 at every store.
#include "../csrc/cd360_common.h"

#define CD360_TEXT_MAX_TOKENS 128  // include/text/cd360_text.h

namespace {

constexpr int kWave = 64;
constexpr int kHeadDim = 64;
constexpr int kLanesPerRow = 4;                       // lanes that share a query row
constexpr int kChan = kHeadDim / kLanesPerRow;        // 16 channels of q, of the dot product and of the output per lane
constexpr int kRowsPerWave = kWave / kLanesPerRow;    // 16
static_assert(kChan == 16, "two 16-byte LDS reads per key and per value row");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) v = v + __shfl_xor(v, s, kWave);
  return v;
}

__device__ __forceinline__ void unpack8(const u32x4 q, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = bf16lo_to_f32(q[e]);
    f[2 * e + 1] = bf16hi_to_f32(q[e]);
  }
}

// ---------------------------------------------------------------------------------------------------------------- embedding
// blockDim = 256: wave w of block b owns row 4 b + w; lane l takes the 16-byte vectors l, l + 64, ... of the row
__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* __restrict__ ids, const uint16_t* __restrict__ tok,
                                                         const uint16_t* __restrict__ pos, uint16_t* __restrict__ out, long rows, int N, int V,
                                                         int D, long ld_out, float* __restrict__ stats) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // (whole waves leave: no barrier below)
  const int lane = threadIdx.x & 63;
  const int n = (int)(row % N);
  const int64_t id = ids[row];
  const bool valid = id >= 0 && id < (int64_t)V;
  const uint16_t* t = tok + (valid ? id : 0) * (long)D;
  const uint16_t* p = pos + (long)n * D;
  uint16_t* o = out + row * ld_out;
  float s = 0.f, ss = 0.f;
  for (int c = lane * 8; c < D; c += kWave * 8) {
    u32x4 r = {0u, 0u, 0u, 0u};
    if (valid) {
      float a[8], b[8];
      unpack8(*reinterpret_cast<const u32x4*>(t + c), a);
      unpack8(*reinterpret_cast<const u32x4*>(p + c), b);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = pack_bf16x2(a[2 * e] + b[2 * e], a[2 * e + 1] + b[2 * e + 1]);
      float f[8];
      unpack8(r, f);  // the statistics are those of the stored values
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s = s + f[e];
        ss = ss + f[e] * f[e];
      }
    }
    *reinterpret_cast<u32x4*>(o + c) = r;
  }
  if (stats) {
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (lane == 0) {
      f32x2 st = {s, ss};
      *reinterpret_cast<f32x2*>(stats + 2 * row) = st;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- causal attention
struct AttnParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  uint16_t* o;
  long qs[3], ks[3], vs[3], os[3];
  int H, N;
  float scale;
};

// blockDim = 4 N rounded up to whole waves (<= 512).  Thread t: query row i = t / 4, channels [16 (t % 4), 16 (t % 4) + 16).  A wave holds
// 16 consecutive rows and walks the keys 0 .. its last row; a lane skips the keys above its own row (never touched: their probability is 0).
// All 16 quads of a wave read the same K / V row of LDS at a time (four distinct 32-byte pieces: broadcast, no bank conflict).
__global__ __launch_bounds__(512) void text_causal_attn_kernel(const AttnParams p) {
  __shared__ __attribute__((aligned(16))) uint16_t sk[CD360_TEXT_MAX_TOKENS * kHeadDim];
  __shared__ __attribute__((aligned(16))) uint16_t sv[CD360_TEXT_MAX_TOKENS * kHeadDim];
  const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int N = p.N;
  const uint16_t* kb = p.k + b * p.ks[0] + h * p.ks[1];
  const uint16_t* vb = p.v + b * p.vs[0] + h * p.vs[1];
  // rows 0 .. N - 1 of K and V, eight 16-byte vectors each; rows >= N are neither read from memory nor from LDS
  for (int idx = threadIdx.x; idx < N * 8; idx += blockDim.x) {
    const int r = idx >> 3, c = (idx & 7) * 8;
    *reinterpret_cast<u32x4*>(sk + r * kHeadDim + c) = *reinterpret_cast<const u32x4*>(kb + r * p.ks[2] + c);
    *reinterpret_cast<u32x4*>(sv + r * kHeadDim + c) = *reinterpret_cast<const u32x4*>(vb + r * p.vs[2] + c);
  }
  __syncthreads();
  const int i = threadIdx.x >> 2, part = threadIdx.x & 3;
  const bool live = i < N;
  float q[kChan], acc[kChan];
#pragma unroll
  for (int e = 0; e < kChan; ++e) {
    q[e] = 0.f;
    acc[e] = 0.f;
  }
  if (live) {
    const uint16_t* qp = p.q + b * p.qs[0] + h * p.qs[1] + i * p.qs[2] + part * kChan;
    unpack8(*reinterpret_cast<const u32x4*>(qp), q);
    unpack8(*reinterpret_cast<const u32x4*>(qp + 8), q + 8);
  }
  const int wave_last = ((threadIdx.x >> 6) + 1) * kRowsPerWave - 1;  // the wave's last row
  const int jend = wave_last < N - 1 ? wave_last : N - 1;
  float m = -INFINITY, l = 0.f;
  for (int j = 0; j <= jend; ++j) {
    float kf[kChan];
    const uint16_t* kr = sk + j * kHeadDim + part * kChan;
    unpack8(*reinterpret_cast<const u32x4*>(kr), kf);
    unpack8(*reinterpret_cast<const u32x4*>(kr + 8), kf + 8);
    float d[kChan];
#pragma unroll
    for (int e = 0; e < kChan; ++e) d[e] = q[e] * kf[e];
    // a fixed tree over the lane's 16 products, then over the four lanes of the row: every lane of a quad ends with the same bits
    float s = (((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]))) + (((d[8] + d[9]) + (d[10] + d[11])) + ((d[12] + d[13]) + (d[14] + d[15])));
    s = s + __shfl_xor(s, 1, kWave);
    s = s + __shfl_xor(s, 2, kWave);
    if (live && j <= i) {
      s = s * p.scale;
      const float mn = s > m ? s : m;
      const float alpha = expf(m - mn);  // first key: exp(-inf) = 0 on an accumulator that is 0
      const float pj = expf(s - mn);
      float vf[kChan];
      const uint16_t* vr = sv + j * kHeadDim + part * kChan;
      unpack8(*reinterpret_cast<const u32x4*>(vr), vf);
      unpack8(*reinterpret_cast<const u32x4*>(vr + 8), vf + 8);
      l = l * alpha + pj;
#pragma unroll
      for (int e = 0; e < kChan; ++e) acc[e] = acc[e] * alpha + pj * vf[e];
      m = mn;
    }
  }
  if (live) {
    uint16_t* op = p.o + b * p.os[0] + h * p.os[1] + i * p.os[2] + part * kChan;
#pragma unroll
    for (int e = 0; e < kChan; e += 4) {
      u32x2 w = {pack_bf16x2(acc[e] / l, acc[e + 1] / l), pack_bf16x2(acc[e + 2] / l, acc[e + 3] / l)};
      *reinterpret_cast<u32x2*>(op + e) = w;  // (o strides are multiples of 4: 8-byte stores)
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- activation
__device__ __forceinline__ float quick_gelu(float x) { return x * (1.f / (1.f + expf(-1.702f * x))); }
__device__ __forceinline__ float gelu_erf(float x) { return (0.5f * x) * (1.f + erff(x * 0.70710678118654752440f)); }

template <int KIND>
__global__ __launch_bounds__(256) void text_act_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, long rows, int vecs_per_row,
                                                       long ld_in, long ld_out) {
  const long total = rows * vecs_per_row;
  for (long vid = (long)blockIdx.x * blockDim.x + threadIdx.x; vid < total; vid += (long)gridDim.x * blockDim.x) {
    const long r = vid / vecs_per_row;
    const int c = (int)(vid - r * vecs_per_row) * 8;
    float f[8];
    unpack8(*reinterpret_cast<const u32x4*>(in + r * ld_in + c), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = KIND == 0 ? quick_gelu(f[e]) : gelu_erf(f[e]);
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pack_bf16x2(f[2 * e], f[2 * e + 1]);
    *reinterpret_cast<u32x4*>(out + r * ld_out + c) = w;
  }
}

// ---------------------------------------------------------------------------------------------------------------- EOT pooling
// blockDim = 256, block b = prompt b.  Every wave finds the argmax on its own (N is a few dozen ids): lane l scans ids l, l + 64, ... in
// rising order and keeps the first maximum, the butterfly keeps the larger id and, among equal ids, the lower index.
__global__ __launch_bounds__(256) void text_eot_pool_kernel(const uint16_t* __restrict__ x, const int64_t* __restrict__ ids, uint16_t* __restrict__ out,
                                                            int N, int D, long ld_x, long ld_out) {
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
  const uint16_t* src = x + ((long)b * N + at) * ld_x;
  uint16_t* dst = out + (long)b * ld_out;
  for (int c = threadIdx.x * 8; c < D; c += blockDim.x * 8) *reinterpret_cast<u32x4*>(dst + c) = *reinterpret_cast<const u32x4*>(src + c);
}

inline bool misaligned(const void* p, unsigned a) { return ((uintptr_t)p % a) != 0; }

}  // namespace

extern "C" int cd360_text_embed_bf16(const void* ids, const void* tok, const void* pos, void* out, int B, int N, int V, int D, int64_t ld_out,
                                     void* stats, void* stream) {
  if (!ids || !tok || !pos || !out || B <= 0 || N <= 0 || V <= 0 || D <= 0) return CD360_ERR_ARG;
  if (misaligned(tok, 16) || misaligned(pos, 16) || misaligned(out, 16) || misaligned(ids, 8) || misaligned(stats, 8)) return CD360_ERR_ARG;
  if (D % 8 || ld_out % 8 || ld_out < D) return CD360_ERR_SHAPE;
  const long rows = (long)B * N;
  if (rows > 0x7fffffffL) return CD360_ERR_SHAPE;
  hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const int64_t*)ids,
                     (const uint16_t*)tok, (const uint16_t*)pos, (uint16_t*)out, rows, N, V, D, (long)ld_out, (float*)stats);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_text_causal_attn_bf16(const void* q, const void* k, const void* v, void* o, int B, int H, int N, const int64_t* q_strides,
                                           const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides, float scale,
                                           void* stream) {
  if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides || !o_strides || B <= 0 || H <= 0) return CD360_ERR_ARG;
  if (misaligned(q, 16) || misaligned(k, 16) || misaligned(v, 16) || misaligned(o, 8)) return CD360_ERR_ARG;
  if (!(scale == scale) || scale - scale != 0.f) return CD360_ERR_ARG;  // NaN or infinite
  if (N < 1 || N > CD360_TEXT_MAX_TOKENS) return CD360_ERR_SHAPE;
  if ((long)B * H > 0x7fffffffL) return CD360_ERR_SHAPE;
  AttnParams p;
  for (int d = 0; d < 3; ++d) {
    if (q_strides[d] < 0 || k_strides[d] < 0 || v_strides[d] < 0 || o_strides[d] < 0) return CD360_ERR_SHAPE;
    if (q_strides[d] % 8 || k_strides[d] % 8 || v_strides[d] % 8 || o_strides[d] % 4) return CD360_ERR_SHAPE;
    p.qs[d] = q_strides[d]; p.ks[d] = k_strides[d]; p.vs[d] = v_strides[d]; p.os[d] = o_strides[d];
  }
  p.q = (const uint16_t*)q; p.k = (const uint16_t*)k; p.v = (const uint16_t*)v; p.o = (uint16_t*)o;
  p.H = H; p.N = N; p.scale = scale;
  const int threads = (N * kLanesPerRow + kWave - 1) / kWave * kWave;
  hipLaunchKernelGGL(text_causal_attn_kernel, dim3((unsigned)(B * H)), dim3(threads), 0, (hipStream_t)stream, p);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_text_act_bf16(const void* in, void* out, int64_t rows, int n, int64_t ld_in, int64_t ld_out, int kind, void* stream) {
  if (!in || !out || rows <= 0 || n <= 0 || (kind != 0 && kind != 1)) return CD360_ERR_ARG;
  if (misaligned(in, 16) || misaligned(out, 16)) return CD360_ERR_ARG;
  if (n % 8 || ld_in % 8 || ld_out % 8 || ld_in < n || ld_out < n) return CD360_ERR_SHAPE;
  const long vecs = rows * (n / 8);
  const long blocks = (vecs + 255) / 256;
  const dim3 grid((unsigned)(blocks > 256L * 8 ? 256L * 8 : blocks));
  if (kind == 0)
    hipLaunchKernelGGL(text_act_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)in, (uint16_t*)out, (long)rows, n / 8,
                       (long)ld_in, (long)ld_out);
  else
    hipLaunchKernelGGL(text_act_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)in, (uint16_t*)out, (long)rows, n / 8,
                       (long)ld_in, (long)ld_out);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_text_eot_pool_bf16(const void* x, const void* ids, void* out, int B, int N, int D, int64_t ld_x, int64_t ld_out, void* stream) {
  if (!x || !ids || !out || B <= 0 || N <= 0 || D <= 0) return CD360_ERR_ARG;
  if (misaligned(x, 16) || misaligned(out, 16) || misaligned(ids, 8)) return CD360_ERR_ARG;
  if (D % 8 || ld_x % 8 || ld_out % 8 || ld_x < D || ld_out < D) return CD360_ERR_SHAPE;
  if ((long)B * N > 0x7fffffffL) return CD360_ERR_SHAPE;
  hipLaunchKernelGGL(text_eot_pool_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (const int64_t*)ids,
                     (uint16_t*)out, N, D, (long)ld_x, (long)ld_out);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
