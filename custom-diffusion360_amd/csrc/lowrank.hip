// Rank-r adapter branch of the pose blocks' attention projections (sgm/modules/attention.py:330-347,373-376,421-424: add_lora=True)
// and the dropout that the reference applies to every adapter output while training.
//
//   cd360_lowrank_add_bf16   out[M, N] = base[M, N] + s * keep(key, i, j) * (T[M, r] @ U[N, r]^T),  r in {8, 16, 32, 64}
//   cd360_dropout_apply_bf16 g[M, N]   = s * keep(key, i, j) * dy[M, N]                           (the mask's backward)
//   cd360_dropout_tick       advances the mask offset kept in device memory                      (one thread, graph-capturable)
//
// The kernel is memory-bound: one 16-byte-vector read of base and one write of out per element, nothing else from HBM (T and U are
// M x r and N x r, r <= 64, and stay in L2).  A wave owns 32 rows of the output; the 32 x 32 product tiles come from
// v_mfma_f32_32x32x16_bf16 with U as the A operand (its row order permuted, see u_row) and T as the B operand, both read straight from
// global memory into the operand registers: with that permutation lane (r, h) of the accumulator holds output row r and the 16 CONTIGUOUS
// columns 16 h .. 16 h + 15 of the tile, so base and out move as two 16-byte vectors per lane and per tile, without an LDS round trip.
// The product accumulates in fp32 and is rounded to bf16 once, after the add of base.
//
// Mask: keep(key, i, j) is a pure function of the (seed, offset) pair in device memory, the host-side site id and the element (i, j), so
// the forward and the backward of a step regenerate the same mask and nothing is stored.  key mixes (seed, offset, site) through the
// murmur3 finaliser; per row, rk = fmix(key ^ fmix(i)); per element, fmix(rk + j * golden) compared against p * 2^32.  fmix is a
// bijection of 32-bit words and j * golden (odd) is one of j mod 2^32, so the elements of a row draw distinct words.
#include "cd360_common.h"

namespace {

constexpr int kWaves = 4;       // waves per workgroup, one 32-row strip each
constexpr int kChunkTiles = 4;  // 32-column tiles per workgroup (128 columns)

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ uint32_t mask_key(const int64_t* state, int64_t site) {
  const uint64_t seed = (uint64_t)state[0], off = (uint64_t)state[1], s = (uint64_t)site;
  uint32_t k = fmix32((uint32_t)seed ^ 0x9e3779b9u);
  k = fmix32(k ^ (uint32_t)(seed >> 32));
  k = fmix32(k + (uint32_t)off);
  k = fmix32(k ^ (uint32_t)(off >> 32));
  k = fmix32(k + (uint32_t)s);
  return fmix32(k ^ (uint32_t)(s >> 32));
}

__device__ __forceinline__ uint32_t row_key(uint32_t key, long i) {
  return fmix32(key ^ fmix32((uint32_t)i + 0x632be5abu) ^ (uint32_t)((uint64_t)i >> 32));
}

__device__ __forceinline__ bool keep(uint32_t rk, long j, uint32_t thresh) { return fmix32(rk + (uint32_t)j * 0x9e3779b1u) >= thresh; }

// MFMA A-operand row i -> tile column: accumulator register g of lane (c, h) is row (g & 3) + 8 (g >> 2) + 4 h of the 32 x 32 result;
// mapping that row to column 16 h + g gives every lane 16 contiguous columns.
__device__ __forceinline__ int u_row(int i) { return 16 * ((i >> 2) & 1) + ((i & 3) | ((i >> 3) << 2)); }

__device__ __forceinline__ void load16(const uint16_t* p, bool ok, u32x4& v) {
  if (ok) v = *reinterpret_cast<const u32x4*>(p);
  else v = u32x4{0u, 0u, 0u, 0u};
}

template <int R, bool MASK, bool BASE>
__global__ __launch_bounds__(64 * kWaves) void lowrank_add_kernel(const uint16_t* __restrict__ base, long ldb, const uint16_t* __restrict__ T,
                                                                 long ldt, const uint16_t* __restrict__ U, long ldu, uint16_t* out, long ldo, long M,
                                                                 int N, float scale, const int64_t* __restrict__ state, int64_t site,
                                                                 uint32_t thresh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const long m = ((long)blockIdx.x * kWaves + wave) * 32 + c;  // this lane's output row
  const bool row_ok = m < M;
  // B operand: B[k = 8 h + e][col c] = T[m][16 s + 8 h + e], one 16-byte vector per 16-wide step of r (r = 8: half a step, the lanes
  // of k = 8 .. 15 hold zeros on both operands and read nothing)
  constexpr int STEPS = (R + 15) / 16;
  const bool k_ok = R % 16 == 0 || h == 0;
  bf16x8 tb[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    u32x4 v;
    load16(T + m * ldt + 16 * s + 8 * h, row_ok && k_ok, v);
    tb[s] = __builtin_bit_cast(bf16x8, v);
  }
  uint32_t rk = 0;
  if (MASK) rk = row_key(mask_key(state, site), m);
  const int nc0 = blockIdx.y * (32 * kChunkTiles);
  const int urow = u_row(c);
#pragma unroll
  for (int t = 0; t < kChunkTiles; ++t) {
    const int n0 = nc0 + 32 * t;
    if (n0 >= N) break;
    const int nl = n0 + 16 * h;  // first of this lane's 16 output columns
    const bool out_ok = row_ok && nl < N;  // N % 16 == 0: a lane's 16 columns are all in range or all out
    u32x4 b0 = u32x4{0u, 0u, 0u, 0u}, b1 = b0;
    if (BASE) {
      load16(base + m * ldb + nl, out_ok, b0);
      load16(base + m * ldb + nl + 8, out_ok, b1);
    }
    const bool u_ok = n0 + urow < N && k_ok;
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      u32x4 v;
      load16(U + (long)(n0 + urow) * ldu + 16 * s + 8 * h, u_ok, v);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, v), tb[s], acc, 0, 0, 0);
    }
    if (!out_ok) continue;
    float y[16];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      y[2 * e] = bf16lo_to_f32(b0[e]);
      y[2 * e + 1] = bf16hi_to_f32(b0[e]);
      y[8 + 2 * e] = bf16lo_to_f32(b1[e]);
      y[8 + 2 * e + 1] = bf16hi_to_f32(b1[e]);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const float f = (MASK && !keep(rk, nl + g, thresh)) ? 0.f : scale;
      y[g] = fmaf(f, acc[g], y[g]);
    }
    u32x4 o0, o1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o0[e] = pack_bf16x2(y[2 * e], y[2 * e + 1]);
      o1[e] = pack_bf16x2(y[8 + 2 * e], y[8 + 2 * e + 1]);
    }
    *reinterpret_cast<u32x4*>(out + m * ldo + nl) = o0;
    *reinterpret_cast<u32x4*>(out + m * ldo + nl + 8) = o1;
  }
}

// g = s * keep * dy, 8 elements (one 16-byte vector) per thread and iteration
__global__ __launch_bounds__(256) void dropout_apply_kernel(const uint16_t* __restrict__ dy, long ldd, uint16_t* out, long ldo, long M, int N,
                                                            float scale, const int64_t* __restrict__ state, int64_t site, uint32_t thresh) {
  const uint32_t key = mask_key(state, site);
  const int vpr = N / 8;
  const long total = M * vpr;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (long)gridDim.x * blockDim.x) {
    const long i = v / vpr;
    const int j = (int)(v - i * vpr) * 8;
    const u32x4 d = *reinterpret_cast<const u32x4*>(dy + i * ldd + j);
    const uint32_t rk = row_key(key, i);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float f0 = keep(rk, j + 2 * e, thresh) ? scale : 0.f, f1 = keep(rk, j + 2 * e + 1, thresh) ? scale : 0.f;
      o[e] = pack_bf16x2(f0 * bf16lo_to_f32(d[e]), f1 * bf16hi_to_f32(d[e]));
    }
    *reinterpret_cast<u32x4*>(out + i * ldo + j) = o;
  }
}

__global__ void dropout_tick_kernel(int64_t* state) { state[1] += 1; }

bool bad_ptr(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// p -> (threshold of the 32-bit draw, scale); false for p outside [0, 1)
bool mask_params(float p, uint32_t& thresh, float& scale) {
  if (!(p >= 0.f && p < 1.f)) return false;
  const double t = (double)p * 4294967296.0;
  thresh = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
  scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  return true;
}

template <int R>
int launch_lowrank(const void* base, int64_t ldb, const void* t, int64_t ldt, const void* u, int64_t ldu, void* out, int64_t ldo, int64_t M, int N,
                   float scale, const void* state, int64_t site, uint32_t thresh, hipStream_t st) {
  const dim3 grid((unsigned)((M + 32 * kWaves - 1) / (32 * kWaves)), (unsigned)((N + 32 * kChunkTiles - 1) / (32 * kChunkTiles)));
  const auto* b = (const uint16_t*)base;
  const auto* T = (const uint16_t*)t;
  const auto* U = (const uint16_t*)u;
  auto* o = (uint16_t*)out;
  const auto* s = (const int64_t*)state;
  const bool mask = thresh != 0;
  if (mask && base) hipLaunchKernelGGL((lowrank_add_kernel<R, true, true>), grid, dim3(64 * kWaves), 0, st, b, ldb, T, ldt, U, ldu, o, ldo, M, N, scale, s, site, thresh);
  else if (mask) hipLaunchKernelGGL((lowrank_add_kernel<R, true, false>), grid, dim3(64 * kWaves), 0, st, b, ldb, T, ldt, U, ldu, o, ldo, M, N, scale, s, site, thresh);
  else if (base) hipLaunchKernelGGL((lowrank_add_kernel<R, false, true>), grid, dim3(64 * kWaves), 0, st, b, ldb, T, ldt, U, ldu, o, ldo, M, N, scale, s, site, thresh);
  else hipLaunchKernelGGL((lowrank_add_kernel<R, false, false>), grid, dim3(64 * kWaves), 0, st, b, ldb, T, ldt, U, ldu, o, ldo, M, N, scale, s, site, thresh);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

}  // namespace

extern "C" int cd360_lowrank_add_bf16(const void* base, int64_t ldb, const void* t, int64_t ldt, const void* u, int64_t ldu, void* out, int64_t ldo,
                                      int64_t M, int N, int r, float p, const void* rng_state, int64_t site, void* stream) {
  if (!t || !u || !out || M <= 0 || N <= 0) return CD360_ERR_ARG;
  if (bad_ptr(t) || bad_ptr(u) || bad_ptr(out) || (base && bad_ptr(base))) return CD360_ERR_ARG;
  uint32_t thresh;
  float scale;
  if (!mask_params(p, thresh, scale)) return CD360_ERR_ARG;
  if (thresh && (!rng_state || (reinterpret_cast<uintptr_t>(rng_state) & 7))) return CD360_ERR_ARG;
  if (N % 16 || ldt % 8 || ldu % 8 || ldo % 8 || ldt < r || ldu < r || ldo < N || (base && (ldb % 8 || ldb < N))) return CD360_ERR_SHAPE;
  if ((M + 32 * kWaves - 1) / (32 * kWaves) > 0x7fffffff) return CD360_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  switch (r) {
    case 8: return launch_lowrank<8>(base, ldb, t, ldt, u, ldu, out, ldo, M, N, scale, rng_state, site, thresh, st);
    case 16: return launch_lowrank<16>(base, ldb, t, ldt, u, ldu, out, ldo, M, N, scale, rng_state, site, thresh, st);
    case 32: return launch_lowrank<32>(base, ldb, t, ldt, u, ldu, out, ldo, M, N, scale, rng_state, site, thresh, st);
    case 64: return launch_lowrank<64>(base, ldb, t, ldt, u, ldu, out, ldo, M, N, scale, rng_state, site, thresh, st);
    default: return CD360_ERR_SHAPE;
  }
}

extern "C" int cd360_dropout_apply_bf16(const void* dy, int64_t ldd, void* out, int64_t ldo, int64_t M, int N, float p, const void* rng_state,
                                        int64_t site, void* stream) {
  if (!dy || !out || !rng_state || M <= 0 || N <= 0) return CD360_ERR_ARG;
  if (bad_ptr(dy) || bad_ptr(out) || (reinterpret_cast<uintptr_t>(rng_state) & 7)) return CD360_ERR_ARG;
  uint32_t thresh;
  float scale;
  if (!mask_params(p, thresh, scale)) return CD360_ERR_ARG;
  if (N % 8 || ldd % 8 || ldo % 8 || ldd < N || ldo < N) return CD360_ERR_SHAPE;
  const long vecs = M * (N / 8);
  const long blocks = (vecs + 255) / 256;
  hipLaunchKernelGGL(dropout_apply_kernel, dim3((unsigned)(blocks > 256L * 32 ? 256L * 32 : blocks)), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)dy, (long)ldd, (uint16_t*)out, (long)ldo, (long)M, N, scale, (const int64_t*)rng_state, site, thresh);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_dropout_tick(void* rng_state, void* stream) {
  if (!rng_state || (reinterpret_cast<uintptr_t>(rng_state) & 7)) return CD360_ERR_ARG;
  hipLaunchKernelGGL(dropout_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (int64_t*)rng_state);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
