// The first-stage decoder's own kernels (AutoencoderKL.decode -> Decoder.forward, sgm/modules/diffusionmodules/model.py:604-733).  Everything
// else the decoder runs (GroupNorm + SiLU, 3 x 3 / 1 x 1 convolutions, Upsample) is the UNet's kernels.
//
//   cd360_attn_single_bf16   the single-head mid-block attention (MemoryEfficientAttnBlock / AttnBlock, model.py:161-265): flash attention
//                            at head dim D = C (64 .. 512), every latent pixel a query and a key.  A workgroup = four waves of 16 queries;
//                            32-key K / V tiles through the LDS (V stored transposed so the P V operand is one 8-byte read per 4 keys);
//                            scores S^T = K Q^T on v_mfma_f32_16x16x32_bf16 so that every lane owns ONE query column and its running
//                            maximum / sum (fp32, base 2); O (fp32, 16 x D per wave) stays in registers.  Few query blocks at one head:
//                            the keys are split over up to 16 workgroups per query block, each writing its normalised partial O and
//                            log2-sum-exp, then attn_single_combine_kernel merges them.
//   cd360_vae_conv_in_f32    Decoder.conv_in (model.py:651-654, :721): fp32 NCHW latent (Cz <= 8) -> bf16 channels-last, + GroupNorm slab sums.
//   cd360_vae_conv_out_bf16  Decoder.conv_out (model.py:699-701, :733): bf16 channels-last (after norm_out + SiLU) -> fp32 NCHW, Cout <= 4.
//   cd360_vae_enc_conv_out_bf16  Encoder.conv_out (model.py:568-574, :600): the same at latent resolution, Cout <= 8, the 9 Cin reduction
//                            split over the threads of a workgroup (16 pixels per workgroup: a 64^2 latent is 256 workgroups).
// (The Encoder's Downsample is the register-staged convolution kernel with its tap centre moved: conv_igemm.hip.)
#include "cd360_common.h"
#include "vae_conv_out.h"

namespace {

constexpr int AS_KT = 32;   // keys per tile
constexpr int AS_QB = 64;   // queries per workgroup (4 waves x 16)
constexpr int AS_MAX_SPLIT = 16;

// q, k, v [B][N][D] at b * bs + n * rs + d; o likewise (bf16).  Keys [split * split_keys, min(N, (split + 1) * split_keys)).
// nsplit == 1: o = softmax_2(qscale * q k^T) v.  nsplit > 1: part [nsplit][B][N][D] fp32 (normalised) and lse2 [nsplit][B][N] fp32.
template <int D>
__global__ __launch_bounds__(256) void attn_single_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                          const uint16_t* __restrict__ v, uint16_t* __restrict__ o, float* __restrict__ part,
                                                          float* __restrict__ lse2, int B, int N, long q_bs, long q_rs, long k_bs, long k_rs,
                                                          long v_bs, long v_rs, long o_bs, long o_rs, float qscale, int split_keys) {
  constexpr int KS = D + 8;        // K row pitch in the LDS (elements): rows 16 bytes apart in bank space
  constexpr int VS = AS_KT + 8;    // transposed-V row pitch (elements)
  constexpr int NQ = D / 32;       // 32-wide K steps of the score MFMA
  constexpr int NT = D / 16;       // 16-column output tiles
  __shared__ __attribute__((aligned(16))) uint16_t Ks[AS_KT * KS];
  __shared__ __attribute__((aligned(16))) uint16_t Vt[D * VS];

  const int b = blockIdx.z, split = blockIdx.y, q0 = blockIdx.x * AS_QB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, grp = lane >> 4;
  const int kbeg = split * split_keys, kend = min(N, kbeg + split_keys);

  // Q fragments (B operand of S^T = K Q^T): lane holds q[query col][32 s + 8 grp .. + 7]
  const int qrow = q0 + wave * 16 + col;
  bf16x8 qf[NQ];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    u32x4 t = {0u, 0u, 0u, 0u};
    if (qrow < N) t = *reinterpret_cast<const u32x4*>(q + b * q_bs + (long)qrow * q_rs + s * 32 + grp * 8);
    qf[s] = __builtin_bit_cast(bf16x8, t);
  }
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -__builtin_inff(), l = 0.f;  // of query col; l is this lane's share (reduced at the end)

  for (int kt = kbeg; kt < kend; kt += AS_KT) {
    __syncthreads();
    for (int c = tid; c < AS_KT * (D / 8); c += 256) {
      const int r = c / (D / 8), cc = c - r * (D / 8), key = kt + r;
      u32x4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
      if (key < kend) {
        kv = *reinterpret_cast<const u32x4*>(k + b * k_bs + (long)key * k_rs + cc * 8);
        vv = *reinterpret_cast<const u32x4*>(v + b * v_bs + (long)key * v_rs + cc * 8);
      }
      *reinterpret_cast<u32x4*>(Ks + r * KS + cc * 8) = kv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Vt[(cc * 8 + 2 * e) * VS + r] = (uint16_t)(vv[e] & 0xffffu);
        Vt[(cc * 8 + 2 * e + 1) * VS + r] = (uint16_t)(vv[e] >> 16);
      }
    }
    __syncthreads();

    // S^T for keys kt + 16 h + 4 grp + r (h = 0, 1), query col
    f32x4 s[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      s[h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Ks + (16 * h + col) * KS + j * 32 + grp * 8));
        s[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[j], s[h], 0, 0, 0);
      }
    }
    float mx = -__builtin_inff();
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = (kt + 16 * h + 4 * grp + r < kend) ? s[h][r] * qscale : -__builtin_inff();
        s[h][r] = x;
        mx = fmaxf(mx, x);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mnew = fmaxf(m, mx);  // finite: key kt < kend is valid
    const float alpha = __builtin_amdgcn_exp2f(m - mnew);
    m = mnew;
    float psum = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[h][r] = __builtin_amdgcn_exp2f(s[h][r] - mnew);
        psum += s[h][r];
      }
    l = l * alpha + psum;
    // P as the A operand of O += P V: k slot 8 grp + e <-> key 16 (e / 4) + 4 grp + e % 4 (the same permutation indexes V's rows)
    const bf16x8 pa = __builtin_bit_cast(bf16x8, u32x4{pack_bf16x2(s[0][0], s[0][1]), pack_bf16x2(s[0][2], s[0][3]),
                                                        pack_bf16x2(s[1][0], s[1][1]), pack_bf16x2(s[1][2], s[1][3])});
    // O rows are queries 4 grp + r: their alpha lives in lane 4 grp + r
    float ar[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, 4 * grp + r);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint16_t* vp = Vt + (t * 16 + col) * VS + 4 * grp;
      const u32x2 lo = *reinterpret_cast<const u32x2*>(vp), hi = *reinterpret_cast<const u32x2*>(vp + 16);
      const bf16x8 vb = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] *= ar[r];
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, acc[t], 0, 0, 0);
    }
  }

  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  float linv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) linv[r] = 1.f / __shfl(l, 4 * grp + r);
  const int qbase = q0 + wave * 16 + 4 * grp;
  if (part == nullptr) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (qbase + r >= N) continue;
      uint16_t* op = o + b * o_bs + (long)(qbase + r) * o_rs + col;
#pragma unroll
      for (int t = 0; t < NT; ++t) op[t * 16] = f32_to_bf16(acc[t][r] * linv[r]);
    }
  } else {
    const long row0 = ((long)split * B + b) * N;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (qbase + r >= N) continue;
      float* pp = part + (row0 + qbase + r) * D + col;
#pragma unroll
      for (int t = 0; t < NT; ++t) pp[t * 16] = acc[t][r] * linv[r];
    }
    if (grp == 0 && qrow < N) lse2[row0 + qrow] = m + log2f(l);
  }
}

// o[b][n][4 c .. 4 c + 3] = sum_s w_s part_s / sum_s w_s with w_s = 2^(lse2_s - max lse2): one thread per 4 outputs
__global__ __launch_bounds__(256) void attn_single_combine_kernel(const float* __restrict__ part, const float* __restrict__ lse2,
                                                                  uint16_t* __restrict__ o, int B, int N, int D, int nsplit, long o_bs,
                                                                  long o_rs) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x, per_row = D / 4;
  const long rows = (long)B * N;
  if (idx >= rows * per_row) return;
  const long row = idx / per_row;
  const int c4 = (int)(idx - row * per_row);
  float mx = -__builtin_inff();
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, lse2[s * rows + row]);
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  float wsum = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float w = __builtin_amdgcn_exp2f(lse2[s * rows + row] - mx);
    const f32x4 p = *reinterpret_cast<const f32x4*>(part + (s * rows + row) * D + 4 * c4);
    sum += w * p;
    wsum += w;
  }
  const float inv = 1.f / wsum;
  const long b = row / N, n = row - b * N;
  *reinterpret_cast<u32x2*>(o + b * o_bs + n * o_rs + 4 * c4) = u32x2{pack_bf16x2(sum[0] * inv, sum[1] * inv), pack_bf16x2(sum[2] * inv, sum[3] * inv)};
}

constexpr int CI_SLAB = 64;  // pixels per workgroup of the input convolution (= pixels per GroupNorm statistics slab)

// z [B][Cz][h][w] fp32; w [Cz * 9][Cout] fp32 (row ci * 9 + 3 ky + kx); out [B][h w][Cout] bf16; stats [B][slabs][Cout][2] | null.
// Grid (slabs, B), Cout / 2 threads: thread = two output channels over the slab's pixels (the latent reads are wave-uniform).
__global__ __launch_bounds__(512) void vae_conv_in_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ bias,
                                                          uint16_t* __restrict__ out, float* __restrict__ stats, int Cz, int H, int W, int Cout) {
  const int b = blockIdx.y, c = 2 * threadIdx.x;
  const long HW = (long)H * W;
  const long p0 = (long)blockIdx.x * CI_SLAB, p1 = min(HW, p0 + CI_SLAB);
  const float b0 = bias ? bias[c] : 0.f, b1 = bias ? bias[c + 1] : 0.f;
  float s0 = 0.f, s1 = 0.f, ss0 = 0.f, ss1 = 0.f;
  for (long p = p0; p < p1; ++p) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    float a0 = b0, a1 = b1;
    for (int ci = 0; ci < Cz; ++ci) {
      const float* zp = z + ((long)b * Cz + ci) * HW;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int yy = y + ky - 1;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int xx = x + kx - 1;
          if (xx < 0 || xx >= W) continue;
          const float zv = zp[(long)yy * W + xx];
          const f32x2 wv = *reinterpret_cast<const f32x2*>(w + (long)(ci * 9 + ky * 3 + kx) * Cout + c);
          a0 = fmaf(zv, wv[0], a0);
          a1 = fmaf(zv, wv[1], a1);
        }
      }
    }
    const uint32_t pk = pack_bf16x2(a0, a1);
    *reinterpret_cast<uint32_t*>(out + ((long)b * HW + p) * Cout + c) = pk;
    const float r0 = bf16lo_to_f32(pk), r1 = bf16hi_to_f32(pk);
    s0 += r0; s1 += r1;
    ss0 = fmaf(r0, r0, ss0); ss1 = fmaf(r1, r1, ss1);
  }
  if (stats) {
    float* sp = stats + (((long)b * gridDim.x + blockIdx.x) * Cout + c) * 2;
    *reinterpret_cast<f32x4*>(sp) = f32x4{s0, ss0, s1, ss1};
  }
}

// x [B][H W][Cin] bf16; w [9][Cin][4] fp32 (tap 3 ky + kx, channel, output channel; columns >= Cout zero); out [B][Cout][H][W] fp32.
// Grid (ceil(H W / 256), B); thread = one output pixel, all Cout <= 4 channels.  The accumulation is vae_conv_out.h's, shared with the
// uint8 epilogue of image_stage.hip.
__global__ __launch_bounds__(256) void vae_conv_out_kernel(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ out, int H, int W, int Cin, int Cout) {
  __shared__ __attribute__((aligned(16))) float wl[9 * CO_CHUNK * 4];
  const int b = blockIdx.y;
  const long HW = (long)H * W, p = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < HW;
  const f32x4 acc = vae_conv_out_accumulate(x, w, wl, b, p, live, H, W, Cin);
  if (!live) return;
#pragma unroll
  for (int co = 0; co < 4; ++co)
    if (co < Cout) out[((long)b * Cout + co) * HW + p] = acc[co] + (bias ? bias[co] : 0.f);
}

constexpr int EO_PX = 16;      // output pixels per workgroup
constexpr int EO_SLICES = 16;  // K slices per pixel (256 threads = 16 pixels x 16 slices)
constexpr int EO_CHUNK = 128;  // input channels whose weights sit in the LDS at a time
constexpr int EO_GP = 8 * 8 + 4;  // LDS floats per 8-channel group of one tap: 8 channels x 8 outputs + 16 bytes of padding, so that the
                                  // slices of one ds_read_b128 lane group read different banks

// x [B][H W][Cin] bf16; w [9][Cin][8] fp32 (tap 3 ky + kx, channel, output channel; columns >= Cout zero); out [B][Cout][H][W] fp32.
// Grid (ceil(H W / 16), B), 256 threads: thread = (slice s = tid / 16, pixel tid % 16).  Per weight chunk, slice s takes the units
// u = s, s + 16, ... of (tap, 8-channel group) and accumulates all 8 outputs of its pixel in fp32; the 16 slices of a pixel are summed
// through the LDS in slice order.  Every sum has a fixed order that does not depend on B: deterministic and batch-invariant.
__global__ __launch_bounds__(256) void vae_enc_conv_out_kernel(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ out, int H, int W, int Cin,
                                                               int Cout) {
  __shared__ __attribute__((aligned(16))) float wl[9 * (EO_CHUNK / 8) * EO_GP];
  __shared__ __attribute__((aligned(16))) float red[EO_SLICES * EO_PX * 8];
  const int b = blockIdx.y, tid = threadIdx.x, s = tid / EO_PX, pp = tid % EO_PX;
  const long HW = (long)H * W, p = (long)blockIdx.x * EO_PX + pp;
  const bool live = p < HW;
  const int y = live ? (int)(p / W) : 0, xq = live ? (int)(p - (long)y * W) : 0;
  const uint16_t* xb = x + (long)b * HW * Cin;
  float acc[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o] = 0.f;
  for (int c0 = 0; c0 < Cin; c0 += EO_CHUNK) {
    const int cn = min(EO_CHUNK, Cin - c0), groups = cn / 8;  // Cin % 64 == 0: cn is 64 or 128
    __syncthreads();
    for (int i = tid; i < 9 * cn * 2; i += 256) {  // f32x4 units: tap, channel, half of the 8 outputs
      const int tap = i / (cn * 2), r = i - tap * cn * 2, ci = r >> 1;
      *reinterpret_cast<f32x4*>(wl + (tap * (EO_CHUNK / 8) + (ci >> 3)) * EO_GP + (ci & 7) * 8 + (r & 1) * 4) =
          *reinterpret_cast<const f32x4*>(w + ((long)tap * Cin + c0) * 8 + r * 4);
    }
    __syncthreads();
    if (!live) continue;
    for (int u = s; u < 9 * groups; u += EO_SLICES) {
      const int tap = u / groups, g = u - tap * groups;
      const int yy = y + tap / 3 - 1, xx = xq + tap % 3 - 1;
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const u32x4 v = *reinterpret_cast<const u32x4*>(xb + ((long)yy * W + xx) * Cin + c0 + g * 8);
      const float* wg = wl + (tap * (EO_CHUNK / 8) + g) * EO_GP;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xv = (e & 1) ? bf16hi_to_f32(v[e >> 1]) : bf16lo_to_f32(v[e >> 1]);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wg + e * 8), w1 = *reinterpret_cast<const f32x4*>(wg + e * 8 + 4);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          acc[o] = fmaf(xv, w0[o], acc[o]);
          acc[4 + o] = fmaf(xv, w1[o], acc[4 + o]);
        }
      }
    }
  }
  *reinterpret_cast<f32x4*>(red + (s * EO_PX + pp) * 8) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(red + (s * EO_PX + pp) * 8 + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  __syncthreads();
  if (tid >= EO_PX * 8) return;
  const int op = tid % EO_PX, co = tid / EO_PX;  // consecutive threads: consecutive pixels of one output channel (coalesced stores)
  const long po = (long)blockIdx.x * EO_PX + op;
  if (co >= Cout || po >= HW) return;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < EO_SLICES; ++k) sum += red[(k * EO_PX + op) * 8 + co];
  out[((long)b * Cout + co) * HW + po] = sum + (bias ? bias[co] : 0.f);
}

}  // namespace

extern "C" int cd360_attn_single_splits(int B, int N) {
  // chosen from N alone: an image takes the same splits (and rounds the same) in a batch of any size; B only multiplies the grid
  if (B <= 0 || N <= 0) return 0;
  const long qblocks = (long)(N + AS_QB - 1) / AS_QB;
  const int ntiles = (N + AS_KT - 1) / AS_KT;
  long s = (1024 + qblocks - 1) / qblocks;  // >= 4 workgroups per CU
  s = min(s, (long)AS_MAX_SPLIT);
  s = min(s, (long)(ntiles / 8));          // >= 8 key tiles per split: the combine stays small next to the split's work
  if (s < 2) return 1;
  const int per = (ntiles + (int)s - 1) / (int)s;  // tiles per split; every split gets >= 1 key
  return (ntiles + per - 1) / per;
}

extern "C" int64_t cd360_attn_single_workspace_bytes(int B, int N, int D) {
  const int s = cd360_attn_single_splits(B, N);
  return s <= 1 ? 0 : (int64_t)s * B * N * (D + 1) * 4;
}

extern "C" int cd360_attn_single_bf16(const void* q, const void* k, const void* v, void* o, int B, int N, int D, const int64_t* q_strides,
                                      const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides, float qscale, void* ws,
                                      void* stream) {
  if (!q || !k || !v || !o || !q_strides || !k_strides || !v_strides || !o_strides || B <= 0 || N <= 0) return CD360_ERR_ARG;
  if (D < 64 || D > 512 || D % 64) return CD360_ERR_SHAPE;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 || (uintptr_t)o % 8) return CD360_ERR_ARG;
  for (int i = 0; i < 2; ++i)
    if (q_strides[i] % 8 || k_strides[i] % 8 || v_strides[i] % 8 || o_strides[i] % 4) return CD360_ERR_SHAPE;
  if (B > 65535) return CD360_ERR_SHAPE;
  const int nsplit = cd360_attn_single_splits(B, N);
  if (nsplit > 1 && (!ws || (uintptr_t)ws % 16)) return CD360_ERR_ARG;
  const int ntiles = (N + AS_KT - 1) / AS_KT, per = (ntiles + nsplit - 1) / nsplit;
  float* part = nsplit > 1 ? (float*)ws : nullptr;
  float* lse2 = nsplit > 1 ? part + (long)nsplit * B * N * D : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((N + AS_QB - 1) / AS_QB, nsplit, B);
#define AS_LAUNCH(DD)                                                                                                                  \
  case DD:                                                                                                                             \
    attn_single_kernel<DD><<<grid, 256, 0, st>>>((const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, (uint16_t*)o, part, lse2, B, \
                                                 N, q_strides[0], q_strides[1], k_strides[0], k_strides[1], v_strides[0], v_strides[1],  \
                                                 o_strides[0], o_strides[1], qscale, per * AS_KT);                                     \
    break;
  switch (D) {
    AS_LAUNCH(64) AS_LAUNCH(128) AS_LAUNCH(192) AS_LAUNCH(256) AS_LAUNCH(320) AS_LAUNCH(384) AS_LAUNCH(448) AS_LAUNCH(512)
  }
#undef AS_LAUNCH
  CD360_LAUNCH_CHECK();
  if (nsplit > 1) {
    const long n4 = (long)B * N * (D / 4);
    attn_single_combine_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(part, lse2, (uint16_t*)o, B, N, D, nsplit, o_strides[0], o_strides[1]);
    CD360_LAUNCH_CHECK();
  }
  return CD360_OK;
}

extern "C" int cd360_vae_conv_in_stats_slabs(int H, int W) { return (int)(((long)H * W + CI_SLAB - 1) / CI_SLAB); }

extern "C" int cd360_vae_conv_in_f32(const void* z, const void* w, const void* bias, void* out, void* tile_stats, int B, int Cz, int H, int W,
                                     int Cout, void* stream) {
  if (!z || !w || !out || B <= 0 || H <= 0 || W <= 0) return CD360_ERR_ARG;
  if (Cz < 1 || Cz > 8 || Cout % 64 || Cout < 64 || Cout > 1024 || B > 65535) return CD360_ERR_SHAPE;
  if (tile_stats && ((long)H * W) % CI_SLAB) return CD360_ERR_SHAPE;  // a slab must not straddle images
  if (((uintptr_t)w | (uintptr_t)out) % 8 || (uintptr_t)tile_stats % 16) return CD360_ERR_ARG;
  const dim3 grid(cd360_vae_conv_in_stats_slabs(H, W), B);
  vae_conv_in_kernel<<<grid, Cout / 2, 0, (hipStream_t)stream>>>((const float*)z, (const float*)w, (const float*)bias, (uint16_t*)out,
                                                                 (float*)tile_stats, Cz, H, W, Cout);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_vae_conv_out_bf16(const void* x, const void* w, const void* bias, void* out, int B, int H, int W, int Cin, int Cout,
                                       void* stream) {
  if (!x || !w || !out || B <= 0 || H <= 0 || W <= 0) return CD360_ERR_ARG;
  if (Cin % 64 || Cin <= 0 || Cout < 1 || Cout > 4 || B > 65535) return CD360_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)w) % 16) return CD360_ERR_ARG;
  const dim3 grid((unsigned)(((long)H * W + 255) / 256), B);
  vae_conv_out_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const uint16_t*)x, (const float*)w, (const float*)bias, (float*)out, H, W, Cin, Cout);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_vae_enc_conv_out_bf16(const void* x, const void* w, const void* bias, void* out, int B, int H, int W, int Cin, int Cout,
                                           void* stream) {
  if (!x || !w || !out || B <= 0 || H <= 0 || W <= 0) return CD360_ERR_ARG;
  if (Cin % 64 || Cin <= 0 || Cout < 1 || Cout > 8 || B > 65535) return CD360_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)w) % 16) return CD360_ERR_ARG;
  const long blocks = ((long)H * W + EO_PX - 1) / EO_PX;
  if (blocks > 0x7fffffffL) return CD360_ERR_SHAPE;
  vae_enc_conv_out_kernel<<<dim3((unsigned)blocks, B), 256, 0, (hipStream_t)stream>>>((const uint16_t*)x, (const float*)w, (const float*)bias,
                                                                                     (float*)out, H, W, Cin, Cout);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
