// libcd360_optim.so (include/optim/cd360_optim.h): the fine-tuning optimiser step with a live learning rate, gradient clipping and an
// exponential moving average of the trained weights.  Three kernels:
//   grad_sumsq_kernel   read-only pass over the bf16 gradients (2 bytes per element): one fp32 partial sum of squares per workgroup
//   grad_clip_kernel    one workgroup: partials -> (sumsq, norm, coef, 0)
//   adamw_live_kernel   adamw_kernel of ../csrc/adamw.hip in exactly its order, with lr / weight decay read from a device table, the
//                       gradient scaled by *coef and the EMA updated from the master it just wrote: 28 bytes per element as before,
//                       + 8 with the EMA (fp32 read and write)
// All HBM-bound and elementwise.  The tensors are scattered, so a launch takes up to 64 tensors by value in its arguments and a thread
// finds the tensor of its 8-value vector by bisection, as adamw_kernel does.  Every reduction runs in an order fixed by the tensor sizes
// alone (no atomics): a thread adds the squares of a vector, then its vectors' sums, in balanced trees; the workgroup adds its threads in
// a fixed tree.  One fp32 rounding per operation (the build passes -ffp-contract=off).
#include "../csrc/cd360_common.h"
#include "../csrc/cd360_adamw.h"

#define CD360_OPTIM_SUMSQ_VECS 2048  // include/optim/cd360_optim.h
#define CD360_OPTIM_SUMSQ_TERMS 64
#define CD360_OPTIM_SUMSQ_DEPTH 6

namespace {

constexpr int kThreads = 256;
constexpr int kVecsPerThread = CD360_OPTIM_SUMSQ_VECS / kThreads;
static_assert(kVecsPerThread * 8 == CD360_OPTIM_SUMSQ_TERMS, "a thread's term count is what the header states");

struct SumsqParams {
  const uint16_t* grad[CD360_ADAMW_MAX_TENSORS];
  long numel[CD360_ADAMW_MAX_TENSORS];
  long vec_end[CD360_ADAMW_MAX_TENSORS];  // cumulative number of 8-element vectors up to and including tensor t (this launch's index space)
  float* partials;
  int n;
};

struct LiveParams {
  const uint16_t* grad[CD360_ADAMW_MAX_TENSORS];
  uint16_t* param[CD360_ADAMW_MAX_TENSORS];
  long begin[CD360_ADAMW_MAX_TENSORS];  // offset of tensor t in the flat state buffers (multiple of 8)
  long numel[CD360_ADAMW_MAX_TENSORS];
  long vec_end[CD360_ADAMW_MAX_TENSORS];
  int row[CD360_ADAMW_MAX_TENSORS];  // tensor t reads (lr, wd) = hyper[2 * row[t]], hyper[2 * row[t] + 1]
  const float* hyper;
  const float* coef;  // null: the gradient is taken as it is
  float* master;
  float* exp_avg;
  float* exp_avg_sq;
  float* ema;  // null: no moving average
  const float* step;
  float beta1, beta2, eps, ema_decay;
  int n;
};

// sum of the workgroup's 256 values in a fixed tree (stride 128, 64, ... 1); the result is valid in thread 0
__device__ __forceinline__ float block_tree_sum(float v, float* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// workgroup b owns vectors [b * 2048, (b + 1) * 2048) of the launch; thread i takes vectors b * 2048 + k * 256 + i, k = 0 .. 7
// (consecutive lanes read consecutive 16-byte vectors, eight loads in flight per thread); a vector's eight squares are added as
// ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)) and the eight vector sums the same way: CD360_OPTIM_SUMSQ_DEPTH = 6 additions above any square
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const SumsqParams p) {
  __shared__ float sh[kThreads];
  const long total = p.vec_end[p.n - 1];
  float sv[kVecsPerThread];  // the sum of squares of each of the thread's vectors; 0 for a vector behind the launch's last
#pragma unroll
  for (int k = 0; k < kVecsPerThread; ++k) {
    const long vid = (long)blockIdx.x * CD360_OPTIM_SUMSQ_VECS + (long)k * kThreads + threadIdx.x;
    float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // the squares; 0 behind a tensor's last value
    if (vid < total) {
      int lo = 0, hi = p.n - 1;  // first tensor whose vec_end > vid
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.vec_end[mid] > vid) hi = mid; else lo = mid + 1;
      }
      const long e0 = (vid - (lo ? p.vec_end[lo - 1] : 0)) * 8;
      const long left = p.numel[lo] - e0;
      const int cnt = left < 8 ? (int)left : 8;
      const uint16_t* g = p.grad[lo] + e0;
      if (cnt == 8 && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const u32x4 gq = *reinterpret_cast<const u32x4*>(g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = bf16lo_to_f32(gq[e]), b = bf16hi_to_f32(gq[e]);
          q[2 * e] = a * a;
          q[2 * e + 1] = b * b;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (e < cnt) {
            const float a = bf16lo_to_f32((uint32_t)g[e]);
            q[e] = a * a;
          }
        }
      }
    }
    sv[k] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
  }
  static_assert(kVecsPerThread == 8, "the tree below adds eight vector sums");
  const float acc = ((sv[0] + sv[1]) + (sv[2] + sv[3])) + ((sv[4] + sv[5]) + (sv[6] + sv[7]));
  const float s = block_tree_sum(acc, sh);
  if (threadIdx.x == 0) p.partials[blockIdx.x] = s;
}

// thread i adds partials i, i + 256, i + 512, ... in this order; then the fixed tree
__global__ __launch_bounds__(256) void grad_clip_kernel(const float* __restrict__ partials, long count, float max_norm, float* __restrict__ out) {
  __shared__ float sh[kThreads];
  float acc = 0.f;
  for (long i = threadIdx.x; i < count; i += kThreads) acc = acc + partials[i];
  const float sumsq = block_tree_sum(acc, sh);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(sumsq);
    const float c = max_norm / (norm + 1e-6f);
    const float coef = c > 1.f ? 1.f : c;  // (a NaN stays a NaN: torch.clamp(max=1.0) keeps it too)
    f32x4 o = {sumsq, norm, coef, 0.f};
    *reinterpret_cast<f32x4*>(out) = o;
  }
}

__global__ __launch_bounds__(256) void adamw_live_kernel(const LiveParams p) {
  const float t = *p.step;
  const float bc1 = 1.f - powf(p.beta1, t), bc2_sqrt = sqrtf(1.f - powf(p.beta2, t));
  const bool clip = p.coef != nullptr, avg = p.ema != nullptr;
  const float coef = clip ? *p.coef : 1.f;
  const float warm = (1.f + t) / (10.f + t);
  const float omd = 1.f - (warm < p.ema_decay ? warm : p.ema_decay);  // 1 - min(ema_decay, (1 + t) / (10 + t))
  const long total = p.vec_end[p.n - 1];
  for (long vid = (long)blockIdx.x * blockDim.x + threadIdx.x; vid < total; vid += (long)gridDim.x * blockDim.x) {
    int lo = 0, hi = p.n - 1;  // first tensor whose vec_end > vid
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.vec_end[mid] > vid) hi = mid; else lo = mid + 1;
    }
    const long e0 = (vid - (lo ? p.vec_end[lo - 1] : 0)) * 8;  // first element of this vector inside tensor lo
    const long left = p.numel[lo] - e0;
    const int cnt = left < 8 ? (int)left : 8;
    const long r = 2L * p.row[lo];
    const float lr = p.hyper[r], decay = 1.f - lr * p.hyper[r + 1], step_size = lr / bc1;
    const uint16_t* g = p.grad[lo] + e0;
    uint16_t* w = p.param[lo] + e0;
    const long s = p.begin[lo] + e0;
    const bool wide = cnt == 8 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
    float gv[8], mv[8], vv[8], xv[8], av[8];
    if (wide) {
      const u32x4 gq = *reinterpret_cast<const u32x4*>(g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gv[2 * e] = bf16lo_to_f32(gq[e]);
        gv[2 * e + 1] = bf16hi_to_f32(gq[e]);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(p.exp_avg + s + 4 * h), v4 = *reinterpret_cast<const f32x4*>(p.exp_avg_sq + s + 4 * h),
                    x4 = *reinterpret_cast<const f32x4*>(p.master + s + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          mv[4 * h + e] = m4[e];
          vv[4 * h + e] = v4[e];
          xv[4 * h + e] = x4[e];
        }
        if (avg) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(p.ema + s + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) av[4 * h + e] = a4[e];
        }
      }
    } else {
      for (int e = 0; e < cnt; ++e) {
        gv[e] = bf16lo_to_f32((uint32_t)g[e]);
        mv[e] = p.exp_avg[s + e];
        vv[e] = p.exp_avg_sq[s + e];
        xv[e] = p.master[s + e];
        if (avg) av[e] = p.ema[s + e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (e < cnt) {  // torch.optim.adamw._single_tensor_adamw, in its order
        if (clip) gv[e] = gv[e] * coef;
        xv[e] *= decay;
        mv[e] += (gv[e] - mv[e]) * (1.f - p.beta1);
        vv[e] = vv[e] * p.beta2 + (1.f - p.beta2) * gv[e] * gv[e];
        const float denom = sqrtf(vv[e]) / bc2_sqrt + p.eps;
        xv[e] -= step_size * (mv[e] / denom);
        if (avg) av[e] = av[e] - omd * (av[e] - xv[e]);  // LitEma.forward: shadow.sub_(one_minus_decay * (shadow - param))
      }
    }
    if (wide) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 m4, v4, x4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          m4[e] = mv[4 * h + e];
          v4[e] = vv[4 * h + e];
          x4[e] = xv[4 * h + e];
        }
        *reinterpret_cast<f32x4*>(p.exp_avg + s + 4 * h) = m4;
        *reinterpret_cast<f32x4*>(p.exp_avg_sq + s + 4 * h) = v4;
        *reinterpret_cast<f32x4*>(p.master + s + 4 * h) = x4;
        if (avg) {
          f32x4 a4;
#pragma unroll
          for (int e = 0; e < 4; ++e) a4[e] = av[4 * h + e];
          *reinterpret_cast<f32x4*>(p.ema + s + 4 * h) = a4;
        }
      }
      u32x4 wq;
#pragma unroll
      for (int e = 0; e < 4; ++e) wq[e] = pack_bf16x2(xv[2 * e], xv[2 * e + 1]);
      *reinterpret_cast<u32x4*>(w) = wq;
    } else {
      for (int e = 0; e < cnt; ++e) {
        p.exp_avg[s + e] = mv[e];
        p.exp_avg_sq[s + e] = vv[e];
        p.master[s + e] = xv[e];
        if (avg) p.ema[s + e] = av[e];
        w[e] = (uint16_t)(pack_bf16x2(xv[e], 0.f) & 0xffffu);
      }
    }
  }
}

// [a, a + bytes) and [b, b + bytes) share a byte
inline bool overlap(const void* a, const void* b, uint64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" int cd360_grad_sumsq_bf16(int n, const void* const* grads, const int64_t* numel, void* partials, void* stream) {
  if (n <= 0 || n > CD360_ADAMW_MAX_TENSORS || !grads || !numel || !partials || (uintptr_t)partials % 4) return CD360_ERR_ARG;
  SumsqParams p;
  long vecs = 0;
  for (int t = 0; t < n; ++t) {
    if (!grads[t] || numel[t] <= 0) return CD360_ERR_ARG;
    if ((uintptr_t)grads[t] % 2) return CD360_ERR_SHAPE;
    p.grad[t] = (const uint16_t*)grads[t];
    p.numel[t] = numel[t];
    vecs += (numel[t] + 7) / 8;
    p.vec_end[t] = vecs;
  }
  p.partials = (float*)partials;
  p.n = n;
  const long blocks = (vecs + CD360_OPTIM_SUMSQ_VECS - 1) / CD360_OPTIM_SUMSQ_VECS;
  if (blocks > 0x7fffffffL) return CD360_ERR_SHAPE;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, p);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_grad_clip_f32(const void* partials, int64_t count, float max_norm, void* out, void* stream) {
  if (!partials || !out || count <= 0 || (uintptr_t)partials % 4 || (uintptr_t)out % 16 || !(max_norm >= 0.f)) return CD360_ERR_ARG;
  const uintptr_t a = (uintptr_t)partials, o = (uintptr_t)out;
  if (o < a + (uint64_t)count * 4 && a < o + 16) return CD360_ERR_ARG;
  hipLaunchKernelGGL(grad_clip_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const float*)partials, (long)count, max_norm, (float*)out);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_adamw_live_bf16(int n, const void* const* grads, void* const* params, const int64_t* begin, const int64_t* numel,
                                     const int32_t* row, const void* hyper, int hyper_rows, const void* coef, void* master, void* exp_avg,
                                     void* exp_avg_sq, void* ema, float ema_decay, const void* step, float beta1, float beta2, float eps,
                                     void* stream) {
  if (n <= 0 || n > CD360_ADAMW_MAX_TENSORS || !grads || !params || !begin || !numel || !row || !hyper || hyper_rows <= 0 || !master || !exp_avg ||
      !exp_avg_sq || !step)
    return CD360_ERR_ARG;
  if (((uintptr_t)master | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) % 16 ||
      ((uintptr_t)step | (uintptr_t)hyper | (uintptr_t)coef) % 4)
    return CD360_ERR_ARG;
  LiveParams p;
  long vecs = 0, extent = 0;
  for (int t = 0; t < n; ++t) {
    if (!grads[t] || !params[t] || numel[t] <= 0 || begin[t] < 0 || row[t] < 0 || row[t] >= hyper_rows) return CD360_ERR_ARG;
    if (begin[t] % 8 || ((uintptr_t)grads[t] | (uintptr_t)params[t]) % 2) return CD360_ERR_SHAPE;
    p.grad[t] = (const uint16_t*)grads[t];
    p.param[t] = (uint16_t*)params[t];
    p.begin[t] = begin[t];
    p.numel[t] = numel[t];
    vecs += (numel[t] + 7) / 8;
    p.vec_end[t] = vecs;
    p.row[t] = row[t];
    if (begin[t] + numel[t] > extent) extent = begin[t] + numel[t];
  }
  if (ema && (overlap(ema, master, (uint64_t)extent * 4) || overlap(ema, exp_avg, (uint64_t)extent * 4) || overlap(ema, exp_avg_sq, (uint64_t)extent * 4)))
    return CD360_ERR_ARG;
  p.hyper = (const float*)hyper; p.coef = (const float*)coef;
  p.master = (float*)master; p.exp_avg = (float*)exp_avg; p.exp_avg_sq = (float*)exp_avg_sq; p.ema = (float*)ema; p.step = (const float*)step;
  p.beta1 = beta1; p.beta2 = beta2; p.eps = eps; p.ema_decay = ema_decay; p.n = n;
  const long blocks = (vecs + 255) / 256;
  hipLaunchKernelGGL(adamw_live_kernel, dim3((unsigned)(blocks > 256L * 16 ? 256L * 16 : blocks)), dim3(kThreads), 0, (hipStream_t)stream, p);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
