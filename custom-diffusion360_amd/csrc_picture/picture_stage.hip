// libcd360_picture.so (include/picture/cd360_picture.h): from a decoded uint8 frame to what the first stage and the loss read.
//   picture_rows_kernel   the horizontal pass: every row of the crop (rows of fill included) through the x tap table -> work [C, h, ow]
//   picture_cols_kernel   the vertical pass over work through the y tap table, then (v / div) * mul + add -> out [C, oh, ow]
//   picture_mask_kernel   threshold + crop + nearest resize of a mask, its k x k dilation and the crop's "inside the picture" map
// The tap tables are made on the host; no filter is evaluated here, so a host restatement with the same table gives the same bits: every
// value is a chain of single fp32 operations in rising tap order (the build passes -ffp-contract=off).  All three are small memory-bound
// launches.  Horizontal: one thread owns one (crop row, output column) and all its channels, so the work planes are written along
// consecutive lanes; its source bytes are a few neighbouring pixels per lane, served by the vector L1.  Vertical: a thread owns four
// neighbouring output columns of one channel row, reads the work planes along x as 16-byte vectors and stores 16 bytes (ow % 4 == 0 and
// an aligned out), or one column in the scalar form.  Loops run to a table's size[i]: no register array is indexed by a loop counter,
// nothing spills.  No cross-workgroup accumulation anywhere.
#include "../csrc/cd360_common.h"

// as include/picture/cd360_picture.h defines them (tests/test_pictures_cpu.py holds the two together)
#define CD360_PICTURE_MAX_TAPS 64
#define CD360_PICTURE_MAX_DILATE 31

namespace {

struct Window {
  int left, top, w, h;
};

__device__ __forceinline__ float round_level(float v) {  // min(255, max(0, floor(v + 0.5)))
  const float r = floorf(v + 0.5f);
  return fminf(255.0f, fmaxf(0.0f, r));
}

// ------------------------------------------------------------------------------------------------ a) the horizontal pass
template <int C>
__global__ __launch_bounds__(256) void picture_rows_kernel(const uint8_t* __restrict__ src, int H, int W, int row_stride, Window win, float fill,
                                                           const int* __restrict__ x_min, const int* __restrict__ x_size,
                                                           const float* __restrict__ x_w, int x_taps, int ow, int round_u8,
                                                           float* __restrict__ work) {
  const long total = (long)win.h * ow;  // < 2^31: checked on the host
  for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long)gridDim.x * blockDim.x) {
    const int y = (int)(u / ow), i = (int)(u - (long)y * ow);
    const int py = win.top + y;
    const bool row_in = py >= 0 && py < H;
    const uint8_t* row = src + (row_in ? py * row_stride : 0);
    const int x0 = x_min[i];
    int n = x_size[i];
    n = n < x_taps ? n : x_taps;
    const float* wt = x_w + i * x_taps;
    float t[C];
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = 0.0f;
    for (int j = 0; j < n; ++j) {
      const int cx = x0 + j;
      if (cx < 0 || cx >= win.w) continue;  // a tap outside the crop: a malformed table, skipped
      const int px = win.left + cx;
      const bool in = row_in && px >= 0 && px < W;
      const float wj = wt[j];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float p = in ? (float)row[px * C + c] : fill;
        t[c] = t[c] + wj * p;
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) work[(c * win.h + y) * ow + i] = round_u8 ? round_level(t[c]) : t[c];
  }
}

// ------------------------------------------------------------------------------------------------ the vertical pass
// a unit = PX neighbouring columns of one output row of one channel; G = ceil(ow / PX) units per row
template <bool VEC>
__global__ __launch_bounds__(256) void picture_cols_kernel(const float* __restrict__ work, int h, const int* __restrict__ y_min,
                                                           const int* __restrict__ y_size, const float* __restrict__ y_w, int y_taps, int C,
                                                           int oh, int ow, int round_u8, float div, float mul, float add,
                                                           float* __restrict__ out) {
  constexpr int PX = VEC ? 4 : 1;
  const int G = (ow + PX - 1) / PX;
  const long total = (long)C * oh * G;
  for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long)gridDim.x * blockDim.x) {
    const int co = (int)(u / G), i = (int)(u - (long)co * G) * PX;
    const int c = co / oh, o = co - c * oh;
    const int y0 = y_min[o];
    int n = y_size[o];
    n = n < y_taps ? n : y_taps;
    const float* wt = y_w + o * y_taps;
    const float* plane = work + c * h * ow + i;
    float v[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) v[q] = 0.0f;
    for (int j = 0; j < n; ++j) {
      const int y = y0 + j;
      if (y < 0 || y >= h) continue;
      const float wj = wt[j];
      if constexpr (VEC) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(plane + y * ow);
        v[0] = v[0] + wj * p.x, v[1] = v[1] + wj * p.y, v[2] = v[2] + wj * p.z, v[3] = v[3] + wj * p.w;
      } else {
        v[0] = v[0] + wj * plane[y * ow];
      }
    }
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      float r = round_u8 ? round_level(v[q]) : v[q];
      r = r / div;
      r = r * mul;
      v[q] = r + add;
    }
    float* dst = out + (c * oh + o) * ow + i;
    if constexpr (VEC) {
      const f32x4 r = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(dst) = r;
    } else {
      dst[0] = v[0];
    }
  }
}

// ------------------------------------------------------------------------------------------------ b) the mask's maps
__device__ __forceinline__ int nearest(int o, int n_in, int n_out) { return (int)(((2LL * o + 1) * n_in) / (2LL * n_out)); }

// (inside the picture, over the threshold) at output (o, i)
__device__ __forceinline__ void mask_at(const uint8_t* __restrict__ src, int H, int W, int row_stride, int thr, Window win, int oh, int ow,
                                        int o, int i, bool& in, bool& on) {
  const int px = win.left + nearest(i, win.w, ow), py = win.top + nearest(o, win.h, oh);
  in = px >= 0 && px < W && py >= 0 && py < H;
  on = in && (int)src[py * row_stride + px] > thr;
}

__global__ __launch_bounds__(256) void picture_mask_kernel(const uint8_t* __restrict__ src, int H, int W, int row_stride, int thr, Window win,
                                                           int oh, int ow, int reach, float* __restrict__ opacity, float* __restrict__ mask,
                                                           float* __restrict__ inside) {
  const long total = (long)oh * ow;
  for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long)gridDim.x * blockDim.x) {
    const int o = (int)(u / ow), i = (int)(u - (long)o * ow);
    bool in, on;
    mask_at(src, H, W, row_stride, thr, win, oh, ow, o, i, in, on);
    if (inside) inside[u] = in ? 1.0f : 0.0f;
    if (opacity) opacity[u] = on ? 1.0f : 0.0f;
    if (mask) {
      bool any = on;
      const int o0 = o - reach < 0 ? 0 : o - reach, o1 = o + reach > oh - 1 ? oh - 1 : o + reach;
      const int i0 = i - reach < 0 ? 0 : i - reach, i1 = i + reach > ow - 1 ? ow - 1 : i + reach;
      for (int a = o0; a <= o1 && !any; ++a)
        for (int b = i0; b <= i1; ++b) {
          bool in2, on2;
          mask_at(src, H, W, row_stride, thr, win, oh, ow, a, b, in2, on2);
          any = any || on2;
        }
      mask[u] = any ? 1.0f : 0.0f;
    }
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

constexpr long LIMIT = 1L << 31;  // offsets are 32-bit
constexpr int REACH = 1 << 30;    // a window coordinate

inline bool window_bad(int left, int top, int w, int h) {
  return left < -REACH || left > REACH || top < -REACH || top > REACH || w > REACH || h > REACH;
}

}  // namespace

extern "C" int cd360_picture_resample_u8(const void* src, int H, int W, int C, int64_t row_stride, int left, int top, int w, int h, int fill,
                                         const void* x_min, const void* x_size, const void* x_w, int x_taps, const void* y_min,
                                         const void* y_size, const void* y_w, int y_taps, int oh, int ow, int round_u8, float div, float mul,
                                         float add, void* work, void* out, void* stream) {
  if (!src || !x_min || !x_size || !x_w || !y_min || !y_size || !y_w || !work || !out) return CD360_ERR_ARG;
  if (!aligned(x_min, 4) || !aligned(x_size, 4) || !aligned(x_w, 4) || !aligned(y_min, 4) || !aligned(y_size, 4) || !aligned(y_w, 4) ||
      !aligned(work, 16) || !aligned(out, 4))
    return CD360_ERR_ARG;
  if ((C != 1 && C != 3) || H <= 0 || W <= 0 || w <= 0 || h <= 0 || oh <= 0 || ow <= 0 || x_taps <= 0 || y_taps <= 0) return CD360_ERR_ARG;
  if (row_stride < (int64_t)W * C || fill < 0 || fill > 255) return CD360_ERR_ARG;
  if (!(fabsf(div) < INFINITY) || div == 0.0f || !(fabsf(mul) < INFINITY) || !(fabsf(add) < INFINITY)) return CD360_ERR_ARG;
  if (x_taps > CD360_PICTURE_MAX_TAPS || y_taps > CD360_PICTURE_MAX_TAPS) return CD360_ERR_SHAPE;
  if (window_bad(left, top, w, h)) return CD360_ERR_SHAPE;
  const long src_bytes = (long)H * row_stride, work_n = (long)C * h * ow, out_n = (long)C * oh * ow;
  if (row_stride >= LIMIT || src_bytes >= LIMIT || work_n >= LIMIT || out_n >= LIMIT) return CD360_ERR_SHAPE;
  if ((long)ow * x_taps >= LIMIT || (long)oh * y_taps >= LIMIT) return CD360_ERR_SHAPE;
  if (overlap(out, out_n * 4, src, src_bytes) || overlap(work, work_n * 4, src, src_bytes) || overlap(out, out_n * 4, work, work_n * 4))
    return CD360_ERR_ARG;
  const Window win{left, top, w, h};
#define CD360_PICTURE_ROWS(CH)                                                                                                                 \
  hipLaunchKernelGGL((picture_rows_kernel<CH>), dim3(stride_grid((long)h * ow)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, H, W, \
                     (int)row_stride, win, (float)fill, (const int*)x_min, (const int*)x_size, (const float*)x_w, x_taps, ow, round_u8,      \
                     (float*)work)
  if (C == 3) CD360_PICTURE_ROWS(3);
  else CD360_PICTURE_ROWS(1);
#undef CD360_PICTURE_ROWS
  CD360_LAUNCH_CHECK();
  const bool vec = ow % 4 == 0 && aligned(out, 16);
#define CD360_PICTURE_COLS(VEC)                                                                                                                  \
  hipLaunchKernelGGL((picture_cols_kernel<VEC>), dim3(stride_grid(out_n / ((VEC) ? 4 : 1))), dim3(256), 0, (hipStream_t)stream,                \
                     (const float*)work, h, (const int*)y_min, (const int*)y_size, (const float*)y_w, y_taps, C, oh, ow, round_u8, div, mul, \
                     add, (float*)out)
  if (vec) CD360_PICTURE_COLS(true);
  else CD360_PICTURE_COLS(false);
#undef CD360_PICTURE_COLS
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}

extern "C" int cd360_picture_mask_u8(const void* src, int H, int W, int64_t row_stride, int thr, int left, int top, int w, int h, int oh, int ow,
                                     int k, void* opacity, void* mask, void* inside, void* stream) {
  if (!src || (!opacity && !mask && !inside)) return CD360_ERR_ARG;
  if (!aligned(opacity, 4) || !aligned(mask, 4) || !aligned(inside, 4)) return CD360_ERR_ARG;
  if (H <= 0 || W <= 0 || w <= 0 || h <= 0 || oh <= 0 || ow <= 0 || row_stride < W || thr < 0 || thr > 255 || k < 1 || k % 2 == 0)
    return CD360_ERR_ARG;
  if (k > CD360_PICTURE_MAX_DILATE || window_bad(left, top, w, h)) return CD360_ERR_SHAPE;
  const long src_bytes = (long)H * row_stride, out_n = (long)oh * ow;
  if (row_stride >= LIMIT || src_bytes >= LIMIT || out_n >= LIMIT) return CD360_ERR_SHAPE;
  const void* outs[3] = {opacity, mask, inside};
  for (int a = 0; a < 3; ++a) {
    if (!outs[a]) continue;
    if (overlap(outs[a], out_n * 4, src, src_bytes)) return CD360_ERR_ARG;
    for (int b = a + 1; b < 3; ++b)
      if (outs[b] && overlap(outs[a], out_n * 4, outs[b], out_n * 4)) return CD360_ERR_ARG;
  }
  const Window win{left, top, w, h};
  hipLaunchKernelGGL(picture_mask_kernel, dim3(stride_grid(out_n)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, H, W, (int)row_stride,
                     thr, win, oh, ow, (k - 1) / 2, (float*)opacity, (float*)mask, (float*)inside);
  CD360_LAUNCH_CHECK();
  return CD360_OK;
}
