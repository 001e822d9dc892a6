/* cd360_picture.h -- C ABI of libcd360_picture.so: from a decoded uint8 frame to the tensors the first stage and the loss read
 * (gfx950 / MI355X).
 *
 * The arithmetic of the reference's data loader between a decoded picture and the first stage (sgm/data/data_co3d.py:332-352, 518-555,
 * 469-471): the square crop that may leave the picture, the antialiased resize with the uint8 roundings of its image library, ToTensor
 * and x * 2 - 1; the thresholded mask, cropped and resized by the nearest rule, its k x k dilation and the all-ones "padding" mask.  A
 * seventh library beside the six older ones, whose headers and exports are closed.  Same conventions as ../cd360_hip.h and
 * ../train/cd360_train.h: device pointers owned by the caller, `stream` a hipStream_t passed as void*, all work enqueued on it with no
 * hidden synchronisation, nothing allocated, the environment never read, 0 on success and CD360_ERR_* (< 0) on error, checked before
 * anything is launched.  All arithmetic is fp32, one rounding per operation, in the order written here (the build passes
 * -ffp-contract=off).  The Python binding types these entry points from cd360/_picture.py::PICTURE_SIGNATURES.
 */
#ifndef CD360_PICTURE_H
#define CD360_PICTURE_H
#include <stdint.h>

#include "../cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the longest row of a tap table (the taps of one output pixel): bicubic down-scaling by up to 15.5, bilinear by up to 31.5 */
#define CD360_PICTURE_MAX_TAPS 64
/* the largest dilation window of the mask entry */
#define CD360_PICTURE_MAX_DILATE 31

/* ---- a) crop + separable resize of one uint8 picture into fp32 planes: two launches ------------------------------------------
 * The crop window (left, top, w, h) is in picture pixels and may leave the picture [0, W) x [0, H) on any side; crop pixel (x, y) is
 * picture pixel (left + x, top + y), or `fill` where that lies outside the picture.  A tap table resizes one axis of the CROP
 * (n_in = w or h) to n_out = ow or oh: xmin int32 [n_out], size int32 [n_out], weights fp32 [n_out, taps] (row i: size[i] weights, the
 * rest ignored); the tables are made on the host (cd360/pictures.py), the kernels evaluate no filter.
 *   horizontal, for every row y of the crop (rows of fill included), output column i, channel c:
 *     t = 0;  for j = 0 .. x_size[i] - 1 in rising order:  t = t + x_w[i, j] * (float)crop[y, x_min[i] + j, c]
 *     round_u8:  t = min(255, max(0, floor(t + 0.5)))
 *     work[c, y, i] = t
 *   vertical, for every output row o, column i, channel c:
 *     v = 0;  for j = 0 .. y_size[o] - 1 in rising order:  v = v + y_w[o, j] * work[c, y_min[o] + j, i]
 *     round_u8:  v = min(255, max(0, floor(v + 0.5)))
 *     out[c, o, i] = (v / div) * mul + add                      three rounded operations; an image: div 255, mul 2, add -1
 * src uint8 [H, W, C] with C in {1, 3}, pixel stride C bytes, row stride `row_stride` bytes (>= W * C); work fp32 [C, h, ow], 16-byte
 * aligned, caller-allocated; out fp32 [C, oh, ow] contiguous at the pointer given (a slot of a batch tensor).  A tap outside its axis
 * (a malformed table) is skipped, never read.  16-byte stores where ow % 4 == 0 and out is 16-byte aligned, scalar ones otherwise.
 * CD360_ERR_ARG: a null or misaligned pointer (tables, work, out: 4 bytes; work 16), C outside {1, 3}, a non-positive size, an empty
 * crop (w <= 0 or h <= 0), row_stride < W * C, fill outside 0..255, taps <= 0, div == 0 or a value that is not finite, out or work
 * overlapping src or each other.  CD360_ERR_SHAPE: x_taps or y_taps > CD360_PICTURE_MAX_TAPS; H * row_stride, C * h * ow or
 * C * oh * ow >= 2^31 (offsets are 32-bit); a window coordinate beyond +-2^30. */
int cd360_picture_resample_u8(const void* src, int H, int W, int C, int64_t row_stride, int left, int top, int w, int h, int fill,
                              const void* x_min, const void* x_size, const void* x_w, int x_taps, const void* y_min, const void* y_size,
                              const void* y_w, int y_taps, int oh, int ow, int round_u8, float div, float mul, float add, void* work,
                              void* out, void* stream);

/* ---- b) the maps of one uint8 mask: one launch ------------------------------------------------------------------------------------
 * With sy(o) = floor((2 o + 1) h / (2 oh)) and sx(i) = floor((2 i + 1) w / (2 ow)) in integers (the nearest rule of a boolean image's
 * resize), (x, y) = (left + sx(i), top + sy(o)) and in = 1 if (x, y) lies in the picture, else 0:
 *   inside[o, i]  = in                                             the all-ones picture through the crop and the resize
 *   opacity[o, i] = in and src[y, x] > thr ? 1 : 0                 the thresholded mask, 0 outside the picture
 *   mask[o, i]    = 1 if any opacity[o + a, i + b] == 1 for |a|, |b| <= (k - 1) / 2 inside the map, else 0
 *                   (zero padding: clamp(conv2d(opacity, ones(k, k), padding="same"), 0, 1))
 * src uint8 [H, W] with row stride `row_stride` bytes (>= W); opacity, mask, inside fp32 [oh, ow], each may be NULL ("not wanted").
 * CD360_ERR_ARG: src null, all three outputs null, a misaligned output, a non-positive size, an empty crop, row_stride < W, thr outside
 * 0..255, k < 1 or even, an output overlapping src or another output.  CD360_ERR_SHAPE: k > CD360_PICTURE_MAX_DILATE; H * row_stride
 * or oh * ow >= 2^31; a window coordinate beyond +-2^30. */
int cd360_picture_mask_u8(const void* src, int H, int W, int64_t row_stride, int thr, int left, int top, int w, int h, int oh, int ow, int k,
                          void* opacity, void* mask, void* inside, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_PICTURE_H */
