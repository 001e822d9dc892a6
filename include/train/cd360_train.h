/* cd360_train.h -- C ABI of libcd360_train.so: the two ends of a captured fine-tuning step (gfx950 / MI355X).
 *
 * The front of StandardDiffusionLossImgRef.__call__ + DiscreteDenoiser (sgm/modules/diffusionmodules/loss.py:146-168, denoiser.py:22-44
 * of the reference, with CubicSampling / DiscreteSampling, EpsScaling and EpsWeighting) and the l2 tail of get_loss (loss.py:183-187), as
 * four launches whose random numbers are a pure function of (seed, noise stream, step, channel, pixel).  A sixth library beside the five
 * older ones, whose headers and exports are closed.  Same conventions as ../cd360_hip.h and ../edit/cd360_edit.h: device pointers owned by
 * the caller, `stream` a hipStream_t passed as void*, all work enqueued on it with no hidden synchronisation, nothing allocated, the
 * environment never read, 0 on success and CD360_ERR_* (< 0) on error, checked before anything is launched.  All arithmetic is fp32, one
 * rounding per operation, in the order written here (the build passes -ffp-contract=off).  The Python binding types these entry points
 * from cd360/_train.py::TRAIN_SIGNATURES.
 *
 * The generator is the one of ../cd360_stochastic.h (Philox4x32-10 + Box-Muller, key = the two halves of seed, counter = (pixel, step,
 * streams[b], domain)) in four new domains; domains 0-3 keep their bits:
 *   4  the per-sample draws of a training step (sigma indices, offset noise)      counter (0, step, streams[b], 4)
 *   5  the target noise                                                            counter (px, step, streams[b], 5)
 *   6  the first noising of the reference views (the loss's)                       counter (view * HW + px, step, streams[b], 6)
 *   7  the second noising of the reference views (the denoiser's)                  counter (view * HW + px, step, streams[b], 7)
 */
#ifndef CD360_TRAIN_H
#define CD360_TRAIN_H
#include <stdint.h>

#include "../cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The scalar row of one sample: CD360_TRAIN_ROW fp32 values, rows[b * CD360_TRAIN_ROW + k]:
 *   0 sigma      1 w = 1 / (sigma * sigma)      2 c_skip = 1      3 c_out = -sigma      4 c_in = 1 / sqrtf(sigma * sigma + 1)
 *   5 sigma_ref  6 c_in_ref = 1 / sqrtf(sigma_ref * sigma_ref + 1)      7 off_tgt      8 off_ref      9..11 zero */
#define CD360_TRAIN_ROW 12
/* how a sigma sampler turns a 32-bit draw r into an index of its table of num_idx entries:
 *   CUBIC     u = (r >> 8) * 2^-24;  idx = (int64)((1.0f - u * u * u) * (float)(num_idx - 1))        (CubicSampling)
 *   DISCRETE  idx = start + r % (num_idx - start)                                                    (DiscreteSampling, num_idx_start) */
#define CD360_TRAIN_CUBIC 0
#define CD360_TRAIN_DISCRETE 1

/* ---- a) the per-sample scalars: one launch of one workgroup ---------------------------------------------------------------
 * Per row b: (r0, r1, r2, r3) = philox(counter (0, *step, streams[b], 4));  sigma = tgt_table[index(tgt_kind, r0)];
 * sigma_ref = ref_table[index(ref_kind, r1)];  (off_tgt, off_ref) = box_muller(r2, r3);  the row above;
 * timesteps[b] = argmin_i |sigma - table[i]| (the first minimum: DiscreteDenoiser.sigma_to_idx);  sigmas_ref_idx[b] = the same of sigma_ref.
 * step_used[0] = *step as it was read; with advance != 0, *step = *step + 1 (modulo 2^32) after every row has read it, so a graph
 * replay draws the next step.  table [n_table], tgt_table [n_tgt], ref_table [n_ref] fp32; seed device int64[1]; streams device
 * int32[B] or NULL (stream 0 for every row); step device int32[1] (in/out with advance; it may overlap no other argument); rows [B, CD360_TRAIN_ROW] fp32; timesteps,
 * sigmas_ref_idx device int64[B]; step_used device int32[1].
 * CD360_ERR_ARG: a null or misaligned pointer (seed 8 bytes, the int64 outputs 8, the others 4), B <= 0, a table size <= 0, a kind
 * outside {0, 1}, step overlapping step_used, rows, timesteps, sigmas_ref_idx, seed or streams.  CD360_ERR_SHAPE: start < 0 or start >= num_idx of a DISCRETE sampler, a CUBIC table of more than 2^24 entries. */
int cd360_train_sigmas_f32(const void* table, int n_table, const void* tgt_table, int n_tgt, int tgt_kind, int tgt_start,
                           const void* ref_table, int n_ref, int ref_kind, int ref_start, const void* seed, const void* streams,
                           void* step, int advance, void* rows, void* timesteps, void* sigmas_ref_idx, void* step_used, int B,
                           void* stream);

/* ---- b) the bulk pass: noised target and noised reference views, scaled for the network --------------------------------------
 * With the row of sample b, z = the domain-5 normal of (px, *step_used, streams[b]), z_a / z_b those of domains 6 / 7 at pixel word
 * view * HW + px:
 *   z'   = level > 0 ? z + level * off_tgt : z          x_t = x0 + z' * sigma           x_in = x_t * c_in
 *   xr0  = drop_im ? drop_im[b] * xr : xr               za' = level > 0 ? z_a + level * off_ref : z_a
 *   xr1  = xr0 + za' * sigma_ref                        xr2 = xr1 + z_b * sigma_ref     xr_in = xr2 * c_in_ref
 * x0, x_t [B, 4, HW] fp32; xr [B, n, 4, HW] fp32 or NULL (then xr_in is not touched and n is ignored); drop_im [B] fp32 or NULL;
 * x_in [B, 4, HW] and xr_in [B, n, 4, HW] in out_dtype: 0 = fp32, 1 = bf16 (round to nearest even of the fp32 value).  It reads
 * step_used, never step.  CD360_ERR_ARG: a null or misaligned pointer, B <= 0, HW <= 0, n <= 0 with xr, out_dtype outside {0, 1}, a
 * level that is negative or not finite, an output overlapping an input.  CD360_ERR_SHAPE: HW > 2^32 or n * HW > 2^32 (the pixel is one
 * 32-bit counter word). */
int cd360_train_noise_f32(const void* x0, const void* xr, const void* drop_im, const void* rows, const void* seed, const void* streams,
                          const void* step_used, float level, void* x_t, void* x_in, void* xr_in, int out_dtype, int B, int n, int64_t HW,
                          void* stream);

/* ---- c) the l2 term of the loss ---------------------------------------------------------------------------------------------
 *   D = eps * c_out + x_t * c_skip      err = D - x0      t = w * (err * err)
 *   mask:     loss[b] = sum_{c, px} t * mask[b, px] / den[b],   den[b] = sum_px mask[b, px] + 1e-6
 *   no mask:  loss[b] = sum_{c, px} t / den[b],                 den[b] = 4 * HW
 * eps [B, 4, H, W] of eps_dtype (0 = fp32, 1 = bf16) addressed by its four element strides eps_strides (a host array: batch, channel,
 * row, column; every stride >= 0), so the network's output is read where it lies, channels-last or not; x_t, x0 [B, 4, H, W] fp32
 * contiguous; mask [B, 1, H, W] fp32 or NULL; loss, den [B] fp32.  One workgroup per sample sums in a fixed order, without atomics: the
 * result does not depend on a grid and is the same bits on every run.
 * CD360_ERR_ARG: a null or misaligned pointer or stride array, B <= 0, H <= 0, W <= 0, eps_dtype outside {0, 1}.  CD360_ERR_SHAPE: a
 * negative stride, H * W > 2^28. */
int cd360_train_l2_f32(const void* eps, int eps_dtype, const int64_t* eps_strides, const void* x_t, const void* x0, const void* rows,
                       const void* mask, void* loss, void* den, int B, int H, int W, void* stream);

/* ---- d) its backward ----------------------------------------------------------------------------------------------------------
 *   d_eps = g[b] * (((((2 * w) * err) * c_out) [* mask[b, px]]) / den[b]);  an exact 0 where g[b] == 0, whatever err holds
 * g [B] fp32 (the gradient of loss); den [B] as c) wrote it; d_eps in eps's dtype, addressed by d_strides like eps by eps_strides. */
int cd360_train_l2_bwd_f32(const void* eps, int eps_dtype, const int64_t* eps_strides, const void* x_t, const void* x0, const void* rows,
                           const void* mask, const void* den, const void* g, void* d_eps, const int64_t* d_strides, int B, int H, int W,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_TRAIN_H */
