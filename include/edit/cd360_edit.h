/* cd360_edit.h -- C ABI of libcd360_edit.so: masked ("inpainting") and image-to-image sampling on the captured step (gfx950 / MI355X).
 *
 * A second, small library beside libcd360_hip.so, whose headers and exports are closed.  Same conventions as
 * ../cd360_hip.h and ../cd360_stochastic.h: device pointers owned by the caller, `stream` a hipStream_t passed as void*, all work enqueued
 * on it with no hidden synchronisation, nothing allocated, the environment never read, 0 on success and CD360_ERR_* (< 0) on error.  The
 * reference accepts `mask` / `init_im` (sgm/models/diffusion.py:376-401, sampling.py:112-136) and never reads them: there is no call site
 * to replace, the formulas below are the specification.  The Python binding types these entry points from cd360/_edit.py::EDIT_SIGNATURES.
 */
#ifndef CD360_EDIT_H
#define CD360_EDIT_H
#include <stdint.h>

#include "../cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the noise of the known region ------------------------------------------------------------------------------------
 * The generator of ../cd360_stochastic.h (Philox4x32-10 + Box-Muller, key = the two halves of seed) with the reserved fourth counter
 * word set to domain 3:
 *
 *   counter = (px, step, streams[smp], 3)
 *
 * Domains 0, 1 and 2 are a step's injected noise, the start latent and the first stage's posterior sample; their bits are what they
 * were.  One Philox call serves the four latent channels of a pixel; the value depends on the row's stream id only, not on bs, the grid
 * or the row's position.  out [bs, 4, HW] fp32; seed: device int64[1]; streams: device int32[bs] or NULL (stream 0 for every row); step:
 * device int32[1].  CD360_ERR_ARG for a null out / seed / step, bs <= 0, HW <= 0, HW > 2^32 (the pixel is one 32-bit counter word). */
int cd360_edit_noise_f32(void* out, const void* seed, const void* streams, const void* step, int bs, int64_t HW, void* stream);

/* ---- the blend that ends a masked sampling step -------------------------------------------------------------------------
 * After a solver's whole step to the noise level s', the region to keep is replaced by the known latent at that level.  Per element,
 * z = the domain-3 normal of (seed, streams[smp], step, channel, px), m = the mask value of the pixel (1 = generate, 0 = keep):
 *
 *   kn = (s' == 0) ? known : known + z * s'
 *   x' = m * x + (1 - m) * kn
 *
 * One fp32 rounding per operation, in this order.  No noise is generated on an s' == 0 row (the last row of a schedule: the kept region
 * ends as `known` itself).  x [bs, 4, HW] fp32 IN PLACE; known [bs, 4, HW] fp32; mask [mask_rows, HW] fp32 with mask_rows = 1 (one row
 * shared by all samples) or bs, a row shared by the four channels; step: device int32, the step word of the counter AND the index of
 * s' = sigma_next[step * sigma_stride], read on the device -- sigma_stride = 4 with sigma_next = column 1 of a [nsteps, 4] step table
 * (the staged step of cd360/job.py::Sampler), sigma_stride = 0 with sigma_next a device scalar (the un-staged step).
 * CD360_ERR_ARG for a null x / known / mask / sigma_next / step / seed, mask_rows outside {1, bs}, sigma_stride < 0, bs <= 0, HW <= 0,
 * HW > 2^32, x overlapping known or mask.  `streams` may be null. */
int cd360_mask_blend_f32(void* x, const void* known, const void* mask, int mask_rows, const void* sigma_next, int sigma_stride,
                         const void* step, const void* seed, const void* streams, int bs, int64_t HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_EDIT_H */
