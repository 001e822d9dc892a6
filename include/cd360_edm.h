/* cd360_edm.h -- C ABI of libcd360_hip.so, part 4: the EDM sampler family with churn, and the Heun corrector (gfx950 / MI355X).
 *
 * Same library, same conventions as cd360_hip.h, cd360_solvers.h and cd360_stochastic.h: device pointers owned by the caller, `stream` a
 * hipStream_t passed as void*, all work enqueued on it with no hidden synchronisation, nothing allocated, the environment never read, 0
 * on success and CD360_ERR_* (< 0) on error.  Each entry point names the reference call site it replaces (paths relative to the
 * reference tree).  The Python binding types these entry points from cd360/_lib.py::EDM_SIGNATURES.
 *
 * EDMSampler.sampler_step (sampling.py:96-110) with gamma > 0 evaluates the network at sigma_hat = sigma (1 + gamma), which is NOT an
 * entry of the denoiser's 1000-entry grid; DiscreteDenoiser snaps it (denoiser.py:47-53).  So c_in, c_out and the time-embedding row come
 * from sq = q(sigma_hat), while to_d and dt keep the un-snapped sigma_hat.  Everything that depends on the schedule alone is evaluated
 * once per schedule on the host (cd360/sampler.py::edm_tables), three [nsteps, 4] fp32 tables:
 *
 *   edm_tab    (sigma_hat, sigma_next, c_in(sq), sq)                   the layout of the Euler step table with column 3 filled
 *   corr_tab   (sigma_next, sigma_next, c_in(sq'), sq'), sq' = q(sigma_next)      the corrector's evaluation
 *   churn_tab  (gamma, noise_std, s_noise, 0), noise_std = (sigma_hat^2 - sigma^2)^0.5
 *
 * den_b, d0 and the two-branch request (a NaN scale_im, tested on the host) are those of cd360_stochastic.h, with the sigma named below.
 * One fp32 rounding per operation, in the order written.
 */
#ifndef CD360_EDM_H
#define CD360_EDM_H
#include <stdint.h>

#include "cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- churn --------------------------------------------------------------------------------------------------------------
 * replaces `x = x + torch.randn_like(x) * s_noise * (sigma_hat**2 - sigma**2) ** 0.5` (sampling.py:98-100), in front of the network:
 *
 *   x <- x + (z * s_noise) * noise_std          (noise_std, s_noise) = churn_tab[step][1 / 2]
 *
 * x [bs, 4, HW] fp32, IN PLACE.  z is the draw of the device noise of cd360_stochastic.h for (seed, streams[row], step, channel, pixel):
 * the same counter layout, the reserved tag word 0; `step` (device int32) is the row of churn_tab and the counter's step word.  On a
 * noise_std == 0 row (gamma = 0) the kernel returns without reading or writing x.  A launch of its own because the stage-in convolution
 * reads a 3x3 halo of x.  CD360_ERR_ARG for a null x / churn_tab / step / seed, bs <= 0, HW <= 0, HW > 2^32.  `streams` may be null. */
int cd360_edm_churn_f32(void* x, const void* churn_tab, const void* step, const void* seed, const void* streams, int bs, int64_t HW,
                        void* stream);

/* ---- predictor ----------------------------------------------------------------------------------------------------------
 * replaces the elementwise tail of EDMSampler.sampler_step up to euler_step (sampling.py:102-106, sampling_utils.py:39-40).  Per element,
 * (sigma_hat, sigma_next, -, sq) one row of edm_tab:
 *
 *   d0  = the CFG combine of den_b = x - sq eps_b
 *   d   = (x - d0) / sigma_hat
 *   xe  = x + d * (sigma_next - sigma_hat)
 *   dir = d                                      when dir is not null
 *
 * With sq == sigma_hat xe holds the bits of the Euler tails of cd360_hip.h.
 *
 * The staged form: x, xe, dir [bs, 4, HW] fp32; xe == x is allowed (the in-place form: with dir null, the churned Euler tail), any other
 * overlap of x / xe / dir is refused; eps [3 bs, HW, ld] bf16 channels-last (channels 0..3 of every ld-wide row; ld >= 4, ld % 4 == 0, eps
 * 8-byte aligned), or [2 bs, HW, ld] for two branches; step: device int32, the row of edm_tab.  CD360_ERR_ARG for a null x / eps / edm_tab /
 * step / xe, a misaligned eps, ld < 4 or ld % 4, bs <= 0, HW <= 0. */
int cd360_cfg_edm_predict_cl(const void* x, const void* eps, const void* edm_tab, const void* step, float scale, float scale_im, void* xe,
                             void* dir, int bs, int64_t HW, int ld, void* stream);

/* The un-staged form: x [n] fp32; eps [3n] fp32, or [2n] for two branches (nothing behind it is read); row [4] = one row of edm_tab, an
 * fp32 device tensor; xe [n] and dir [n] (or null) fp32: buffers of their own, overlapping neither an input nor each other (CD360_ERR_ARG
 * otherwise, as for a null x / eps / row / xe or n <= 0). */
int cd360_cfg_edm_predict_f32(const void* x, const void* eps, const void* row, float scale, float scale_im, void* xe, void* dir, int64_t n,
                              void* stream);

/* ---- corrector ----------------------------------------------------------------------------------------------------------
 * replaces the elementwise tail of HeunEDMSampler.possible_correction_step (sampling.py:329-337).  x holds x_hat (the latent the
 * predictor read), xe and dir are the predictor's outputs, eps2 the network's output at (xe, sigma_next); (sigma_hat, sigma_next) from the
 * row of edm_tab, sq' from column 3 of the row of corr_tab:
 *
 *   d0'   = the CFG combine of den_b = xe - sq' eps2_b
 *   d_new = (xe - d0') / sigma_next
 *   d'    = (dir + d_new) / 2.0
 *   x    <- x + d' * (sigma_next - sigma_hat)
 *
 * On a row whose sigma_next is not > 0: x <- xe, and neither eps2 nor dir is read (the reference's torch.where, sampling.py:334-336).
 *
 * The staged form: x [bs, 4, HW] fp32 IN PLACE; xe, dir [bs, 4, HW] fp32, read; the three are distinct buffers; eps2, ld as eps above; step:
 * device int32, the row of both tables.  CD360_ERR_ARG for a null pointer, an overlap among x / xe / dir, a misaligned eps2, ld < 4 or
 * ld % 4, bs <= 0, HW <= 0. */
int cd360_cfg_edm_correct_cl(void* x, const void* xe, const void* dir, const void* eps2, const void* edm_tab, const void* corr_tab,
                             const void* step, float scale, float scale_im, int bs, int64_t HW, int ld, void* stream);

/* The un-staged form: x, xe, dir [n] fp32; eps2 [3n] fp32, or [2n] for two branches; row / corr_row [4] = one row of edm_tab / corr_tab,
 * fp32 device tensors; out [n] fp32: a buffer of its own (CD360_ERR_ARG where it overlaps an input, as for a null pointer or n <= 0). */
int cd360_cfg_edm_correct_f32(const void* x, const void* xe, const void* dir, const void* eps2, const void* row, const void* corr_row,
                              float scale, float scale_im, void* out, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_EDM_H */
