/* cd360_highorder.h -- C ABI of libcd360_hip.so, part 5: DPM++ 2S ancestral and linear multistep sampling steps (gfx950 / MI355X).
 *
 * Same library, same conventions as cd360_hip.h, cd360_solvers.h, cd360_stochastic.h and cd360_edm.h: device pointers owned by the caller,
 * `stream` a hipStream_t passed as void*, all work enqueued on it with no hidden synchronisation, nothing allocated, the environment never
 * read, 0 on success and CD360_ERR_* (< 0) on error.  Each entry point names the reference call site it replaces (paths relative to the
 * reference tree).  The Python binding types these entry points from cd360/_lib.py::HIGHORDER_SIGNATURES.
 *
 * den_b, d0 and the two-branch request (a NaN scale_im, tested on the host) are those of cd360_stochastic.h, with the sigma named below.
 * One fp32 rounding per operation, in the order written.  Every `_cl` form takes eps [3 bs, HW, ld] bf16 channels-last (channels 0..3 of
 * every ld-wide row; ld >= 4, ld % 4 == 0, eps 8-byte aligned), or [2 bs, HW, ld] for two branches, its per-step scalars from [nsteps, 4]
 * fp32 tables and `step`, a device int32 that names the row; every `_f32` form takes eps [3n] fp32 (u | ic | c), or [2n] for two branches
 * (nothing behind it is read), and single table rows as 4-element fp32 device tensors.
 *
 * DPMPP2SAncestralSampler.sampler_step (sampling.py:365-387) evaluates the network twice: at (x, sigma) and at (x2, to_sigma(s)), where
 * s is the midpoint of sigma and sigma_down in -log sigma.  to_sigma(s) is NOT an entry of the denoiser's 1000-entry grid; DiscreteDenoiser
 * snaps it (denoiser.py:47-53), so c_in, c_out and the time-embedding row of the second evaluation come from sq_mid = q(sigma_mid).
 * Everything that depends on the schedule alone is evaluated once per schedule on the host (cd360/sampler.py::dpmpp2s_tables):
 *
 *   anc_tab     (sigma_down, sigma_up, s_noise, 0)                      the ancestral table of cd360_stochastic.h, as it is
 *   mid_tab     (sigma_mid, sigma_down, c_in(sq_mid), sq_mid)           the layout of cd360_edm.h's corr_tab: the second evaluation
 *   mult2s_tab  (m1, m2, m3, m4) = get_mult(h, s, t, t_next)            sampling.py:357-363
 *
 * A row with sigma_down = 0 (the last row; for eta > 1 interior rows as well) takes ONE evaluation in the reference (sampling.py:370-372)
 * and is exactly the ancestral Euler tail: run cd360_cfg_euler_ancestral_step_* there.  The tables hold finite filler on such rows (mid =
 * the step's own (sigma, sigma_next, c_in, sigma), mult2s = 0); the two entry points below are not meant for them.
 *
 * LinearMultistepSampler.__call__ (sampling.py:287-311) keeps the last `order` directions d = to_d(x, sigma, denoised).  Here they live in
 * a ring [order, bs, 4, HW] fp32 owned by the caller; step i writes slot i % order and reads slots (i - j) % order for 1 <= j <
 * min(i + 1, order).  lms_tab [nsteps, 4] = (c_0 .. c_3), c_j = linear_multistep_coeff(min(i + 1, order), sigmas, i, j), zero-padded
 * (cd360/sampler.py::lms_coefficients).  Slots with j >= min(i + 1, order) are never read: they may hold another image's history or nothing.
 */
#ifndef CD360_HIGHORDER_H
#define CD360_HIGHORDER_H
#include <stdint.h>

#include "cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- DPM++ 2S: the midpoint ---------------------------------------------------------------------------------------------
 * replaces `x2 = mult[0] * x - mult[1] * denoised` (sampling.py:379) and the elementwise tail of the denoise call in front of it.  Per
 * element, sigma = step_tab[step][0], (m1, m2) = mult2s_tab[step][0 / 1]:
 *
 *   d0 = the CFG combine of den_b = x - sigma eps_b
 *   x2 = m1 * x - m2 * d0
 *
 * The staged form: x [bs, 4, HW] fp32, READ ONLY (the second tail needs it); x2 [bs, 4, HW] fp32, a buffer of its own.  CD360_ERR_ARG for
 * a null x / eps / step_tab / mult2s_tab / step / x2, an overlap of x and x2, a misaligned eps, ld < 4 or ld % 4, bs <= 0, HW <= 0. */
int cd360_cfg_dpmpp2s_mid_cl(const void* x, const void* eps, const void* step_tab, const void* mult2s_tab, const void* step, float scale,
                             float scale_im, void* x2, int bs, int64_t HW, int ld, void* stream);

/* The un-staged form: x [n] fp32; sigma [1] and mult [4] = one row of mult2s_tab, fp32 device tensors; x2 [n] fp32: a buffer of its own,
 * overlapping no input (CD360_ERR_ARG otherwise, as for a null pointer or n <= 0). */
int cd360_cfg_dpmpp2s_mid_f32(const void* x, const void* eps, const void* sigma, const void* mult, float scale, float scale_im, void* x2, int64_t n,
                              void* stream);

/* ---- DPM++ 2S: the step -------------------------------------------------------------------------------------------------
 * replaces `x_dpmpp2s = mult[2] * x - mult[3] * denoised2` (sampling.py:381), the elementwise tail of the denoise call in front of it and
 * AncestralSampler.ancestral_step (sampling.py:250-256).  x holds the latent the midpoint read, x2 the midpoint's output, eps2 the
 * network's output at (x2, sigma_mid); sq_mid = mid_tab[step][3], (m3, m4) = mult2s_tab[step][2 / 3], (sigma_up, s_noise) =
 * anc_tab[step][1 / 2]:
 *
 *   d0' = the CFG combine of den_b = x2 - sq_mid eps2_b
 *   x'  = m3 * x - m4 * d0'
 *   x'  = x' + (z * s_noise) * sigma_up          where sigma_up != 0
 *
 * z is the draw of the device noise of cd360_stochastic.h for (seed, streams[row], step, channel, pixel): the same counter layout, the
 * reserved tag word 0; `step` is the row of the tables and the counter's step word.  Nothing is drawn on a sigma_up == 0 row.
 *
 * The staged form: x [bs, 4, HW] fp32 IN PLACE; x2 [bs, 4, HW] fp32, read: distinct buffers.  CD360_ERR_ARG for a null x / x2 / eps2 /
 * mid_tab / mult2s_tab / anc_tab / step / seed, an overlap of x and x2, a misaligned eps2, ld < 4 or ld % 4, bs <= 0, HW <= 0, HW > 2^32.
 * `streams` may be null (stream 0 for every row). */
int cd360_cfg_dpmpp2s_step_cl(void* x, const void* x2, const void* eps2, const void* mid_tab, const void* mult2s_tab, const void* anc_tab,
                              const void* step, const void* seed, const void* streams, float scale, float scale_im, int bs, int64_t HW, int ld,
                              void* stream);

/* The un-staged form: x, x2 [bs, 4, HW] fp32; eps2 [3 bs, 4, HW] fp32, or [2 bs, 4, HW]; mid_row / mult / anc [4] = one row of mid_tab /
 * mult2s_tab / anc_tab; step: device int32, the counter's step word; out [bs, 4, HW] fp32: a buffer of its own (CD360_ERR_ARG where it
 * overlaps an input, as for a null pointer other than streams, bs <= 0, HW <= 0, HW > 2^32). */
int cd360_cfg_dpmpp2s_step_f32(const void* x, const void* x2, const void* eps2, const void* mid_row, const void* mult, const void* anc,
                               const void* seed, const void* streams, const void* step, float scale, float scale_im, void* out, int bs, int64_t HW,
                               void* stream);

/* ---- linear multistep ---------------------------------------------------------------------------------------------------
 * replaces the elementwise lines of LinearMultistepSampler.__call__ behind the network (sampling.py:299-309, sampling_utils.py:39-40).
 * Per element, sigma = step_tab[step][0], (c_0 .. c_3) = lms_tab[step], i = step:
 *
 *   d0  = the CFG combine of den_b = x - sigma eps_b
 *   d   = (x - d0) / sigma;   ring[i % order] = d
 *   acc = c_0 * d;   acc += c_j * ring[(i - j) % order]   for j = 1 .. min(i + 1, order) - 1, in that order
 *   x'  = x + acc
 *
 * The staged form: x [bs, 4, HW] fp32 IN PLACE; ring [order, bs, 4, HW] fp32.  CD360_ERR_ARG for a null x / ring / eps / step_tab /
 * lms_tab / step, an overlap of x and the ring, a misaligned eps, ld < 4 or ld % 4, bs <= 0, HW <= 0, order outside 1..4. */
int cd360_cfg_lms_step_cl(void* x, void* ring, const void* eps, const void* step_tab, const void* lms_tab, const void* step, float scale,
                          float scale_im, int order, int bs, int64_t HW, int ld, void* stream);

/* The un-staged form: x [n] fp32; ring [order, n] fp32; sigma [1], row [4] = one row of lms_tab, step [1] int32: device tensors; out [n]
 * fp32: a buffer of its own.  CD360_ERR_ARG where out overlaps x, eps or the ring, or the ring overlaps x or eps, as for a null pointer,
 * n <= 0 or order outside 1..4. */
int cd360_cfg_lms_step_f32(const void* x, const void* eps, void* ring, const void* sigma, const void* row, const void* step, float scale,
                           float scale_im, int order, void* out, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_HIGHORDER_H */
