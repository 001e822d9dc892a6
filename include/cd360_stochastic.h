/* cd360_stochastic.h -- C ABI of libcd360_hip.so, part 3: device noise and the stochastic sampler steps built on it (gfx950 / MI355X).
 *
 * Same library, same conventions as cd360_hip.h and cd360_solvers.h: device pointers owned by the caller, `stream` a hipStream_t passed
 * as void*, all work enqueued on it with no hidden synchronisation, nothing allocated, the environment never read, 0 on success and
 * CD360_ERR_* (< 0) on error.  Each entry point names the reference call site it replaces (paths relative to the reference tree).  The
 * Python binding types these entry points from cd360/_lib.py::STOCHASTIC_SIGNATURES.
 */
#ifndef CD360_STOCHASTIC_H
#define CD360_STOCHASTIC_H
#include <stdint.h>

#include "cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device noise -----------------------------------------------------------------------------------------------------
 * replaces `torch.randn_like(x)` where a sampler draws noise inside a step (sampling.py:242, the `noise_sampler` of AncestralSampler;
 * sampling.py:99, the churn of EDMSampler): standard normals that are a PURE FUNCTION of (seed, noise stream, step index, channel,
 * pixel), so a graph replay, an eager launch, a fresh sampler and any batch / rank layout draw the same bits, and a captured step
 * holds no generator state.  Per replay row smp in [0, bs) and pixel px in [0, HW):
 *
 *   key     = (low 32 bits of seed, high 32 bits of seed)        seed: device int64[1], read on the device (reseeding = one 8-byte copy)
 *   counter = (px, step, streams[smp], 0)                        step: device int32[1]; streams: device int32[bs], NULL = stream 0 for
 *                                                                every row; the last word is a reserved domain tag
 *   r0..r3  = Philox4x32-10 as published in Random123 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85)
 *   u1 = ((r0 >> 8) + 1) 2^-24 in (0, 1],  u2 = (r1 >> 8) 2^-24 in [0, 1)
 *   rad = sqrtf(-2 logf(u1)),  z0 = rad cosf(6.2831855f u2),  z1 = rad sinf(6.2831855f u2);  (z2, z3) the same from (r2, r3)
 *
 * z_c is the noise of channel c of that pixel: one Philox call serves the four latent channels.  The value depends on the row's stream
 * id only, not on bs, the grid or the row's position.  out [bs, 4, HW] fp32.  CD360_ERR_ARG for a null out / seed / step, bs <= 0,
 * HW <= 0, HW > 2^32 (the pixel is one 32-bit counter word). */
int cd360_sampler_noise_f32(void* out, const void* seed, const void* streams, const void* step, int bs, int64_t HW, void* stream);

/* ---- ancestral Euler --------------------------------------------------------------------------------------------------
 * replaces the elementwise tail of one EulerAncestralSampler.sampler_step (sampling.py:340-347: ancestral_euler_step, :244-248, and
 * ancestral_step, :250-256) under DiscreteDenoiser + EpsScaling (denoiser.py:41-44, denoiser_scaling.py:26-32) and
 * ScheduledCFGImgTextRef / VanillaCFGImgRef (guiders.py:111-114, 144-147).  get_ancestral_step (sampling_utils.py:27-36) depends on the
 * schedule alone, so the caller evaluates it once per schedule (cd360/sampler.py::euler_ancestral_table) and hands in
 * (sigma_down, sigma_up, s_noise, 0) per step.  Per element, s = sigma of the step, z = the noise defined above:
 *
 *   den_b = x - s eps_b                                          per CFG branch
 *   d0    = den_u + scale (den_c - den_ic) + scale_im (den_ic - den_u)      three branches (u | ic | c)
 *         = den_u + scale (den_c - den_u)                                   two branches (u | c): a NaN scale_im, as in cd360_hip.h
 *   x_e   = x + (x - d0) / s * (sigma_down - s)
 *   x'    = (sigma_up == 0) ? x_e : x_e + (z * s_noise) * sigma_up
 *
 * One fp32 rounding per operation, in this order.  No noise is generated on a sigma_up == 0 row (the last row of a schedule, and every
 * row for eta = 0: plain Euler).  The NaN scale_im is tested on the host and never reaches a kernel.
 *
 * The un-staged form: x [bs, 4, HW] fp32; eps [3 bs, 4, HW] fp32, or [2 bs, 4, HW] for two branches (nothing behind it is read);
 * sigma [1] and anc [4] = (sigma_down, sigma_up, s_noise, 0) fp32 device tensors; seed / streams / step as above; out [bs, 4, HW] fp32, a
 * buffer of its own.  CD360_ERR_ARG for a null x / eps / sigma / anc / seed / step / out, bs <= 0, HW <= 0, HW > 2^32, out overlapping x
 * or eps.  `streams` may be null. */
int cd360_cfg_euler_ancestral_step_f32(const void* x, const void* eps, const void* sigma, const void* anc, const void* seed,
                                       const void* streams, const void* step, float scale, float scale_im, void* out, int bs, int64_t HW,
                                       void* stream);

/* The staged form (the end of a CAPTURED step of cd360/job.py::Sampler): x [bs, 4, HW] fp32 IN PLACE; eps [3 bs, HW, ld] bf16
 * channels-last (channels 0..3 of every ld-wide row; ld >= 4, ld % 4 == 0, eps 8-byte aligned), or [2 bs, HW, ld] for two branches (no
 * row of a third branch read); step_tab [nsteps, 4] fp32, of which column 0 (sigma) is read; anc_tab [nsteps, 4] fp32 = (sigma_down,
 * sigma_up, s_noise, 0); step: device int32, the row of both tables and the step word of the noise counter.  CD360_ERR_ARG for a null
 * x / eps / table / step / seed, a misaligned eps, ld < 4 or ld % 4, bs <= 0, HW <= 0, HW > 2^32.  `streams` may be null. */
int cd360_cfg_euler_ancestral_step_cl(void* x, const void* eps, const void* step_tab, const void* anc_tab, const void* step,
                                      const void* seed, const void* streams, float scale, float scale_im, int bs, int64_t HW, int ld,
                                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_STOCHASTIC_H */
