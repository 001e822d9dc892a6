/* cd360_solvers.h -- C ABI of libcd360_hip.so, part 2: sampler steps beyond Euler (gfx950 / MI355X).
 *
 * Same library, same conventions as cd360_hip.h: device pointers owned by the caller, `stream` a hipStream_t passed as void*, all work
 * enqueued on it with no hidden synchronisation, nothing allocated, the environment never read, 0 on success and CD360_ERR_* (< 0) on
 * error.  Each entry point names the reference call site it replaces (paths relative to the reference tree).  The Python binding types
 * these entry points from cd360/_lib.py::SOLVER_SIGNATURES.
 */
#ifndef CD360_SOLVERS_H
#define CD360_SOLVERS_H
#include <stdint.h>

#include "cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- DPM++ 2M ---------------------------------------------------------------------------------------------------------
 * replaces the elementwise tail of one DPMPP2MSampler.sampler_step (sampling.py:413-445) under DiscreteDenoiser + EpsScaling
 * (denoiser.py:41-44, denoiser_scaling.py:26-32) and ScheduledCFGImgTextRef / VanillaCFGImgRef (guiders.py:111-114, 144-147): the
 * second-order multistep solver at one network evaluation per step, in TABLE form.  get_variables / get_mult (sampling.py:391-411)
 * depend on the schedule alone, so the caller evaluates them once per schedule (cd360/sampler.py::dpmpp2m_multipliers) and hands in
 * (m1, m2, m3, m4) per step, with (m3, m4) = (1, 0) where the reference takes its first-order shortcut (sampling.py:433-435: the first
 * step, and sigma_next = 0).  Per element, s = sigma of the step:
 *
 *   den_b = x - s eps_b                                          per CFG branch
 *   d0    = den_u + scale (den_c - den_ic) + scale_im (den_ic - den_u)      three branches (u | ic | c)
 *         = den_u + scale (den_c - den_u)                                   two branches (u | c): a NaN scale_im, as in cd360_hip.h
 *   dd    = (m4 == 0) ? d0 : m3 d0 - m4 old
 *   x'    = m1 x - m2 dd;   old' = d0
 *
 * One fp32 rounding per operation, in this order.  `old` is NOT read when m4 == 0: on the first step of an image it may hold the previous
 * image's value or uninitialised memory (a NaN there must not reach x through 0 * NaN).  The NaN scale_im is tested on the host and
 * never reaches a kernel.
 *
 * The un-staged form (partner of the Euler f32 tail): x, old [n] fp32; eps [3n] fp32, or [2n] for two branches (nothing behind
 * eps[2n - 1] is read); sigma [1] and mult [4] = (m1, m2, m3, m4) fp32 device tensors; out, old_out [n] fp32: buffers of their own,
 * overlapping neither an input nor each other (CD360_ERR_ARG otherwise, as for a null pointer or n <= 0). */
int cd360_cfg_dpmpp2m_step_f32(const void* x, const void* eps, const void* old, const void* sigma, const void* mult, float scale,
                               float scale_im, void* out, void* old_out, int64_t n, void* stream);

/* The staged form (partner of the Euler channels-last tail, the end of a CAPTURED step of cd360/job.py::Sampler): x, old [bs, 4, HW] fp32,
 * both updated IN PLACE; eps [3 bs, HW, ld] bf16 channels-last (channels 0..3 of every ld-wide row; ld >= 4, ld % 4 == 0, eps 8-byte
 * aligned), or [2 bs, HW, ld] for two branches (no row of a third branch read); step_tab [nsteps, 4] fp32, of which column 0 (sigma) is
 * read; mult_tab [nsteps, 4] fp32 = (m1, m2, m3, m4); step: device int32, the row of both tables.  CD360_ERR_ARG for a null pointer,
 * `old` overlapping `x`, a misaligned eps, ld < 4 or ld % 4, bs <= 0, HW <= 0. */
int cd360_cfg_dpmpp2m_step_cl(void* x, void* old, const void* eps, const void* step_tab, const void* mult_tab, const void* step, float scale,
                              float scale_im, int bs, int64_t HW, int ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_SOLVERS_H */
