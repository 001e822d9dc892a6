/* cd360_optim.h -- C ABI of libcd360_optim.so: the fine-tuning optimiser step with a live learning rate, gradient clipping and an
 * exponential moving average of the trained weights, inside the one pass that reads the gradient (gfx950 / MI355X).
 *
 * A third, small library beside libcd360_hip.so and libcd360_edit.so, whose headers and exports are closed.  Same conventions as
 * ../cd360_hip.h: device pointers owned by the caller, `stream` a hipStream_t passed as void*, all work enqueued on it with no hidden
 * synchronisation, nothing allocated, the environment never read, 0 on success and CD360_ERR_* (< 0) on error.  Pointer, size and row
 * ARRAYS are HOST arrays read before the call returns (they travel by value in the kernel arguments), as in cd360_adamw_bf16 of
 * ../cd360_hip.h; everything else named "device" is read or written by the kernels only, so every entry point can be captured into a
 * hipGraph and the values behind those pointers may change between replays.  The step counter is the one of ../cd360_hip.h: advance it
 * with cd360_adamw_tick before the cd360_adamw_live_bf16 launches of a step.  The Python binding types these entry points from
 * cd360/_optim.py::OPTIM_SIGNATURES.
 */
#ifndef CD360_OPTIM_H
#define CD360_OPTIM_H
#include <stdint.h>

#include "../cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One workgroup of the sum-of-squares pass owns CD360_OPTIM_SUMSQ_VECS consecutive 8-value vectors of its launch (a tensor of numel
 * values is ceil(numel / 8) vectors, the last one short) and writes ONE partial.  A launch over tensors of sizes numel[0 .. n-1] therefore
 * writes exactly
 *
 *   ceil( sum_t ceil(numel[t] / 8) / CD360_OPTIM_SUMSQ_VECS )
 *
 * partials: a function of the sizes alone.  A thread adds its CD360_OPTIM_SUMSQ_TERMS squares (8 vectors of 8) in a balanced tree: every
 * square passes through CD360_OPTIM_SUMSQ_DEPTH additions there, then through the 8 levels of the workgroup's tree over 256 threads. */
#define CD360_OPTIM_SUMSQ_VECS 2048
#define CD360_OPTIM_SUMSQ_TERMS 64
#define CD360_OPTIM_SUMSQ_DEPTH 6

/* ---- squared L2 norm of the gradients, first pass --------------------------------------------------------------------------
 * Replaces the norm half of torch.nn.utils.clip_grad_norm_ (torch/nn/utils/clip_grad.py: _foreach_norm over the gradients, then
 * linalg.vector_norm of the stack; Lightning's gradient_clip_val under which the reference trains, main.py) by one read-only pass over the
 * bf16 gradients.  n <= CD360_ADAMW_MAX_TENSORS tensors; grads[t] a bf16 device pointer (2-byte aligned is enough) to numel[t] values.
 * partials: device fp32, this launch's slice, of the length given above; EVERY entry of the slice is written by every launch (no
 * zero-fill is needed, nothing is accumulated into, no atomics).  Grid, slice length and the order of every addition depend on the
 * sizes alone: the bits of the result are the same run to run and between an eager launch and a graph replay.  Each square and each
 * addition is one fp32 rounding.
 * CD360_ERR_ARG for n outside 1 .. CD360_ADAMW_MAX_TENSORS, a null grads / numel / partials / grads[t], numel[t] <= 0, partials not
 * 4-byte aligned; CD360_ERR_SHAPE for an odd grads[t]. */
int cd360_grad_sumsq_bf16(int n, const void* const* grads, const int64_t* numel, void* partials, void* stream);

/* ---- norm and clip factor, second pass -----------------------------------------------------------------------------------
 * Replaces the other half of clip_grad_norm_ (clip_coef = max_norm / (total_norm + 1e-6); clip_coef_clamped = clamp(clip_coef, max=1.0))
 * without its host read.  One workgroup of 256 threads reduces partials[0 .. count-1] in a fixed order (thread i adds partials i, i + 256,
 * ... one after the other, then a tree of 8 levels) and writes
 *
 *   out[0] = sumsq      out[1] = norm = sqrtf(sumsq)      out[2] = coef = min(1, max_norm / (norm + 1e-6f))      out[3] = 0
 *
 * one fp32 rounding per operation, in the order written.  A non-finite norm PROPAGATES, as with torch's default error_if_nonfinite=False:
 * norm = +inf gives coef = 0, norm = NaN gives coef = NaN (the min keeps a NaN), and the update that multiplies by coef turns non-finite
 * accordingly; nothing is skipped and nothing is reported to the host.  partials, out: device fp32, out 16-byte aligned, not overlapping.
 * CD360_ERR_ARG for a null partials / out, count <= 0, a misaligned pointer, max_norm negative or NaN, out inside the partials. */
int cd360_grad_clip_f32(const void* partials, int64_t count, float max_norm, void* out, void* stream);

/* ---- AdamW with a live learning rate, clipping and EMA ------------------------------------------------------------------
 * cd360_adamw_bf16 of ../cd360_hip.h (torch.optim.AdamW semantics; torch/optim/adamw.py::_single_tensor_adamw in its order) with three
 * differences.  With coef and ema null and hyper holding the same values it writes the same bits.
 *  (1) lr and weight decay of tensor t are READ ON THE DEVICE from hyper[2 * row[t]] and hyper[2 * row[t] + 1]: hyper is a device fp32
 *      table [hyper_rows, 2], row[] a host int32 array.  A schedule (the reference's sgm/lr_scheduler.py through
 *      DiffusionEngine.configure_optimizers, sgm/models/diffusion.py:362-374) rewrites the table between replays of a captured step.
 *  (2) coef: device fp32 scalar or null.  Non-null: g <- g * *coef, one rounding, before anything else (pass &out[2] of
 *      cd360_grad_clip_f32): the scaling half of clip_grad_norm_ (_foreach_mul_ of the gradients) without its pass and without
 *      re-rounding the gradient to bf16.  The gradient tensors themselves are not modified.
 *  (3) ema: device fp32, flat and laid out like master, or null.  Non-null: after the master update of an element, with t = *step,
 *        d = min(ema_decay, (1 + t) / (10 + t))      omd = 1 - d      ema <- ema - omd * (ema - x_new)
 *      one fp32 rounding per operation; x_new is the fp32 master just written, not its bf16 rounding.  This is LitEma.forward with
 *      use_num_upates=True (sgm/modules/ema.py:33-52; DiffusionEngine.on_train_batch_end, diffusion.py), num_updates = the step count.
 * grads[t] / params[t]: bf16 device pointers to numel[t] values (parameter OVERWRITTEN with the rounded new master); begin[t] (a multiple
 * of 8) the tensor's offset in the flat fp32 buffers master / exp_avg / exp_avg_sq / ema (16-byte aligned); step: device fp32.
 * CD360_ERR_ARG for n outside 1 .. CD360_ADAMW_MAX_TENSORS, a null array / grads[t] / params[t] / master / exp_avg / exp_avg_sq / step /
 * hyper, numel[t] <= 0, begin[t] < 0, row[t] < 0 or >= hyper_rows, hyper_rows <= 0, a flat buffer not 16-byte aligned, step / hyper /
 * coef not 4-byte aligned, ema overlapping master, exp_avg or exp_avg_sq over the extent the tensors span; CD360_ERR_SHAPE for begin[t]
 * not a multiple of 8 or an odd grads[t] / params[t]. */
int cd360_adamw_live_bf16(int n, const void* const* grads, void* const* params, const int64_t* begin, const int64_t* numel, const int32_t* row,
                          const void* hyper, int hyper_rows, const void* coef, void* master, void* exp_avg, void* exp_avg_sq, void* ema,
                          float ema_decay, const void* step, float beta1, float beta2, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_OPTIM_H */
