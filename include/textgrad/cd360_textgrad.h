/* cd360_textgrad.h -- C ABI of libcd360_textgrad.so: the backward of the two prompt encoders (CLIP-L and the OpenCLIP-bigG text tower) with
 * respect to the modifier-token rows of their token tables, beside the Linear layers and LayerNorms: the backward of the causal
 * self-attention, of the MLP activation and of the EOT pooling, and the reduction of the embedding gradient onto the modifier rows
 * (gfx950 / MI355X).  Custom Diffusion trains those rows and nothing else of the towers (sgm/models/diffusion.py:342-355,
 * sgm/modules/encoders/modules.py:499-511, 724-730 of the reference), so no weight gradient exists here.
 *
 * A fifth, small library beside libcd360_hip.so, libcd360_edit.so, libcd360_optim.so and libcd360_text.so, whose headers and exports are
 * closed.  Same conventions as ../text/cd360_text.h: device pointers owned by the caller, `stream` a hipStream_t passed as void*, all work
 * enqueued on it with no hidden synchronisation, nothing allocated, the environment never read, 0 on success and CD360_ERR_* (< 0) on
 * error, and nothing is launched when an error is returned.  Strides are in ELEMENTS.  No kernel uses a floating-point atomic: every sum
 * has one owner and a fixed order that does not depend on the grid, so every result is reproducible bit for bit.  The data gradients of
 * the Linear layers (dX = dY W) run on the GEMM entry of ../cd360_hip.h, both LayerNorm backwards on its add-LayerNorm backward entry;
 * nothing of those is restated here.  The Python binding types these entry points from cd360/_textgrad.py::TEXTGRAD_SIGNATURES.
 */
#ifndef CD360_TEXTGRAD_H
#define CD360_TEXTGRAD_H
#include <stdint.h>

#include "../cd360_hip.h"
#include "../text/cd360_text.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- backward of the causal self-attention, head dim 64 -----------------------------------------------------------------------
 * The backward of the causal attention entry of ../text/cd360_text.h: B * H independent problems of N tokens,
 * 1 <= N <= CD360_TEXT_MAX_TOKENS.  With s[i][j] = scale * q[i] . k[j] and P = softmax over the visible keys j <= i (fp32, recomputed
 * from q and k: at 77 tokens the recomputation is cheaper than another saved tensor, and the forward entry needs no change),
 *
 *   dP[i][j] = dO[i] . v[j]          D[i] = sum_{j <= i} P[i][j] dP[i][j]          dS[i][j] = P[i][j] (dP[i][j] - D[i])
 *   dq[i] = scale * sum_{j <= i} dS[i][j] k[j]       dk[j] = scale * sum_{i >= j} dS[i][j] q[i]       dv[j] = sum_{i >= j} P[i][j] dO[i]
 *
 * all in fp32, one rounding to bf16 per output element.  A masked pair (j > i) is never touched and contributes exactly nothing:
 * dq[0] is exactly 0 (row 0 has one key, P = 1, dS = P (dP - dP)), dq[: i + 1] does not depend on the keys and values behind i, and
 * dk[j :], dv[j :] do not depend on the queries and output gradients before j.  Rows at index >= N are neither read nor written.
 * Strided form, that of the forward entry: q[b][h][n][d] at q + b*qs[0] + h*qs[1] + n*qs[2] + d (element strides), k, v, d_o, dq, dk, dv
 * likewise; every stride a multiple of 8, every pointer 16-byte aligned.  With these strides the kernel consumes the three column slices
 * of the saved merged q|k|v projection [B * N, 3 * H * 64] in place and writes dq | dk | dv as the three column slices of one buffer of
 * the same shape.  No output may overlap an input or another output.
 * One workgroup per problem; q, k, v and dO (bf16, 4 x 16 KiB at N = 128) go to LDS once.  Four lanes share a row, 16 of the 64 channels
 * each.  Phase 1, a quad per QUERY row: one walk over the keys 0 .. i for the row maximum, the row sum and D (online, rescaled like the
 * forward's accumulator), a second walk for dq; the three row scalars go to LDS.  Phase 2, a quad per KEY row: one walk over the queries
 * j .. N - 1 in rising order for dk and dv, with P rebuilt from the row scalars by the same operations, so both phases see the same bits.
 * All five contractions run on the VECTOR pipe, not on MFMA, for the forward's reason: at N = 77 the causal triangle of one head is
 * 0.4 MFLOP per contraction, the launch is bound by its latency, and a 32 x 32 MFMA tile would spend over half of its work above the
 * diagonal -- and a fixed per-row summation order falls out of this layout with no atomics and no cross-workgroup reduction.
 * CD360_ERR_ARG for a null q / k / v / d_o / dq / dk / dv / stride array, B or H <= 0, a misaligned pointer, a scale that is not finite;
 * CD360_ERR_SHAPE for N outside 1 .. CD360_TEXT_MAX_TOKENS, a stride that is no multiple of 8, a negative stride, or B * H beyond
 * 2^31 - 1. */
int cd360_textgrad_causal_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* d_o, void* dq, void* dk, void* dv, int B, int H,
                                        int N, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                        const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides,
                                        const int64_t* dv_strides, float scale, void* stream);

/* ---- backward of the MLP activation -------------------------------------------------------------------------------------------
 * dx = dy * f'(x), x the saved PRE-activation, for the two kinds of the forward's activation entry:
 *   kind 0   QuickGELU:   f'(x) = s (1 + 1.702 x (1 - s)),  s = sigmoid(1.702 x)
 *   kind 1   exact GELU:  f'(x) = Phi(x) + x phi(x),  Phi(x) = erfc(-x / sqrt 2) / 2 (no cancellation in the negative tail), phi the density
 * x [rows, n] bf16 with row stride ld_x, dy likewise with ld_dy -> dx [rows, n] bf16 with row stride ld_dx (dx == dy is allowed:
 * elementwise; dx must not overlap x).  Computed in fp32, one rounding at the store; 16-byte loads and stores.  For large |x| the
 * derivative goes to 0 or 1 and stays finite.  n % 8 == 0, every stride % 8 == 0 and >= n; 16-byte aligned pointers.
 * CD360_ERR_ARG for a null x / dy / dx, rows or n <= 0, a misaligned pointer, kind outside {0, 1}; CD360_ERR_SHAPE for n or a stride that
 * is no multiple of 8 or a stride below n. */
int cd360_textgrad_act_bwd_bf16(const void* x, const void* dy, void* dx, int64_t rows, int n, int64_t ld_x, int64_t ld_dy, int64_t ld_dx,
                                int kind, void* stream);

/* ---- backward of the EOT pooling ----------------------------------------------------------------------------------------------
 * The backward of the pooling entry of ../text/cd360_text.h: the gradient of the pooled row goes to the row it was gathered from.
 *   d_pooled bf16 [B, D], row stride ld_dp          ids int64 [B, N] contiguous          dx bf16 [B * N, D], row stride ld_dx, IN / OUT
 *   dx[b * N + argmax_n ids[b, n]] = bf16(fp32(dx[...]) + fp32(d_pooled[b])), the LOWEST n among equal maxima; every other row of dx is
 *   left as it is.  The argmax runs on the device, by the forward's rule.  One row per prompt: no two writers share a row.
 * D % 8 == 0, strides % 8 == 0 and >= D; d_pooled and dx 16-byte, ids 8-byte aligned.
 * CD360_ERR_ARG for a null d_pooled / ids / dx, B, N or D <= 0, a misaligned pointer; CD360_ERR_SHAPE for D or a stride that is no
 * multiple of 8, a stride below D, or B * N beyond 2^31 - 1. */
int cd360_textgrad_eot_scatter_bf16(const void* d_pooled, const void* ids, void* dx, int B, int N, int D, int64_t ld_dp, int64_t ld_dx,
                                    void* stream);

/* ---- gradient of the modifier rows of the token table ---------------------------------------------------------------------------
 * The reference lets the gradient of the embedding through at the modifier positions only ((1 - indices) * x.detach() + indices * x):
 * no other token row and no position row receives anything.  For each of the k modifier ids, 1 <= k <= CD360_TEXTGRAD_MAX_MODIFIERS,
 *   out[m] = sum over the positions (b, n) with ids[b, n] == mod_ids[m], in rising (b, n) order, of fp32(d_x0[b * N + n])
 *   d_x0 bf16 [B * N, D], row stride ld_dx     ids int64 [B, N] contiguous     mod_ids: a HOST array of k ids     out fp32 [k, D] contiguous
 * out is WRITTEN, not accumulated; a modifier that occurs nowhere gives a row of zeros.  One thread owns eight columns of one modifier and
 * walks all B * N ids: fp32 adds in one fixed order whatever B, no atomics.
 * D % 8 == 0, ld_dx % 8 == 0 and >= D; d_x0 and out 16-byte, ids 8-byte aligned.
 * CD360_ERR_ARG for a null d_x0 / ids / mod_ids / out, B, N or D <= 0, a misaligned pointer; CD360_ERR_SHAPE for k outside
 * 1 .. CD360_TEXTGRAD_MAX_MODIFIERS, D or ld_dx no multiple of 8, ld_dx below D, or B * N beyond 2^31 - 1. */
#define CD360_TEXTGRAD_MAX_MODIFIERS 3
int cd360_textgrad_token_rows_f32(const void* d_x0, const void* ids, const int64_t* mod_ids, void* out, int B, int N, int D, int k, int64_t ld_dx,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_TEXTGRAD_H */
