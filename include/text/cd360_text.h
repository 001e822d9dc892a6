/* cd360_text.h -- C ABI of libcd360_text.so: what the two prompt encoders of the conditioner (CLIP-L and the OpenCLIP-bigG text tower,
 * sgm/modules/encoders/modules.py of the reference) need beside the Linear layers: the token + position embedding, the causal
 * self-attention, the MLP activation and the EOT pooling (gfx950 / MI355X).  Forward only.
 *
 * A fourth, small library beside libcd360_hip.so, libcd360_edit.so and libcd360_optim.so, whose headers and exports are closed.  Same
 * conventions as ../cd360_hip.h: device pointers owned by the caller, `stream` a hipStream_t passed as void*, all work enqueued on it
 * with no hidden synchronisation, nothing allocated, the environment never read, 0 on success and CD360_ERR_* (< 0) on error, and nothing
 * is launched when an error is returned.  Strides are in ELEMENTS.  The Linear layers of the towers (q|k|v with the first LayerNorm
 * folded, out-proj, FC1 with the second LayerNorm folded, FC2, the text projection) run on the GEMM entry of ../cd360_hip.h, the final
 * LayerNorms on its add-LayerNorm entry; nothing of those is restated here.  The Python binding types these entry points from
 * cd360/_text.py::TEXT_SIGNATURES.
 */
#ifndef CD360_TEXT_H
#define CD360_TEXT_H
#include <stdint.h>

#include "../cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The causal attention holds the keys and values of one (batch, head) problem in LDS: at most this many tokens. */
#define CD360_TEXT_MAX_TOKENS 128

/* ---- token + position embedding -----------------------------------------------------------------------------------------------
 * Replaces text_model.embeddings(input_ids=tokens) of HF's CLIPTextModel (sgm/modules/encoders/modules.py:509) and
 * model.token_embedding(text) + model.positional_embedding of open_clip (modules.py:722-732).
 *   ids   int64 [B, N] contiguous          tok  bf16 [V, D] contiguous          pos  bf16 [>= N, D] contiguous
 *   out   bf16 [B * N, D], row stride ld_out:   out[b * N + n] = bf16(fp32(tok[ids[b, n]]) + fp32(pos[n])), ONE rounding (to nearest even)
 *   stats fp32 [B * N, 1, 2] | NULL: (sum, sum of squares) of the STORED (rounded) row, fp32 -- the layout the row-statistics entry of
 *         ../cd360_hip.h writes, so the LayerNorm fold of the first q|k|v GEMM needs no pass of its own
 * An id outside [0, V) writes a row of zeros (statistics 0, 0) and reads neither table: nothing is read out of bounds.  (The Python
 * caller checks the ids on the host, where they come from, and raises before the launch.)
 * One wave per row, 16-byte accesses.  D % 8 == 0, ld_out % 8 == 0, ld_out >= D; tok, pos, out 16-byte aligned, ids and stats 8-byte.
 * CD360_ERR_ARG for a null ids / tok / pos / out, B, N, V or D <= 0, a misaligned pointer; CD360_ERR_SHAPE for D % 8, ld_out % 8,
 * ld_out < D, or B * N beyond 2^31 - 1. */
int cd360_text_embed_bf16(const void* ids, const void* tok, const void* pos, void* out, int B, int N, int V, int D, int64_t ld_out, void* stats,
                          void* stream);

/* ---- causal self-attention, head dim 64 ---------------------------------------------------------------------------------------
 * Replaces the attention inside HF's CLIPAttention under the additive mask of modules.py:451-458 (finfo.min above the diagonal) and
 * nn.MultiheadAttention under model.attn_mask of open_clip (-inf above the diagonal; modules.py:734): B * H independent problems of
 * Nq = Nk = N tokens, 1 <= N <= CD360_TEXT_MAX_TOKENS,
 *
 *   o[i] = sum_{j <= i} softmax_j(scale * q[i] . k[j]) v[j]
 *
 * Key j is visible to query i iff j <= i; a masked probability is exactly 0 (the masked keys are never touched by the row -- after the
 * fp32 softmax both references' masks give the same), so row 0 is v[0] bit for bit.  Keys and values at index >= N are never read.
 * Strided form, exactly that of the bf16 attention entry of ../cd360_hip.h: q[b][h][n][d] at q + b*qs[0] + h*qs[1] + n*qs[2] + d
 * (element strides, multiples of 8), k and v likewise (v row-major), o like q (strides multiples of 4); q, k, v 16-byte and o 8-byte
 * aligned.  With these strides the kernel consumes the three column slices of one merged q|k|v projection output [B * N, 3 * H * 64] in
 * place and writes [B * N, H * 64].  o must not overlap q, k or v.
 * One workgroup per problem: K and V (bf16, 2 x 16 KiB at N = 128) go to LDS once; four lanes share a query row, 16 of the 64 channels
 * each, and walk the keys 0 .. i with an online softmax; scores, probabilities and the output accumulate in fp32, one division by the
 * row sum and one rounding to bf16 at the end.  Both contractions run on the VECTOR pipe, not on MFMA: at N = 77 the causal triangle of
 * one head is 0.4 MFLOP, the launch is bound by its latency, and a 32 x 32 MFMA tile would spend over half of its work above the diagonal.
 * CD360_ERR_ARG for a null q / k / v / o / stride array, B or H <= 0, a misaligned pointer, a scale that is not finite;
 * CD360_ERR_SHAPE for N outside 1 .. CD360_TEXT_MAX_TOKENS, a q / k / v stride that is no multiple of 8, an o stride no multiple of 4,
 * a negative stride, or B * H beyond 2^31 - 1. */
int cd360_text_causal_attn_bf16(const void* q, const void* k, const void* v, void* o, int B, int H, int N, const int64_t* q_strides,
                                const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides, float scale, void* stream);

/* ---- MLP activation -----------------------------------------------------------------------------------------------------------
 * Replaces the activation between the two MLP Linears:
 *   kind 0   QuickGELU, x * sigmoid(1.702 x)            -- HF CLIP-L's hidden_act "quick_gelu" (CLIPMLP.activation_fn)
 *   kind 1   exact GELU, 0.5 x (1 + erf(x / sqrt 2))    -- open_clip's nn.GELU in the bigG text tower's ResidualAttentionBlock.mlp
 * in [rows, n] bf16 with row stride ld_in -> out [rows, n] bf16 with row stride ld_out (out == in is allowed: elementwise).  Computed in
 * fp32, one rounding at the store; 16-byte loads and stores.  n % 8 == 0, ld_in % 8 == 0, ld_out % 8 == 0, both >= n; 16-byte aligned.
 * CD360_ERR_ARG for a null in / out, rows or n <= 0, a misaligned pointer, kind outside {0, 1}; CD360_ERR_SHAPE for n or a stride that is
 * no multiple of 8 or a stride below n. */
int cd360_text_act_bf16(const void* in, void* out, int64_t rows, int n, int64_t ld_in, int64_t ld_out, int kind, void* stream);

/* ---- EOT pooling --------------------------------------------------------------------------------------------------------------
 * Replaces x[torch.arange(x.shape[0]), text.argmax(dim=-1)] of FrozenOpenCLIPEmbedder.pool (modules.py:747-753); the projection behind
 * it is a GEMM call on the transposed text_projection.
 *   x bf16 [B * N, D], row stride ld_x          ids int64 [B, N] contiguous          out bf16 [B, D], row stride ld_out
 *   out[b] = x[b * N + argmax_n ids[b, n]], the LOWEST n among equal maxima (torch.argmax's choice); the argmax runs on the device.
 * D % 8 == 0, strides % 8 == 0 and >= D; x and out 16-byte, ids 8-byte aligned.
 * CD360_ERR_ARG for a null x / ids / out, B, N or D <= 0, a misaligned pointer; CD360_ERR_SHAPE for D or a stride that is no multiple of
 * 8, a stride below D, or B * N beyond 2^31 - 1. */
int cd360_text_eot_pool_bf16(const void* x, const void* ids, void* out, int B, int N, int D, int64_t ld_x, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_TEXT_H */
