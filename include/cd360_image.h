/* cd360_image.h -- C ABI of libcd360_hip.so, part 6: the joints between the sampler and the first stage (gfx950 / MI355X): the start
 * latent of a trajectory, the first stage's posterior sample, the decoder's front end and its uint8 image output.
 *
 * Same library, same conventions as the five older headers: device pointers owned by the caller, `stream` a hipStream_t passed as void*,
 * all work enqueued on it with no hidden synchronisation, nothing allocated, the environment never read, 0 on success and CD360_ERR_*
 * (< 0) on error.  Each entry point names the reference call site it replaces (paths relative to the reference tree).  The Python binding
 * types these entry points from cd360/_lib.py::IMAGE_SIGNATURES.
 *
 * The noise is the documented noise of cd360_stochastic.h -- Philox4x32-10 under key = the two halves of the seed, then Box-Muller, z_c the
 * noise of channel c of a pixel, one Philox call for a pixel's four latent channels -- with the LAST counter word, which a sampling step
 * leaves 0, naming the consumer: 1 = the start of a trajectory, 2 = the posterior sample.  So the start latent, the posterior sample and a
 * step's injected noise under one seed are three unrelated draws, and each is a pure function of its counter: the same bits on any batch
 * size, grid and rank layout.  One fp32 rounding per operation everywhere below, in the order written (no contraction).
 */
#ifndef CD360_IMAGE_H
#define CD360_IMAGE_H
#include <stdint.h>

#include "cd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- start latent -------------------------------------------------------------------------------------------------------
 * replaces `torch.randn` of the start noise (sample.py:290-292) and `x *= torch.sqrt(1.0 + sigmas[0] ** 2.0)` of prepare_sampling_loop
 * (sampling.py:50).  Per replay row smp in [0, bs) and pixel px in [0, HW):
 *
 *   counter = (px, 0, streams[smp], 1)                out[smp, c, px] = z_c * scale[0]
 *
 * out [bs, 4, HW] fp32; seed: device int64[1]; streams: device int32[bs], NULL = stream 0 for every row (all poses of a job share their
 * start noise, as sample.py:290-292 repeats one draw); scale: device fp32[1], computed by the caller as sampling.py:50 computes it.
 * CD360_ERR_ARG for a null out / seed / scale, bs <= 0, HW <= 0, HW > 2^32 (the pixel is one 32-bit counter word). */
int cd360_start_noise_f32(void* out, const void* seed, const void* streams, const void* scale, int bs, int64_t HW, void* stream);

/* ---- posterior sample ---------------------------------------------------------------------------------------------------
 * replaces, behind Encoder.forward, `self.quant_conv(h)` and `DiagonalGaussianDistribution(moments)` with `.sample()` (autoencoder.py:304-311
 * and :319-322, AutoencoderKLInferenceWrapper; distributions.py:24-41) and `z = self.scale_factor * z` of encode_first_stage
 * (diffusion.py:214-219).  moments [B, 8, HW] fp32 NCHW (what the Encoder returns: t_0..t_7 of a pixel); w [8][8] (output, input) and
 * bias [8] fp32: quant_conv's 1 x 1 weight and bias.  Per image b and pixel px:
 *
 *   m_o   = (((w[o][0] t_0 + w[o][1] t_1) + w[o][2] t_2) + ... + w[o][7] t_7) + bias[o]           o = 0..7
 *   mean  = m_0..3,   lv = min(max(m_4..7, -30), 20),   std = expf(0.5f * lv)
 *   out_c = (mean_c + std_c * z_c) * scale_factor       counter = (px, draw[0], streams[b], 2)
 *
 * draw: device int32[1], the training step or the call count -- successive samples of one image under one seed differ by it.
 * A NULL seed selects `.mode()`: out_c = mean_c * scale_factor; no noise is generated and streams / draw are not read.  A NaN logvar stays
 * a NaN, as under torch.clamp.  Only z_channels = 4 is served.  out [B, 4, HW] fp32, not overlapping moments.  CD360_ERR_ARG for a null
 * moments / w / bias / out, B <= 0, HW <= 0, HW > 2^32, out overlapping moments, and, with a seed, a null draw. */
int cd360_posterior_sample_f32(const void* moments, const void* w, const void* bias, const void* seed, const void* streams, const void* draw,
                               float scale_factor, void* out, int B, int64_t HW, void* stream);

/* ---- decoder front end --------------------------------------------------------------------------------------------------
 * replaces `z = 1.0 / self.scale_factor * z` of decode_first_stage (diffusion.py:208-212) and `self.post_quant_conv(z)` of
 * AutoencoderKL.decode (autoencoder.py:313-316; 4 -> 4, 1 x 1).  z [B, 4, HW] fp32; w [4][4] (output, input) and bias [4] fp32; inv_scale =
 * 1 / scale_factor as the caller rounds it to fp32.  Per pixel:
 *
 *   t_i   = z_i * inv_scale
 *   out_o = (((w[o][0] t_0 + w[o][1] t_1) + w[o][2] t_2) + w[o][3] t_3) + bias[o]
 *
 * out [B, 4, HW] fp32, not overlapping z.  CD360_ERR_ARG for a null z / w / bias / out, B <= 0, HW <= 0, out overlapping z. */
int cd360_post_quant_f32(const void* z, const void* w, const void* bias, float inv_scale, void* out, int B, int64_t HW, void* stream);

/* ---- image out ----------------------------------------------------------------------------------------------------------
 * replaces Decoder.conv_out (model.py:699-701, :733) followed by `(torch.clip(x.permute(1, 2, 0) * 0.5 + 0.5, 0, 1.).cpu().numpy() * 255)
 * .astype(np.uint8)` (sample.py:346).  x, w, bias, B, H, W, Cin, Cout and their errors are those of the fp32 output convolution
 * cd360_vae_conv_out_bf16 of cd360_hip.h (x [B, H W, Cin] bf16 channels-last, w [9][Cin][4] fp32, Cin % 64 == 0, Cout in 1..4), and the
 * fp32 value acc + bias is the very value that entry point writes, bit for bit (one accumulation function serves both).  Per value v:
 *
 *   t = v * 0.5f + 0.5f    (two roundings)       t = min(max(t, 0), 1)       out = (uint8) truncate(t * 255.f)
 *
 * out [B, H, W, Cout] uint8, channels last: what Image.fromarray takes.  A NaN v writes 0: torch.clip hands a NaN on and numpy's cast of a
 * NaN to uint8 is undefined, so the reference fixes no value there.  CD360_ERR_ARG for a null x / w / out or a misaligned x / w,
 * CD360_ERR_SHAPE for Cin % 64, Cout outside 1..4, B > 65535. */
int cd360_vae_conv_out_u8(const void* x, const void* w, const void* bias, void* out, int B, int H, int W, int Cin, int Cout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CD360_IMAGE_H */
