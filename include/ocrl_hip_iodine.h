/* C ABI of the IODINE kernels and of the broadcast decoder's own kernels in libocrl_hip.so (gfx950), one launcher (or one short
 * launcher sequence) per entry: what ocrl_iodine_forward / ocrl_iodine_backward and the Slot-Attention configuration of SLATE run as
 * part of a model, reachable on caller-owned tensors so that each kernel can be compared with a reference of its own operation.  An
 * eighth header beside ocrl_hip.h, ocrl_hip_dqn.h, ocrl_hip_rollout.h, ocrl_hip_replay.h, ocrl_hip_c51.h, ocrl_hip_noisy.h and
 * ocrl_hip_classifier.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads them all).  Conventions: every entry is stateless
 * and takes device pointers (fp32, dense unless a leading dimension is an argument, 16-byte aligned base pointers), an `int` entry returns
 * 0 on success and the message of a failure is ocrl_last_error(), every argument is checked before any launch, work is enqueued on
 * `stream` (a hipStream_t) with no host synchronisation.  Layouts are the kernels': activations NHWC / [rows, features], obs NCHW.
 *
 * ocrl_iodine_elbo: the mixture likelihood of one refinement iteration on out4 [B*K][S*S][4] = (rgb means, mask logit) and obs [B][3][S][S].
 *   part[0] += sum of the pixel log-likelihoods, part[1] += sum of (obs - recon)^2  (accumulated: the caller zeroes them).
 *   enc [B*K][S*S][17] (nullable): the refinement encoding; with `layer_norm` channels 9..14 are normalised (needs st2).
 *   st1 [B*K][4] (written when enc is given, required then): sums of the four normalised groups before normalisation;
 *   st2 [B*K][4] (written when enc is given and layer_norm, required then): their sums of squared deviations.
 *   dout4 [B*K][S*S][4] (nullable) = d(B * elbo) / d out4;  masks [B*K][S*S], recon [B][3][S][S], recons_masked [B*K][3][S][S] (each
 *   nullable; recon and recons_masked clamped to [0, 1]).  1 <= K <= 16 and S % 16 == 0.  ws: ocrl_iodine_elbo_ws_floats(B, K, S) floats.
 * ocrl_iodine_elbo_bwd: dout4 = d(cw * sum of pixel log-likelihoods + <enc, denc>) / d out4 with the encoding's gradient and likelihood
 *   channels held constant; denc [B*K][S*S][17] nullable.
 * ocrl_iodine_sample: slots = mu + exp(ls) * eps, eps_out = eps, kl_out[0] = sum(-ls + (exp(2 ls) + mu^2) / 2 - 1/2) (written), n
 *   elements; eps = noise, or (noise NULL) Box-Muller draws of the counter RNG at (seed, site).  ws: ocrl_iodine_sample_ws_floats(n).
 * ocrl_iodine_latent: latent[row][0..4L) = (mu, ls, LN(ds - beta mu), LN(ds sigma eps - beta (sigma^2 - 1))) with row stride ld >= 4L
 *   (columns past 4L are not touched); LN: mean and unbiased std over L, eps on the std, or the identity without layer_norm.  L >= 2.
 * ocrl_iodine_post_grad: gmu += ds + kw mu (+ dlat[row][0..L)), gls += ds sigma eps + kw (sigma^2 - 1) (+ dlat[row][L..2L)); dlat
 *   (row stride ldl) nullable.
 * ocrl_iodine_im2col / ocrl_iodine_col2im: the stride-2, pad-1 3x3 window of x [Bn][Hi][Wi][C] as rows col[(b, oy, ox)][tap * C + c]
 *   of stride ldc >= 9 C (zero padded), Ho = (Hi - 1) / 2 + 1; and its transpose times elu'(act) (act = the ELU output, nullable).
 *   force_generic != 0 picks the 64-bit-index kernel whatever the launcher's own dispatch would take.
 * ocrl_iodine_refw_pack: backward == 0: src = W [64][C][3][3] -> dst = Wp [64][ldc] (column tap * C + c, zero padded);
 *   backward != 0: src = dWp [64][ldc] -> dst = dW [64][C][3][3].
 * ocrl_iodine_pool: dpool NULL: out [BK][64] = mean over the n pixels of r [BK][n][64]; dpool [BK][64] given: out [BK][n][64] =
 *   dpool / n * elu'(r).
 * ocrl_iodine_elu2: dy NULL: y = elu(elu(a)); dy given: y = dy * elu'(elu(a)) * elu'(a).  rows x F elements, row strides lda, ldy, lddy.
 * ocrl_iodine_lstm: backward == 0: gates [rows][4H] (i, f, g, o pre-activations), c0 -> acts [rows][4H], c1, h1.  backward != 0: acts,
 *   c0, c1, dh1, dc1 (each of the two nullable = zero) -> dgates [rows][4H] (pre-activation), dc0.
 * ocrl_bcdec_c4: the 3x3 64 -> 4 output convolution with W [co_n][64][3][3], co_n <= 4 (missing output channels have zero weights).
 *   mode 0: Y [Bn][S][S][4] = conv(X [Bn][S][S][64]) + bias[0..4).  mode 1: Y [Bn][S][S][64] = conv^T(X [Bn][S][S][4]) gated by the
 *   derivative of the saved activation act [Bn][S][S][64]: ReLU' (elu == 0) or ELU' (elu != 0).  ws: ocrl_bcdec_c4_ws_floats() floats
 *   (the packed weights).
 * ocrl_bcdec_c4_wgrad: per-block partials part[nb][4][64][9] of dW = sum over pixels of dY [.,4] x window(X [.,64]), nb =
 *   ocrl_bcdec_c4_wgrad_blocks(Bn, S) (0 for a refused shape); the caller sums the blocks.  form: 0 = as the process switch
 *   OCRL_BC_WGRAD decides, 1 = the VALU kernel, 2 = the MFMA kernel.
 * ocrl_bcdec_mix: recon [B][S][S][4] = sum_k softmax_k(logit) rgb_k (channel 3 = 0), loss_out[0] = sum (obs - recon)^2 / B over the C <= 3
 *   channels of obs [B][C][S][S], dout4 = its gradient; recon and dout4 nullable.  1 <= K <= 16.  ws: ocrl_bcdec_mix_ws_floats() floats.
 * ocrl_bcdec_compose / _bwd: Wc[tap][co][0..3] = sum_ci W1[co][ci][tap] Wpos[ci][j], Wc[tap][co][4] = sum_ci W1[co][ci][tap] bpos[ci],
 *   W1r[tap][co][ci] = W1[co][ci][tap] for W1 [64][D][5][5], Wpos [D][4], bpos [D]; and the gradients dW1, dWpos, dbpos from dWc, dW1r. */
#ifndef OCRL_HIP_IODINE_H
#define OCRL_HIP_IODINE_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t ocrl_iodine_elbo_ws_floats(int B, int K, int S);
int ocrl_iodine_elbo(const float* out4, const float* obs, int B, int K, int S, float sigma, int layer_norm, float* enc, float* st1, float* st2,
                     float* dout4, float* part, float* masks, float* recon, float* recons_masked, float* ws, size_t ws_floats, void* stream);
int ocrl_iodine_elbo_bwd(const float* out4, const float* obs, const float* denc, int B, int K, int S, float sigma, float cw, float* dout4,
                         void* stream);
size_t ocrl_iodine_sample_ws_floats(long long n);
int ocrl_iodine_sample(const float* mu, const float* ls, const float* noise /* NULL = draw */, float* eps_out, float* slots, float* kl_out,
                       long long n, unsigned long long seed, unsigned site, float* ws, size_t ws_floats, void* stream);
int ocrl_iodine_latent(const float* mu, const float* ls, const float* eps, const float* ds, float* latent, long long BK, int L, float beta,
                       int layer_norm, int ld, void* stream);
int ocrl_iodine_post_grad(const float* mu, const float* ls, const float* eps, const float* ds, const float* dlat, int ldl, float kw, float* gmu,
                          float* gls, long long BK, int L, void* stream);
int ocrl_iodine_im2col(const float* x, float* col, long long Bn, int C, int Hi, int Wi, int ldc, int force_generic, void* stream);
int ocrl_iodine_col2im(const float* dcol, const float* act, float* dx, long long Bn, int C, int Hi, int Wi, int ldc, int force_generic,
                       void* stream);
int ocrl_iodine_refw_pack(const float* src, float* dst, int C, int ldc, int backward, void* stream);
int ocrl_iodine_pool(const float* r, const float* dpool /* NULL = forward */, float* out, long long BK, int n, void* stream);
int ocrl_iodine_elu2(const float* a, int lda, float* y, int ldy, long long rows, int F, const float* dy /* NULL = forward */, int lddy,
                     void* stream);
int ocrl_iodine_lstm(const float* gates, const float* c0, float* acts, float* c1, float* h1, const float* dh1, const float* dc1, float* dgates,
                     float* dc0, long long rows, int H, int backward, void* stream);
size_t ocrl_bcdec_c4_ws_floats(void);
int ocrl_bcdec_c4(const float* W, int co_n, const float* bias, const float* X, const float* act, float* Y, int Bn, int S, int mode, int elu,
                  float* ws, size_t ws_floats, void* stream);
int ocrl_bcdec_c4_wgrad_blocks(int Bn, int S);
int ocrl_bcdec_c4_wgrad(const float* X, const float* dY, float* part, size_t part_floats, int Bn, int S, int form, void* stream);
size_t ocrl_bcdec_mix_ws_floats(void);
int ocrl_bcdec_mix(const float* out4, const float* obs, float* recon, float* dout4, float* loss_out, int B, int K, int S, int C, float* ws,
                   size_t ws_floats, void* stream);
int ocrl_bcdec_compose(const float* W1, const float* Wpos, const float* bpos, float* Wc, float* W1r, int D, void* stream);
int ocrl_bcdec_compose_bwd(const float* W1, const float* Wpos, const float* bpos, const float* dWc, const float* dW1r, float* dW1, float* dWpos,
                           float* dbpos, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif
