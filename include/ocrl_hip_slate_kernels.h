/* C ABI of the SLATE token-path and helper kernels in libocrl_hip.so (gfx950), one launcher of elementwise.hip per entry: what every SLATE
 * step (and, through the column sums, IODINE, the VAE, the pooling heads and slot attention) runs as part of a model, reachable on
 * caller-owned tensors so that each kernel can be compared with a reference of its own operation.  A tenth header beside ocrl_hip.h,
 * ocrl_hip_dqn.h, ocrl_hip_rollout.h, ocrl_hip_replay.h, ocrl_hip_c51.h, ocrl_hip_noisy.h, ocrl_hip_classifier.h, ocrl_hip_iodine.h and
 * ocrl_hip_qr.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads them all).  Conventions: every entry is stateless and takes
 * device pointers (fp32, or int32 for tokens; dense unless a leading dimension is an argument), an `int` entry returns 0 on success and the
 * message of a failure is ocrl_last_error(), every argument is checked before any launch (null pointers that are not marked nullable, sizes
 * below 1, the limits named below, 16-byte alignment of every base pointer a kernel reads or writes as float4), work is enqueued on
 * `stream` (a hipStream_t) with no host synchronisation.  Token values are device data and cannot be checked: they must lie in [0, V).
 *
 * ocrl_tp_gumbel_softmax: per row of V logits, logp = log_softmax(raw), g = -log(e + tiny): z = softmax((logp + g1) / tau), tokens[row] =
 *   first argmax of logp + g2, zst (nullable) = (onehot(first argmax z) - z) + z.  e1, e2 [R][V] ~ Exp(1), both given or both NULL (drawn
 *   from the counter RNG at `seed`).  V % 256 == 0, V <= 4096, tau > 0.
 * ocrl_tp_softmax_bwd_rows: in place d = z * (d - sum_v z d) * scale per row.  V % 256 == 0, V <= 4096.
 * ocrl_tp_softmax_stat_combine: stat [R][nseg][2] = per 64-column segment (max, sum exp(x - max)), an empty segment is (-inf, 0) ->
 *   lse [R].  hstat [R][nseg], hidx [R][nseg] (segment maximum and its column; both or neither, and tokens with them) -> tokens[row] =
 *   the column of the greatest segment maximum, the lower column on a tie; without them tokens is not touched.  pred [R][ldp] (nullable;
 *   needs tok [R] with values < V, out and ws): out[0] = scale * sum_row (lse[row] - pred[row][tok[row]]); without pred neither out nor
 *   ws is touched.  1 <= nseg <= 64, 1 <= V <= ldp, ws_floats >= ceil(R / 16).
 * ocrl_tp_exp_rows: z[row][v] = exp(y[row][v] - lse[row]).  V % 4 == 0.
 * ocrl_tp_rowdot_bias64: out[row] = sum_c g[row][c] * (act[row][c] - bias[c]) over 64 columns.
 * ocrl_tp_embed_fwd: out [B][T][d] = dropout((t == 0 ? bos : dict[tokens[b][t - 1]]) + pe[t]), tokens [B][T] (token (b, T - 1) is not
 *   read), dict [V][d], pe [T][d]; the keep mask is that of site 1 over a [B][T + 1][d] tensor.  d % 4 == 0, 0 <= p < 1.
 * ocrl_tp_embed_bwd: g [B][T][d] <- g * mask / (1 - p) in place (p > 0), then ddict [V][d] = sum of the rows (b, t > 0) of g whose token
 *   (b, t - 1) is the row's index; absent tokens get 0; every element of ddict is written.  d % 4 == 0, d <= 1024, V + 1 <= 16384,
 *   ws_floats >= ocrl_tp_embed_bwd_ws_floats(B * T, V, d) (0 for a refused shape).
 * ocrl_tp_embed_step: out [B][d] = (t == 0 ? bos : dict[tokens[b][t - 1]]) + pe[t].  0 <= t < T.
 * ocrl_tp_dropout_apply: y = x * keep / (1 - p) over n elements at (seed, site).  n % 4 == 0, 0 <= p < 1.
 * ocrl_tp_dropout_mask: y[i] = 1 where element i of the site is kept, else 0.
 * ocrl_tp_colsum: out[c] (+= when accumulate) scale * sum_r X[r][c] for X [R][F] of row stride ld >= F; ws_floats floats of scratch at a
 *   16-byte aligned ws (a scratch too small for the smallest chunking is refused with "workspace too small").
 * ocrl_tp_mse: out[0] = sum (recon - obs)^2 / B over obs [B][C][H][W] and recon [B][H][W][4]; drecon [B][H][W][4] (nullable) = 2 (recon -
 *   obs) / B, channels >= C zero.  1 <= C <= 4, ws_floats >= 1024.
 * ocrl_tp_pixel_shuffle: forward != 0: out [B][2h][2w][Cout] from in [B][h][w][4 Cout], out[b][2y + i][2x + j][c] = in[b][y][x][4c + 2i +
 *   j]; forward == 0 the inverse map, times (mask > 0) for a mask [B][h][w][4 Cout] (nullable).
 * ocrl_tp_nchw_to_nhwc8: out [B][H][W][8] from in [B][C][H][W], channels >= C zero.  C <= 8.
 * ocrl_tp_patchify4: out [B (S/4)^2][16 C], column c * 16 + ky * 4 + kx, from in [B][C][S][S].  S % 4 == 0.
 * ocrl_tp_pad_cols: out[r][c] = c < C ? in[r][c] : 0 for c < Cout, row strides ldi >= C and ldo >= Cout.
 * ocrl_tp_im2col5: col[(b, y, x)][tap * C + c] = x8[b][y + tap / 5 - 2][x + tap % 5 - 2][c], zero outside the image and in columns
 *   25 C .. ldc, x8 [B][H][W][8].  ldc >= 25 C, C <= 8.
 * ocrl_tp_unpack5: dW [64][C][5][5] from dWp [64][ldc], dW[co][c][tap] = dWp[co][tap * C + c].  ldc >= 25 C, C <= 8.
 * ocrl_tp_posmap: out [S][S][C] = sum_j grid[j][y][x] Wpos[c][j] + bpos[c], grid = (north, south, west, east) ramps; ocrl_tp_posgrid:
 *   out [S * S][4] = the grid itself.
 * ocrl_tp_onehot: z [rows][V] = (v == tokens[row]).
 * ocrl_tp_slot_init: slots0 [BK][D] = mu[c] + exp(logsig[c]) * eps, eps = noise [BK][D], or (noise NULL) N(0, 1) draws of the counter RNG
 *   at `seed`.  ocrl_tp_slot_init_bwd: dmu[c] = sum_r d[r][c], dlogsig[c] = exp(logsig[c]) sum_r d[r][c] eps[r][c], the same eps.
 * ocrl_tp_argmax_pos: tokens[b * T + t] = first argmax over V of row b * T + t of pred [B * T][V], or (dense_rows != 0) of row b of pred
 *   [B][V]; no other token is written.  0 <= t < T.
 * ocrl_tp_decode_attn: out [B][d] = causal soft-max attention of query row t over the keys / values 0 .. t of qkv [B * T][ld] = (q | k | v),
 *   h heads.  d % h == 0, (d / h) % 4 == 0, d / h <= 64, 0 <= t < T, ld % 4 == 0, ld >= 3 d, T within the 64 KB score buffer. */
#ifndef OCRL_HIP_SLATE_KERNELS_H
#define OCRL_HIP_SLATE_KERNELS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int ocrl_tp_gumbel_softmax(const float* raw, const float* e1, const float* e2, float* z, int* tokens, float* zst /* nullable */, long long R,
                           int V, float tau, unsigned long long seed, void* stream);
int ocrl_tp_softmax_bwd_rows(const float* z, float* d, long long R, int V, float scale, void* stream);
int ocrl_tp_softmax_stat_combine(const float* stat, int nseg, long long R, float* lse, const float* hstat, const int* hidx, int* tokens,
                                 const float* pred, int ldp, int V, const int* tok, float* out, float scale, float* ws, size_t ws_floats,
                                 void* stream);
int ocrl_tp_exp_rows(const float* y, const float* lse, float* z, long long R, int V, void* stream);
int ocrl_tp_rowdot_bias64(const float* g, const float* act, const float* bias, long long R, float* out, void* stream);
int ocrl_tp_embed_fwd(const int* tokens, const float* dict, const float* bos, const float* pe, float* out, int B, int T, int d, float p,
                      unsigned long long seed, void* stream);
size_t ocrl_tp_embed_bwd_ws_floats(long long BT, int V, int d);
int ocrl_tp_embed_bwd(float* g, const int* tokens, float* ddict, int B, int T, int V, int d, float p, unsigned long long seed, float* ws,
                      size_t ws_floats, void* stream);
int ocrl_tp_embed_step(const int* tokens, const float* dict, const float* bos, const float* pe, float* out, int B, int T, int d, int t,
                       void* stream);
int ocrl_tp_dropout_apply(const float* x, float* y, long long n, float p, unsigned long long seed, unsigned site, void* stream);
int ocrl_tp_dropout_mask(float* y, unsigned site, long long n, float p, unsigned long long seed, void* stream);
int ocrl_tp_colsum(const float* X, long long ld, float* out, long long R, int F, int accumulate, float scale, float* ws, size_t ws_floats,
                   void* stream);
int ocrl_tp_mse(const float* obs, const float* recon, float* drecon /* nullable */, float* out, int B, int C, int H, int W, float* ws,
                size_t ws_floats, void* stream);
int ocrl_tp_pixel_shuffle(const float* in, float* out, int B, int h, int w, int Cout, int forward, const float* mask /* nullable */,
                          void* stream);
int ocrl_tp_nchw_to_nhwc8(const float* in, float* out, int B, int C, int H, int W, void* stream);
int ocrl_tp_patchify4(const float* in, float* out, int B, int C, int S, void* stream);
int ocrl_tp_pad_cols(const float* in, int ldi, float* out, int ldo, long long R, int C, int Cout, void* stream);
int ocrl_tp_im2col5(const float* x8, float* col, int B, int H, int W, int C, int ldc, void* stream);
int ocrl_tp_unpack5(const float* dWp, float* dW, int C, int ldc, void* stream);
int ocrl_tp_posmap(const float* Wpos, const float* bpos, float* out, int S, int C, void* stream);
int ocrl_tp_posgrid(float* out, int S, void* stream);
int ocrl_tp_onehot(const int* tokens, float* z, long long rows, int V, void* stream);
int ocrl_tp_slot_init(const float* mu, const float* logsig, const float* noise /* NULL = draw */, float* slots0, int BK, int D,
                      unsigned long long seed, void* stream);
int ocrl_tp_slot_init_bwd(const float* dslots0, const float* logsig, const float* noise /* NULL = draw */, float* dmu, float* dlogsig, int BK,
                          int D, unsigned long long seed, void* stream);
int ocrl_tp_argmax_pos(const float* pred, int* tokens, int B, int T, int V, int t, int dense_rows, void* stream);
int ocrl_tp_decode_attn(const float* qkv, float* out, int B, int T, int t, int d, int h, int ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif
