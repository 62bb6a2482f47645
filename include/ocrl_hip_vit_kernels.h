/* C ABI of the pooling-Transformer and masked-autoencoder kernels in libocrl_hip.so (gfx950), one launcher of pool.hip, pool_long.hip and
 * mae.hip per entry: what every RL step (pooling = transformer, cnn_transformer, SLATE-CNN) and every MAE step runs as part of a model,
 * reachable on caller-owned tensors so that each kernel can be compared with a reference of its own operation.  An eleventh header beside
 * ocrl_hip.h, ocrl_hip_dqn.h, ocrl_hip_rollout.h, ocrl_hip_replay.h, ocrl_hip_c51.h, ocrl_hip_noisy.h, ocrl_hip_classifier.h,
 * ocrl_hip_iodine.h, ocrl_hip_qr.h and ocrl_hip_slate_kernels.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads them all).
 * Conventions: every entry is stateless and takes device pointers (fp32, or int32 for ids; dense unless a leading dimension is an
 * argument), an `int` entry returns 0 on success and the message of a failure is ocrl_last_error(), every argument is checked before any
 * launch (null pointers that are not marked nullable, sizes below 1, the limits named below, 16-byte alignment of every base pointer a
 * kernel reads or writes as float4, element counts below 2^31), work is enqueued on `stream` (a hipStream_t) with no host
 * synchronisation.  The "host only" entries launch nothing.  Dropout: 0 <= p < 1, the keep decision of an element is that of
 * ocrl_tp_dropout_mask (ocrl_hip_slate_kernels.h) at the same (seed, site) and the element index named per entry.
 *
 * Short path (S = K + 1 <= 32 tokens, one workgroup per sample):
 * ocrl_vit_pool_embed: x0 [B][K + 1][d]: row 0 = cls, row 1 + k = lin[b][k], plus pos [K + 1][d] when given.  d % 4 == 0.
 * ocrl_vit_pool_rows: mode 0: out [B][K][d] = in [B][K + 1][d] without row 0; mode 1: out [B][K + 1][d] = in [B][d] at row 0, zeros
 *   elsewhere; mode 2: out [B][d] = row 0 of in [B][K + 1][d].  d % 4 == 0.
 * ocrl_vit_pool_attn_fwd: qkv [B S][3 d] = (q | k | v), h heads of d / h channels -> P [B][h][S][S] = softmax(q k^T / sqrt(d / h)) before
 *   dropout, O [B S][d] = dropout(P) v; the dropout element is ((b h + head) S + query) S + key.  ocrl_vit_pool_attn_bwd: dqkv [B S][3 d]
 *   from dO [B S][d] and the saved P.  Limits of either: 1 <= S <= 32, d % h == 0, head size d / h in {8, 16, 32, 64}, and the LDS request
 *   of the direction <= 160 KiB: forward 12 S d bytes, backward 4 (4 S d + 2 h S S) bytes.
 * ocrl_vit_pool_short_ok (host only): 1 when the short path (ocrl_pool_transformer_fwd and _bwd) runs K slots of width Din at d_model d
 *   and h heads in BOTH directions: 1 <= K <= 31, Din % 4 == 0, d in {64, 128, 192, 256}, h | d and the limits of ocrl_vit_pool_attn_fwd
 *   and _bwd at S = K + 1; otherwise 0, and ocrl_last_error() is the reason.  ocrl_pool_transformer_fwd / _bwd refuse such a shape with
 *   that reason before any launch.
 *
 * Long path:
 * ocrl_vit_pool_cols: dst[r][c] = c < ncopy ? src[r][c] : 0 for c < ncols, row strides lds >= ncopy, ldd >= ncols; ncopy <= ncols.
 * ocrl_vit_cls_drop: out [B][N] = (resid ? resid[b ldr + c] : 0) + dropout(x [B][N]), the dropout element is b S N + c (row 0 of image b
 *   of a [B][S][N] tensor); resid nullable, ldr >= N with it; out may be x.
 * ocrl_vit_cls_add: dX [B][S][d] row 0 += v [B][d].
 * ocrl_vit_flash_fwd: qkv [B S][3 d] -> O [B S][d], lse [B h][S] (log-sum-exp of the scaled scores); any S >= 1; the dropout element is
 *   that of the short path.  ocrl_vit_flash_bwd: Dd [B h][S] = dO . O per head, dqkv [B S][3 d].  d % h == 0, head size in {16, 32, 48,
 *   64}, B h <= 65535.
 * ocrl_vit_cls_nchunk (host only): the number of position chunks per image the CLS-row attention splits S rows into at batch B; *chunk
 *   (nullable) = rows per chunk, a multiple of 64.  ocrl_vit_cls_part_floats (host only): the floats of `part` either direction needs: B
 *   nchunk h (d + 4) forward, B nchunk h d backward; 0 for a refused shape.
 * ocrl_vit_cls_attn_fwd: attention of the query row q [B][d] (row 0 of the last layer, bias included) over the S rows of X [B][S][d] with
 *   the projections folded, Win [3 d][d], bin [3 d] the in-projection: U [B][h][d] = W_k,h^T q_h / sqrt(d / h), z [B][h][d] = sum_j p'_hj
 *   x_j, stat [B][h][2] = (sum_j p'_hj, log-sum-exp), o [B][d] = W_v,h z_h + b_v,h sum_j p'_hj; p' = dropout(p), the dropout element is (b
 *   h + head) S S + key.  ocrl_vit_cls_attn_bwd: from dO [B][d] and the forward's U, z, stat: G [B][h][d] = W_v,h^T dO_h, gD [B][h][2] =
 *   (b_v,h . dO_h, sum_j p'_hj dp'_hj), dX [B][S][d] through keys and values (every row written), w [B][h][d] = sum_j ds_hj x_j, dq [B][d],
 *   dW [3 d][d] and db [3 d] summed over the batch (x0 [B][d] = row 0 of X; the k rows of db are exactly 0).  d % 4 == 0, d <= 256, h <=
 *   16, h d <= 4096, d % h == 0, B <= 65535, part_floats >= ocrl_vit_cls_part_floats of the direction.
 *
 * Masked autoencoder (token rows [B][n + 1][D] with the CLS row first):
 * ocrl_vit_patch_gather: out [B n][3 p p], row (b, i) = patch ids[b n + i] (ids NULL: i) of obs [B][3][S][S] in (c, ph, pw) order.  S % p
 *   == 0, 1 <= n <= L = (S / p)^2 <= 1024.  Four pixels per thread when p % 4 == 0 and obs, out are 16-byte aligned and force_scalar ==
 *   0; one otherwise.  ids are device data: they must lie in [0, L).
 * ocrl_vit_tokens_fwd: x0 [B][n + 1][D]: row 0 = cls + pos[0], row 1 + i = embed[b][i] + pos[1 + ids[b n + i]] (ids NULL: i), pos [L +
 *   1][D].  ocrl_vit_tokens_bwd: dembed [B n][D] = dx0 without its CLS rows, dcls [D] = sum_b dx0[b][0].  D % 4 == 0.
 * ocrl_vit_unshuffle_fwd: xd [B][L + 1][D]: row 0 = e[b][0], row 1 + l = (restore[b][l] < len_keep ? e[b][1 + restore[b][l]] : mtok), plus
 *   dpos [L + 1][D]; e [B][len_keep + 1][D].  ocrl_vit_unshuffle_bwd: de [B][len_keep + 1][D] = dxd rows (0, 1 + keep[b][r]), dmtok [D] =
 *   sum of the rows 1 + l with mask[b][l] != 0; part: B D floats of scratch.  D % 4 == 0, 1 <= len_keep <= L <= 1024.
 * ocrl_vit_gelu_fwd: y = x Phi(x) (erf form) over n elements; ocrl_vit_gelu_bwd: dpre = dy gelu'(pre), dpre may be dy.  n % 4 == 0.
 * ocrl_vit_ln_fwd: y = (x - mean) rstd g + b per row of F, rstd = (var + eps)^-1/2, mean and rstd [R] saved.  ocrl_vit_ln_bwd: dx (+ resid
 *   [R][F], nullable), dg, db [F]; part_floats >= 2 F ocrl_vit_ln_chunks(R).  ocrl_vit_ln_chunks (host only): the row chunks of the g / b
 *   gradient partials, at most 256 (0 for R < 1).  F % 4 == 0, F >= 4.
 * ocrl_vit_loss: loss[0] = loss[1] = sum_{b, l} mask[b][l] mean_j (pred[b][l][j] - target)^2 / (B (L - len_keep)), pred [B][L][3 p p],
 *   target = obs [B][3][S][S] in patchify's (ph, pw, c) order; dpred [B][L + 1][3 p p] (nullable; needs dloss [1], a device scalar) = its
 *   gradient times dloss, the CLS rows zero; part: B L floats (needed with loss).  loss and dpred are both nullable, not both null.  S % p
 *   == 0, L == (S / p)^2 <= 1024, 1 <= len_keep <= L (len_keep == L: the loss is NaN, as in the reference). */
#ifndef OCRL_HIP_VIT_KERNELS_H
#define OCRL_HIP_VIT_KERNELS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int ocrl_vit_pool_embed(const float* lin, const float* cls, const float* pos /* nullable */, float* x0, int B, int K, int d, void* stream);
int ocrl_vit_pool_rows(const float* in, float* out, int B, int K, int d, int mode, void* stream);
int ocrl_vit_pool_attn_fwd(const float* qkv, float* P, float* O, int B, int S, int d, int h, float p, unsigned long long seed, unsigned site,
                           void* stream);
int ocrl_vit_pool_attn_bwd(const float* qkv, const float* P, const float* dO, float* dqkv, int B, int S, int d, int h, float p,
                           unsigned long long seed, unsigned site, void* stream);
int ocrl_vit_pool_short_ok(int K, int Din, int d, int h);

int ocrl_vit_pool_cols(const float* src, int lds, float* dst, int ldd, long long rows, int ncols, int ncopy, void* stream);
int ocrl_vit_cls_drop(const float* x, const float* resid /* nullable */, int ldr, float* out, int B, int N, int S, float p,
                      unsigned long long seed, unsigned site, void* stream);
int ocrl_vit_cls_add(float* dX, const float* v, int B, int d, int S, void* stream);
int ocrl_vit_flash_fwd(const float* qkv, float* O, float* lse, int B, int S, int d, int h, float p, unsigned long long seed, unsigned site,
                       void* stream);
int ocrl_vit_flash_bwd(const float* qkv, const float* O, const float* lse, const float* dO, float* Dd, float* dqkv, int B, int S, int d, int h,
                       float p, unsigned long long seed, unsigned site, void* stream);
int ocrl_vit_cls_nchunk(int B, int S, int* chunk /* nullable */);
size_t ocrl_vit_cls_part_floats(int B, int S, int d, int h, int backward);
int ocrl_vit_cls_attn_fwd(const float* X, const float* Win, const float* bin, const float* q, float* U, float* z, float* stat, float* o,
                          float* part, size_t part_floats, int B, int S, int d, int h, float p, unsigned long long seed, unsigned site,
                          void* stream);
int ocrl_vit_cls_attn_bwd(const float* X, const float* Win, const float* bin, const float* q, const float* U, const float* z, const float* stat,
                          const float* dO, const float* x0, float* G, float* gD, float* dX, float* w, float* dq, float* dW, float* db,
                          float* part, size_t part_floats, int B, int S, int d, int h, float p, unsigned long long seed, unsigned site,
                          void* stream);

int ocrl_vit_patch_gather(const float* obs, const int* ids /* nullable */, float* out, int B, int n, int S, int p, int force_scalar,
                          void* stream);
int ocrl_vit_tokens_fwd(const float* embed, const float* cls, const float* pos, const int* ids /* nullable */, float* x0, int B, int n, int L,
                        int D, void* stream);
int ocrl_vit_tokens_bwd(const float* dx0, float* dembed, float* dcls, int B, int n, int D, void* stream);
int ocrl_vit_unshuffle_fwd(const float* e, const float* mtok, const float* dpos, const int* restore, float* xd, int B, int L, int len_keep,
                           int D, void* stream);
int ocrl_vit_unshuffle_bwd(const float* dxd, const int* keep, const float* mask, float* de, float* dmtok, float* part, int B, int L,
                           int len_keep, int D, void* stream);
int ocrl_vit_gelu_fwd(const float* pre, float* y, long long n, void* stream);
int ocrl_vit_gelu_bwd(const float* dy, const float* pre, float* dpre, long long n, void* stream);
int ocrl_vit_ln_chunks(long long R);
int ocrl_vit_ln_fwd(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, long long R, int F, float eps,
                    void* stream);
int ocrl_vit_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, const float* resid /* nullable */,
                    float* dx, float* dg, float* db, float* part, size_t part_floats, long long R, int F, void* stream);
int ocrl_vit_loss(const float* pred, const float* obs, const float* mask, const float* dloss /* nullable */, float* part /* nullable */,
                  float* loss /* nullable */, float* dpred /* nullable */, int B, int L, int len_keep, int S, int p, void* stream);

#ifdef __cplusplus
}
#endif
#endif
