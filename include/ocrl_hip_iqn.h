/* C ABI of DQN's implicit quantile head in libocrl_hip.so (gfx950): the return distribution of IQN (Dabney, Ostrovski, Silver and Munos
 * 2018) as a function of a sampled fraction tau: a cosine embedding of tau gates the features, a chain of small Linear layers maps the
 * gated features to one quantile value per action, and every row of a batch is evaluated at N fractions of its own.  With it its draw of
 * the fractions, its epsilon-greedy collection step and its fused TD step (the quantile Huber loss of QR-DQN at the sampled fractions,
 * with a target sample count of its own, and its gradient).  A header beside ocrl_hip_qr.h, self-contained and in the same dialect
 * (ocrl_amd/_abi.py reads them all); the conventions are ocrl_hip_qr.h's: every entry is stateless and takes device pointers (fp32 unless
 * said otherwise), an `int` entry returns 0 on success and the message of a failure is ocrl_last_error(), every argument is checked
 * before any launch, work is enqueued on `stream` (a hipStream_t) with no host synchronisation, there are no atomics, every loop is
 * bounded and the results are bit-reproducible: partial sums are folded in a fixed order, and a row's forward results do not depend on
 * its position in the batch or on B.
 *
 * The head.  N = the fractions per batch row of this call (the online network's N, a target forward's N', acting's K), C = the number
 *   of cosines.  taus [B, N] holds the fractions; expanded row e = b * N + s is sample s of batch row b.  Per expanded row, in fp32:
 *     c_k    = cospif((float)k * tau[b, s]),  k = 0 .. C - 1      -- the paper's sum from i = 0; the product is one fp32 rounding
 *     phi_j  = max(0, be[j] + sum_k We[j, k] c_k)                  -- We [F, C], be [F]; always ReLU
 *     z_j    = features[b, j] * phi_j
 *     theta[b, a, s] = Linear(last, A)( chain(z) )                 -- chain = n x [Linear(dims[l]), acts[l]]; acts: 0 none, 1 ReLU, 2 tanh
 *     q[b, a] = (sum_s theta[b, a, s]) * (1 / N), the sum serial in ascending s
 *   w / dw: host arrays of device pointers: (We, be), then (weight [out, in], bias [out]) per layer of the chain in state_dict order,
 *   then the output Linear's weight [A, last] and bias [A]: 2 (n + 2) pointers.
 *   Limits: B >= 1, B * N < 2^23 expanded rows, F a multiple of 4 in 4 .. 256 (z is an activation tile and the embedding has F outputs),
 *   1 <= A <= 64, 1 <= N <= 64, 1 <= Np <= 64, C a multiple of 4 in 4 .. 64, 0 <= n <= 8, widths multiples of 4 up to 256, and for the
 *   TD step kappa finite and > 0.  Anything else is rejected before any launch: ocrl_iqn_ws_floats returns 0, the other entries non-zero,
 *   each with an ocrl_last_error message that names the limit.
 *   Arithmetic: every Linear, the embedding included, is ocrl_qnet_*'s (exact fp32 products on the matrix pipe, a layer output = two
 *   k-interleaved chains + bias).  q is formed by the same serial sum in every kernel: ocrl_iqn_act's q is ocrl_iqn_fwd's bit for bit on
 *   the same taus.
 *   Workspace: ocrl_iqn_ws_floats(d) = the Q head's workspace (ocrl_qnet_ws_floats) of E = B * N rows of C features through the layers
 *   (F ReLU, dims ..., A), followed by four blocks, each rounded up to a multiple of 64 floats: E * A (theta when `quantiles` is NULL),
 *   E (the rows' partial losses), E (theta of the action taken), E * F (dz * phi).
 *
 * ocrl_iqn_taus: one launch.  out[b, s] = k / 2^24 with k the top 24 bits of a word of the library's counter RNG at site 450: with
 *   R = row_offset + b and G = 32 R + (s >> 1), (x, y) are the two 32-bit words at key high word G >> 32, counter G & 0xffffffff of
 *   stream `seed`; tau = ((s even ? x : y) >> 8) / 2^24.  A pure function of (seed, row_offset + b, s): it does not depend on B or N.
 *
 * ocrl_iqn_fwd: `quantiles` [B, A, N] (theta) and q [B, A] may each be NULL, but not both.  One launch for theta alone, two with q (the
 *   tiles, then the fold over s).  save != 0 keeps phi and the chain's layer outputs in ws for ocrl_iqn_bwd; the workspace is needed
 *   (ws_floats >= ocrl_iqn_ws_floats) when save != 0 or when `quantiles` is NULL, and not otherwise (a target network's forward).
 * ocrl_iqn_bwd: the cotangent dquantiles [B, A, N] of a forward that ran with save != 0 on the same ws and the same taus -> dw and
 *   dfeatures [B, F] (may be NULL), overwritten, not accumulated; taus get no gradient.  Two launches (the tiles' backward, the fold of
 *   the partial dw), three with dfeatures (the fold over s).  Given dz, the cotangent of z from the chain:
 *     dfeatures[b, j] = sum_s dz[b, s, j] * phi[b, s, j], serial in ascending s
 *     dphi = dz * features, masked by phi > 0, then into dWe and dbe as any layer's.
 *
 * ocrl_iqn_act: the collection step in one launch, no workspace: one workgroup per batch row walks its N samples in ascending s.  taus
 *   [B, N], or NULL: the kernel draws exactly what ocrl_iqn_taus(seed, row_offset, B, N) writes.  The coin and the random action are
 *   ocrl_dqn_act's, word for word: row r takes two 24-bit uniforms of row R = row_offset + r of stream `seed`, with (x, y) the two 32-bit
 *   words of the counter RNG at site 410, key high word R >> 32, counter R & 0xffffffff,
 *     u0 = (x >> 8) / 2^24,  u1 = (y >> 8) / 2^24;   `uniforms` [B, 2] (u0, u1 per row, each k / 2^24) replaces the draw
 *     u0 < epsilon:  action = floor(u1 * A), computed on the 24 bits b = u1 * 2^24 as (b * A) >> 24;
 *     otherwise:     action = the lowest index of the maximum of q[r, :].
 *   actions: int64 [B].  q [B, A] may be NULL.
 *
 * ocrl_iqn_td_fwd_bwd: the whole gradient step of the head in four launches (the tiles' forward + loss + backward, the fold over s of
 *   the rows' terms and of dfeatures, the fold of the partial dw, the fold of the scalars).  It is ocrl_qr_td_fwd_bwd's with the sampled
 *   fractions taus [B, N] and Np target samples: next_quantiles [B, A, Np] is the target network's theta at fractions of its own, next_q
 *   [B, A] the target network's q, or the online network's for double Q-learning.  Per row b, with a = actions[b] (int64) clamped into
 *   [0, A), a* = the lowest index of the maximum of next_q[b, :], g_b = discounts[b] or gamma, w_b = weights[b] or 1:
 *     row not done:  T_j = fma(g_b, next_quantiles[b, a*, j], r_b),  j < Np
 *     row done:      T_j = r_b       -- a select: next_quantiles and next_q of a finished row are never read and may be NaN / inf
 *     u_ij   = T_j - theta[b, a, i]
 *     L(u)   = 0.5 u^2 if |u| <= kappa, else kappa (|u| - 0.5 kappa)
 *     rho_ij = |taus[b, i] - [u_ij < 0]| * L(u_ij)       -- [.] is 1 or 0; no division by kappa
 *     ql_b   = sum_i ( (1 / Np) * sum_j rho_ij ), j ascending inside, i ascending outside;   loss = mean_b w_b ql_b
 *     dtheta[b, a, i] = -(w_b / B) * (1 / Np) * sum_j |taus[b, i] - [u_ij < 0]| * clamp(u_ij, -kappa, kappa), j ascending; zero for the
 *                       other actions
 *   scalars [3] = loss, mean_b q[b, a_b], mean_b (1 / Np) sum_j T_j (j ascending).  row_loss [B] (may be NULL) = ql_b, unweighted: the
 *   priority of prioritized replay.  dones: uint8 [B].  dw (and dfeatures [B, F], may be NULL) are the gradients of `loss`, overwritten,
 *   not accumulated.  ws_floats >= ocrl_iqn_ws_floats.  The scalar terms of 16 batch rows are added in row order, the groups of a slab
 *   in ascending order, the slabs in slab order, as ocrl_dqn_td_fwd_bwd's. */
#ifndef OCRL_HIP_IQN_H
#define OCRL_HIP_IQN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int B, F, A, N, C, n;
    int dims[8];
    int acts[8];
} ocrl_iqn_desc;
size_t ocrl_iqn_desc_size(void);
size_t ocrl_iqn_ws_floats(const ocrl_iqn_desc* d);
int ocrl_iqn_taus(unsigned long long seed, unsigned long long row_offset, int B, int N, float* out, void* stream);
int ocrl_iqn_fwd(const ocrl_iqn_desc* d, const float* features, const float* taus, const float* const* w, float* quantiles /* may be NULL */,
                 float* q /* may be NULL */, int save, float* ws, size_t ws_floats, void* stream);
int ocrl_iqn_bwd(const ocrl_iqn_desc* d, const float* features, const float* taus, const float* const* w, const float* dquantiles,
                 float* dfeatures /* may be NULL */, float* const* dw, float* ws, size_t ws_floats, void* stream);
int ocrl_iqn_act(const ocrl_iqn_desc* d, const float* features, const float* const* w, unsigned long long seed,
                 unsigned long long row_offset, float epsilon, const float* uniforms /* [B, 2] or NULL = draw */,
                 const float* taus /* [B, N] or NULL = draw */, long long* actions, float* q /* may be NULL */, void* stream);
int ocrl_iqn_td_fwd_bwd(const ocrl_iqn_desc* d, const float* features, const float* taus, const float* const* w, const float* next_quantiles,
                        int Np, const float* next_q, const long long* actions, const float* rewards, const unsigned char* dones,
                        const float* discounts /* may be NULL */, const float* weights /* may be NULL */, float gamma, float kappa,
                        float* scalars, float* row_loss /* may be NULL */, float* dfeatures /* may be NULL */, float* const* dw, float* ws,
                        size_t ws_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
