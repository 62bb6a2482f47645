/* C ABI of DQN's quantile head in libocrl_hip.so (gfx950): the return distribution of QR-DQN (Dabney et al. 2018) as N quantile values per
 * action, with no support to set, an optional dueling aggregation, its epsilon-greedy collection step and its fused TD step (the quantile
 * Huber loss between the chosen action's quantiles and the Bellman-shifted quantiles of the bootstrap action, and its gradient).  A header
 * beside ocrl_hip_c51.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads them all); the conventions are ocrl_hip_c51.h's:
 * every entry is stateless and takes device pointers (fp32 unless said otherwise), an `int` entry returns 0 on success and the message of a
 * failure is ocrl_last_error(), every argument is checked before any launch, work is enqueued on `stream` (a hipStream_t) with no host
 * synchronisation, there are no atomics, every loop is bounded and the results are bit-reproducible: partial sums are folded in a fixed
 * order, and a row's forward results do not depend on its position in the batch or on B.
 *
 * The head: features [B, F] -> n x [Linear(dims[l]), acts[l]] -> the advantage Linear(last, A * N), and with `dueling` != 0 a value
 *   Linear(last, N) beside it on the same latent.  acts: 0 none, 1 ReLU, 2 tanh.  Column a * N + i of the advantage Linear is quantile i
 *   of action a.  w / dw: host arrays of device pointers in ocrl_c51_*'s order: (weight [out, in], bias [out]) per layer of the chain in
 *   state_dict order, then the advantage Linear's weight [A * N, last] and bias [A * N], then, when dueling, the value Linear's weight
 *   [N, last] and bias [N]: 2 (n + 1) pointers, 2 (n + 2) when dueling.
 *   Limits: B >= 1, F >= 1, 1 <= A <= 64, 1 <= N <= 64, A * N <= 256, 0 <= n <= 8, widths multiples of 4 up to 256, and for the TD step
 *   kappa finite and > 0.  Anything else is rejected before any launch: ocrl_qr_ws_floats returns 0, the other entries non-zero, each with
 *   an ocrl_last_error message that names the limit.
 *   Arithmetic: the Linear layers are ocrl_qnet_*'s (exact fp32 products on the matrix pipe, a layer output = two k-interleaved chains +
 *   bias).  Everything below is fp32, each sum serial in the order written:
 *     theta[a, i] = Adv[a, i]                                                 -- dueling == 0
 *     theta[a, i] = (V[i] + Adv[a, i]) - (1 / A) S_i,  S_i = sum_a' Adv[a', i] in ascending a'      -- dueling != 0
 *     q[a]        = (sum_i theta[a, i]) * (1 / N), the sum in ascending i
 *     tau_i       = (i + 0.5) / N
 *   q is formed by one device function in every kernel: ocrl_qr_act's q and the TD step's q are ocrl_qr_fwd's bit for bit.
 *
 * ocrl_qr_fwd: one launch.  quantiles [B, A, N] (theta) and q [B, A] may each be NULL, but not both.  save != 0 keeps the chain's layer
 *   outputs in ws (ws_floats >= ocrl_qr_ws_floats); save == 0 (the target network) needs no workspace.
 * ocrl_qr_bwd: the cotangent dquantiles [B, A, N] of a forward that ran with save != 0 on the same ws -> dw and dfeatures [B, F] (may be
 *   NULL), overwritten; two launches (the tiles' backward, the fold of the partial dw).  With dueling, as ocrl_c51_bwd,
 *     dV[i] = sum_a dtheta[a, i] in ascending a;   dAdv[a, i] = dtheta[a, i] - (1 / A) dV[i].
 *
 * ocrl_qr_act: the collection step: forward, mean and choice in one launch, no workspace.  The coin and the random action are
 *   ocrl_dqn_act's, word for word: row r takes two 24-bit uniforms of row R = row_offset + r of stream `seed`, with (x, y) the two 32-bit
 *   words of the library's counter RNG at site 410, key high word R >> 32, counter R & 0xffffffff,
 *     u0 = (x >> 8) / 2^24,  u1 = (y >> 8) / 2^24;   `uniforms` [B, 2] (u0, u1 per row, each k / 2^24) replaces the draw
 *     u0 < epsilon:  action = floor(u1 * A), computed on the 24 bits b = u1 * 2^24 as (b * A) >> 24;
 *     otherwise:     action = the lowest index of the maximum of q[r, :].
 *   ocrl_dqn_act_uniforms (ocrl_hip_dqn.h) writes exactly what is drawn.  actions: int64 [B].  q [B, A] may be NULL.
 *
 * ocrl_qr_td_fwd_bwd: the whole gradient step of the head in three launches (the tiles' forward + loss + backward, the fold of the
 *   partial dw, the fold of the scalars).  next_quantiles [B, A, N] and next_q [B, A] describe the next observations: next_quantiles is
 *   the target network's, next_q the target network's, or the online network's for double Q-learning.  Per row b, with a = actions[b]
 *   (int64) clamped into [0, A), a* = the lowest index of the maximum of next_q[b, :], g_b = discounts[b] or gamma, w_b = weights[b] or 1:
 *     row not done:  T_j = r_b + g_b * next_quantiles[b, a*, j]
 *     row done:      T_j = r_b       -- a select: next_quantiles and next_q of a finished row are never read and may be NaN / inf
 *     u_ij   = T_j - theta[a, i]
 *     L(u)   = 0.5 u^2 if |u| <= kappa, else kappa (|u| - 0.5 kappa)
 *     rho_ij = |tau_i - [u_ij < 0]| * L(u_ij)       -- [.] is 1 or 0; no division by kappa (the paper's loss at kappa = 1)
 *     ql_b   = sum_i ( (1 / N) * sum_j rho_ij ), j ascending inside, i ascending outside;   loss = mean_b w_b ql_b
 *     dtheta[b, a, i] = -(w_b / B) * (1 / N) * sum_j |tau_i - [u_ij < 0]| * clamp(u_ij, -kappa, kappa), j ascending; zero for the other
 *                       actions
 *   scalars [3] = loss, mean_b q[b, a_b], mean_b (1 / N) sum_j T_j (j ascending).  row_loss [B] (may be NULL) = ql_b, unweighted: the
 *   priority of prioritized replay.  dones: uint8 [B].  dw (and dfeatures [B, F], may be NULL) are the gradients of `loss`, overwritten,
 *   not accumulated.  ws_floats >= ocrl_qr_ws_floats.  A tile's scalar terms are added in row order, the tiles of a slab in tile order,
 *   the slabs in slab order, as ocrl_dqn_td_fwd_bwd's. */
#ifndef OCRL_HIP_QR_H
#define OCRL_HIP_QR_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int B, F, A, N, n, dueling;
    int dims[8];
    int acts[8];
} ocrl_qr_desc;
size_t ocrl_qr_desc_size(void);
size_t ocrl_qr_ws_floats(const ocrl_qr_desc* d);
int ocrl_qr_fwd(const ocrl_qr_desc* d, const float* features, const float* const* w, float* quantiles /* may be NULL */,
                float* q /* may be NULL */, int save, float* ws, size_t ws_floats, void* stream);
int ocrl_qr_bwd(const ocrl_qr_desc* d, const float* features, const float* const* w, const float* dquantiles,
                float* dfeatures /* may be NULL */, float* const* dw, float* ws, size_t ws_floats, void* stream);
int ocrl_qr_act(const ocrl_qr_desc* d, const float* features, const float* const* w, unsigned long long seed,
                unsigned long long row_offset, float epsilon, const float* uniforms /* [B, 2] or NULL = draw */, long long* actions,
                float* q /* may be NULL */, void* stream);
int ocrl_qr_td_fwd_bwd(const ocrl_qr_desc* d, const float* features, const float* const* w, const float* next_quantiles,
                       const float* next_q, const long long* actions, const float* rewards, const unsigned char* dones,
                       const float* discounts /* may be NULL */, const float* weights /* may be NULL */, float gamma, float kappa,
                       float* scalars, float* row_loss /* may be NULL */, float* dfeatures /* may be NULL */, float* const* dw, float* ws,
                       size_t ws_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
