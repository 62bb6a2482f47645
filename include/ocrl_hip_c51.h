/* C ABI of DQN's categorical head in libocrl_hip.so (gfx950): the return distribution of C51 (Bellemare et al. 2017) on a fixed support,
 * with an optional dueling aggregation, its epsilon-greedy collection step and its fused TD step (projection of the target distribution,
 * cross-entropy, gradient).  A fifth header beside ocrl_hip.h, ocrl_hip_dqn.h, ocrl_hip_rollout.h and ocrl_hip_replay.h, self-contained
 * and in the same dialect (ocrl_amd/_abi.py reads them all); the conventions are ocrl_hip_dqn.h's: every entry is stateless and takes
 * device pointers (fp32 unless said otherwise), an `int` entry returns 0 on success and the message of a failure is ocrl_last_error(),
 * every argument is checked before any launch, work is enqueued on `stream` (a hipStream_t) with no host synchronisation, there are no
 * atomics, every loop is bounded and the results are bit-reproducible: partial sums are folded in a fixed order, and a row's forward
 * results do not depend on its position in the batch or on B.
 *
 * The head: features [B, F] -> n x [Linear(dims[l]), acts[l]] -> the advantage Linear(last, A * Z), and with `dueling` != 0 a value
 *   Linear(last, Z) beside it on the same latent.  acts: 0 none, 1 ReLU, 2 tanh.  Column a * Z + j of the advantage Linear is atom j of
 *   action a.  w / dw: host arrays of device pointers, (weight [out, in], bias [out]) per layer of the chain in state_dict order, then the
 *   advantage Linear's weight [A * Z, last] and bias [A * Z], then, when dueling, the value Linear's weight [Z, last] and bias [Z]:
 *   2 (n + 1) pointers, 2 (n + 2) when dueling.
 *   Limits: B >= 1, F >= 1, 1 <= A <= 64, 2 <= Z <= 64, A * Z <= 256, 0 <= n <= 8, widths multiples of 4 up to 256, v_min < v_max and
 *   both finite.  Anything else is rejected before any launch: ocrl_c51_ws_floats returns 0, the other entries non-zero, each with an
 *   ocrl_last_error message that names the limit.
 *   Arithmetic: the Linear layers are ocrl_qnet_*'s (exact fp32 products on the matrix pipe, a layer output = two k-interleaved chains +
 *   bias).  Everything below is fp32, each sum serial in the order written:
 *     dz = (v_max - v_min) / (Z - 1);   z_j = v_min + j * dz
 *     logit[a, j] = Adv[a, j]                                                 -- dueling == 0
 *     logit[a, j] = (V[j] + Adv[a, j]) - (1 / A) S_j,  S_j = sum_a' Adv[a', j] in ascending a'      -- dueling != 0
 *     p[a, j]     = exp(logit[a, j] - M_a) / sum_j' exp(logit[a, j'] - M_a),  M_a = max_j logit[a, j], the sum in ascending j'
 *     q[a]        = sum_j p[a, j] z_j in ascending j
 *
 * ocrl_c51_fwd: one launch.  logits [B, A, Z], probs [B, A, Z] and q [B, A] may each be NULL, but not all three.  save != 0 keeps the
 *   chain's layer outputs in ws (ws_floats >= ocrl_c51_ws_floats); save == 0 (the target network) needs no workspace.
 * ocrl_c51_bwd: the cotangent dlogits [B, A, Z] of a forward that ran with save != 0 on the same ws -> dw and dfeatures [B, F] (may be
 *   NULL), overwritten; two launches (the tiles' backward, the fold of the partial dw).  With dueling
 *     dV[j] = sum_a dlogit[a, j] in ascending a;   dAdv[a, j] = dlogit[a, j] - (1 / A) dV[j].
 *
 * ocrl_c51_act: the collection step: forward, expectation and choice in one launch, no workspace.  The coin and the random action are
 *   ocrl_dqn_act's, word for word: row r takes two 24-bit uniforms of row R = row_offset + r of stream `seed`, with (x, y) the two 32-bit
 *   words of the library's counter RNG at site 410, key high word R >> 32, counter R & 0xffffffff,
 *     u0 = (x >> 8) / 2^24,  u1 = (y >> 8) / 2^24;   `uniforms` [B, 2] (u0, u1 per row, each k / 2^24) replaces the draw
 *     u0 < epsilon:  action = floor(u1 * A), computed on the 24 bits b = u1 * 2^24 as (b * A) >> 24;
 *     otherwise:     action = the lowest index of the maximum of q[r, :].
 *   ocrl_dqn_act_uniforms (ocrl_hip_dqn.h) writes exactly what is drawn.  actions: int64 [B].  q [B, A] may be NULL; it is
 *   ocrl_c51_fwd's q bit for bit.
 *
 * ocrl_c51_td_fwd_bwd: the whole gradient step of the head in three launches (the tiles' forward + loss + backward, the fold of the
 *   partial dw, the fold of the scalars).  next_probs [B, A, Z] and next_q [B, A] describe the next observations: next_probs is the target
 *   network's, next_q the target network's, or the online network's for double Q-learning.  Per row b, with a = actions[b] (int64)
 *   clamped into [0, A), a* = the lowest index of the maximum of next_q[b, :], g_b = discounts[b] or gamma, w_b = weights[b] or 1:
 *     row not done:  T_j = clamp(r_b + g_b z_j, v_min, v_max);  beta_j = (T_j - v_min) / dz
 *                    m_i = sum_j next_probs[b, a*, j] max(0, 1 - |beta_j - i|) in ascending j
 *     row done:      beta = (clamp(r_b, v_min, v_max) - v_min) / dz;   m_i = max(0, 1 - |beta - i|)
 *                    -- a select: next_probs and next_q of a finished row are never read
 *   the gather form of the projection onto the support: no write conflicts and a fixed order of summation; it equals the textbook scatter
 *   (each target atom's mass split between floor(beta_j) and ceil(beta_j)) exactly.
 *     ce_b  = -sum_i m_i log p[a, i],  log p[a, i] = (logit[a, i] - M_a) - log sum_j exp(logit[a, j] - M_a);   loss = mean_b w_b ce_b
 *     dlogit[b, a, i] = w_b (p[a, i] sum_i' m_i' - m_i) / B, zero for the other actions
 *   scalars [3] = loss, mean_b q[b, a_b], mean_b sum_i m_i z_i.  row_loss [B] (may be NULL) = ce_b, unweighted: the priority of
 *   prioritized replay.  dones: uint8 [B].  dw (and dfeatures [B, F], may be NULL) are the gradients of `loss`, overwritten, not
 *   accumulated.  ws_floats >= ocrl_c51_ws_floats.  A tile's scalar terms are added in row order, the tiles of a slab in tile order, the
 *   slabs in slab order, as ocrl_dqn_td_fwd_bwd's. */
#ifndef OCRL_HIP_C51_H
#define OCRL_HIP_C51_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int B, F, A, Z, n, dueling;
    int dims[8];
    int acts[8];
} ocrl_c51_desc;
size_t ocrl_c51_desc_size(void);
size_t ocrl_c51_ws_floats(const ocrl_c51_desc* d);
int ocrl_c51_fwd(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max,
                 float* logits /* may be NULL */, float* probs /* may be NULL */, float* q /* may be NULL */, int save, float* ws,
                 size_t ws_floats, void* stream);
int ocrl_c51_bwd(const ocrl_c51_desc* d, const float* features, const float* const* w, const float* dlogits,
                 float* dfeatures /* may be NULL */, float* const* dw, float* ws, size_t ws_floats, void* stream);
int ocrl_c51_act(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max, unsigned long long seed,
                 unsigned long long row_offset, float epsilon, const float* uniforms /* [B, 2] or NULL = draw */, long long* actions,
                 float* q /* may be NULL */, void* stream);
int ocrl_c51_td_fwd_bwd(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max,
                        const float* next_probs, const float* next_q, const long long* actions, const float* rewards,
                        const unsigned char* dones, const float* discounts /* may be NULL */, const float* weights /* may be NULL */,
                        float gamma, float* scalars, float* row_loss /* may be NULL */, float* dfeatures /* may be NULL */,
                        float* const* dw, float* ws, size_t ws_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
