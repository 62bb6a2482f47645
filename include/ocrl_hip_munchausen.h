/* C ABI of DQN's Munchausen targets in libocrl_hip.so (gfx950): Munchausen RL (Vieillard, Pietquin and Geist 2020) adds the scaled, clipped
 * log-policy of the action taken to the reward and bootstraps from the soft value of a soft-max policy in place of the hard maximum over
 * the next actions.  It touches no head: one launch rewrites `rewards` and the target network's values at the next observation, the two
 * things ocrl_dqn_td_fwd_bwd_ext, ocrl_qr_td_fwd_bwd and ocrl_iqn_td_fwd_bwd already take as inputs, and those run after it unchanged.  A
 * header beside ocrl_hip_iqn.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads them all); the conventions are
 * ocrl_hip_iqn.h's: the entry is stateless and takes device pointers (fp32 unless said otherwise), it returns 0 on success and the message
 * of a failure is ocrl_last_error(), every argument is checked before the launch, work is enqueued on `stream` (a hipStream_t) with no host
 * synchronisation, there are no atomics, every loop is bounded and the results are bit-reproducible: every sum is serial in a stated order,
 * and a row's outputs do not depend on its position in the batch or on B.
 *
 * ocrl_munchausen_targets: one launch (one 64-lane workgroup per batch row), no workspace.  cur_q [B, A] and next_q [B, A] are the *target*
 *   network's action values at the observation and at the next observation, next_quantiles [B, A, Np] its quantile values at the next
 *   observation (the quantile and implicit quantile heads; NULL with Np = 0 for the scalar head).  actions: int64 [B]; dones: uint8 [B].
 *
 *   The policy of a vector x[0 .. A), in fp32; every operation below is one rounding to nearest, expf / logf are the device library's:
 *     v        = max_a x_a
 *     s_a      = (x_a - v) / tau                        -- a subtraction, then an IEEE division
 *     Z        = sum_a expf(s_a), serial in ascending a from 0
 *     logpi_a  = s_a - logf(Z)
 *     pi_a     = expf(logpi_a)
 *     c_a      = tau * logpi_a
 *   s_a = 0 at the maximum, so 1 <= Z <= A and logf(Z) is finite; everything is finite while (x_a - v) / tau is.  An action far below the
 *   maximum has pi_a = 0 and a finite logpi_a: its terms below are 0, not NaN.
 *
 *   The bonus, of every row, finished ones included (cur_q of every row is read), with a = actions[b] clamped into [0, A) and c of
 *   cur_q[b, :]:
 *     bonus_b        = alpha * fminf(0, fmaxf(clip_lo, c_a))
 *     rewards_out[b] = rewards[b] + bonus_b
 *
 *   Row not done, with pi, c of next_q[b, :]:
 *     V_b   = sum_a pi_a * (next_q[b, a] - c_a):               t = next_q[b, a] - c_a, then V = fmaf(pi_a, t, V), ascending a from V = 0
 *     M_bj  = sum_a pi_a * (next_quantiles[b, a, j] - c_a):    the same two steps in the same order, j < Np
 *     next_v[b, a]    = V_b  for every a
 *     next_m[b, a, j] = M_bj for every a
 *   Row done:
 *     next_v[b, :] = 0 and next_m[b, :, :] = 0     -- a select: next_q and next_quantiles of a finished row are never read and may be
 *                                                     NaN / inf
 *   The broadcast over a is the point: whatever bootstrap action a TD kernel picks from next_v, it reads V_b from it and M_b. from next_m,
 *   so the three TD entries above consume rewards_out as `rewards`, next_v as `next_q` and next_m as `next_quantiles` through the arguments
 *   they have.
 *
 *   Two facts follow and hold bit for bit: with A = 1 (Z = 1, logpi = 0, pi = 1) rewards_out == rewards and, on rows not done, next_v ==
 *   next_q and next_m == next_quantiles; with alpha = 0 rewards_out == rewards.
 *
 *   Limits: B >= 1, 1 <= A <= 64, Np = 0 with next_quantiles and next_m both NULL or 1 <= Np <= 64 with both given, alpha in [0, 1], tau
 *   finite and > 0, clip_lo finite and <= 0, no other pointer NULL.  Anything else is rejected before the launch with an ocrl_last_error
 *   message that names the limit.  The outputs may not overlap the inputs. */
#ifndef OCRL_HIP_MUNCHAUSEN_H
#define OCRL_HIP_MUNCHAUSEN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int ocrl_munchausen_targets(const float* cur_q /* [B, A] */, const float* next_q /* [B, A] */,
                            const float* next_quantiles /* [B, A, Np] or NULL */, int Np, const long long* actions, const float* rewards,
                            const unsigned char* dones, int B, int A, float alpha, float tau, float clip_lo, float* rewards_out /* [B] */,
                            float* next_v /* [B, A] */, float* next_m /* [B, A, Np], NULL iff next_quantiles is */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
