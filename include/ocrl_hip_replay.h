/* C ABI of DQN's replay extensions in libocrl_hip.so (gfx950): n-step returns read from the ring, the TD step with double Q-learning,
 * per-row discounts and importance weights, and a proportional priority store with its sampler and update.  A fourth header beside
 * ocrl_hip.h, ocrl_hip_dqn.h and ocrl_hip_rollout.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads them all); the
 * conventions are ocrl_hip_dqn.h's: every entry is stateless and takes device pointers, an `int` entry returns 0 on success and the
 * message of a failure is ocrl_last_error(), arguments are checked before any launch, work is enqueued on `stream` (a hipStream_t) with
 * no host synchronisation, there are no atomics, every loop is bounded and the results are bit-reproducible.
 *
 * The ring is ocrl_hip_dqn.h's: obs [N, E, S bytes], actions int64 [N, E], rewards fp32 [N, E], dones uint8 [N, E]; slot t + k holds
 * step t + k of the same environment, so an n-step return is a read.  below(w, m) = (w * m) >> 32 on 64-bit integers.
 *
 * ocrl_replay_sample_nstep: ocrl_replay_sample's rule restricted to the slots whose whole n-step window is stored; the same words
 *   (x, y) of site 420, key high word update & 0xffffffff, counter r:
 *     full == 0:  t = below(x, pos - n + 1)                     -- slots 0 .. pos - n (pos >= n)
 *     full != 0:  t = (pos + 1 + below(x, N - n)) % N           -- every slot but pos and the n - 1 before it
 *     e = below(y, E);  idx[r] = t * E + e
 *   1 <= n <= 16, n < N; the other limits are ocrl_replay_sample's.  At n == 1 the result is ocrl_replay_sample's bit for bit.
 *
 * ocrl_replay_gather_nstep: one launch.  For id t * E + e (clamped into [0, N * E)) walk k = 0 .. n - 1 over the slots (t + k) % N:
 *     R = 0; g = 1;   per step  R = R + g * r_k;  g = g * gamma;   stop after the first k whose dones is set
 *   each product and sum rounded to fp32 on its own, in that order (no contraction: a numpy float32 loop matches bit for bit).  With m
 *   the number of steps taken: returns_out = R, discounts_out = g (gamma^m), dones_out = whether the walk stopped on a done,
 *   next_obs_out = obs[(t + m) % N, e], obs_out and actions_out = slot t's.  Access widths and alignment: ocrl_replay_gather's.  At
 *   n == 1 obs, next_obs, actions and dones are ocrl_replay_gather's bit for bit, and so are the returns (0 + 1 * r; a reward of -0.0
 *   comes back as +0.0).
 *
 * ocrl_dqn_td_fwd_bwd_ext: ocrl_dqn_td_fwd_bwd with four optional per-row arrays, each may be NULL.  Per row b, a = actions[b] clamped:
 *     a*    = the lowest index of the maximum of next_q_online[b, :] when that is given, else of next_q[b, :]
 *     y     = rewards[b] + (dones[b] ? 0 : disc_b * next_q[b, a*]),   disc_b = discounts[b] or gamma
 *     delta = Q[b, a] - y;   l_b = w_b * huber(delta),   w_b = weights[b] or 1
 *     dQ[b, a] = w_b * clamp(delta, -1, 1) / B;   abs_td[b] = |delta|
 *   scalars [3] = mean l_b, mean Q[b, a_b], mean y_b.  With all four NULL every output is ocrl_dqn_td_fwd_bwd's bit for bit; the three
 *   launches and the workspace (ocrl_qnet_ws_floats) are that entry's.  `d` points to an ocrl_qnet_desc of ocrl_hip_dqn.h (this header
 *   stays self-contained and declares no struct of its own: the pointer is a `const void*` here).
 *
 * The priority store: one buffer of ocrl_per_bytes(NE) bytes, 8-byte aligned, 1 <= NE < 2^31, for NE transition ids:
 *     uint32 leaves[NE]            a leaf q = the fixed-point priority of an id; 0 = not sampleable
 *     uint32 maxq                  the largest priority written so far (the priority of a new transition)
 *     4 bytes of padding when NE is even, so that what follows starts on a multiple of 8 bytes
 *     uint64 level_1[n_1], level_2[n_2], ... level_L[1]     n_0 = NE, n_l = ceil(n_{l-1} / 64), up to the first level of one node
 *   node j of level l is the exact integer sum of nodes 64 j .. 64 j + 63 of level l - 1 (the leaves for l = 1); the last level's one
 *   node is the total.  The sums are integers: they do not depend on the order of summation.
 *   A priority v is stored as q = clamp(floor(v * 65536 + 0.5), 1, 2^24), v = (|delta| + eps)^alpha in fp32 (the sum, the product by
 *   65536 and the + 0.5 each rounded on their own); alpha == 1 takes v = |delta| + eps without powf, alpha == 0 takes v = 1; a value
 *   that is not finite gives 2^24.
 * ocrl_per_init: all leaves and sums 0, maxq = 65536 (priority 1).  One launch.
 * ocrl_per_set_range: leaves first .. first + count - 1 (inside [0, NE), count >= 1): mode 0 writes 0, mode 1 writes the current maxq;
 *   the sums above them are rebuilt.  Two launches (one when NE <= 64).
 * ocrl_per_update: q_b of (abs_td[b], alpha, eps) goes to leaves[idx[b]] (int64 ids, clamped into [0, NE)) where that leaf is non-zero: a
 *   zero leaf stays zero; maxq = max(maxq, max_b q_b) over every row; the sums above the touched leaves are rebuilt from the leaves.
 *   Duplicate ids must carry identical values (a row's TD error does not depend on its position in the batch): they are written
 *   twice.  One launch of one workgroup.
 * ocrl_per_sample: row r takes (x, y) of site 430, key high word update & 0xffffffff, counter r:
 *     target = ((x << 32 | y) * total) >> 64                    -- uniform over [0, total); `targets` (uint64 [B], may be NULL)
 *                                                                  replaces the draw, clamped to total - 1
 *     idx[r] = the smallest i with leaves[0] + .. + leaves[i] > target     -- exact; never an id whose leaf is 0
 *     weights[r] = ((float)q_min / (float)q_r)^beta,  q_r = leaves[idx[r]], q_min = the smallest q_r of this batch
 *   the importance weight (1 / (NE P(i)))^beta divided by the batch's largest; beta == 0 gives 1 exactly, beta == 1 the quotient
 *   without powf.  An empty store (total == 0) is the caller's error and cannot be reported without a host read: every row then gets
 *   idx -1 and weight 0.  Two launches.  idx int64 [B], weights fp32 [B]. */
#ifndef OCRL_HIP_REPLAY_H
#define OCRL_HIP_REPLAY_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int ocrl_replay_sample_nstep(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, int n, long long* idx,
                             void* stream);
int ocrl_replay_gather_nstep(const void* obs, const long long* actions, const float* rewards, const unsigned char* dones, int N, int E,
                             long long S, int n, float gamma, const long long* idx, int B, void* obs_out, void* next_obs_out,
                             long long* actions_out, float* returns_out, unsigned char* dones_out, float* discounts_out, void* stream);
int ocrl_dqn_td_fwd_bwd_ext(const void* d /* an ocrl_qnet_desc */, const float* features, const float* const* w, const float* next_q,
                            const float* next_q_online /* may be NULL */, const long long* actions, const float* rewards,
                            const unsigned char* dones, const float* discounts /* may be NULL */, const float* weights /* may be NULL */,
                            float gamma, float* scalars, float* abs_td /* may be NULL */, float* dfeatures /* may be NULL */, float* const* dw,
                            float* ws, size_t ws_floats, void* stream);
size_t ocrl_per_bytes(long long NE);
int ocrl_per_init(void* tree, long long NE, void* stream);
int ocrl_per_set_range(void* tree, long long NE, long long first, long long count, int mode, void* stream);
int ocrl_per_update(void* tree, long long NE, const long long* idx, const float* abs_td, int B, float alpha, float eps, void* stream);
int ocrl_per_sample(void* tree, long long NE, unsigned long long seed, unsigned long long update, int B, float beta,
                    const unsigned long long* targets /* may be NULL */, long long* idx, float* weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif
