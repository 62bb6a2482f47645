/* C ABI of DQN's fully parameterized quantile function in libocrl_hip.so (gfx950): FQF (Yang, Zhao, Lin, Qin, Bian and Liu 2019).  The
 * fractions at which the implicit quantile head of ocrl_hip_iqn.h is evaluated are neither fixed nor drawn: a Linear on the features
 * followed by a soft-max proposes them per row, and is trained to minimise the 1-Wasserstein error of the staircase they make.  This
 * header holds what the head does not have: the proposal, the probability-weighted q, the collection step on proposed fractions and the
 * fraction loss's gradient into the proposal's Linear.  The head itself (ocrl_iqn_fwd, ocrl_iqn_bwd, ocrl_iqn_td_fwd_bwd) takes the
 * fractions as an input and is used unchanged.  A header beside ocrl_hip_iqn.h, self-contained and in the same dialect (ocrl_amd/_abi.py
 * reads them all); the conventions are ocrl_hip_iqn.h's: every entry is stateless and takes device pointers (fp32 unless said
 * otherwise), an `int` entry returns 0 on success and the message of a failure is ocrl_last_error(), every argument is checked before
 * any launch, work is enqueued on `stream` (a hipStream_t) with no host synchronisation, there are no atomics, every loop is bounded and
 * the results are bit-reproducible: partial sums are folded in a fixed order, and a row's forward results (ocrl_fqf_fractions,
 * ocrl_fqf_q, ocrl_fqf_act) do not depend on its position in the batch or on B.
 *
 * Limits: B >= 1, F (feature_dim) a multiple of 4 in 4 .. 256, 2 <= N (n_fractions) <= 32 so that the 2 N - 1 <= 63 fractions of
 *   eval_taus fit the head's 64 per row, 1 <= A (n_actions) <= 64; ocrl_fqf_act takes the head's other limits from ocrl_hip_iqn.h (C a
 *   multiple of 4 in 4 .. 64, 0 <= n <= 8, widths multiples of 4 up to 256); ent_coef finite.  Anything else is rejected before any
 *   launch: ocrl_fqf_ws_floats returns 0, the other entries non-zero, each with an ocrl_last_error message that names the limit.
 *   Every product and sum written below is one fp32 rounding unless it is written fmaf(a, b, c) = a * b + c rounded once, or said to be in fp64.
 *
 * ocrl_fqf_fractions: one launch, no workspace.  features [B, F], Wf [N, F], bf [N].  Per row, with x the row's features:
 *     z_i    = bf[i] + sum_j Wf[i, j] * x_j                                      -- in fp64 (the products are exact there), serial in
 *                                                                                   ascending j, starting from the bias
 *     m      = max_i z_i,  d_i = (float)(z_i - m)                                -- the difference in fp64, rounded to fp32 once: a logit
 *                                                                                   40 below the maximum keeps its digits in logp and H
 *     e_i    = expf(d_i)
 *     c_0    = 0,  c_{i+1} = c_i + e_i                                           -- the serial sum in ascending i;  Z = c_N
 *     logp_i = d_i - logf(Z),   p_i = expf(logp_i)
 *     tau_i  = c_i / Z,  i = 0 .. N                                              -- IEEE division
 *     tau_hat_i = 0.5 * (tau_i + tau_{i+1}),  i < N
 *     H      = -(sum_i p_i * logp_i), the sum serial in ascending i
 *   tau_i is the serial sum of p_0 .. p_{i-1} in exact arithmetic.  In fp32 it is formed on the un-normalised e and divided once, because
 *   that is what makes a row non-decreasing by construction and not by a clamp: e_i >= 0, so c_i <= c_{i+1} <= Z under rounding to
 *   nearest, division by the same Z > 0 keeps the order, tau_0 = 0 / Z = 0 and tau_N = Z / Z = 1 exactly.  (A serial sum of the rounded
 *   p_i can pass 1 by a few ulps before its last term when that term underflows.)  Some e_i and p_i may underflow to 0; logp stays
 *   finite for finite features and weights, and 0 * logp_i adds 0 to H.
 *   It writes taus [B, N + 1], tau_hats [B, N], eval_taus [B, 2 N - 1] = (tau_1 .. tau_{N-1}, then tau_hat_0 .. tau_hat_{N-1}: one block of
 *   fractions the head can be evaluated at, the same bits as the other two), logp [B, N] and entropy [B] (H).  Any output but taus may be
 *   NULL.
 *
 * ocrl_fqf_q: one launch.  quantiles [B, A, N] (theta: the head at tau_hats), taus [B, N + 1] ->
 *     q[b, a] = fmaf(tau_N - tau_{N-1}, theta[b, a, N-1], ... fmaf(tau_1 - tau_0, theta[b, a, 0], 0))     -- serial in ascending i
 *   Each difference is one fp32 rounding.
 *
 * ocrl_fqf_act: the collection step after ocrl_fqf_fractions, in one launch, no workspace: acting is two launches in all.  It is
 *   ocrl_iqn_act (d: the head's descriptor with N fractions per row; w: the head's 2 (n + 2) parameter pointers in ocrl_iqn_fwd's order)
 *   with the row's fractions tau_hat_i = 0.5 * (taus[b, i] + taus[b, i + 1]) derived from the given taus [B, N + 1], and with
 *   ocrl_fqf_q's fold in place of the mean: its q [B, A] (may be NULL) is bit for bit ocrl_fqf_q(ocrl_iqn_fwd(tau_hats), taus) on the
 *   same inputs.  The coin and the random action are ocrl_dqn_act's, word for word: row r takes two 24-bit uniforms of row
 *   R = row_offset + r of stream `seed`, with (x, y) the two 32-bit words of the library's counter RNG at site 410, key high word
 *   R >> 32, counter R & 0xffffffff,
 *     u0 = (x >> 8) / 2^24,  u1 = (y >> 8) / 2^24;   `uniforms` [B, 2] (u0, u1 per row, each k / 2^24) replaces the draw
 *     u0 < epsilon:  action = floor(u1 * A), computed on the 24 bits b = u1 * 2^24 as (b * A) >> 24;
 *     otherwise:     action = the lowest index of the maximum of q[r, :].
 *   actions: int64 [B].
 *
 * ocrl_fqf_fraction_bwd: the gradient of the fraction loss into the proposal's Linear, in two launches (the rows' terms into the slabs'
 *   partial sums, the fold of the slabs).  features [B, F]; logp [B, N] and entropy [B] as ocrl_fqf_fractions wrote them; quantiles
 *   [B, A, 2 N - 1] = the online head at eval_taus (no gradient); actions int64 [B], clamped into [0, A); weights [B] or NULL; ent_coef.
 *   Per row b, with a = actions[b], w_b = weights[b] or 1, theta(tau_i) = quantiles[b, a, i - 1], theta(tau_hat_i) = quantiles[b, a, N - 1 + i],
 *   p_k = expf(logp[b, k]) and H_b = entropy[b]:
 *     g_i   = (w_b / B) * (((2 * theta(tau_i)) - theta(tau_hat_i)) - theta(tau_hat_{i-1})),  i = 1 .. N-1     (the paper's dW1 / dtau_i)
 *     dp_k  = sum_{i = k+1 .. N-1} g_i, formed from the top: dp_{N-1} = 0, dp_k = dp_{k+1} + g_{k+1}           (tau_i = sum_{k<i} p_k)
 *     s     = sum_m p_m * dp_m, serial in ascending m
 *     dz_k  = p_k * (dp_k - s) + ((ent_coef / B) * p_k) * (logp_k + H_b)             (the second term is d(-ent_coef * mean H) / dz_k)
 *     l_b   = sum_{i = 1 .. N-1} g_i * t_i, ascending, with t_i the serial sum of p_0 .. p_{i-1}: products and sums in fp64 on the fp32 g_i, p_k
 *   dWf [N, F] = dz^T x, dbf [N] = sum_b dz, scalars [2] = (sum_b l_b: the fraction loss, reported only; (sum_b H_b) / B: the mean
 *   entropy): sums that cancel or run over the whole batch, reported only; they are carried in fp64 and rounded to fp32 once at the end.
 *   All four are overwritten, not accumulated.  The features receive no gradient: the proposal reads them detached.  The sums
 *   over the rows: groups of 8 rows are added in row order, slab s of S = min(ceil(B / 8), 16) takes the groups s, s + S, ... in
 *   ascending order, and the slabs are folded in slab order.  ws_floats >= ocrl_fqf_ws_floats(B, F, N) = S blocks of N * F + N + 4
 *   floats (the two fp64 sums first), each rounded up to a multiple of 64. */
#ifndef OCRL_HIP_FQF_H
#define OCRL_HIP_FQF_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the implicit quantile head's descriptor, field for field ocrl_hip_iqn.h's ocrl_iqn_desc: N = the proposed fractions per row */
typedef struct {
    int B, F, A, N, C, n;
    int dims[8];
    int acts[8];
} ocrl_fqf_desc;
size_t ocrl_fqf_desc_size(void);
size_t ocrl_fqf_ws_floats(int B, int F, int N);
int ocrl_fqf_fractions(const float* features, const float* Wf, const float* bf, int B, int F, int N, float* taus,
                       float* tau_hats /* may be NULL */, float* eval_taus /* may be NULL */, float* logp /* may be NULL */,
                       float* entropy /* may be NULL */, void* stream);
int ocrl_fqf_q(const float* quantiles, const float* taus, int B, int A, int N, float* q, void* stream);
int ocrl_fqf_act(const ocrl_fqf_desc* d, const float* features, const float* const* w, const float* taus, unsigned long long seed,
                 unsigned long long row_offset, float epsilon, const float* uniforms /* [B, 2] or NULL = draw */, long long* actions,
                 float* q /* may be NULL */, void* stream);
int ocrl_fqf_fraction_bwd(const float* features, const float* logp, const float* entropy, const float* quantiles, const long long* actions,
                          const float* weights /* may be NULL */, float ent_coef, int B, int F, int A, int N, float* dWf, float* dbf,
                          float* scalars, float* ws, size_t ws_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
