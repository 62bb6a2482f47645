/* C ABI of the DQN pieces of libocrl_hip.so (gfx950): the Q head, the epsilon-greedy collection step, the fused TD step and the replay
 * ring's sampling and batch read.  A second header beside ocrl_hip.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads
 * both); the error convention is ocrl_hip.h's: every `int` entry returns 0 on success, the message of a failure is ocrl_last_error().
 *
 * Every entry is stateless, takes device pointers (fp32 unless said otherwise), enqueues on `stream` (a hipStream_t), never synchronises
 * with the host and uses no atomics.  Every loop is bounded and the results are bit-reproducible: partial sums are folded in a fixed
 * order, and a row's outputs do not depend on its position in the batch or on B.
 *
 * The Q head: features [B, F] -> n x [Linear(dims[l]), acts[l]] -> Linear(last, A) = q [B, A].  acts: 0 none, 1 ReLU, 2 tanh.
 *   w / dw: host arrays of 2 (n + 1) device pointers in state_dict order, (weight [out, in], bias [out]) per layer, then the output Linear.
 *   Limits (those of ocrl_acnet_desc): B >= 1, F >= 1, 1 <= A <= 64, 0 <= n <= 8, widths multiples of 4 up to 256.  Anything else is
 *   rejected before any launch: ocrl_qnet_ws_floats returns 0, the other entries non-zero, each with an ocrl_last_error message.
 *   Arithmetic: that of ocrl_acnet_* (exact fp32 products on the matrix pipe, a layer output = two k-interleaved chains + bias).
 *
 * ocrl_qnet_fwd: one launch.  save != 0 keeps the layer outputs in ws (ws_floats >= ocrl_qnet_ws_floats); save == 0 (the target
 *   network) needs no workspace.
 * ocrl_qnet_bwd: the cotangent dq [B, A] of a forward that ran with save != 0 on the same ws -> dw and dfeatures [B, F] (may be NULL),
 *   overwritten; two launches (the tiles' backward, the fold of the partial dw).
 *
 * ocrl_dqn_act: the collection step, forward and choice in one launch, no workspace.  Row r takes two 24-bit uniforms of row
 *   R = row_offset + r of stream `seed`: with (x, y) the two 32-bit words of the library's counter RNG at site 410, key high word
 *   R >> 32, counter R & 0xffffffff,
 *     u0 = (x >> 8) / 2^24,  u1 = (y >> 8) / 2^24       -- a pure function of (seed, R);
 *   `uniforms` [B, 2] (u0, u1 per row, each k / 2^24) replaces the draw.
 *     u0 < epsilon:  action = floor(u1 * A), computed on the 24 bits b = u1 * 2^24 as (b * A) >> 24;
 *     otherwise:     action = the lowest index of the maximum of q[r, :].
 *   So epsilon <= 0 never explores and epsilon >= 1 always does.  actions: int64 [B].  q [B, A] may be NULL.
 *   ocrl_dqn_act_uniforms writes out[i] = (u0, u1) of row row_offset + i, i < n: exactly what _act draws.
 *
 * ocrl_dqn_td_fwd_bwd: the whole gradient step of the head in three launches (the tiles' forward + loss + backward, the fold of the
 *   partial dw, the fold of the scalars).  Per row b, with a = actions[b] (int64) clamped into [0, A):
 *     y     = rewards[b] + (dones[b] ? 0 : gamma * max_a next_q[b, a])    -- a select: next_q of a finished row is never used
 *     delta = Q[b, a] - y
 *     l_b   = |delta| < 1 ? 0.5 delta^2 : |delta| - 0.5                   -- Huber, threshold 1
 *     loss  = mean_b l_b;   dQ[b, a] = clamp(delta, -1, 1) / B, zero elsewhere
 *   scalars [3] = loss, mean_b Q[b, a_b], mean_b y_b.  dones: uint8 [B].  dw (and dfeatures [B, F], may be NULL) are the gradients of
 *   `loss`, overwritten, not accumulated.  ws_floats >= ocrl_qnet_ws_floats.
 *
 * The replay ring: obs [N, E, S bytes], actions int64 [N, E], rewards fp32 [N, E], dones uint8 [N, E]; slot t holds one step of E
 *   environments, S = the byte size of one observation, a multiple of 4 (uint8 frames [3, H, W] or fp32 state rows).  The observation
 *   after slot t's step is stored in slot (t + 1) % N (the writer keeps that invariant).
 * ocrl_replay_gather: one launch.  idx int64 [B] holds transition ids t * E + e; an id outside [0, N * E) is clamped into range.
 *     obs_out [B, S] = obs[t, e], next_obs_out [B, S] = obs[(t + 1) % N, e], actions_out / rewards_out / dones_out [B] = slot t's.
 *   16-byte accesses when S % 16 == 0 (the pointers then must be 16-byte aligned), 4-byte accesses otherwise (4-byte aligned).
 * ocrl_replay_sample: idx[r], r < B, of update `update`: with (x, y) the counter RNG's words at site 420, key high word
 *   update & 0xffffffff, counter r, and below(w, m) = (w * m) >> 32 on 64-bit integers,
 *     full == 0:  t = below(x, pos)                             -- slots 0 .. pos - 1 (pos >= 1)
 *     full != 0:  t = (pos + 1 + below(x, N - 1)) % N           -- every slot but pos
 *     e = below(y, E);  idx[r] = t * E + e                      -- a pure function of (seed, update, r)
 *   pos is the slot the next write goes to, 0 <= pos < N; N >= 2, E >= 1, B >= 1, N * E < 2^31. */
#ifndef OCRL_HIP_DQN_H
#define OCRL_HIP_DQN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int B, F, A, n;
    int dims[8];
    int acts[8];
} ocrl_qnet_desc;
size_t ocrl_qnet_desc_size(void);
size_t ocrl_qnet_ws_floats(const ocrl_qnet_desc* d);
int ocrl_qnet_fwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, float* q, int save, float* ws, size_t ws_floats,
                  void* stream);
int ocrl_qnet_bwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, const float* dq, float* dfeatures /* may be NULL */,
                  float* const* dw, float* ws, size_t ws_floats, void* stream);
int ocrl_dqn_act(const ocrl_qnet_desc* d, const float* features, const float* const* w, unsigned long long seed,
                 unsigned long long row_offset, float epsilon, const float* uniforms /* [B, 2] or NULL = draw */, long long* actions,
                 float* q /* may be NULL */, void* stream);
int ocrl_dqn_act_uniforms(unsigned long long seed, unsigned long long row_offset, long long n, float* out, void* stream);
int ocrl_dqn_td_fwd_bwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, const float* next_q, const long long* actions,
                        const float* rewards, const unsigned char* dones, float gamma, float* scalars, float* dfeatures /* may be NULL */,
                        float* const* dw, float* ws, size_t ws_floats, void* stream);
int ocrl_replay_gather(const void* obs, const long long* actions, const float* rewards, const unsigned char* dones, int N, int E,
                       long long S, const long long* idx, int B, void* obs_out, void* next_obs_out, long long* actions_out,
                       float* rewards_out, unsigned char* dones_out, void* stream);
int ocrl_replay_sample(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, long long* idx,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
