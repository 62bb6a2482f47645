// C ABI of the DQN pieces (include/ocrl_hip_dqn.h: ocrl_qnet_*, ocrl_dqn_*, ocrl_replay_*).  Stateless: the caller owns parameters,
// gradients, the ring and the workspace.  Parameter order (w, dw): (weight, bias) per hidden layer, then the output Linear's.
#include "../../include/ocrl_hip_dqn.h"
#include "acnet_host.h"
#include "dqn.h"

extern "C" {

size_t ocrl_qnet_desc_size(void) { return sizeof(ocrl_qnet_desc); }

size_t ocrl_qnet_ws_floats(const ocrl_qnet_desc* d) {
    if (check_qnet(d, "ocrl_qnet_ws_floats")) return 0;                // the shapes the other entries reject get no workspace
    return head_layout(qnet_spec(d)).total;
}

int ocrl_qnet_fwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, float* q, int save, float* ws, size_t ws_floats,
                  void* stream) {
    const char* who = "ocrl_qnet_fwd";
    RC(check_qnet(d, who));
    const HeadSpec s = qnet_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && q, "%s: null argument", who);
    RC(check_ptrs(w, y.np, who));
    if (save) RC(ws_check(who, ws ? ws_floats : (size_t)0, y.total));
    AcnetArgs a;
    head_args(a, s, y, features, w, save ? ws : nullptr, save != 0);
    a.logits = q;
    return acnet_fwd_launch(a, static_cast<hipStream_t>(stream));
}

int ocrl_qnet_bwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, const float* dq, float* dfeatures, float* const* dw, float* ws,
                  size_t ws_floats, void* stream) {
    const char* who = "ocrl_qnet_bwd";
    RC(check_qnet(d, who));
    const HeadSpec s = qnet_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && dq && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    a.dlogits = dq; a.dx = dfeatures;
    RC(acnet_bwd_launch(a, st));
    return reduce_dw(a, y, dw, st);
}

int ocrl_dqn_act(const ocrl_qnet_desc* d, const float* features, const float* const* w, unsigned long long seed, unsigned long long row_offset,
                 float epsilon, const float* uniforms, long long* actions, float* q, void* stream) {
    const char* who = "ocrl_dqn_act";
    RC(check_qnet(d, who));
    const HeadSpec s = qnet_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && actions, "%s: null argument", who);
    RC(check_ptrs(w, y.np, who));
    AcnetArgs a;
    head_args(a, s, y, features, w, nullptr, false);
    a.logits = q;
    const DqnActArgs t{seed, row_offset, epsilon, uniforms, actions};
    return dqn_act_launch(a, t, static_cast<hipStream_t>(stream));
}

int ocrl_dqn_act_uniforms(unsigned long long seed, unsigned long long row_offset, long long n, float* out, void* stream) {
    OCRL_REQUIRE(out && n >= 1, "ocrl_dqn_act_uniforms: null output or n < 1 (got %lld)", n);
    return dqn_act_uniforms_launch(seed, row_offset, n, out, static_cast<hipStream_t>(stream));
}

int ocrl_dqn_td_fwd_bwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, const float* next_q, const long long* actions,
                        const float* rewards, const unsigned char* dones, float gamma, float* scalars, float* dfeatures, float* const* dw, float* ws,
                        size_t ws_floats, void* stream) {
    const char* who = "ocrl_dqn_td_fwd_bwd";
    RC(check_qnet(d, who));
    const HeadSpec s = qnet_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && next_q && actions && rewards && dones && scalars && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    a.dx = dfeatures;
    const DqnTdArgs t{next_q, actions, rewards, dones, gamma, nullptr, nullptr, nullptr, nullptr};
    RC(dqn_td_launch(a, t, false, st));
    RC(reduce_dw(a, y, dw, st));
    return head_scalars_launch(a.scal_slab, y.S, d->B, false, scalars, st);
}

int ocrl_replay_gather(const void* obs, const long long* actions, const float* rewards, const unsigned char* dones, int N, int E, long long S,
                       const long long* idx, int B, void* obs_out, void* next_obs_out, long long* actions_out, float* rewards_out,
                       unsigned char* dones_out, void* stream) {
    OCRL_REQUIRE(obs && actions && rewards && dones && idx && obs_out && next_obs_out && actions_out && rewards_out && dones_out,
                 "ocrl_replay_gather: null argument");
    OCRL_REQUIRE(N >= 2 && E >= 1 && B >= 1 && (long long)N * E < (1LL << 31), "ocrl_replay_gather: slots >= 2, envs >= 1, batch >= 1 and slots * envs < 2^31 (got %d, %d, %d)",
                 N, E, B);
    OCRL_REQUIRE(S >= 4 && S % 4 == 0, "ocrl_replay_gather: the byte size of an observation is a positive multiple of 4 (got %lld)", S);
    const uintptr_t al = (uintptr_t)obs | (uintptr_t)obs_out | (uintptr_t)next_obs_out;
    OCRL_REQUIRE((al & (S % 16 == 0 ? 15 : 3)) == 0, "ocrl_replay_gather: observation pointers must be %d-byte aligned for observations of %lld bytes",
                 S % 16 == 0 ? 16 : 4, S);
    const ReplayGatherArgs g{static_cast<const unsigned char*>(obs), actions, rewards, dones, N, E, B, S, idx, static_cast<unsigned char*>(obs_out),
                             static_cast<unsigned char*>(next_obs_out), actions_out, rewards_out, dones_out};
    return replay_gather_launch(g, static_cast<hipStream_t>(stream));
}

int ocrl_replay_sample(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, long long* idx, void* stream) {
    OCRL_REQUIRE(idx, "ocrl_replay_sample: null argument");
    OCRL_REQUIRE(N >= 2 && E >= 1 && B >= 1 && (long long)N * E < (1LL << 31), "ocrl_replay_sample: slots >= 2, envs >= 1, batch >= 1 and slots * envs < 2^31 (got %d, %d, %d)",
                 N, E, B);
    OCRL_REQUIRE(pos >= 0 && pos < N && (full || pos >= 1), "ocrl_replay_sample: 0 <= pos < slots, and pos >= 1 while the ring is not full (got pos %d of %d, full %d)",
                 pos, N, full);
    return replay_sample_launch(seed, update, B, N, E, pos, full, idx, static_cast<hipStream_t>(stream));
}

}  // extern "C"
