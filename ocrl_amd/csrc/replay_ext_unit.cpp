// C ABI of DQN's replay extensions (include/ocrl_hip_replay.h: ocrl_replay_*_nstep, ocrl_dqn_td_fwd_bwd_ext, ocrl_per_*).  Stateless: the
// caller owns the ring, the priority store's buffer, parameters, gradients and the workspace.  The Q head's host side is acnet_host.h's.
#include "../../include/ocrl_hip_replay.h"
#include "acnet_host.h"
#include "replay_ext.h"

namespace {

int check_ring(int N, int E, int B, const char* who) {
    OCRL_REQUIRE(N >= 2 && E >= 1 && B >= 1 && (long long)N * E < (1LL << 31), "%s: slots >= 2, envs >= 1, batch >= 1 and slots * envs < 2^31 (got %d, %d, %d)", who,
                 N, E, B);
    return 0;
}

int check_nstep(int n, int N, const char* who) {
    OCRL_REQUIRE(n >= 1 && n <= REPLAY_MAX_NSTEP && n < N, "%s: 1 <= n <= %d and n < slots (got n %d of %d slots)", who, REPLAY_MAX_NSTEP, n, N);
    return 0;
}

// the layout of include/ocrl_hip_replay.h over `tree` (null: the sizes alone)
int per_tree(PerTree& t, void* tree, long long NE, const char* who) {
    OCRL_REQUIRE(NE >= 1 && NE < (1LL << 31), "%s: 1 <= NE < 2^31 transition ids (got %lld)", who, NE);
    OCRL_REQUIRE(((uintptr_t)tree & 7) == 0, "%s: the store's buffer must be 8-byte aligned", who);
    t = PerTree{};
    unsigned char* base = static_cast<unsigned char*>(tree);
    t.leaves = reinterpret_cast<uint32_t*>(base);
    t.maxq = t.leaves + NE;
    size_t off = ((size_t)(NE + 1) * 4 + 7) & ~(size_t)7;
    t.n[0] = NE;
    long long n = NE;
    do {
        n = (n + PER_FAN - 1) / PER_FAN;
        t.lvl[t.L] = reinterpret_cast<unsigned long long*>(base + off);
        t.n[++t.L] = n;
        off += (size_t)n * 8;
    } while (n > 1);
    t.words = (long long)(off / 4);
    return 0;
}

}  // namespace

extern "C" {

int ocrl_replay_sample_nstep(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, int n, long long* idx,
                             void* stream) {
    const char* who = "ocrl_replay_sample_nstep";
    OCRL_REQUIRE(idx, "%s: null argument", who);
    RC(check_ring(N, E, B, who));
    RC(check_nstep(n, N, who));
    OCRL_REQUIRE(pos >= 0 && pos < N && (full || pos >= n), "%s: 0 <= pos < slots, and pos >= n while the ring is not full (got pos %d of %d, full %d, n %d)", who,
                 pos, N, full, n);
    return replay_sample_nstep_launch(seed, update, B, N, E, pos, full, n, idx, static_cast<hipStream_t>(stream));
}

int ocrl_replay_gather_nstep(const void* obs, const long long* actions, const float* rewards, const unsigned char* dones, int N, int E, long long S,
                             int n, float gamma, const long long* idx, int B, void* obs_out, void* next_obs_out, long long* actions_out,
                             float* returns_out, unsigned char* dones_out, float* discounts_out, void* stream) {
    const char* who = "ocrl_replay_gather_nstep";
    OCRL_REQUIRE(obs && actions && rewards && dones && idx && obs_out && next_obs_out && actions_out && returns_out && dones_out && discounts_out,
                 "%s: null argument", who);
    RC(check_ring(N, E, B, who));
    RC(check_nstep(n, N, who));
    OCRL_REQUIRE(S >= 4 && S % 4 == 0, "%s: the byte size of an observation is a positive multiple of 4 (got %lld)", who, S);
    const uintptr_t al = (uintptr_t)obs | (uintptr_t)obs_out | (uintptr_t)next_obs_out;
    OCRL_REQUIRE((al & (S % 16 == 0 ? 15 : 3)) == 0, "%s: observation pointers must be %d-byte aligned for observations of %lld bytes", who,
                 S % 16 == 0 ? 16 : 4, S);
    ReplayGatherNstepArgs a{};
    a.g = ReplayGatherArgs{static_cast<const unsigned char*>(obs), actions, rewards, dones, N, E, B, S, idx, static_cast<unsigned char*>(obs_out),
                           static_cast<unsigned char*>(next_obs_out), actions_out, returns_out, dones_out};
    a.n = n; a.gamma = gamma; a.discounts_out = discounts_out;
    return replay_gather_nstep_launch(a, static_cast<hipStream_t>(stream));
}

int ocrl_dqn_td_fwd_bwd_ext(const void* dv, const float* features, const float* const* w, const float* next_q, const float* next_q_online,
                            const long long* actions, const float* rewards, const unsigned char* dones, const float* discounts, const float* weights,
                            float gamma, float* scalars, float* abs_td, float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_dqn_td_fwd_bwd_ext";
    const ocrl_qnet_desc* d = static_cast<const ocrl_qnet_desc*>(dv);
    RC(check_qnet(d, who));
    const HeadSpec s = qnet_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && next_q && actions && rewards && dones && scalars && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    a.dx = dfeatures;
    const DqnTdArgs t{next_q, actions, rewards, dones, gamma, next_q_online, discounts, weights, abs_td};
    RC(dqn_td_launch(a, t, true, st));
    RC(reduce_dw(a, y, dw, st));
    return head_scalars_launch(a.scal_slab, y.S, d->B, false, scalars, st);
}

size_t ocrl_per_bytes(long long NE) {
    PerTree t;
    if (per_tree(t, nullptr, NE, "ocrl_per_bytes")) return 0;
    return (size_t)t.words * 4;
}

int ocrl_per_init(void* tree, long long NE, void* stream) {
    OCRL_REQUIRE(tree, "ocrl_per_init: null argument");
    PerTree t;
    RC(per_tree(t, tree, NE, "ocrl_per_init"));
    return per_init_launch(t, static_cast<hipStream_t>(stream));
}

int ocrl_per_set_range(void* tree, long long NE, long long first, long long count, int mode, void* stream) {
    OCRL_REQUIRE(tree, "ocrl_per_set_range: null argument");
    PerTree t;
    RC(per_tree(t, tree, NE, "ocrl_per_set_range"));
    OCRL_REQUIRE(first >= 0 && count >= 1 && first < NE && count <= NE - first, "ocrl_per_set_range: leaves first .. first + count - 1 inside [0, NE) (got first %lld, count %lld, NE %lld)",
                 first, count, NE);
    OCRL_REQUIRE(mode == 0 || mode == 1, "ocrl_per_set_range: mode 0 (zero) or 1 (the running maximum) (got %d)", mode);
    return per_set_range_launch(t, first, count, mode, static_cast<hipStream_t>(stream));
}

int ocrl_per_update(void* tree, long long NE, const long long* idx, const float* abs_td, int B, float alpha, float eps, void* stream) {
    OCRL_REQUIRE(tree && idx && abs_td, "ocrl_per_update: null argument");
    PerTree t;
    RC(per_tree(t, tree, NE, "ocrl_per_update"));
    OCRL_REQUIRE(B >= 1, "ocrl_per_update: batch >= 1 (got %d)", B);
    OCRL_REQUIRE(alpha >= 0.f && alpha <= 1.f && eps >= 0.f, "ocrl_per_update: 0 <= alpha <= 1 and eps >= 0 (got %g, %g)", (double)alpha, (double)eps);
    return per_update_launch(t, idx, abs_td, B, alpha, eps, static_cast<hipStream_t>(stream));
}

int ocrl_per_sample(void* tree, long long NE, unsigned long long seed, unsigned long long update, int B, float beta, const unsigned long long* targets,
                    long long* idx, float* weights, void* stream) {
    OCRL_REQUIRE(tree && idx && weights, "ocrl_per_sample: null argument");
    PerTree t;
    RC(per_tree(t, tree, NE, "ocrl_per_sample"));
    OCRL_REQUIRE(B >= 1, "ocrl_per_sample: batch >= 1 (got %d)", B);
    OCRL_REQUIRE(beta >= 0.f && beta <= 1.f, "ocrl_per_sample: 0 <= beta <= 1 (got %g)", (double)beta);
    return per_sample_launch(t, seed, update, B, beta, targets, idx, weights, static_cast<hipStream_t>(stream));
}

}  // extern "C"
