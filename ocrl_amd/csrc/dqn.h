// Kernel arguments and launchers of the DQN pieces (dqn.hip; C entry points in dqn_unit.cpp; include/ocrl_hip_dqn.h is the specification).
// The Q head runs on the actor-critic head's tile code (acnet_tile.h) as AcnetArgs with an empty shared trunk, the hidden layers as the
// policy trunk, the output Linear as the action head and no value head (wv == null); its plain forward is acnet_fwd_launch itself.
#pragma once
#include "../../include/ocrl_hip_dqn.h"
#include "acnet.h"

#define SITE_DQN_ACT 410u          // rng site of the exploration coin and the random action (acnet.h has 400, sprite_env.h 500 ..)
#define SITE_REPLAY_SAMPLE 420u    // rng site of the replay ring's draws

// the choice of dqn_act: row r draws (u0, u1) from (seed, row_offset + r) unless `uniforms` [B, 2] is given
struct DqnActArgs {
    unsigned long long seed, row_offset;
    float epsilon;
    const float* uniforms;
    long long* actions;                               // [B]
};

// the TD target's inputs, each [B] but next_q [B, A]
struct DqnTdArgs {
    const float* next_q;
    const long long* actions;
    const float* rewards;
    const unsigned char* dones;
    float gamma;
};

// the ring [N, E, ...] and one batch read of it
struct ReplayGatherArgs {
    const unsigned char* obs;
    const long long* actions;
    const float* rewards;
    const unsigned char* dones;
    int N, E, B;
    long long S;                                      // bytes of one observation
    const long long* idx;                             // [B] transition ids t * E + e
    unsigned char *obs_out, *next_out;                // [B, S]
    long long* actions_out;
    float* rewards_out;
    unsigned char* dones_out;
};

// the Q head's host side (dqn_unit.cpp), shared by the entry points of ocrl_hip_dqn.h and ocrl_hip_replay.h: the limits, the workspace's
// layout, the head as the tile code's arguments and the fold of the slabs' partial dw
namespace qnet {
struct QLay {
    size_t saved[ACNET_MAX_LAYERS], slab, scal, total;
    long long off[2 * ACNET_MAX_LAYERS + 3];
    int np, S, ntiles;
};
int check_qnet(const ocrl_qnet_desc* d, const char* who);
QLay q_layout(const ocrl_qnet_desc* d);
void fill_args(AcnetArgs& a, const ocrl_qnet_desc* d, const QLay& y, const float* x, const float* const* w, float* ws, bool saved);
int check_ptrs(const void* const* w, int np, const char* who);
int reduce_dw(const AcnetArgs& a, const QLay& y, float* const* dw, hipStream_t st);
}  // namespace qnet

int dqn_act_launch(const AcnetArgs& a, const DqnActArgs& s, hipStream_t st);
int dqn_act_uniforms_launch(unsigned long long seed, unsigned long long row_offset, long long n, float* out, hipStream_t st);
int dqn_td_launch(const AcnetArgs& a, const DqnTdArgs& s, hipStream_t st);
int dqn_scalars_launch(const float* scal_slab, int S, int B, float* out, hipStream_t st);
int replay_gather_launch(const ReplayGatherArgs& g, hipStream_t st);
int replay_sample_launch(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, long long* idx, hipStream_t st);
