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

// the TD target's inputs, each [B] but next_q and next_q_online [B, A]; the optional ones (null: not given) are read by the `ext` kernel
// alone
struct DqnTdArgs {
    const float* next_q;
    const long long* actions;
    const float* rewards;
    const unsigned char* dones;
    float gamma;
    const float* next_q_online;                       // optional: where the maximum is looked for (double Q-learning)
    const float* discounts;                           // optional: replaces gamma
    const float* weights;                             // optional: scales a row's loss and gradient
    float* abs_td;                                    // optional, out
};

// the TD inputs the distributional heads share (C51TdArgs, QrTdArgs and IqnTdArgs hold them as `row`; td_row of qhead_tile.h reads them):
// each [B] but next_q [B, A], where the bootstrap action is looked for
struct QTdArgs {
    const float* next_q;
    const long long* actions;
    const float* rewards;
    const unsigned char* dones;
    const float *discounts, *weights;                 // may be null
    float gamma;
    float* row_loss;                                  // may be null
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

int dqn_act_launch(const AcnetArgs& a, const DqnActArgs& s, hipStream_t st);
int dqn_act_uniforms_launch(unsigned long long seed, unsigned long long row_offset, long long n, float* out, hipStream_t st);
int dqn_td_launch(const AcnetArgs& a, const DqnTdArgs& s, bool ext, hipStream_t st);      // ext: the kernel that reads the optional inputs
// out[0..2] = the slabs' three scalar sums over B; count2: out[2] stays the sum (C51 and the classifier fold their scalars here too)
int head_scalars_launch(const float* scal_slab, int S, int B, bool count2, float* out, hipStream_t st);
int replay_gather_launch(const ReplayGatherArgs& g, hipStream_t st);
int replay_sample_launch(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, long long* idx, hipStream_t st);
