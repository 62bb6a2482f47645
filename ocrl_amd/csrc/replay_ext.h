// Kernel arguments and launchers of DQN's replay extensions (replay_ext.hip; C entry points in replay_ext_unit.cpp;
// include/ocrl_hip_replay.h is the specification): the n-step sampling and batch read and the priority store; the
// extended TD step is dqn_td_launch of dqn.h.
#pragma once
#include "dqn.h"

#define SITE_PER_SAMPLE 430u       // rng site of the priority store's draws (dqn.h has 410 and 420)
#define REPLAY_MAX_NSTEP 16
#define PER_FAN 64                 // children per node of the priority store: one wave reads a node's children, one lane each
#define PER_MAX_LEVELS 6           // ceil(31 / 6): levels of sums above fewer than 2^31 leaves
#define PER_Q_ONE 65536u           // the fixed point's 1
#define PER_Q_MAX 16777216u        // 2^24: the largest stored priority (exact as a float)

struct ReplayGatherNstepArgs {
    ReplayGatherArgs g;                               // rewards_out takes the returns
    int n;
    float gamma;
    float* discounts_out;
};

// the priority store's buffer, taken apart: n[0] = NE leaves, n[l] nodes of level l = 1 .. L, lvl[l - 1] their sums; n[L] == 1
struct PerTree {
    uint32_t* leaves;
    uint32_t* maxq;
    unsigned long long* lvl[PER_MAX_LEVELS];
    long long n[PER_MAX_LEVELS + 1];
    int L;
    long long words;                                  // 32-bit words of the whole buffer
};

int replay_sample_nstep_launch(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, int n, long long* idx,
                               hipStream_t st);
int replay_gather_nstep_launch(const ReplayGatherNstepArgs& a, hipStream_t st);
int per_init_launch(const PerTree& t, hipStream_t st);
int per_set_range_launch(const PerTree& t, long long first, long long count, int mode, hipStream_t st);
int per_update_launch(const PerTree& t, const long long* idx, const float* abs_td, int B, float alpha, float eps, hipStream_t st);
int per_sample_launch(const PerTree& t, unsigned long long seed, unsigned long long update, int B, float beta, const unsigned long long* targets,
                      long long* idx, float* weights, hipStream_t st);
