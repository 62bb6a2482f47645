// Kernel arguments and launcher of DQN's Munchausen targets (munchausen.hip; C entry point in munchausen_unit.cpp;
// include/ocrl_hip_munchausen.h is the specification).  One launch in front of the unchanged TD kernels: it rewrites the rewards and the
// target network's values at the next observation.
#pragma once
#include "../../include/ocrl_hip_munchausen.h"
#include "common.h"

#define MUNCHAUSEN_MAX_ACTIONS 64
#define MUNCHAUSEN_MAX_SAMPLES 64

struct MunchausenArgs {
    const float *cur_q, *next_q;                      // [B, A]: the target network at the observations, at the next observations
    const float* next_quantiles;                      // [B, A, Np] or null (Np == 0)
    const long long* actions;
    const float* rewards;
    const unsigned char* dones;
    int B, A, Np;
    float alpha, tau, clip_lo;
    float *rewards_out, *next_v, *next_m;             // [B], [B, A], [B, A, Np] or null
};

int munchausen_launch(const MunchausenArgs& a, hipStream_t st);
