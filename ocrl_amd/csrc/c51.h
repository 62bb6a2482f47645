// Kernel arguments and launchers of DQN's categorical head (c51.hip; C entry points in c51_unit.cpp; include/ocrl_hip_c51.h is the
// specification).  The chain runs on the actor-critic head's per-layer tile steps (acnet_tile.h) as the policy trunk of an AcnetArgs;
// the advantage Linear [A * Z, last] sits in wa / ba and the dueling value Linear [Z, last] in wv / bv (null: no dueling), each with its
// slab offsets; AcnetArgs::A is the number of actions.  The fold of the partial dw is acnet_reduce_launch, the fold of the three scalars
// head_scalars_launch.
#pragma once
#include "../../include/ocrl_hip_c51.h"
#include "acnet.h"
#include "dqn.h"

#define C51_MAX_ATOMS 64
#define C51_MAX_COLS 256           // A * Z: the logits tile is one activation tile of acnet_tile.h

// the support and what a forward writes out (each may be null)
struct C51Args {
    int Z;
    float v_min, v_max, dz;
    float *logits, *probs, *q;                        // [B, A, Z], [B, A, Z], [B, A]
    const float* dlogits;                             // c51_bwd: [B, A, Z]
};

// the TD target's inputs: next_probs [B, A, Z] and the shared ones (dqn.h)
struct C51TdArgs {
    const float* next_probs;
    QTdArgs row;
};

int c51_fwd_launch(const AcnetArgs& a, const C51Args& c, hipStream_t st);
int c51_act_launch(const AcnetArgs& a, const C51Args& c, const DqnActArgs& s, hipStream_t st);
int c51_bwd_launch(const AcnetArgs& a, const C51Args& c, hipStream_t st);
int c51_td_launch(const AcnetArgs& a, const C51Args& c, const C51TdArgs& s, hipStream_t st);
