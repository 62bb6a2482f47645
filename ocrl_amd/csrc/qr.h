// Kernel arguments and launchers of DQN's quantile head (qr.hip; C entry points in qr_unit.cpp; include/ocrl_hip_qr.h is the
// specification).  The head is laid out as the categorical one (c51.h): the chain is the policy trunk of an AcnetArgs, the advantage
// Linear [A * N, last] sits in wa / ba and the dueling value Linear [N, last] in wv / bv (null: no dueling), each with its slab offsets;
// AcnetArgs::A is the number of actions.  The fold of the partial dw is acnet_reduce_launch, the fold of the three scalars
// head_scalars_launch.
#pragma once
#include "../../include/ocrl_hip_qr.h"
#include "acnet.h"
#include "dqn.h"

#define QR_MAX_QUANTILES 64
#define QR_MAX_COLS 256            // A * N: the quantile tile is one activation tile of acnet_tile.h

// the quantile count and what a forward writes out (each may be null)
struct QrArgs {
    int N;
    float *quantiles, *q;                             // [B, A, N], [B, A]
    const float* dquantiles;                          // qr_bwd: [B, A, N]
};

// the TD target's inputs: next_quantiles [B, A, N], the shared ones (dqn.h) and the Huber threshold
struct QrTdArgs {
    const float* next_quantiles;
    QTdArgs row;
    float kappa;
};

int qr_fwd_launch(const AcnetArgs& a, const QrArgs& c, hipStream_t st);
int qr_act_launch(const AcnetArgs& a, const QrArgs& c, const DqnActArgs& s, hipStream_t st);
int qr_bwd_launch(const AcnetArgs& a, const QrArgs& c, hipStream_t st);
int qr_td_launch(const AcnetArgs& a, const QrArgs& c, const QrTdArgs& s, hipStream_t st);
