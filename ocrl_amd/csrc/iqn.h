// Kernel arguments and launchers of DQN's implicit quantile head (iqn.hip; C entry points in iqn_unit.cpp; include/ocrl_hip_iqn.h is the
// specification).  The head runs on the tile code over E = B * N expanded rows (row e = b * N + s: sample s of batch row b): in the
// AcnetArgs B is E, F the number of cosines, the cosine embedding Linear [F, C] (ReLU) is the one layer of the shared trunk (its saved
// output in the workspace is phi), the chain is the policy trunk, the output Linear [A, last] sits in wa / ba and there is no value
// head.  AcnetArgs::x is unused: the features are per batch row (IqnArgs::feat).  The fold of the partial dw is acnet_reduce_launch, the
// fold of the three scalars head_scalars_launch.
#pragma once
#include "../../include/ocrl_hip_iqn.h"
#include "acnet.h"
#include "dqn.h"

#define SITE_IQN_TAU 450u          // rng site of the sampled fractions (noisy.h has 440, sprite_env.h 500 ..)
#define IQN_MAX_SAMPLES 64
#define IQN_MAX_COS 64

// the batch behind the expanded rows and what a forward writes out (each may be null)
struct IqnArgs {
    int Bb, N, C;                                     // batch rows, fractions per row, cosines
    const float* feat;                                // features [Bb, F]
    const float* taus;                                // [Bb, N] (iqn_act: null = draw)
    float *theta, *q;                                 // [Bb, A, N] (`quantiles`, or the workspace's block when q alone is asked for), [Bb, A]
    const float* dquantiles;                          // iqn_bwd: [Bb, A, N]
    float* dzphi;                                     // [E, F] in the workspace: dz * phi per expanded row (null: no dfeatures)
    float* dfeat;                                     // dfeatures [Bb, F] or null
};

// the TD target's inputs: next_quantiles [Bb, A, Np], the shared ones (dqn.h, over the Bb batch rows) and the Huber threshold; part / tha
// [E] are the workspace's blocks
struct IqnTdArgs {
    const float* next_quantiles;
    int Np;
    QTdArgs row;
    float kappa;
    float *part, *tha;                                // (1 / Np) sum_j rho_ij and theta[b, a_b, i] of expanded row b * N + i
};

int iqn_taus_launch(unsigned long long seed, unsigned long long row_offset, int B, int N, float* out, hipStream_t st);
int iqn_fwd_launch(const AcnetArgs& a, const IqnArgs& c, hipStream_t st);                           // the tiles, and with c.q the fold over s
int iqn_act_launch(const AcnetArgs& a, const IqnArgs& c, const DqnActArgs& s, hipStream_t st);
// ocrl_fqf_act (include/ocrl_hip_fqf.h): the act kernel with c.taus = the fractions' boundaries [Bb, N + 1]; iqn_fqf_act (iqn_unit.cpp)
// checks the descriptor as ocrl_iqn_act does, under the caller's name, and launches it
int iqn_act_fqf_launch(const AcnetArgs& a, const IqnArgs& c, const DqnActArgs& s, hipStream_t st);
int iqn_fqf_act(const ocrl_iqn_desc* d, const char* who, const float* features, const float* const* w, const float* taus, const DqnActArgs& t,
                float* q, hipStream_t st);
int iqn_bwd_launch(const AcnetArgs& a, const IqnArgs& c, hipStream_t st);                           // the tiles, and with c.dfeat the fold over s
int iqn_td_launch(const AcnetArgs& a, const IqnArgs& c, const IqnTdArgs& s, hipStream_t st);        // the tiles, then the fold over s
