// Kernel arguments and launchers of the actor-critic head (acnet.hip; C entry points in acnet_unit.cpp).
#pragma once
#include "common.h"

#define ACNET_MAX_LAYERS 8      // per trunk (OCRL_ACNET_MAX_LAYERS)
#define ACNET_MAX_WIDTH 256     // of a trunk layer
#define ACNET_MAX_ACTIONS 64
#define ACNET_MAX_SLABS 64      // partial-gradient slabs: workgroup s walks the row tiles s, s + S, ...
#define SITE_ACNET_ACT 400u     // rng site of the action draw (common.h keeps the encoder's sites below 300, pool_unit.cpp 300 .. 399)
#define ACNET_NPARAM (2 * (3 * ACNET_MAX_LAYERS + 2))

// trunks: 0 = shared, 1 = policy, 2 = value.  act: 0 none, 1 ReLU, 2 tanh.  Every pointer is fp32 device memory.
struct AcnetArgs {
    int B, F, A;                                      // A == 0: no heads (the trunks alone, CustomNetwork)
    int n[3], dim[3][ACNET_MAX_LAYERS], act[3][ACNET_MAX_LAYERS];
    const float* w[3][ACNET_MAX_LAYERS];
    const float* b[3][ACNET_MAX_LAYERS];
    const float *wa, *ba, *wv, *bv;                   // action_net [A, latent_pi], value_net [1, latent_vf] (wv null: no value head, dqn.h)
    const float* x;                                   // features [B, F]
    float *logits, *values, *lat_pi, *lat_vf;         // forward outputs (each may be null)
    float* saved[3][ACNET_MAX_LAYERS];                // layer outputs [B, dim] in the workspace (null: not kept)
    // backward
    const float *dlogits, *dvalues, *dlat_pi, *dlat_vf;
    float* dx;                                        // dfeatures [B, F] or null
    float* slab;                                      // [S][slab_stride] partial parameter gradients
    long long slab_stride, off_w[3][ACNET_MAX_LAYERS], off_b[3][ACNET_MAX_LAYERS], off_wa, off_ba, off_wv, off_bv;
    int S, ntiles;
    // PPO and A2C (A2C reads neither old_logp nor clip)
    const long long* actions;
    const float *old_logp, *adv, *ret, *stats;        // stats: {mean, 1 / (std + 1e-8)} of the advantages
    float clip, vf_coef, ent_coef;
    int norm;
    float* scal_slab;                                 // [S][8] partial sums of the scalars (PPO five, A2C three)
};

// the sampling tail of acnet_act: row r draws from (seed, row_offset + r) unless `uniforms` [B] is given
struct AcnetActArgs {
    unsigned long long seed, row_offset;
    const float* uniforms;
    int deterministic;                                // the lowest index of the maximum logit instead of a draw
    long long* actions;                               // [B]
    float* log_prob;                                  // [B] log-probability of the action taken
};

struct AcnetReduceArgs {
    const float* slab;
    long long stride, total, off[ACNET_NPARAM + 1];   // parameter q covers [off[q], off[q + 1]) of a slab
    float* dst[ACNET_NPARAM];
    int S, np, B;
    const float* scal_slab;                           // null: no scalars
    int nsum;                                         // partial sums per slab: 5 (PPO) or 3 (A2C)
    float* scal_out;                                  // {loss, policy_loss, value_loss, entropy_loss} and for PPO {approx_kl, clip_fraction}
    float vf_coef, ent_coef;
};

int acnet_fwd_launch(const AcnetArgs& a, hipStream_t st);
int acnet_act_launch(const AcnetArgs& a, const AcnetActArgs& s, hipStream_t st);
int acnet_act_uniforms_launch(unsigned long long seed, unsigned long long row_offset, long long n, float* out, hipStream_t st);
int acnet_bwd_launch(const AcnetArgs& a, hipStream_t st);
int acnet_ppo_launch(const AcnetArgs& a, hipStream_t st);
int acnet_a2c_launch(const AcnetArgs& a, hipStream_t st);
int acnet_reduce_launch(const AcnetReduceArgs& r, hipStream_t st);
int acnet_adv_stats_launch(const float* adv, int B, float* stats, hipStream_t st);
int acnet_gae_launch(const float* rewards, const float* values, const float* starts, const float* last_values, const float* dones, float* adv, float* ret,
                     int T, int E, float gamma, float lam, hipStream_t st);
