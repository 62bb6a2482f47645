// Kernel arguments and launchers of DQN's fully parameterized quantile function (fqf.hip; C entry points in fqf_unit.cpp;
// include/ocrl_hip_fqf.h is the specification): the proposal of the fractions, the probability-weighted q and the fraction loss's
// gradient.  The collection step runs the implicit quantile head's own act kernel (iqn.hip, iqn_act_fqf_launch in iqn.h) with the two
// device functions below for the fractions and the fold, so that its q is ocrl_fqf_q's bit for bit.
#pragma once
#include "../../include/ocrl_hip_fqf.h"
#include "common.h"

#define FQF_MAX_FRACTIONS 32
#define FQF_MAX_FEATURES 256
#define FQF_MAX_ACTIONS 64
#define FQF_ROWS 8                 // rows of a group of the fraction loss's backward
#define FQF_MAX_SLABS 16
#define FQF_SLAB_HEAD 4            // floats at the head of a slab: the two fp64 sums of the reported scalars

// tau_hat_i of the interval [t0, t1]
__device__ __forceinline__ float fqf_tau_hat(float t0, float t1) { return __fmul_rn(0.5f, __fadd_rn(t0, t1)); }
// one term of the weighted q: acc + (t1 - t0) * theta, the difference rounded, the rest one fma
__device__ __forceinline__ float fqf_q_term(float acc, float t0, float t1, float theta) { return __fmaf_rn(__fsub_rn(t1, t0), theta, acc); }

struct FqfFracArgs {
    const float *x, *Wf, *bf;                         // [B, F], [N, F], [N]
    int B, F, N, L;                                   // L: lanes per row, the power of two >= N
    float *taus, *tau_hats, *eval_taus, *logp, *entropy;      // all but taus may be null
};

struct FqfBwdArgs {
    const float *x, *logp, *entropy, *quantiles;      // [B, F], [B, N], [B], [B, A, 2 N - 1]
    const long long* actions;
    const float* weights;                             // may be null
    float ent_coef;
    int B, F, A, N, S, ngroups, stride;               // S slabs of `stride` floats: the two fp64 sums, dWf [N * F], dbf [N]
    float *slab, *dWf, *dbf, *scalars;
};

static inline int fqf_slabs(int B) { const int g = cdiv(B, FQF_ROWS); return g < FQF_MAX_SLABS ? g : FQF_MAX_SLABS; }
static inline size_t fqf_stride(int F, int N) { return ((size_t)N * F + N + FQF_SLAB_HEAD + 63) & ~(size_t)63; }

int fqf_fractions_launch(const FqfFracArgs& a, hipStream_t st);
int fqf_q_launch(const float* quantiles, const float* taus, int B, int A, int N, float* q, hipStream_t st);
int fqf_bwd_launch(const FqfBwdArgs& a, hipStream_t st);
