// Kernel arguments and launchers of DQN's noisy linear layers (noisy.hip; C entry points in noisy_unit.cpp; include/ocrl_hip_noisy.h is
// the specification).  One launch covers every layer of a descriptor: the layers travel as a table in the kernel's arguments, and a
// workgroup finds its tensor by a bounded scan of the table's block counts.
#pragma once
#include "../../include/ocrl_hip_noisy.h"
#include "common.h"

#define SITE_NOISY 440u            // rng site of the noise factors (dqn.h has 410 and 420, replay_ext.h 430)
#define NOISY_MAX_LAYERS 10
#define NOISY_MAX_WIDTH 65536

// `factors`: per layer f_in at fin[l], f_out at fout[l], each block rounded up to a multiple of 4 floats; total = the whole buffer
struct NoisyFactorLayout {
    int fin[NOISY_MAX_LAYERS], fout[NOISY_MAX_LAYERS];
    int total;
};

// one tensor pair of a layer: a weight [out, in] and a bias [out].  a: mu (perturb) or dw_eff (grad); s: sigma (perturb only); dst: w_eff
// or dsigma
struct NoisyLayer {
    const float *a_w, *s_w, *a_b, *s_b;
    float *dst_w, *dst_b;
    int in, out, fin, fout;
};
struct NoisyArgs {
    NoisyLayer lay[NOISY_MAX_LAYERS];
    long long first[2 * NOISY_MAX_LAYERS + 1];        // first[2 l] / first[2 l + 1]: the first workgroup of layer l's weight / bias
    const float* factors;
    int n_layers;
};

struct NoisyFactorArgs {
    NoisyFactorLayout lay;
    int in[NOISY_MAX_LAYERS], out[NOISY_MAX_LAYERS];
    int n_layers;
    unsigned long long seed, draw;
    const float* eps;
    float* factors;
};

NoisyFactorLayout noisy_factor_layout(const ocrl_noisy_desc* d);
int noisy_factors_launch(const NoisyFactorArgs& a, hipStream_t st);
int noisy_apply_launch(NoisyArgs& a, bool grad, hipStream_t st);      // fills a.first
