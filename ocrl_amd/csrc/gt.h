// Kernel arguments and launchers of the ground-truth-state encoder's per-object MLP (gt.hip; C entry points in gt_unit.cpp).
#pragma once
#include "../../include/ocrl_hip.h"
#include "common.h"

#define GT_TM 16                    // rows of a tile: one workgroup's share of the M object rows
#define GT_MAX_SLABS 64             // weight-gradient partials of the backward (as conv_slab caps them)

// the backward's split of the tiles into slabs: one workgroup walks a slab's tiles in order, so the partial of a slab, and with the
// slab-order sum of gt_mlp_reduce the whole gradient, depends on M alone
struct GtSlab { int tiles, per_slab, slabs; };
inline GtSlab gt_slab(int M) {
    GtSlab s;
    s.tiles = cdiv(M, GT_TM);
    s.per_slab = cdiv(s.tiles, GT_MAX_SLABS);
    s.slabs = cdiv(s.tiles, s.per_slab);
    return s;
}

struct GtFwdArgs {
    const float* x;                                 // [M, D]
    const float* w[OCRL_GT_MLP_MAX_LAYERS];         // [dims[l], dims[l - 1]] (torch layout)
    const float* b[OCRL_GT_MLP_MAX_LAYERS];
    float* h[OCRL_GT_MLP_MAX_LAYERS];               // every layer's post-activation output [M, dims[l]], saved for the backward; may be null
    float* out;                                     // [M, dims[nl - 1]]
    int M, D, nl;
    int dims[OCRL_GT_MLP_MAX_LAYERS], relu[OCRL_GT_MLP_MAX_LAYERS];
};

struct GtBwdArgs {
    const float *x, *dout;
    const float* w[OCRL_GT_MLP_MAX_LAYERS];
    const float* h[OCRL_GT_MLP_MAX_LAYERS];
    float* dx;                                      // [M, D] or null
    float* dw[OCRL_GT_MLP_MAX_LAYERS];              // slab 0's weight gradient: the caller's tensor (one slab) or the partial buffer
    float* db[OCRL_GT_MLP_MAX_LAYERS];
    long long slab_stride;                          // floats between the partials of two slabs
    int M, D, nl, per_slab;
    int dims[OCRL_GT_MLP_MAX_LAYERS], relu[OCRL_GT_MLP_MAX_LAYERS];
};

struct GtReduceArgs {
    const float* part;                              // [slabs, P]: per slab W0, b0, W1, b1, ..
    float* dst[2 * OCRL_GT_MLP_MAX_LAYERS];         // dw0, db0, dw1, ..
    int end[2 * OCRL_GT_MLP_MAX_LAYERS];            // one past the last float of each within a slab
    int n, P, slabs;
};

int gt_mlp_fwd_launch(const GtFwdArgs& a, hipStream_t st);
int gt_mlp_bwd_launch(const GtBwdArgs& a, int slabs, hipStream_t st);
int gt_mlp_reduce_launch(const GtReduceArgs& a, hipStream_t st);
