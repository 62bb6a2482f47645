// C ABI of DQN's categorical head (include/ocrl_hip_c51.h: ocrl_c51_*).  Stateless: the caller owns parameters, gradients and the
// workspace.  Parameter order (w, dw): (weight, bias) per layer of the chain, then the advantage Linear's, then, with dueling, the value
// Linear's.  The workspace is the Q head's (dqn_unit.cpp) over this head's parameter list: the saved layer outputs, the slabs of partial
// gradients, the slabs' scalar sums.
#include <cmath>

#include "../../include/ocrl_hip_c51.h"
#include "c51.h"

namespace {
constexpr int C51_MAX_LAYERS = ACNET_MAX_LAYERS;
constexpr int C51_NPARAM = 2 * (C51_MAX_LAYERS + 2);
static_assert(sizeof(ocrl_c51_desc::dims) == C51_MAX_LAYERS * sizeof(int) && sizeof(ocrl_c51_desc::acts) == C51_MAX_LAYERS * sizeof(int),
              "ocrl_c51_desc holds the layers of one acnet trunk");
static_assert(sizeof(ocrl_c51_desc) == (6 + 2 * C51_MAX_LAYERS) * sizeof(int), "ocrl_c51_desc is 22 ints without padding");
static_assert(C51_NPARAM <= ACNET_NPARAM, "the fold of the slabs is acnet_reduce");

struct CLay {
    size_t saved[C51_MAX_LAYERS], slab, scal, total;
    long long off[C51_NPARAM + 1];
    int np, S, ntiles;
};

int check_c51(const ocrl_c51_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    OCRL_REQUIRE(d->B >= 1 && d->F >= 1, "%s: batch >= 1 and feature_dim >= 1 (got %d, %d)", who, d->B, d->F);
    OCRL_REQUIRE(d->A >= 1 && d->A <= ACNET_MAX_ACTIONS, "%s: 1 <= n_actions <= %d (got %d)", who, ACNET_MAX_ACTIONS, d->A);
    OCRL_REQUIRE(d->Z >= 2 && d->Z <= C51_MAX_ATOMS, "%s: 2 <= n_atoms <= %d (got %d)", who, C51_MAX_ATOMS, d->Z);
    OCRL_REQUIRE(d->A * d->Z <= C51_MAX_COLS, "%s: n_actions * n_atoms <= %d (got %d * %d)", who, C51_MAX_COLS, d->A, d->Z);
    OCRL_REQUIRE(d->n >= 0 && d->n <= C51_MAX_LAYERS, "%s: at most %d hidden layers (got %d)", who, C51_MAX_LAYERS, d->n);
    long long wmax = d->F > C51_MAX_COLS ? d->F : C51_MAX_COLS;
    for (int l = 0; l < d->n; ++l) {
        const int w = d->dims[l], a = d->acts[l];
        OCRL_REQUIRE(w >= 4 && w <= ACNET_MAX_WIDTH && w % 4 == 0, "%s: layer widths are multiples of 4 up to %d (layer %d is %d)", who, ACNET_MAX_WIDTH, l, w);
        OCRL_REQUIRE(a >= 0 && a <= 2, "%s: activation 0 (none), 1 (relu) or 2 (tanh) (layer %d has %d)", who, l, a);
    }
    OCRL_REQUIRE((long long)d->B * wmax < (1LL << 31), "%s: batch %d times width %lld leaves the int32 range of one call", who, d->B, wmax);
    return 0;
}

int check_support(float v_min, float v_max, const char* who) {
    OCRL_REQUIRE(std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max, "%s: v_min < v_max, both finite (got %g, %g)", who, (double)v_min,
                 (double)v_max);
    return 0;
}

CLay c_layout(const ocrl_c51_desc* d) {
    CLay y;
    WsTake take;
    long long off = 0;
    int K = d->F;
    y.np = 0;
    for (int l = 0; l < d->n; ++l) {
        const int N = d->dims[l];
        y.saved[l] = take((size_t)d->B * N);
        y.off[y.np++] = off; off += (long long)N * K;
        y.off[y.np++] = off; off += N;
        K = N;
    }
    const int NZ = d->A * d->Z;
    y.off[y.np++] = off; off += (long long)NZ * K;
    y.off[y.np++] = off; off += NZ;
    if (d->dueling) {
        y.off[y.np++] = off; off += (long long)d->Z * K;
        y.off[y.np++] = off; off += d->Z;
    }
    y.off[y.np] = off;
    y.ntiles = (d->B + 15) / 16;
    y.S = y.ntiles < ACNET_MAX_SLABS ? y.ntiles : ACNET_MAX_SLABS;
    y.slab = take((size_t)y.S * (size_t)off);
    y.scal = take((size_t)y.S * 8);
    y.total = take.end;
    return y;
}

// the head as the tile code's arguments: the chain is the policy trunk, the advantage Linear the action head, the value Linear wv / bv
void fill_args(AcnetArgs& a, C51Args& c, const ocrl_c51_desc* d, const CLay& y, const float* x, const float* const* w, float v_min, float v_max,
               float* ws, bool saved) {
    a = AcnetArgs{};
    a.B = d->B; a.F = d->F; a.A = d->A;
    a.n[1] = d->n;
    int q = 0;
    for (int l = 0; l < d->n; ++l) {
        a.dim[1][l] = d->dims[l]; a.act[1][l] = d->acts[l];
        a.off_w[1][l] = y.off[q]; a.w[1][l] = w[q++];
        a.off_b[1][l] = y.off[q]; a.b[1][l] = w[q++];
        a.saved[1][l] = saved ? ws + y.saved[l] : nullptr;
    }
    a.off_wa = y.off[q]; a.wa = w[q++];
    a.off_ba = y.off[q]; a.ba = w[q++];
    if (d->dueling) {
        a.off_wv = y.off[q]; a.wv = w[q++];
        a.off_bv = y.off[q]; a.bv = w[q++];
    }
    a.x = x;
    a.S = y.S; a.ntiles = y.ntiles;
    if (ws) { a.slab = ws + y.slab; a.scal_slab = ws + y.scal; }
    a.slab_stride = y.off[y.np];
    c = C51Args{};
    c.Z = d->Z; c.v_min = v_min; c.v_max = v_max; c.dz = (v_max - v_min) / (float)(d->Z - 1);
}

// dw = the slabs' partial gradients in slab order
int reduce_dw(const AcnetArgs& a, const CLay& y, float* const* dw, hipStream_t st) {
    AcnetReduceArgs r{};
    r.slab = a.slab; r.stride = a.slab_stride; r.total = a.slab_stride; r.S = y.S; r.np = y.np; r.B = a.B;
    for (int q = 0; q <= y.np; ++q) r.off[q] = y.off[q];
    for (int q = 0; q < y.np; ++q) r.dst[q] = dw[q];
    return acnet_reduce_launch(r, st);
}
}  // namespace

extern "C" {

size_t ocrl_c51_desc_size(void) { return sizeof(ocrl_c51_desc); }

size_t ocrl_c51_ws_floats(const ocrl_c51_desc* d) {
    if (check_c51(d, "ocrl_c51_ws_floats")) return 0;                  // the shapes the other entries reject get no workspace
    return c_layout(d).total;
}

int ocrl_c51_fwd(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max, float* logits, float* probs, float* q,
                 int save, float* ws, size_t ws_floats, void* stream) {
    RC(check_c51(d, "ocrl_c51_fwd"));
    RC(check_support(v_min, v_max, "ocrl_c51_fwd"));
    const CLay y = c_layout(d);
    OCRL_REQUIRE(features && w, "ocrl_c51_fwd: null argument");
    OCRL_REQUIRE(logits || probs || q, "ocrl_c51_fwd: logits, probs and q are all null: nothing to write");
    RC(qnet::check_ptrs((const void* const*)w, y.np, "ocrl_c51_fwd"));
    if (save) OCRL_REQUIRE(ws && ws_floats >= y.total, "ocrl_c51_fwd: workspace too small (%zu < %zu floats)", ws ? ws_floats : (size_t)0, y.total);
    AcnetArgs a;
    C51Args c;
    fill_args(a, c, d, y, features, w, v_min, v_max, save ? ws : nullptr, save != 0);
    c.logits = logits; c.probs = probs; c.q = q;
    return c51_fwd_launch(a, c, static_cast<hipStream_t>(stream));
}

int ocrl_c51_bwd(const ocrl_c51_desc* d, const float* features, const float* const* w, const float* dlogits, float* dfeatures, float* const* dw,
                 float* ws, size_t ws_floats, void* stream) {
    RC(check_c51(d, "ocrl_c51_bwd"));
    const CLay y = c_layout(d);
    OCRL_REQUIRE(features && w && dlogits && dw && ws, "ocrl_c51_bwd: null argument");
    RC(qnet::check_ptrs((const void* const*)w, y.np, "ocrl_c51_bwd"));
    RC(qnet::check_ptrs((const void* const*)dw, y.np, "ocrl_c51_bwd"));
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_c51_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    C51Args c;
    fill_args(a, c, d, y, features, w, 0.f, 1.f, ws, true);            // the support plays no part in the backward of the logits
    c.dlogits = dlogits; a.dx = dfeatures;
    RC(c51_bwd_launch(a, c, st));
    return reduce_dw(a, y, dw, st);
}

int ocrl_c51_act(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max, unsigned long long seed,
                 unsigned long long row_offset, float epsilon, const float* uniforms, long long* actions, float* q, void* stream) {
    RC(check_c51(d, "ocrl_c51_act"));
    RC(check_support(v_min, v_max, "ocrl_c51_act"));
    const CLay y = c_layout(d);
    OCRL_REQUIRE(features && w && actions, "ocrl_c51_act: null argument");
    RC(qnet::check_ptrs((const void* const*)w, y.np, "ocrl_c51_act"));
    AcnetArgs a;
    C51Args c;
    fill_args(a, c, d, y, features, w, v_min, v_max, nullptr, false);
    c.q = q;
    const DqnActArgs s{seed, row_offset, epsilon, uniforms, actions};
    return c51_act_launch(a, c, s, static_cast<hipStream_t>(stream));
}

int ocrl_c51_td_fwd_bwd(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max, const float* next_probs,
                        const float* next_q, const long long* actions, const float* rewards, const unsigned char* dones, const float* discounts,
                        const float* weights, float gamma, float* scalars, float* row_loss, float* dfeatures, float* const* dw, float* ws,
                        size_t ws_floats, void* stream) {
    RC(check_c51(d, "ocrl_c51_td_fwd_bwd"));
    RC(check_support(v_min, v_max, "ocrl_c51_td_fwd_bwd"));
    const CLay y = c_layout(d);
    OCRL_REQUIRE(features && w && next_probs && next_q && actions && rewards && dones && scalars && dw && ws, "ocrl_c51_td_fwd_bwd: null argument");
    RC(qnet::check_ptrs((const void* const*)w, y.np, "ocrl_c51_td_fwd_bwd"));
    RC(qnet::check_ptrs((const void* const*)dw, y.np, "ocrl_c51_td_fwd_bwd"));
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_c51_td_fwd_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    C51Args c;
    fill_args(a, c, d, y, features, w, v_min, v_max, ws, true);
    a.dx = dfeatures;
    const C51TdArgs s{next_probs, next_q, actions, rewards, dones, discounts, weights, gamma, row_loss};
    RC(c51_td_launch(a, c, s, st));
    RC(reduce_dw(a, y, dw, st));
    return dqn_scalars_launch(a.scal_slab, y.S, d->B, scalars, st);
}

}  // extern "C"
