// C ABI of the DQN pieces (include/ocrl_hip_dqn.h: ocrl_qnet_*, ocrl_dqn_*, ocrl_replay_*).  Stateless: the caller owns parameters,
// gradients, the ring and the workspace.  Parameter order (w, dw): (weight, bias) per hidden layer, then the output Linear's.
#include "../../include/ocrl_hip_dqn.h"
#include "dqn.h"

namespace {
constexpr int QNET_MAX_LAYERS = ACNET_MAX_LAYERS;
static_assert(sizeof(ocrl_qnet_desc::dims) == QNET_MAX_LAYERS * sizeof(int) && sizeof(ocrl_qnet_desc::acts) == QNET_MAX_LAYERS * sizeof(int),
              "ocrl_qnet_desc holds the layers of one acnet trunk");
static_assert(sizeof(ocrl_qnet_desc) == (4 + 2 * QNET_MAX_LAYERS) * sizeof(int), "ocrl_qnet_desc is 20 ints without padding");
}  // namespace

// the Q head's host side, shared with replay_ext_unit.cpp (declared in dqn.h)
namespace qnet {

int check_qnet(const ocrl_qnet_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    OCRL_REQUIRE(d->B >= 1 && d->F >= 1, "%s: batch >= 1 and feature_dim >= 1 (got %d, %d)", who, d->B, d->F);
    OCRL_REQUIRE(d->A >= 1 && d->A <= ACNET_MAX_ACTIONS, "%s: 1 <= n_actions <= %d (got %d)", who, ACNET_MAX_ACTIONS, d->A);
    OCRL_REQUIRE(d->n >= 0 && d->n <= QNET_MAX_LAYERS, "%s: at most %d hidden layers (got %d)", who, QNET_MAX_LAYERS, d->n);
    long long wmax = d->F;
    for (int l = 0; l < d->n; ++l) {
        const int w = d->dims[l], a = d->acts[l];
        OCRL_REQUIRE(w >= 4 && w <= ACNET_MAX_WIDTH && w % 4 == 0, "%s: layer widths are multiples of 4 up to %d (layer %d is %d)", who, ACNET_MAX_WIDTH, l, w);
        OCRL_REQUIRE(a >= 0 && a <= 2, "%s: activation 0 (none), 1 (relu) or 2 (tanh) (layer %d has %d)", who, l, a);
        if (w > wmax) wmax = w;
    }
    OCRL_REQUIRE((long long)d->B * wmax < (1LL << 31), "%s: batch %d times width %lld leaves the int32 range of one call", who, d->B, wmax);
    return 0;
}

QLay q_layout(const ocrl_qnet_desc* d) {
    QLay y;
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
    y.off[y.np++] = off; off += (long long)d->A * K;
    y.off[y.np++] = off; off += d->A;
    y.off[y.np] = off;
    y.ntiles = (d->B + 15) / 16;
    y.S = y.ntiles < ACNET_MAX_SLABS ? y.ntiles : ACNET_MAX_SLABS;
    y.slab = take((size_t)y.S * (size_t)off);
    y.scal = take((size_t)y.S * 8);
    y.total = take.end;
    return y;
}

// the Q head as the tile code's arguments: the hidden layers are the policy trunk, the output Linear the action head
void fill_args(AcnetArgs& a, const ocrl_qnet_desc* d, const QLay& y, const float* x, const float* const* w, float* ws, bool saved) {
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
    a.x = x;
    a.S = y.S; a.ntiles = y.ntiles;
    if (ws) { a.slab = ws + y.slab; a.scal_slab = ws + y.scal; }
    a.slab_stride = y.off[y.np];
}

int check_ptrs(const void* const* w, int np, const char* who) {
    OCRL_REQUIRE(w, "%s: null argument", who);
    for (int q = 0; q < np; ++q) OCRL_REQUIRE(w[q], "%s: parameter pointer %d of %d is null", who, q, np);
    return 0;
}

// dw = the slabs' partial gradients in slab order
int reduce_dw(const AcnetArgs& a, const QLay& y, float* const* dw, hipStream_t st) {
    AcnetReduceArgs r{};
    r.slab = a.slab; r.stride = a.slab_stride; r.total = a.slab_stride; r.S = y.S; r.np = y.np; r.B = a.B;
    for (int q = 0; q <= y.np; ++q) r.off[q] = y.off[q];
    for (int q = 0; q < y.np; ++q) r.dst[q] = dw[q];
    return acnet_reduce_launch(r, st);
}
}  // namespace qnet
using namespace qnet;

extern "C" {

size_t ocrl_qnet_desc_size(void) { return sizeof(ocrl_qnet_desc); }

size_t ocrl_qnet_ws_floats(const ocrl_qnet_desc* d) {
    if (check_qnet(d, "ocrl_qnet_ws_floats")) return 0;                // the shapes the other entries reject get no workspace
    return q_layout(d).total;
}

int ocrl_qnet_fwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, float* q, int save, float* ws, size_t ws_floats,
                  void* stream) {
    RC(check_qnet(d, "ocrl_qnet_fwd"));
    const QLay y = q_layout(d);
    OCRL_REQUIRE(features && w && q, "ocrl_qnet_fwd: null argument");
    RC(check_ptrs((const void* const*)w, y.np, "ocrl_qnet_fwd"));
    if (save) OCRL_REQUIRE(ws && ws_floats >= y.total, "ocrl_qnet_fwd: workspace too small (%zu < %zu floats)", ws ? ws_floats : (size_t)0, y.total);
    AcnetArgs a;
    fill_args(a, d, y, features, w, save ? ws : nullptr, save != 0);
    a.logits = q;
    return acnet_fwd_launch(a, static_cast<hipStream_t>(stream));
}

int ocrl_qnet_bwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, const float* dq, float* dfeatures, float* const* dw, float* ws,
                  size_t ws_floats, void* stream) {
    RC(check_qnet(d, "ocrl_qnet_bwd"));
    const QLay y = q_layout(d);
    OCRL_REQUIRE(features && w && dq && dw && ws, "ocrl_qnet_bwd: null argument");
    RC(check_ptrs((const void* const*)w, y.np, "ocrl_qnet_bwd"));
    RC(check_ptrs((const void* const*)dw, y.np, "ocrl_qnet_bwd"));
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_qnet_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    fill_args(a, d, y, features, w, ws, true);
    a.dlogits = dq; a.dx = dfeatures;
    RC(acnet_bwd_launch(a, st));
    return reduce_dw(a, y, dw, st);
}

int ocrl_dqn_act(const ocrl_qnet_desc* d, const float* features, const float* const* w, unsigned long long seed, unsigned long long row_offset,
                 float epsilon, const float* uniforms, long long* actions, float* q, void* stream) {
    RC(check_qnet(d, "ocrl_dqn_act"));
    const QLay y = q_layout(d);
    OCRL_REQUIRE(features && w && actions, "ocrl_dqn_act: null argument");
    RC(check_ptrs((const void* const*)w, y.np, "ocrl_dqn_act"));
    AcnetArgs a;
    fill_args(a, d, y, features, w, nullptr, false);
    a.logits = q;
    const DqnActArgs s{seed, row_offset, epsilon, uniforms, actions};
    return dqn_act_launch(a, s, static_cast<hipStream_t>(stream));
}

int ocrl_dqn_act_uniforms(unsigned long long seed, unsigned long long row_offset, long long n, float* out, void* stream) {
    OCRL_REQUIRE(out && n >= 1, "ocrl_dqn_act_uniforms: null output or n < 1 (got %lld)", n);
    return dqn_act_uniforms_launch(seed, row_offset, n, out, static_cast<hipStream_t>(stream));
}

int ocrl_dqn_td_fwd_bwd(const ocrl_qnet_desc* d, const float* features, const float* const* w, const float* next_q, const long long* actions,
                        const float* rewards, const unsigned char* dones, float gamma, float* scalars, float* dfeatures, float* const* dw, float* ws,
                        size_t ws_floats, void* stream) {
    RC(check_qnet(d, "ocrl_dqn_td_fwd_bwd"));
    const QLay y = q_layout(d);
    OCRL_REQUIRE(features && w && next_q && actions && rewards && dones && scalars && dw && ws, "ocrl_dqn_td_fwd_bwd: null argument");
    RC(check_ptrs((const void* const*)w, y.np, "ocrl_dqn_td_fwd_bwd"));
    RC(check_ptrs((const void* const*)dw, y.np, "ocrl_dqn_td_fwd_bwd"));
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_dqn_td_fwd_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    fill_args(a, d, y, features, w, ws, true);
    a.dx = dfeatures;
    const DqnTdArgs s{next_q, actions, rewards, dones, gamma};
    RC(dqn_td_launch(a, s, st));
    RC(reduce_dw(a, y, dw, st));
    return dqn_scalars_launch(a.scal_slab, y.S, d->B, scalars, st);
}

int ocrl_replay_gather(const void* obs, const long long* actions, const float* rewards, const unsigned char* dones, int N, int E, long long S,
                       const long long* idx, int B, void* obs_out, void* next_obs_out, long long* actions_out, float* rewards_out,
                       unsigned char* dones_out, void* stream) {
    OCRL_REQUIRE(obs && actions && rewards && dones && idx && obs_out && next_obs_out && actions_out && rewards_out && dones_out,
                 "ocrl_replay_gather: null argument");
    OCRL_REQUIRE(N >= 2 && E >= 1 && B >= 1 && (long long)N * E < (1LL << 31), "ocrl_replay_gather: slots >= 2, envs >= 1, batch >= 1 and slots * envs < 2^31 (got %d, %d, %d)",
                 N, E, B);
    OCRL_REQUIRE(S >= 4 && S % 4 == 0, "ocrl_replay_gather: the byte size of an observation is a positive multiple of 4 (got %lld)", S);
    const uintptr_t al = (uintptr_t)obs | (uintptr_t)obs_out | (uintptr_t)next_obs_out;
    OCRL_REQUIRE((al & (S % 16 == 0 ? 15 : 3)) == 0, "ocrl_replay_gather: observation pointers must be %d-byte aligned for observations of %lld bytes",
                 S % 16 == 0 ? 16 : 4, S);
    const ReplayGatherArgs g{static_cast<const unsigned char*>(obs), actions, rewards, dones, N, E, B, S, idx, static_cast<unsigned char*>(obs_out),
                             static_cast<unsigned char*>(next_obs_out), actions_out, rewards_out, dones_out};
    return replay_gather_launch(g, static_cast<hipStream_t>(stream));
}

int ocrl_replay_sample(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, long long* idx, void* stream) {
    OCRL_REQUIRE(idx, "ocrl_replay_sample: null argument");
    OCRL_REQUIRE(N >= 2 && E >= 1 && B >= 1 && (long long)N * E < (1LL << 31), "ocrl_replay_sample: slots >= 2, envs >= 1, batch >= 1 and slots * envs < 2^31 (got %d, %d, %d)",
                 N, E, B);
    OCRL_REQUIRE(pos >= 0 && pos < N && (full || pos >= 1), "ocrl_replay_sample: 0 <= pos < slots, and pos >= 1 while the ring is not full (got pos %d of %d, full %d)",
                 pos, N, full);
    return replay_sample_launch(seed, update, B, N, E, pos, full, idx, static_cast<hipStream_t>(stream));
}

}  // extern "C"
