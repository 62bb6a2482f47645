// The host side of the heads that run on the actor-critic head's tile code (acnet_tile.h): the actor-critic head itself (acnet_unit.cpp),
// the Q head (dqn_unit.cpp, replay_ext_unit.cpp, classifier_unit.cpp) and the categorical head (c51_unit.cpp).  Each rule below decides
// the size of a workspace or the order a sum runs in, so it is written here once and nowhere else: the per-layer limits, the parameter
// order and its slab offsets, the row tiles and slabs, the workspace's layout, the head as the tile code's arguments and the fold of the
// slabs' partial dw.  Host only.  What is particular to a head stays in its unit: its descriptor's mapping onto HeadSpec and the limits
// of its action and atom counts.
#pragma once
#include <stdio.h>

#include "../../include/ocrl_hip_dqn.h"
#include "acnet.h"
#include "unit_base.h"

// A head as the tile code sees it: trunks 0 = shared, 1 = policy, 2 = value (n[t] == 0: empty, dims / acts unread), the action Linear
// [na, latent of trunk 1] and the value Linear [nv, latent of trunk vt]; a Linear of 0 rows is absent.
struct HeadSpec {
    int B = 0, F = 0;
    int n[3] = {0, 0, 0};
    const int* dims[3] = {nullptr, nullptr, nullptr};
    const int* acts[3] = {nullptr, nullptr, nullptr};
    int na = 0, nv = 0;
    int vt = 2;                                       // 1: the value Linear reads the policy trunk's latent (C51's dueling stream)
    bool stats = false;                               // the workspace ends with the 8 floats of the advantages' statistics
};

// Parameter order (w, dw, the slabs): (weight, bias) per layer of trunk 0, 1, 2, then the action Linear's, then the value Linear's.
struct HeadLay {
    size_t saved[3][ACNET_MAX_LAYERS], slab, scal, stats, total;
    long long off[ACNET_NPARAM + 1];                  // parameter q covers [off[q], off[q + 1]) of a slab
    int np, S, ntiles;
};

inline int check_batch(int B, int F, const char* who) {
    OCRL_REQUIRE(B >= 1 && F >= 1, "%s: batch >= 1 and feature_dim >= 1 (got %d, %d)", who, B, F);
    return 0;
}

// The limits of the trunks' layers.  `trunks`: the messages name a layer by trunk and layer (the actor-critic head), else by its place
// in the one chain (trunk 1).  wmin: a floor of the widest row of a call (C51's logits tile).
inline int check_layers(const HeadSpec& s, bool trunks, long long wmin, const char* who) {
    struct Name {                                     // of layer l of trunk t; built only where a message needs it
        char text[40];
        Name(bool trunks, int t, int l) {
            if (trunks) snprintf(text, sizeof(text), "trunk %d layer %d", t, l);
            else snprintf(text, sizeof(text), "layer %d", l);
        }
    };
    long long wmax = s.F > wmin ? s.F : wmin;
    for (int t = 0; t < 3; ++t) {
        if (trunks)
            OCRL_REQUIRE(s.n[t] >= 0 && s.n[t] <= ACNET_MAX_LAYERS, "%s: at most %d layers per trunk (trunk %d has %d)", who, ACNET_MAX_LAYERS, t, s.n[t]);
        else
            OCRL_REQUIRE(s.n[t] >= 0 && s.n[t] <= ACNET_MAX_LAYERS, "%s: at most %d hidden layers (got %d)", who, ACNET_MAX_LAYERS, s.n[t]);
        for (int l = 0; l < s.n[t]; ++l) {
            const int w = s.dims[t][l], a = s.acts[t][l];
            OCRL_REQUIRE(w >= 4 && w <= ACNET_MAX_WIDTH && w % 4 == 0, "%s: layer widths are multiples of 4 up to %d (%s is %d)", who, ACNET_MAX_WIDTH,
                         Name(trunks, t, l).text, w);
            OCRL_REQUIRE(a >= 0 && a <= 2, "%s: activation 0 (none), 1 (relu) or 2 (tanh) (%s has %d)", who, Name(trunks, t, l).text, a);
            if (w > wmax) wmax = w;
        }
    }
    OCRL_REQUIRE((long long)s.B * wmax < (1LL << 31), "%s: batch %d times width %lld leaves the int32 range of one call", who, s.B, wmax);
    return 0;
}

inline HeadLay head_layout(const HeadSpec& s) {
    HeadLay y;
    WsTake take;
    const int Kh = s.n[0] ? s.dims[0][s.n[0] - 1] : s.F;
    auto latent = [&](int t) { return t && s.n[t] ? s.dims[t][s.n[t] - 1] : Kh; };
    long long off = 0;
    y.np = 0;
    auto param = [&](long long N, int K) {
        y.off[y.np++] = off; off += N * K;
        y.off[y.np++] = off; off += N;
    };
    for (int t = 0; t < 3; ++t)
        for (int l = 0; l < s.n[t]; ++l) {
            y.saved[t][l] = take((size_t)s.B * s.dims[t][l]);
            param(s.dims[t][l], l ? s.dims[t][l - 1] : (t ? Kh : s.F));
        }
    if (s.na) param(s.na, latent(1));
    if (s.nv) param(s.nv, latent(s.vt));
    y.off[y.np] = off;
    y.ntiles = (s.B + 15) / 16;
    y.S = y.ntiles < ACNET_MAX_SLABS ? y.ntiles : ACNET_MAX_SLABS;
    y.slab = take((size_t)y.S * (size_t)off);
    y.scal = take((size_t)y.S * 8);
    y.stats = s.stats ? take(8) : 0;
    y.total = take.end;
    return y;
}

template <class T>
int check_ptrs(T* const* w, int np, const char* who) {
    OCRL_REQUIRE(w, "%s: null argument", who);
    for (int q = 0; q < np; ++q) OCRL_REQUIRE(w[q], "%s: parameter pointer %d of %d is null", who, q, np);
    return 0;
}

// the part of the kernel arguments every entry point shares; AcnetArgs::A = the action Linear's rows
inline void head_args(AcnetArgs& a, const HeadSpec& s, const HeadLay& y, const float* x, const float* const* w, float* ws, bool saved) {
    a = AcnetArgs{};
    a.B = s.B; a.F = s.F; a.A = s.na;
    int q = 0;
    for (int t = 0; t < 3; ++t) {
        a.n[t] = s.n[t];
        for (int l = 0; l < s.n[t]; ++l) {
            a.dim[t][l] = s.dims[t][l]; a.act[t][l] = s.acts[t][l];
            a.off_w[t][l] = y.off[q]; a.w[t][l] = w[q++];
            a.off_b[t][l] = y.off[q]; a.b[t][l] = w[q++];
            a.saved[t][l] = saved ? ws + y.saved[t][l] : nullptr;
        }
    }
    if (s.na) {
        a.off_wa = y.off[q]; a.wa = w[q++];
        a.off_ba = y.off[q]; a.ba = w[q++];
    }
    if (s.nv) {
        a.off_wv = y.off[q]; a.wv = w[q++];
        a.off_bv = y.off[q]; a.bv = w[q++];
    }
    a.x = x;
    a.S = y.S; a.ntiles = y.ntiles;
    if (ws) {
        a.slab = ws + y.slab; a.scal_slab = ws + y.scal;
        if (s.stats) a.stats = ws + y.stats;
    }
    a.slab_stride = y.off[y.np];
}

// What a backward or a fused step runs after its own null check: the parameter pointers (dw null: none to check), the workspace against
// the layout and the arguments.
inline int head_begin(AcnetArgs& a, const HeadSpec& s, const HeadLay& y, const char* who, const float* x, const float* const* w, float* const* dw,
                      float* ws, size_t ws_floats, bool saved = true) {
    if (y.np) RC(check_ptrs(w, y.np, who));
    if (y.np && dw) RC(check_ptrs(dw, y.np, who));
    RC(ws_check(who, ws_floats, y.total));
    head_args(a, s, y, x, w, ws, saved);
    return 0;
}

// dw = the slabs' partial gradients in slab order; the caller may add the scalars' fields before acnet_reduce_launch
inline AcnetReduceArgs reduce_args(const AcnetArgs& a, const HeadLay& y, float* const* dw) {
    AcnetReduceArgs r{};
    r.slab = a.slab; r.stride = a.slab_stride; r.total = a.slab_stride; r.S = y.S; r.np = y.np; r.B = a.B;
    for (int q = 0; q <= y.np; ++q) r.off[q] = y.off[q];
    for (int q = 0; q < y.np; ++q) r.dst[q] = dw[q];
    return r;
}
inline int reduce_dw(const AcnetArgs& a, const HeadLay& y, float* const* dw, hipStream_t st) { return acnet_reduce_launch(reduce_args(a, y, dw), st); }

// ---- the Q head (ocrl_qnet_desc): the hidden layers are the policy trunk, the output Linear the action head, no value head.  Its
// entry points are those of ocrl_hip_dqn.h, ocrl_hip_replay.h and ocrl_hip_classifier.h.
static_assert(sizeof(ocrl_qnet_desc::dims) == ACNET_MAX_LAYERS * sizeof(int) && sizeof(ocrl_qnet_desc::acts) == ACNET_MAX_LAYERS * sizeof(int),
              "ocrl_qnet_desc holds the layers of one acnet trunk");
static_assert(sizeof(ocrl_qnet_desc) == (4 + 2 * ACNET_MAX_LAYERS) * sizeof(int), "ocrl_qnet_desc is 20 ints without padding");

inline HeadSpec qnet_spec(const ocrl_qnet_desc* d) {
    HeadSpec s;
    s.B = d->B; s.F = d->F; s.n[1] = d->n; s.dims[1] = d->dims; s.acts[1] = d->acts; s.na = d->A;
    return s;
}

inline int check_qnet(const ocrl_qnet_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    RC(check_batch(d->B, d->F, who));
    OCRL_REQUIRE(d->A >= 1 && d->A <= ACNET_MAX_ACTIONS, "%s: 1 <= n_actions <= %d (got %d)", who, ACNET_MAX_ACTIONS, d->A);
    return check_layers(qnet_spec(d), false, 0, who);
}
