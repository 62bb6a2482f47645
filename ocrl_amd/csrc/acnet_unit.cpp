// C ABI of the actor-critic head (include/ocrl_hip.h: ocrl_acnet_*, ocrl_gae): sb3s/custom_acnets.py:8-96 (CustomNetwork) with the
// action_net / value_net heads of its ActorCriticPolicy, the PPO minibatch loss (configs/sb3/ppo.yaml) and the A2C loss
// (configs/sb3/a2c.yaml).  Stateless: the caller owns
// parameters, gradients and the workspace.  Parameter order (w, dw): state_dict order of the trunks, shared_net, policy_net, value_net,
// (weight, bias) per layer, then with heads (A > 0) action_net.weight, action_net.bias, value_net.weight, value_net.bias.
#include "../../include/ocrl_hip.h"
#include "acnet.h"

namespace {
struct AcLay {
    size_t saved[3][ACNET_MAX_LAYERS], slab, scal, stats, total;
    long long off[ACNET_NPARAM + 1];
    int np, S, ntiles;
};

int check_acnet(const ocrl_acnet_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    OCRL_REQUIRE(d->B >= 1 && d->F >= 1, "%s: batch >= 1 and feature_dim >= 1 (got %d, %d)", who, d->B, d->F);
    OCRL_REQUIRE(d->A >= 0 && d->A <= ACNET_MAX_ACTIONS, "%s: 1 <= n_actions <= %d, or 0 for the trunks alone (got %d)", who, ACNET_MAX_ACTIONS, d->A);
    long long wmax = d->F;
    for (int t = 0; t < 3; ++t) {
        OCRL_REQUIRE(d->n[t] >= 0 && d->n[t] <= ACNET_MAX_LAYERS, "%s: at most %d layers per trunk (trunk %d has %d)", who, ACNET_MAX_LAYERS, t, d->n[t]);
        for (int l = 0; l < d->n[t]; ++l) {
            const int w = d->dims[t][l], a = d->acts[t][l];
            OCRL_REQUIRE(w >= 4 && w <= ACNET_MAX_WIDTH && w % 4 == 0, "%s: layer widths are multiples of 4 up to %d (trunk %d layer %d is %d)", who,
                         ACNET_MAX_WIDTH, t, l, w);
            OCRL_REQUIRE(a >= 0 && a <= 2, "%s: activation 0 (none), 1 (relu) or 2 (tanh) (trunk %d layer %d has %d)", who, t, l, a);
            if (w > wmax) wmax = w;
        }
    }
    OCRL_REQUIRE((long long)d->B * wmax < (1LL << 31), "%s: batch %d times width %lld leaves the int32 range of one call", who, d->B, wmax);
    return 0;
}

AcLay ac_layout(const ocrl_acnet_desc* d) {
    AcLay y;
    WsTake take;
    const int Kh = d->n[0] ? d->dims[0][d->n[0] - 1] : d->F;
    long long off = 0;
    y.np = 0;
    for (int t = 0; t < 3; ++t)
        for (int l = 0; l < d->n[t]; ++l) {
            const int K = l ? d->dims[t][l - 1] : (t ? Kh : d->F), N = d->dims[t][l];
            y.saved[t][l] = take((size_t)d->B * N);
            y.off[y.np++] = off; off += (long long)N * K;
            y.off[y.np++] = off; off += N;
        }
    if (d->A > 0) {
        const int Kp = d->n[1] ? d->dims[1][d->n[1] - 1] : Kh, Kv = d->n[2] ? d->dims[2][d->n[2] - 1] : Kh;
        y.off[y.np++] = off; off += (long long)d->A * Kp;
        y.off[y.np++] = off; off += d->A;
        y.off[y.np++] = off; off += Kv;
        y.off[y.np++] = off; off += 1;
    }
    y.off[y.np] = off;
    y.ntiles = (d->B + 15) / 16;
    y.S = y.ntiles < ACNET_MAX_SLABS ? y.ntiles : ACNET_MAX_SLABS;
    y.slab = take((size_t)y.S * (size_t)off);
    y.scal = take((size_t)y.S * 8);
    y.stats = take(8);
    y.total = take.end;
    return y;
}

// the part of the kernel arguments every entry point shares
void fill_args(AcnetArgs& a, const ocrl_acnet_desc* d, const AcLay& y, const float* x, const float* const* w, float* ws, bool saved) {
    a = AcnetArgs{};
    a.B = d->B; a.F = d->F; a.A = d->A;
    int q = 0;
    for (int t = 0; t < 3; ++t) {
        a.n[t] = d->n[t];
        for (int l = 0; l < d->n[t]; ++l) {
            a.dim[t][l] = d->dims[t][l]; a.act[t][l] = d->acts[t][l];
            a.off_w[t][l] = y.off[q]; a.w[t][l] = w[q++];
            a.off_b[t][l] = y.off[q]; a.b[t][l] = w[q++];
            a.saved[t][l] = saved ? ws + y.saved[t][l] : nullptr;
        }
    }
    if (d->A > 0) {
        a.off_wa = y.off[q]; a.wa = w[q++];
        a.off_ba = y.off[q]; a.ba = w[q++];
        a.off_wv = y.off[q]; a.wv = w[q++];
        a.off_bv = y.off[q]; a.bv = w[q++];
    }
    a.x = x;
    a.S = y.S; a.ntiles = y.ntiles;
    if (ws) { a.slab = ws + y.slab; a.scal_slab = ws + y.scal; a.stats = ws + y.stats; }
    a.slab_stride = y.off[y.np];
}

int check_ptrs(const float* const* w, int np, const char* who) {
    OCRL_REQUIRE(w, "%s: null argument", who);
    for (int q = 0; q < np; ++q) OCRL_REQUIRE(w[q], "%s: parameter pointer %d of %d is null", who, q, np);
    return 0;
}

void fill_reduce(AcnetReduceArgs& r, const AcnetArgs& a, const AcLay& y, float* const* dw) {
    r = AcnetReduceArgs{};
    r.slab = a.slab; r.stride = a.slab_stride; r.total = a.slab_stride; r.S = y.S; r.np = y.np; r.B = a.B;
    for (int q = 0; q <= y.np; ++q) r.off[q] = y.off[q];
    for (int q = 0; q < y.np; ++q) r.dst[q] = dw[q];
}
}  // namespace

extern "C" {

size_t ocrl_acnet_desc_size(void) { return sizeof(ocrl_acnet_desc); }

size_t ocrl_acnet_ws_floats(const ocrl_acnet_desc* d) {
    if (check_acnet(d, "ocrl_acnet_ws_floats")) return 0;              // the shapes fwd / bwd reject get no workspace
    return ac_layout(d).total;
}

int ocrl_acnet_fwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, float* latent_pi, float* latent_vf, float* logits,
                   float* values, int save, float* ws, size_t ws_floats, void* stream) {
    RC(check_acnet(d, "ocrl_acnet_fwd"));
    const AcLay y = ac_layout(d);
    OCRL_REQUIRE(features && (y.np == 0 || w), "ocrl_acnet_fwd: null argument");
    if (y.np) RC(check_ptrs(w, y.np, "ocrl_acnet_fwd"));
    if (save) OCRL_REQUIRE(ws && ws_floats >= y.total, "ocrl_acnet_fwd: workspace too small (%zu < %zu floats)", ws ? ws_floats : (size_t)0, y.total);
    AcnetArgs a;
    fill_args(a, d, y, features, w, save ? ws : nullptr, save != 0);
    a.lat_pi = latent_pi; a.lat_vf = latent_vf; a.logits = logits; a.values = values;
    return acnet_fwd_launch(a, static_cast<hipStream_t>(stream));
}

int ocrl_acnet_act(const ocrl_acnet_desc* d, const float* features, const float* const* w, unsigned long long seed, unsigned long long row_offset,
                   const float* uniforms, int deterministic, long long* actions, float* values, float* log_prob, float* logits, void* stream) {
    RC(check_acnet(d, "ocrl_acnet_act"));
    OCRL_REQUIRE(d->A >= 1, "ocrl_acnet_act: acting needs the heads (1 <= n_actions <= %d, got 0)", ACNET_MAX_ACTIONS);
    const AcLay y = ac_layout(d);
    OCRL_REQUIRE(features && w && actions && values && log_prob, "ocrl_acnet_act: null argument");
    RC(check_ptrs(w, y.np, "ocrl_acnet_act"));
    AcnetArgs a;
    fill_args(a, d, y, features, w, nullptr, false);
    a.logits = logits; a.values = values;
    AcnetActArgs s{seed, row_offset, uniforms, deterministic ? 1 : 0, actions, log_prob};
    return acnet_act_launch(a, s, static_cast<hipStream_t>(stream));
}

int ocrl_acnet_act_uniforms(unsigned long long seed, unsigned long long row_offset, long long n, float* out, void* stream) {
    OCRL_REQUIRE(out && n >= 1, "ocrl_acnet_act_uniforms: null output or n < 1 (got %lld)", n);
    return acnet_act_uniforms_launch(seed, row_offset, n, out, static_cast<hipStream_t>(stream));
}

int ocrl_acnet_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const float* dlatent_pi, const float* dlatent_vf,
                   const float* dlogits, const float* dvalues, float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    RC(check_acnet(d, "ocrl_acnet_bwd"));
    const AcLay y = ac_layout(d);
    OCRL_REQUIRE(features && ws && (y.np == 0 || (w && dw)), "ocrl_acnet_bwd: null argument");
    if (y.np) {
        RC(check_ptrs(w, y.np, "ocrl_acnet_bwd"));
        RC(check_ptrs(dw, y.np, "ocrl_acnet_bwd"));
    }
    OCRL_REQUIRE(d->A > 0 || (!dlogits && !dvalues), "ocrl_acnet_bwd: dlogits / dvalues given for a network without heads (n_actions = 0)");
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_acnet_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    fill_args(a, d, y, features, w, ws, true);
    a.dlat_pi = dlatent_pi; a.dlat_vf = dlatent_vf; a.dlogits = dlogits; a.dvalues = dvalues; a.dx = dfeatures;
    RC(acnet_bwd_launch(a, st));
    if (y.np == 0) return 0;
    AcnetReduceArgs r;
    fill_reduce(r, a, y, dw);
    return acnet_reduce_launch(r, st);
}

int ocrl_acnet_ppo_fwd_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const long long* actions, const float* old_log_prob,
                           const float* advantages, const float* returns, float clip_range, float vf_coef, float ent_coef, int normalize_advantage,
                           float* scalars, float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    RC(check_acnet(d, "ocrl_acnet_ppo_fwd_bwd"));
    OCRL_REQUIRE(d->A >= 1, "ocrl_acnet_ppo_fwd_bwd: the loss needs the heads (1 <= n_actions <= %d, got 0)", ACNET_MAX_ACTIONS);
    OCRL_REQUIRE(!(normalize_advantage && d->B < 2), "ocrl_acnet_ppo_fwd_bwd: normalize_advantage needs batch >= 2 (the std of one advantage is undefined)");
    const AcLay y = ac_layout(d);
    OCRL_REQUIRE(features && w && actions && old_log_prob && advantages && returns && scalars && dw && ws, "ocrl_acnet_ppo_fwd_bwd: null argument");
    RC(check_ptrs(w, y.np, "ocrl_acnet_ppo_fwd_bwd"));
    RC(check_ptrs(dw, y.np, "ocrl_acnet_ppo_fwd_bwd"));
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_acnet_ppo_fwd_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    fill_args(a, d, y, features, w, ws, true);
    a.actions = actions; a.old_logp = old_log_prob; a.adv = advantages; a.ret = returns;
    a.clip = clip_range; a.vf_coef = vf_coef; a.ent_coef = ent_coef; a.norm = normalize_advantage ? 1 : 0;
    a.dx = dfeatures;
    if (a.norm) RC(acnet_adv_stats_launch(advantages, d->B, ws + y.stats, st));
    RC(acnet_ppo_launch(a, st));
    AcnetReduceArgs r;
    fill_reduce(r, a, y, dw);
    r.scal_slab = a.scal_slab; r.nsum = 5; r.scal_out = scalars; r.vf_coef = vf_coef; r.ent_coef = ent_coef;
    return acnet_reduce_launch(r, st);
}

int ocrl_acnet_a2c_fwd_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const long long* actions, const float* advantages,
                           const float* returns, float vf_coef, float ent_coef, int normalize_advantage, float* scalars, float* dfeatures,
                           float* const* dw, float* ws, size_t ws_floats, void* stream) {
    RC(check_acnet(d, "ocrl_acnet_a2c_fwd_bwd"));
    OCRL_REQUIRE(d->A >= 1, "ocrl_acnet_a2c_fwd_bwd: the loss needs the heads (1 <= n_actions <= %d, got 0)", ACNET_MAX_ACTIONS);
    OCRL_REQUIRE(!(normalize_advantage && d->B < 2), "ocrl_acnet_a2c_fwd_bwd: normalize_advantage needs batch >= 2 (the std of one advantage is undefined)");
    const AcLay y = ac_layout(d);
    OCRL_REQUIRE(features && w && actions && advantages && returns && scalars && dw && ws, "ocrl_acnet_a2c_fwd_bwd: null argument");
    RC(check_ptrs(w, y.np, "ocrl_acnet_a2c_fwd_bwd"));
    RC(check_ptrs(dw, y.np, "ocrl_acnet_a2c_fwd_bwd"));
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_acnet_a2c_fwd_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    fill_args(a, d, y, features, w, ws, true);
    a.actions = actions; a.adv = advantages; a.ret = returns;
    a.vf_coef = vf_coef; a.ent_coef = ent_coef; a.norm = normalize_advantage ? 1 : 0;
    a.dx = dfeatures;
    if (a.norm) RC(acnet_adv_stats_launch(advantages, d->B, ws + y.stats, st));
    RC(acnet_a2c_launch(a, st));
    AcnetReduceArgs r;
    fill_reduce(r, a, y, dw);
    r.scal_slab = a.scal_slab; r.nsum = 3; r.scal_out = scalars; r.vf_coef = vf_coef; r.ent_coef = ent_coef;
    return acnet_reduce_launch(r, st);
}

int ocrl_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values, const float* dones, float* advantages,
             float* returns, int T, int E, float gamma, float gae_lambda, void* stream) {
    OCRL_REQUIRE(rewards && values && episode_starts && last_values && dones && advantages && returns, "ocrl_gae: null argument");
    OCRL_REQUIRE(T >= 1 && E >= 1 && (long long)T * E < (1LL << 31), "ocrl_gae: steps >= 1, envs >= 1 and steps * envs < 2^31 (got %d, %d)", T, E);
    return acnet_gae_launch(rewards, values, episode_starts, last_values, dones, advantages, returns, T, E, gamma, gae_lambda, static_cast<hipStream_t>(stream));
}

}  // extern "C"
