// C ABI of the actor-critic head (include/ocrl_hip.h: ocrl_acnet_*, ocrl_gae): sb3s/custom_acnets.py:8-96 (CustomNetwork) with the
// action_net / value_net heads of its ActorCriticPolicy, the PPO minibatch loss (configs/sb3/ppo.yaml) and the A2C loss
// (configs/sb3/a2c.yaml).  Stateless: the caller owns
// parameters, gradients and the workspace.  Parameter order (w, dw): state_dict order of the trunks, shared_net, policy_net, value_net,
// (weight, bias) per layer, then with heads (A > 0) action_net.weight, action_net.bias, value_net.weight, value_net.bias.
#include "../../include/ocrl_hip.h"
#include "acnet_host.h"

namespace {
HeadSpec ac_spec(const ocrl_acnet_desc* d) {
    HeadSpec s;
    s.B = d->B; s.F = d->F; s.na = d->A; s.nv = d->A > 0 ? 1 : 0; s.stats = true;
    for (int t = 0; t < 3; ++t) { s.n[t] = d->n[t]; s.dims[t] = d->dims[t]; s.acts[t] = d->acts[t]; }
    return s;
}

int check_acnet(const ocrl_acnet_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    RC(check_batch(d->B, d->F, who));
    OCRL_REQUIRE(d->A >= 0 && d->A <= ACNET_MAX_ACTIONS, "%s: 1 <= n_actions <= %d, or 0 for the trunks alone (got %d)", who, ACNET_MAX_ACTIONS, d->A);
    return check_layers(ac_spec(d), true, 0, who);
}

// what the two losses ask before anything else
int check_loss(const ocrl_acnet_desc* d, int normalize_advantage, const char* who) {
    RC(check_acnet(d, who));
    OCRL_REQUIRE(d->A >= 1, "%s: the loss needs the heads (1 <= n_actions <= %d, got 0)", who, ACNET_MAX_ACTIONS);
    OCRL_REQUIRE(!(normalize_advantage && d->B < 2), "%s: normalize_advantage needs batch >= 2 (the std of one advantage is undefined)", who);
    return 0;
}

// the fold of the slabs with the loss's scalars from their nsum partial sums
int reduce_loss(const AcnetArgs& a, const HeadLay& y, float* const* dw, int nsum, float* scalars, hipStream_t st) {
    AcnetReduceArgs r = reduce_args(a, y, dw);
    r.scal_slab = a.scal_slab; r.nsum = nsum; r.scal_out = scalars; r.vf_coef = a.vf_coef; r.ent_coef = a.ent_coef;
    return acnet_reduce_launch(r, st);
}
}  // namespace

extern "C" {

size_t ocrl_acnet_desc_size(void) { return sizeof(ocrl_acnet_desc); }

size_t ocrl_acnet_ws_floats(const ocrl_acnet_desc* d) {
    if (check_acnet(d, "ocrl_acnet_ws_floats")) return 0;              // the shapes fwd / bwd reject get no workspace
    return head_layout(ac_spec(d)).total;
}

int ocrl_acnet_fwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, float* latent_pi, float* latent_vf, float* logits,
                   float* values, int save, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_acnet_fwd";
    RC(check_acnet(d, who));
    const HeadSpec s = ac_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && (y.np == 0 || w), "%s: null argument", who);
    if (y.np) RC(check_ptrs(w, y.np, who));
    if (save) RC(ws_check(who, ws ? ws_floats : (size_t)0, y.total));
    AcnetArgs a;
    head_args(a, s, y, features, w, save ? ws : nullptr, save != 0);
    a.lat_pi = latent_pi; a.lat_vf = latent_vf; a.logits = logits; a.values = values;
    return acnet_fwd_launch(a, static_cast<hipStream_t>(stream));
}

int ocrl_acnet_act(const ocrl_acnet_desc* d, const float* features, const float* const* w, unsigned long long seed, unsigned long long row_offset,
                   const float* uniforms, int deterministic, long long* actions, float* values, float* log_prob, float* logits, void* stream) {
    const char* who = "ocrl_acnet_act";
    RC(check_acnet(d, who));
    OCRL_REQUIRE(d->A >= 1, "%s: acting needs the heads (1 <= n_actions <= %d, got 0)", who, ACNET_MAX_ACTIONS);
    const HeadSpec s = ac_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && actions && values && log_prob, "%s: null argument", who);
    RC(check_ptrs(w, y.np, who));
    AcnetArgs a;
    head_args(a, s, y, features, w, nullptr, false);
    a.logits = logits; a.values = values;
    AcnetActArgs t{seed, row_offset, uniforms, deterministic ? 1 : 0, actions, log_prob};
    return acnet_act_launch(a, t, static_cast<hipStream_t>(stream));
}

int ocrl_acnet_act_uniforms(unsigned long long seed, unsigned long long row_offset, long long n, float* out, void* stream) {
    OCRL_REQUIRE(out && n >= 1, "ocrl_acnet_act_uniforms: null output or n < 1 (got %lld)", n);
    return acnet_act_uniforms_launch(seed, row_offset, n, out, static_cast<hipStream_t>(stream));
}

int ocrl_acnet_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const float* dlatent_pi, const float* dlatent_vf,
                   const float* dlogits, const float* dvalues, float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_acnet_bwd";
    RC(check_acnet(d, who));
    const HeadSpec s = ac_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && ws && (y.np == 0 || (w && dw)), "%s: null argument", who);
    OCRL_REQUIRE(d->A > 0 || (!dlogits && !dvalues), "%s: dlogits / dvalues given for a network without heads (n_actions = 0)", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    a.dlat_pi = dlatent_pi; a.dlat_vf = dlatent_vf; a.dlogits = dlogits; a.dvalues = dvalues; a.dx = dfeatures;
    RC(acnet_bwd_launch(a, st));
    return y.np ? reduce_dw(a, y, dw, st) : 0;
}

int ocrl_acnet_ppo_fwd_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const long long* actions, const float* old_log_prob,
                           const float* advantages, const float* returns, float clip_range, float vf_coef, float ent_coef, int normalize_advantage,
                           float* scalars, float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_acnet_ppo_fwd_bwd";
    RC(check_loss(d, normalize_advantage, who));
    const HeadSpec s = ac_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && actions && old_log_prob && advantages && returns && scalars && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    a.actions = actions; a.old_logp = old_log_prob; a.adv = advantages; a.ret = returns;
    a.clip = clip_range; a.vf_coef = vf_coef; a.ent_coef = ent_coef; a.norm = normalize_advantage ? 1 : 0;
    a.dx = dfeatures;
    if (a.norm) RC(acnet_adv_stats_launch(advantages, d->B, ws + y.stats, st));
    RC(acnet_ppo_launch(a, st));
    return reduce_loss(a, y, dw, 5, scalars, st);
}

int ocrl_acnet_a2c_fwd_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const long long* actions, const float* advantages,
                           const float* returns, float vf_coef, float ent_coef, int normalize_advantage, float* scalars, float* dfeatures,
                           float* const* dw, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_acnet_a2c_fwd_bwd";
    RC(check_loss(d, normalize_advantage, who));
    const HeadSpec s = ac_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && actions && advantages && returns && scalars && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    a.actions = actions; a.adv = advantages; a.ret = returns;
    a.vf_coef = vf_coef; a.ent_coef = ent_coef; a.norm = normalize_advantage ? 1 : 0;
    a.dx = dfeatures;
    if (a.norm) RC(acnet_adv_stats_launch(advantages, d->B, ws + y.stats, st));
    RC(acnet_a2c_launch(a, st));
    return reduce_loss(a, y, dw, 3, scalars, st);
}

int ocrl_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values, const float* dones, float* advantages,
             float* returns, int T, int E, float gamma, float gae_lambda, void* stream) {
    OCRL_REQUIRE(rewards && values && episode_starts && last_values && dones && advantages && returns, "ocrl_gae: null argument");
    OCRL_REQUIRE(T >= 1 && E >= 1 && (long long)T * E < (1LL << 31), "ocrl_gae: steps >= 1, envs >= 1 and steps * envs < 2^31 (got %d, %d)", T, E);
    return acnet_gae_launch(rewards, values, episode_starts, last_values, dones, advantages, returns, T, E, gamma, gae_lambda, static_cast<hipStream_t>(stream));
}

}  // extern "C"
