// C ABI of DQN's categorical head (include/ocrl_hip_c51.h: ocrl_c51_*).  Stateless: the caller owns parameters, gradients and the
// workspace.  Parameter order (w, dw): (weight, bias) per layer of the chain, then the advantage Linear's, then, with dueling, the value
// Linear's.  The workspace is the Q head's (acnet_host.h) over this head's parameter list: the saved layer outputs, the slabs of partial
// gradients, the slabs' scalar sums.
#include <cmath>

#include "../../include/ocrl_hip_c51.h"
#include "acnet_host.h"
#include "c51.h"

namespace {
static_assert(sizeof(ocrl_c51_desc::dims) == ACNET_MAX_LAYERS * sizeof(int) && sizeof(ocrl_c51_desc::acts) == ACNET_MAX_LAYERS * sizeof(int),
              "ocrl_c51_desc holds the layers of one acnet trunk");
static_assert(sizeof(ocrl_c51_desc) == (6 + 2 * ACNET_MAX_LAYERS) * sizeof(int), "ocrl_c51_desc is 22 ints without padding");

// the chain is the policy trunk, the advantage Linear [A * Z, last] the action head, the dueling value Linear [Z, last] reads the chain too
HeadSpec c51_spec(const ocrl_c51_desc* d) {
    HeadSpec s;
    s.B = d->B; s.F = d->F; s.n[1] = d->n; s.dims[1] = d->dims; s.acts[1] = d->acts;
    s.na = d->A * d->Z; s.nv = d->dueling ? d->Z : 0; s.vt = 1;
    return s;
}

int check_c51(const ocrl_c51_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    RC(check_batch(d->B, d->F, who));
    OCRL_REQUIRE(d->A >= 1 && d->A <= ACNET_MAX_ACTIONS, "%s: 1 <= n_actions <= %d (got %d)", who, ACNET_MAX_ACTIONS, d->A);
    OCRL_REQUIRE(d->Z >= 2 && d->Z <= C51_MAX_ATOMS, "%s: 2 <= n_atoms <= %d (got %d)", who, C51_MAX_ATOMS, d->Z);
    OCRL_REQUIRE(d->A * d->Z <= C51_MAX_COLS, "%s: n_actions * n_atoms <= %d (got %d * %d)", who, C51_MAX_COLS, d->A, d->Z);
    return check_layers(c51_spec(d), false, C51_MAX_COLS, who);
}

int check_support(float v_min, float v_max, const char* who) {
    OCRL_REQUIRE(std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max, "%s: v_min < v_max, both finite (got %g, %g)", who, (double)v_min,
                 (double)v_max);
    return 0;
}

// what the head's kernels take beside the tile code's arguments: AcnetArgs::A is the number of actions here, not the action Linear's rows
C51Args c51_args(AcnetArgs& a, const ocrl_c51_desc* d, float v_min, float v_max) {
    a.A = d->A;
    C51Args c{};
    c.Z = d->Z; c.v_min = v_min; c.v_max = v_max; c.dz = (v_max - v_min) / (float)(d->Z - 1);
    return c;
}
}  // namespace

extern "C" {

size_t ocrl_c51_desc_size(void) { return sizeof(ocrl_c51_desc); }

size_t ocrl_c51_ws_floats(const ocrl_c51_desc* d) {
    if (check_c51(d, "ocrl_c51_ws_floats")) return 0;                  // the shapes the other entries reject get no workspace
    return head_layout(c51_spec(d)).total;
}

int ocrl_c51_fwd(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max, float* logits, float* probs, float* q,
                 int save, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_c51_fwd";
    RC(check_c51(d, who));
    RC(check_support(v_min, v_max, who));
    const HeadSpec s = c51_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w, "%s: null argument", who);
    OCRL_REQUIRE(logits || probs || q, "%s: logits, probs and q are all null: nothing to write", who);
    RC(check_ptrs(w, y.np, who));
    if (save) RC(ws_check(who, ws ? ws_floats : (size_t)0, y.total));
    AcnetArgs a;
    head_args(a, s, y, features, w, save ? ws : nullptr, save != 0);
    C51Args c = c51_args(a, d, v_min, v_max);
    c.logits = logits; c.probs = probs; c.q = q;
    return c51_fwd_launch(a, c, static_cast<hipStream_t>(stream));
}

int ocrl_c51_bwd(const ocrl_c51_desc* d, const float* features, const float* const* w, const float* dlogits, float* dfeatures, float* const* dw,
                 float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_c51_bwd";
    RC(check_c51(d, who));
    const HeadSpec s = c51_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && dlogits && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    C51Args c = c51_args(a, d, 0.f, 1.f);                              // the support plays no part in the backward of the logits
    c.dlogits = dlogits; a.dx = dfeatures;
    RC(c51_bwd_launch(a, c, st));
    return reduce_dw(a, y, dw, st);
}

int ocrl_c51_act(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max, unsigned long long seed,
                 unsigned long long row_offset, float epsilon, const float* uniforms, long long* actions, float* q, void* stream) {
    const char* who = "ocrl_c51_act";
    RC(check_c51(d, who));
    RC(check_support(v_min, v_max, who));
    const HeadSpec s = c51_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && actions, "%s: null argument", who);
    RC(check_ptrs(w, y.np, who));
    AcnetArgs a;
    head_args(a, s, y, features, w, nullptr, false);
    C51Args c = c51_args(a, d, v_min, v_max);
    c.q = q;
    const DqnActArgs t{seed, row_offset, epsilon, uniforms, actions};
    return c51_act_launch(a, c, t, static_cast<hipStream_t>(stream));
}

int ocrl_c51_td_fwd_bwd(const ocrl_c51_desc* d, const float* features, const float* const* w, float v_min, float v_max, const float* next_probs,
                        const float* next_q, const long long* actions, const float* rewards, const unsigned char* dones, const float* discounts,
                        const float* weights, float gamma, float* scalars, float* row_loss, float* dfeatures, float* const* dw, float* ws,
                        size_t ws_floats, void* stream) {
    const char* who = "ocrl_c51_td_fwd_bwd";
    RC(check_c51(d, who));
    RC(check_support(v_min, v_max, who));
    const HeadSpec s = c51_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && next_probs && next_q && actions && rewards && dones && scalars && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    const C51Args c = c51_args(a, d, v_min, v_max);
    a.dx = dfeatures;
    const C51TdArgs t{next_probs, {next_q, actions, rewards, dones, discounts, weights, gamma, row_loss}};
    RC(c51_td_launch(a, c, t, st));
    RC(reduce_dw(a, y, dw, st));
    return head_scalars_launch(a.scal_slab, y.S, d->B, false, scalars, st);
}

}  // extern "C"
