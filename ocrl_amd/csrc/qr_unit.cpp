// C ABI of DQN's quantile head (include/ocrl_hip_qr.h: ocrl_qr_*).  Stateless: the caller owns parameters, gradients and the workspace.
// Parameter order (w, dw): (weight, bias) per layer of the chain, then the advantage Linear's, then, with dueling, the value Linear's.
// The workspace is the Q head's (acnet_host.h) over this head's parameter list: the saved layer outputs, the slabs of partial gradients,
// the slabs' scalar sums.
#include <cmath>

#include "../../include/ocrl_hip_qr.h"
#include "acnet_host.h"
#include "qr.h"

namespace {
static_assert(sizeof(ocrl_qr_desc::dims) == ACNET_MAX_LAYERS * sizeof(int) && sizeof(ocrl_qr_desc::acts) == ACNET_MAX_LAYERS * sizeof(int),
              "ocrl_qr_desc holds the layers of one acnet trunk");
static_assert(sizeof(ocrl_qr_desc) == (6 + 2 * ACNET_MAX_LAYERS) * sizeof(int), "ocrl_qr_desc is 22 ints without padding");

// the chain is the policy trunk, the advantage Linear [A * N, last] the action head, the dueling value Linear [N, last] reads the chain too
HeadSpec qr_spec(const ocrl_qr_desc* d) {
    HeadSpec s;
    s.B = d->B; s.F = d->F; s.n[1] = d->n; s.dims[1] = d->dims; s.acts[1] = d->acts;
    s.na = d->A * d->N; s.nv = d->dueling ? d->N : 0; s.vt = 1;
    return s;
}

int check_qr(const ocrl_qr_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    RC(check_batch(d->B, d->F, who));
    OCRL_REQUIRE(d->A >= 1 && d->A <= ACNET_MAX_ACTIONS, "%s: 1 <= n_actions <= %d (got %d)", who, ACNET_MAX_ACTIONS, d->A);
    OCRL_REQUIRE(d->N >= 1 && d->N <= QR_MAX_QUANTILES, "%s: 1 <= n_quantiles <= %d (got %d)", who, QR_MAX_QUANTILES, d->N);
    OCRL_REQUIRE(d->A * d->N <= QR_MAX_COLS, "%s: n_actions * n_quantiles <= %d (got %d * %d)", who, QR_MAX_COLS, d->A, d->N);
    return check_layers(qr_spec(d), false, QR_MAX_COLS, who);
}

int check_kappa(float kappa, const char* who) {
    OCRL_REQUIRE(std::isfinite(kappa) && kappa > 0.f, "%s: kappa finite and > 0 (got %g)", who, (double)kappa);
    return 0;
}

// what the head's kernels take beside the tile code's arguments: AcnetArgs::A is the number of actions here, not the action Linear's rows
QrArgs qr_args(AcnetArgs& a, const ocrl_qr_desc* d) {
    a.A = d->A;
    QrArgs c{};
    c.N = d->N;
    return c;
}
}  // namespace

extern "C" {

size_t ocrl_qr_desc_size(void) { return sizeof(ocrl_qr_desc); }

size_t ocrl_qr_ws_floats(const ocrl_qr_desc* d) {
    if (check_qr(d, "ocrl_qr_ws_floats")) return 0;                    // the shapes the other entries reject get no workspace
    return head_layout(qr_spec(d)).total;
}

int ocrl_qr_fwd(const ocrl_qr_desc* d, const float* features, const float* const* w, float* quantiles, float* q, int save, float* ws,
                size_t ws_floats, void* stream) {
    const char* who = "ocrl_qr_fwd";
    RC(check_qr(d, who));
    const HeadSpec s = qr_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w, "%s: null argument", who);
    OCRL_REQUIRE(quantiles || q, "%s: quantiles and q are both null: nothing to write", who);
    RC(check_ptrs(w, y.np, who));
    if (save) RC(ws_check(who, ws ? ws_floats : (size_t)0, y.total));
    AcnetArgs a;
    head_args(a, s, y, features, w, save ? ws : nullptr, save != 0);
    QrArgs c = qr_args(a, d);
    c.quantiles = quantiles; c.q = q;
    return qr_fwd_launch(a, c, static_cast<hipStream_t>(stream));
}

int ocrl_qr_bwd(const ocrl_qr_desc* d, const float* features, const float* const* w, const float* dquantiles, float* dfeatures, float* const* dw,
                float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_qr_bwd";
    RC(check_qr(d, who));
    const HeadSpec s = qr_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && dquantiles && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    QrArgs c = qr_args(a, d);
    c.dquantiles = dquantiles; a.dx = dfeatures;
    RC(qr_bwd_launch(a, c, st));
    return reduce_dw(a, y, dw, st);
}

int ocrl_qr_act(const ocrl_qr_desc* d, const float* features, const float* const* w, unsigned long long seed, unsigned long long row_offset,
                float epsilon, const float* uniforms, long long* actions, float* q, void* stream) {
    const char* who = "ocrl_qr_act";
    RC(check_qr(d, who));
    const HeadSpec s = qr_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && actions, "%s: null argument", who);
    RC(check_ptrs(w, y.np, who));
    AcnetArgs a;
    head_args(a, s, y, features, w, nullptr, false);
    QrArgs c = qr_args(a, d);
    c.q = q;
    const DqnActArgs t{seed, row_offset, epsilon, uniforms, actions};
    return qr_act_launch(a, c, t, static_cast<hipStream_t>(stream));
}

int ocrl_qr_td_fwd_bwd(const ocrl_qr_desc* d, const float* features, const float* const* w, const float* next_quantiles, const float* next_q,
                       const long long* actions, const float* rewards, const unsigned char* dones, const float* discounts, const float* weights,
                       float gamma, float kappa, float* scalars, float* row_loss, float* dfeatures, float* const* dw, float* ws, size_t ws_floats,
                       void* stream) {
    const char* who = "ocrl_qr_td_fwd_bwd";
    RC(check_qr(d, who));
    RC(check_kappa(kappa, who));
    const HeadSpec s = qr_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && next_quantiles && next_q && actions && rewards && dones && scalars && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats));
    const QrArgs c = qr_args(a, d);
    a.dx = dfeatures;
    const QrTdArgs t{next_quantiles, {next_q, actions, rewards, dones, discounts, weights, gamma, row_loss}, kappa};
    RC(qr_td_launch(a, c, t, st));
    RC(reduce_dw(a, y, dw, st));
    return head_scalars_launch(a.scal_slab, y.S, d->B, false, scalars, st);
}

}  // extern "C"
