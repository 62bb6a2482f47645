// C ABI of DQN's implicit quantile head (include/ocrl_hip_iqn.h: ocrl_iqn_*).  Stateless: the caller owns parameters, gradients and the
// workspace.  Parameter order (w, dw): the cosine embedding's (weight, bias), (weight, bias) per layer of the chain, then the output
// Linear's.  The workspace is the Q head's (acnet_host.h) over E = B * N expanded rows with the embedding as the shared trunk's one
// layer (the saved layer outputs, phi first; the slabs of partial gradients; the slabs' scalar sums), then this head's four blocks.
#include <cmath>

#include "../../include/ocrl_hip_iqn.h"
#include "acnet_host.h"
#include "iqn.h"

namespace {
static_assert(sizeof(ocrl_iqn_desc::dims) == ACNET_MAX_LAYERS * sizeof(int) && sizeof(ocrl_iqn_desc::acts) == ACNET_MAX_LAYERS * sizeof(int),
              "ocrl_iqn_desc holds the layers of one acnet trunk");
static_assert(sizeof(ocrl_iqn_desc) == (6 + 2 * ACNET_MAX_LAYERS) * sizeof(int), "ocrl_iqn_desc is 22 ints without padding");
constexpr long long IQN_MAX_ROWS = (1LL << 31) / ACNET_MAX_WIDTH;     // expanded rows of one call: row * width stays an int32

// the embedding's one layer: the shared trunk of the head, C -> F, ReLU
struct IqnSpec {
    int edim[1], eact[1];
    HeadSpec s;
};

// The tile code's view: E rows of C "features", the embedding as the shared trunk, the chain as the policy trunk, the output Linear
// [A, last] as the action head.  The spec points into `out`, which must outlive it.
void iqn_spec(const ocrl_iqn_desc* d, IqnSpec& out) {
    out.edim[0] = d->F; out.eact[0] = 1;
    HeadSpec& s = out.s;
    s = HeadSpec{};
    s.B = d->B * d->N; s.F = d->C;
    s.n[0] = 1; s.dims[0] = out.edim; s.acts[0] = out.eact;
    s.n[1] = d->n; s.dims[1] = d->dims; s.acts[1] = d->acts;
    s.na = d->A;
}

int check_samples(int N, const char* what, const char* who) {
    OCRL_REQUIRE(N >= 1 && N <= IQN_MAX_SAMPLES, "%s: 1 <= %s <= %d (got %d)", who, what, IQN_MAX_SAMPLES, N);
    return 0;
}

int check_iqn(const ocrl_iqn_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    OCRL_REQUIRE(d->B >= 1, "%s: batch >= 1 (got %d)", who, d->B);
    OCRL_REQUIRE(d->F >= 4 && d->F <= ACNET_MAX_WIDTH && d->F % 4 == 0, "%s: feature_dim is a multiple of 4 in 4 .. %d (got %d)", who,
                 ACNET_MAX_WIDTH, d->F);
    OCRL_REQUIRE(d->A >= 1 && d->A <= ACNET_MAX_ACTIONS, "%s: 1 <= n_actions <= %d (got %d)", who, ACNET_MAX_ACTIONS, d->A);
    RC(check_samples(d->N, "n_samples", who));
    OCRL_REQUIRE(d->C >= 4 && d->C <= IQN_MAX_COS && d->C % 4 == 0, "%s: n_cos is a multiple of 4 in 4 .. %d (got %d)", who, IQN_MAX_COS, d->C);
    OCRL_REQUIRE((long long)d->B * d->N < IQN_MAX_ROWS, "%s: batch * n_samples < %lld expanded rows (got %d * %d)", who, IQN_MAX_ROWS, d->B, d->N);
    IqnSpec sp;
    iqn_spec(d, sp);
    return check_layers(sp.s, false, 0, who);
}

int check_kappa(float kappa, const char* who) {
    OCRL_REQUIRE(std::isfinite(kappa) && kappa > 0.f, "%s: kappa finite and > 0 (got %g)", who, (double)kappa);
    return 0;
}

// the head's layout with this head's blocks behind it
struct IqnLay {
    HeadLay y;
    size_t theta, part, tha, dzphi, total;
};
IqnLay iqn_layout(const ocrl_iqn_desc* d, const HeadSpec& s) {
    IqnLay l;
    l.y = head_layout(s);
    WsTake take;
    take.end = l.y.total;
    const size_t E = (size_t)s.B;
    l.theta = take(E * d->A);
    l.part = take(E);
    l.tha = take(E);
    l.dzphi = take(E * d->F);
    l.total = take.end;
    return l;
}

// what the head's kernels take beside the tile code's arguments
IqnArgs iqn_args(const ocrl_iqn_desc* d, const float* features, const float* taus) {
    IqnArgs c{};
    c.Bb = d->B; c.N = d->N; c.C = d->C;
    c.feat = features; c.taus = taus;
    return c;
}
}  // namespace

int iqn_fqf_act(const ocrl_iqn_desc* d, const char* who, const float* features, const float* const* w, const float* taus, const DqnActArgs& t,
                float* q, hipStream_t st) {
    RC(check_iqn(d, who));
    IqnSpec sp;
    iqn_spec(d, sp);
    const HeadLay y = head_layout(sp.s);
    RC(check_ptrs(w, y.np, who));
    AcnetArgs a;
    head_args(a, sp.s, y, nullptr, w, nullptr, false);
    IqnArgs c = iqn_args(d, features, taus);
    c.q = q;
    return iqn_act_fqf_launch(a, c, t, st);
}

extern "C" {

size_t ocrl_iqn_desc_size(void) { return sizeof(ocrl_iqn_desc); }

size_t ocrl_iqn_ws_floats(const ocrl_iqn_desc* d) {
    if (check_iqn(d, "ocrl_iqn_ws_floats")) return 0;                   // the shapes the other entries reject get no workspace
    IqnSpec sp;
    iqn_spec(d, sp);
    return iqn_layout(d, sp.s).total;
}

int ocrl_iqn_taus(unsigned long long seed, unsigned long long row_offset, int B, int N, float* out, void* stream) {
    const char* who = "ocrl_iqn_taus";
    OCRL_REQUIRE(B >= 1, "%s: batch >= 1 (got %d)", who, B);
    RC(check_samples(N, "n_samples", who));
    OCRL_REQUIRE(out, "%s: null argument", who);
    return iqn_taus_launch(seed, row_offset, B, N, out, static_cast<hipStream_t>(stream));
}

int ocrl_iqn_fwd(const ocrl_iqn_desc* d, const float* features, const float* taus, const float* const* w, float* quantiles, float* q, int save,
                 float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_iqn_fwd";
    RC(check_iqn(d, who));
    IqnSpec sp;
    iqn_spec(d, sp);
    const IqnLay l = iqn_layout(d, sp.s);
    OCRL_REQUIRE(features && taus && w, "%s: null argument", who);
    OCRL_REQUIRE(quantiles || q, "%s: quantiles and q are both null: nothing to write", who);
    RC(check_ptrs(w, l.y.np, who));
    const bool need_ws = save || !quantiles;
    if (need_ws) RC(ws_check(who, ws ? ws_floats : (size_t)0, l.total));
    AcnetArgs a;
    head_args(a, sp.s, l.y, nullptr, w, save ? ws : nullptr, save != 0);
    IqnArgs c = iqn_args(d, features, taus);
    c.theta = quantiles ? quantiles : ws + l.theta;
    c.q = q;
    return iqn_fwd_launch(a, c, static_cast<hipStream_t>(stream));
}

int ocrl_iqn_bwd(const ocrl_iqn_desc* d, const float* features, const float* taus, const float* const* w, const float* dquantiles,
                 float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_iqn_bwd";
    RC(check_iqn(d, who));
    IqnSpec sp;
    iqn_spec(d, sp);
    const IqnLay l = iqn_layout(d, sp.s);
    OCRL_REQUIRE(features && taus && w && dquantiles && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(ws_check(who, ws_floats, l.total));
    RC(head_begin(a, sp.s, l.y, who, nullptr, w, dw, ws, ws_floats));
    IqnArgs c = iqn_args(d, features, taus);
    c.dquantiles = dquantiles;
    if (dfeatures) { c.dfeat = dfeatures; c.dzphi = ws + l.dzphi; }
    RC(iqn_bwd_launch(a, c, st));
    return reduce_dw(a, l.y, dw, st);
}

int ocrl_iqn_act(const ocrl_iqn_desc* d, const float* features, const float* const* w, unsigned long long seed, unsigned long long row_offset,
                 float epsilon, const float* uniforms, const float* taus, long long* actions, float* q, void* stream) {
    const char* who = "ocrl_iqn_act";
    RC(check_iqn(d, who));
    IqnSpec sp;
    iqn_spec(d, sp);
    const HeadLay y = head_layout(sp.s);
    OCRL_REQUIRE(features && w && actions, "%s: null argument", who);
    RC(check_ptrs(w, y.np, who));
    AcnetArgs a;
    head_args(a, sp.s, y, nullptr, w, nullptr, false);
    IqnArgs c = iqn_args(d, features, taus);
    c.q = q;
    const DqnActArgs t{seed, row_offset, epsilon, uniforms, actions};
    return iqn_act_launch(a, c, t, static_cast<hipStream_t>(stream));
}

int ocrl_iqn_td_fwd_bwd(const ocrl_iqn_desc* d, const float* features, const float* taus, const float* const* w, const float* next_quantiles,
                        int Np, const float* next_q, const long long* actions, const float* rewards, const unsigned char* dones,
                        const float* discounts, const float* weights, float gamma, float kappa, float* scalars, float* row_loss,
                        float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_iqn_td_fwd_bwd";
    RC(check_iqn(d, who));
    RC(check_samples(Np, "n_target_samples", who));
    RC(check_kappa(kappa, who));
    IqnSpec sp;
    iqn_spec(d, sp);
    const IqnLay l = iqn_layout(d, sp.s);
    OCRL_REQUIRE(features && taus && w && next_quantiles && next_q && actions && rewards && dones && scalars && dw && ws, "%s: null argument", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(ws_check(who, ws_floats, l.total));
    RC(head_begin(a, sp.s, l.y, who, nullptr, w, dw, ws, ws_floats));
    IqnArgs c = iqn_args(d, features, taus);
    if (dfeatures) { c.dfeat = dfeatures; c.dzphi = ws + l.dzphi; }
    const IqnTdArgs t{next_quantiles, Np, {next_q, actions, rewards, dones, discounts, weights, gamma, row_loss}, kappa, ws + l.part, ws + l.tha};
    RC(iqn_td_launch(a, c, t, st));
    RC(reduce_dw(a, l.y, dw, st));
    return head_scalars_launch(a.scal_slab, cdiv(d->B, 16) < ACNET_MAX_SLABS ? cdiv(d->B, 16) : ACNET_MAX_SLABS, d->B, false, scalars, st);
}

}  // extern "C"
