// C ABI of DQN's fully parameterized quantile function (include/ocrl_hip_fqf.h: ocrl_fqf_*).  Stateless: the caller owns every tensor
// and the workspace.  ocrl_fqf_act hands the head's descriptor to the implicit quantile head's own checks and act kernel (iqn.h).
#include <cmath>
#include <cstdint>

#include "../../include/ocrl_hip_fqf.h"
#include "fqf.h"
#include "iqn.h"

namespace {
static_assert(sizeof(ocrl_fqf_desc) == sizeof(ocrl_iqn_desc) && offsetof(ocrl_fqf_desc, dims) == offsetof(ocrl_iqn_desc, dims) &&
                  offsetof(ocrl_fqf_desc, acts) == offsetof(ocrl_iqn_desc, acts) && offsetof(ocrl_fqf_desc, n) == offsetof(ocrl_iqn_desc, n),
              "ocrl_fqf_desc is ocrl_iqn_desc field for field");
static_assert(2 * FQF_MAX_FRACTIONS - 1 <= IQN_MAX_SAMPLES, "eval_taus fits the head's fractions per row");

int check_batch(int B, const char* who) {
    OCRL_REQUIRE(B >= 1, "%s: batch >= 1 (got %d)", who, B);
    return 0;
}
int check_features(int F, const char* who) {
    OCRL_REQUIRE(F >= 4 && F <= FQF_MAX_FEATURES && F % 4 == 0, "%s: feature_dim is a multiple of 4 in 4 .. %d (got %d)", who, FQF_MAX_FEATURES, F);
    return 0;
}
int check_fractions(int N, const char* who) {
    OCRL_REQUIRE(N >= 2 && N <= FQF_MAX_FRACTIONS, "%s: 2 <= n_fractions <= %d (got %d)", who, FQF_MAX_FRACTIONS, N);
    return 0;
}
int check_actions(int A, const char* who) {
    OCRL_REQUIRE(A >= 1 && A <= FQF_MAX_ACTIONS, "%s: 1 <= n_actions <= %d (got %d)", who, FQF_MAX_ACTIONS, A);
    return 0;
}
}  // namespace

extern "C" {

size_t ocrl_fqf_desc_size(void) { return sizeof(ocrl_fqf_desc); }

size_t ocrl_fqf_ws_floats(int B, int F, int N) {
    const char* who = "ocrl_fqf_ws_floats";
    if (check_batch(B, who) || check_features(F, who) || check_fractions(N, who)) return 0;
    return (size_t)fqf_slabs(B) * fqf_stride(F, N);
}

int ocrl_fqf_fractions(const float* features, const float* Wf, const float* bf, int B, int F, int N, float* taus, float* tau_hats,
                       float* eval_taus, float* logp, float* entropy, void* stream) {
    const char* who = "ocrl_fqf_fractions";
    RC(check_batch(B, who));
    RC(check_features(F, who));
    RC(check_fractions(N, who));
    OCRL_REQUIRE(features && Wf && bf && taus, "%s: null argument", who);
    int L = 2;
    while (L < N) L <<= 1;
    const FqfFracArgs a{features, Wf, bf, B, F, N, L, taus, tau_hats, eval_taus, logp, entropy};
    return fqf_fractions_launch(a, static_cast<hipStream_t>(stream));
}

int ocrl_fqf_q(const float* quantiles, const float* taus, int B, int A, int N, float* q, void* stream) {
    const char* who = "ocrl_fqf_q";
    RC(check_batch(B, who));
    RC(check_actions(A, who));
    RC(check_fractions(N, who));
    OCRL_REQUIRE(quantiles && taus && q, "%s: null argument", who);
    return fqf_q_launch(quantiles, taus, B, A, N, q, static_cast<hipStream_t>(stream));
}

int ocrl_fqf_act(const ocrl_fqf_desc* d, const float* features, const float* const* w, const float* taus, unsigned long long seed,
                 unsigned long long row_offset, float epsilon, const float* uniforms, long long* actions, float* q, void* stream) {
    const char* who = "ocrl_fqf_act";
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    RC(check_fractions(d->N, who));
    OCRL_REQUIRE(features && w && taus && actions, "%s: null argument", who);
    const DqnActArgs t{seed, row_offset, epsilon, uniforms, actions};
    return iqn_fqf_act(reinterpret_cast<const ocrl_iqn_desc*>(d), who, features, w, taus, t, q, static_cast<hipStream_t>(stream));
}

int ocrl_fqf_fraction_bwd(const float* features, const float* logp, const float* entropy, const float* quantiles, const long long* actions,
                          const float* weights, float ent_coef, int B, int F, int A, int N, float* dWf, float* dbf, float* scalars, float* ws,
                          size_t ws_floats, void* stream) {
    const char* who = "ocrl_fqf_fraction_bwd";
    RC(check_batch(B, who));
    RC(check_features(F, who));
    RC(check_actions(A, who));
    RC(check_fractions(N, who));
    OCRL_REQUIRE(std::isfinite(ent_coef), "%s: ent_coef finite (got %g)", who, (double)ent_coef);
    OCRL_REQUIRE(features && logp && entropy && quantiles && actions && dWf && dbf && scalars && ws, "%s: null argument", who);
    OCRL_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "%s: workspace 8-byte aligned (it holds the scalars' fp64 sums)", who);
    const int S = fqf_slabs(B);
    const size_t stride = fqf_stride(F, N);
    OCRL_REQUIRE(ws_floats >= (size_t)S * stride, "%s: workspace of %zu floats, ocrl_fqf_ws_floats asks for %zu", who, ws_floats, (size_t)S * stride);
    const FqfBwdArgs a{features, logp, entropy, quantiles, actions, weights, ent_coef, B, F, A, N, S, cdiv(B, FQF_ROWS), (int)stride,
                       ws, dWf, dbf, scalars};
    return fqf_bwd_launch(a, static_cast<hipStream_t>(stream));
}

}  // extern "C"
