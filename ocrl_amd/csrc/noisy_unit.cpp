// C ABI of DQN's noisy linear layers (include/ocrl_hip_noisy.h: ocrl_noisy_*).  Stateless: the caller owns the parameters, the noise
// factors, the effective tensors and the gradients.  Pointer order (mu, sigma, w_eff, dw_eff, dsigma): (weight, bias) per layer.
#include "../../include/ocrl_hip_noisy.h"
#include "noisy.h"

namespace {
static_assert(sizeof(ocrl_noisy_desc::in) == NOISY_MAX_LAYERS * sizeof(int) && sizeof(ocrl_noisy_desc::out) == NOISY_MAX_LAYERS * sizeof(int),
              "ocrl_noisy_desc holds NOISY_MAX_LAYERS layers");
static_assert(sizeof(ocrl_noisy_desc) == (1 + 2 * NOISY_MAX_LAYERS) * sizeof(int), "ocrl_noisy_desc is 21 ints without padding");
static_assert(NOISY_MAX_LAYERS <= 16 && NOISY_MAX_WIDTH <= (1 << 27), "the counter of a draw is (l << 28) | (s << 27) | i");

int check_noisy(const ocrl_noisy_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    OCRL_REQUIRE(d->n_layers >= 1 && d->n_layers <= NOISY_MAX_LAYERS, "%s: 1 <= n_layers <= %d (got %d)", who, NOISY_MAX_LAYERS, d->n_layers);
    for (int l = 0; l < d->n_layers; ++l)
        OCRL_REQUIRE(d->in[l] >= 1 && d->in[l] <= NOISY_MAX_WIDTH && d->out[l] >= 1 && d->out[l] <= NOISY_MAX_WIDTH,
                     "%s: 1 <= in, out <= %d (layer %d has in %d, out %d)", who, NOISY_MAX_WIDTH, l, d->in[l], d->out[l]);
    return 0;
}

// every entry of a pointer array present and 16-byte aligned
int check_ptrs(const void* const* w, int np, const char* who) {
    OCRL_REQUIRE(w, "%s: null argument", who);
    for (int q = 0; q < np; ++q) OCRL_REQUIRE(w[q], "%s: parameter pointer %d of %d is null", who, q, np);
    for (int q = 0; q < np; ++q) OCRL_REQUIRE(aligned16(w[q]), "%s: parameter pointer %d of %d is not 16-byte aligned", who, q, np);
    return 0;
}

// the layer table of a launch: a / s are read (s may be null: the gradient has no second operand), dst is written
void fill_args(NoisyArgs& a, const ocrl_noisy_desc* d, const float* const* src, const float* const* s, const float* factors, float* const* dst) {
    a = NoisyArgs{};
    const NoisyFactorLayout y = noisy_factor_layout(d);
    a.n_layers = d->n_layers;
    a.factors = factors;
    for (int l = 0; l < d->n_layers; ++l) {
        NoisyLayer& L = a.lay[l];
        L.in = d->in[l]; L.out = d->out[l]; L.fin = y.fin[l]; L.fout = y.fout[l];
        L.a_w = src[2 * l]; L.a_b = src[2 * l + 1];
        if (s) { L.s_w = s[2 * l]; L.s_b = s[2 * l + 1]; }
        L.dst_w = dst[2 * l]; L.dst_b = dst[2 * l + 1];
    }
}
}  // namespace

extern "C" {

size_t ocrl_noisy_desc_size(void) { return sizeof(ocrl_noisy_desc); }

size_t ocrl_noisy_factor_floats(const ocrl_noisy_desc* d) {
    if (check_noisy(d, "ocrl_noisy_factor_floats")) return 0;          // the shapes the other entries reject get no buffer
    return (size_t)noisy_factor_layout(d).total;
}

int ocrl_noisy_factors(const ocrl_noisy_desc* d, unsigned long long seed, unsigned long long draw, const float* eps, float* factors, void* stream) {
    RC(check_noisy(d, "ocrl_noisy_factors"));
    OCRL_REQUIRE(factors, "ocrl_noisy_factors: null argument");
    NoisyFactorArgs a{};
    a.lay = noisy_factor_layout(d);
    a.n_layers = d->n_layers;
    for (int l = 0; l < d->n_layers; ++l) { a.in[l] = d->in[l]; a.out[l] = d->out[l]; }
    a.seed = seed; a.draw = draw; a.eps = eps; a.factors = factors;
    return noisy_factors_launch(a, static_cast<hipStream_t>(stream));
}

int ocrl_noisy_perturb(const ocrl_noisy_desc* d, const float* const* mu, const float* const* sigma, const float* factors, float* const* w_eff,
                       void* stream) {
    RC(check_noisy(d, "ocrl_noisy_perturb"));
    OCRL_REQUIRE(mu && sigma && factors && w_eff, "ocrl_noisy_perturb: null argument");
    OCRL_REQUIRE(aligned16(factors), "ocrl_noisy_perturb: factors must be 16-byte aligned");
    const int np = 2 * d->n_layers;
    RC(check_ptrs((const void* const*)mu, np, "ocrl_noisy_perturb"));
    RC(check_ptrs((const void* const*)sigma, np, "ocrl_noisy_perturb"));
    RC(check_ptrs((const void* const*)w_eff, np, "ocrl_noisy_perturb"));
    NoisyArgs a;
    fill_args(a, d, mu, sigma, factors, w_eff);
    return noisy_apply_launch(a, false, static_cast<hipStream_t>(stream));
}

int ocrl_noisy_grad(const ocrl_noisy_desc* d, const float* const* dw_eff, const float* factors, float* const* dsigma, void* stream) {
    RC(check_noisy(d, "ocrl_noisy_grad"));
    OCRL_REQUIRE(dw_eff && factors && dsigma, "ocrl_noisy_grad: null argument");
    OCRL_REQUIRE(aligned16(factors), "ocrl_noisy_grad: factors must be 16-byte aligned");
    const int np = 2 * d->n_layers;
    RC(check_ptrs((const void* const*)dw_eff, np, "ocrl_noisy_grad"));
    RC(check_ptrs((const void* const*)dsigma, np, "ocrl_noisy_grad"));
    NoisyArgs a;
    fill_args(a, d, dw_eff, nullptr, factors, dsigma);
    return noisy_apply_launch(a, true, static_cast<hipStream_t>(stream));
}

}  // extern "C"
