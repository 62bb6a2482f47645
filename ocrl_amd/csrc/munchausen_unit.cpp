// C ABI of DQN's Munchausen targets (include/ocrl_hip_munchausen.h: ocrl_munchausen_targets).  Stateless: the caller owns every tensor.
#include <cmath>

#include "../../include/ocrl_hip_munchausen.h"
#include "munchausen.h"

extern "C" {

int ocrl_munchausen_targets(const float* cur_q, const float* next_q, const float* next_quantiles, int Np, const long long* actions,
                            const float* rewards, const unsigned char* dones, int B, int A, float alpha, float tau, float clip_lo,
                            float* rewards_out, float* next_v, float* next_m, void* stream) {
    const char* who = "ocrl_munchausen_targets";
    OCRL_REQUIRE(B >= 1, "%s: batch >= 1 (got %d)", who, B);
    OCRL_REQUIRE(A >= 1 && A <= MUNCHAUSEN_MAX_ACTIONS, "%s: 1 <= n_actions <= %d (got %d)", who, MUNCHAUSEN_MAX_ACTIONS, A);
    OCRL_REQUIRE((Np == 0 && !next_quantiles && !next_m) || (Np >= 1 && Np <= MUNCHAUSEN_MAX_SAMPLES && next_quantiles && next_m),
                 "%s: n_target_samples is 0 with next_quantiles and next_m both null, or 1 <= n_target_samples <= %d with both given (got %d, "
                 "next_quantiles %s, next_m %s)", who, MUNCHAUSEN_MAX_SAMPLES, Np, next_quantiles ? "given" : "null", next_m ? "given" : "null");
    OCRL_REQUIRE(alpha >= 0.f && alpha <= 1.f, "%s: alpha in [0, 1] (got %g)", who, (double)alpha);
    OCRL_REQUIRE(std::isfinite(tau) && tau > 0.f, "%s: tau finite and > 0 (got %g)", who, (double)tau);
    OCRL_REQUIRE(std::isfinite(clip_lo) && clip_lo <= 0.f, "%s: clip_lo finite and <= 0 (got %g)", who, (double)clip_lo);
    OCRL_REQUIRE(cur_q && next_q && actions && rewards && dones && rewards_out && next_v, "%s: null argument", who);
    const MunchausenArgs a{cur_q, next_q, next_quantiles, actions, rewards, dones, B, A, Np, alpha, tau, clip_lo, rewards_out, next_v, next_m};
    return munchausen_launch(a, static_cast<hipStream_t>(stream));
}

}  // extern "C"
