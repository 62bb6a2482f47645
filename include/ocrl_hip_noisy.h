/* C ABI of DQN's noisy linear layers in libocrl_hip.so (gfx950): the factorised Gaussian parameter noise of NoisyNet (Fortunato et al.
 * 2018, section 3b), the sixth component of Rainbow (Hessel et al. 2018).  A sixth header beside ocrl_hip.h, ocrl_hip_dqn.h,
 * ocrl_hip_rollout.h, ocrl_hip_replay.h and ocrl_hip_c51.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads them all); the
 * conventions are ocrl_hip_c51.h's: every entry is stateless and takes device pointers (fp32), an `int` entry returns 0 on success and the
 * message of a failure is ocrl_last_error(), every argument is checked before any launch, work is enqueued on `stream` (a hipStream_t) with
 * no host synchronisation, there are no atomics, every loop is bounded and the results are bit-reproducible.
 *
 * The layers sit in front of the heads of ocrl_hip_dqn.h and ocrl_hip_c51.h, which take their parameters as a host array of device
 * pointers: ocrl_noisy_perturb writes the perturbed (effective) weights of one draw into tensors of the caller's, which are handed to the
 * unchanged heads as `w`, and ocrl_noisy_grad forms the gradient of the noise scales from the `dw` the heads produce.  The gradient of mu
 * is dw itself: there is no entry for it.
 *
 * The descriptor: n_layers Linear layers, layer l with in[l] inputs and out[l] outputs (10 = 8 hidden layers + advantage + value; the
 *   layers need not chain: a dueling head's advantage and value layers share their input).
 *   Limits: 1 <= n_layers <= 10 and 1 <= in[l], out[l] <= 65536.  Anything else is rejected before any launch: ocrl_noisy_factor_floats
 *   returns 0, the other entries non-zero, each with an ocrl_last_error message that names the limit.
 *   Pointer arrays: mu, sigma, w_eff, dw_eff and dsigma are host arrays of 2 * n_layers device pointers, (weight [out, in], bias [out]) per
 *   layer in descriptor order.  A null entry is rejected ("parameter pointer i of n is null").  Every tensor is dense and its base pointer
 *   16-byte aligned; in[l] is free, so the rows of a weight are not aligned and nothing assumes that they are.
 *
 * `factors`: the noise of one draw, ocrl_noisy_factor_floats(d) floats.  Layers in order; per layer f_in (in[l] floats), then f_out (out[l]
 *   floats); each of the two blocks is rounded up to a multiple of 4 floats and the padding is written as 0.
 *
 * ocrl_noisy_factors: one launch.  Element i of side s (0 = in, 1 = out) of layer l of draw t takes one 64-bit word (x, y) of the
 *   library's counter RNG at site 440 of stream `seed`, at the counter ((t mod 2^32) << 32) | (l << 28) | (s << 27) | i (the key's high
 *   word is t mod 2^32, the counter's low word (l << 28) | (s << 27) | i):
 *     u0 = fp32((x >> 8) + 0.5) / 2^24,  u1 = fp32((y >> 8) + 0.5) / 2^24      -- the sum rounded to fp32 (to even): u in (0, 1]
 *     g  = sqrt(-2 log u0) * cos(6.2831853 u1)          -- Box-Muller with the fast hardware log and cos, the library's Gaussian
 *     f  = copysign(sqrt(|g|), g)
 *   `eps`, when given, replaces g: it has the layout of `factors` (its padding is not read).  The entry writes exactly the f that
 *   ocrl_noisy_perturb and ocrl_noisy_grad are then given; neither of them draws.
 *
 * ocrl_noisy_perturb: one launch over all layers.  Each value is the fp32 operations in the order written, each rounded once (no fused
 *   multiply-add):
 *     p = f_out[o] * f_in[i];   w_eff[o, i] = mu[o, i] + sigma[o, i] * p
 *     b_eff[o] = b_mu[o] + b_sigma[o] * f_out[o]
 *
 * ocrl_noisy_grad: one launch over all layers.  The cotangent dw_eff of w_eff -> dsigma, overwritten, with the same rounded p:
 *     dsigma_w[o, i] = dw_eff[o, i] * p;   dsigma_b[o] = db_eff[o] * f_out[o] */
#ifndef OCRL_HIP_NOISY_H
#define OCRL_HIP_NOISY_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int n_layers;
    int in[10];
    int out[10];
} ocrl_noisy_desc;
size_t ocrl_noisy_desc_size(void);
size_t ocrl_noisy_factor_floats(const ocrl_noisy_desc* d);
int ocrl_noisy_factors(const ocrl_noisy_desc* d, unsigned long long seed, unsigned long long draw, const float* eps /* may be NULL = draw */,
                       float* factors, void* stream);
int ocrl_noisy_perturb(const ocrl_noisy_desc* d, const float* const* mu, const float* const* sigma, const float* factors,
                       float* const* w_eff, void* stream);
int ocrl_noisy_grad(const ocrl_noisy_desc* d, const float* const* dw_eff, const float* factors, float* const* dsigma, void* stream);

#ifdef __cplusplus
}
#endif
#endif
