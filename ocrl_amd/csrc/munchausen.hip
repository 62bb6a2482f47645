// DQN's Munchausen targets (include/ocrl_hip_munchausen.h states the arithmetic; munchausen.h the arguments): the clipped log-policy bonus
// on the rewards and the soft value of the target network's soft-max policy in place of its values at the next observation.  A few
// thousand elements: the launch is latency-bound, so one 64-lane workgroup takes one batch row and walks it in the order the header
// states.  Lane a holds action a's terms in LDS; the sums over the actions are serial and every lane that needs one forms it itself in
// the same order from the same LDS words, so no value crosses lanes through a reduction.  Built with -ffp-contract=off; the roundings
// are spelled with the round-to-nearest intrinsics besides, which are never fused.
#include "munchausen.h"

namespace {
constexpr int NL = 64;             // lanes of a workgroup: one wave, MUNCHAUSEN_MAX_ACTIONS and MUNCHAUSEN_MAX_SAMPLES
static_assert(MUNCHAUSEN_MAX_ACTIONS <= NL && MUNCHAUSEN_MAX_SAMPLES <= NL, "one lane per action and per target sample");

// s_a of the row in sx, given its maximum
__device__ __forceinline__ float scaled(const float* sx, int a, float v, float tau) { return __fdiv_rn(__fsub_rn(sx[a], v), tau); }

// Reads x[0 .. A) into sx (lane a its own element) and returns the row's maximum in v and logf(Z) as the result, the same bits in every
// lane.  se is scratch.  Two barriers; the caller puts one between two uses of the same arrays.
__device__ __forceinline__ float row_log_z(const float* __restrict__ x, int A, float tau, float* sx, float* se, float& v) {
    const int t = threadIdx.x;
    if (t < A) sx[t] = x[t];
    __syncthreads();
    v = sx[0];
    for (int a = 1; a < A; ++a) v = fmaxf(v, sx[a]);
    if (t < A) se[t] = expf(scaled(sx, t, v, tau));
    __syncthreads();
    float Z = 0.f;
    for (int a = 0; a < A; ++a) Z = __fadd_rn(Z, se[a]);
    return logf(Z);
}

__global__ __launch_bounds__(NL) void munchausen_kernel(MunchausenArgs p) {
    __shared__ float sx[NL], se[NL], sp[NL], sc[NL], sm[NL];
    const int t = threadIdx.x, A = p.A, Np = p.Np;
    const long long b = blockIdx.x;

    // the bonus: c of the action taken under the policy of cur_q[b, :]
    float v;
    float lz = row_log_z(p.cur_q + b * A, A, p.tau, sx, se, v);
    if (t == 0) {
        long long a = p.actions[b];
        a = a < 0 ? 0 : a >= A ? A - 1 : a;
        const float c = __fmul_rn(p.tau, __fsub_rn(scaled(sx, (int)a, v, p.tau), lz));
        p.rewards_out[b] = __fadd_rn(p.rewards[b], __fmul_rn(p.alpha, fminf(0.f, fmaxf(p.clip_lo, c))));
    }

    float* __restrict__ nv = p.next_v + b * A;
    float* __restrict__ nm = Np ? p.next_m + b * A * Np : nullptr;
    const int cols = A * Np;
    if (p.dones[b]) {                                          // uniform: a finished row's next inputs are never read
        if (t < A) nv[t] = 0.f;
        for (int e = t; e < cols; e += NL) nm[e] = 0.f;
        return;
    }
    __syncthreads();                                           // every lane is done with cur_q's sx / se

    // the soft value: pi and c of next_q[b, :]
    lz = row_log_z(p.next_q + b * A, A, p.tau, sx, se, v);
    if (t < A) {
        const float lp = __fsub_rn(scaled(sx, t, v, p.tau), lz);
        sp[t] = expf(lp);
        sc[t] = __fmul_rn(p.tau, lp);
    }
    __syncthreads();
    float V = 0.f;
    for (int a = 0; a < A; ++a) V = __fmaf_rn(sp[a], __fsub_rn(sx[a], sc[a]), V);
    if (t < A) nv[t] = V;
    if (!Np) return;                                           // uniform
    if (t < Np) {
        const float* __restrict__ q = p.next_quantiles + b * A * Np + t;
        float M = 0.f;
        for (int a = 0; a < A; ++a) M = __fmaf_rn(sp[a], __fsub_rn(q[(long long)a * Np], sc[a]), M);
        sm[t] = M;
    }
    __syncthreads();
    for (int e = t; e < cols; e += NL) nm[e] = sm[e % Np];     // next_m[b, a, j] = M_bj for every a: consecutive lanes, consecutive floats
}
}  // namespace

int munchausen_launch(const MunchausenArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(munchausen_kernel, dim3((unsigned)a.B), dim3(NL), 0, st, a);
    OCRL_CHECK_LAUNCH("munchausen_targets");
    return 0;
}
