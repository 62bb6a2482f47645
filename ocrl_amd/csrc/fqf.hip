// DQN's fully parameterized quantile function (include/ocrl_hip_fqf.h states the arithmetic; fqf.h the arguments): the proposal of the
// fractions, the probability-weighted q and the fraction loss's gradient into the proposal's Linear.  A few thousand elements each: the
// launches are latency-bound.
//   fqf_fractions  a row sits in L = the power of two >= N consecutive lanes of one wave, 64 / L rows to a wave, four waves to a
//                  workgroup: lane i forms z_i (in fp64, rounded to fp32 once the maximum is off), the maximum is a butterfly over the L lanes, and the serial sums (Z and its prefixes
//                  c_i, the entropy) are formed by every lane itself from the same broadcast words in the same order, so all lanes of a
//                  row hold the same bits.  Cross-lane moves only: no LDS word, no barrier.  Lanes past N or past the batch go through
//                  every move and write nothing.
//   fqf_q          one thread per (b, a): the serial fold over i
//   fqf_bwd        workgroup s walks the groups s, s + S, ... of 8 rows: thread r < 8 walks row r's N fractions serially (g, dp, s,
//                  dz, the row's loss) into LDS, then thread e adds the group's 8 terms of output element e to its word of the slab.
//                  The two reported scalars are sums that cancel (the loss) or run over the whole batch: they are carried in fp64, the
//                  slab's first four floats holding the two doubles, and rounded once by the fold
//   fqf_bwd_fold   one thread per output element: the slabs in slab order
// Built with -ffp-contract=off; the roundings are spelled with the round-to-nearest intrinsics besides, which are never fused.  No atomics.
#include "fqf.h"

namespace {
constexpr int NT = 256;
constexpr int LN = FQF_MAX_FRACTIONS + 1;          // row stride of the LDS arrays of the backward

__global__ __launch_bounds__(NT) void fqf_fractions_kernel(FqfFracArgs p) {
    const int L = p.L, N = p.N, F = p.F;
    const int i = threadIdx.x & (L - 1);
    const long long row = (long long)blockIdx.x * (NT / L) + threadIdx.x / L;
    const bool in_batch = row < p.B, live = i < N;
    const long long r = in_batch ? row : (long long)p.B - 1;         // a lane past the batch walks the last row and writes nothing
    double z = -INFINITY;                                            // fp64: a logit far below the maximum keeps its digits (logp, H)
    if (live) {
        const float* __restrict__ w = p.Wf + (long long)i * F;
        const float* __restrict__ x = p.x + r * F;
        double acc = (double)p.bf[i];
        for (int j = 0; j < F; ++j) acc += (double)w[j] * (double)x[j];              // the product of two floats is exact in fp64
        z = acc;
    }
    double m = z;
    for (int o = L >> 1; o; o >>= 1) m = fmax(m, __shfl_xor(m, o, L));
    const float zm = live ? (float)(z - m) : 0.f;
    const float e = live ? expf(zm) : 0.f;
    float c = 0.f, Z = 0.f;                                          // c_i is Z as it stood before e_i went in
    for (int k = 0; k < N; ++k) {
        const float ek = __shfl(e, k, L);
        if (k == i) c = Z;
        Z = __fadd_rn(Z, ek);
    }
    const float lp = __fsub_rn(zm, logf(Z));
    const float pr = expf(lp);
    const float pl = live ? __fmul_rn(pr, lp) : 0.f;
    float hs = 0.f;
    for (int k = 0; k < N; ++k) hs = __fadd_rn(hs, __shfl(pl, k, L));
    if (!live || !in_batch) return;                                  // every cross-lane move is behind us
    const float t0 = __fdiv_rn(c, Z), t1 = __fdiv_rn(__fadd_rn(c, e), Z);      // c + e is c_{i+1} as lane i + 1 holds it; Z for i = N - 1
    const float th = fqf_tau_hat(t0, t1);
    float* __restrict__ taus = p.taus + row * (N + 1);
    taus[i] = t0;
    if (i == N - 1) taus[N] = t1;
    if (p.tau_hats) p.tau_hats[row * N + i] = th;
    if (p.eval_taus) {
        float* __restrict__ ev = p.eval_taus + row * (2 * N - 1);
        if (i) ev[i - 1] = t0;
        ev[N - 1 + i] = th;
    }
    if (p.logp) p.logp[row * N + i] = lp;
    if (p.entropy && i == 0) p.entropy[row] = -hs;
}

__global__ __launch_bounds__(NT) void fqf_q_kernel(const float* __restrict__ theta, const float* __restrict__ taus, long long total, int A, int N,
                                                   float* __restrict__ q) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const float* __restrict__ t = taus + (e / A) * (N + 1);
    const float* __restrict__ th = theta + e * N;
    float acc = 0.f;
    for (int i = 0; i < N; ++i) acc = fqf_q_term(acc, t[i], t[i + 1], th[i]);
    q[e] = acc;
}

__global__ __launch_bounds__(NT) void fqf_bwd_kernel(FqfBwdArgs p) {
    __shared__ float sp[FQF_ROWS][LN], sg[FQF_ROWS][LN], sdz[FQF_ROWS][LN];
    __shared__ double sl[FQF_ROWS][2];
    const int N = p.N, F = p.F, A = p.A, tid = threadIdx.x;
    const int NF = N * F, total = NF + N;
    double* __restrict__ sums = reinterpret_cast<double*>(p.slab + (size_t)blockIdx.x * p.stride);       // 256-byte aligned: the stride is a multiple of 64 floats
    float* __restrict__ slab = p.slab + (size_t)blockIdx.x * p.stride + FQF_SLAB_HEAD;
    for (int grp = blockIdx.x; grp < p.ngroups; grp += p.S) {
        const long long b0 = (long long)grp * FQF_ROWS;
        const int rows = p.B - b0 < FQF_ROWS ? (int)(p.B - b0) : FQF_ROWS;
        if (tid < FQF_ROWS) {
            float *pr = sp[tid], *g = sg[tid], *dz = sdz[tid];
            double l = 0.0;
            float H = 0.f;
            if (tid < rows) {
                const long long row = b0 + tid;
                long long a = p.actions[row];
                a = a < 0 ? 0 : a >= A ? A - 1 : a;
                const float sc = __fdiv_rn(p.weights ? p.weights[row] : 1.f, (float)p.B);
                const float* __restrict__ th = p.quantiles + (row * A + a) * (2 * N - 1);
                const float* __restrict__ lp = p.logp + row * N;
                H = p.entropy[row];
                for (int k = 0; k < N; ++k) pr[k] = expf(lp[k]);
                double t = 0.0;                                      // the reported loss: fp64 sums of the fp32 p_k and g_i
                for (int i = 1; i < N; ++i) {
                    t += (double)pr[i - 1];
                    const float gi = __fmul_rn(sc, __fsub_rn(__fsub_rn(__fmul_rn(2.f, th[i - 1]), th[N - 1 + i]), th[N - 2 + i]));
                    g[i] = gi;
                    l += (double)gi * t;
                }
                float* dp = dz;                                      // dz_k overwrites dp_k once s is known
                dp[N - 1] = 0.f;
                for (int k = N - 2; k >= 0; --k) dp[k] = __fadd_rn(dp[k + 1], g[k + 1]);
                float s = 0.f;
                for (int k = 0; k < N; ++k) s = __fadd_rn(s, __fmul_rn(pr[k], dp[k]));
                const float ec = __fdiv_rn(p.ent_coef, (float)p.B);
                for (int k = 0; k < N; ++k)
                    dz[k] = __fadd_rn(__fmul_rn(pr[k], __fsub_rn(dp[k], s)), __fmul_rn(__fmul_rn(ec, pr[k]), __fadd_rn(lp[k], H)));
            }
            sl[tid][0] = l; sl[tid][1] = (double)H;
        }
        __syncthreads();
        const bool first = grp == (int)blockIdx.x;
        for (int e = tid; e < total; e += NT) {
            float acc = first ? 0.f : slab[e];
            if (e < NF) {
                const int k = e / F, j = e - k * F;
                for (int r = 0; r < rows; ++r) acc = __fadd_rn(acc, __fmul_rn(sdz[r][k], p.x[(b0 + r) * F + j]));
            } else {
                for (int r = 0; r < rows; ++r) acc = __fadd_rn(acc, sdz[r][e - NF]);
            }
            slab[e] = acc;
        }
        if (tid < 2) {
            double acc = first ? 0.0 : sums[tid];
            for (int r = 0; r < rows; ++r) acc += sl[r][tid];
            sums[tid] = acc;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void fqf_bwd_fold_kernel(FqfBwdArgs p) {
    const int NF = p.N * p.F, total = NF + p.N + 2;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    if (e >= NF + p.N) {                                             // the two scalars: fp64, rounded once
        const int k = e - NF - p.N;
        double acc = 0.0;
        for (int s = 0; s < p.S; ++s) acc += reinterpret_cast<const double*>(p.slab + (size_t)s * p.stride)[k];
        p.scalars[k] = (float)(k ? acc / (double)p.B : acc);
        return;
    }
    float acc = 0.f;
    for (int s = 0; s < p.S; ++s) acc = __fadd_rn(acc, p.slab[(size_t)s * p.stride + FQF_SLAB_HEAD + e]);
    if (e < NF) p.dWf[e] = acc;
    else p.dbf[e - NF] = acc;
}
}  // namespace

int fqf_fractions_launch(const FqfFracArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(fqf_fractions_kernel, dim3(cdiv(a.B, NT / a.L)), dim3(NT), 0, st, a);
    OCRL_CHECK_LAUNCH("fqf_fractions");
    return 0;
}
int fqf_q_launch(const float* quantiles, const float* taus, int B, int A, int N, float* q, hipStream_t st) {
    const long long total = (long long)B * A;
    hipLaunchKernelGGL(fqf_q_kernel, GRID1D(total), 0, st, quantiles, taus, total, A, N, q);
    OCRL_CHECK_LAUNCH("fqf_q");
    return 0;
}
int fqf_bwd_launch(const FqfBwdArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(fqf_bwd_kernel, dim3(a.S), dim3(NT), 0, st, a);
    OCRL_CHECK_LAUNCH("fqf_bwd");
    hipLaunchKernelGGL(fqf_bwd_fold_kernel, GRID1D(a.N * a.F + a.N + 2), 0, st, a);
    OCRL_CHECK_LAUNCH("fqf_bwd_fold");
    return 0;
}
