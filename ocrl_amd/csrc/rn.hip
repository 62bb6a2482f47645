// Relation Network pooling (poolings/rn/rn_module.py:8-59): the kernels around the GEMMs of g and f that the GEMM cannot express.
// Pairs are the ordered pairs (i, j), i != j, of one image's K slots in itertools.permutations order: p = i * (K - 1) + j - (j > i),
// P = K (K - 1) rows per image, row b * P + p.  The first layer of g is factored (rn_unit.cpp): [A | Bq] = s [U | V]^T on the B K slot
// rows (U, V = the halves of its weight), so its pair row (i, j) is relu(A_i + Bq_j + b1).
//   rn_pair_fwd      h1[b, p] = relu(AB[b, i, 0:g] + AB[b, j, g:2g] + b1)                                   thread = float4 of a pair row
//   rn_pair_bwd      dAB[b, k, 0:g] = sum_j dh1[b, (k, j)],  dAB[b, k, g:2g] = sum_i dh1[b, (i, k)]         thread = float4 of a slot row
//   rn_pairsum_fwd   y[b] = sum_p gL[b, p]                                                                   thread = float4 of an image row
//   rn_pairsum_bwd   dgL[b, p] = dy[b] * (gL[b, p] > 0)                                                      thread = float4 of a pair row
// Every sum is one thread's loop in ascending index order: no atomics, results are reproducible bit for bit.  dh1 arrives already
// masked by h1 > 0 (the dX product of the next g layer applies the mask in its epilogue, or rn_pairsum_bwd when g has one layer).
#include "common.h"
#include "kernels.h"

__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

__global__ __launch_bounds__(256) void rn_pair_fwd_kernel(const float* __restrict__ AB, const float* __restrict__ b1, float* __restrict__ h1,
                                                          long long n4, int K, int g4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n4) return;
    const int c = (int)(t % g4);
    const long long row = t / g4;
    const int P = K * (K - 1);
    const long long b = row / P;
    const int p = (int)(row - b * P);
    const int i = p / (K - 1), jj = p - i * (K - 1), j = jj + (jj >= i);
    const float4* ab = reinterpret_cast<const float4*>(AB);
    float4 v = ab[(b * K + i) * 2 * g4 + c];
    add4(v, ab[(b * K + j) * 2 * g4 + g4 + c]);
    add4(v, reinterpret_cast<const float4*>(b1)[c]);
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    reinterpret_cast<float4*>(h1)[t] = v;
}

__global__ __launch_bounds__(256) void rn_pair_bwd_kernel(const float* __restrict__ dh1, float* __restrict__ dAB, long long n4, int K, int g4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n4) return;
    const int c2 = (int)(t % (2 * g4));
    const long long row = t / (2 * g4);                 // b * K + k
    const long long b = row / K;
    const int k = (int)(row - b * K), K1 = K - 1;
    const float4* d = reinterpret_cast<const float4*>(dh1) + b * K * K1 * g4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c2 < g4) {                                      // k as the first slot of the pair: rows k (K-1) .. k (K-1) + K - 2
        for (int jj = 0; jj < K1; ++jj) add4(s, d[(long long)(k * K1 + jj) * g4 + c2]);
    } else {                                            // k as the second slot: row i (K-1) + k - (k > i) of every i != k
        const int c = c2 - g4;
        for (int i = 0; i < K; ++i)
            if (i != k) add4(s, d[(long long)(i * K1 + k - (k > i)) * g4 + c]);
    }
    reinterpret_cast<float4*>(dAB)[t] = s;
}

__global__ __launch_bounds__(256) void rn_pairsum_fwd_kernel(const float* __restrict__ g, float* __restrict__ y, long long n4, int P, int g4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n4) return;
    const int c = (int)(t % g4);
    const long long b = t / g4;
    const float4* src = reinterpret_cast<const float4*>(g) + b * P * g4 + c;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = 0; p < P; ++p) add4(s, src[(long long)p * g4]);
    reinterpret_cast<float4*>(y)[t] = s;
}

__global__ __launch_bounds__(256) void rn_pairsum_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ g, float* __restrict__ dg, long long n4,
                                                             int P, int g4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n4) return;
    const int c = (int)(t % g4);
    const long long b = t / g4 / P;
    const float4 d = reinterpret_cast<const float4*>(dy)[b * g4 + c];
    const float4 v = reinterpret_cast<const float4*>(g)[t];
    reinterpret_cast<float4*>(dg)[t] = make_float4(v.x > 0.f ? d.x : 0.f, v.y > 0.f ? d.y : 0.f, v.z > 0.f ? d.z : 0.f, v.w > 0.f ? d.w : 0.f);
}

int rn_pair_fwd_launch(const float* AB, const float* b1, float* h1, int B, int K, int g, hipStream_t st) {
    OCRL_REQUIRE(K >= 2 && g % 4 == 0, "rn_pair_fwd: K >= 2 and g %% 4 == 0 (got %d, %d)", K, g);
    const long long n4 = (long long)B * K * (K - 1) * (g / 4);
    hipLaunchKernelGGL(rn_pair_fwd_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, st, AB, b1, h1, n4, K, g / 4);
    OCRL_CHECK_LAUNCH("rn_pair_fwd");
    return 0;
}
int rn_pair_bwd_launch(const float* dh1, float* dAB, int B, int K, int g, hipStream_t st) {
    OCRL_REQUIRE(K >= 2 && g % 4 == 0, "rn_pair_bwd: K >= 2 and g %% 4 == 0 (got %d, %d)", K, g);
    const long long n4 = (long long)B * K * (g / 2);
    hipLaunchKernelGGL(rn_pair_bwd_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, st, dh1, dAB, n4, K, g / 4);
    OCRL_CHECK_LAUNCH("rn_pair_bwd");
    return 0;
}
int rn_pairsum_fwd_launch(const float* gL, float* y, int B, int P, int g, hipStream_t st) {
    OCRL_REQUIRE(P >= 1 && g % 4 == 0, "rn_pairsum_fwd: P >= 1 and g %% 4 == 0 (got %d, %d)", P, g);
    const long long n4 = (long long)B * (g / 4);
    hipLaunchKernelGGL(rn_pairsum_fwd_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, st, gL, y, n4, P, g / 4);
    OCRL_CHECK_LAUNCH("rn_pairsum_fwd");
    return 0;
}
int rn_pairsum_bwd_launch(const float* dy, const float* gL, float* dgL, int B, int P, int g, hipStream_t st) {
    OCRL_REQUIRE(P >= 1 && g % 4 == 0, "rn_pairsum_bwd: P >= 1 and g %% 4 == 0 (got %d, %d)", P, g);
    const long long n4 = (long long)B * P * (g / 4);
    hipLaunchKernelGGL(rn_pairsum_bwd_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, st, dy, gL, dgL, n4, P, g / 4);
    OCRL_CHECK_LAUNCH("rn_pairsum_bwd");
    return 0;
}
