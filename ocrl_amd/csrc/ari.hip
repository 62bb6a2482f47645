// Segmentation ARI counts (utils/tools.py:309-320 of the reference, with the foreground masking of slate_module.py:211-213 and
// iodine_module.py:263-265 folded in): per image, the contingency table of (true label, predicted label) over the pixels and the three
// pair sums the adjusted Rand index is made of, in exact integers.
//   ari_count   one workgroup per chunk of an image's pixels.  A lane takes VEC pixels and walks the channels of both stacks once, keeping
//               the first maximum (torch.argmax: strict >, a NaN beats every number, the first NaN stays).  fuse_fg: the predicted
//               scores are attn_k * fg for k < K and fg for k = K, fg = 1 - truth[Ct-1]; one fp32 subtract and one fp32 multiply
//               (__fsub_rn / __fmul_rn: never contracted), so every tie of the three torch lines is reproduced.
//               Counting: nearly every pixel of a wave falls in one or two bins, so the wave aggregates before it touches LDS: the
//               first pending lane's bin is broadcast, the lanes that share it are balloted, one lane adds the popcount; after
//               AGG_ROUNDS rounds the few lanes left add 1 each.  One Ct x Cp histogram per workgroup in LDS, its non-zero bins
//               added to the global table with integer atomics (order-independent: two runs agree exactly).
//               VEC = 4: both stacks pixel-contiguous and 16-byte aligned, one 16-byte load per lane and channel.  VEC = 1: any
//               element strides, e.g. the [B, N, K] attention buffer of the SLATE engine read in place (a lane's K scores are
//               adjacent, the wave's loads of one pass share their cache lines with the next).
//   ari_sums    one wave per image, after ari_count on the same stream: sum C(n_ij), sum C(a_i), sum C(b_j), C(x) = x (x - 1) / 2.
// Every index that addresses memory comes from the arguments checked in ocrl_ari_counts: b < B, channel < Ct / Cp, pixel < N.
#include "common.h"
#include "../../include/ocrl_hip.h"

namespace {

constexpr int ARI_THREADS = 256;
constexpr int ARI_MAX_BINS = OCRL_ARI_MAX_CHANNELS * OCRL_ARI_MAX_CHANNELS;
constexpr int AGG_ROUNDS = 4;

struct AriStack { const float* p; long long sb, sc, sn; int C; };

template <int VEC>
__device__ inline void ari_load(const float* p, long long sn, int cnt, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        if (cnt == 4) {                                   // sn == 1 and p 16-byte aligned (checked by the launcher)
            const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = q[i];
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = i < cnt ? p[i * sn] : 0.f;
}

// torch.argmax's order: v replaces best when it is greater, or when it is the first NaN
__device__ inline void ari_take(float v, int c, float& best, int& idx) {
    if (v > best || (v != v && best == best)) { best = v; idx = c; }
}

__device__ inline void ari_add(int* hist, int code, bool valid) {
    bool todo = valid;
    for (int r = 0; r < AGG_ROUNDS; ++r) {
        if (!__any(todo)) return;
        if (todo) {
            const int lead = __builtin_amdgcn_readfirstlane(code);
            if (code == lead) {
                const unsigned long long m = __ballot(1);
                if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&hist[lead], __popcll(m));
                todo = false;
            }
        }
    }
    if (todo) atomicAdd(&hist[code], 1);
}

template <int VEC>
__global__ __launch_bounds__(ARI_THREADS) void ari_count_kernel(AriStack T, AriStack P, int fuse_fg, long long N, int chunk, int G,
                                                                int* __restrict__ table) {
    __shared__ int hist[ARI_MAX_BINS];
    const int b = blockIdx.x / G, g = blockIdx.x % G;
    const int Cp = P.C + (fuse_fg ? 1 : 0), bins = T.C * Cp;
    for (int i = threadIdx.x; i < bins; i += ARI_THREADS) hist[i] = 0;
    __syncthreads();
    const long long start = (long long)g * chunk, end = start + chunk < N ? start + chunk : N;
    const float* tp = T.p + b * T.sb;
    const float* pp = P.p + b * P.sb;                     // never dereferenced when P.C == 0
    for (long long n0 = start + (long long)threadIdx.x * VEC; n0 < end; n0 += ARI_THREADS * VEC) {
        const int cnt = end - n0 < VEC ? (int)(end - n0) : VEC;
        float v[VEC], best[VEC], fg[VEC];
        int ti[VEC], pi[VEC];
        ari_load<VEC>(tp + n0 * T.sn, T.sn, cnt, best);
#pragma unroll
        for (int i = 0; i < VEC; ++i) { ti[i] = 0; fg[i] = best[i]; }
        for (int c = 1; c < T.C; ++c) {
            ari_load<VEC>(tp + c * T.sc + n0 * T.sn, T.sn, cnt, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) { ari_take(v[i], c, best[i], ti[i]); fg[i] = v[i]; }
        }
        // predicted label: channels 0 .. P.C-1 from memory (times fg when fused), then fg itself as channel P.C when fused
        if (fuse_fg) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) fg[i] = __fsub_rn(1.f, fg[i]);
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) pi[i] = 0;
        for (int c = 0; c < P.C; ++c) {
            ari_load<VEC>(pp + c * P.sc + n0 * P.sn, P.sn, cnt, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float s = fuse_fg ? __fmul_rn(v[i], fg[i]) : v[i];
                if (c == 0) best[i] = s;
                else ari_take(s, c, best[i], pi[i]);
            }
        }
        if (fuse_fg && P.C > 0) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) ari_take(fg[i], P.C, best[i], pi[i]);
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) ari_add(hist, ti[i] * Cp + pi[i], i < cnt);
    }
    __syncthreads();
    int* tb = table + (long long)b * bins;
    for (int i = threadIdx.x; i < bins; i += ARI_THREADS)
        if (hist[i]) atomicAdd(&tb[i], hist[i]);
}

__device__ inline long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int lo = __shfl_xor((int)(unsigned)(unsigned long long)v, o, 64), hi = __shfl_xor((int)((unsigned long long)v >> 32), o, 64);
        v += (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    }
    return v;
}

__global__ __launch_bounds__(64) void ari_sums_kernel(const int* __restrict__ table, int Ct, int Cp, long long* __restrict__ sums) {
    const int lane = threadIdx.x, bins = Ct * Cp;
    const int* t = table + (long long)blockIdx.x * bins;
    long long s_ij = 0, s_a = 0, s_b = 0;
    for (int i = lane; i < bins; i += 64) { const long long x = t[i]; s_ij += x * (x - 1) / 2; }
    if (lane < Ct) {
        long long a = 0;
        for (int j = 0; j < Cp; ++j) a += t[lane * Cp + j];
        s_a = a * (a - 1) / 2;
    }
    if (lane < Cp) {
        long long c = 0;
        for (int i = 0; i < Ct; ++i) c += t[i * Cp + lane];
        s_b = c * (c - 1) / 2;
    }
    s_ij = wave_sum_i64(s_ij); s_a = wave_sum_i64(s_a); s_b = wave_sum_i64(s_b);
    if (lane == 0) {
        long long* o = sums + (long long)blockIdx.x * 3;
        o[0] = s_ij; o[1] = s_a; o[2] = s_b;
    }
}

bool ari_vec4(const float* p, long long sb, long long sc, long long sn) {
    return sn == 1 && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && sb % 4 == 0 && sc % 4 == 0;
}

}  // namespace

extern "C" int ocrl_ari_counts(const float* truth, long long t_sb, long long t_sc, long long t_sn, int Ct, const float* pred, long long p_sb,
                               long long p_sc, long long p_sn, int Cp, int fuse_fg, int B, long long N, int* table, long long* sums, void* stream) {
    const int M = OCRL_ARI_MAX_CHANNELS;
    OCRL_REQUIRE(Ct >= 1 && Ct <= M && Cp >= 1 && Cp <= M, "ocrl_ari_counts: invalid channel counts %d / %d (1 .. %d each)", Ct, Cp, M);
    OCRL_REQUIRE(B >= 1 && N >= 1 && N <= 0x7fffffffLL, "ocrl_ari_counts: invalid batch %d or pixel count %lld (counts are int32)", B, N);
    const int K = fuse_fg ? Cp - 1 : Cp;                  // channels read from pred
    OCRL_REQUIRE(truth && table && sums && (pred || K == 0), "ocrl_ari_counts: invalid (null) pointer");
    OCRL_REQUIRE(t_sb >= 0 && t_sc >= 0 && t_sn >= 0 && p_sb >= 0 && p_sc >= 0 && p_sn >= 0, "ocrl_ari_counts: invalid (negative) stride");
    // pixels per workgroup: 4096, halved down to 1024 while that leaves the chip with fewer than 1024 workgroups
    int chunk = 4096;
    while (chunk > 1024 && (long long)B * cdiv(N, chunk) < 1024) chunk /= 2;
    const int G = cdiv(N, chunk);
    OCRL_REQUIRE((long long)B * G <= 0x7fffffffLL, "ocrl_ari_counts: invalid size: %d images of %lld pixels exceed the grid", B, N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    OCRL_HIP(hipMemsetAsync(table, 0, sizeof(int) * (size_t)B * Ct * Cp, st));
    const AriStack T{truth, t_sb, t_sc, t_sn, Ct}, P{pred, p_sb, p_sc, p_sn, K};
    if (ari_vec4(truth, t_sb, t_sc, t_sn) && (K == 0 || ari_vec4(pred, p_sb, p_sc, p_sn)))
        hipLaunchKernelGGL(ari_count_kernel<4>, dim3(B * G), dim3(ARI_THREADS), 0, st, T, P, fuse_fg ? 1 : 0, N, chunk, G, table);
    else
        hipLaunchKernelGGL(ari_count_kernel<1>, dim3(B * G), dim3(ARI_THREADS), 0, st, T, P, fuse_fg ? 1 : 0, N, chunk, G, table);
    OCRL_CHECK_LAUNCH("ari_count");
    hipLaunchKernelGGL(ari_sums_kernel, dim3(B), dim3(64), 0, st, table, Ct, Cp, sums);
    OCRL_CHECK_LAUNCH("ari_sums");
    return 0;
}
