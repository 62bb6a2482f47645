// Cross attention of the transformer decoder to the K projected slots (reference: ocrs/common/transformer.py:23-50 called from
// TransformerDecoderBlock.forward :181-185 with k = v = the slot memory), folded the way slot attention is (slot_attn.hip):
// the key / value side has only K <= 16 rows per image, so the two d x d projections around the attention collapse into two small
// per-image matrices
//     scores[t, (h,k)] = LN(x)[t] . A_b[:, (h,k)],   A_b[e, (h,k)]  = dh^-1/2 * sum_j Wq[h dh + j, e] * ck_b[k, h dh + j]
//     out[t]           = sum_(h,k) Pd[t, (h,k)] Vo_b[(h,k)],   Vo_b[(h,k), o] = sum_j cv_b[k, h dh + j] * Wo[o, h dh + j]
// (ck = mem Wk^T, cv = mem Wv^T as before).  One launch per block replaces: the query projection, the attention kernel and the
// output projection (2 x 2 d^2 FLOP per token become 2 x 2 d h K) -- it reads LN(x) and the residual once and writes the new
// residual stream once.  The backward mirrors it: d Pd = d out Vo^T, soft-max backward per head, d LN(x) = d scores A^T in one
// launch; the per-image sums d Vo_b = Pd^T d out and d A_b = d scores^T LN(x) are two batched products of the GEMM family, and four
// more (batched over image and head, xattn_fold_bwd_launch below) take them back to Wq, Wo, ck, cv.  Only the summation order differs from the reference's three products.
//
// Column layout: col = head * KP + slot with the heads padded to KP = 8 (K <= 8) or 16 slots, so that on the matrix cores
// (scores^T = A^T x^T: accumulator lane = (token li, column group g'), register r = column 16 tt + 4 g' + r) a head is two (KP = 8)
// or four (KP = 16) consecutive 4-column groups of one 16-column tile: its soft-max is in-lane arithmetic plus one or two cross-row
// exchanges (v_permlane16/32_swap), and the probabilities are already the B operand of the second product.
//
// The plain form (cross_attn_*: the attention alone, between the callers' projections) is at the end of the file: generate() runs
// it one query row at a time, training with OCRL_XATTN=0 or at a shape the fold does not support.
#include "common.h"
#include "kernels.h"

#define XA_T 256          // threads per workgroup (4 waves, 16 tokens each per step)

__device__ __forceinline__ float xa_xrow16(float v, bool is_max) {
    const int a = __builtin_bit_cast(int, v);
    const auto r = __builtin_amdgcn_permlane16_swap(a, a, false, false);
    const float x = __builtin_bit_cast(float, (int)r[0]), y = __builtin_bit_cast(float, (int)r[1]);
    return is_max ? __builtin_amdgcn_fmed3f(x, y, INFINITY) : x + y;
}
__device__ __forceinline__ float xa_xrow32(float v, bool is_max) {
    const int a = __builtin_bit_cast(int, v);
    const auto r = __builtin_amdgcn_permlane32_swap(a, a, false, false);
    const float x = __builtin_bit_cast(float, (int)r[0]), y = __builtin_bit_cast(float, (int)r[1]);
    return is_max ? __builtin_amdgcn_fmed3f(x, y, INFINITY) : x + y;
}
template <int KP>
__device__ __forceinline__ float xa_head_reduce(float v, bool is_max) {      // over the KP / 4 column groups of a head
    v = xa_xrow16(v, is_max);
    if (KP == 16) v = xa_xrow32(v, is_max);
    return v;
}

// ------------------------------------------------------------------------------------------- per-image operands (all blocks, one launch)
struct XaFoldArgs {
    const float* mem;            // [B,K,d] projected slots
    const float* Wq[8]; const float* Wk[8]; const float* Wv[8]; const float* Wo[8];      // per block, [d,d] row-major (out, in)
    float* ck[8]; float* cv[8];              // [B,K,d]
    float* Ab[8]; float* AbT[8]; float* Vo[8]; float* VoT[8];      // [B,NC,d], [B,d,NC], [B,NC,d], [B,d,NC]; padding columns stay zero
    int B, K, d, h, KP, NC;
};
__global__ __launch_bounds__(256) void xattn_fold_fwd_kernel(XaFoldArgs a) {
    extern __shared__ float sm[];          // mem [K][d] | ck [K][d] | cv [K][d]
    const int b = blockIdx.x, blk = blockIdx.y, K = a.K, d = a.d, dh = d / a.h, tid = threadIdx.x;
    float* mem = sm;
    float* ck = mem + K * d;
    float* cv = ck + K * d;
    for (int i = tid; i < K * d; i += 256) mem[i] = a.mem[(size_t)b * K * d + i];
    __syncthreads();
    const float *Wq = a.Wq[blk], *Wk = a.Wk[blk], *Wv = a.Wv[blk], *Wo = a.Wo[blk];
    // ck = mem Wk^T, cv = mem Wv^T: output (which, o) per thread, all K rows at once (the weight row is read once)
    for (int i = tid; i < 2 * d; i += 256) {
        const int which = i / d, o = i - which * d;
        const float* w = (which ? Wv : Wk) + (size_t)o * d;
        float acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.f;
        for (int e = 0; e < d; e += 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(w + e);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < K) {
                    const float4 m4 = *reinterpret_cast<const float4*>(mem + k * d + e);
                    acc[k] += (w4.x * m4.x + w4.y * m4.y) + (w4.z * m4.z + w4.w * m4.w);
                }
        }
        float* dst = which ? cv : ck;
        float* gdst = (which ? a.cv[blk] : a.ck[blk]) + (size_t)b * K * d;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < K) { dst[k * d + o] = acc[k]; gdst[k * d + o] = acc[k]; }
    }
    __syncthreads();
    const float scale = rsqrtf((float)dh);
    float* Ab = a.Ab[blk] + (size_t)b * a.NC * d;
    float* AbT = a.AbT[blk] + (size_t)b * d * a.NC;
    float* Vo = a.Vo[blk] + (size_t)b * a.NC * d;
    float* VoT = a.VoT[blk] + (size_t)b * d * a.NC;
    // A_b[col][e] = scale sum_j ck[k][h dh + j] Wq[h dh + j][e]      (threads over e: coalesced weight reads)
    for (int i = tid; i < a.h * d; i += 256) {
        const int hh = i / d, e = i - hh * d;
        float acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.f;
        for (int j = 0; j < dh; ++j) {
            const float w = Wq[(size_t)(hh * dh + j) * d + e];
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < K) acc[k] += ck[k * d + hh * dh + j] * w;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < K) {
                const int col = hh * a.KP + k;
                Ab[(size_t)col * d + e] = acc[k] * scale;
                AbT[(size_t)e * a.NC + col] = acc[k] * scale;
            }
    }
    // Vo_b[col][o] = sum_j cv[k][h dh + j] Wo[o][h dh + j]
    for (int i = tid; i < a.h * d; i += 256) {
        const int hh = i / d, o = i - hh * d;
        float acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.f;
        const float* w = Wo + (size_t)o * d + hh * dh;
        for (int j = 0; j < dh; j += 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(w + j);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < K) {
                    const float4 c4 = *reinterpret_cast<const float4*>(cv + k * d + hh * dh + j);
                    acc[k] += (w4.x * c4.x + w4.y * c4.y) + (w4.z * c4.z + w4.w * c4.w);
                }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < K) {
                const int col = hh * a.KP + k;
                Vo[(size_t)col * d + o] = acc[k];
                VoT[(size_t)o * a.NC + col] = acc[k];
            }
    }
}

// ------------------------------------------------------------------------------------------- forward
struct XaArgs {
    const float* x;          // [B,T,d] LN(x): the attention input
    const float* resid;      // [B,T,d] residual stream (forward) / unused (backward)
    float* y;                // forward: new residual stream = resid + dropout(out);   backward: d LN(x)
    float* P;                // [B,h,T,K] probabilities before dropout (written by the forward, read by the backward)
    const float* Ab; const float* AbT; const float* Vo; const float* VoT;       // per-image operands of this block
    const float* gd;         // backward: gradient wrt out (after the output dropout's backward) [B,T,d]
    float* Pd; float* dS;    // backward: [B*T, NC] dropped probabilities and score gradients (operands of the per-image sums)
    int B, T, K, d, h, NS;
    float p; unsigned long long seed; unsigned site_p, site_o;
};
// LDS row strides: operands read as ds_read_b128 at [row][16c + 4g] (row = lane & 15): stride = cols + 4 spreads the 16 rows over the banks
template <int NM, int NT, int KP>
__global__ __launch_bounds__(XA_T, 3) void xattn_fwd_kernel(XaArgs a) {
    constexpr int D = 16 * NM, NC = 16 * NT, LDA = D + 4, LDV = NC + 4;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* As = sm;                    // [NC][LDA]   A_b: column-major scores operand
    float* Vs = As + NC * LDA;         // [D][LDV]    Vo_b^T
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.NS, hs = blockIdx.x % a.NS;
    const int T = a.T, K = a.K;
    {
        const float* Ab = a.Ab + (size_t)b * NC * D;
        for (int i = tid; i < NC * (D / 4); i += XA_T) {
            const int r = i / (D / 4), c4 = i - r * (D / 4);
            *reinterpret_cast<float4*>(As + r * LDA + 4 * c4) = *reinterpret_cast<const float4*>(Ab + (size_t)r * D + 4 * c4);
        }
        const float* VoT = a.VoT + (size_t)b * D * NC;
        for (int i = tid; i < D * (NC / 4); i += XA_T) {
            const int r = i / (NC / 4), c4 = i - r * (NC / 4);
            *reinterpret_cast<float4*>(Vs + r * LDV + 4 * c4) = *reinterpret_cast<const float4*>(VoT + (size_t)r * NC + 4 * c4);
        }
    }
    __syncthreads();
    const int ntile = (T + 15) / 16, per = (ntile + a.NS - 1) / a.NS;
    const int t0 = hs * per, t1 = (t0 + per < ntile) ? t0 + per : ntile;
    const uint32_t thr = drop_thresh(a.p);
    const float dsc = a.p > 0.f ? 1.0f / (1.0f - a.p) : 1.f;
    // column bookkeeping of this lane: column 16 tt + 4 g + r  ->  head = col / KP, slot = col % KP
    const int slot0 = (4 * g) % KP;                   // slot of r = 0 (the same for every tile: 16 % KP == 0)
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = slot0 + r < K ? 0.f : -1e30f;
#pragma unroll 1
    for (int t = t0 + wv; t < t1; t += XA_T / 64) {
        const int tok = t * 16 + li;
        const bool live = tok < T;
        const size_t row = ((size_t)b * T + (live ? tok : 0)) * D;
        float4 xv[NM];
#pragma unroll
        for (int c = 0; c < NM; ++c) xv[c] = live ? *reinterpret_cast<const float4*>(a.x + row + 16 * c + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        // ---- scores^T[col][tok] = A_b^T x^T
        f32x4 s[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) s[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NM; ++c) {
            float4 av[NT];
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) av[tt] = *reinterpret_cast<const float4*>(As + (16 * tt + li) * LDA + 16 * c + 4 * g);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) s[tt] = MFMA16(av[tt].x, xv[c].x, s[tt]);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) s[tt] = MFMA16(av[tt].y, xv[c].y, s[tt]);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) s[tt] = MFMA16(av[tt].z, xv[c].z, s[tt]);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) s[tt] = MFMA16(av[tt].w, xv[c].w, s[tt]);
            if ((c & 1) == 1) __builtin_amdgcn_sched_barrier(0);
        }
        // ---- soft-max over the slots of each head, dropout
        f32x4 pd[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            const int head = (16 * tt + 4 * g) / KP;
            float l[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) l[r] = s[tt][r] + bias[r];
            float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
            mx = xa_head_reduce<KP>(mx, true);
            float e[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) e[r] = __expf(l[r] - mx);
            float sum = (e[0] + e[1]) + (e[2] + e[3]);
            sum = xa_head_reduce<KP>(sum, false);
            const float inv = __builtin_amdgcn_rcpf(sum);
            const long long prow = (((long long)b * a.h + head) * T + (live ? tok : 0)) * K;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pr = e[r] * inv;
                float v = pr;
                if (slot0 + r < K) {
                    if (live) a.P[prow + slot0 + r] = pr;
                    if (a.p > 0.f) {
                        const uint64_t idx = (uint64_t)prow + slot0 + r;
                        v = rng_keep(rng_bits4(a.seed, a.site_p, idx >> 2), (int)(idx & 3), thr) ? pr * dsc : 0.f;
                    }
                } else v = 0.f;
                pd[tt][r] = v;
            }
        }
        // ---- out^T[o][tok] = Vo_b^T Pd^T
        f32x4 o[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) o[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
            for (int m = 0; m < NM; m += 4) {          // four operand rows in flight, then their 16 MFMAs (the barrier keeps later reads from being hoisted)
                float4 v4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v4[u] = *reinterpret_cast<const float4*>(Vs + (16 * (m + u) + li) * LDV + 16 * tt + 4 * g);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    o[m + u] = MFMA16(v4[u].x, pd[tt][0], o[m + u]);
                    o[m + u] = MFMA16(v4[u].y, pd[tt][1], o[m + u]);
                    o[m + u] = MFMA16(v4[u].z, pd[tt][2], o[m + u]);
                    o[m + u] = MFMA16(v4[u].w, pd[tt][3], o[m + u]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- y = resid + dropout(out): lane (token li, g) holds out[16 m + 4 g .. + 3]
        if (live) {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const float4 rvm = *reinterpret_cast<const float4*>(a.resid + row + 16 * m + 4 * g);
                float4 v = make_float4(o[m][0], o[m][1], o[m][2], o[m][3]);
                if (a.p > 0.f) {
                    const uint64_t idx = (uint64_t)row + 16 * m + 4 * g;          // multiple of 4
                    const uint2 bits = rng_bits4(a.seed, a.site_o, idx >> 2);
                    v.x = rng_keep(bits, 0, thr) ? v.x * dsc : 0.f; v.y = rng_keep(bits, 1, thr) ? v.y * dsc : 0.f;
                    v.z = rng_keep(bits, 2, thr) ? v.z * dsc : 0.f; v.w = rng_keep(bits, 3, thr) ? v.w * dsc : 0.f;
                }
                v.x += rvm.x; v.y += rvm.y; v.z += rvm.z; v.w += rvm.w;
                *reinterpret_cast<float4*>(a.y + row + 16 * m + 4 * g) = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------- backward
template <int NM, int NT, int KP>
__global__ __launch_bounds__(XA_T, 3) void xattn_bwd_kernel(XaArgs a) {
    constexpr int D = 16 * NM, NC = 16 * NT, LDA = D + 4, LDV = NC + 4;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Vs = sm;                    // [NC][LDA]   Vo_b: d Pd^T = Vo gd^T
    float* As = Vs + NC * LDA;         // [D][LDV]    A_b^T ([e][col]): d x^T = A dS^T
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.NS, hs = blockIdx.x % a.NS;
    const int T = a.T, K = a.K;
    {
        const float* Vo = a.Vo + (size_t)b * NC * D;
        for (int i = tid; i < NC * (D / 4); i += XA_T) {
            const int r = i / (D / 4), c4 = i - r * (D / 4);
            *reinterpret_cast<float4*>(Vs + r * LDA + 4 * c4) = *reinterpret_cast<const float4*>(Vo + (size_t)r * D + 4 * c4);
        }
        const float* AbT = a.AbT + (size_t)b * D * NC;
        for (int i = tid; i < D * (NC / 4); i += XA_T) {
            const int r = i / (NC / 4), c4 = i - r * (NC / 4);
            *reinterpret_cast<float4*>(As + r * LDV + 4 * c4) = *reinterpret_cast<const float4*>(AbT + (size_t)r * NC + 4 * c4);
        }
    }
    __syncthreads();
    const int ntile = (T + 15) / 16, per = (ntile + a.NS - 1) / a.NS;
    const int t0 = hs * per, t1 = (t0 + per < ntile) ? t0 + per : ntile;
    const uint32_t thr = drop_thresh(a.p);
    const float dsc = a.p > 0.f ? 1.0f / (1.0f - a.p) : 1.f;
    const int slot0 = (4 * g) % KP;
#pragma unroll 1
    for (int t = t0 + wv; t < t1; t += XA_T / 64) {
        const int tok = t * 16 + li;
        const bool live = tok < T;
        const size_t trow = (size_t)b * T + (live ? tok : 0);
        const size_t row = trow * D;
        float4 gv[NM];
#pragma unroll
        for (int c = 0; c < NM; ++c) gv[c] = live ? *reinterpret_cast<const float4*>(a.gd + row + 16 * c + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        // the saved probabilities of this lane's columns
        float pr[NT][4];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            const int head = (16 * tt + 4 * g) / KP;
            const long long prow = (((long long)b * a.h + head) * T + (live ? tok : 0)) * K;
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[tt][r] = (live && slot0 + r < K) ? a.P[prow + slot0 + r] : 0.f;
        }
        // ---- d Pd^T[col][tok] = Vo_b gd^T
        f32x4 dp[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) dp[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NM; ++c) {
            float4 av[NT];
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) av[tt] = *reinterpret_cast<const float4*>(Vs + (16 * tt + li) * LDA + 16 * c + 4 * g);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) dp[tt] = MFMA16(av[tt].x, gv[c].x, dp[tt]);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) dp[tt] = MFMA16(av[tt].y, gv[c].y, dp[tt]);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) dp[tt] = MFMA16(av[tt].z, gv[c].z, dp[tt]);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) dp[tt] = MFMA16(av[tt].w, gv[c].w, dp[tt]);
            if ((c & 1) == 1) __builtin_amdgcn_sched_barrier(0);
        }
        // ---- dropout backward, soft-max backward per head
        f32x4 ds[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            const int head = (16 * tt + 4 * g) / KP;
            const long long prow = (((long long)b * a.h + head) * T + (live ? tok : 0)) * K;
            float keep[4], dpr[4];
            float dot = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                keep[r] = 1.f;
                if (a.p > 0.f && slot0 + r < K) {
                    const uint64_t idx = (uint64_t)prow + slot0 + r;
                    keep[r] = rng_keep(rng_bits4(a.seed, a.site_p, idx >> 2), (int)(idx & 3), thr) ? dsc : 0.f;
                }
                dpr[r] = dp[tt][r] * keep[r];
                dot += pr[tt][r] * dpr[r];
            }
            dot = xa_head_reduce<KP>(dot, false);
            float4 pdv, dsv;
            float* pdp = &pdv.x;
            float* dsp = &dsv.x;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pdp[r] = pr[tt][r] * keep[r];
                dsp[r] = slot0 + r < K ? pr[tt][r] * (dpr[r] - dot) : 0.f;      // padding: +0, not 0 * (negative) = -0
                ds[tt][r] = dsp[r];
            }
            if (live) {
                *reinterpret_cast<float4*>(a.Pd + trow * NC + 16 * tt + 4 * g) = pdv;
                *reinterpret_cast<float4*>(a.dS + trow * NC + 16 * tt + 4 * g) = dsv;
            }
        }
        // ---- d x^T[e][tok] = A_b dS^T
        f32x4 o[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) o[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
            for (int m = 0; m < NM; m += 4) {
                float4 v4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v4[u] = *reinterpret_cast<const float4*>(As + (16 * (m + u) + li) * LDV + 16 * tt + 4 * g);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    o[m + u] = MFMA16(v4[u].x, ds[tt][0], o[m + u]);
                    o[m + u] = MFMA16(v4[u].y, ds[tt][1], o[m + u]);
                    o[m + u] = MFMA16(v4[u].z, ds[tt][2], o[m + u]);
                    o[m + u] = MFMA16(v4[u].w, ds[tt][3], o[m + u]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (live) {
#pragma unroll
            for (int m = 0; m < NM; ++m) *reinterpret_cast<float4*>(a.y + row + 16 * m + 4 * g) = make_float4(o[m][0], o[m][1], o[m][2], o[m][3]);
        }
    }
}

// ------------------------------------------------------------------------------------------- launchers
// The shape rule of the folded form, in one place (host only): xattn_supported, the fold and xattn_launch all read it, so what it
// reports is what runs.  KP: slots per head after padding; NC = h * KP columns (one, two or four 16-column tiles); NM = d / 16 row
// tiles (64-, 128-, 192- and 256-wide kernels are built); lds: dynamic LDS bytes of the forward / backward kernel (both operands,
// row strides padded by 4).
bool xattn_plan(int K, int d, int h, XaPlan* out) {
    XaPlan p;
    if (K >= 1 && K <= 16 && d >= 64 && d <= 256 && d % 64 == 0 && h >= 1 && d % h == 0 && (d / h) % 4 == 0) {
        p.KP = (K <= 8 && h > 1) ? 8 : 16;
        p.NC = h * p.KP;
        p.NM = d / 16;
        p.lds = (size_t)(p.NC * (d + 4) + d * (p.NC + 4)) * sizeof(float);
        p.supported = p.NC == 16 || p.NC == 32 || p.NC == 64;
    }
    if (!p.supported) p = XaPlan();
    if (out) *out = p;
    return p.supported;
}
bool xattn_supported(int K, int d, int h) { return xattn_plan(K, d, h, nullptr); }
int xattn_kp(int K, int h) { return (K <= 8 && h > 1) ? 8 : 16; }

int xattn_fold_fwd_launch(const XaFoldHost& f, hipStream_t st) {
    OCRL_REQUIRE(xattn_supported(f.K, f.d, f.h) && f.nblk >= 1 && f.nblk <= 8, "xattn_fold: unsupported shape");
    XaFoldArgs a;
    XaPlan pl;
    xattn_plan(f.K, f.d, f.h, &pl);
    a.mem = f.mem; a.B = f.B; a.K = f.K; a.d = f.d; a.h = f.h; a.KP = pl.KP; a.NC = pl.NC;
    for (int i = 0; i < f.nblk; ++i) {
        a.Wq[i] = f.Wq[i]; a.Wk[i] = f.Wk[i]; a.Wv[i] = f.Wv[i]; a.Wo[i] = f.Wo[i];
        a.ck[i] = f.ck[i]; a.cv[i] = f.cv[i]; a.Ab[i] = f.Ab[i]; a.AbT[i] = f.AbT[i]; a.Vo[i] = f.Vo[i]; a.VoT[i] = f.VoT[i];
    }
    hipLaunchKernelGGL(xattn_fold_fwd_kernel, dim3(f.B, f.nblk), dim3(256), 3 * f.K * f.d * sizeof(float), st, a);
    OCRL_CHECK_LAUNCH("xattn_fold_fwd");
    return 0;
}

static int xa_splits(int B, int T) {
    int ncu = 256, dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
    const int ntile = (T + 15) / 16;
    int ns = B <= 2 * ncu ? (2 * ncu) / B : 1;          // two resident workgroups per CU, one round
    if (ns > ntile / 4) ns = ntile / 4;                  // at least one 16-token tile per wave
    return ns < 1 ? 1 : ns;
}

template <int NM, int NT, int KP>
static int xattn_launch_t(XaArgs& a, size_t smem, int backward, hipStream_t st) {
    static bool attr[2] = {false, false};
    if (!attr[backward]) {
        if (backward) OCRL_HIP(hipFuncSetAttribute((const void*)xattn_bwd_kernel<NM, NT, KP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        else OCRL_HIP(hipFuncSetAttribute((const void*)xattn_fwd_kernel<NM, NT, KP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        attr[backward] = true;
    }
    a.NS = xa_splits(a.B, a.T);
    if (backward) hipLaunchKernelGGL((xattn_bwd_kernel<NM, NT, KP>), dim3(a.B * a.NS), dim3(XA_T), smem, st, a);
    else hipLaunchKernelGGL((xattn_fwd_kernel<NM, NT, KP>), dim3(a.B * a.NS), dim3(XA_T), smem, st, a);
    OCRL_CHECK_LAUNCH("xattn");
    return 0;
}
template <int NM>
static int xattn_launch_m(XaArgs& a, const XaPlan& pl, int backward, hipStream_t st) {
    const int KP = pl.KP, NC = pl.NC;
    if (KP == 8 && NC == 16) return xattn_launch_t<NM, 1, 8>(a, pl.lds, backward, st);
    if (KP == 8 && NC == 32) return xattn_launch_t<NM, 2, 8>(a, pl.lds, backward, st);
    if (KP == 8 && NC == 64) return xattn_launch_t<NM, 4, 8>(a, pl.lds, backward, st);
    if (KP == 16 && NC == 16) return xattn_launch_t<NM, 1, 16>(a, pl.lds, backward, st);
    if (KP == 16 && NC == 32) return xattn_launch_t<NM, 2, 16>(a, pl.lds, backward, st);
    if (KP == 16 && NC == 64) return xattn_launch_t<NM, 4, 16>(a, pl.lds, backward, st);
    OCRL_REQUIRE(false, "xattn: unsupported column count %d", NC);
}
int xattn_launch(const XaHost& h, int backward, hipStream_t st) {
    XaPlan pl;
    OCRL_REQUIRE(xattn_plan(h.K, h.d, h.h, &pl), "xattn: unsupported shape (K %d, d %d, heads %d)", h.K, h.d, h.h);
    OCRL_REQUIRE(h.B >= 1 && h.T >= 1, "xattn: empty batch or sequence");
    OCRL_REQUIRE(h.x && h.y && h.P && h.Ab && h.AbT && h.Vo && h.VoT, "xattn: missing buffers");
    OCRL_REQUIRE((long long)h.B * h.T * h.d < (1ll << 40), "xattn: too large");
    XaArgs a;
    a.x = h.x; a.resid = h.resid; a.y = h.y; a.P = h.P; a.Ab = h.Ab; a.AbT = h.AbT; a.Vo = h.Vo; a.VoT = h.VoT; a.gd = h.gd; a.Pd = h.Pd; a.dS = h.dS;
    a.B = h.B; a.T = h.T; a.K = h.K; a.d = h.d; a.h = h.h; a.p = h.p; a.seed = h.seed; a.site_p = h.site_p; a.site_o = h.site_o; a.NS = 1;
    if (backward) OCRL_REQUIRE(h.gd && h.Pd && h.dS, "xattn backward: missing buffers");
    else OCRL_REQUIRE(h.resid, "xattn forward: missing residual");
    switch (pl.NM) {
        case 4: return xattn_launch_m<4>(a, pl, backward, st);
        case 8: return xattn_launch_m<8>(a, pl, backward, st);
        case 12: return xattn_launch_m<12>(a, pl, backward, st);
        case 16: return xattn_launch_m<16>(a, pl, backward, st);
        default: OCRL_REQUIRE(false, "xattn: d_model %d not built (64, 128, 192, 256)", h.d);
    }
}

// Backward of the fold: from the per-token operands of xattn_launch(.., 1) (Pd, dS) to d ck, d cv and the two projection weight
// gradients.  Two per-image sums over the tokens, four products batched over (image, head), two sums over the images in a fixed order.
int xattn_fold_bwd_launch(const XaFoldBwdHost& f, hipStream_t st) {
    XaPlan pl;
    OCRL_REQUIRE(xattn_plan(f.K, f.d, f.h, &pl), "xattn_fold_bwd: unsupported shape (K %d, d %d, heads %d)", f.K, f.d, f.h);
    OCRL_REQUIRE(f.B >= 1 && f.T >= 1, "xattn_fold_bwd: empty batch or sequence");
    OCRL_REQUIRE(f.Pd && f.dS && f.gd && f.x && f.Wq && f.Wo && f.ck && f.cv && f.dVo && f.dAb && f.dck && f.dcv && f.pq && f.po && f.dWq && f.dWo && f.ws,
                 "xattn_fold_bwd: missing buffers");
    const int B = f.B, T = f.T, K = f.K, d = f.d, NH = f.h, KP = pl.KP, NC = pl.NC, dh = d / NH;
    const float scale = 1.0f / sqrtf((float)dh);
    GemmArgs ga;      // per-image sums over the tokens: d Vo_b = Pd^T d out,  d A_b = dS^T LN(x)      [NC, d] each
    ga.M = NC; ga.N = d; ga.K = T; ga.lda = NC; ga.ldb = d; ga.ldc = d; ga.akc = 0; ga.bkc = 0; ga.batch = B;
    ga.sA = (long long)T * NC; ga.sB = (long long)T * d; ga.sC = (long long)NC * d;
    ga.A = f.Pd; ga.B = f.gd; ga.C = f.dVo;
    RC(gemm_launch(ga, st));
    ga.A = f.dS; ga.B = f.x; ga.C = f.dAb;
    RC(gemm_launch(ga, st));
    // back through the fold, batched over (image, head):
    GemmArgs gb;      // d ck[k, h dh + j] = scale sum_e dA_b[(h,k), e] Wq[h dh + j, e]
    gb.M = K; gb.N = dh; gb.K = d; gb.akc = 1; gb.bkc = 1; gb.lda = d; gb.ldb = d; gb.ldc = d; gb.batch = B * NH; gb.batch_inner = NH; gb.alpha = scale;
    gb.A = f.dAb; gb.sA = (long long)NC * d; gb.sAi = (long long)KP * d;
    gb.B = f.Wq; gb.sB = 0; gb.sBi = (long long)dh * d;
    gb.C = f.dck; gb.sC = (long long)K * d; gb.sCi = dh;
    RC(gemm_launch(gb, st));
    GemmArgs gc;      // d cv[k, h dh + j] = sum_o dVo_b[(h,k), o] Wo[o, h dh + j]
    gc.M = K; gc.N = dh; gc.K = d; gc.akc = 1; gc.bkc = 0; gc.lda = d; gc.ldb = d; gc.ldc = d; gc.batch = B * NH; gc.batch_inner = NH;
    gc.A = f.dVo; gc.sA = (long long)NC * d; gc.sAi = (long long)KP * d;
    gc.B = f.Wo; gc.sB = 0; gc.sBi = dh;
    gc.C = f.dcv; gc.sC = (long long)K * d; gc.sCi = dh;
    RC(gemm_launch(gc, st));
    GemmArgs gq;      // this image's d Wq[h dh + j, e] = scale sum_k ck[k, h dh + j] dA_b[(h,k), e]
    gq.M = dh; gq.N = d; gq.K = K; gq.akc = 0; gq.bkc = 0; gq.lda = d; gq.ldb = d; gq.ldc = d; gq.batch = B * NH; gq.batch_inner = NH; gq.alpha = scale;
    gq.A = f.ck; gq.sA = (long long)K * d; gq.sAi = dh;
    gq.B = f.dAb; gq.sB = (long long)NC * d; gq.sBi = (long long)KP * d;
    gq.C = f.pq; gq.sC = (long long)d * d; gq.sCi = (long long)dh * d;
    RC(gemm_launch(gq, st));
    GemmArgs go;      // this image's d Wo[o, h dh + j] = sum_k dVo_b[(h,k), o] cv[k, h dh + j]
    go.M = d; go.N = dh; go.K = K; go.akc = 0; go.bkc = 0; go.lda = d; go.ldb = d; go.ldc = d; go.batch = B * NH; go.batch_inner = NH;
    go.A = f.dVo; go.sA = (long long)NC * d; go.sAi = (long long)KP * d;
    go.B = f.cv; go.sB = (long long)K * d; go.sBi = dh;
    go.C = f.po; go.sC = (long long)d * d; go.sCi = dh;
    RC(gemm_launch(go, st));
    RC(colsum_launch(f.pq, (long long)d * d, f.dWq, B, d * d, 0, 1.f, f.ws, f.ws_floats, st));
    RC(colsum_launch(f.po, (long long)d * d, f.dWo, B, d * d, 0, 1.f, f.ws, f.ws_floats, st));
    return 0;
}

// =========================================================================================== the plain form (OCRL_XATTN=0, generate())
// ------------------------------------------------------------------ cross attention to K (<= 16) slots
// Q [B,T,d] (projected, unscaled), Km/Vm [B,K,d], heads h, dh = d/h (<= 64).  One thread per (b,head,q).
// P [B,h,T,K] = softmax (pre-dropout) is saved for the backward.
// MAXK (8 or 16) is the compile-time slot capacity: per-slot values live in registers.
#define CA_MAXDH 64
template <int CA_MAXK>
__global__ __launch_bounds__(256) void cross_attn_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ Km,
                                                             const float* __restrict__ Vm, float* __restrict__ O,
                                                             float* __restrict__ P, int T, int K, int d, int h, float p,
                                                             unsigned long long seed, unsigned site) {
    extern __shared__ float sm[];   // Ks [K][dh], Vs [K][dh]
    const int dh = d / h;
    const int nqb = (T + 255) / 256;
    int bid = blockIdx.x;
    const int qb = bid % nqb; bid /= nqb;
    const int hd = bid % h;
    const long long b = bid / h;
    float* Ks = sm;
    float* Vs = sm + K * dh;
    for (int i = threadIdx.x; i < K * dh; i += 256) {
        const int k = i / dh, c = i % dh;
        Ks[i] = Km[(b * K + k) * d + hd * dh + c];
        Vs[i] = Vm[(b * K + k) * d + hd * dh + c];
    }
    __syncthreads();
    const int q = qb * 256 + threadIdx.x;
    if (q >= T) return;
    const float scale = rsqrtf((float)dh);
    float qv[CA_MAXDH];
    const float* qp = Q + (b * T + q) * d + hd * dh;
#pragma unroll
    for (int c = 0; c < CA_MAXDH; c += 4)
        if (c < dh) {
            const float4 v = *reinterpret_cast<const float4*>(qp + c);
            qv[c] = v.x * scale; qv[c + 1] = v.y * scale; qv[c + 2] = v.z * scale; qv[c + 3] = v.w * scale;
        }
    float s[CA_MAXK];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < CA_MAXK; ++k)
        if (k < K) {
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < CA_MAXDH; c += 4)              // broadcast ds_read_b128: a quarter of the LDS instructions
                if (c < dh) {
                    const float4 k4 = *reinterpret_cast<const float4*>(Ks + k * dh + c);
                    a += (qv[c] * k4.x + qv[c + 1] * k4.y) + (qv[c + 2] * k4.z + qv[c + 3] * k4.w);
                }
            s[k] = a;
            mx = fmaxf(mx, a);
        }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CA_MAXK; ++k)
        if (k < K) { s[k] = __expf(s[k] - mx); sum += s[k]; }
    const float inv = 1.0f / sum;
    const uint32_t thr = drop_thresh(p);
    const float sc = p > 0.f ? 1.0f / (1.0f - p) : 1.f;
    const long long prow = ((b * h + hd) * T + q) * K;
    float o[CA_MAXDH];
#pragma unroll
    for (int c = 0; c < CA_MAXDH; ++c) o[c] = 0.f;
#pragma unroll
    for (int k = 0; k < CA_MAXK; ++k)
        if (k < K) {
            const float pr = s[k] * inv;
            P[prow + k] = pr;
            float pd = pr;
            if (p > 0.f) {
                const uint64_t idx = (uint64_t)prow + k;
                pd = rng_keep(rng_bits4(seed, site, idx >> 2), (int)(idx & 3), thr) ? pr * sc : 0.f;
            }
#pragma unroll
            for (int c = 0; c < CA_MAXDH; c += 4)
                if (c < dh) {
                    const float4 v4 = *reinterpret_cast<const float4*>(Vs + k * dh + c);
                    o[c] += pd * v4.x; o[c + 1] += pd * v4.y; o[c + 2] += pd * v4.z; o[c + 3] += pd * v4.w;
                }
        }
    float* op = O + (b * T + q) * d + hd * dh;
#pragma unroll
    for (int c = 0; c < CA_MAXDH; c += 4)
        if (c < dh) *reinterpret_cast<float4*>(op + c) = make_float4(o[c], o[c + 1], o[c + 2], o[c + 3]);
}

// backward: dQ [B,T,d] written; the slot-side gradients leave each workgroup as one partial [2][K*dh] (dV, dK) in `part`,
// summed over the query blocks in a fixed order by cross_attn_reduce_kernel (no float atomics: bitwise reproducible).  The
// per-query outer products are reduced over the 64 queries of a wave through a wave-private LDS staging tile (queries x (K + dh)),
// then over the four waves through LDS.
template <int CA_MAXK>
__global__ __launch_bounds__(256) void cross_attn_bwd_kernel(const float* __restrict__ dO, const float* __restrict__ Q,
                                                             const float* __restrict__ Km, const float* __restrict__ Vm,
                                                             const float* __restrict__ P, float* __restrict__ dQ,
                                                             float* __restrict__ part, int T, int K, int d,
                                                             int h, float p, unsigned long long seed, unsigned site) {
    extern __shared__ float sm[];   // Ks [K][dh], Vs [K][dh], stage [4][64][CA_SW]
    constexpr int CA_SW = CA_MAXK + CA_MAXDH + 1;
    float* mypart = part + (size_t)blockIdx.x * 2 * K * (d / h);
    const int dh = d / h;
    const int nqb = (T + 255) / 256;
    int bid = blockIdx.x;
    const int qb = bid % nqb; bid /= nqb;
    const int hd = bid % h;
    const long long b = bid / h;
    float* Ks = sm;
    float* Vs = sm + K * dh;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* stg = sm + 2 * K * dh + wv * 64 * CA_SW;      // this wave's staging tile
    for (int i = threadIdx.x; i < K * dh; i += 256) {
        const int k = i / dh, c = i % dh;
        Ks[i] = Km[(b * K + k) * d + hd * dh + c];
        Vs[i] = Vm[(b * K + k) * d + hd * dh + c];
    }
    __syncthreads();
    const int q = qb * 256 + threadIdx.x;
    const bool act = q < T;
    const float scale = rsqrtf((float)dh);
    // The wave's 64 query rows of dO (and later of Q) are fetched as one coalesced tile (consecutive lanes = consecutive 16 bytes of a
    // row) straight into the staging tile the matrix products read; a thread then takes its own row from LDS.  Thread-per-row global
    // loads (64 different cache lines per instruction) were what bound this kernel.
    const int q0 = qb * 256 + wv * 64, dh4 = dh >> 2;
    // All dh/4 loads of a lane are issued before the first LDS store (a rolled load -> store loop paid one memory round trip per
    // 16 bytes: 2 x 12 round trips per workgroup, with two workgroups per CU to hide them).  (row, chunk) advance without divisions.
    const int r_step = 64 / dh4, c_step = 64 - r_step * dh4;
    auto load_tile = [&](const float* src, float mul) {
        float4 tmp[CA_MAXDH / 4];
        int r = lane / dh4, c4 = lane - r * dh4;
#pragma unroll
        for (int i = 0; i < CA_MAXDH / 4; ++i) {
            tmp[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < dh4 && q0 + r < T) tmp[i] = *reinterpret_cast<const float4*>(src + (b * T + q0 + r) * d + hd * dh + 4 * c4);
            r += r_step; c4 += c_step;
            if (c4 >= dh4) { c4 -= dh4; ++r; }
        }
        r = lane / dh4; c4 = lane - r * dh4;
#pragma unroll
        for (int i = 0; i < CA_MAXDH / 4; ++i) {
            if (i < dh4) {
                float* dst = stg + r * CA_SW + CA_MAXK + 4 * c4;
                dst[0] = tmp[i].x * mul; dst[1] = tmp[i].y * mul; dst[2] = tmp[i].z * mul; dst[3] = tmp[i].w * mul;
            }
            r += r_step; c4 += c_step;
            if (c4 >= dh4) { c4 -= dh4; ++r; }
        }
        __builtin_amdgcn_wave_barrier();
    };
    load_tile(dO, 1.f);
    float go[CA_MAXDH];
    float pr[CA_MAXK], dp[CA_MAXK], keepv[CA_MAXK];
#pragma unroll
    for (int c = 0; c < CA_MAXDH; ++c) go[c] = c < dh ? stg[lane * CA_SW + CA_MAXK + c] : 0.f;
#pragma unroll
    for (int k = 0; k < CA_MAXK; ++k) { pr[k] = 0.f; dp[k] = 0.f; keepv[k] = 0.f; }
    float delta = 0.f;
    if (act) {
        const uint32_t thr = drop_thresh(p);
        const float sc = p > 0.f ? 1.0f / (1.0f - p) : 1.f;
        const long long prow = ((b * h + hd) * T + q) * K;
#pragma unroll
        for (int k = 0; k < CA_MAXK; ++k)
            if (k < K) {
                pr[k] = P[prow + k];
                float keep = 1.f;
                if (p > 0.f) {
                    const uint64_t idx = (uint64_t)prow + k;
                    keep = rng_keep(rng_bits4(seed, site, idx >> 2), (int)(idx & 3), thr) ? sc : 0.f;
                }
                keepv[k] = keep;
                float a = 0.f;
#pragma unroll
                for (int c = 0; c < CA_MAXDH; c += 4)          // one broadcast ds_read_b128 per four channels (the per-channel form waited on 576 LDS reads per query)
                    if (c < dh) {
                        const float4 v4 = *reinterpret_cast<const float4*>(Vs + k * dh + c);
                        a += (go[c] * v4.x + go[c + 1] * v4.y) + (go[c + 2] * v4.z + go[c + 3] * v4.w);
                    }
                dp[k] = a * keep;
                delta += pr[k] * dp[k];
            }
    }
    // ---- dV[k][c] += sum_q pd[q][k] * go[q][c]      (go is already in the staging tile)
#pragma unroll
    for (int k = 0; k < CA_MAXK; ++k) stg[lane * CA_SW + k] = pr[k] * keepv[k];
    __syncthreads();
    // [slots x 64 queries] . [64 queries x dh] on the matrix cores: slots on the 16 MFMA rows, 16-channel tiles on the columns, four
    // queries per v_mfma_f32_16x16x4_f32 (lane (li, g): A = stage[query 4s+g][slot li], B = stage[query 4s+g][channel 16m+li])
    const int li = lane & 15, g4 = lane >> 4, nmt = (dh + 15) >> 4;
    f32x4 acc[CA_MAXDH / 16];
#pragma unroll
    for (int m = 0; m < CA_MAXDH / 16; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s16 = 0; s16 < 16; ++s16) {
        const float* rowp = stg + (4 * s16 + g4) * CA_SW;
        const float a = li < CA_MAXK ? rowp[li] : 0.f;
#pragma unroll
        for (int m = 0; m < CA_MAXDH / 16; ++m)
            if (m < nmt) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, rowp[CA_MAXK + 16 * m + li], acc[m], 0, 0, 0);
    }
    __syncthreads();                                       // every wave is done reading its staging tile
#pragma unroll
    for (int m = 0; m < CA_MAXDH / 16; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 4 * g4 + r, c = 16 * m + li;
            if (m < nmt && k < K && c < dh) stg[k * dh + c] = acc[m][r];
        }
    __syncthreads();
    for (int o = threadIdx.x; o < K * dh; o += 256) {
        const float* r = sm + 2 * K * dh + o;
        mypart[o] = (r[0] + r[64 * CA_SW]) + (r[2 * 64 * CA_SW] + r[3 * 64 * CA_SW]);
    }
    __syncthreads();
    // ---- dS, dQ, and dK[k][c] += sum_q ds[q][k] * q'[q][c]
    float dq[CA_MAXDH];
#pragma unroll
    for (int c = 0; c < CA_MAXDH; ++c) dq[c] = 0.f;
#pragma unroll
    for (int k = 0; k < CA_MAXK; ++k) {
        const float ds = (k < K) ? pr[k] * (dp[k] - delta) : 0.f;
        stg[lane * CA_SW + k] = ds;
        if (k < K) {
#pragma unroll
            for (int c = 0; c < CA_MAXDH; c += 4)
                if (c < dh) {
                    const float4 k4 = *reinterpret_cast<const float4*>(Ks + k * dh + c);
                    dq[c] += ds * k4.x; dq[c + 1] += ds * k4.y; dq[c + 2] += ds * k4.z; dq[c + 3] += ds * k4.w;
                }
        }
    }
    load_tile(Q, scale);                                   // q' = scale * q of the wave's rows, straight into the staging tile
    __syncthreads();
#pragma unroll
    for (int m = 0; m < CA_MAXDH / 16; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s16 = 0; s16 < 16; ++s16) {
        const float* rowp = stg + (4 * s16 + g4) * CA_SW;
        const float a = li < CA_MAXK ? rowp[li] : 0.f;
#pragma unroll
        for (int m = 0; m < CA_MAXDH / 16; ++m)
            if (m < nmt) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, rowp[CA_MAXK + 16 * m + li], acc[m], 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < CA_MAXDH / 16; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 4 * g4 + r, c = 16 * m + li;
            if (m < nmt && k < K && c < dh) stg[k * dh + c] = acc[m][r];
        }
    __syncthreads();
    for (int o = threadIdx.x; o < K * dh; o += 256) {
        const float* r = sm + 2 * K * dh + o;
        mypart[K * dh + o] = (r[0] + r[64 * CA_SW]) + (r[2 * 64 * CA_SW] + r[3 * 64 * CA_SW]);
    }
    __syncthreads();                                       // the partials are out: the staging tile carries dQ to a coalesced store
#pragma unroll
    for (int c = 0; c < CA_MAXDH; ++c)
        if (c < dh) stg[lane * CA_SW + CA_MAXK + c] = dq[c] * scale;
    __builtin_amdgcn_wave_barrier();
    for (int idx = lane; idx < 64 * dh4; idx += 64) {
        const int r = idx / dh4, c4 = idx - r * dh4;
        if (q0 + r < T) {
            const float* src = stg + r * CA_SW + CA_MAXK + 4 * c4;
            *reinterpret_cast<float4*>(dQ + (b * T + q0 + r) * d + hd * dh + 4 * c4) = make_float4(src[0], src[1], src[2], src[3]);
        }
    }
}

int cross_attn_fwd_launch(const float* Q, const float* Km, const float* Vm, float* O, float* P, int B, int T, int K, int d, int h, float p,
                          unsigned long long seed, unsigned site, hipStream_t st) {
    OCRL_REQUIRE(K >= 1 && K <= 16 && d % h == 0 && (d / h) <= CA_MAXDH && (d / h) % 4 == 0, "cross_attn: unsupported K=%d d=%d h=%d", K, d, h);
    const int grid = B * h * cdiv(T, 256);
    if (K <= 8) hipLaunchKernelGGL(cross_attn_fwd_kernel<8>, dim3(grid), dim3(256), 2 * K * (d / h) * 4, st, Q, Km, Vm, O, P, T, K, d, h, p, seed, site);
    else hipLaunchKernelGGL(cross_attn_fwd_kernel<16>, dim3(grid), dim3(256), 2 * K * (d / h) * 4, st, Q, Km, Vm, O, P, T, K, d, h, p, seed, site);
    OCRL_CHECK_LAUNCH("cross_attn_fwd");
    return 0;
}
// dKm / dVm [B,K,d] = sum over the query blocks of the per-workgroup partials, in block order
__global__ void cross_attn_reduce_kernel(const float* __restrict__ part, float* __restrict__ dKm, float* __restrict__ dVm, long long n, int nqb,
                                         int K, int d, int h) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // over [B][K][d]
    if (i >= n) return;
    const int dh = d / h;
    const int col = i % d, k = (i / d) % K;
    const long long b = i / ((long long)d * K);
    const int hd = col / dh, c = col - hd * dh;
    const float* src = part + ((b * h + hd) * nqb) * 2 * K * dh + k * dh + c;
    float av = 0.f, ak = 0.f;
    for (int q = 0; q < nqb; ++q) { av += src[(size_t)q * 2 * K * dh]; ak += src[(size_t)q * 2 * K * dh + K * dh]; }
    dVm[i] = av;
    dKm[i] = ak;
}

size_t cross_attn_bwd_ws_floats(int B, int T, int K, int d, int h) { return (size_t)B * h * cdiv(T, 256) * 2 * K * (d / h); }

template <int MAXK>
static int cross_attn_bwd_launch_k(const float* dO, const float* Q, const float* Km, const float* Vm, const float* P, float* dQ, float* dKm, float* dVm,
                                   int B, int T, int K, int d, int h, float p, unsigned long long seed, unsigned site, float* part, hipStream_t st) {
    constexpr int SW = MAXK + CA_MAXDH + 1;
    const int grid = B * h * cdiv(T, 256);
    static bool attr_set = false;
    if (!attr_set) {
        OCRL_HIP(hipFuncSetAttribute((const void*)cross_attn_bwd_kernel<MAXK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (2 * MAXK * CA_MAXDH + 4 * 64 * SW) * 4));
        attr_set = true;
    }
    hipLaunchKernelGGL(cross_attn_bwd_kernel<MAXK>, dim3(grid), dim3(256), (2 * K * (d / h) + 4 * 64 * SW) * 4, st, dO, Q, Km, Vm, P, dQ, part, T, K, d, h, p, seed, site);
    OCRL_CHECK_LAUNCH("cross_attn_bwd");
    const long long n = (long long)B * K * d;
    hipLaunchKernelGGL(cross_attn_reduce_kernel, GRID1D(n), 0, st, part, dKm, dVm, n, cdiv(T, 256), K, d, h);
    OCRL_CHECK_LAUNCH("cross_attn_reduce");
    return 0;
}
// dKm / dVm are written (not accumulated); part: cross_attn_bwd_ws_floats() floats of scratch
int cross_attn_bwd_launch(const float* dO, const float* Q, const float* Km, const float* Vm, const float* P, float* dQ, float* dKm, float* dVm,
                          int B, int T, int K, int d, int h, float p, unsigned long long seed, unsigned site, float* part, size_t part_floats,
                          hipStream_t st) {
    OCRL_REQUIRE(K >= 1 && K <= 16 && d % h == 0 && (d / h) <= CA_MAXDH && (d / h) % 4 == 0, "cross_attn: unsupported K=%d d=%d h=%d", K, d, h);
    OCRL_REQUIRE(part && part_floats >= cross_attn_bwd_ws_floats(B, T, K, d, h), "cross_attn_bwd: scratch too small");
    if (K <= 8) return cross_attn_bwd_launch_k<8>(dO, Q, Km, Vm, P, dQ, dKm, dVm, B, T, K, d, h, p, seed, site, part, st);
    return cross_attn_bwd_launch_k<16>(dO, Q, Km, Vm, P, dQ, dKm, dVm, B, T, K, d, h, p, seed, site, part, st);
}
