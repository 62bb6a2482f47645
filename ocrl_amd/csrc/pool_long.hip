// Transformer pooling over long token sequences (a CNN feature map: S = H*W + 1 tokens, include/ocrl_hip.h ocrl_pool_transformer_long_*).
// The output is the CLS row of the last post-norm layer, so that layer needs the query of row 0 only; with the projections folded,
//   u_h = hd^-1/2 W_k,h^T q_h          score_hj = x_j . u_h  (+ a constant that drops out of the soft-max)
//   o_h = W_v,h (sum_j p'_hj x_j) + b_v,h sum_j p'_hj      (p' = p after dropout)
// one pass over the token rows X [B][S][d] gives the attention of the CLS row (pool_cls_*).  Layers before the last run on every row:
// non-causal flash attention with the log-sum-exp saved (pool_flash_*), no S^2 buffer.
//   pool_cols          pack / unpack a ragged [rows, n] matrix to a stride-4 copy (input Linear with any rep_dim)
//   pool_cls_drop      y = resid + dropout(x) on the B CLS rows with the element index of the full [B, S, N] tensor
//   pool_cls_u         U [B][h][d] from q and W_k
//   pool_cls_fwd       partial (max, sum, sum p', sum p' x) per (image, chunk of positions, head): online soft-max over 64-row tiles
//   pool_cls_merge     merge the chunks; z = sum p' x, a = sum p', lse; o = W_v z + b_v a
//   pool_cls_bprep     G = W_v,h^T dO_h, gb = b_v,h . dO_h, D = sum p' dp'
//   pool_cls_bwd       dX = sum_h ds_hj u_h + p'_hj G_h, partial sum_j ds_hj x_j per chunk
//   pool_cls_wsum      w = sum over chunks, dq = hd^-1/2 W_k,h w_h
//   pool_cls_wgrad     d in_proj_{weight,bias} from dq / x0, q / w, dO / z, a (the k bias gradient is zero: soft-max is shift invariant)
//   pool_flash_fwd     thread = query, 32-key tiles in LDS, online soft-max; O and lse
//   pool_flash_bwd_q   thread = query: dq;   pool_flash_bwd_kv  thread = key: dk, dv
// Attention dropout uses the site and element index of the short path: ((b*h + head)*S + query)*S + key (64-bit).
#include "common.h"
#include "kernels.h"

#define PL_T 256
#define PL_TP 64          // token rows per tile of the CLS kernels
#define PL_NACC 4         // float4 accumulators per thread: h * d / 4 <= 1024

__device__ __forceinline__ bool pl_keep(unsigned long long seed, unsigned site, unsigned long long idx, uint32_t thr) {
    return rng_keep(rng_bits4(seed, site, idx >> 2), (int)(idx & 3), thr);
}

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ void fma4(float4& acc, float s, float4 v) { acc.x += s * v.x; acc.y += s * v.y; acc.z += s * v.z; acc.w += s * v.w; }

// dst[r][c] = c < ncopy ? src[r][c] : 0  for c < ncols
__global__ void pool_cols_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd, long long rows, int ncols, int ncopy) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ncols) return;
    const long long r = i / ncols;
    const int c = (int)(i - r * ncols);
    dst[r * ldd + c] = c < ncopy ? src[r * lds + c] : 0.f;
}
int pool_cols_launch(const float* src, int lds, float* dst, int ldd, long long rows, int ncols, int ncopy, hipStream_t st) {
    const long long n = rows * ncols;
    if (n == 0) return 0;
    hipLaunchKernelGGL(pool_cols_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, src, lds, dst, ldd, rows, ncols, ncopy);
    OCRL_CHECK_LAUNCH("pool_cols");
    return 0;
}

// out[b][c] = (resid ? resid[b*ldr + c] : 0) + dropout(x[b][c]);  the keep decision of element (b*S + 0, c) of a [B*S, N] tensor
__global__ void pool_cls_drop_kernel(const float* x, const float* __restrict__ resid, int ldr, float* out, int B, int N, int S,
                                     float p, unsigned long long seed, unsigned site) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * N) return;
    const int b = (int)(i / N), c = (int)(i - (long long)b * N);
    float v = x[i];
    if (p > 0.f) v = pl_keep(seed, site, (unsigned long long)b * S * N + c, drop_thresh(p)) ? v * (1.f / (1.f - p)) : 0.f;
    if (resid) v += resid[(long long)b * ldr + c];
    out[i] = v;
}
int pool_cls_drop_launch(const float* x, const float* resid, int ldr, float* out, int B, int N, int S, float p, unsigned long long seed, unsigned site,
                         hipStream_t st) {
    const long long n = (long long)B * N;
    hipLaunchKernelGGL(pool_cls_drop_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, x, resid, ldr, out, B, N, S, p, seed, site);
    OCRL_CHECK_LAUNCH("pool_cls_drop");
    return 0;
}

// dX[b][0] += v[b]
__global__ void pool_cls_add_kernel(float* __restrict__ dX, const float* __restrict__ v, int B, int d, int S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * d) return;
    const int b = i / d, c = i - b * d;
    dX[(size_t)b * S * d + c] += v[i];
}

// U[b][hh][c] = scale * sum_e q[b][hh*hd + e] * Wk[hh*hd + e][c]       grid B*h
__global__ __launch_bounds__(PL_T) void pool_cls_u_kernel(const float* __restrict__ q, const float* __restrict__ Win, float* __restrict__ U, int d, int h) {
    const int bh = blockIdx.x, b = bh / h, hh = bh - b * h, hd = d / h;
    const float scale = rsqrtf((float)hd);
    const float* Wk = Win + (size_t)d * d;
    for (int c = threadIdx.x; c < d; c += PL_T) {
        float a = 0.f;
        for (int e = 0; e < hd; ++e) a += q[(size_t)b * d + hh * hd + e] * Wk[(size_t)(hh * hd + e) * d + c];
        U[(size_t)bh * d + c] = a * scale;
    }
}

// stage rows [j, j + PL_TP) of one image (zeros past `jend`) in sx [PL_TP][d + 4]
__device__ __forceinline__ void pl_stage(const float* __restrict__ Xb, float* sx, int j, int jend, int d) {
    const int d4 = d >> 2, ld = d + 4;
    for (int i = threadIdx.x; i < PL_TP * d4; i += PL_T) {
        const int r = i / d4, c4 = i - r * d4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j + r < jend) v = *reinterpret_cast<const float4*>(Xb + (size_t)(j + r) * d + c4 * 4);
        *reinterpret_cast<float4*>(sx + r * ld + c4 * 4) = v;
    }
}

// grid (nchunk, B); part [B][nchunk][h][d + 4]: sum_j e'_hj x_j (d), then (max, sum e, sum e') at d..d+2, e = exp(s - max)
__global__ __launch_bounds__(PL_T) void pool_cls_fwd_kernel(const float* __restrict__ X, const float* __restrict__ U, float* __restrict__ part, int S, int d,
                                                           int h, int chunk, float p, unsigned long long seed, unsigned site) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int nchunk = gridDim.x, ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int ld = d + 4, d4 = d >> 2, hd4 = h * d4;
    float* su = sm;                      // [h][d]
    float* sx = su + h * d;              // [PL_TP][d + 4]
    float* sw = sx + PL_TP * ld;         // [PL_TP][h]  e' of the tile
    float* sal = sw + PL_TP * h;         // [h]         rescale of the running sums
    for (int i = tid; i < h * d; i += PL_T) su[i] = U[(size_t)b * h * d + i];
    const int j0 = ch * chunk, j1 = min(S, j0 + chunk);
    const float* Xb = X + (size_t)b * S * d;
    const float keep_sc = p > 0.f ? 1.f / (1.f - p) : 1.f;
    const uint32_t thr = drop_thresh(p);
    const int pr = tid & 63, hg = tid >> 6;          // scores: lane = row of the tile, wave = heads hg, hg + 4, ...
    float m[4], l[4], a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { m[k] = -INFINITY; l[k] = 0.f; a[k] = 0.f; }
    float4 acc[PL_NACC];
#pragma unroll
    for (int k = 0; k < PL_NACC; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int jt = j0; jt < j1; jt += PL_TP) {
        pl_stage(Xb, sx, jt, j1, d);
        __syncthreads();
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c4 = 0; c4 < d4; ++c4) {
            const float4 xv = *reinterpret_cast<const float4*>(sx + pr * ld + c4 * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (hg + 4 * k < h) s[k] += dot4(xv, *reinterpret_cast<const float4*>(su + (hg + 4 * k) * d + c4 * 4));
        }
        const int j = jt + pr;
        const bool valid = j < j1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int hh = hg + 4 * k;
            if (hh >= h) continue;
            const float sv = valid ? s[k] : -INFINITY;
            const float mn = fmaxf(m[k], wave_max(sv));
            const float al = __expf(m[k] - mn);
            const float e = valid ? __expf(sv - mn) : 0.f;
            float ew = e;
            if (p > 0.f && valid) ew = pl_keep(seed, site, ((unsigned long long)(b * h + hh) * S) * S + j, thr) ? e * keep_sc : 0.f;
            l[k] = l[k] * al + wave_sum(e);
            a[k] = a[k] * al + wave_sum(ew);
            m[k] = mn;
            sw[pr * h + hh] = ew;
            if (pr == 0) sal[hh] = al;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PL_NACC; ++k) {
            const int f = tid + k * PL_T;
            if (f < hd4) {
                const int hh = f / d4, c4 = f - hh * d4;
                const float al = sal[hh];
                float4 t = make_float4(acc[k].x * al, acc[k].y * al, acc[k].z * al, acc[k].w * al);
                for (int r = 0; r < PL_TP; ++r) fma4(t, sw[r * h + hh], *reinterpret_cast<const float4*>(sx + r * ld + c4 * 4));
                acc[k] = t;
            }
        }
        __syncthreads();
    }
    float* pb = part + ((size_t)b * nchunk + ch) * h * ld;
#pragma unroll
    for (int k = 0; k < PL_NACC; ++k) {
        const int f = tid + k * PL_T;
        if (f < hd4) {
            const int hh = f / d4, c4 = f - hh * d4;
            *reinterpret_cast<float4*>(pb + hh * ld + c4 * 4) = acc[k];
        }
    }
    if (pr == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int hh = hg + 4 * k;
            if (hh < h) { pb[hh * ld + d] = m[k]; pb[hh * ld + d + 1] = l[k]; pb[hh * ld + d + 2] = a[k]; }
        }
    }
}

// grid B*h: z [B][h][d], stat [B][h][2] = (a, lse); o[b][hh*hd + e] = Wv[hh*hd + e] . z + bv[hh*hd + e] * a
__global__ __launch_bounds__(PL_T) void pool_cls_merge_kernel(const float* __restrict__ part, const float* __restrict__ Win, const float* __restrict__ bin,
                                                             float* __restrict__ z, float* __restrict__ stat, float* __restrict__ o, int nchunk, int d, int h) {
    __shared__ float sz[256];
    const int bh = blockIdx.x, b = bh / h, hh = bh - b * h, hd = d / h, ld = d + 4, tid = threadIdx.x;
    const float* pb = part + (size_t)b * nchunk * h * ld + (size_t)hh * ld;
    const size_t cs = (size_t)h * ld;                 // chunk stride
    float M = -INFINITY;
    for (int c = 0; c < nchunk; ++c) M = fmaxf(M, pb[c * cs + d]);
    float Ls = 0.f, As = 0.f;
    for (int c = 0; c < nchunk; ++c) {
        const float f = __expf(pb[c * cs + d] - M);
        Ls += f * pb[c * cs + d + 1];
        As += f * pb[c * cs + d + 2];
    }
    const float inv = 1.f / Ls;
    for (int i = tid; i < d; i += PL_T) {
        float t = 0.f;
        for (int c = 0; c < nchunk; ++c) t += __expf(pb[c * cs + d] - M) * pb[c * cs + i];
        sz[i] = t * inv;
        z[(size_t)bh * d + i] = t * inv;
    }
    if (tid == 0) { stat[2 * bh] = As * inv; stat[2 * bh + 1] = M + logf(Ls); }
    __syncthreads();
    const int wv = tid >> 6, lane = tid & 63;
    const float* Wv = Win + (size_t)2 * d * d;
    for (int e = wv; e < hd; e += PL_T / 64) {
        const int r = hh * hd + e;
        float t = 0.f;
        for (int c = lane; c < d; c += 64) t += Wv[(size_t)r * d + c] * sz[c];
        t = wave_sum(t);
        if (lane == 0) o[(size_t)b * d + r] = t + bin[2 * d + r] * As * inv;
    }
}

// grid B*h: G [B][h][d] = W_v,h^T dO_h; gD [B][h][2] = (b_v,h . dO_h, D = z . G + a gb)
__global__ __launch_bounds__(PL_T) void pool_cls_bprep_kernel(const float* __restrict__ dO, const float* __restrict__ Win, const float* __restrict__ bin,
                                                             const float* __restrict__ z, const float* __restrict__ stat, float* __restrict__ G,
                                                             float* __restrict__ gD, int d, int h) {
    __shared__ float red[PL_T / 64];
    const int bh = blockIdx.x, b = bh / h, hh = bh - b * h, hd = d / h, tid = threadIdx.x;
    const float* Wv = Win + (size_t)2 * d * d;
    const float* g = dO + (size_t)b * d + hh * hd;
    float dz = 0.f;
    for (int c = tid; c < d; c += PL_T) {
        float t = 0.f;
        for (int e = 0; e < hd; ++e) t += Wv[(size_t)(hh * hd + e) * d + c] * g[e];
        G[(size_t)bh * d + c] = t;
        dz += t * z[(size_t)bh * d + c];
    }
    dz = wave_sum(dz);
    if ((tid & 63) == 0) red[tid >> 6] = dz;
    __syncthreads();
    if (tid == 0) {
        float gb = 0.f;
        for (int e = 0; e < hd; ++e) gb += bin[2 * d + hh * hd + e] * g[e];
        float D = 0.f;
        for (int w = 0; w < PL_T / 64; ++w) D += red[w];
        gD[2 * bh] = gb;
        gD[2 * bh + 1] = D + stat[2 * bh] * gb;
    }
}

// grid (nchunk, B): dX rows of the chunk; wpart [B][nchunk][h][d] = sum_j ds_hj x_j
__global__ __launch_bounds__(PL_T) void pool_cls_bwd_kernel(const float* __restrict__ X, const float* __restrict__ U, const float* __restrict__ G,
                                                           const float* __restrict__ stat, const float* __restrict__ gD, float* __restrict__ dX,
                                                           float* __restrict__ wpart, int S, int d, int h, int chunk, float p, unsigned long long seed,
                                                           unsigned site) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int nchunk = gridDim.x, ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int ld = d + 4, d4 = d >> 2, hd4 = h * d4;
    float* su = sm;                      // [h][d]
    float* sg = su + h * d;              // [h][d]
    float* sx = sg + h * d;              // [PL_TP][d + 4]
    float* sds = sx + PL_TP * ld;        // [PL_TP][h]
    float* spd = sds + PL_TP * h;        // [PL_TP][h]
    for (int i = tid; i < h * d; i += PL_T) { su[i] = U[(size_t)b * h * d + i]; sg[i] = G[(size_t)b * h * d + i]; }
    const int j0 = ch * chunk, j1 = min(S, j0 + chunk);
    const float* Xb = X + (size_t)b * S * d;
    const float keep_sc = p > 0.f ? 1.f / (1.f - p) : 1.f;
    const uint32_t thr = drop_thresh(p);
    const int pr = tid & 63, hg = tid >> 6;
    float lse[4], gb[4], D[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int hh = min(hg + 4 * k, h - 1);
        lse[k] = stat[2 * (b * h + hh) + 1]; gb[k] = gD[2 * (b * h + hh)]; D[k] = gD[2 * (b * h + hh) + 1];
    }
    float4 acc[PL_NACC];
#pragma unroll
    for (int k = 0; k < PL_NACC; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int jt = j0; jt < j1; jt += PL_TP) {
        pl_stage(Xb, sx, jt, j1, d);
        __syncthreads();
        float s[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c4 = 0; c4 < d4; ++c4) {
            const float4 xv = *reinterpret_cast<const float4*>(sx + pr * ld + c4 * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (hg + 4 * k < h) {
                    s[k] += dot4(xv, *reinterpret_cast<const float4*>(su + (hg + 4 * k) * d + c4 * 4));
                    t[k] += dot4(xv, *reinterpret_cast<const float4*>(sg + (hg + 4 * k) * d + c4 * 4));
                }
        }
        const int j = jt + pr;
        const bool valid = j < j1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int hh = hg + 4 * k;
            if (hh >= h) continue;
            float ds = 0.f, pd = 0.f;
            if (valid) {
                const float pj = __expf(s[k] - lse[k]);
                float kp = 1.f;
                if (p > 0.f) kp = pl_keep(seed, site, ((unsigned long long)(b * h + hh) * S) * S + j, thr) ? keep_sc : 0.f;
                pd = pj * kp;
                ds = pj * ((t[k] + gb[k]) * kp - D[k]);
            }
            sds[pr * h + hh] = ds;
            spd[pr * h + hh] = pd;
        }
        __syncthreads();
        for (int i = tid; i < PL_TP * d4; i += PL_T) {
            const int r = i / d4, c4 = i - r * d4;
            if (jt + r >= j1) break;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int hh = 0; hh < h; ++hh) {
                fma4(v, sds[r * h + hh], *reinterpret_cast<const float4*>(su + hh * d + c4 * 4));
                fma4(v, spd[r * h + hh], *reinterpret_cast<const float4*>(sg + hh * d + c4 * 4));
            }
            *reinterpret_cast<float4*>(dX + ((size_t)b * S + jt + r) * d + c4 * 4) = v;
        }
#pragma unroll
        for (int k = 0; k < PL_NACC; ++k) {
            const int f = tid + k * PL_T;
            if (f < hd4) {
                const int hh = f / d4, c4 = f - hh * d4;
                float4 v = acc[k];
                for (int r = 0; r < PL_TP; ++r) fma4(v, sds[r * h + hh], *reinterpret_cast<const float4*>(sx + r * ld + c4 * 4));
                acc[k] = v;
            }
        }
        __syncthreads();
    }
    float* pb = wpart + ((size_t)b * nchunk + ch) * h * d;
#pragma unroll
    for (int k = 0; k < PL_NACC; ++k) {
        const int f = tid + k * PL_T;
        if (f < hd4) *reinterpret_cast<float4*>(pb + (size_t)f * 4) = acc[k];
    }
}

// grid B*h: w [B][h][d] = sum over chunks; dq[b][hh*hd + e] = scale * Wk[hh*hd + e] . w
__global__ __launch_bounds__(PL_T) void pool_cls_wsum_kernel(const float* __restrict__ wpart, const float* __restrict__ Win, float* __restrict__ w,
                                                            float* __restrict__ dq, int nchunk, int d, int h) {
    __shared__ float sw[256];
    const int bh = blockIdx.x, b = bh / h, hh = bh - b * h, hd = d / h, tid = threadIdx.x;
    for (int i = tid; i < d; i += PL_T) {
        float t = 0.f;
        for (int c = 0; c < nchunk; ++c) t += wpart[(((size_t)b * nchunk + c) * h + hh) * d + i];
        sw[i] = t;
        w[(size_t)bh * d + i] = t;
    }
    __syncthreads();
    const float scale = rsqrtf((float)hd);
    const float* Wk = Win + (size_t)d * d;
    const int wv = tid >> 6, lane = tid & 63;
    for (int e = wv; e < hd; e += PL_T / 64) {
        const int r = hh * hd + e;
        float t = 0.f;
        for (int c = lane; c < d; c += 64) t += Wk[(size_t)r * d + c] * sw[c];
        t = wave_sum(t);
        if (lane == 0) dq[(size_t)b * d + r] = t * scale;
    }
}

// dW [3d][d], db [3d]: rows of q from dq x0^T, of k from scale * q w^T, of v from dO z^T (sums over the B images)
__global__ void pool_cls_wgrad_kernel(const float* __restrict__ dq, const float* __restrict__ x0, const float* __restrict__ q, const float* __restrict__ w,
                                      const float* __restrict__ dO, const float* __restrict__ z, const float* __restrict__ stat, float* __restrict__ dW,
                                      float* __restrict__ db, int B, int d, int h) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nW = 3LL * d * d;
    const int hd = d / h;
    const float scale = rsqrtf((float)hd);
    if (i < nW) {
        const int r = (int)(i / d), c = (int)(i - (long long)r * d);
        float t = 0.f;
        if (r < d) {
            for (int b = 0; b < B; ++b) t += dq[(size_t)b * d + r] * x0[(size_t)b * d + c];
        } else if (r < 2 * d) {
            const int rr = r - d, hh = rr / hd;
            for (int b = 0; b < B; ++b) t += q[(size_t)b * d + rr] * w[((size_t)b * h + hh) * d + c];
            t *= scale;
        } else {
            const int rr = r - 2 * d, hh = rr / hd;
            for (int b = 0; b < B; ++b) t += dO[(size_t)b * d + rr] * z[((size_t)b * h + hh) * d + c];
        }
        dW[i] = t;
    } else if (i < nW + 3 * d) {
        const int r = (int)(i - nW);
        float t = 0.f;
        if (r < d) {
            for (int b = 0; b < B; ++b) t += dq[(size_t)b * d + r];
        } else if (r >= 2 * d) {
            const int rr = r - 2 * d, hh = rr / hd;
            for (int b = 0; b < B; ++b) t += dO[(size_t)b * d + rr] * stat[2 * (b * h + hh)];
        }
        db[r] = t;
    }
}

int pool_cls_nchunk(int B, int S, int* chunk) {
    int want = cdiv(1024, B);                        // about four workgroups per CU over the batch
    if (want > cdiv(S, PL_TP)) want = cdiv(S, PL_TP);
    if (want < 1) want = 1;
    const int c = cdiv(cdiv(S, want), PL_TP) * PL_TP;
    if (chunk) *chunk = c;
    return cdiv(S, c);
}

static size_t cls_fwd_smem(int d, int h) { return ((size_t)h * d + PL_TP * (d + 4) + PL_TP * h + h) * 4; }
static size_t cls_bwd_smem(int d, int h) { return ((size_t)2 * h * d + PL_TP * (d + 4) + 2 * PL_TP * h) * 4; }

int pool_cls_attn_fwd_launch(const PoolClsArgs& a, hipStream_t st) {
    const int d = a.d, h = a.h;
    OCRL_REQUIRE(d % 4 == 0 && d <= 256 && h >= 1 && h * d <= 4 * PL_T * PL_NACC && h <= 16 && d % h == 0, "pool_cls: d %d / h %d not supported", d, h);
    int chunk;
    const int nchunk = pool_cls_nchunk(a.B, a.S, &chunk);
    hipLaunchKernelGGL(pool_cls_u_kernel, dim3(a.B * h), dim3(PL_T), 0, st, a.q, a.Win, a.U, d, h);
    OCRL_CHECK_LAUNCH("pool_cls_u");
    const size_t smem = cls_fwd_smem(d, h);
    static bool attr_set = false;                    // once, for the largest shape accepted (d = 256, h = 16)
    if (!attr_set) {
        OCRL_HIP(hipFuncSetAttribute((const void*)pool_cls_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cls_fwd_smem(256, 16)));
        attr_set = true;
    }
    hipLaunchKernelGGL(pool_cls_fwd_kernel, dim3(nchunk, a.B), dim3(PL_T), smem, st, a.X, a.U, a.part, a.S, d, h, chunk, a.p, a.seed, a.site);
    OCRL_CHECK_LAUNCH("pool_cls_fwd");
    hipLaunchKernelGGL(pool_cls_merge_kernel, dim3(a.B * h), dim3(PL_T), 0, st, a.part, a.Win, a.bin, a.z, a.stat, a.o, nchunk, d, h);
    OCRL_CHECK_LAUNCH("pool_cls_merge");
    return 0;
}

int pool_cls_attn_bwd_launch(const PoolClsArgs& a, hipStream_t st) {
    const int d = a.d, h = a.h;
    OCRL_REQUIRE(d % 4 == 0 && d <= 256 && h >= 1 && h * d <= 4 * PL_T * PL_NACC && h <= 16 && d % h == 0, "pool_cls: d %d / h %d not supported", d, h);
    int chunk;
    const int nchunk = pool_cls_nchunk(a.B, a.S, &chunk);
    hipLaunchKernelGGL(pool_cls_bprep_kernel, dim3(a.B * h), dim3(PL_T), 0, st, a.dO, a.Win, a.bin, a.z, a.stat, a.G, a.gD, d, h);
    OCRL_CHECK_LAUNCH("pool_cls_bprep");
    const size_t smem = cls_bwd_smem(d, h);
    static bool attr_set = false;
    if (!attr_set) {
        OCRL_HIP(hipFuncSetAttribute((const void*)pool_cls_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cls_bwd_smem(256, 16)));
        attr_set = true;
    }
    hipLaunchKernelGGL(pool_cls_bwd_kernel, dim3(nchunk, a.B), dim3(PL_T), smem, st, a.X, a.U, a.G, a.stat, a.gD, a.dX, a.part, a.S, d, h, chunk, a.p,
                       a.seed, a.site);
    OCRL_CHECK_LAUNCH("pool_cls_bwd");
    hipLaunchKernelGGL(pool_cls_wsum_kernel, dim3(a.B * h), dim3(PL_T), 0, st, a.part, a.Win, a.w, a.dq, nchunk, d, h);
    OCRL_CHECK_LAUNCH("pool_cls_wsum");
    const long long n = 3LL * d * d + 3 * d;
    hipLaunchKernelGGL(pool_cls_wgrad_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a.dq, a.x0, a.q, a.w, a.dO, a.z, a.stat, a.dW, a.db, a.B, d, h);
    OCRL_CHECK_LAUNCH("pool_cls_wgrad");
    return 0;
}

int pool_cls_add_launch(float* dX, const float* v, int B, int d, int S, hipStream_t st) {
    hipLaunchKernelGGL(pool_cls_add_kernel, dim3(cdiv((long long)B * d, 256)), dim3(256), 0, st, dX, v, B, d, S);
    OCRL_CHECK_LAUNCH("pool_cls_add");
    return 0;
}

// ---------------------------------------------------------------- non-causal flash attention over all rows (layers before the last)
#define PF_T 128
#define PF_KT 32

// qkv [B*S][3d], O [B*S][d], lse [B*h][S]; grid (cdiv(S, PF_T), B*h)
template <int HD>
__global__ __launch_bounds__(PF_T) void pool_flash_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ O, float* __restrict__ lse, int S, int h,
                                                             float p, unsigned long long seed, unsigned site) {
    __shared__ __attribute__((aligned(16))) float sk[PF_KT][HD];
    __shared__ __attribute__((aligned(16))) float sv[PF_KT][HD];
    const int bh = blockIdx.y, b = bh / h, hh = bh - b * h, d = h * HD, tid = threadIdx.x;
    const int i = blockIdx.x * PF_T + tid;
    const bool valid = i < S;
    const float scale = rsqrtf((float)HD), keep_sc = p > 0.f ? 1.f / (1.f - p) : 1.f;
    const uint32_t thr = drop_thresh(p);
    const float* base = qkv + (size_t)b * S * 3 * d + hh * HD;
    float q[HD], o[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) { q[c] = valid ? base[(size_t)i * 3 * d + c] * scale : 0.f; o[c] = 0.f; }
    float m = -INFINITY, l = 0.f;
    const unsigned long long row = ((unsigned long long)bh * S + (valid ? i : 0)) * S;
    for (int j0 = 0; j0 < S; j0 += PF_KT) {
        for (int t = tid; t < PF_KT * HD / 4; t += PF_T) {
            const int r = t / (HD / 4), c4 = t - r * (HD / 4);
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (j0 + r < S) {
                kv = *reinterpret_cast<const float4*>(base + (size_t)(j0 + r) * 3 * d + d + c4 * 4);
                vv = *reinterpret_cast<const float4*>(base + (size_t)(j0 + r) * 3 * d + 2 * d + c4 * 4);
            }
            *reinterpret_cast<float4*>(&sk[r][c4 * 4]) = kv;
            *reinterpret_cast<float4*>(&sv[r][c4 * 4]) = vv;
        }
        __syncthreads();
        const int jn = min(PF_KT, S - j0);
#pragma unroll 1
        for (int jb = 0; jb < jn; jb += 8) {           // sub-blocks of 8 keys: the scores of one sub-block stay in registers
            float s[8];
            float tmax = -INFINITY;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float a = 0.f;
#pragma unroll
                for (int c = 0; c < HD; ++c) a += q[c] * sk[jb + u][c];
                s[u] = jb + u < jn ? a : -INFINITY;
                tmax = fmaxf(tmax, s[u]);
            }
            const float mn = fmaxf(m, tmax), al = __expf(m - mn);
            l *= al;
#pragma unroll
            for (int c = 0; c < HD; ++c) o[c] *= al;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float e = jb + u < jn ? __expf(s[u] - mn) : 0.f;
                l += e;
                float w = e;
                if (p > 0.f && jb + u < jn) w = pl_keep(seed, site, row + j0 + jb + u, thr) ? e * keep_sc : 0.f;
#pragma unroll
                for (int c = 0; c < HD; ++c) o[c] += w * sv[jb + u][c];
            }
            m = mn;
        }
        __syncthreads();
    }
    if (valid) {
        const float inv = 1.f / l;
        float* orow = O + ((size_t)b * S + i) * d + hh * HD;
#pragma unroll
        for (int c = 0; c < HD; c += 4) *reinterpret_cast<float4*>(orow + c) = make_float4(o[c] * inv, o[c + 1] * inv, o[c + 2] * inv, o[c + 3] * inv);
        lse[(size_t)bh * S + i] = m + logf(l);
    }
}

// Dd[b*h + hh][i] = dO_i . O_i over the head's channels
__global__ void pool_flash_dot_kernel(const float* __restrict__ dO, const float* __restrict__ O, float* __restrict__ Dd, int B, int S, int h, int hd) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * h * S) return;
    const int i = (int)(t % S);
    const long long bh = t / S;
    const int b = (int)(bh / h), hh = (int)(bh % h), d = h * hd;
    const float* a = dO + ((size_t)b * S + i) * d + hh * hd;
    const float* c = O + ((size_t)b * S + i) * d + hh * hd;
    float s = 0.f;
    for (int e = 0; e < hd; ++e) s += a[e] * c[e];
    Dd[t] = s;
}

// thread = query: dq into dqkv[:, 0:d]
template <int HD>
__global__ __launch_bounds__(PF_T) void pool_flash_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ lse,
                                                               const float* __restrict__ Dd, float* __restrict__ dqkv, int S, int h, float p,
                                                               unsigned long long seed, unsigned site) {
    __shared__ __attribute__((aligned(16))) float sk[PF_KT][HD];
    __shared__ __attribute__((aligned(16))) float sv[PF_KT][HD];
    const int bh = blockIdx.y, b = bh / h, hh = bh - b * h, d = h * HD, tid = threadIdx.x;
    const int i = blockIdx.x * PF_T + tid;
    const bool valid = i < S;
    const float scale = rsqrtf((float)HD), keep_sc = p > 0.f ? 1.f / (1.f - p) : 1.f;
    const uint32_t thr = drop_thresh(p);
    const float* base = qkv + (size_t)b * S * 3 * d + hh * HD;
    const float* gbase = dO + (size_t)b * S * d + hh * HD;
    float q[HD], g[HD], dq[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) {
        q[c] = valid ? base[(size_t)i * 3 * d + c] * scale : 0.f;
        g[c] = valid ? gbase[(size_t)i * d + c] : 0.f;
        dq[c] = 0.f;
    }
    const float L = valid ? lse[(size_t)bh * S + i] : 0.f, D = valid ? Dd[(size_t)bh * S + i] : 0.f;
    const unsigned long long row = ((unsigned long long)bh * S + (valid ? i : 0)) * S;
    for (int j0 = 0; j0 < S; j0 += PF_KT) {
        for (int t = tid; t < PF_KT * HD / 4; t += PF_T) {
            const int r = t / (HD / 4), c4 = t - r * (HD / 4);
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (j0 + r < S) {
                kv = *reinterpret_cast<const float4*>(base + (size_t)(j0 + r) * 3 * d + d + c4 * 4);
                vv = *reinterpret_cast<const float4*>(base + (size_t)(j0 + r) * 3 * d + 2 * d + c4 * 4);
            }
            *reinterpret_cast<float4*>(&sk[r][c4 * 4]) = kv;
            *reinterpret_cast<float4*>(&sv[r][c4 * 4]) = vv;
        }
        __syncthreads();
        const int jn = min(PF_KT, S - j0);
        for (int jj = 0; jj < jn; ++jj) {
            float s = 0.f, t = 0.f;
#pragma unroll
            for (int c = 0; c < HD; ++c) { s += q[c] * sk[jj][c]; t += g[c] * sv[jj][c]; }
            const float pj = __expf(s - L);
            float kp = 1.f;
            if (p > 0.f) kp = pl_keep(seed, site, row + j0 + jj, thr) ? keep_sc : 0.f;
            const float ds = pj * (t * kp - D);
#pragma unroll
            for (int c = 0; c < HD; ++c) dq[c] += ds * sk[jj][c];
        }
        __syncthreads();
    }
    if (valid) {
        float* out = dqkv + ((size_t)b * S + i) * 3 * d + hh * HD;
#pragma unroll
        for (int c = 0; c < HD; c += 4) *reinterpret_cast<float4*>(out + c) = make_float4(dq[c] * scale, dq[c + 1] * scale, dq[c + 2] * scale, dq[c + 3] * scale);
    }
}

// thread = key: dk, dv into dqkv[:, d:3d]
template <int HD>
__global__ __launch_bounds__(PF_T) void pool_flash_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ lse,
                                                                const float* __restrict__ Dd, float* __restrict__ dqkv, int S, int h, float p,
                                                                unsigned long long seed, unsigned site) {
    __shared__ __attribute__((aligned(16))) float sq[PF_KT][HD];
    __shared__ __attribute__((aligned(16))) float sg[PF_KT][HD];
    __shared__ float sl[PF_KT], sd[PF_KT];
    const int bh = blockIdx.y, b = bh / h, hh = bh - b * h, d = h * HD, tid = threadIdx.x;
    const int j = blockIdx.x * PF_T + tid;
    const bool valid = j < S;
    const float scale = rsqrtf((float)HD), keep_sc = p > 0.f ? 1.f / (1.f - p) : 1.f;
    const uint32_t thr = drop_thresh(p);
    const float* base = qkv + (size_t)b * S * 3 * d + hh * HD;
    const float* gbase = dO + (size_t)b * S * d + hh * HD;
    float k[HD], v[HD], dk[HD], dv[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) {
        k[c] = valid ? base[(size_t)j * 3 * d + d + c] : 0.f;
        v[c] = valid ? base[(size_t)j * 3 * d + 2 * d + c] : 0.f;
        dk[c] = 0.f; dv[c] = 0.f;
    }
    const int jv = valid ? j : 0;
    for (int i0 = 0; i0 < S; i0 += PF_KT) {
        for (int t = tid; t < PF_KT * HD / 4; t += PF_T) {
            const int r = t / (HD / 4), c4 = t - r * (HD / 4);
            float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), gv = qv;
            if (i0 + r < S) {
                qv = *reinterpret_cast<const float4*>(base + (size_t)(i0 + r) * 3 * d + c4 * 4);
                gv = *reinterpret_cast<const float4*>(gbase + (size_t)(i0 + r) * d + c4 * 4);
            }
            qv.x *= scale; qv.y *= scale; qv.z *= scale; qv.w *= scale;
            *reinterpret_cast<float4*>(&sq[r][c4 * 4]) = qv;
            *reinterpret_cast<float4*>(&sg[r][c4 * 4]) = gv;
        }
        if (tid < PF_KT) {
            const bool ok = i0 + tid < S;
            sl[tid] = ok ? lse[(size_t)bh * S + i0 + tid] : 0.f;
            sd[tid] = ok ? Dd[(size_t)bh * S + i0 + tid] : 0.f;
        }
        __syncthreads();
        const int in = min(PF_KT, S - i0);
        for (int ii = 0; ii < in; ++ii) {
            float s = 0.f, t = 0.f;
#pragma unroll
            for (int c = 0; c < HD; ++c) { s += sq[ii][c] * k[c]; t += sg[ii][c] * v[c]; }
            const float pj = __expf(s - sl[ii]);
            float kp = 1.f;
            if (p > 0.f) kp = pl_keep(seed, site, ((unsigned long long)bh * S + i0 + ii) * S + jv, thr) ? keep_sc : 0.f;
            const float ds = pj * (t * kp - sd[ii]), pd = pj * kp;
#pragma unroll
            for (int c = 0; c < HD; ++c) { dk[c] += ds * sq[ii][c]; dv[c] += pd * sg[ii][c]; }
        }
        __syncthreads();
    }
    if (valid) {
        float* out = dqkv + ((size_t)b * S + j) * 3 * d + hh * HD;
#pragma unroll
        for (int c = 0; c < HD; c += 4) {
            *reinterpret_cast<float4*>(out + d + c) = make_float4(dk[c], dk[c + 1], dk[c + 2], dk[c + 3]);
            *reinterpret_cast<float4*>(out + 2 * d + c) = make_float4(dv[c], dv[c + 1], dv[c + 2], dv[c + 3]);
        }
    }
}

template <int HD>
static int pool_flash_k(const float* qkv, float* O, float* lse, const float* dO, float* Dd, float* dqkv, int B, int S, int h, float p,
                        unsigned long long seed, unsigned site, int backward, hipStream_t st) {
    const dim3 grid(cdiv(S, PF_T), B * h);
    if (!backward) {
        hipLaunchKernelGGL((pool_flash_fwd_kernel<HD>), grid, dim3(PF_T), 0, st, qkv, O, lse, S, h, p, seed, site);
        OCRL_CHECK_LAUNCH("pool_flash_fwd");
        return 0;
    }
    const long long n = (long long)B * h * S;
    hipLaunchKernelGGL(pool_flash_dot_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dO, O, Dd, B, S, h, HD);
    OCRL_CHECK_LAUNCH("pool_flash_dot");
    hipLaunchKernelGGL((pool_flash_bwd_q_kernel<HD>), grid, dim3(PF_T), 0, st, qkv, dO, lse, Dd, dqkv, S, h, p, seed, site);
    OCRL_CHECK_LAUNCH("pool_flash_bwd_q");
    hipLaunchKernelGGL((pool_flash_bwd_kv_kernel<HD>), grid, dim3(PF_T), 0, st, qkv, dO, lse, Dd, dqkv, S, h, p, seed, site);
    OCRL_CHECK_LAUNCH("pool_flash_bwd_kv");
    return 0;
}
int pool_flash_launch(const float* qkv, float* O, float* lse, const float* dO, float* Dd, float* dqkv, int B, int S, int d, int h, float p,
                      unsigned long long seed, unsigned site, int backward, hipStream_t st) {
    OCRL_REQUIRE(B > 0 && S >= 1 && h >= 1 && d % h == 0, "pool_flash: bad shape");
    switch (d / h) {
        case 16: return pool_flash_k<16>(qkv, O, lse, dO, Dd, dqkv, B, S, h, p, seed, site, backward, st);
        case 32: return pool_flash_k<32>(qkv, O, lse, dO, Dd, dqkv, B, S, h, p, seed, site, backward, st);
        case 48: return pool_flash_k<48>(qkv, O, lse, dO, Dd, dqkv, B, S, h, p, seed, site, backward, st);
        case 64: return pool_flash_k<64>(qkv, O, lse, dO, Dd, dqkv, B, S, h, p, seed, site, backward, st);
    }
    OCRL_REQUIRE(false, "pool_flash: head size %d not supported (16, 32, 48, 64)", d / h);
    return -1;
}
