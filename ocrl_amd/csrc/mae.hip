// Masked autoencoder (ocrs/mae/models_mae.py, include/ocrl_hip.h ocrl_mae_*): the kernels that are not GEMMs or attention.
// The Linear layers run on the library's GEMM (lin_fwd / lin_bwd_x / lin_bwd_w) and the attention on pool_flash_launch; here are the
// bandwidth-bound passes around them.  Token rows are [B, N, D] with the CLS row first; D, the decoder width and 3 p p are multiples
// of 4, so every row pass moves float4.
//   mae_rank        rank of every entry of a noise row [B, L] (ties by index): ids_restore = rank, mask = rank >= len_keep,
//                   ids_keep[rank] = index for rank < len_keep; what argsort(argsort(noise)) yields.  One workgroup per image, the row in LDS.
//   mae_patch_gather  rows of the patch-embedding GEMM: patch ids[b, i] (or i) of obs [B, 3, S, S] in the Conv2d weight's (c, ph, pw) order
//   mae_tokens      x0[b, 0] = cls + pos[0];  x0[b, 1 + i] = embed[b, i] + pos[1 + id(b, i)];  backward: the embed rows copied out, d cls
//                   summed over the images in image order
//   mae_unshuffle   decoder input: the CLS row, then position l reads embedded row ids_restore[b, l] (< len_keep) or the mask token, plus
//                   decoder_pos_embed; backward gathers the rows back through ids_keep and sums d mask_token per image, then over images
//   mae_gelu        exact (erf) GELU of the stored pre-activation; backward d pre = d y gelu'(pre), in place on d y
//   mae_ln          LayerNorm of any width F % 4 == 0 with the eps given (ViT: 1e-6); one wave per row; backward with an optional residual
//                   added to d x, gamma / beta gradients through per-chunk partials
//   mae_loss        sum_{b, l} mask mean_j (pred - target)^2 / sum mask, the target read from obs in patchify's (ph, pw, c) order;
//                   the same pass writes d pred (scaled by the device scalar d loss) when asked
// No atomics: every sum runs in an order fixed by the shapes, so results repeat bit for bit.
#include "common.h"
#include "kernels.h"

namespace {

__global__ __launch_bounds__(256) void mae_rank_kernel(const float* __restrict__ noise, int* __restrict__ restore, int* __restrict__ keep,
                                                       float* __restrict__ mask, int* __restrict__ restore_out, float* __restrict__ mask_out, int L,
                                                       int len_keep) {
    __shared__ float sn[MAE_MAX_PATCHES];
    const int b = blockIdx.x;
    for (int l = threadIdx.x; l < L; l += 256) sn[l] = noise[(size_t)b * L + l];
    __syncthreads();
    for (int l = threadIdx.x; l < L; l += 256) {
        const float v = sn[l];
        int r = 0;
        for (int j = 0; j < L; ++j) {                 // every lane reads the same LDS word: a broadcast
            const float u = sn[j];
            r += (u < v || (u == v && j < l)) ? 1 : 0;
        }
        const float m = r >= len_keep ? 1.f : 0.f;
        restore[(size_t)b * L + l] = r;
        mask[(size_t)b * L + l] = m;
        if (restore_out) restore_out[(size_t)b * L + l] = r;
        if (mask_out) mask_out[(size_t)b * L + l] = m;
        if (r < len_keep) keep[(size_t)b * len_keep + r] = l;
    }
}

// one thread per 4 (VEC) or 1 consecutive pw of a patch row; out [B n, 3 p p]
template <int VEC>
__global__ __launch_bounds__(256) void mae_patch_gather_kernel(const float* __restrict__ obs, const int* __restrict__ ids, float* __restrict__ out,
                                                               long long total, int n, int S, int p) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int pv = p / VEC, P = 3 * p * p, G = S / p;
    const int w = (int)(t % pv) * VEC;
    long long r = t / pv;
    const int ph = (int)(r % p); r /= p;
    const int c = (int)(r % 3); r /= 3;                // r = b n + i
    const long long b = r / n;
    const int id = ids ? ids[r] : (int)(r - b * n);
    const int gy = id / G, gx = id - gy * G;
    const float* src = obs + ((b * 3 + c) * S + (gy * p + ph)) * (long long)S + gx * p + w;
    float* dst = out + r * P + (c * p + ph) * p + w;
    if (VEC == 4) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
    else dst[0] = src[0];
}

__global__ __launch_bounds__(256) void mae_tokens_fwd_kernel(const float* __restrict__ embed, const float* __restrict__ cls,
                                                             const float* __restrict__ pos, const int* __restrict__ ids, float* __restrict__ x0,
                                                             long long total, int n, int D4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % D4);
    const long long row = t / D4;                      // b (n + 1) + k
    const long long b = row / (n + 1);
    const int k = (int)(row - b * (n + 1));
    float4 a, q;
    if (k == 0) {
        a = reinterpret_cast<const float4*>(cls)[c];
        q = reinterpret_cast<const float4*>(pos)[c];
    } else {
        const long long e = b * n + k - 1;
        const int id = ids ? ids[e] : k - 1;
        a = reinterpret_cast<const float4*>(embed)[e * D4 + c];
        q = reinterpret_cast<const float4*>(pos)[(long long)(1 + id) * D4 + c];
    }
    reinterpret_cast<float4*>(x0)[t] = make_float4(a.x + q.x, a.y + q.y, a.z + q.z, a.w + q.w);
}

// dst[b n + i] = src[b (n + 1) + 1 + idx], idx = ids ? ids[b n + i] : i   (rows of D4 float4): the patch rows without the CLS row
// (tokens backward, ids = null), or the decoder rows back at their kept order (unshuffle backward, ids = ids_keep, src rows [B, Ls + 1])
__global__ __launch_bounds__(256) void mae_rows_kernel(const float* __restrict__ src, const int* __restrict__ ids, float* __restrict__ dst,
                                                       long long total, int n, int Ls, int D4, int dst_cls) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % D4);
    const long long row = t / D4;                      // dst_cls: b (n + 1) + k, row k = 0 is the CLS row; else b n + i
    const int nd = n + dst_cls;
    const long long b = row / nd;
    const int k = (int)(row - b * nd);
    long long s;
    if (dst_cls && k == 0) s = b * (Ls + 1);
    else {
        const int i = k - dst_cls;
        s = b * (Ls + 1) + 1 + (ids ? ids[b * n + i] : i);
    }
    reinterpret_cast<float4*>(dst)[t] = reinterpret_cast<const float4*>(src)[s * D4 + c];
}

// out[c] = sum_{k < n} src[k ld + c] in k order, one thread per column
__global__ __launch_bounds__(256) void mae_rowsum_kernel(const float* __restrict__ src, long long ld, float* __restrict__ out, int n, int F) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= F) return;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s += src[(long long)k * ld + c];
    out[c] = s;
}

__global__ __launch_bounds__(256) void mae_unshuffle_fwd_kernel(const float* __restrict__ e, const float* __restrict__ mtok,
                                                                const float* __restrict__ dpos, const int* __restrict__ restore,
                                                                float* __restrict__ xd, long long total, int L, int len_keep, int D4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % D4);
    const long long row = t / D4;                      // b (L + 1) + k
    const long long b = row / (L + 1);
    const int k = (int)(row - b * (L + 1));
    float4 a;
    if (k == 0) a = reinterpret_cast<const float4*>(e)[b * (len_keep + 1) * D4 + c];
    else {
        const int r = restore[b * L + k - 1];
        a = r < len_keep ? reinterpret_cast<const float4*>(e)[(b * (len_keep + 1) + 1 + r) * D4 + c] : reinterpret_cast<const float4*>(mtok)[c];
    }
    const float4 q = reinterpret_cast<const float4*>(dpos)[(long long)k * D4 + c];
    reinterpret_cast<float4*>(xd)[t] = make_float4(a.x + q.x, a.y + q.y, a.z + q.z, a.w + q.w);
}

// part[b][c] = sum over the removed positions l of image b (in l order) of dxd[b, 1 + l, c]
__global__ __launch_bounds__(256) void mae_mtok_part_kernel(const float* __restrict__ dxd, const float* __restrict__ mask, float* __restrict__ part,
                                                            int L, int Dd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (c >= Dd) return;
    const float* g = dxd + ((long long)b * (L + 1) + 1) * Dd + c;
    const float* m = mask + (long long)b * L;
    float s = 0.f;
    for (int l = 0; l < L; ++l)
        if (m[l] != 0.f) s += g[(long long)l * Dd];
    part[(long long)b * Dd + c] = s;
}

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

__global__ __launch_bounds__(256) void mae_gelu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ y, long long n4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n4) return;
    const float4 v = reinterpret_cast<const float4*>(pre)[t];
    reinterpret_cast<float4*>(y)[t] = make_float4(gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w));
}

__global__ __launch_bounds__(256) void mae_gelu_bwd_kernel(const float* dy, const float* __restrict__ pre, float* dpre,
                                                           long long n4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n4) return;
    const float4 v = reinterpret_cast<const float4*>(pre)[t];
    const float4 g = reinterpret_cast<const float4*>(dy)[t];
    reinterpret_cast<float4*>(dpre)[t] = make_float4(g.x * gelu_d(v.x), g.y * gelu_d(v.y), g.z * gelu_d(v.z), g.w * gelu_d(v.w));
}

// one wave per row, 4 rows per workgroup; the row is read again from cache for the variance and the output
__global__ __launch_bounds__(256) void mae_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ bta,
                                                         float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, long long R,
                                                         int F4, float eps) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    const float4* xr = reinterpret_cast<const float4*>(x) + row * F4;
    // the sums are divided by F, not multiplied by a rounded 1 / F: a row whose sum is exact (a constant row) then has its exact mean;
    // one ulp of the mean, magnified by rstd <= eps^-1/2, was 1e-4 of y at F = 252
    const float nF = 4.f * F4;
    float s = 0.f;
    for (int c = lane; c < F4; c += 64) { const float4 v = xr[c]; s += (v.x + v.y) + (v.z + v.w); }
    const float mu = wave_sum(s) / nF;
    float q = 0.f;
    for (int c = lane; c < F4; c += 64) {
        const float4 v = xr[c];
        const float a = v.x - mu, b = v.y - mu, cc = v.z - mu, d = v.w - mu;
        q += (a * a + b * b) + (cc * cc + d * d);
    }
    const float rs = rsqrtf(wave_sum(q) / nF + eps);
    float4* yr = reinterpret_cast<float4*>(y) + row * F4;
    for (int c = lane; c < F4; c += 64) {
        const float4 v = xr[c], gg = reinterpret_cast<const float4*>(g)[c], bb = reinterpret_cast<const float4*>(bta)[c];
        yr[c] = make_float4((v.x - mu) * rs * gg.x + bb.x, (v.y - mu) * rs * gg.y + bb.y, (v.z - mu) * rs * gg.z + bb.z, (v.w - mu) * rs * gg.w + bb.w);
    }
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

// dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) (+ resid)
__global__ __launch_bounds__(256) void mae_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ g, const float* __restrict__ resid,
                                                         float* __restrict__ dx, long long R, int F4) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    const float4* xr = reinterpret_cast<const float4*>(x) + row * F4;
    const float4* dr = reinterpret_cast<const float4*>(dy) + row * F4;
    const float mu = mean[row], rs = rstd[row], inv = 1.f / (4.f * F4);
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < F4; c += 64) {
        const float4 v = xr[c], d = dr[c], gg = reinterpret_cast<const float4*>(g)[c];
        const float a0 = d.x * gg.x, a1 = d.y * gg.y, a2 = d.z * gg.z, a3 = d.w * gg.w;
        s1 += (a0 + a1) + (a2 + a3);
        s2 += (a0 * (v.x - mu) + a1 * (v.y - mu)) + (a2 * (v.z - mu) + a3 * (v.w - mu));
    }
    const float m1 = wave_sum(s1) * inv, m2 = wave_sum(s2) * rs * inv;
    float4* out = reinterpret_cast<float4*>(dx) + row * F4;
    for (int c = lane; c < F4; c += 64) {
        const float4 v = xr[c], d = dr[c], gg = reinterpret_cast<const float4*>(g)[c];
        float4 o = make_float4(rs * (d.x * gg.x - m1 - (v.x - mu) * rs * m2), rs * (d.y * gg.y - m1 - (v.y - mu) * rs * m2),
                               rs * (d.z * gg.z - m1 - (v.z - mu) * rs * m2), rs * (d.w * gg.w - m1 - (v.w - mu) * rs * m2));
        if (resid) {
            const float4 r = reinterpret_cast<const float4*>(resid)[row * F4 + c];
            o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        out[c] = o;
    }
}

// part[chunk][0:F] = sum over the chunk's rows (in row order) of dy xhat, part[chunk][F:2F] = of dy; one thread per column
__global__ __launch_bounds__(256) void mae_ln_dgb_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, float* __restrict__ part, long long R, int F, long long rpc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= F) return;
    const long long r0 = (long long)blockIdx.y * rpc;
    long long r1 = r0 + rpc;
    if (r1 > R) r1 = R;
    float sg = 0.f, sb = 0.f;
    for (long long r = r0; r < r1; ++r) {
        const float d = dy[r * F + c];
        sg += d * (x[r * F + c] - mean[r]) * rstd[r];
        sb += d;
    }
    part[(long long)blockIdx.y * 2 * F + c] = sg;
    part[(long long)blockIdx.y * 2 * F + F + c] = sb;
}

// grid (L + 1, B): workgroup (0, b) zeroes the CLS row of d pred [B, L + 1, P]; workgroup (1 + l, b) sums patch l's squared error
__global__ __launch_bounds__(256) void mae_loss_kernel(const float* __restrict__ pred, const float* __restrict__ obs, const float* __restrict__ mask,
                                                       const float* __restrict__ dloss, float* __restrict__ part, float* __restrict__ dpred, int L,
                                                       int S, int p, float inv_nmask) {
    __shared__ float red[256];
    const int b = blockIdx.y, P = 3 * p * p, tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (dpred)
            for (int j = tid; j < P; j += 256) dpred[(long long)b * (L + 1) * P + j] = 0.f;
        return;
    }
    const int l = blockIdx.x - 1, G = S / p, gy = l / G, gx = l - gy * G;
    const float m = mask[(long long)b * L + l];
    const float* pr = pred + ((long long)b * L + l) * P;
    float* dp = dpred ? dpred + ((long long)b * (L + 1) + 1 + l) * P : nullptr;
    // d loss / d pred = d loss  mask  2 (pred - target) / (P  sum mask)
    const float gs = dpred ? dloss[0] * m * 2.f / (float)P * inv_nmask : 0.f;
    float s = 0.f;
    for (int j = tid; j < P; j += 256) {               // j = (ph p + pw) 3 + c
        const int c = j % 3, q = j / 3, ph = q / p, pw = q - ph * p;
        const float tg = obs[(((long long)b * 3 + c) * S + gy * p + ph) * S + gx * p + pw];
        const float d = pr[j] - tg;
        s += d * d;
        if (dp) dp[j] = gs * d;
    }
    if (!part) return;
    red[tid] = s;
    __syncthreads();
    block_tree_sum<256>(red);
    if (tid == 0) part[(long long)b * L + l] = m * red[0] / (float)P;
}

// out[0] = out[1] = (sum of part[0 .. n) in a fixed order) * scale: 256 strided partial sums, then a tree
__global__ __launch_bounds__(256) void mae_loss_final_kernel(const float* __restrict__ part, float* __restrict__ out, long long n, float scale) {
    __shared__ float red[256];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    block_tree_sum<256>(red);
    if (threadIdx.x == 0) out[0] = out[1] = red[0] * scale;
}

}  // namespace

int mae_rank_launch(const float* noise, int* restore, int* keep, float* mask, int* restore_out, float* mask_out, int B, int L, int len_keep,
                    hipStream_t st) {
    OCRL_REQUIRE(L >= 1 && L <= MAE_MAX_PATCHES, "mae_rank: 1 <= L <= %d patches (got %d): the noise row is ranked in LDS", MAE_MAX_PATCHES, L);
    OCRL_REQUIRE(B >= 1 && len_keep >= 1 && len_keep <= L, "mae_rank: len_keep must be 1 .. L (got %d of %d)", len_keep, L);
    hipLaunchKernelGGL(mae_rank_kernel, dim3(B), dim3(256), 0, st, noise, restore, keep, mask, restore_out, mask_out, L, len_keep);
    OCRL_CHECK_LAUNCH("mae_rank");
    return 0;
}

int mae_patch_gather_launch(const float* obs, const int* ids, float* out, int B, int n, int S, int p, hipStream_t st, int force_scalar) {
    OCRL_REQUIRE(p >= 1 && S % p == 0 && n >= 1 && n <= (S / p) * (S / p), "mae_patch_gather: bad shape (S %d, patch %d, n %d)", S, p, n);
    if (!force_scalar && p % 4 == 0 && aligned16(obs, out)) {
        const long long total = (long long)B * n * 3 * p * (p / 4);
        hipLaunchKernelGGL(mae_patch_gather_kernel<4>, GRID1D(total), 0, st, obs, ids, out, total, n, S, p);
    } else {
        const long long total = (long long)B * n * 3 * p * p;
        hipLaunchKernelGGL(mae_patch_gather_kernel<1>, GRID1D(total), 0, st, obs, ids, out, total, n, S, p);
    }
    OCRL_CHECK_LAUNCH("mae_patch_gather");
    return 0;
}

int mae_tokens_fwd_launch(const float* embed, const float* cls, const float* pos, const int* ids, float* x0, int B, int n, int D, hipStream_t st) {
    OCRL_REQUIRE(D % 4 == 0 && aligned16(embed, cls, pos, x0), "mae_tokens: D %% 4 == 0 and 16-byte aligned rows (D = %d)", D);
    const long long total = (long long)B * (n + 1) * (D / 4);
    hipLaunchKernelGGL(mae_tokens_fwd_kernel, GRID1D(total), 0, st, embed, cls, pos, ids, x0, total, n, D / 4);
    OCRL_CHECK_LAUNCH("mae_tokens_fwd");
    return 0;
}

int mae_rowsum_launch(const float* src, long long ld, float* out, int n, int F, hipStream_t st) {
    hipLaunchKernelGGL(mae_rowsum_kernel, GRID1D(F), 0, st, src, ld, out, n, F);
    OCRL_CHECK_LAUNCH("mae_rowsum");
    return 0;
}

int mae_tokens_bwd_launch(const float* dx0, float* dembed, float* dcls, int B, int n, int D, hipStream_t st) {
    OCRL_REQUIRE(D % 4 == 0 && aligned16(dx0, dembed), "mae_tokens: D %% 4 == 0 and 16-byte aligned rows (D = %d)", D);
    const long long total = (long long)B * n * (D / 4);
    hipLaunchKernelGGL(mae_rows_kernel, GRID1D(total), 0, st, dx0, (const int*)nullptr, dembed, total, n, n, D / 4, 0);
    OCRL_CHECK_LAUNCH("mae_tokens_bwd");
    return mae_rowsum_launch(dx0, (long long)(n + 1) * D, dcls, B, D, st);
}

int mae_unshuffle_fwd_launch(const float* e, const float* mtok, const float* dpos, const int* restore, float* xd, int B, int L, int len_keep, int Dd,
                             hipStream_t st) {
    OCRL_REQUIRE(Dd % 4 == 0 && aligned16(e, mtok, dpos, xd), "mae_unshuffle: width %% 4 == 0 and 16-byte aligned rows (%d)", Dd);
    const long long total = (long long)B * (L + 1) * (Dd / 4);
    hipLaunchKernelGGL(mae_unshuffle_fwd_kernel, GRID1D(total), 0, st, e, mtok, dpos, restore, xd, total, L, len_keep, Dd / 4);
    OCRL_CHECK_LAUNCH("mae_unshuffle_fwd");
    return 0;
}

int mae_unshuffle_bwd_launch(const float* dxd, const int* keep, const float* mask, float* de, float* dmtok, float* part, int B, int L, int len_keep,
                             int Dd, hipStream_t st) {
    OCRL_REQUIRE(Dd % 4 == 0 && aligned16(dxd, de), "mae_unshuffle: width %% 4 == 0 and 16-byte aligned rows (%d)", Dd);
    const long long total = (long long)B * (len_keep + 1) * (Dd / 4);
    hipLaunchKernelGGL(mae_rows_kernel, GRID1D(total), 0, st, dxd, keep, de, total, len_keep, L, Dd / 4, 1);
    OCRL_CHECK_LAUNCH("mae_unshuffle_bwd");
    hipLaunchKernelGGL(mae_mtok_part_kernel, dim3(cdiv(Dd, 256), B), dim3(256), 0, st, dxd, mask, part, L, Dd);
    OCRL_CHECK_LAUNCH("mae_mtok_part");
    return mae_rowsum_launch(part, Dd, dmtok, B, Dd, st);
}

int mae_gelu_fwd_launch(const float* pre, float* y, long long n, hipStream_t st) {
    OCRL_REQUIRE(n % 4 == 0 && aligned16(pre, y), "mae_gelu: n %% 4 == 0 and 16-byte aligned buffers");
    hipLaunchKernelGGL(mae_gelu_fwd_kernel, GRID1D(n / 4), 0, st, pre, y, n / 4);
    OCRL_CHECK_LAUNCH("mae_gelu_fwd");
    return 0;
}

int mae_gelu_bwd_launch(const float* dy, const float* pre, float* dpre, long long n, hipStream_t st) {
    OCRL_REQUIRE(n % 4 == 0 && aligned16(pre, dy, dpre), "mae_gelu: n %% 4 == 0 and 16-byte aligned buffers");
    hipLaunchKernelGGL(mae_gelu_bwd_kernel, GRID1D(n / 4), 0, st, dy, pre, dpre, n / 4);
    OCRL_CHECK_LAUNCH("mae_gelu_bwd");
    return 0;
}

int mae_ln_fwd_launch(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, long long R, int F, float eps, hipStream_t st) {
    OCRL_REQUIRE(F >= 4 && F % 4 == 0 && aligned16(x, g, b, y), "mae_ln: F %% 4 == 0 and 16-byte aligned rows (F = %d)", F);
    hipLaunchKernelGGL(mae_ln_fwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, st, x, g, b, y, mean, rstd, R, F / 4, eps);
    OCRL_CHECK_LAUNCH("mae_ln_fwd");
    return 0;
}

int mae_ln_chunks(long long R) {
    long long n = (R + 7) / 8;                         // at least 8 rows per chunk
    if (n > 256) n = 256;
    const long long rpc = (R + n - 1) / n;
    return (int)((R + rpc - 1) / rpc);
}

int mae_ln_bwd_launch(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, const float* resid, float* dx, float* dg,
                      float* db, float* part, long long R, int F, hipStream_t st) {
    OCRL_REQUIRE(F >= 4 && F % 4 == 0 && aligned16(x, g, dy, dx, resid),
                 "mae_ln: F %% 4 == 0 and 16-byte aligned rows (F = %d)", F);
    hipLaunchKernelGGL(mae_ln_bwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, st, dy, x, mean, rstd, g, resid, dx, R, F / 4);
    OCRL_CHECK_LAUNCH("mae_ln_bwd");
    const int n = mae_ln_chunks(R);
    const long long rpc = (R + n - 1) / n;
    hipLaunchKernelGGL(mae_ln_dgb_kernel, dim3(cdiv(F, 256), n), dim3(256), 0, st, dy, x, mean, rstd, part, R, F, rpc);
    OCRL_CHECK_LAUNCH("mae_ln_dgb");
    RC(mae_rowsum_launch(part, 2LL * F, dg, n, F, st));
    return mae_rowsum_launch(part + F, 2LL * F, db, n, F, st);
}

int mae_loss_launch(const float* pred, const float* obs, const float* mask, const float* dloss, float* part, float* loss, float* dpred, int B, int L,
                    int len_keep, int S, int p, hipStream_t st) {
    OCRL_REQUIRE(p >= 1 && S % p == 0 && L == (S / p) * (S / p) && (!dpred || dloss), "mae_loss: bad arguments");
    // every image removes L - len_keep patches; at len_keep == L the divisor is zero and the loss NaN, as in the reference
    const float inv_nmask = 1.f / ((float)B * (float)(L - len_keep));
    hipLaunchKernelGGL(mae_loss_kernel, dim3(L + 1, B), dim3(256), 0, st, pred, obs, mask, dloss, part, dpred, L, S, p, inv_nmask);
    OCRL_CHECK_LAUNCH("mae_loss");
    if (loss) {
        hipLaunchKernelGGL(mae_loss_final_kernel, dim3(1), dim3(256), 0, st, part, loss, (long long)B * L, inv_nmask);
        OCRL_CHECK_LAUNCH("mae_loss_final");
    }
    return 0;
}
