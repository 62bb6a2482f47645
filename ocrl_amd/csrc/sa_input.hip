// The chain between the CNN encoder and slot attention, x = W2 relu(W0 LN(e4) + b0) + b2 over [B*N, 64] rows, in one pass per direction.
//
// Unfused, the chain is a LayerNorm launch and two GEMM launches forward (6 passes over a [B*N,64] tensor) and five launches plus their
// reduction tails backward (12 passes).  Here a workgroup walks 64-row tiles: the forward reads e4 and writes h1 and x (3 passes), the
// backward reads dx, h1, e4 and writes d e4 (4 passes); LN(e4) is rebuilt from e4, mean and rstd, and d h1 / d LN never leave LDS.
//
// Bitwise contract.  mean, rstd, h1, x and d e4 equal what layernorm16_fwd_kernel<1, 4> / gemm_kernel / layernorm16_bwd_kernel<1, 4> produce:
//   * the LayerNorm arithmetic is theirs: the same 16 lanes per row and float4 per lane, and the row functions of layernorm16.h that
//     those kernels call are the ones called here;
//   * every product is a K = 64 dot product accumulated from zero on v_mfma_f32_32x32x2_f32 over chunks c = 0..7 and steps s = 0..3,
//     MFMA step (c, s) taking k = 8c + s from lanes 0..31 and k = 8c + 4 + s from lanes 32..63 -- gemm_kernel's order, in which the tile
//     shape does not enter -- followed by gemm_kernel's epilogue expressions.
// Each of the 4 waves owns a 32x32 block of the 64x64 output, so a 64x64 weight is a wave's B operand for the life of the workgroup.
// The forward keeps each lane's 32 + 32 values of W0 and W2 in registers and only two row tiles in LDS (three workgroups per CU); the
// backward, short of registers, keeps W0 and half of W2 in LDS beside its three row tiles (two workgroups per CU).  The next tile's
// global loads are in flight, in registers, during the current tile's MFMAs.
//
// The backward also accumulates, in registers over the workgroup's tiles, dW2 += dx^T h1, dW0 += dh1^T LN, db2, db0, dgamma, dbeta and
// leaves them as one slab of SA_INPUT_SLAB floats per workgroup; sa_input_reduce_kernel sums the slabs in a fixed order (no atomics).
#include "common.h"
#include "kernels.h"
#include "layernorm16.h"

#define SAI_TR 64                 // rows per tile
#define SAI_LD 68                 // LDS row stride of a tile: float4 rows stay aligned, 8 consecutive rows cover the banks
#define SAI_MAX_WGS 512           // backward: two workgroups on each of the 256 CUs (256 VGPRs, 75 KB of LDS)
#define SAI_FWD_MAX_WGS 768       // forward: three (168 VGPRs, 34 KB)

// float4 c4 of row `row` of a [R,64] tensor, zero past the end.  The load itself is unconditional (from the last row when past the end):
// a branch around it would keep the prefetch registers of the callers in scratch memory.
__device__ __forceinline__ float4 sai_ld4(const float* __restrict__ p, long long row, long long R, int c4) {
    const float4 v = *reinterpret_cast<const float4*>(p + (row < R ? row : R - 1) * 64 + c4 * 4);
    return row < R ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float sai_ld1(const float* __restrict__ p, long long row, long long R) {
    const float v = p[row < R ? row : R - 1];
    return row < R ? v : 0.f;
}

// C[32x32] = A[32 rows x 64 k] B, A k-contiguous in LDS at `as` (row 0 of the wave's rows), B in registers: wf[c][s] = B(8c + 4h + s, n)
__device__ __forceinline__ void sai_mma_kc(const float* __restrict__ as, const float (&wf)[8][4], f32x16& acc) {
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(as + li * SAI_LD + c * 8 + 4 * lh);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, wf[c][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, wf[c][1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, wf[c][2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, wf[c][3], acc, 0, 0, 0);
    }
}
// C[32x32] += A^T B over the 64 rows of a tile: both operands row-major tiles in LDS, `as` / `bs` at the wave's first column
__device__ __forceinline__ void sai_mma_rows(const float* __restrict__ as, const float* __restrict__ bs, f32x16& acc) {
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
#pragma unroll 2
    for (int c = 0; c < 8; ++c) {
        float fa[4], fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fa[j] = as[(c * 8 + 4 * lh + j) * SAI_LD + li];
            fb[j] = bs[(c * 8 + 4 * lh + j) * SAI_LD + li];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[s], acc, 0, 0, 0);
    }
}

__global__ __launch_bounds__(256, 3) void sa_input_fwd_kernel(const float* __restrict__ e4, const float* __restrict__ g, const float* __restrict__ bta,
                                                              const float* __restrict__ W0, const float* __restrict__ b0,
                                                              const float* __restrict__ W2, const float* __restrict__ b2,
                                                              float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ ln0,
                                                              float* __restrict__ h1, float* __restrict__ x, long long R) {
    __shared__ __attribute__((aligned(16))) float At[SAI_TR * SAI_LD], Ht[SAI_TR * SAI_LD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c4 = lane & 15, rsub = lane >> 4;
    const int li = lane & 31, lh = lane >> 5;
    const int wm0 = (wv >> 1) * 32, wn0 = (wv & 1) * 32;
    // y = a W^T: B(k, n) = W[n][k], k-contiguous
    float w0f[8][4], w2f[8][4];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float4 a = *reinterpret_cast<const float4*>(W0 + (wn0 + li) * 64 + c * 8 + 4 * lh);
        const float4 b = *reinterpret_cast<const float4*>(W2 + (wn0 + li) * 64 + c * 8 + 4 * lh);
        w0f[c][0] = a.x; w0f[c][1] = a.y; w0f[c][2] = a.z; w0f[c][3] = a.w;
        w2f[c][0] = b.x; w2f[c][1] = b.y; w2f[c][2] = b.z; w2f[c][3] = b.w;
    }
    const float b0v = b0[wn0 + li], b2v = b2[wn0 + li];
    const float4 gg = *reinterpret_cast<const float4*>(g + c4 * 4), bb = *reinterpret_cast<const float4*>(bta + c4 * 4);
    const long long ntiles = (R + SAI_TR - 1) / SAI_TR;
    const int lr0 = wv * 16 + rsub;                // this thread's rows of a tile: lr0 + 4 i
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = sai_ld4(e4, (long long)blockIdx.x * SAI_TR + lr0 + 4 * i, R, c4);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long r0 = tile * SAI_TR;
        // ---- LayerNorm -> At
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lr = lr0 + 4 * i;
            const long long row = r0 + lr;
            float mu, rs;
            layernorm16_row_fwd<1>(&v[i], mu, rs);
            const float4 y = layernorm16_affine(v[i], rs, gg, bb);
            *reinterpret_cast<float4*>(At + lr * SAI_LD + c4 * 4) = y;
            if (row < R) {
                if (ln0) *reinterpret_cast<float4*>(ln0 + row * 64 + c4 * 4) = y;
                if (c4 == 0) { mean[row] = mu; rstd[row] = rs; }
            }
        }
        // the next tile's rows (past the last tile: zeros, unused)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = sai_ld4(e4, (tile + gridDim.x) * SAI_TR + lr0 + 4 * i, R, c4);
        __syncthreads();
        // ---- h1 = relu(ln0 W0^T + b0) -> Ht
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        sai_mma_kc(At + wm0 * SAI_LD, w0f, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            Ht[(wm0 + row) * SAI_LD + wn0 + li] = fmaxf(acc[r] + b0v, 0.f);
        }
        __syncthreads();
        // ---- x = h1 W2^T + b2 -> At (the ln0 tile is dead)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        sai_mma_kc(Ht + wm0 * SAI_LD, w2f, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            At[(wm0 + row) * SAI_LD + wn0 + li] = acc[r] + b2v;
        }
        __syncthreads();
        // ---- both tiles leave as float4 rows
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lr = lr0 + 4 * i;
            const long long row = r0 + lr;
            if (row < R) {
                *reinterpret_cast<float4*>(h1 + row * 64 + c4 * 4) = *reinterpret_cast<const float4*>(Ht + lr * SAI_LD + c4 * 4);
                *reinterpret_cast<float4*>(x + row * 64 + c4 * 4) = *reinterpret_cast<const float4*>(At + lr * SAI_LD + c4 * 4);
            }
        }
        __syncthreads();
    }
}

// slab of one workgroup: dW2 [64,64] | dW0 [64,64] | db2 | db0 | dgamma | dbeta
__global__ __launch_bounds__(256, 2) void sa_input_bwd_kernel(const float* __restrict__ dx, const float* __restrict__ h1, const float* __restrict__ e4,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ g, const float* __restrict__ bta,
                                                              const float* __restrict__ W0, const float* __restrict__ W2,
                                                              float* __restrict__ de4, float* __restrict__ slab, long long R) {
    // T0: dx, then d ln0;  T1: h1, then ln0;  T2: d h1
    __shared__ __attribute__((aligned(16))) float T0[SAI_TR * SAI_LD], T1[SAI_TR * SAI_LD], T2[SAI_TR * SAI_LD], W0s[64 * 64], W2s[32 * 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c4 = lane & 15, rsub = lane >> 4;
    const int li = lane & 31, lh = lane >> 5;
    const int wm0 = (wv >> 1) * 32, wn0 = (wv & 1) * 32;
    // dx_in = dy W: B(k, n) = W[k][n], n-contiguous.  The registers hold the fragments of W2's rows 0..31 only, LDS its rows 32..63 and
    // W0: with more of them in registers the kernel spills, and a spill reload waits for the prefetch loads issued before it
    float w2f[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) w2f[c][j] = W2[(c * 8 + 4 * lh + j) * 64 + wn0 + li];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(W0s + (threadIdx.x + 256 * i) * 4) = *reinterpret_cast<const float4*>(W0 + (threadIdx.x + 256 * i) * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i)
        *reinterpret_cast<float4*>(W2s + (threadIdx.x + 256 * i) * 4) = *reinterpret_cast<const float4*>(W2 + 2048 + (threadIdx.x + 256 * i) * 4);
    f32x16 dW2a, dW0a;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dW2a[r] = 0.f; dW0a[r] = 0.f; }
    float4 dg = make_float4(0.f, 0.f, 0.f, 0.f), db = dg, db2 = dg;
    float db0 = 0.f;
    const long long ntiles = (R + SAI_TR - 1) / SAI_TR;
    const int lr0 = wv * 16 + rsub;
    float4 dxn[4], hn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        dxn[i] = sai_ld4(dx, (long long)blockIdx.x * SAI_TR + lr0 + 4 * i, R, c4);
        hn[i] = sai_ld4(h1, (long long)blockIdx.x * SAI_TR + lr0 + 4 * i, R, c4);
    }
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long r0 = tile * SAI_TR;
        float4 xe[4];
        float mu[4], rs[4];
        __syncthreads();                           // the previous tile's readers of T0 / T1 are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lr = lr0 + 4 * i;
            *reinterpret_cast<float4*>(T0 + lr * SAI_LD + c4 * 4) = dxn[i];
            *reinterpret_cast<float4*>(T1 + lr * SAI_LD + c4 * 4) = hn[i];
            db2.x += dxn[i].x; db2.y += dxn[i].y; db2.z += dxn[i].z; db2.w += dxn[i].w;
            // e4, mean, rstd of this tile are first used after the two products below
            xe[i] = sai_ld4(e4, r0 + lr, R, c4);
            mu[i] = sai_ld1(mean, r0 + lr, R);
            rs[i] = sai_ld1(rstd, r0 + lr, R);
        }
        // the next tile's rows (past the last tile: zeros, unused)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dxn[i] = sai_ld4(dx, (tile + gridDim.x) * SAI_TR + lr0 + 4 * i, R, c4);
            hn[i] = sai_ld4(h1, (tile + gridDim.x) * SAI_TR + lr0 + 4 * i, R, c4);
        }
        __syncthreads();
        // ---- d h1 = (dx W2) masked by h1 > 0 (gemm_kernel's mask epilogue) -> T2
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 a = *reinterpret_cast<const float4*>(T0 + (wm0 + li) * SAI_LD + c * 8 + 4 * lh);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w2f[c][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w2f[c][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w2f[c][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w2f[c][3], acc, 0, 0, 0);
        }
#pragma unroll 2
        for (int c = 4; c < 8; ++c) {
            const float4 a = *reinterpret_cast<const float4*>(T0 + (wm0 + li) * SAI_LD + c * 8 + 4 * lh);
            const float* const wk = W2s + ((c - 4) * 8 + 4 * lh) * 64 + wn0 + li;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wk[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wk[64], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wk[128], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wk[192], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int idx = (wm0 + (r & 3) + 8 * (r >> 2) + 4 * lh) * SAI_LD + wn0 + li;
            const float mk = T1[idx];
            float t = acc[r];
            t = mk > 0.f ? t : 0.f * t * (mk + 1.f);
            T2[idx] = t;
            db0 += t;
        }
        // ---- dW2 += dx^T h1
        sai_mma_rows(T0 + wm0, T1 + wn0, dW2a);
        __syncthreads();
        // ---- ln0 rebuilt with the forward's expression -> T1;  d ln0 = d h1 W0 -> T0
        // gamma and beta are re-read per tile (cache hits): held across the loop they cost 8 registers the kernel does not have
        const float4 gg = *reinterpret_cast<const float4*>(g + c4 * 4), bb = *reinterpret_cast<const float4*>(bta + c4 * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 dd = make_float4(xe[i].x - mu[i], xe[i].y - mu[i], xe[i].z - mu[i], xe[i].w - mu[i]);
            *reinterpret_cast<float4*>(T1 + (lr0 + 4 * i) * SAI_LD + c4 * 4) = layernorm16_affine(dd, rs[i], gg, bb);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 2
        for (int c = 0; c < 8; ++c) {
            const float4 a = *reinterpret_cast<const float4*>(T2 + (wm0 + li) * SAI_LD + c * 8 + 4 * lh);
            const float* const wk = W0s + (c * 8 + 4 * lh) * 64 + wn0 + li;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wk[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wk[64], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wk[128], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wk[192], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) T0[(wm0 + (r & 3) + 8 * (r >> 2) + 4 * lh) * SAI_LD + wn0 + li] = acc[r];
        __syncthreads();
        // ---- dW0 += d h1^T ln0
        sai_mma_rows(T2 + wm0, T1 + wn0, dW0a);
        // ---- d e4
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lr = lr0 + 4 * i;
            const long long row = r0 + lr;
            const float4 yv = *reinterpret_cast<const float4*>(T0 + lr * SAI_LD + c4 * 4);
            const Ln16Bwd<1> r = layernorm16_row_bwd<1>(&xe[i], &yv, mu[i], rs[i], &gg, &dg, &db);
            if (row < R) *reinterpret_cast<float4*>(de4 + row * 64 + c4 * 4) = layernorm16_row_dx(r, rs[i], 0);
        }
    }
    // ---- the workgroup's slab
    float* const sl = slab + (size_t)blockIdx.x * SA_INPUT_SLAB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = (wm0 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 64 + wn0 + li;
        sl[o] = dW2a[r];
        sl[4096 + o] = dW0a[r];
    }
    __syncthreads();
    float4* const red = reinterpret_cast<float4*>(T0);          // [3][16 row groups][16]
    red[(0 * 16 + wv * 4 + rsub) * 16 + c4] = db2;
    red[(1 * 16 + wv * 4 + rsub) * 16 + c4] = dg;
    red[(2 * 16 + wv * 4 + rsub) * 16 + c4] = db;
    T1[(wv * 2 + lh) * 32 + li] = db0;                          // column wn0 + li: partials of (wave row, lane half)
    __syncthreads();
    if (threadIdx.x < 48) {
        const int which = threadIdx.x >> 4, c = threadIdx.x & 15;
        float4 a = red[(which * 16) * 16 + c];
#pragma unroll
        for (int k = 1; k < 16; ++k) { const float4 t = red[(which * 16 + k) * 16 + c]; a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w; }
        *reinterpret_cast<float4*>(sl + 8192 + (which == 0 ? 0 : which == 1 ? 128 : 192) + c * 4) = a;
    } else if (threadIdx.x >= 64 && threadIdx.x < 128) {
        const int col = threadIdx.x - 64, wn = col >> 5, i = col & 31;
        sl[8192 + 64 + col] = ((T1[((0 * 2 + wn) * 2 + 0) * 32 + i] + T1[((0 * 2 + wn) * 2 + 1) * 32 + i]) +
                               (T1[((1 * 2 + wn) * 2 + 0) * 32 + i] + T1[((1 * 2 + wn) * 2 + 1) * 32 + i]));
    }
}

// out[col] = sum over the slabs in a fixed order: 8 groups of consecutive slabs, each summed front to back, then the 8 group sums
__global__ __launch_bounds__(256) void sa_input_reduce_kernel(const float* __restrict__ slab, int nslab, float* __restrict__ dW2, float* __restrict__ dW0,
                                                              float* __restrict__ db2, float* __restrict__ db0, float* __restrict__ dgam,
                                                              float* __restrict__ dbet) {
    __shared__ float red[8][32];
    const int ci = threadIdx.x & 31, grp = threadIdx.x >> 5, col = blockIdx.x * 32 + ci;
    const int per = (nslab + 7) / 8, s0 = grp * per, s1 = min(nslab, s0 + per);
    float a = 0.f;
    for (int s = s0; s < s1; ++s) a += slab[(size_t)s * SA_INPUT_SLAB + col];
    red[grp][ci] = a;
    __syncthreads();
    if (threadIdx.x < 32) {
        float t = red[0][ci];
#pragma unroll
        for (int k = 1; k < 8; ++k) t += red[k][ci];
        float* out = col < 4096 ? dW2 + col : col < 8192 ? dW0 + (col - 4096) : col < 8256 ? db2 + (col - 8192) : col < 8320 ? db0 + (col - 8256)
                   : col < 8384 ? dgam + (col - 8320) : dbet + (col - 8384);
        *out = t;
    }
}

void sa_input_plan(long long R, int max_wgs, int out[3]) {
    const long long ntiles = (R + SAI_TR - 1) / SAI_TR;
    long long wgs = max_wgs > 0 && max_wgs < SAI_MAX_WGS ? max_wgs : SAI_MAX_WGS;
    if (wgs > ntiles) wgs = ntiles;
    out[0] = SAI_TR; out[1] = (int)wgs; out[2] = SA_INPUT_SLAB;
}

int sa_input_fwd_launch(const float* e4, const float* gamma, const float* beta, const float* W0, const float* b0, const float* W2, const float* b2,
                        float* mean, float* rstd, float* ln0, float* h1, float* x, long long R, int max_wgs, hipStream_t st) {
    OCRL_REQUIRE(R > 0, "sa_input_fwd: no rows");
    OCRL_REQUIRE(e4 && gamma && beta && W0 && b0 && W2 && b2 && mean && rstd && h1 && x, "sa_input_fwd: null argument");
    OCRL_REQUIRE(aligned16(e4, gamma, beta, W0, W2, ln0, h1, x), "sa_input_fwd: tensors must be 16-byte aligned");
    const long long ntiles = (R + SAI_TR - 1) / SAI_TR;
    long long wgs = max_wgs > 0 && max_wgs < SAI_FWD_MAX_WGS ? max_wgs : SAI_FWD_MAX_WGS;
    if (wgs > ntiles) wgs = ntiles;
    hipLaunchKernelGGL(sa_input_fwd_kernel, dim3((unsigned)wgs), dim3(256), 0, st, e4, gamma, beta, W0, b0, W2, b2, mean, rstd, ln0, h1, x, R);
    OCRL_CHECK_LAUNCH("sa_input_fwd");
    return 0;
}

int sa_input_bwd_launch(const float* dx, const float* h1, const float* e4, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        const float* W0, const float* W2, float* de4, float* dW0, float* db0, float* dW2, float* db2, float* dgamma, float* dbeta,
                        long long R, int max_wgs, float* ws, size_t ws_floats, hipStream_t st) {
    OCRL_REQUIRE(R > 0, "sa_input_bwd: no rows");
    OCRL_REQUIRE(dx && h1 && e4 && mean && rstd && gamma && beta && W0 && W2 && de4 && dW0 && db0 && dW2 && db2 && dgamma && dbeta && ws,
                 "sa_input_bwd: null argument");
    OCRL_REQUIRE(aligned16(dx, h1, e4, gamma, beta, W0, de4, ws), "sa_input_bwd: tensors must be 16-byte aligned");
    int plan[3];
    sa_input_plan(R, max_wgs, plan);
    OCRL_REQUIRE((size_t)plan[1] * SA_INPUT_SLAB <= ws_floats, "sa_input_bwd: workspace too small (%d slabs of %d floats)", plan[1], SA_INPUT_SLAB);
    hipLaunchKernelGGL(sa_input_bwd_kernel, dim3(plan[1]), dim3(256), 0, st, dx, h1, e4, mean, rstd, gamma, beta, W0, W2, de4, ws, R);
    OCRL_CHECK_LAUNCH("sa_input_bwd");
    hipLaunchKernelGGL(sa_input_reduce_kernel, dim3(SA_INPUT_SLAB / 32), dim3(256), 0, st, ws, plan[1], dW2, dW0, db2, db0, dgamma, dbeta);
    OCRL_CHECK_LAUNCH("sa_input_reduce");
    return 0;
}
