// The row-tile steps of the small-Linear-chain heads, shared by acnet.hip (actor-critic), dqn.hip (the Q head), classifier.hip and, through qhead_tile.h, the value heads: one workgroup (4 waves)
// owns a tile of 16 batch rows and walks a chain of Linear layers with the activations in LDS; see acnet.hip for the order of every sum.
// Device code in an unnamed namespace: each translation unit that includes this compiles its own copy into its kernels.
#pragma once
#include "acnet.h"

namespace {

constexpr int TR = 16;                          // rows of a tile
constexpr int LD = ACNET_MAX_WIDTH + 4;         // row stride of an LDS activation tile (16-byte aligned rows, slots (i + kq) % 16)
constexpr int LA = ACNET_MAX_ACTIONS + 4;       // row stride of the logits tile

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a [rows, K] operand: an LDS tile (rows = 16) or rows of a global tensor (rows past the batch read as 0)
struct Src { const float* p; long long ld; int rows; bool vec; };
// a [16, K] destination: an LDS tile or rows of a global tensor (rows past the batch are not written); p == null discards
struct Dst { float* p; long long ld; int rows; };

__device__ __forceinline__ Src gsrc(const float* p, int K, int rows) { return Src{p, K, rows, (K & 3) == 0 && aligned16(p)}; }
__device__ __forceinline__ Src lsrc(const float* p) { return Src{p, LD, TR, true}; }

// elements k .. k + 3 of a row of K floats (0 past the end or for a null row)
__device__ __forceinline__ float4 ld4(const float* row, int k, int K, bool vec) {
    if (!row || k >= K) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) return *reinterpret_cast<const float4*>(row + k);
    return make_float4(row[k], k + 1 < K ? row[k + 1] : 0.f, k + 2 < K ? row[k + 2] : 0.f, k + 3 < K ? row[k + 3] : 0.f);
}

__device__ __forceinline__ float act_fwd(float v, int act) { return act == 1 ? fmaxf(v, 0.f) : act == 2 ? tanhf(v) : v; }

// y [16, N] = act(x [16, K] W^T + bias), W [N, K] row-major in global memory.  Lane (i, kq) holds k = 16 g + 4 kq + u of both operands
// (the same k permutation on both sides).  The waves take the 16-column blocks of N in turn.  y (LDS, stride ldy), g0, g1 (global
// [rows, N] at the tile's first row) may each be null.
__device__ void lin_fwd_tile(Src x, const float* __restrict__ W, const float* __restrict__ bias, int K, int N, int act, float* y, int ldy,
                             float* g0, float* g1, int rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
    const bool wvec = (K & 3) == 0 && aligned16(W);
    const float* xr = i < x.rows ? x.p + (long long)i * x.ld : nullptr;
    for (int nt = wave; nt * 16 < N; nt += 4) {
        const int n = nt * 16 + i;
        const float* wr = n < N ? W + (long long)n * K : nullptr;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k0 = 0; k0 < K; k0 += 32) {
            const int ka = k0 + 4 * kq, kb = ka + 16;
            const float4 xa = ld4(xr, ka, K, x.vec), wa = ld4(wr, ka, K, wvec);
            const float4 xb = ld4(xr, kb, K, x.vec), wb = ld4(wr, kb, K, wvec);
            a0 = mfma4(xa.x, wa.x, a0); a1 = mfma4(xb.x, wb.x, a1);
            a0 = mfma4(xa.y, wa.y, a0); a1 = mfma4(xb.y, wb.y, a1);
            a0 = mfma4(xa.z, wa.z, a0); a1 = mfma4(xb.z, wb.z, a1);
            a0 = mfma4(xa.w, wa.w, a0); a1 = mfma4(xb.w, wb.w, a1);
        }
        if (n < N) {                                    // C: column = lane & 15, row = 4 (lane >> 4) + r
            const float bv = bias[n];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * kq + r;
                const float v = act_fwd(a0[r] + a1[r] + bv, act);
                if (y) y[row * ldy + n] = v;
                if (row < rows) {
                    if (g0) g0[(long long)row * N + n] = v;
                    if (g1) g1[(long long)row * N + n] = v;
                }
            }
        }
    }
}

// global copy of a [rows, K] operand (the latents of an empty trunk)
__device__ void copy_rows(Src s, int K, float* g, int rows) {
    for (int e = threadIdx.x; e < rows * K; e += blockDim.x) {
        const int r = e / K, k = e - r * K;
        g[(long long)r * K + k] = s.p[(long long)r * s.ld + k];
    }
}

// one trunk on a tile: ping-pong between two LDS tiles; returns where its output is (the input itself for an empty trunk)
__device__ Src run_trunk(const AcnetArgs& p, int t, Src in, int& K, float* b0, float* b1, long long row0, int rows, float* lat) {
    for (int l = 0; l < p.n[t]; ++l) {
        const int N = p.dim[t][l];
        float* y = (l & 1) ? b1 : b0;
        float* sv = p.saved[t][l] ? p.saved[t][l] + row0 * N : nullptr;
        lin_fwd_tile(in, p.w[t][l], p.b[t][l], K, N, p.act[t][l], y, LD, sv, l == p.n[t] - 1 && lat ? lat + row0 * N : nullptr, rows);
        __syncthreads();
        in = lsrc(y);
        K = N;
    }
    if (p.n[t] == 0 && lat) copy_rows(in, K, lat + row0 * K, rows);
    return in;
}

// forward of one tile; leaves the logits in lg [16][LA] and the values in vl [16] when the heads exist
__device__ void fwd_tile(const AcnetArgs& p, long long row0, int rows, float* buf, float* lg, float* vl) {
    int Kh = p.F;
    const Src h = run_trunk(p, 0, gsrc(p.x + row0 * p.F, p.F, rows), Kh, buf, buf + TR * LD, row0, rows, nullptr);
    float* f0 = buf + (p.n[0] & 1) * TR * LD;          // the shared output sits in tile (n0 - 1) & 1: the other one and tile 2 are free
    float* f1 = buf + 2 * TR * LD;
    int Kp = Kh;
    const Src lp = run_trunk(p, 1, h, Kp, f0, f1, row0, rows, p.lat_pi);
    if (p.A > 0) {
        lin_fwd_tile(lp, p.wa, p.ba, Kp, p.A, 0, lg, LA, p.logits ? p.logits + row0 * p.A : nullptr, nullptr, rows);
        __syncthreads();
    }
    int Kv = Kh;
    const Src lv = run_trunk(p, 2, h, Kv, f0, f1, row0, rows, p.lat_vf);
    if (p.A > 0 && p.wv) {                              // wv == null: no value head (the Q head of dqn.hip)
        lin_fwd_tile(lv, p.wv, p.bv, Kv, 1, 0, vl, 1, p.values ? p.values + row0 : nullptr, nullptr, rows);
        __syncthreads();
    }
}

// The fold of a tile's scalar terms: the row threads left term j of row r in rs[r][j] and a barrier has passed.  Thread j < N adds the 16
// rows' terms in row order into the workgroup's row of scal_slab [S][8]: written when `first`, else added to (the tiles of a slab in tile
// order).  Ends on a barrier.
template <int N, int M>
__device__ void tile_scalars(const float (*rs)[M], bool first, float* scal_slab) {
    if (threadIdx.x < N) {
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < TR; ++q) sum += rs[q][threadIdx.x];
        float* d = scal_slab + (long long)blockIdx.x * 8 + threadIdx.x;
        *d = first ? sum : *d + sum;
    }
    __syncthreads();
}

// Backward of y = act(x W^T + b) on a tile.  dy [16][ldd] (LDS) holds dL/dy and is turned into dL/d(pre-activation) in place (rows past
// the batch become 0); ys = the layer's saved output [rows, N] (unused for act 0); x = the layer's input as a global operand.
//   dWs [N, K], dbs [N]  the slab's partial sums: written when `first`, else added to
//   dx                   dL/dx [16, K]: written, or added to when `accum`
__device__ void lin_bwd_tile(float* dy, int ldd, const float* ys, int act, Src x, const float* __restrict__ W, int K, int N,
                             float* dWs, float* dbs, bool first, Dst dx, bool accum, int rows) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kq = lane >> 4;
    for (int e = tid; e < TR * N; e += blockDim.x) {
        const int r = e / N, n = e - r * N;
        float g = 0.f;
        if (r < rows) {
            g = dy[r * ldd + n];
            if (act) {
                const float yv = ys[(long long)r * N + n];
                g = act == 1 ? (yv > 0.f ? g : 0.f) : g * (1.f - yv * yv);
            }
        }
        dy[r * ldd + n] = g;
    }
    __syncthreads();
    for (int n = tid; n < N; n += blockDim.x) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < TR; ++r) s += dy[r * ldd + n];
        dbs[n] = first ? s : dbs[n] + s;
    }
    // dW [N, K] += dz^T x: A[n][row] from LDS, B[row][k] from global, 16 rows = 4 steps
    const int ntk = (K + 15) >> 4, ntn = (N + 15) >> 4;
    for (int t = wave; t < ntn * ntk; t += 4) {
        const int tn = t / ntk, tk = t - tn * ntk;
        const int n = tn * 16 + i, kc = tk * 16 + i;
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r = 4 * s + kq;
            const float a = n < N ? dy[r * ldd + n] : 0.f;
            const float b = (kc < K && r < x.rows) ? x.p[(long long)r * x.ld + kc] : 0.f;
            c = mfma4(a, b, c);
        }
        if (kc < K) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nn = tn * 16 + 4 * kq + r;
                if (nn < N) {
                    float* d = dWs + (long long)nn * K + kc;
                    *d = first ? c[r] : *d + c[r];
                }
            }
        }
    }
    // dx [16, K] = dz [16, N] W: A[row][n] from LDS, B[n][k] streamed from global
    if (dx.p) {
        for (int tk = wave; tk * 16 < K; tk += 4) {
            const int kc = tk * 16 + i;
            f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
            for (int n0 = 0; n0 < N; n0 += 32) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int na = n0 + 4 * kq + u, nb = na + 16;
                    const float aa = na < N ? dy[i * ldd + na] : 0.f, ab = nb < N ? dy[i * ldd + nb] : 0.f;
                    const float ba = (na < N && kc < K) ? W[(long long)na * K + kc] : 0.f;
                    const float bb = (nb < N && kc < K) ? W[(long long)nb * K + kc] : 0.f;
                    c0 = mfma4(aa, ba, c0);
                    c1 = mfma4(ab, bb, c1);
                }
            }
            if (kc < K) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * kq + r;
                    if (row < dx.rows) {
                        float* d = dx.p + (long long)row * dx.ld + kc;
                        const float v = c0[r] + c1[r];
                        *d = accum ? *d + v : v;
                    }
                }
            }
        }
    }
    __syncthreads();
}

// d [16, K] = (or +=) a global cotangent g [rows, K] (null: zeros)
__device__ void seed_rows(Dst d, const float* g, int K, bool accum, int rows) {
    if (!d.p || (accum && !g)) return;
    for (int e = threadIdx.x; e < TR * K; e += blockDim.x) {
        const int r = e / K, k = e - r * K;
        if (r >= d.rows) continue;
        const float v = (g && r < rows) ? g[(long long)r * K + k] : 0.f;
        float* q = d.p + (long long)r * d.ld + k;
        *q = accum ? *q + v : v;
    }
}

// Backward of trunk t's layers, last to first.  cur [16][LD] (LDS) holds the cotangent of the trunk's output; a layer's input cotangent
// goes to whichever of g0, g1 `cur` is not, and the walk goes on from there.  Layer 0 is the callers' own: x0 [., K0] is its input and its
// dx goes to *d0, added to when `accum0`; d0 == null sends it to the next tile like every other layer's.  The layers between read their
// inputs from the saved outputs of the workspace.  Returns the tile the walk ended in: with d0 == null the one that holds layer 0's dx
// (`cur` itself for an empty trunk).
__device__ float* bwd_trunk(const AcnetArgs& p, int t, float* cur, float* g0, float* g1, Src x0, int K0, const Dst* d0, bool accum0, float* slab,
                            bool first, long long row0, int rows) {
    for (int l = p.n[t] - 1; l >= 0; --l) {
        const int N = p.dim[t][l], K = l ? p.dim[t][l - 1] : K0;
        const Src x = l ? Src{p.saved[t][l - 1] + row0 * K, K, rows, false} : x0;
        float* nxt = cur == g0 ? g1 : g0;
        lin_bwd_tile(cur, LD, p.saved[t][l] + row0 * N, p.act[t][l], x, p.w[t][l], K, N, slab + p.off_w[t][l], slab + p.off_b[t][l], first,
                     l || !d0 ? Dst{nxt, LD, TR} : *d0, l ? false : accum0, rows);
        cur = nxt;
    }
    return cur;
}

// backward of one head + trunk: head cotangent dhead [16][ldh] (LDS, null without heads), latent cotangent dlat (global, may be null);
// the result is added into dh (`hw`: dh already holds a contribution)
__device__ void bwd_side(const AcnetArgs& p, int t, float* dhead, int ldh, const float* Wh, long long off_wh, long long off_bh, int NH,
                         const float* dlat, Src h, int Kh, Dst dh, bool& hw, float* g0, float* g1, float* slab, bool first, long long row0, int rows) {
    const int nl = p.n[t];
    const int Kl = nl ? p.dim[t][nl - 1] : Kh;          // latent width
    const Dst dlt = nl ? Dst{g0, LD, TR} : dh;
    bool lw = nl ? false : hw;
    if (dlat) { seed_rows(dlt, dlat + row0 * Kl, Kl, lw, rows); lw = true; }
    if (dhead) {
        const Src lat = nl ? Src{p.saved[t][nl - 1] + row0 * Kl, Kl, rows, false} : h;
        lin_bwd_tile(dhead, ldh, nullptr, 0, lat, Wh, Kl, NH, slab + off_wh, slab + off_bh, first, dlt, lw, rows);
        lw = true;
    }
    if (!lw) { seed_rows(dlt, nullptr, Kl, false, rows); lw = true; }
    __syncthreads();
    if (!nl) { hw = lw; return; }
    bwd_trunk(p, t, g0, g0, g1, h, Kh, &dh, hw, slab, first, row0, rows);
    if (dh.p) hw = true;
}

// backward of one tile from the head cotangents in lg / vl (LDS) and the latent cotangents of the arguments
__device__ void bwd_tile(const AcnetArgs& p, long long row0, int rows, bool first, float* buf, float* lg, float* vl) {
    float* slab = p.slab + (long long)blockIdx.x * p.slab_stride;
    const int ns = p.n[0];
    const int Kh = ns ? p.dim[0][ns - 1] : p.F;
    const Src h = ns ? Src{p.saved[0][ns - 1] + row0 * Kh, Kh, rows, false} : Src{p.x + row0 * p.F, p.F, rows, false};
    float *g0 = buf, *g1 = buf + TR * LD, *gh = buf + 2 * TR * LD;
    const Dst dh = ns ? Dst{gh, LD, TR} : Dst{p.dx ? p.dx + row0 * p.F : nullptr, p.F, rows};
    bool hw = false;
    bwd_side(p, 1, p.A > 0 ? lg : nullptr, LA, p.wa, p.off_wa, p.off_ba, p.A, p.dlat_pi, h, Kh, dh, hw, g0, g1, slab, first, row0, rows);
    bwd_side(p, 2, p.A > 0 && p.wv ? vl : nullptr, 1, p.wv, p.off_wv, p.off_bv, 1, p.dlat_vf, h, Kh, dh, hw, g0, g1, slab, first, row0, rows);
    const Dst dx = Dst{p.dx ? p.dx + row0 * p.F : nullptr, p.F, rows};
    bwd_trunk(p, 0, gh, g0, g1, Src{p.x + row0 * p.F, p.F, rows, false}, p.F, &dx, false, slab, first, row0, rows);
}

}  // namespace
