// Actor-critic head and PPO minibatch step (sb3s/custom_acnets.py:8-96 plus the action / value heads and the loss that
// stable-baselines3's ActorCriticPolicy and PPO.train put on it; include/ocrl_hip.h ocrl_acnet_*, ocrl_gae).
// Chains of small Linear layers: shared trunk -> policy trunk -> logits, shared trunk -> value trunk -> values.  One workgroup
// (4 waves) owns a tile of 16 batch rows and walks the whole chain with the tile's activations in LDS; every product runs on
// v_mfma_f32_16x16x4_f32 (exact fp32), weights are streamed from global memory straight into the B operand (the first layer's
// [width, F] never has to fit LDS), and the features are read from global memory as the A operand.
//   acnet_fwd        one launch: features -> latents, logits, values; with `saved` set, each trunk layer's output also goes to
//                    the workspace (what dW needs)
//   acnet_bwd        cotangents of latents / logits / values -> per-slab partial dW, db and dfeatures
//   acnet_ppo        forward, log-softmax, log-prob gather, entropy, ratio, clipping, the loss sums and their gradient, and the
//                    backward, per row tile in one kernel; logits, probabilities and layer cotangents never leave LDS
//   acnet_a2c        the same for A2C's loss (no ratio, no clipping): -adv log_prob, the squared value error and the entropy
//   acnet_act        the forward with the rollout's tail in the same launch: log-softmax, the action (drawn from one 24-bit uniform
//                    per row, or the argmax) and its log-probability; one lane owns a row's tail (include/ocrl_hip.h ocrl_acnet_act)
//   acnet_reduce     dw = sum of the slabs in slab order; the six PPO (four A2C) scalars from their partial sums
//   acnet_adv_stats  mean and 1 / (std + 1e-8) (unbiased std) of the advantages, one workgroup, fixed order
//   gae              generalised advantage estimation, one thread per environment walking T backwards
// Order of every sum: a layer output is acc0 + acc1 + bias with acc0 / acc1 the MFMA chains over the even / odd 16-wide k chunks in
// ascending k; workgroup s accumulates its tiles s, s + S, ... into slab s in that order; slabs are summed in slab order.  Nothing
// depends on timing (no atomics), and a row's forward result does not depend on which tile or position it sits in.
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
    if (p.A > 0) {
        lin_fwd_tile(lv, p.wv, p.bv, Kv, 1, 0, vl, 1, p.values ? p.values + row0 : nullptr, nullptr, rows);
        __syncthreads();
    }
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
    float* cur = g0;
    for (int l = nl - 1; l >= 0; --l) {
        const int N = p.dim[t][l], K = l ? p.dim[t][l - 1] : Kh;
        const Src x = l ? Src{p.saved[t][l - 1] + row0 * K, K, rows, false} : h;
        float* nxt = cur == g0 ? g1 : g0;
        const Dst d = l ? Dst{nxt, LD, TR} : dh;
        lin_bwd_tile(cur, LD, p.saved[t][l] + row0 * N, p.act[t][l], x, p.w[t][l], K, N, slab + p.off_w[t][l], slab + p.off_b[t][l], first, d,
                     l ? false : hw, rows);
        cur = nxt;
    }
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
    bwd_side(p, 2, p.A > 0 ? vl : nullptr, 1, p.wv, p.off_wv, p.off_bv, 1, p.dlat_vf, h, Kh, dh, hw, g0, g1, slab, first, row0, rows);
    float* cur = gh;
    for (int l = ns - 1; l >= 0; --l) {
        const int N = p.dim[0][l], K = l ? p.dim[0][l - 1] : p.F;
        const Src x = l ? Src{p.saved[0][l - 1] + row0 * K, K, rows, false} : Src{p.x + row0 * p.F, p.F, rows, false};
        float* nxt = cur == g0 ? g1 : g0;
        const Dst d = l ? Dst{nxt, LD, TR} : Dst{p.dx ? p.dx + row0 * p.F : nullptr, p.F, rows};
        lin_bwd_tile(cur, LD, p.saved[0][l] + row0 * N, p.act[0][l], x, p.w[0][l], K, N, slab + p.off_w[0][l], slab + p.off_b[0][l], first, d, false,
                     rows);
        cur = nxt;
    }
}

__global__ __launch_bounds__(256) void acnet_fwd_kernel(AcnetArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    fwd_tile(p, row0, rows, buf, lg, vl);
}

// the uniform of global row `idx` of a sampling stream: the top 24 bits of one counter draw, in [0, 1)
__host__ __device__ inline float act_uniform(unsigned long long seed, unsigned long long idx) {
    const uint32_t key = rng_key(seed, SITE_ACNET_ACT, (uint32_t)(idx >> 32));
    return (float)(rng_bits1_keyed(key, (uint32_t)idx) >> 8) * (1.f / 16777216.f);
}

// Forward of a tile, then lane r < rows finishes row r from the logits and the value in LDS (A <= 64: the tail is serial in a).
__global__ __launch_bounds__(256) void acnet_act_kernel(AcnetArgs p, AcnetActArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    fwd_tile(p, row0, rows, buf, lg, vl);               // ends on a barrier: lg and vl are complete
    const int r = threadIdx.x;
    if (r >= rows) return;
    const long long row = row0 + r;
    const float* z = lg + r * LA;
    const int A = p.A;
    float m = z[0];
    int best = 0;
    for (int a = 1; a < A; ++a)
        if (z[a] > m) { m = z[a]; best = a; }           // strict: the lowest index of the maximum
    float se = 0.f;
    for (int a = 0; a < A; ++a) se += expf(z[a] - m);
    const float lse = m + logf(se);
    int act = best;
    if (!s.deterministic) {
        const float u = s.uniforms ? s.uniforms[row] : act_uniform(s.seed, s.row_offset + (unsigned long long)row);
        float c = 0.f;
        act = 0;
        for (int a = 0; a + 1 < A; ++a) {
            c += expf(z[a] - lse);
            act += c <= u ? 1 : 0;
        }
    }
    s.actions[row] = act;
    s.log_prob[row] = z[act] - lse;
}

__global__ __launch_bounds__(256) void acnet_act_uniforms_kernel(unsigned long long seed, unsigned long long row_offset, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = act_uniform(seed, row_offset + (unsigned long long)i);
}

__global__ __launch_bounds__(256) void acnet_bwd_kernel(AcnetArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        if (p.A > 0) {
            for (int e = threadIdx.x; e < TR * p.A; e += blockDim.x) {
                const int r = e / p.A, a = e - r * p.A;
                lg[r * LA + a] = (p.dlogits && r < rows) ? p.dlogits[(row0 + r) * p.A + a] : 0.f;
            }
            if (threadIdx.x < TR) vl[threadIdx.x] = (p.dvalues && (int)threadIdx.x < rows) ? p.dvalues[row0 + threadIdx.x] : 0.f;
        }
        __syncthreads();
        bwd_tile(p, row0, rows, tile == (int)blockIdx.x, buf, lg, vl);
        __syncthreads();
    }
}

// The PPO minibatch step of one tile after its forward: thread r < 16 owns row r.  Replaces the logits in lg by dL/dlogits and the values
// in vl by dL/dvalues (L = the mean loss: every row carries 1 / B), and adds the row's six terms to the slab's partial sums.
__device__ void ppo_rows(const AcnetArgs& p, long long row0, int rows, bool first, float* lg, float* vl, float (*rs)[6]) {
    const int r = threadIdx.x;
    if (r < TR) {
        float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float* z = lg + r * LA;
        if (r < rows) {
            const long long row = row0 + r;
            const int A = p.A;
            float m = z[0];
            for (int a = 1; a < A; ++a) m = fmaxf(m, z[a]);
            float se = 0.f;
            for (int a = 0; a < A; ++a) se += expf(z[a] - m);
            const float lse = m + logf(se);
            float H = 0.f;
            for (int a = 0; a < A; ++a) { const float lq = z[a] - lse; H -= expf(lq) * lq; }
            long long act = p.actions[row];
            act = act < 0 ? 0 : act >= A ? A - 1 : act;
            const float logp = z[act] - lse, old = p.old_logp[row];
            float adv = p.adv[row];
            if (p.norm) adv = (adv - p.stats[0]) * p.stats[1];
            const float lr = logp - old, ratio = expf(lr), lo = 1.f - p.clip, hi = 1.f + p.clip;
            const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, lo), hi);
            const bool inside = ratio >= lo && ratio <= hi;
            // d min(s1, s2) / d logp: s1 alone carries a gradient once the clamp is active; a tie shares it evenly (torch.min)
            const float dmin = inside ? s1 : s1 < s2 ? s1 : s1 == s2 ? 0.5f * s1 : 0.f;
            const float v = vl[r], dv = v - p.ret[row], invB = 1.f / (float)p.B;
            t[0] = -fminf(s1, s2); t[1] = dv * dv; t[2] = -H; t[3] = (ratio - 1.f) - lr; t[4] = fabsf(ratio - 1.f) > p.clip ? 1.f : 0.f;
            for (int a = 0; a < A; ++a) {
                const float lq = z[a] - lse, q = expf(lq);
                const float dlogp = (a == act ? 1.f : 0.f) - q;
                z[a] = invB * (-dmin * dlogp + p.ent_coef * q * (lq + H));
            }
            vl[r] = invB * p.vf_coef * 2.f * dv;
        } else {
            for (int a = 0; a < p.A; ++a) z[a] = 0.f;
            vl[r] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) rs[r][j] = t[j];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < TR; ++q) s += rs[q][threadIdx.x];
        float* d = p.scal_slab + (long long)blockIdx.x * 8 + threadIdx.x;
        *d = first ? s : *d + s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void acnet_ppo_kernel(AcnetArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    __shared__ float rs[TR][6];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        const bool first = tile == (int)blockIdx.x;
        fwd_tile(p, row0, rows, buf, lg, vl);
        ppo_rows(p, row0, rows, first, lg, vl, rs);
        bwd_tile(p, row0, rows, first, buf, lg, vl);
        __syncthreads();
    }
}

// The A2C step of one tile after its forward, in the shape of ppo_rows: lse, q_a and H are computed by the same operations.  Replaces
// the logits in lg by dL/dlogits and the values in vl by dL/dvalues and adds the row's three terms (-adv log_prob, (v - ret)^2, -H) to the
// slab's partial sums.
__device__ void a2c_rows(const AcnetArgs& p, long long row0, int rows, bool first, float* lg, float* vl, float (*rs)[3]) {
    const int r = threadIdx.x;
    if (r < TR) {
        float t[3] = {0.f, 0.f, 0.f};
        float* z = lg + r * LA;
        if (r < rows) {
            const long long row = row0 + r;
            const int A = p.A;
            float m = z[0];
            for (int a = 1; a < A; ++a) m = fmaxf(m, z[a]);
            float se = 0.f;
            for (int a = 0; a < A; ++a) se += expf(z[a] - m);
            const float lse = m + logf(se);
            float H = 0.f;
            for (int a = 0; a < A; ++a) { const float lq = z[a] - lse; H -= expf(lq) * lq; }
            long long act = p.actions[row];
            act = act < 0 ? 0 : act >= A ? A - 1 : act;
            const float logp = z[act] - lse;
            float adv = p.adv[row];
            if (p.norm) adv = (adv - p.stats[0]) * p.stats[1];
            const float v = vl[r], dv = v - p.ret[row], invB = 1.f / (float)p.B;
            t[0] = -(adv * logp); t[1] = dv * dv; t[2] = -H;
            for (int a = 0; a < A; ++a) {
                const float lq = z[a] - lse, q = expf(lq);
                const float dlogp = (a == act ? 1.f : 0.f) - q;
                z[a] = invB * (-adv * dlogp + p.ent_coef * q * (lq + H));
            }
            vl[r] = invB * p.vf_coef * 2.f * dv;
        } else {
            for (int a = 0; a < p.A; ++a) z[a] = 0.f;
            vl[r] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) rs[r][j] = t[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < TR; ++q) s += rs[q][threadIdx.x];
        float* d = p.scal_slab + (long long)blockIdx.x * 8 + threadIdx.x;
        *d = first ? s : *d + s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void acnet_a2c_kernel(AcnetArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    __shared__ float rs[TR][3];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        const bool first = tile == (int)blockIdx.x;
        fwd_tile(p, row0, rows, buf, lg, vl);
        a2c_rows(p, row0, rows, first, lg, vl, rs);
        bwd_tile(p, row0, rows, first, buf, lg, vl);
        __syncthreads();
    }
}

// scalars: the first three partial sums are policy, value and entropy terms for both losses; PPO carries two more (nsum = 5: approx_kl
// and the clip fraction, outputs 4 and 5), A2C none (nsum = 3: four outputs)
__global__ __launch_bounds__(256) void acnet_reduce_kernel(AcnetReduceArgs r) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < r.total) {
        float s = 0.f;
        for (int k = 0; k < r.S; ++k) s += r.slab[k * r.stride + e];
        int q = 0;
        while (q + 1 < r.np && e >= r.off[q + 1]) ++q;
        r.dst[q][e - r.off[q]] = s;
    }
    if (r.scal_slab && blockIdx.x == 0 && threadIdx.x == 0) {
        float t[5];
        for (int j = 0; j < r.nsum; ++j) {
            float s = 0.f;
            for (int k = 0; k < r.S; ++k) s += r.scal_slab[k * 8 + j];
            t[j] = s / (float)r.B;
        }
        r.scal_out[0] = t[0] + r.ent_coef * t[2] + r.vf_coef * t[1];
        r.scal_out[1] = t[0]; r.scal_out[2] = t[1]; r.scal_out[3] = t[2];
        for (int j = 3; j < r.nsum; ++j) r.scal_out[j + 1] = t[j];
    }
}

// fixed-order block sum: thread t adds elements t, t + 256, ...; the 256 partials are folded in a tree
__device__ float block_sum256(float v, float* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    block_tree_sum<256>(sh);
    const float s = sh[0];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(256) void acnet_adv_stats_kernel(const float* __restrict__ adv, int B, float* __restrict__ stats) {
    __shared__ float sh[256];
    float s = 0.f;
    for (int e = threadIdx.x; e < B; e += 256) s += adv[e];
    const float mean = block_sum256(s, sh) / (float)B;
    float q = 0.f;
    for (int e = threadIdx.x; e < B; e += 256) { const float d = adv[e] - mean; q += d * d; }
    const float var = block_sum256(q, sh) / (float)(B - 1);
    if (threadIdx.x == 0) { stats[0] = mean; stats[1] = 1.f / (sqrtf(var) + 1e-8f); }
}

__global__ __launch_bounds__(64) void gae_kernel(const float* __restrict__ rw, const float* __restrict__ val, const float* __restrict__ st,
                                                 const float* __restrict__ lastv, const float* __restrict__ dones, float* __restrict__ adv,
                                                 float* __restrict__ ret, int T, int E, float gamma, float lam) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    float a = 0.f, nv = lastv[e], nt = 1.f - dones[e];
    for (int t = T - 1; t >= 0; --t) {
        const long long q = (long long)t * E + e;
        const float v = val[q];
        const float delta = rw[q] + gamma * nv * nt - v;
        a = delta + gamma * lam * nt * a;
        adv[q] = a;
        ret[q] = a + v;
        nv = v;
        nt = 1.f - st[q];
    }
}

}  // namespace

int acnet_fwd_launch(const AcnetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(acnet_fwd_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("acnet_fwd");
    return 0;
}
int acnet_act_launch(const AcnetArgs& a, const AcnetActArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(acnet_act_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a, s);
    OCRL_CHECK_LAUNCH("acnet_act");
    return 0;
}
int acnet_act_uniforms_launch(unsigned long long seed, unsigned long long row_offset, long long n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(acnet_act_uniforms_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, seed, row_offset, n, out);
    OCRL_CHECK_LAUNCH("acnet_act_uniforms");
    return 0;
}
int acnet_bwd_launch(const AcnetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(acnet_bwd_kernel, dim3(a.S), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("acnet_bwd");
    return 0;
}
int acnet_ppo_launch(const AcnetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(acnet_ppo_kernel, dim3(a.S), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("acnet_ppo");
    return 0;
}
int acnet_a2c_launch(const AcnetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(acnet_a2c_kernel, dim3(a.S), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("acnet_a2c");
    return 0;
}
int acnet_reduce_launch(const AcnetReduceArgs& r, hipStream_t st) {
    hipLaunchKernelGGL(acnet_reduce_kernel, dim3(cdiv(r.total > 0 ? r.total : 1, 256)), dim3(256), 0, st, r);
    OCRL_CHECK_LAUNCH("acnet_reduce");
    return 0;
}
int acnet_adv_stats_launch(const float* adv, int B, float* stats, hipStream_t st) {
    hipLaunchKernelGGL(acnet_adv_stats_kernel, dim3(1), dim3(256), 0, st, adv, B, stats);
    OCRL_CHECK_LAUNCH("acnet_adv_stats");
    return 0;
}
int acnet_gae_launch(const float* rewards, const float* values, const float* starts, const float* last_values, const float* dones, float* adv, float* ret,
                     int T, int E, float gamma, float lam, hipStream_t st) {
    hipLaunchKernelGGL(gae_kernel, dim3(cdiv(E, 64)), dim3(64), 0, st, rewards, values, starts, last_values, dones, adv, ret, T, E, gamma, lam);
    OCRL_CHECK_LAUNCH("ocrl_gae");
    return 0;
}
