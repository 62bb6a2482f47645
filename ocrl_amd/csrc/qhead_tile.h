// The device steps DQN's value heads share (dqn.hip, c51.hip, qr.hip, iqn.hip), each written once on the row-tile code of acnet_tile.h:
//   unit24            24 random bits as a uniform in [0, 1)
//   eps_greedy        the epsilon-greedy choice of a row from its q values
//   td_row            a row's TD inputs: the action taken, the bootstrap action, done, reward, discount, importance weight
//   wide_fwd_tile     the chain, a wide advantage Linear of A * n columns (entry i of action a in column a * n + i) and, with dueling,
//   wide_bwd_tile     a value Linear of n columns on the same latent, with the dueling rule; forward and backward of one tile
//   wide_bwd_tiles    the body of a wide head's stand-alone backward kernel
//   qhuber_pair       one (i, j) term of the quantile Huber loss and of its cotangent
//   serial_mean       the mean every quantile head forms its q with
// Order of every sum: acnet.hip's for the layers and the slabs; the sums over actions and quantiles here are serial in ascending index.
// Device code in an unnamed namespace: each translation unit that includes this compiles its own copy into its kernels.
#pragma once
#include "acnet_tile.h"
#include "dqn.h"

namespace {

constexpr int WIDE_MAX_N = 64;                  // columns per action of a wide head (atoms, quantiles)
constexpr int LV = WIDE_MAX_N + 4;              // row stride of the value head's tile
constexpr int LQ = ACNET_MAX_ACTIONS;           // row stride of the q tile of a wide head's act kernel

// the uniform in [0, 1) of 24 random bits
__device__ __forceinline__ float unit24(uint32_t bits) { return (float)bits * (1.f / 16777216.f); }

// The choice of `row` from its A q values z (LDS; A <= 64: the scan is serial in a): the thread flips the row's coin and takes the random
// action or the lowest index of the maximum q.
__device__ __forceinline__ void eps_greedy(const float* z, int A, long long row, const DqnActArgs& s) {
    float m = z[0];
    int best = 0;
    for (int a = 1; a < A; ++a)
        if (z[a] > m) { m = z[a]; best = a; }           // strict: the lowest index of the maximum
    uint32_t b0, b1;                                    // the 24 bits of u0 and u1
    if (s.uniforms) {
        b0 = (uint32_t)(s.uniforms[2 * row] * 16777216.f);
        b1 = (uint32_t)(s.uniforms[2 * row + 1] * 16777216.f);
    } else {
        const uint2 w = rng_bits4(s.seed, SITE_DQN_ACT, s.row_offset + (unsigned long long)row);
        b0 = w.x >> 8; b1 = w.y >> 8;
    }
    const float u0 = unit24(b0);
    int act = best;
    if (u0 < s.epsilon) {
        act = (int)(((unsigned long long)b1 * (unsigned long long)A) >> 24);
        act = act < A ? act : A - 1;                    // only a given uniform >= 1 gets here
    }
    s.actions[row] = act;
}

// a row's part of a distributional TD step; star is the bootstrap action, the lowest index of the maximum next_q
struct TdRow {
    int act, star, done;
    float rw, g, wt;
};
__device__ __forceinline__ TdRow td_row(const QTdArgs& s, int A, long long row) {
    TdRow t;
    const long long a = s.actions[row];
    t.act = (int)(a < 0 ? 0 : a >= A ? A - 1 : a);
    t.done = s.dones[row] ? 1 : 0;
    t.rw = s.rewards[row];
    t.g = s.discounts ? s.discounts[row] : s.gamma;
    t.wt = s.weights ? s.weights[row] : 1.f;
    t.star = 0;
    if (!t.done) {                                      // a select: next_q of a finished row is not read
        const float* nq = s.next_q + row * A;
        float m = nq[0];
        for (int k = 1; k < A; ++k)
            if (nq[k] > m) { m = nq[k]; t.star = k; }
    }
    return t;
}

// Forward of one tile of a wide head: leaves the A * n columns in lg [16][LD] (rows past the batch hold the biases' image: finite, never
// written out) and ends on a barrier.  vt [16][LV] is touched only with dueling.
__device__ void wide_fwd_tile(const AcnetArgs& p, int n, long long row0, int rows, float* buf, float* lg, float* vt) {
    int K = p.F;
    const Src lat = run_trunk(p, 1, gsrc(p.x + row0 * p.F, p.F, rows), K, buf, buf + TR * LD, row0, rows, nullptr);
    const int A = p.A;
    lin_fwd_tile(lat, p.wa, p.ba, K, A * n, 0, lg, LD, nullptr, nullptr, rows);
    if (p.wv) lin_fwd_tile(lat, p.wv, p.bv, K, n, 0, vt, LV, nullptr, nullptr, rows);
    __syncthreads();
    if (p.wv) {                                         // one thread per (row, entry): (V + Adv) - mean over the actions
        const float invA = 1.f / (float)A;
        for (int e = threadIdx.x; e < TR * n; e += blockDim.x) {
            const int r = e / n, j = e - r * n;
            float* col = lg + r * LD + j;
            float s = 0.f;
            for (int a = 0; a < A; ++a) s += col[a * n];
            const float v = vt[r * LV + j], mean = invA * s;
            for (int a = 0; a < A; ++a) col[a * n] = (v + col[a * n]) - mean;
        }
        __syncthreads();
    }
}

// Backward of one tile of a wide head from the columns' cotangent in lg (LDS): the dueling rule, the two heads into the latent's
// cotangent, the chain (bwd_trunk).  The chain's tiles are free by now: the layer inputs come from the workspace.
__device__ void wide_bwd_tile(const AcnetArgs& p, int n, long long row0, int rows, bool first, float* buf, float* lg, float* vt) {
    float* slab = p.slab + (long long)blockIdx.x * p.slab_stride;
    const int A = p.A;
    if (p.wv) {                                         // dV = sum over the actions, dAdv = dcolumn - dV / A
        const float invA = 1.f / (float)A;
        for (int e = threadIdx.x; e < TR * n; e += blockDim.x) {
            const int r = e / n, j = e - r * n;
            float* col = lg + r * LD + j;
            float s = 0.f;
            for (int a = 0; a < A; ++a) s += col[a * n];
            vt[r * LV + j] = s;
            const float mean = invA * s;
            for (int a = 0; a < A; ++a) col[a * n] -= mean;
        }
        __syncthreads();
    }
    const int nl = p.n[1];
    const int Kl = nl ? p.dim[1][nl - 1] : p.F;
    const Src feat = Src{p.x + row0 * p.F, p.F, rows, false};
    const Src lat = nl ? Src{p.saved[1][nl - 1] + row0 * Kl, Kl, rows, false} : feat;
    float *g0 = buf, *g1 = buf + TR * LD;
    const Dst dx = Dst{p.dx ? p.dx + row0 * p.F : nullptr, p.F, rows};
    const Dst dlt = nl ? Dst{g0, LD, TR} : dx;
    lin_bwd_tile(lg, LD, nullptr, 0, lat, p.wa, Kl, A * n, slab + p.off_wa, slab + p.off_ba, first, dlt, false, rows);
    if (p.wv) lin_bwd_tile(vt, LV, nullptr, 0, lat, p.wv, Kl, n, slab + p.off_wv, slab + p.off_bv, first, dlt, true, rows);
    bwd_trunk(p, 1, g0, g0, g1, feat, p.F, &dx, false, slab, first, row0, rows);
}

// A wide head's backward kernel: the workgroup's tiles in tile order, each from the cotangent dcols [B, A * n]
__device__ void wide_bwd_tiles(const AcnetArgs& p, int n, const float* dcols, float* buf, float* vt) {
    float* lg = buf + 2 * TR * LD;
    const int NC = p.A * n;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        for (int e = threadIdx.x; e < TR * NC; e += blockDim.x) {
            const int r = e / NC, c = e - r * NC;
            lg[r * LD + c] = r < rows ? dcols[(row0 + r) * NC + c] : 0.f;
        }
        __syncthreads();
        wide_bwd_tile(p, n, row0, rows, tile == (int)blockIdx.x, buf, lg, vt);
        __syncthreads();
    }
}

// the serial mean of N values: every q of the quantile heads is formed by this sum
__device__ __forceinline__ float serial_mean(const float* th, int N) {
    float s = 0.f;
    for (int i = 0; i < N; ++i) s += th[i];
    return s * (1.f / (float)N);
}

// The pair (i, j) of the quantile Huber loss at kappa: Tj = the target's quantile j, x = the quantile value at fraction tau.  Adds the
// loss term to ls and the cotangent term to gs.
__device__ __forceinline__ void qhuber_pair(float Tj, float x, float tau, float kappa, float& ls, float& gs) {
    const float u = Tj - x, au = fabsf(u);
    const float w = fabsf(tau - (u < 0.f ? 1.f : 0.f));
    ls += w * (au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa));
    gs += w * fminf(fmaxf(u, -kappa), kappa);
}

}  // namespace
