// DQN's quantile head on the device (include/ocrl_hip_qr.h): a chain of small Linear layers, a wide advantage Linear of A * N columns
// (quantile i of action a in column a * N + i) and, with dueling, a value Linear of N columns on the same latent.  The row-tile kernel
// family of c51.hip with the quantile values in the place of the logits: one workgroup of four waves owns 16 batch rows, the chain
// ping-pongs between the first two LDS activation tiles (run_trunk, lin_fwd_tile, lin_bwd_tile of acnet_tile.h), the third one holds
// theta [16][LD] (A * N <= 256 columns) and the value head has a [16][LV] tile.
//   qr_fwd     chain, heads, the dueling rule, then one thread per (row, action): the mean q over the quantiles
//   qr_act     the same, then lane r of a tile flips row r's coin and takes the random action or the lowest index of the maximum q
//              (dqn_act's rule and words)
//   qr_bwd     cotangent of theta -> the dueling rule's backward, the heads' and the chain's backward into the workgroup's slab
//   qr_td      forward, the quantile Huber loss and the cotangent, and the backward, per row tile in one kernel.  Once the heads have
//              run the two chain tiles are free (the backward reads the saved layer outputs from the workspace): one takes the bootstrap
//              action's shifted quantiles T [16][N], the other the (row, i) partial losses.  The pairwise part runs one thread per
//              (row, i): a serial loop over j accumulates the loss term and the cotangent term together (the lanes of a row read the
//              same T[r][j]: an LDS broadcast), then the thread writes the cotangent over column i of theta in place, zeros for the other
//              actions.  Partial dw go to the workgroup's slab, the three scalar sums to its row of scal_slab
// The fold of the slabs is acnet_reduce (slab order), the fold of the scalars head_scalars (slab order).
// Order of every sum: acnet.hip's for the layers and the slabs; the sums over actions and quantiles are serial in ascending index; a
// tile's scalar terms are added in row order, the tiles of a slab in tile order.  Every kernel forms q with qr_mean.  No atomics.
#include "acnet_tile.h"
#include "qr.h"

namespace {

constexpr int LV = QR_MAX_QUANTILES + 4;        // row stride of the value head's tile
constexpr int LQ = ACNET_MAX_ACTIONS;           // row stride of the q tile of qr_act
static_assert(QR_MAX_COLS <= ACNET_MAX_WIDTH, "the quantile tile is an activation tile");
static_assert(QR_MAX_QUANTILES <= ACNET_MAX_WIDTH, "T and the partial losses take a row of a chain tile each");

// q of one action: the mean of its N quantile values
__device__ __forceinline__ float qr_mean(const float* th, int N) {
    float s = 0.f;
    for (int i = 0; i < N; ++i) s += th[i];
    return s * (1.f / (float)N);
}

// Forward of one tile: leaves theta in th [16][LD] (rows past the batch hold the biases' image: finite, never written out) and ends on
// a barrier.  vt [16][LV] is touched only with dueling.
__device__ void qr_fwd_tile(const AcnetArgs& p, const QrArgs& c, long long row0, int rows, float* buf, float* th, float* vt) {
    int K = p.F;
    const Src lat = run_trunk(p, 1, gsrc(p.x + row0 * p.F, p.F, rows), K, buf, buf + TR * LD, row0, rows, nullptr);
    const int A = p.A, N = c.N;
    lin_fwd_tile(lat, p.wa, p.ba, K, A * N, 0, th, LD, nullptr, nullptr, rows);
    if (p.wv) lin_fwd_tile(lat, p.wv, p.bv, K, N, 0, vt, LV, nullptr, nullptr, rows);
    __syncthreads();
    if (p.wv) {                                         // one thread per (row, quantile): (V + Adv) - mean over the actions
        const float invA = 1.f / (float)A;
        for (int e = threadIdx.x; e < TR * N; e += blockDim.x) {
            const int r = e / N, i = e - r * N;
            float* col = th + r * LD + i;
            float s = 0.f;
            for (int a = 0; a < A; ++a) s += col[a * N];
            const float v = vt[r * LV + i], mean = invA * s;
            for (int a = 0; a < A; ++a) col[a * N] = (v + col[a * N]) - mean;
        }
        __syncthreads();
    }
}

// One thread per (row, action) of the batch's rows: q to c.q (global, may be null) and to qs [16][LQ] (LDS, may be null).
__device__ void qr_q_rows(const AcnetArgs& p, const QrArgs& c, long long row0, int rows, const float* th, float* qs) {
    const int A = p.A, N = c.N;
    for (int e = threadIdx.x; e < rows * A; e += blockDim.x) {
        const int r = e / A, a = e - r * A;
        const float q = qr_mean(th + r * LD + a * N, N);
        if (qs) qs[r * LQ + a] = q;
        if (c.q) c.q[(row0 + r) * A + a] = q;
    }
}

__global__ __launch_bounds__(256) void qr_fwd_kernel(AcnetArgs p, QrArgs c) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    float* th = buf + 2 * TR * LD;
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    qr_fwd_tile(p, c, row0, rows, buf, th, vt);
    const int NC = p.A * c.N;
    if (c.quantiles)
        for (int e = threadIdx.x; e < rows * NC; e += blockDim.x) {
            const int r = e / NC, n = e - r * NC;
            c.quantiles[(row0 + r) * NC + n] = th[r * LD + n];
        }
    qr_q_rows(p, c, row0, rows, th, nullptr);
}

// Forward of a tile, then lane r < rows chooses for row r from the q values in LDS: dqn_act_kernel's tail.
__global__ __launch_bounds__(256) void qr_act_kernel(AcnetArgs p, QrArgs c, DqnActArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    __shared__ float qs[TR * LQ];
    float* th = buf + 2 * TR * LD;
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    qr_fwd_tile(p, c, row0, rows, buf, th, vt);
    qr_q_rows(p, c, row0, rows, th, qs);
    __syncthreads();
    const int r = threadIdx.x;
    if (r >= rows) return;
    const long long row = row0 + r;
    const float* z = qs + r * LQ;
    const int A = p.A;
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
    const float u0 = (float)b0 * (1.f / 16777216.f);
    int act = best;
    if (u0 < s.epsilon) {
        act = (int)(((unsigned long long)b1 * (unsigned long long)A) >> 24);
        act = act < A ? act : A - 1;                    // only a given uniform >= 1 gets here
    }
    s.actions[row] = act;
}

// Backward of one tile from theta's cotangent in th (LDS): the dueling rule, the two heads into the latent's cotangent, the chain
// (c51_bwd_tile's steps).  The chain's tiles are free by now: the layer inputs come from the workspace.
__device__ void qr_bwd_tile(const AcnetArgs& p, const QrArgs& c, long long row0, int rows, bool first, float* buf, float* th, float* vt) {
    float* slab = p.slab + (long long)blockIdx.x * p.slab_stride;
    const int A = p.A, N = c.N;
    if (p.wv) {                                         // dV = sum over the actions, dAdv = dtheta - dV / A
        const float invA = 1.f / (float)A;
        for (int e = threadIdx.x; e < TR * N; e += blockDim.x) {
            const int r = e / N, i = e - r * N;
            float* col = th + r * LD + i;
            float s = 0.f;
            for (int a = 0; a < A; ++a) s += col[a * N];
            vt[r * LV + i] = s;
            const float mean = invA * s;
            for (int a = 0; a < A; ++a) col[a * N] -= mean;
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
    lin_bwd_tile(th, LD, nullptr, 0, lat, p.wa, Kl, A * N, slab + p.off_wa, slab + p.off_ba, first, dlt, false, rows);
    if (p.wv) lin_bwd_tile(vt, LV, nullptr, 0, lat, p.wv, Kl, N, slab + p.off_wv, slab + p.off_bv, first, dlt, true, rows);
    float* cur = g0;
    for (int l = nl - 1; l >= 0; --l) {
        const int W = p.dim[1][l], K = l ? p.dim[1][l - 1] : p.F;
        const Src x = l ? Src{p.saved[1][l - 1] + row0 * K, K, rows, false} : feat;
        float* nxt = cur == g0 ? g1 : g0;
        lin_bwd_tile(cur, LD, p.saved[1][l] + row0 * W, p.act[1][l], x, p.w[1][l], K, W, slab + p.off_w[1][l], slab + p.off_b[1][l], first,
                     l ? Dst{nxt, LD, TR} : dx, false, rows);
        cur = nxt;
    }
}

__global__ __launch_bounds__(256) void qr_bwd_kernel(AcnetArgs p, QrArgs c) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    float* th = buf + 2 * TR * LD;
    const int NC = p.A * c.N;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        for (int e = threadIdx.x; e < TR * NC; e += blockDim.x) {
            const int r = e / NC, n = e - r * NC;
            th[r * LD + n] = r < rows ? c.dquantiles[(row0 + r) * NC + n] : 0.f;
        }
        __syncthreads();
        qr_bwd_tile(p, c, row0, rows, tile == (int)blockIdx.x, buf, th, vt);
        __syncthreads();
    }
}

// what the row threads of qr_td leave for the (row, quantile) threads
struct TdRows {
    int act[TR], star[TR], done[TR];
    float rw[TR], g[TR], wt[TR];
    float rs[TR][3];
};

// The TD step of one tile after its forward.  Replaces theta in th by dL/dtheta (L = the mean loss), adds the row's three terms
// (w ql, q[a], mean T) to the slab's partial sums and writes row_loss.  T (one chain tile) and PL (the other) are [16][LD] views.
__device__ void qr_td_rows(const AcnetArgs& p, const QrArgs& c, const QrTdArgs& s, long long row0, int rows, bool first, float* buf, float* th,
                           TdRows& t) {
    const int A = p.A, N = c.N, tid = threadIdx.x;
    const float invN = 1.f / (float)N, kappa = s.kappa;
    float* T = buf;
    float* PL = buf + TR * LD;
    if (tid < TR) {                                     // thread r: the row's actions, its inputs and the q of the action taken
        const int r = tid;
        int act = 0, star = 0, done = 1;
        float rw = 0.f, g = 0.f, wt = 0.f, q = 0.f;
        if (r < rows) {
            const long long row = row0 + r;
            const long long a = s.actions[row];
            act = (int)(a < 0 ? 0 : a >= A ? A - 1 : a);
            done = s.dones[row] ? 1 : 0;
            rw = s.rewards[row];
            g = s.discounts ? s.discounts[row] : s.gamma;
            wt = s.weights ? s.weights[row] : 1.f;
            if (!done) {                                // a select: next_q of a finished row is not read
                const float* nq = s.next_q + row * A;
                float m = nq[0];
                for (int k = 1; k < A; ++k)
                    if (nq[k] > m) { m = nq[k]; star = k; }
            }
            q = qr_mean(th + r * LD + act * N, N);
        }
        t.act[r] = act; t.star[r] = star; t.done[r] = done;
        t.rw[r] = rw; t.g[r] = g; t.wt[r] = wt;
        t.rs[r][1] = q;
    }
    __syncthreads();
    for (int e = tid; e < TR * N; e += blockDim.x) {    // thread (r, j): the bootstrap action's quantile j, shifted
        const int r = e / N, j = e - r * N;
        float v = 0.f;
        if (r < rows) {
            v = t.rw[r];
            if (!t.done[r]) v += t.g[r] * s.next_quantiles[((row0 + r) * A + t.star[r]) * N + j];
        }
        T[r * LD + j] = v;
    }
    __syncthreads();
    for (int e = tid; e < TR * N; e += blockDim.x) {    // thread (r, i): the pairs (i, j) in ascending j, loss and cotangent together
        const int r = e / N, i = e - r * N;
        float* col = th + r * LD + i;
        float ls = 0.f, gs = 0.f;
        int act = -1;
        if (r < rows) {
            act = t.act[r];
            const float x = col[act * N];
            const float tau = ((float)i + 0.5f) / (float)N;
            const float* Tr = T + r * LD;
            for (int j = 0; j < N; ++j) {
                const float u = Tr[j] - x, au = fabsf(u);
                const float w = fabsf(tau - (u < 0.f ? 1.f : 0.f));
                ls += w * (au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa));
                gs += w * fminf(fmaxf(u, -kappa), kappa);
            }
        }
        PL[r * LD + i] = invN * ls;
        const float d = r < rows ? -(t.wt[r] / (float)p.B) * invN * gs : 0.f;
        for (int a = 0; a < A; ++a) col[a * N] = a == act ? d : 0.f;   // column i of the row is this thread's alone
    }
    __syncthreads();
    if (tid < TR) {                                     // thread r: the row's sums over the quantiles
        const int r = tid;
        float ql = 0.f, tm = 0.f;
        if (r < rows) {
            for (int i = 0; i < N; ++i) ql += PL[r * LD + i];
            tm = qr_mean(T + r * LD, N);
            if (s.row_loss) s.row_loss[row0 + r] = ql;
        }
        t.rs[r][0] = t.wt[r] * ql;
        t.rs[r][2] = tm;
    }
    __syncthreads();
    tile_scalars<3>(t.rs, first, p.scal_slab);
}

__global__ __launch_bounds__(256) void qr_td_kernel(AcnetArgs p, QrArgs c, QrTdArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    __shared__ TdRows t;
    float* th = buf + 2 * TR * LD;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        const bool first = tile == (int)blockIdx.x;
        qr_fwd_tile(p, c, row0, rows, buf, th, vt);
        qr_td_rows(p, c, s, row0, rows, first, buf, th, t);
        qr_bwd_tile(p, c, row0, rows, first, buf, th, vt);
        __syncthreads();
    }
}

}  // namespace

int qr_fwd_launch(const AcnetArgs& a, const QrArgs& c, hipStream_t st) {
    hipLaunchKernelGGL(qr_fwd_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a, c);
    OCRL_CHECK_LAUNCH("qr_fwd");
    return 0;
}
int qr_act_launch(const AcnetArgs& a, const QrArgs& c, const DqnActArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(qr_act_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a, c, s);
    OCRL_CHECK_LAUNCH("qr_act");
    return 0;
}
int qr_bwd_launch(const AcnetArgs& a, const QrArgs& c, hipStream_t st) {
    hipLaunchKernelGGL(qr_bwd_kernel, dim3(a.S), dim3(256), 0, st, a, c);
    OCRL_CHECK_LAUNCH("qr_bwd");
    return 0;
}
int qr_td_launch(const AcnetArgs& a, const QrArgs& c, const QrTdArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(qr_td_kernel, dim3(a.S), dim3(256), 0, st, a, c, s);
    OCRL_CHECK_LAUNCH("qr_td");
    return 0;
}
