// DQN's quantile head on the device (include/ocrl_hip_qr.h): a chain of small Linear layers, a wide advantage Linear of A * N columns
// (quantile i of action a in column a * N + i) and, with dueling, a value Linear of N columns on the same latent: the wide head of
// qhead_tile.h (wide_fwd_tile, wide_bwd_tile) with n = N, the quantile values in the place of c51.hip's logits.  One workgroup of four waves
// owns 16 batch rows, the chain ping-pongs between the first two LDS activation tiles, the third one holds theta [16][LD] (A * N <= 256
// columns) and the value head has a [16][LV] tile.
//   qr_fwd     chain, heads, the dueling rule, then one thread per (row, action): the mean q over the quantiles
//   qr_act     the same, then lane r of a tile chooses for row r from the q values (eps_greedy)
//   qr_bwd     cotangent of theta -> the dueling rule's backward, the heads' and the chain's backward into the workgroup's slab
//   qr_td      forward, the quantile Huber loss and the cotangent, and the backward, per row tile in one kernel.  Once the heads have
//              run the two chain tiles are free (the backward reads the saved layer outputs from the workspace): one takes the bootstrap
//              action's shifted quantiles T [16][N], the other the (row, i) partial losses.  The pairwise part runs one thread per
//              (row, i): a serial loop over j accumulates the loss term and the cotangent term together (the lanes of a row read the
//              same T[r][j]: an LDS broadcast), then the thread writes the cotangent over column i of theta in place, zeros for the other
//              actions.  Partial dw go to the workgroup's slab, the three scalar sums to its row of scal_slab
// The fold of the slabs is acnet_reduce (slab order), the fold of the scalars head_scalars (slab order).
// Order of every sum: acnet.hip's for the layers and the slabs; the sums over actions and quantiles are serial in ascending index; a
// tile's scalar terms are added in row order, the tiles of a slab in tile order.  Every kernel forms q with serial_mean; the pairs are qhuber_pair's.  No atomics.
#include "qhead_tile.h"
#include "qr.h"

namespace {

static_assert(QR_MAX_QUANTILES <= WIDE_MAX_N, "the quantiles of an action fit a row of the value head's tile");
static_assert(QR_MAX_COLS <= ACNET_MAX_WIDTH, "the quantile tile is an activation tile");
static_assert(QR_MAX_QUANTILES <= ACNET_MAX_WIDTH, "T and the partial losses take a row of a chain tile each");

// One thread per (row, action) of the batch's rows: q to c.q (global, may be null) and to qs [16][LQ] (LDS, may be null).
__device__ void qr_q_rows(const AcnetArgs& p, const QrArgs& c, long long row0, int rows, const float* th, float* qs) {
    const int A = p.A, N = c.N;
    for (int e = threadIdx.x; e < rows * A; e += blockDim.x) {
        const int r = e / A, a = e - r * A;
        const float q = serial_mean(th + r * LD + a * N, N);
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
    wide_fwd_tile(p, c.N, row0, rows, buf, th, vt);
    const int NC = p.A * c.N;
    if (c.quantiles)
        for (int e = threadIdx.x; e < rows * NC; e += blockDim.x) {
            const int r = e / NC, n = e - r * NC;
            c.quantiles[(row0 + r) * NC + n] = th[r * LD + n];
        }
    qr_q_rows(p, c, row0, rows, th, nullptr);
}

// Forward of a tile, then lane r < rows chooses for row r from the q values in LDS.
__global__ __launch_bounds__(256) void qr_act_kernel(AcnetArgs p, QrArgs c, DqnActArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    __shared__ float qs[TR * LQ];
    float* th = buf + 2 * TR * LD;
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    wide_fwd_tile(p, c.N, row0, rows, buf, th, vt);
    qr_q_rows(p, c, row0, rows, th, qs);
    __syncthreads();
    const int r = threadIdx.x;
    if (r < rows) eps_greedy(qs + r * LQ, p.A, row0 + r, s);
}

__global__ __launch_bounds__(256) void qr_bwd_kernel(AcnetArgs p, QrArgs c) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    wide_bwd_tiles(p, c.N, c.dquantiles, buf, vt);
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
        TdRow in{0, 0, 1, 0.f, 0.f, 0.f};
        float q = 0.f;
        if (r < rows) {
            in = td_row(s.row, A, row0 + r);
            q = serial_mean(th + r * LD + in.act * N, N);
        }
        t.act[r] = in.act; t.star[r] = in.star; t.done[r] = in.done;
        t.rw[r] = in.rw; t.g[r] = in.g; t.wt[r] = in.wt;
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
            for (int j = 0; j < N; ++j) qhuber_pair(Tr[j], x, tau, kappa, ls, gs);
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
            tm = serial_mean(T + r * LD, N);
            if (s.row.row_loss) s.row.row_loss[row0 + r] = ql;
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
        wide_fwd_tile(p, c.N, row0, rows, buf, th, vt);
        qr_td_rows(p, c, s, row0, rows, first, buf, th, t);
        wide_bwd_tile(p, c.N, row0, rows, first, buf, th, vt);
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
