// DQN's categorical head on the device (include/ocrl_hip_c51.h): a chain of small Linear layers, a wide advantage Linear of A * Z
// columns (atom j of action a in column a * Z + j) and, with dueling, a value Linear of Z columns on the same latent: the wide head of
// qhead_tile.h (wide_fwd_tile, wide_bwd_tile) with n = Z.  One workgroup of four waves owns 16 batch rows, the chain ping-pongs between the
// first two LDS activation tiles and the third one holds the logits [16][LD] (A * Z <= 256 columns: the 64-column `lg` tile of fwd_tile /
// bwd_tile is too narrow, so neither is called here); the value head has a [16][LV] tile.
//   c51_fwd    chain, heads, the dueling rule, then one thread per (row, action): softmax over the atoms and the expectation q
//   c51_act    the same, then lane r of a tile chooses for row r from the q values (eps_greedy)
//   c51_bwd    cotangent of the logits -> the dueling rule's backward, the heads' and the chain's backward into the workgroup's slab
//   c51_td     forward, the projected target distribution m (one thread per (row, atom) gathers m_i), the cross-entropy, the cotangent
//              written over the logits in place, and the backward, per row tile in one kernel.  Once the heads have run the two chain
//              tiles are free (the backward reads the saved layer outputs from the workspace): they hold the bootstrap action's
//              next_probs, beta and m.  Partial dw go to the workgroup's slab, the three scalar sums to its row of scal_slab
// The fold of the slabs is acnet_reduce (slab order), the fold of the scalars head_scalars (slab order).
// Order of every sum: acnet.hip's for the layers and the slabs; the sums over actions and atoms are serial in ascending index; a tile's
// scalar terms are added in row order, the tiles of a slab in tile order.  The expectation accumulates with fused multiply-adds
// (z_j = fma(j, dz, v_min), q = fma(p_j, z_j, q)) so that every kernel here forms the same q.  No atomics.
#include "c51.h"
#include "qhead_tile.h"

namespace {

static_assert(C51_MAX_ATOMS <= WIDE_MAX_N, "the atoms of an action fit a row of the value head's tile");
static_assert(C51_MAX_COLS <= ACNET_MAX_WIDTH, "the logits tile is an activation tile");
static_assert(2 * C51_MAX_ATOMS <= ACNET_MAX_WIDTH, "next_probs and beta share the rows of one chain tile, m takes the other");

__device__ __forceinline__ float atom(const C51Args& c, int j) { return __fmaf_rn((float)j, c.dz, c.v_min); }

// max and sum of exponentials of one action's Z logits
__device__ __forceinline__ void lse_parts(const float* l, int Z, float& m, float& se) {
    m = l[0];
    for (int j = 1; j < Z; ++j) m = fmaxf(m, l[j]);
    se = 0.f;
    for (int j = 0; j < Z; ++j) se += expf(l[j] - m);
}

// One thread per (row, action) of the batch's rows: probabilities to c.probs, q to c.q (global, each may be null) and to qs [16][LQ]
// (LDS, may be null).
__device__ void c51_softmax_rows(const AcnetArgs& p, const C51Args& c, long long row0, int rows, const float* lg, float* qs) {
    const int A = p.A, Z = c.Z;
    for (int e = threadIdx.x; e < rows * A; e += blockDim.x) {
        const int r = e / A, a = e - r * A;
        const float* l = lg + r * LD + a * Z;
        float m, se;
        lse_parts(l, Z, m, se);
        float* pr = c.probs ? c.probs + ((row0 + r) * A + a) * Z : nullptr;
        float q = 0.f;
        for (int j = 0; j < Z; ++j) {
            const float pj = expf(l[j] - m) / se;
            if (pr) pr[j] = pj;
            q = __fmaf_rn(pj, atom(c, j), q);
        }
        if (qs) qs[r * LQ + a] = q;
        if (c.q) c.q[(row0 + r) * A + a] = q;
    }
}

__global__ __launch_bounds__(256) void c51_fwd_kernel(AcnetArgs p, C51Args c) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    float* lg = buf + 2 * TR * LD;
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    wide_fwd_tile(p, c.Z, row0, rows, buf, lg, vt);
    const int NZ = p.A * c.Z;
    if (c.logits)
        for (int e = threadIdx.x; e < rows * NZ; e += blockDim.x) {
            const int r = e / NZ, n = e - r * NZ;
            c.logits[(row0 + r) * NZ + n] = lg[r * LD + n];
        }
    c51_softmax_rows(p, c, row0, rows, lg, nullptr);
}

// Forward of a tile, then lane r < rows chooses for row r from the q values in LDS.
__global__ __launch_bounds__(256) void c51_act_kernel(AcnetArgs p, C51Args c, DqnActArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    __shared__ float qs[TR * LQ];
    float* lg = buf + 2 * TR * LD;
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    wide_fwd_tile(p, c.Z, row0, rows, buf, lg, vt);
    c51_softmax_rows(p, c, row0, rows, lg, qs);
    __syncthreads();
    const int r = threadIdx.x;
    if (r < rows) eps_greedy(qs + r * LQ, p.A, row0 + r, s);
}

__global__ __launch_bounds__(256) void c51_bwd_kernel(AcnetArgs p, C51Args c) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    wide_bwd_tiles(p, c.Z, c.dlogits, buf, vt);
}

// what the row threads of c51_td leave for the (row, atom) and (row, column) threads
struct TdRows {
    int act[TR], star[TR], done[TR];
    float rw[TR], g[TR], wt[TR], mx[TR], se[TR], sm[TR];
    float rs[TR][3];
};

// The TD step of one tile after its forward.  Replaces the logits in lg by dL/dlogits (L = the mean loss), adds the row's three terms
// (w ce, q[a], sum m z) to the slab's partial sums and writes row_loss.  P, BT (one chain tile) and M (the other) are [16][LD] views.
__device__ void c51_td_rows(const AcnetArgs& p, const C51Args& c, const C51TdArgs& s, long long row0, int rows, bool first, float* buf, float* lg,
                            TdRows& t) {
    const int A = p.A, Z = c.Z, tid = threadIdx.x;
    float* P = buf;
    float* BT = buf + C51_MAX_ATOMS;
    float* M = buf + TR * LD;
    if (tid < TR) {                                     // thread r: the row's actions, its inputs and the softmax of the action taken
        const int r = tid;
        TdRow in{0, 0, 1, 0.f, 0.f, 0.f};
        float mx = 0.f, se = 1.f, q = 0.f;
        if (r < rows) {
            in = td_row(s.row, A, row0 + r);
            const float* l = lg + r * LD + in.act * Z;
            lse_parts(l, Z, mx, se);
            for (int j = 0; j < Z; ++j) q = __fmaf_rn(expf(l[j] - mx) / se, atom(c, j), q);
        }
        t.act[r] = in.act; t.star[r] = in.star; t.done[r] = in.done;
        t.rw[r] = in.rw; t.g[r] = in.g; t.wt[r] = in.wt; t.mx[r] = mx; t.se[r] = se;
        t.rs[r][1] = q;
    }
    __syncthreads();
    for (int e = tid; e < rows * Z; e += blockDim.x) {  // thread (r, j): the bootstrap action's mass at atom j and where its target lands
        const int r = e / Z, j = e - r * Z;
        if (t.done[r]) continue;
        P[r * LD + j] = s.next_probs[((row0 + r) * A + t.star[r]) * Z + j];
        const float T = fminf(fmaxf(t.rw[r] + t.g[r] * atom(c, j), c.v_min), c.v_max);
        BT[r * LD + j] = (T - c.v_min) / c.dz;
    }
    __syncthreads();
    for (int e = tid; e < TR * Z; e += blockDim.x) {    // thread (r, i): gathers m_i in ascending j
        const int r = e / Z, i = e - r * Z;
        float m = 0.f;
        if (r < rows) {
            if (t.done[r]) {
                const float beta = (fminf(fmaxf(t.rw[r], c.v_min), c.v_max) - c.v_min) / c.dz;
                m = fmaxf(0.f, 1.f - fabsf(beta - (float)i));
            } else {
                const float *pr = P + r * LD, *bt = BT + r * LD;
                for (int j = 0; j < Z; ++j) m += pr[j] * fmaxf(0.f, 1.f - fabsf(bt[j] - (float)i));
            }
        }
        M[r * LD + i] = m;
    }
    __syncthreads();
    if (tid < TR) {                                     // thread r: the row's sums over the atoms
        const int r = tid;
        float sm = 0.f, ce = 0.f, tz = 0.f;
        if (r < rows) {
            const float* l = lg + r * LD + t.act[r] * Z;
            const float* m = M + r * LD;
            const float mx = t.mx[r], ls = logf(t.se[r]);
            for (int i = 0; i < Z; ++i) {
                sm += m[i];
                ce -= m[i] * ((l[i] - mx) - ls);
                tz += m[i] * atom(c, i);
            }
            if (s.row.row_loss) s.row.row_loss[row0 + r] = ce;
        }
        t.sm[r] = sm;
        t.rs[r][0] = t.wt[r] * ce;
        t.rs[r][2] = tz;
    }
    __syncthreads();
    const int NZ = A * Z;
    for (int e = tid; e < TR * NZ; e += blockDim.x) {   // thread (r, column): the cotangent over the logits
        const int r = e / NZ, n = e - r * NZ;
        const int a = n / Z, i = n - a * Z;
        float v = 0.f;
        if (r < rows && a == t.act[r]) {
            const float pi = expf(lg[r * LD + n] - t.mx[r]) / t.se[r];
            v = t.wt[r] * (pi * t.sm[r] - M[r * LD + i]) / (float)p.B;
        }
        lg[r * LD + n] = v;
    }
    tile_scalars<3>(t.rs, first, p.scal_slab);
}

__global__ __launch_bounds__(256) void c51_td_kernel(AcnetArgs p, C51Args c, C51TdArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float vt[TR * LV];
    __shared__ TdRows t;
    float* lg = buf + 2 * TR * LD;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        const bool first = tile == (int)blockIdx.x;
        wide_fwd_tile(p, c.Z, row0, rows, buf, lg, vt);
        c51_td_rows(p, c, s, row0, rows, first, buf, lg, t);
        wide_bwd_tile(p, c.Z, row0, rows, first, buf, lg, vt);
        __syncthreads();
    }
}

}  // namespace

int c51_fwd_launch(const AcnetArgs& a, const C51Args& c, hipStream_t st) {
    hipLaunchKernelGGL(c51_fwd_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a, c);
    OCRL_CHECK_LAUNCH("c51_fwd");
    return 0;
}
int c51_act_launch(const AcnetArgs& a, const C51Args& c, const DqnActArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(c51_act_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a, c, s);
    OCRL_CHECK_LAUNCH("c51_act");
    return 0;
}
int c51_bwd_launch(const AcnetArgs& a, const C51Args& c, hipStream_t st) {
    hipLaunchKernelGGL(c51_bwd_kernel, dim3(a.S), dim3(256), 0, st, a, c);
    OCRL_CHECK_LAUNCH("c51_bwd");
    return 0;
}
int c51_td_launch(const AcnetArgs& a, const C51Args& c, const C51TdArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(c51_td_kernel, dim3(a.S), dim3(256), 0, st, a, c, s);
    OCRL_CHECK_LAUNCH("c51_td");
    return 0;
}
