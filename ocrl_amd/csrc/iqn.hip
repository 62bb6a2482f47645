// DQN's implicit quantile head on the device (include/ocrl_hip_iqn.h): every batch row is evaluated at N sampled fractions, so the row
// tiles of qr.hip run over E = B * N expanded rows (row e = b * N + s).  One workgroup of four waves owns 16 expanded rows: it builds
// the cosine tile [16][LC] in LDS, runs the embedding Linear (lin_fwd_tile, ReLU; phi goes to the workspace when the backward needs it)
// into the third activation tile, multiplies by features[e / N] in place (z), walks the chain between the first two tiles (run_trunk)
// and leaves theta in a [16][LA] tile.  A tile may hold rows of several batch rows, or a part of one: nothing in the forward couples
// them, and what crosses expanded rows (q, the row losses, dfeatures) is folded over s by a small kernel after the tiles.
//   iqn_taus    one thread per (b, s): the fraction from the counter RNG
//   iqn_fwd     a tile's forward; theta to [B, A, N] with stride N
//   iqn_q       one thread per (b, a): q = the mean of theta over s, serial
//   iqn_act     one workgroup per batch row walks its samples in tiles of 16, ascending: thread a adds theta[s][a] to its sum in s order
//               (the serial sum of iqn_q), then thread 0 chooses for the row (eps_greedy of qhead_tile.h)
//   iqn_bwd     cotangent of theta -> the output Linear's, the chain's and the embedding's backward into the workgroup's slab; z is
//               rebuilt from phi in the third tile (the chain's first layer reads it), dz * phi goes to the workspace for dfeatures
//   iqn_dx      one thread per (b, j): dfeatures = the sum of dz * phi over s, serial
//   iqn_td      forward, the quantile Huber loss and the cotangent, and the backward, per tile in one kernel.  Once the output Linear
//               has run the two chain tiles are free: the first takes the shifted quantiles T [<= 16][Np] of the batch rows present in
//               the tile.  One thread per expanded row walks j serially, leaves its partial loss and the theta of the action taken in
//               the workspace and writes the cotangent over its row of the theta tile
//   iqn_td_fold one thread per batch row: the sums over i of the partial losses and of theta, the mean of T, row_loss, and the three
//               scalar terms into the slabs' sums (tile_scalars); and dfeatures as iqn_dx
// The fold of the slabs is acnet_reduce (slab order), the fold of the scalars head_scalars (slab order).
// Order of every sum: acnet.hip's for the layers and the slabs; every sum over s, i or j is serial in ascending index.  No atomics.
#include "fqf.h"
#include "iqn.h"
#include "qhead_tile.h"

namespace {

constexpr int LC = IQN_MAX_COS + 4;             // row stride of the cosine tile
static_assert(IQN_MAX_SAMPLES <= ACNET_MAX_WIDTH, "T takes a row of a chain tile per batch row");
static_assert((3 * TR * LD + TR * LC + TR * LA) * sizeof(float) + 1024 <= 65536, "the tiles stay under the static LDS limit");

// the fraction of sample s of row R: the top 24 bits of word s & 1 of group 32 R + (s >> 1)
__device__ __forceinline__ float iqn_tau(unsigned long long seed, unsigned long long R, int s) {
    const uint2 w = rng_bits4(seed, SITE_IQN_TAU, R * 32ull + (unsigned long long)(s >> 1));
    return unit24(((s & 1) ? w.y : w.x) >> 8);
}

__global__ __launch_bounds__(256) void iqn_taus_kernel(unsigned long long seed, unsigned long long row_offset, long long total, int N,
                                                       float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long long b = e / N;
    out[e] = iqn_tau(seed, row_offset + (unsigned long long)b, (int)(e - b * N));
}

// The cosine tile of the 16 expanded rows whose fractions are in tl (LDS; a barrier has passed): ct [16][LC], rows past `rows` zero.
// Ends on a barrier.
__device__ void iqn_cos_tile(const IqnArgs& c, int rows, const float* tl, float* ct) {
    const int C = c.C;
    for (int e = threadIdx.x; e < TR * C; e += blockDim.x) {
        const int r = e / C, k = e - r * C;
        ct[r * LC + k] = r < rows ? cospif((float)k * tl[r]) : 0.f;
    }
    __syncthreads();
}

// z = features[e / N] * phi in place on the tile zt [16][LD] that holds phi (rows past `rows` become 0).  Ends on a barrier.
__device__ void iqn_gate_tile(const IqnArgs& c, int F, long long e0, int rows, float* zt) {
    for (int e = threadIdx.x; e < TR * F; e += blockDim.x) {
        const int r = e / F, j = e - r * F;
        zt[r * LD + j] = r < rows ? c.feat[((e0 + r) / c.N) * F + j] * zt[r * LD + j] : 0.f;
    }
    __syncthreads();
}

// Forward of one tile of expanded rows e0 .. e0 + rows: leaves the cosines in ct, z in the third tile of buf and theta in ot [16][LA]
// (rows past `rows` hold the biases' image: finite, never written out) and ends on a barrier.
__device__ void iqn_fwd_tile(const AcnetArgs& p, const IqnArgs& c, long long e0, int rows, const float* tl, float* buf, float* ct, float* ot) {
    const int F = p.dim[0][0];
    float* zt = buf + 2 * TR * LD;
    iqn_cos_tile(c, rows, tl, ct);
    lin_fwd_tile(Src{ct, LC, TR, true}, p.w[0][0], p.b[0][0], c.C, F, 1, zt, LD, p.saved[0][0] ? p.saved[0][0] + e0 * F : nullptr, nullptr, rows);
    __syncthreads();
    iqn_gate_tile(c, F, e0, rows, zt);
    int K = F;
    const Src lat = run_trunk(p, 1, lsrc(zt), K, buf, buf + TR * LD, e0, rows, nullptr);
    lin_fwd_tile(lat, p.wa, p.ba, K, p.A, 0, ot, LA, nullptr, nullptr, rows);
    __syncthreads();
}

// the fractions of a tile's rows into tl [16] (LDS); ends on a barrier
__device__ void iqn_load_taus(const IqnArgs& c, long long e0, int rows, float* tl) {
    if (threadIdx.x < TR) tl[threadIdx.x] = (int)threadIdx.x < rows ? c.taus[e0 + threadIdx.x] : 0.f;
    __syncthreads();
}

__global__ __launch_bounds__(256) void iqn_fwd_kernel(AcnetArgs p, IqnArgs c) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float ct[TR * LC];
    __shared__ __attribute__((aligned(16))) float ot[TR * LA];
    __shared__ float tl[TR];
    const long long e0 = (long long)blockIdx.x * TR;
    const int rows = p.B - e0 < TR ? (int)(p.B - e0) : TR;
    iqn_load_taus(c, e0, rows, tl);
    iqn_fwd_tile(p, c, e0, rows, tl, buf, ct, ot);
    const int A = p.A, N = c.N;
    for (int e = threadIdx.x; e < rows * A; e += blockDim.x) {
        const int r = e / A, a = e - r * A;
        const long long b = (e0 + r) / N, s = (e0 + r) - b * N;
        c.theta[(b * A + a) * N + s] = ot[r * LA + a];
    }
}

__global__ __launch_bounds__(256) void iqn_q_kernel(const float* __restrict__ theta, long long total, int N, float* __restrict__ q) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) q[e] = serial_mean(theta + e * N, N);
}

// One workgroup per batch row.  p.B is the number of expanded rows, c.Bb the grid.  FQF (include/ocrl_hip_fqf.h: ocrl_fqf_act): c.taus is
// [Bb, N + 1], the proposed fractions' boundaries; sample s sits at their midpoint and q is the fold of fqf.h weighted by the intervals.
template <bool FQF>
__global__ __launch_bounds__(256) void iqn_act_kernel(AcnetArgs p, IqnArgs c, DqnActArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float ct[TR * LC];
    __shared__ __attribute__((aligned(16))) float ot[TR * LA];
    __shared__ float tl[TR];
    __shared__ float qs[ACNET_MAX_ACTIONS];
    const long long row = blockIdx.x;
    const int A = p.A, N = c.N, tid = threadIdx.x;
    if (tid < A) qs[tid] = 0.f;
    for (int s0 = 0; s0 < N; s0 += TR) {
        const int rows = N - s0 < TR ? N - s0 : TR;
        const long long e0 = row * N + s0;
        if (tid < TR) {
            float t = 0.f;
            if (FQF) {
                if (tid < rows) t = fqf_tau_hat(c.taus[row * (N + 1) + s0 + tid], c.taus[row * (N + 1) + s0 + tid + 1]);
            } else if (tid < rows) {
                t = c.taus ? c.taus[e0 + tid] : iqn_tau(s.seed, s.row_offset + (unsigned long long)row, s0 + tid);
            }
            tl[tid] = t;
        }
        __syncthreads();
        iqn_fwd_tile(p, c, e0, rows, tl, buf, ct, ot);
        if (tid < A) {                                  // thread a: the serial sum over s goes on where the last tile left it
            float acc = qs[tid];
            if (FQF) {
                const float* bt = c.taus + row * (N + 1) + s0;
                for (int r = 0; r < rows; ++r) acc = fqf_q_term(acc, bt[r], bt[r + 1], ot[r * LA + tid]);
            } else {
                for (int r = 0; r < rows; ++r) acc += ot[r * LA + tid];
            }
            qs[tid] = acc;
        }
        __syncthreads();
    }
    if (tid < A) {
        const float q = FQF ? qs[tid] : qs[tid] * (1.f / (float)N);
        qs[tid] = q;
        if (c.q) c.q[row * A + tid] = q;
    }
    __syncthreads();
    if (!tid) eps_greedy(qs, A, row, s);
}

// Backward of one tile from theta's cotangent in ot (LDS), with the cosines in ct and z in the third tile of buf: the output Linear and
// the chain into dz (bwd_trunk), dz * phi to the workspace, dphi = dz * features in place, the embedding's backward.
__device__ void iqn_bwd_tile(const AcnetArgs& p, const IqnArgs& c, long long e0, int rows, bool first, float* buf, float* ct, float* ot) {
    float* slab = p.slab + (long long)blockIdx.x * p.slab_stride;
    const int nl = p.n[1], F = p.dim[0][0];
    const int Kl = nl ? p.dim[1][nl - 1] : F;
    float *g0 = buf, *g1 = buf + TR * LD, *zt = buf + 2 * TR * LD;
    const Src lat = nl ? Src{p.saved[1][nl - 1] + e0 * Kl, Kl, rows, false} : lsrc(zt);
    lin_bwd_tile(ot, LA, nullptr, 0, lat, p.wa, Kl, p.A, slab + p.off_wa, slab + p.off_ba, first, Dst{g0, LD, TR}, false, rows);
    float* cur = bwd_trunk(p, 1, g0, g0, g1, lsrc(zt), F, nullptr, false, slab, first, e0, rows);       // dz: layer 0's dx stays in LDS
    const float* phi = p.saved[0][0] + e0 * F;
    for (int e = threadIdx.x; e < rows * F; e += blockDim.x) {      // rows past `rows`: lin_bwd_tile reads them as 0
        const int r = e / F, j = e - r * F;
        const float dz = cur[r * LD + j];
        if (c.dzphi) c.dzphi[(e0 + r) * F + j] = dz * phi[(long long)r * F + j];
        cur[r * LD + j] = dz * c.feat[((e0 + r) / c.N) * F + j];
    }
    __syncthreads();
    lin_bwd_tile(cur, LD, phi, 1, Src{ct, LC, TR, true}, p.w[0][0], c.C, F, slab + p.off_w[0][0], slab + p.off_b[0][0], first,
                 Dst{nullptr, 0, 0}, false, rows);
}

__global__ __launch_bounds__(256) void iqn_bwd_kernel(AcnetArgs p, IqnArgs c) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float ct[TR * LC];
    __shared__ __attribute__((aligned(16))) float ot[TR * LA];
    __shared__ float tl[TR];
    const int A = p.A, N = c.N, F = p.dim[0][0];
    float* zt = buf + 2 * TR * LD;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long e0 = (long long)tile * TR;
        const int rows = p.B - e0 < TR ? (int)(p.B - e0) : TR;
        iqn_load_taus(c, e0, rows, tl);
        iqn_cos_tile(c, rows, tl, ct);
        for (int e = threadIdx.x; e < TR * A; e += blockDim.x) {
            const int r = e / A, a = e - r * A;
            float v = 0.f;
            if (r < rows) {
                const long long b = (e0 + r) / N, s = (e0 + r) - b * N;
                v = c.dquantiles[(b * A + a) * N + s];
            }
            ot[r * LA + a] = v;
        }
        for (int e = threadIdx.x; e < TR * F; e += blockDim.x) {    // phi of the forward, then z as the forward formed it
            const int r = e / F, j = e - r * F;
            zt[r * LD + j] = r < rows ? p.saved[0][0][(e0 + r) * F + j] : 0.f;
        }
        __syncthreads();
        iqn_gate_tile(c, F, e0, rows, zt);
        iqn_bwd_tile(p, c, e0, rows, tile == (int)blockIdx.x, buf, ct, ot);
        __syncthreads();
    }
}

// dfeatures of the batch rows b0 .. b0 + rows: one thread per (b, j), the sum over s serial
__device__ void iqn_dx_rows(const IqnArgs& c, int F, long long b0, int rows) {
    const int N = c.N;
    for (int e = threadIdx.x; e < rows * F; e += blockDim.x) {
        const int r = e / F, j = e - r * F;
        const float* src = c.dzphi + (b0 + r) * N * F + j;
        float s = 0.f;
        for (int i = 0; i < N; ++i) s += src[(long long)i * F];
        c.dfeat[(b0 + r) * F + j] = s;
    }
}

__global__ __launch_bounds__(256) void iqn_dx_kernel(IqnArgs c, int F) {
    const long long b0 = (long long)blockIdx.x * TR;
    iqn_dx_rows(c, F, b0, c.Bb - b0 < TR ? (int)(c.Bb - b0) : TR);
}

// T_j of a row
__device__ __forceinline__ float iqn_td_target(const IqnTdArgs& s, const TdRow& t, int A, long long row, int j) {
    return t.done ? t.rw : fmaf(t.g, s.next_quantiles[(row * A + t.star) * s.Np + j], t.rw);
}

// The TD step of one tile after its forward.  Replaces theta in ot by dL/dtheta (L = the mean loss) and leaves the rows' partial losses
// and the theta of the action taken in the workspace.  T is the first chain tile: row lb holds the T of batch row e0 / N + lb.
__device__ void iqn_td_rows(const AcnetArgs& p, const IqnArgs& c, const IqnTdArgs& s, long long e0, int rows, const float* tl, float* buf,
                            float* ot, TdRow* tr) {
    const int A = p.A, N = c.N, Np = s.Np, tid = threadIdx.x;
    const float invNp = 1.f / (float)Np, kappa = s.kappa;
    const long long b0 = e0 / N;
    const int nb = (int)((e0 + rows - 1) / N - b0) + 1;             // batch rows present in the tile: at most 16
    float* T = buf;
    if (tid < nb) tr[tid] = td_row(s.row, A, b0 + tid);
    __syncthreads();
    for (int e = tid; e < nb * Np; e += blockDim.x) {
        const int lb = e / Np, j = e - lb * Np;
        T[lb * LD + j] = iqn_td_target(s, tr[lb], A, b0 + lb, j);
    }
    __syncthreads();
    if (tid < TR) {                                     // thread r: the pairs (i, j) of expanded row r in ascending j, loss and cotangent together
        const int r = tid;
        float* th = ot + r * LA;
        int act = -1;
        float d = 0.f;
        if (r < rows) {
            const int lb = (int)((e0 + r) / N - b0);
            act = tr[lb].act;
            const float x = th[act], tau = tl[r];
            const float* Tr = T + lb * LD;
            float ls = 0.f, gs = 0.f;
            for (int j = 0; j < Np; ++j) qhuber_pair(Tr[j], x, tau, kappa, ls, gs);
            s.part[e0 + r] = invNp * ls;
            s.tha[e0 + r] = x;
            d = -(tr[lb].wt / (float)c.Bb) * invNp * gs;
        }
        for (int a = 0; a < A; ++a) th[a] = a == act ? d : 0.f;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void iqn_td_kernel(AcnetArgs p, IqnArgs c, IqnTdArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float ct[TR * LC];
    __shared__ __attribute__((aligned(16))) float ot[TR * LA];
    __shared__ float tl[TR];
    __shared__ TdRow tr[TR];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long e0 = (long long)tile * TR;
        const int rows = p.B - e0 < TR ? (int)(p.B - e0) : TR;
        iqn_load_taus(c, e0, rows, tl);
        iqn_fwd_tile(p, c, e0, rows, tl, buf, ct, ot);
        iqn_td_rows(p, c, s, e0, rows, tl, buf, ot, tr);
        iqn_bwd_tile(p, c, e0, rows, tile == (int)blockIdx.x, buf, ct, ot);
        __syncthreads();
    }
}

// Workgroup g walks the groups g, g + G, ... of 16 batch rows (G = gridDim.x <= ACNET_MAX_SLABS): thread r folds row r's terms over i.
__global__ __launch_bounds__(256) void iqn_td_fold_kernel(IqnArgs c, IqnTdArgs s, int A, int F, int ngroups, float* scal_slab) {
    __shared__ float rs[TR][3];
    const int N = c.N, Np = s.Np;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long b0 = (long long)grp * TR;
        const int rows = c.Bb - b0 < TR ? (int)(c.Bb - b0) : TR;
        if (threadIdx.x < TR) {
            const int r = threadIdx.x;
            float wl = 0.f, q = 0.f, tm = 0.f;
            if (r < rows) {
                const long long row = b0 + r;
                const TdRow t = td_row(s.row, A, row);
                float ql = 0.f;
                for (int i = 0; i < N; ++i) ql += s.part[row * N + i];
                q = serial_mean(s.tha + row * N, N);
                float ts = 0.f;
                for (int j = 0; j < Np; ++j) ts += iqn_td_target(s, t, A, row, j);
                tm = ts * (1.f / (float)Np);
                if (s.row.row_loss) s.row.row_loss[row] = ql;
                wl = t.wt * ql;
            }
            rs[r][0] = wl; rs[r][1] = q; rs[r][2] = tm;
        }
        if (c.dfeat) iqn_dx_rows(c, F, b0, rows);
        __syncthreads();
        tile_scalars<3>(rs, grp == (int)blockIdx.x, scal_slab);
    }
}

}  // namespace

int iqn_taus_launch(unsigned long long seed, unsigned long long row_offset, int B, int N, float* out, hipStream_t st) {
    const long long total = (long long)B * N;
    hipLaunchKernelGGL(iqn_taus_kernel, GRID1D(total), 0, st, seed, row_offset, total, N, out);
    OCRL_CHECK_LAUNCH("iqn_taus");
    return 0;
}
int iqn_fwd_launch(const AcnetArgs& a, const IqnArgs& c, hipStream_t st) {
    hipLaunchKernelGGL(iqn_fwd_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a, c);
    OCRL_CHECK_LAUNCH("iqn_fwd");
    if (c.q) {
        const long long total = (long long)c.Bb * a.A;
        hipLaunchKernelGGL(iqn_q_kernel, GRID1D(total), 0, st, (const float*)c.theta, total, c.N, c.q);
        OCRL_CHECK_LAUNCH("iqn_q");
    }
    return 0;
}
int iqn_act_launch(const AcnetArgs& a, const IqnArgs& c, const DqnActArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(iqn_act_kernel<false>, dim3(c.Bb), dim3(256), 0, st, a, c, s);
    OCRL_CHECK_LAUNCH("iqn_act");
    return 0;
}
int iqn_act_fqf_launch(const AcnetArgs& a, const IqnArgs& c, const DqnActArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(iqn_act_kernel<true>, dim3(c.Bb), dim3(256), 0, st, a, c, s);
    OCRL_CHECK_LAUNCH("fqf_act");
    return 0;
}
int iqn_bwd_launch(const AcnetArgs& a, const IqnArgs& c, hipStream_t st) {
    hipLaunchKernelGGL(iqn_bwd_kernel, dim3(a.S), dim3(256), 0, st, a, c);
    OCRL_CHECK_LAUNCH("iqn_bwd");
    if (c.dfeat) {
        hipLaunchKernelGGL(iqn_dx_kernel, dim3(cdiv(c.Bb, TR)), dim3(256), 0, st, c, a.dim[0][0]);
        OCRL_CHECK_LAUNCH("iqn_dx");
    }
    return 0;
}
int iqn_td_launch(const AcnetArgs& a, const IqnArgs& c, const IqnTdArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(iqn_td_kernel, dim3(a.S), dim3(256), 0, st, a, c, s);
    OCRL_CHECK_LAUNCH("iqn_td");
    const int ngroups = cdiv(c.Bb, TR);
    hipLaunchKernelGGL(iqn_td_fold_kernel, dim3(ngroups < ACNET_MAX_SLABS ? ngroups : ACNET_MAX_SLABS), dim3(256), 0, st, c, s, a.A, a.dim[0][0],
                       ngroups, a.scal_slab);
    OCRL_CHECK_LAUNCH("iqn_td_fold");
    return 0;
}
