// The per-object MLP of the ground-truth-state encoder (ocrs/gt/gt_module.py:14-27: [Linear, ReLU?] x 1..4 on the rows of the state),
// one launch forward and one down the chain backward.  The rows are M = B (hi + 1), a few to a few thousand, of width 5: a workgroup
// takes GT_TM rows, keeps their activations in two LDS buffers that swap roles from layer to layer and streams each weight
// (at most 256 x 256, from L2) through a 16-row LDS stage.  fp32 FMAs on the vector pipe; no atomics: every output has one owner.
#include "gt.h"

namespace {
constexpr int LD = 260;             // floats between two rows of an activation buffer: 256 + 4 keeps float4 reads aligned
constexpr int JT = 16;              // rows of the weight stage
constexpr int BLD = 257;            // floats between two rows of the stage: odd, so the transposing fill spreads over the banks

// stage[jj][c] = B[j0 + jj][c], c < C, where B [J, C] is W itself (TRANS false: W is [J, C]) or its transpose (TRANS true: W is
// [C, J], the torch layout of a forward product); rows at or past J are zero, so nothing is read beyond the weight
template <bool TRANS>
__device__ __forceinline__ void stage_fill(const float* __restrict__ W, int J, int C, int j0, float* __restrict__ stage) {
    for (int i = threadIdx.x; i < C * JT; i += 256) {
        const int c = TRANS ? i / JT : i % C, jj = TRANS ? i % JT : i / C;
        const int j = j0 + jj;
        float v = 0.f;
        if (j < J) v = TRANS ? W[(size_t)c * J + j] : W[(size_t)j * C + c];
        stage[jj * BLD + c] = v;
    }
}

// acc[q][u] = sum_j in[rq * 4 + u][j] * B[j][c] for the thread's items i = threadIdx.x + 256 q < 4 C, c = i % C, rq = i / C: a column
// of four rows.  `in` holds zeros (or finite values) in columns J .. pad4(J) - 1.  Begins with a barrier, so what the caller wrote to
// `in` before the call is seen; ends without one.
template <bool TRANS>
__device__ __forceinline__ void tile_product(const float* __restrict__ in, const float* __restrict__ W, int J, int C, float* __restrict__ stage,
                                             float (&acc)[4][4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[q][u] = 0.f;
    const int Jp = (J + 3) & ~3;
    for (int j0 = 0; j0 < Jp; j0 += JT) {
        __syncthreads();
        stage_fill<TRANS>(W, J, C, j0, stage);
        __syncthreads();
        const int jn = Jp - j0 < JT ? Jp - j0 : JT;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = threadIdx.x + 256 * q;
            if (i >= 4 * C) break;
            const int c = i % C, rq = i / C;
            for (int jj = 0; jj < jn; jj += 4) {
                const float b0 = stage[jj * BLD + c], b1 = stage[(jj + 1) * BLD + c], b2 = stage[(jj + 2) * BLD + c], b3 = stage[(jj + 3) * BLD + c];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 a = *reinterpret_cast<const float4*>(in + (rq * 4 + u) * LD + j0 + jj);
                    acc[q][u] = fmaf(a.w, b3, fmaf(a.z, b2, fmaf(a.y, b1, fmaf(a.x, b0, acc[q][u]))));
                }
            }
        }
    }
}

// rows row0 .. row0 + GT_TM - 1 of src [M, K] into buf, zero in the pad columns K .. pad4(K) - 1 and in the rows at or past M
__device__ __forceinline__ void tile_load(const float* __restrict__ src, int M, int K, int row0, float* __restrict__ buf) {
    const int Kp = (K + 3) & ~3;
    for (int i = threadIdx.x; i < GT_TM * Kp; i += 256) {
        const int r = i / Kp, k = i % Kp;
        buf[r * LD + k] = (row0 + r < M && k < K) ? src[(size_t)(row0 + r) * K + k] : 0.f;
    }
}

__global__ __launch_bounds__(256) void gt_mlp_fwd_kernel(GtFwdArgs a) {
    __shared__ __align__(16) float act[2][GT_TM * LD];
    __shared__ float stage[JT * BLD];
    const int row0 = blockIdx.x * GT_TM;
    tile_load(a.x, a.M, a.D, row0, act[0]);
    int cur = 0, J = a.D;
    float acc[4][4];
    for (int l = 0; l < a.nl; ++l) {
        const int C = a.dims[l];
        tile_product<true>(act[cur], a.w[l], J, C, stage, acc);
        float* nxt = act[cur ^ 1];                    // last read by the layer before: every thread has passed this layer's barriers since
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = threadIdx.x + 256 * q;
            if (i >= 4 * C) break;
            const int c = i % C, rq = i / C;
            const float bias = a.b[l][c];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float v = acc[q][u] + bias;
                if (a.relu[l]) v = v < 0.f ? 0.f : v;
                const int r = rq * 4 + u;
                nxt[r * LD + c] = v;
                if (row0 + r < a.M) {
                    const size_t o = (size_t)(row0 + r) * C + c;
                    if (a.h[l]) a.h[l][o] = v;
                    if (l == a.nl - 1) a.out[o] = v;
                }
            }
        }
        cur ^= 1;
        J = C;
    }
}

// One workgroup per slab of tiles, the tiles in order.  Per tile and layer, from the last one down: the tile's dz^T x and column sums of
// dz are added to the slab's weight-gradient partial (the first tile writes it, so it needs no zeroing; an element is always the same
// thread's), then dz W, masked by the saved output of the layer below, becomes that layer's dz in the buffer its input was read from.
__global__ __launch_bounds__(256) void gt_mlp_bwd_kernel(GtBwdArgs a, int tiles) {
    __shared__ __align__(16) float buf[2][GT_TM * LD];
    __shared__ float stage[JT * BLD];
    const int t0 = blockIdx.x * a.per_slab, t1 = t0 + a.per_slab < tiles ? t0 + a.per_slab : tiles;
    const long long slab_off = (long long)blockIdx.x * a.slab_stride;
    float acc[4][4];
    for (int tile = t0; tile < t1; ++tile) {
        const int row0 = tile * GT_TM;
        const bool first = tile == t0;
        __syncthreads();                              // the tile before is read no more
        {
            const int C = a.dims[a.nl - 1];
            const float* hl = a.h[a.nl - 1];
            for (int i = threadIdx.x; i < GT_TM * C; i += 256) {
                const int r = i / C, c = i % C;
                float v = 0.f;
                if (row0 + r < a.M) {
                    const size_t o = (size_t)(row0 + r) * C + c;
                    v = a.dout[o];
                    if (a.relu[a.nl - 1] && !(hl[o] > 0.f)) v = 0.f;
                }
                buf[0][r * LD + c] = v;
            }
        }
        int cur = 0;
        for (int l = a.nl - 1; l >= 0; --l) {
            const int N = a.dims[l], K = l ? a.dims[l - 1] : a.D, K4 = (K + 3) >> 2;
            const float* dz = buf[cur];
            float* xs = buf[cur ^ 1];
            __syncthreads();                          // xs was the dz of the layer above: its product is over
            tile_load(l ? a.h[l - 1] : a.x, a.M, K, row0, xs);
            __syncthreads();
            float* dW = a.dw[l] + slab_off;
            float* dB = a.db[l] + slab_off;
            for (int i = threadIdx.x; i < N * K4; i += 256) {
                const int n = i / K4, k = (i % K4) * 4;
                float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < GT_TM; ++r) {
                    const float d = dz[r * LD + n];
                    const float4 xv = *reinterpret_cast<const float4*>(xs + r * LD + k);
                    s[0] = fmaf(d, xv.x, s[0]); s[1] = fmaf(d, xv.y, s[1]); s[2] = fmaf(d, xv.z, s[2]); s[3] = fmaf(d, xv.w, s[3]);
                }
                float* p = dW + (size_t)n * K + k;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u < K) p[u] = first ? s[u] : p[u] + s[u];
            }
            for (int n = threadIdx.x; n < N; n += 256) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < GT_TM; ++r) s += dz[r * LD + n];
                dB[n] = first ? s : dB[n] + s;
            }
            if (l == 0 && !a.dx) break;
            tile_product<false>(dz, a.w[l], N, K, stage, acc);     // its first barrier ends the reads of xs above
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = threadIdx.x + 256 * q;
                if (i >= 4 * K) break;
                const int c = i % K, rq = i / K;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = rq * 4 + u;
                    float v = acc[q][u];
                    if (l) {
                        if (a.relu[l - 1] && !(xs[r * LD + c] > 0.f)) v = 0.f;
                        xs[r * LD + c] = v;               // this thread alone reads and writes the element
                    } else if (row0 + r < a.M) {
                        a.dx[(size_t)(row0 + r) * K + c] = v;
                    }
                }
            }
            cur ^= 1;
        }
    }
}

// dst[e] = part[0][e] + part[1][e] + .. in slab order, one thread per float of a slab's partial
__global__ __launch_bounds__(256) void gt_mlp_reduce_kernel(GtReduceArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.P) return;
    float s = a.part[e];
    for (int sl = 1; sl < a.slabs; ++sl) s += a.part[(size_t)sl * a.P + e];
    int begin = 0;
    for (int i = 0; i < a.n; ++i) {
        if (e < a.end[i]) {
            a.dst[i][e - begin] = s;
            return;
        }
        begin = a.end[i];
    }
}
}  // namespace

int gt_mlp_fwd_launch(const GtFwdArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(gt_mlp_fwd_kernel, dim3(cdiv(a.M, GT_TM)), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("gt_mlp_fwd");
    return 0;
}
int gt_mlp_bwd_launch(const GtBwdArgs& a, int slabs, hipStream_t st) {
    hipLaunchKernelGGL(gt_mlp_bwd_kernel, dim3(slabs), dim3(256), 0, st, a, cdiv(a.M, GT_TM));
    OCRL_CHECK_LAUNCH("gt_mlp_bwd");
    return 0;
}
int gt_mlp_reduce_launch(const GtReduceArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(gt_mlp_reduce_kernel, GRID1D(a.P), 0, st, a);
    OCRL_CHECK_LAUNCH("gt_mlp_reduce");
    return 0;
}
