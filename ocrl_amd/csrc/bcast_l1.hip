// First layer of a spatial-broadcast decoder without the broadcast tensor, shared by the Slot-Attention configuration of SLATE
// (5x5, ReLU: bcdec.hip, ocrs/common/models.py:110-141) and by IODINE (3x3, ELU: iodine.hip, iodine_module.py:438-470).
//
// The KS x KS "same" convolution runs on  s[bk,:] + pos[y,x,:]  (spatially constant per slot plus a batch-independent map), and a
// convolution is linear, so
//     c1[bk,y,x,:] = act( P1[y,x,:] + T[bk, class(y,x), :] [+ b] )
// P1 = conv(pos) is the position term; T sums the per-slot tap products  M[bk,tap,:] = W_tap s  (one small GEMM, the caller's) over
// the taps that stay inside the image for the pixel's border class: KS row classes x KS column classes.  The backward sums the
// pre-activation gradient per class (row partials, then the rows of a row class) and transposes the class sum back onto the taps.
// Every reduction has a fixed order (no float atomics): the results are bitwise reproducible.
// Templated on KS in {5, 3}, R = KS / 2; the channel count is 64.
#include "common.h"
#include "kernels.h"

// border class of a coordinate: 0..R-1 the first R rows/columns, R the interior, R+1..2R the last R
template <int R> __device__ inline int l1_class(int i, int S) { return i < R ? i : (i >= S - R ? 2 * R - (S - 1 - i) : R); }
// tap offset k (0..2R) stays inside the image for class c
template <int R> __device__ inline bool l1_valid(int c, int k) { return (c >= R || k >= R - c) && (c <= R || k <= 3 * R - c); }

// Position features of a pixel: NF values f_j, of which the first NW carry a weight per (tap, co) in the position term.  ROUNDED is
// the set of features (bit j) whose product in l1_tap_sums is rounded before it is added; the others go through one FMA.
// SLATE: the four ramps of the position grid [north, south, west, east] and 1 (the position embedding's bias, folded per tap)
struct RampFeat {
    static constexpr int NF = 5, NW = 5;
    static constexpr unsigned ROUNDED = 0;
    __device__ void operator()(int y, int x, int S, float (&f)[NF]) const {
        const float east = S > 1 ? (float)x / (float)(S - 1) : 0.f, south = S > 1 ? (float)y / (float)(S - 1) : 0.f;
        f[0] = 1.f - south; f[1] = south; f[2] = 1.f - east; f[3] = east; f[4] = 1.f;
    }
};
// IODINE: the two coordinate channels (xx, yy) in [-1, 1]; the trailing 1 only collects the bias gradient.  The yy product is rounded
// on its own: that is how this sum was first compiled (the packed add took the yy and bias accumulators together), and the weight
// gradients are pinned bit for bit, so the rounding is now written down instead of left to the vectoriser.
struct LinFeat {
    static constexpr int NF = 3, NW = 2;
    static constexpr unsigned ROUNDED = 1u << 1;
    __device__ void operator()(int y, int x, int S, float (&f)[NF]) const { f[0] = io_lin(x, S); f[1] = io_lin(y, S); f[2] = 1.f; }
};

// P1[y][x][co] = b0[co] + sum over taps inside the image of W[tap][co][0..NW) . f(y+dy, x+dx)      (b0 nullable)
template <int KS, typename F>
__global__ void bcast_l1_pos_kernel(const float* __restrict__ W, const float* __restrict__ b0, float* __restrict__ P1, int S) {
    constexpr int R = KS / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * S * 64) return;
    const int co = i & 63, x = (i >> 6) % S, y = (i >> 6) / S;
    float a = b0 ? b0[co] : 0.f;
    for (int ky = 0; ky < KS; ++ky)
        for (int kx = 0; kx < KS; ++kx) {
            const int yy = y + ky - R, xx = x + kx - R;
            if (yy < 0 || yy >= S || xx < 0 || xx >= S) continue;
            float f[F::NF];
            F()(yy, xx, S, f);
            const float* w = W + ((ky * KS + kx) * 64 + co) * F::NW;
            float t = w[0] * f[0];
#pragma unroll
            for (int j = 1; j < F::NW; ++j) t += w[j] * f[j];
            a += t;
        }
    P1[i] = a;
}

// forward: T[bk][cls][co] = sum_{taps valid in cls} M[bk][tap][co];  backward (transpose): dM[bk][tap][co] = sum_{cls valid for tap} dT
template <int KS>
__global__ void bcast_l1_class_sum_kernel(const float* __restrict__ in, float* __restrict__ out, long long BK, int forward) {
    constexpr int R = KS / 2, NC = KS * KS;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK * NC * 64) return;
    const int co = i & 63, a = (i >> 6) % NC;
    const long long bk = i / (NC * 64);
    float s = 0.f;
    for (int b = 0; b < NC; ++b) {
        const int cls = forward ? a : b, tap = forward ? b : a;
        if (l1_valid<R>(cls / KS, tap / KS) && l1_valid<R>(cls % KS, tap % KS)) s += in[(bk * NC + b) * 64 + co];
    }
    out[i] = s;
}

template <int ACT> __device__ inline float l1_act(float v) { return ACT == BCAST_L1_ELU ? elu_(v) : fmaxf(v, 0.f); }

// c1[bk][y][x][co] = act((P1[y][x][co] + T[bk][cls(y,x)][co]) + b1[co])      (one thread per float4; b1 nullable)
template <int KS, int ACT>
__global__ void bcast_l1_fwd_kernel(const float* __restrict__ P1, const float* __restrict__ T, const float* __restrict__ b1,
                                    float* __restrict__ c1, long long BK, int S) {
    constexpr int R = KS / 2, NC = KS * KS;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK * S * S * 16) return;
    const int c4 = i & 15;
    const long long pix = (i >> 4) % ((long long)S * S), bk = (i >> 4) / ((long long)S * S);
    const int x = pix % S, y = pix / S;
    const int cls = l1_class<R>(y, S) * KS + l1_class<R>(x, S);
    const float4 p = *reinterpret_cast<const float4*>(P1 + pix * 64 + c4 * 4);
    const float4 t = *reinterpret_cast<const float4*>(T + (bk * NC + cls) * 64 + c4 * 4);
    float4 v = make_float4(p.x + t.x, p.y + t.y, p.z + t.z, p.w + t.w);
    if (b1) {
        const float4 b = *reinterpret_cast<const float4*>(b1 + c4 * 4);
        v = make_float4(v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w);
    }
    *reinterpret_cast<float4*>(c1 + i * 4) = make_float4(l1_act<ACT>(v.x), l1_act<ACT>(v.y), l1_act<ACT>(v.z), l1_act<ACT>(v.w));
}

// rowpart[bk][y][k][co] = sum over the pixels of row y in column class k of g[bk][y][x][co]      (one block per (bk, y), threads
// (co, x mod 4); the accumulators stay in registers through the select form: a dynamically indexed array would go to scratch)
template <int KS>
__global__ __launch_bounds__(256) void bcast_l1_bwd_kernel(const float* __restrict__ g, float* __restrict__ rowpart, int S) {
    constexpr int R = KS / 2;
    __shared__ float red[4][KS][64];
    const int y = blockIdx.x % S;
    const long long bk = blockIdx.x / S;
    const int co = threadIdx.x & 63, part = threadIdx.x >> 6;
    float a[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) a[k] = 0.f;
    const float* row = g + ((bk * S + y) * S) * 64 + co;
    for (int x = part; x < S; x += 4) {
        const float v = row[(size_t)x * 64];
        const int cls = l1_class<R>(x, S);
#pragma unroll
        for (int k = 0; k < KS; ++k) a[k] += (cls == k) ? v : 0.f;
    }
#pragma unroll
    for (int k = 0; k < KS; ++k) red[part][k][co] = a[k];
    __syncthreads();
    if (part == 0) {
#pragma unroll
        for (int k = 0; k < KS; ++k) rowpart[((bk * S + y) * KS + k) * 64 + co] = (red[0][k][co] + red[1][k][co]) + (red[2][k][co] + red[3][k][co]);
    }
}
// dT[bk][rc*KS+k][co] = sum over the rows y of row class rc, in row order, of rowpart[bk][y][k][co]
template <int KS>
__global__ void bcast_l1_reduce_kernel(const float* __restrict__ rowpart, float* __restrict__ dT, long long n, int S) {
    constexpr int R = KS / 2, NC = KS * KS;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // over [BK][NC][64]
    if (i >= n) return;
    const int co = i & 63, cls = (i >> 6) % NC;
    const long long bk = i / (NC * 64);
    const int rc = cls / KS, k = cls - rc * KS;
    const int y0 = rc <= R ? rc : S - 2 * R - 1 + rc, y1 = rc == R ? S - R : y0 + 1;
    float a = 0.f;
    for (int y = y0; y < y1; ++y) a += rowpart[((bk * S + y) * KS + k) * 64 + co];
    dT[i] = a;
}

// a + v * f with the product rounded on its own: never contracted into an FMA
__device__ inline float l1_mul_add(float a, float v, float f) {
#pragma clang fp contract(off)
    return a + v * f;
}

// s[j] = sum over the pixels (y, x) where tap blockIdx.x is inside the image of G[y][x][co] * f_j(y+dy, x+dx),  co = threadIdx.x & 63
// (one block of 256 threads per tap, G = the pre-activation gradient summed over bk; every thread returns its channel's sums)
template <int KS, typename F>
__device__ inline void l1_tap_sums(const float* __restrict__ G, int S, float (&s)[F::NF]) {
    constexpr int R = KS / 2, NF = F::NF;
    __shared__ float red[4][NF][64];
    const int tap = blockIdx.x, ky = tap / KS, kx = tap % KS;
    const int co = threadIdx.x & 63, part = threadIdx.x >> 6;
    float a[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) a[j] = 0.f;
    for (int pix = part; pix < S * S; pix += 4) {
        const int x = pix % S, y = pix / S;
        const int yy = y + ky - R, xx = x + kx - R;
        if (yy < 0 || yy >= S || xx < 0 || xx >= S) continue;
        float f[NF];
        F()(yy, xx, S, f);
        const float v = G[(size_t)pix * 64 + co];
#pragma unroll
        for (int j = 0; j < NF; ++j) a[j] = (F::ROUNDED >> j & 1) ? l1_mul_add(a[j], v, f[j]) : __builtin_fmaf(v, f[j], a[j]);
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) red[part][j][co] = a[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NF; ++j) s[j] = red[0][j][co] + red[1][j][co] + red[2][j][co] + red[3][j][co];
}

// SLATE: dWc[tap][co][j] = sum_{y,x : tap inside} G[y][x][co] * (grid_j(y+dy, x+dx) | 1)
__global__ __launch_bounds__(256) void bc_posconv_bwd_kernel(const float* __restrict__ G, float* __restrict__ dWc, int S) {
    float s[5];
    l1_tap_sums<5, RampFeat>(G, S, s);
    if (threadIdx.x < 64)
#pragma unroll
        for (int j = 0; j < 5; ++j) dWc[(blockIdx.x * 64 + threadIdx.x) * 5 + j] = s[j];
}
// IODINE: weight gradient of layer 1 from the accumulated pieces: dW1[co][ci<L][tap] = dW1r[tap][co][ci];
// dW1[co][L+j][tap] = sum_{pixels where tap is inside} G[y][x][co] * coord_j;  db1[co] = sum G
__global__ __launch_bounds__(256) void io_w1_grad_kernel(const float* __restrict__ dW1r, const float* __restrict__ G, float* __restrict__ dW1,
                                                         float* __restrict__ db1, int S, int L) {
    const int tap = blockIdx.x, co = threadIdx.x;
    float s[3];
    l1_tap_sums<3, LinFeat>(G, S, s);
    if (co < 64) {
        dW1[((size_t)co * (L + 2) + L) * 9 + tap] = s[0];
        dW1[((size_t)co * (L + 2) + L + 1) * 9 + tap] = s[1];
        if (tap == 4) db1[co] = s[2];
    }
    for (int i = threadIdx.x; i < 64 * L; i += 256) {
        const int ci = i % L, c2 = i / L;
        dW1[((size_t)c2 * (L + 2) + ci) * 9 + tap] = dW1r[((size_t)tap * 64 + c2) * L + ci];
    }
}

// ================================================================== launchers
int bc_posconv_launch(const float* Wc, float* P1, int S, hipStream_t st) {
    OCRL_REQUIRE(S >= 5, "broadcast decoder needs obs_size >= 5");
    hipLaunchKernelGGL((bcast_l1_pos_kernel<5, RampFeat>), GRID1D(S * S * 64), 0, st, Wc, nullptr, P1, S);
    OCRL_CHECK_LAUNCH("bc_posconv");
    return 0;
}
int io_p1_launch(const float* Wxy, const float* b1, float* P1, int S, hipStream_t st) {
    hipLaunchKernelGGL((bcast_l1_pos_kernel<3, LinFeat>), GRID1D(S * S * 64), 0, st, Wxy, b1, P1, S);
    OCRL_CHECK_LAUNCH("io_p1");
    return 0;
}
int bcast_l1_class_sum_launch(const float* in, float* out, long long BK, int ks, int forward, hipStream_t st) {
    OCRL_REQUIRE(ks == 5 || ks == 3, "bcast_l1: kernel size 5 or 3");
    if (ks == 5) hipLaunchKernelGGL(bcast_l1_class_sum_kernel<5>, GRID1D(BK * 25 * 64), 0, st, in, out, BK, forward);
    else hipLaunchKernelGGL(bcast_l1_class_sum_kernel<3>, GRID1D(BK * 9 * 64), 0, st, in, out, BK, forward);
    OCRL_CHECK_LAUNCH("bcast_l1_class_sum");
    return 0;
}
int bcast_l1_fwd_launch(const float* P1, const float* T, const float* bias, float* c1, long long BK, int S, int ks, int act, hipStream_t st) {
    OCRL_REQUIRE((ks == 5 && act == BCAST_L1_RELU) || (ks == 3 && act == BCAST_L1_ELU), "bcast_l1: 5x5 with ReLU or 3x3 with ELU");
    OCRL_REQUIRE(S >= ks, "bcast_l1: obs_size %d below the kernel size %d", S, ks);
    if (ks == 5) hipLaunchKernelGGL((bcast_l1_fwd_kernel<5, BCAST_L1_RELU>), GRID1D(BK * S * S * 16), 0, st, P1, T, bias, c1, BK, S);
    else hipLaunchKernelGGL((bcast_l1_fwd_kernel<3, BCAST_L1_ELU>), GRID1D(BK * S * S * 16), 0, st, P1, T, bias, c1, BK, S);
    OCRL_CHECK_LAUNCH("bcast_l1_fwd");
    return 0;
}
size_t bcast_l1_bwd_ws_floats(long long BK, int S, int ks) { return (size_t)BK * S * ks * 64; }
// dT [BK][ks*ks][64] is written (not accumulated); ws: bcast_l1_bwd_ws_floats() floats of scratch
int bcast_l1_bwd_launch(const float* g, float* dT, long long BK, int S, int ks, float* ws, size_t ws_floats, hipStream_t st) {
    OCRL_REQUIRE(ks == 5 || ks == 3, "bcast_l1: kernel size 5 or 3");
    OCRL_REQUIRE(S >= ks && ws && ws_floats >= bcast_l1_bwd_ws_floats(BK, S, ks), "bcast_l1_bwd: obs_size below the kernel size or scratch too small");
    const long long n = BK * ks * ks * 64;
    if (ks == 5) {
        hipLaunchKernelGGL(bcast_l1_bwd_kernel<5>, dim3((unsigned)(BK * S)), dim3(256), 0, st, g, ws, S);
        hipLaunchKernelGGL(bcast_l1_reduce_kernel<5>, GRID1D(n), 0, st, ws, dT, n, S);
    } else {
        hipLaunchKernelGGL(bcast_l1_bwd_kernel<3>, dim3((unsigned)(BK * S)), dim3(256), 0, st, g, ws, S);
        hipLaunchKernelGGL(bcast_l1_reduce_kernel<3>, GRID1D(n), 0, st, ws, dT, n, S);
    }
    OCRL_CHECK_LAUNCH("bcast_l1_bwd");
    return 0;
}
int bc_posconv_bwd_launch(const float* G, float* dWc, int S, hipStream_t st) {
    hipLaunchKernelGGL(bc_posconv_bwd_kernel, dim3(25), dim3(256), 0, st, G, dWc, S);
    OCRL_CHECK_LAUNCH("bc_posconv_bwd");
    return 0;
}
int io_w1_grad_launch(const float* dW1r, const float* G, float* dW1, float* db1, int S, int L, hipStream_t st) {
    hipLaunchKernelGGL(io_w1_grad_kernel, dim3(9), dim3(256), 0, st, dW1r, G, dW1, db1, S, L);
    OCRL_CHECK_LAUNCH("io_w1_grad");
    return 0;
}
