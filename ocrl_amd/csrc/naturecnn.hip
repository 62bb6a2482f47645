// Valid strided convolutions of NatureCNN (ocrs/naturecnn/naturecnn_module.py:29-44): Conv2d(k 8, s 4), Conv2d(k 4, s 2) and
// Conv2d(k 3, s 1), padding 0, every one followed by a ReLU.  Implicit GEMMs on v_mfma_f32_16x16x4_f32: exact fp32 products, fp32
// accumulation, the same arithmetic contract as conv.hip.  A 16 x 32 output tile (two accumulators sharing the A operand) is one
// workgroup whose four waves split its K range and sum their partial tiles through LDS in wave order; the dW partials give one tile to
// each wave.  Operands are gathered straight from global memory: at the shapes of the RL loop (B = 4 .. 256, maps of 15 x 15 and below)
// the whole problem is L2-resident and the cost is launches, not bandwidth.
//
// Maps are addressed through NcMap strides, so one kernel reads the NCHW observation, the [B, G C, H, W] intermediate maps, the
// [G, B, C, OH, OW] last map whose per-module flatten is NCHW (the Linear's input), and the [B, OH OW, C] token map of use_cnn_feat.
// A "group" g is one NatureCNN module of MultipleCNN: its own weights (w[g], b[g]) and its own output channels; the input channels it
// reads start at g * x.sG (x.sG = 0 for the first layer: every module reads the same image, all G modules in one launch).
//
// Weights are read in torch's [COUT, CIN, KS, KS] layout, so the GEMM k index is k = ci KS KS + kh KS + kw; nothing is packed.
//   nc_conv_fwd     Y[m, n] = relu(b[n] + sum_k X(m, k) W[n, k])                     m = (b, oh, ow)  (Y2: optional second copy)
//   nc_conv_bwd     blocks [0, dw_blocks):  partial dW over one slab of the m rows: P[s][g][n][k] = sum_{m in s} dY[m, n] X(m, k),
//                                          with k = K the ones column, so P[..][n][K] is the slab's bias gradient
//                   blocks [dw_blocks, ..): dX[i, ci] = (act[i, ci] > 0) sum_{co, kh, kw} dY[(ih - kh) / S, (iw - kw) / S, co] W[co, ci, kh, kw]
//                                          over the output positions that cover input pixel i (gather form; no atomics)
//   nc_dw_reduce    dW[g][n, k] = sum_s P[s][g][n][k] in slab order (all layers of a backward in one launch)
//   nc_relu_mask    d = dout * (act > 0)
// The VAE (vae_unit.cpp) adds two forms: 2 x 2 stride 2 (its encoder) and 3 x 3 with zero padding 1 (its decoder below 32 x 32; the
// padding taps read nothing, and dX gathers from oh = (ih + PAD - kh) / S).  PAD is a template parameter: the PAD = 0 forms are unchanged.
// Every sum runs in an order fixed by the shapes alone: results are reproducible bit for bit.
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ long long map_off(const NcMap& m, long long b, int g, int c, int h, int w) {
    return b * m.sN + g * m.sG + (long long)c * m.sC + (long long)h * m.sH + (long long)w * m.sW;
}

// sum of the four waves' partial tiles in wave order (fixed: bitwise reproducible); true in wave 0, which holds the sums
__device__ __forceinline__ bool reduce4(f32x4& acc0, f32x4& acc1, int wave, int lane) {
    __shared__ f32x4 red[3][2][64];
    if (wave) { red[wave - 1][0][lane] = acc0; red[wave - 1][1][lane] = acc1; }
    __syncthreads();
    if (wave) return false;
#pragma unroll
    for (int w = 0; w < 3; ++w) { acc0 += red[w][0][lane]; acc1 += red[w][1][lane]; }
    return true;
}

template <int KS, int S, int PAD>
__global__ __launch_bounds__(256) void nc_conv_fwd_kernel(NcFwdArgs p) {
    constexpr int KK = KS * KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int OHW = p.OH * p.OW;
    const long long M = (long long)p.B * OHW;
    const int mtiles = (int)((M + 15) / 16), ntiles = (p.cout + 31) / 32;
    long long t = blockIdx.x;                                          // one tile per workgroup; its 4 waves split K
    const int mt = (int)(t % mtiles); t /= mtiles;
    const int nt = (int)(t % ntiles);
    const int g = (int)(t / ntiles);
    const long long m0 = (long long)mt * 16;
    const int n0 = nt * 32;
    const int K = p.cin * KK;
    const float* __restrict__ W = p.w[g];

    // this lane's A row: output pixel m0 + i
    const long long m = m0 + i;
    const bool mok = m < M;
    const float* xb = p.X;
    int ih0 = 0, iw0 = 0;                                              // top-left input pixel of the window (PAD > 0: may lie outside)
    if (mok) {
        const long long b = m / OHW;
        const int r = (int)(m - b * OHW), oh = r / p.OW, ow = r - oh * p.OW;
        if constexpr (PAD == 0) xb = p.X + map_off(p.x, b, g, 0, oh * S, ow * S);
        else { xb = p.X + map_off(p.x, b, g, 0, 0, 0); ih0 = oh * S - PAD; iw0 = ow * S - PAD; }
    }
    const int na = n0 + i, nb = n0 + 16 + i;
    const bool naok = na < p.cout, nbok = nb < p.cout;
    const float* wa = W + (long long)na * K;
    const float* wb = W + (long long)nb * K;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    // wave-uniform trip count; four MFMA steps per iteration so that their loads are issued together (steps past K add exact zeros).
    // Wave w takes the 16-wide k blocks w, w + 4, ...: a quarter of the dependent load chain of one tile
    for (int k0 = 16 * wave; k0 < K; k0 += 64) {
        float a[4], b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + kq;
            const bool kok = k < K;
            const int ci = k / KK, rr = k - ci * KK, kh = rr / KS, kw = rr - kh * KS;
            if constexpr (PAD == 0) {
                a[u] = (mok && kok) ? xb[(long long)ci * p.x.sC + (long long)kh * p.x.sH + (long long)kw * p.x.sW] : 0.f;
            } else {                                                   // zero padding: taps outside the map read nothing
                const int ih = ih0 + kh, iw = iw0 + kw;
                a[u] = (mok && kok && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W)
                           ? xb[(long long)ci * p.x.sC + (long long)ih * p.x.sH + (long long)iw * p.x.sW] : 0.f;
            }
            b0[u] = (naok && kok) ? wa[k] : 0.f;
            b1[u] = (nbok && kok) ? wb[k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b0[u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b1[u], acc1, 0, 0, 0);
        }
    }
    if (!reduce4(acc0, acc1, wave, lane)) return;
    // C/D map: col = lane & 15, row = 4 (lane >> 4) + r
    const float* bias = p.bias[g];
    const float bv0 = naok ? bias[na] : 0.f, bv1 = nbok ? bias[nb] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long mm = m0 + 4 * kq + r;
        if (mm >= M) break;
        const long long b = mm / OHW;
        const int rr = (int)(mm - b * OHW), oh = rr / p.OW, ow = rr - oh * p.OW;
        if (naok) {
            const long long o = map_off(p.y, b, g, na, oh, ow);
            const float v = fmaxf(acc0[r] + bv0, 0.f);
            p.Y[o] = v;
            if (p.Y2) p.Y2[o] = v;
        }
        if (nbok) {
            const long long o = map_off(p.y, b, g, nb, oh, ow);
            const float v = fmaxf(acc1[r] + bv1, 0.f);
            p.Y[o] = v;
            if (p.Y2) p.Y2[o] = v;
        }
    }
}

// partial weight (and bias) gradient of one (slab, group, 16 output channels, 32 k columns) tile
template <int KS, int S, int PAD>
__device__ __forceinline__ void nc_dw_tile(const NcBwdArgs& p, long long t, int lane) {
    constexpr int KK = KS * KS;
    const int i = lane & 15, kq = lane >> 4;
    const int K = p.cin * KK, K1 = K + 1;
    const int ntiles = (p.cout + 15) / 16, ktiles = (K1 + 31) / 32;
    const int kt = (int)(t % ktiles); t /= ktiles;
    const int nt = (int)(t % ntiles); t /= ntiles;
    const int g = (int)(t % p.G);
    const int s = (int)(t / p.G);
    const int OHW = p.OH * p.OW;
    const long long M = (long long)p.B * OHW;
    const long long mbeg = (long long)s * p.slab_rows;
    const long long mend = mbeg + p.slab_rows < M ? mbeg + p.slab_rows : M;
    const int n = nt * 16 + i;                        // A operand row (output channel)
    const bool nok = n < p.cout;
    // B operand columns: k = k0 + i and k0 + 16 + i, fixed over the loop
    const int ka = kt * 32 + i, kb = ka + 16;
    auto koff = [&](int k) -> long long {
        const int ci = k / KK, rr = k - ci * KK, kh = rr / KS, kw = rr - kh * KS;
        return (long long)ci * p.x.sC + (long long)kh * p.x.sH + (long long)kw * p.x.sW;
    };
    const long long offa = ka < K ? koff(ka) : 0, offb = kb < K ? koff(kb) : 0;
    // PAD > 0: the (kh, kw) tap of each B column, to test the input pixel against the map
    const int kha = ka < K ? (ka % KK) / KS : 0, kwa = ka < K ? (ka % KK) % KS : 0;
    const int khb = kb < K ? (kb % KK) / KS : 0, kwb = kb < K ? (kb % KK) % KS : 0;
    // the lane's reduction row m = mbeg + kq + 4 j, tracked as (b, oh, ow) and stepped by 4
    long long b = 0;
    int oh = 0, ow = 0;
    {
        const long long m = mbeg + kq;
        b = m / OHW;
        const int r = (int)(m - b * OHW);
        oh = r / p.OW; ow = r - oh * p.OW;
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (long long m4 = mbeg; m4 < mend; m4 += 4) {                     // wave-uniform trip count
        const bool mok = m4 + kq < mend;
        float a = 0.f, b0 = 0.f, b1 = 0.f;
        if (mok) {
            if (nok) a = p.dY[map_off(p.dy, b, g, n, oh, ow)];
            if constexpr (PAD == 0) {
                const float* xb = p.X + map_off(p.x, b, g, 0, oh * S, ow * S);
                b0 = ka < K ? xb[offa] : (ka == K ? 1.f : 0.f);
                b1 = kb < K ? xb[offb] : (kb == K ? 1.f : 0.f);
            } else {
                const int ih = oh * S - PAD, iw = ow * S - PAD;
                const float* xb = p.X + map_off(p.x, b, g, 0, 0, 0) + (long long)ih * p.x.sH + (long long)iw * p.x.sW;
                const bool ina = ih + kha >= 0 && ih + kha < p.H && iw + kwa >= 0 && iw + kwa < p.W;
                const bool inb = ih + khb >= 0 && ih + khb < p.H && iw + kwb >= 0 && iw + kwb < p.W;
                b0 = ka < K ? (ina ? xb[offa] : 0.f) : (ka == K ? 1.f : 0.f);
                b1 = kb < K ? (inb ? xb[offb] : 0.f) : (kb == K ? 1.f : 0.f);
            }
        }
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
        ow += 4;
        while (ow >= p.OW) {
            ow -= p.OW;
            if (++oh == p.OH) { oh = 0; ++b; }
        }
    }
    // rows = output channels 4 kq + r, columns = k
    float* P = p.part + ((long long)s * p.G + g) * p.cout * K1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nn = nt * 16 + 4 * kq + r;
        if (nn >= p.cout) break;
        if (ka < K1) P[(long long)nn * K1 + ka] = acc0[r];
        if (kb < K1) P[(long long)nn * K1 + kb] = acc1[r];
    }
}

// masked data gradient of one (group, 16 input pixels, 32 input channels) tile
template <int KS, int S, int PAD>
__device__ __forceinline__ void nc_dx_tile(const NcBwdArgs& p, long long t, int wave, int lane) {
    constexpr int KK = KS * KS;
    const int i = lane & 15, kq = lane >> 4;
    const int HW = p.H * p.W;
    const long long M = (long long)p.B * HW;
    const int mtiles = (int)((M + 15) / 16), ntiles = (p.cin + 31) / 32;
    const int mt = (int)(t % mtiles); t /= mtiles;
    const int nt = (int)(t % ntiles);
    const int g = (int)(t / ntiles);
    const long long m0 = (long long)mt * 16;
    const int K = p.cout * KK;                        // k = co KS KS + kh KS + kw
    const long long m = m0 + i;
    const bool mok = m < M;
    long long b = 0;
    int ih = 0, iw = 0;
    if (mok) {
        b = m / HW;
        const int r = (int)(m - b * HW);
        ih = r / p.W; iw = r - ih * p.W;
    }
    const float* __restrict__ W = p.w[g];
    const int ca = nt * 32 + i, cb = ca + 16;
    const bool caok = ca < p.cin, cbok = cb < p.cin;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 16 * wave; k0 < K; k0 += 64) {                      // as in nc_conv_fwd: K split over the 4 waves
        float a[4], b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + kq;
            const bool kok = k < K;
            const int co = k / KK, rr = k - co * KK, kh = rr / KS, kw = rr - kh * KS;
            const int ohn = ih + PAD - kh, own = iw + PAD - kw;
            const int oh = ohn / S, ow = own / S;
            a[u] = 0.f;
            if (mok && kok && ohn >= 0 && own >= 0 && oh * S == ohn && ow * S == own && oh < p.OH && ow < p.OW)
                a[u] = p.dY[map_off(p.dy, b, g, co, oh, ow)];
            const long long wo = (long long)co * p.cin * KK + rr;
            b0[u] = (caok && kok) ? W[wo + (long long)ca * KK] : 0.f;
            b1[u] = (cbok && kok) ? W[wo + (long long)cb * KK] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b0[u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b1[u], acc1, 0, 0, 0);
        }
    }
    if (!reduce4(acc0, acc1, wave, lane)) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long mm = m0 + 4 * kq + r;
        if (mm >= M) break;
        const long long bb = mm / HW;
        const int rr = (int)(mm - bb * HW), h = rr / p.W, w = rr - h * p.W;
        if (caok) {
            const long long o = map_off(p.x, bb, g, ca, h, w);
            p.dX[o] = p.X[o] > 0.f ? acc0[r] : 0.f;
        }
        if (cbok) {
            const long long o = map_off(p.x, bb, g, cb, h, w);
            p.dX[o] = p.X[o] > 0.f ? acc1[r] : 0.f;
        }
    }
}

template <int KS, int S, int PAD>
__global__ __launch_bounds__(256) void nc_conv_bwd_kernel(NcBwdArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < p.dw_blocks) {
        const long long t = (long long)blockIdx.x * 4 + wave;
        if (t < p.dw_tiles) nc_dw_tile<KS, S, PAD>(p, t, lane);
    } else {
        nc_dx_tile<KS, S, PAD>(p, (long long)(blockIdx.x - p.dw_blocks), wave, lane);   // one tile per workgroup
    }
}

__global__ __launch_bounds__(256) void nc_dw_reduce_kernel(NcReduceArgs p) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int l = 0;
    while (l < p.nlayers && t >= p.L[l].n) { t -= p.L[l].n; ++l; }
    if (l >= p.nlayers) return;
    const NcReduceLayer& y = p.L[l];
    const int K1 = y.K + 1;
    const long long per = (long long)y.cout * K1;
    const int g = (int)(t / per);
    const long long e = t - g * per;
    const long long stride = (long long)y.G * per;
    const float* src = y.part + g * per + e;
    float s = 0.f;
    for (int j = 0; j < y.slabs; ++j) s += src[(long long)j * stride];
    const int n = (int)(e / K1), k = (int)(e - (long long)n * K1);
    if (k < y.K) p.dw[l][g][(long long)n * y.K + k] = s;
    else p.db[l][g][n] = s;
}

__global__ __launch_bounds__(256) void nc_relu_mask_kernel(const float* __restrict__ d, const float* __restrict__ a, float* __restrict__ o, long long n) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) o[t] = a[t] > 0.f ? d[t] : 0.f;
}

}  // namespace

int nc_conv_fwd_launch(const NcFwdArgs& a, hipStream_t st) {
    OCRL_REQUIRE(a.B >= 1 && a.G >= 1 && a.G <= OCRL_NATURECNN_MAX_GROUPS && a.cin >= 1 && a.cout >= 1 && a.OH >= 1 && a.OW >= 1,
                 "nc_conv_fwd: bad shape");
    const long long tiles = (((long long)a.B * a.OH * a.OW + 15) / 16) * ((a.cout + 31) / 32) * a.G;
    const dim3 grid((unsigned)tiles), block(256);
    if (a.ks == 8 && a.stride == 4 && a.pad == 0) hipLaunchKernelGGL((nc_conv_fwd_kernel<8, 4, 0>), grid, block, 0, st, a);
    else if (a.ks == 4 && a.stride == 2 && a.pad == 0) hipLaunchKernelGGL((nc_conv_fwd_kernel<4, 2, 0>), grid, block, 0, st, a);
    else if (a.ks == 3 && a.stride == 1 && a.pad == 0) hipLaunchKernelGGL((nc_conv_fwd_kernel<3, 1, 0>), grid, block, 0, st, a);
    else if (a.ks == 2 && a.stride == 2 && a.pad == 0) hipLaunchKernelGGL((nc_conv_fwd_kernel<2, 2, 0>), grid, block, 0, st, a);   // VAE encoder
    else if (a.ks == 3 && a.stride == 1 && a.pad == 1) hipLaunchKernelGGL((nc_conv_fwd_kernel<3, 1, 1>), grid, block, 0, st, a);   // VAE decoder, small maps
    else OCRL_REQUIRE(false, "nc_conv_fwd: (kernel %d, stride %d, padding %d) is not built", a.ks, a.stride, a.pad);
    OCRL_CHECK_LAUNCH("nc_conv_fwd");
    return 0;
}

int nc_conv_bwd_launch(NcBwdArgs a, hipStream_t st) {
    OCRL_REQUIRE(a.B >= 1 && a.G >= 1 && a.G <= OCRL_NATURECNN_MAX_GROUPS && a.cin >= 1 && a.cout >= 1 && a.OH >= 1 && a.OW >= 1 && a.slabs >= 1 &&
                 a.slab_rows >= 1, "nc_conv_bwd: bad shape");
    const int K1 = a.cin * a.ks * a.ks + 1;
    a.dw_tiles = (long long)a.slabs * a.G * ((a.cout + 15) / 16) * ((K1 + 31) / 32);
    a.dw_blocks = cdiv(a.dw_tiles, 4);
    a.dx_tiles = a.dX ? (((long long)a.B * a.H * a.W + 15) / 16) * ((a.cin + 31) / 32) * a.G : 0;
    const dim3 grid((unsigned)(a.dw_blocks + a.dx_tiles)), block(256);
    if (a.ks == 8 && a.stride == 4 && a.pad == 0) hipLaunchKernelGGL((nc_conv_bwd_kernel<8, 4, 0>), grid, block, 0, st, a);
    else if (a.ks == 4 && a.stride == 2 && a.pad == 0) hipLaunchKernelGGL((nc_conv_bwd_kernel<4, 2, 0>), grid, block, 0, st, a);
    else if (a.ks == 3 && a.stride == 1 && a.pad == 0) hipLaunchKernelGGL((nc_conv_bwd_kernel<3, 1, 0>), grid, block, 0, st, a);
    else if (a.ks == 2 && a.stride == 2 && a.pad == 0) hipLaunchKernelGGL((nc_conv_bwd_kernel<2, 2, 0>), grid, block, 0, st, a);   // VAE encoder
    else if (a.ks == 3 && a.stride == 1 && a.pad == 1) hipLaunchKernelGGL((nc_conv_bwd_kernel<3, 1, 1>), grid, block, 0, st, a);   // VAE decoder, small maps
    else OCRL_REQUIRE(false, "nc_conv_bwd: (kernel %d, stride %d, padding %d) is not built", a.ks, a.stride, a.pad);
    OCRL_CHECK_LAUNCH("nc_conv_bwd");
    return 0;
}

int nc_dw_reduce_launch(const NcReduceArgs& a, hipStream_t st) {
    OCRL_REQUIRE(a.nlayers >= 1 && a.nlayers <= OCRL_NATURECNN_MAX_CONVS, "nc_dw_reduce: bad layer count %d", a.nlayers);
    long long n = 0;
    for (int l = 0; l < a.nlayers; ++l) n += a.L[l].n;
    hipLaunchKernelGGL(nc_dw_reduce_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("nc_dw_reduce");
    return 0;
}

int nc_relu_mask_launch(const float* d, const float* act, float* out, long long n, hipStream_t st) {
    hipLaunchKernelGGL(nc_relu_mask_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, d, act, out, n);
    OCRL_CHECK_LAUNCH("nc_relu_mask");
    return 0;
}
