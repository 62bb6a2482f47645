// First layer of the NatureCNN pooling heads (poolings/common/naturecnn.py:14-15 behind utils/tools.py slot_to_img): Conv2d(D, 32, k 8, s 4),
// padding 0, ReLU, over a channels-last token map [B, H, W, D] (the [B, H W, C + 3] tokens SLATE returns with use_cnn_feat; D = 67 is the
// case that matters).  The arithmetic contract is that of conv.hip and naturecnn.hip: exact fp32 products, fp32 accumulation on
// v_mfma_f32_16x16x4_f32, no atomics, every summation order fixed by the shapes alone.  Unlike nc_conv_fwd, whose k = ci 64 + kh 8 + kw
// puts every lane of an A-operand load on its own cache line of such a map, k here walks (kh, kw D + ci): the window of an output
// pixel is 8 runs of 8 D contiguous floats, and 16 horizontally adjacent output pixels read, per kh, one run of 68 D floats.
//
// That run is seen as 17 blocks of 4 D floats (4 input pixels): output pixel i uses blocks i and i + 1 ("half" 0 and 1 of its 8 D
// floats), so adjacent pixels share half their window in LDS.  A block starts at a multiple of 16 D bytes: with W D % 4 == 0 every
// piece is a 16-byte aligned float4 (VEC), otherwise the same pieces are read float by float.  K is walked in steps (kh, c): chunk c
// holds columns [64 c, 64 c + 64) of both halves, as groups of 16 columns; NG = ceil(4 D / 16) groups per half, zero-padded.
//
//   pc_pack_w     w [32, D, 8, 8] -> Wp [8 nchunk][32][128]: the LDS image of each step's weights (column = half 64 + r)
//   pc_fwd        Y [B, 32, OH, OW] = relu(b + conv): one workgroup per (image, R output rows, 16 output columns) x 32 channels; its 4 waves
//                 split the groups of a step and sum their partial tiles through LDS in wave order.  The next step's global reads are
//                 issued before the current step's MFMAs.  R (1 or 2) changes the tile, not the order of any sum
//   pc_dw         partial dW over one slab of (image, output row, 16 columns) units for one step: P[s][step][n][128], the bias partial
//                 (the ones column) from the workgroups of step 0.  The waves stage one unit each per iteration and take 32 columns each
//   pc_dw_reduce  dW [32, D, 8, 8], db [32] = sums of the slabs in slab order
//   pc_pack_wd    w -> Wd [4 ph][4 pw][128][Dp]: per phase, k = (tap a, tap e, n) with kh = ph + 4 a, kw = pw + 4 e
//   pc_dx         dX [B, H, W, D]: input pixel (ih, iw) is reached only by kh = ih % 4 + 4 a, kw = iw % 4 + 4 e from output positions
//                 (ih / 4 - a, iw / 4 - e): K = 128 per pixel.  One workgroup per (ph, group of (image, row, 16 column quads) units,
//                 pass over NBG 16-channel blocks); wave pw keeps its phase's weights in registers.  No ReLU mask: tokens are no ReLU
//                 output.  Pixels no window covers get 0; every element is written.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int CK = 64;        // columns of one half per step
constexpr int TS = 68;        // row stride of the forward's token tile: 16-byte aligned rows, ds_read_b128 slots (i + kq) % 16
constexpr int WS = 132;       // row stride of the weight tile, the same slot pattern
constexpr int TD = 80;        // row stride of the token tile in pc_dw: ds_read_b32 banks 16 kq + i
constexpr int YS = 18;        // row stride of the dY tile in pc_dw: banks 18 n + kq distinct over a half wave
constexpr int YX = 17;        // row stride of the dY tile in pc_dx (17 output columns)

template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* p) {
    if constexpr (VEC) return *reinterpret_cast<const float4*>(p);
    else return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// (half, kw, ci) of packed column `col` of chunk c; false past the 4 D columns of a half
__device__ __forceinline__ bool col_tap(int col, int c, int D, int& kw, int& ci) {
    const int half = col / CK, r = c * CK + (col - half * CK);
    if (r >= 4 * D) return false;
    const int kp = half * 4 * D + r;
    kw = kp / D; ci = kp - kw * D;
    return true;
}

__global__ __launch_bounds__(256) void pc_pack_w_kernel(const float* __restrict__ w, float* __restrict__ Wp, int D, int nchunk) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)8 * nchunk * 32 * 128) return;
    const int col = (int)(t & 127), n = (int)((t >> 7) & 31), it = (int)(t >> 12);
    const int kh = it / nchunk, c = it - kh * nchunk;
    int kw, ci;
    Wp[t] = col_tap(col, c, D, kw, ci) ? w[(((long long)n * D + ci) * 8 + kh) * 8 + kw] : 0.f;
}

template <int R, bool VEC>
__global__ __launch_bounds__(256) void pc_fwd_kernel(PcFwdArgs p) {
    constexpr int NX = (R * 272 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float T[R * 17 * TS];
    __shared__ __attribute__((aligned(16))) float Wl[32 * WS];
    static_assert(3 * R * 2 * 64 * 4 <= 32 * WS, "the reduction reuses the weight tile");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int OHG = (p.OH + R - 1) / R;
    long long t = blockIdx.x;
    const int owt = (int)(t % p.OWT); t /= p.OWT;
    const int ohg = (int)(t % OHG);
    const long long b = t / OHG;
    const int oh0 = ohg * R, ow0 = owt * 16;
    const int D4 = 4 * p.D, nit = 8 * p.nchunk;

    float4 xr[NX], wr0, wr1, wr2, wr3;
    auto load = [&](int it) {
        const int kh = it / p.nchunk, c = it - kh * p.nchunk;
#pragma unroll
        for (int s = 0; s < NX; ++s) {
            const int f = tid + 256 * s;
            xr[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (f < R * 272) {
                const int rr = f / 272, g = f - rr * 272, j = g >> 4, q = g & 15;
                const int col = c * CK + 4 * q, oh = oh0 + rr, px = 4 * (ow0 + j);
                if (oh < p.OH && px + 4 <= p.W && col < D4)
                    xr[s] = ld4<VEC>(p.X + ((b * p.H + 4 * oh + kh) * p.W + px) * p.D + col);
            }
        }
        const float* wp = p.Wp + (long long)it * 4096;
        wr0 = *reinterpret_cast<const float4*>(wp + 4 * tid);
        wr1 = *reinterpret_cast<const float4*>(wp + 4 * (tid + 256));
        wr2 = *reinterpret_cast<const float4*>(wp + 4 * (tid + 512));
        wr3 = *reinterpret_cast<const float4*>(wp + 4 * (tid + 768));
    };
    auto store = [&]() {
#pragma unroll
        for (int s = 0; s < NX; ++s) {
            const int f = tid + 256 * s;
            if (f < R * 272) {
                const int rr = f / 272, g = f - rr * 272, j = g >> 4, q = g & 15;
                *reinterpret_cast<float4*>(&T[(rr * 17 + j) * TS + 4 * q]) = xr[s];
            }
        }
        float* wl = &Wl[(tid >> 5) * WS + 4 * (tid & 31)];           // float4 f = tid + 256 s: row f / 32 = tid / 32 + 8 s
        *reinterpret_cast<float4*>(wl) = wr0;
        *reinterpret_cast<float4*>(wl + 8 * WS) = wr1;
        *reinterpret_cast<float4*>(wl + 16 * WS) = wr2;
        *reinterpret_cast<float4*>(wl + 24 * WS) = wr3;
    };

    f32x4 acc[R][2];
#pragma unroll
    for (int r = 0; r < R; ++r) { acc[r][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[r][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    load(0);
    for (int it = 0; it < nit; ++it) {
        __syncthreads();                                              // the previous step's reads of T / Wl are done
        store();
        __syncthreads();
        if (it + 1 < nit) load(it + 1);
        const int c = it % p.nchunk;
        const int ng = p.NG - 4 * c < 4 ? p.NG - 4 * c : 4;
        // items (half, group) of this step, dealt to the waves in turn; lane (i, kq) holds k = 16 g + 4 kq + u of both operands
        for (int item = wave; item < 2 * ng; item += 4) {
            const int half = item / ng, gi = item - half * ng;
            const int kc = 16 * gi + 4 * kq;
            const float4 b0 = *reinterpret_cast<const float4*>(&Wl[i * WS + half * CK + kc]);
            const float4 b1 = *reinterpret_cast<const float4*>(&Wl[(16 + i) * WS + half * CK + kc]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 a = *reinterpret_cast<const float4*>(&T[(r * 17 + i + half) * TS + kc]);
                acc[r][0] = mfma4(a.x, b0.x, acc[r][0]); acc[r][1] = mfma4(a.x, b1.x, acc[r][1]);
                acc[r][0] = mfma4(a.y, b0.y, acc[r][0]); acc[r][1] = mfma4(a.y, b1.y, acc[r][1]);
                acc[r][0] = mfma4(a.z, b0.z, acc[r][0]); acc[r][1] = mfma4(a.z, b1.z, acc[r][1]);
                acc[r][0] = mfma4(a.w, b0.w, acc[r][0]); acc[r][1] = mfma4(a.w, b1.w, acc[r][1]);
            }
        }
    }
    // the four waves' partial tiles summed in wave order (fixed: bitwise reproducible)
    __syncthreads();
    f32x4* red = reinterpret_cast<f32x4*>(Wl);
    if (wave) {
#pragma unroll
        for (int r = 0; r < R; ++r) { red[(((wave - 1) * R + r) * 2 + 0) * 64 + lane] = acc[r][0]; red[(((wave - 1) * R + r) * 2 + 1) * 64 + lane] = acc[r][1]; }
    }
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int r = 0; r < R; ++r) { acc[r][0] += red[((w * R + r) * 2 + 0) * 64 + lane]; acc[r][1] += red[((w * R + r) * 2 + 1) * 64 + lane]; }
    // C/D map: col (channel) = lane & 15, row (pixel) = 4 (lane >> 4) + e
    const float bv0 = p.bias[i], bv1 = p.bias[16 + i];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int oh = oh0 + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ow = ow0 + 4 * kq + e;
            if (oh >= p.OH || ow >= p.OW) continue;
            p.Y[((b * 32 + i) * p.OH + oh) * p.OW + ow] = fmaxf(acc[r][0][e] + bv0, 0.f);
            p.Y[((b * 32 + 16 + i) * p.OH + oh) * p.OW + ow] = fmaxf(acc[r][1][e] + bv1, 0.f);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void pc_dw_kernel(PcDwArgs p) {
    __shared__ __attribute__((aligned(16))) float T[4 * 17 * TD];
    __shared__ float Yl[4 * 32 * YS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int nit = 8 * p.nchunk;
    const int it = (int)(blockIdx.x % nit), s = (int)(blockIdx.x / nit);
    const int kh = it / p.nchunk, c = it - kh * p.nchunk;
    const int D4 = 4 * p.D, rem = D4 - c * CK;                         // valid columns of this chunk in each half
    const long long ubeg = (long long)s * p.slab_units;
    const long long uend = ubeg + p.slab_units < p.units ? ubeg + p.slab_units : p.units;

    // wave w stages unit u0 + w of an iteration: the unit's decode is wave-uniform
    float4 xr[5];
    float yr[8];
    auto load = [&](long long u0) {
        const long long u = u0 + wave;
        const bool uok = u < uend;
        long long b = 0;
        int oh = 0, ow0 = 0;
        if (uok) {
            long long q = u;
            ow0 = (int)(q % p.OWT) * 16; q /= p.OWT;
            oh = (int)(q % p.OH); b = q / p.OH;
        }
        const float* xrow = p.X + ((b * p.H + 4 * oh + kh) * p.W) * p.D;
#pragma unroll
        for (int z = 0; z < 5; ++z) {
            const int f = lane + 64 * z;
            xr[z] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (f < 272) {
                const int j = f >> 4, q = f & 15;
                const int px = 4 * (ow0 + j);
                if (uok && px + 4 <= p.W && 4 * q < rem) xr[z] = ld4<VEC>(xrow + (long long)px * p.D + c * CK + 4 * q);
            }
        }
#pragma unroll
        for (int z = 0; z < 8; ++z) {
            const int f = lane + 64 * z, n = f >> 4, m = f & 15;
            yr[z] = (uok && ow0 + m < p.OW) ? p.dY[((b * 32 + n) * p.OH + oh) * p.OW + ow0 + m] : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int z = 0; z < 5; ++z) {
            const int f = lane + 64 * z;
            if (f < 272) *reinterpret_cast<float4*>(&T[(wave * 17 + (f >> 4)) * TD + 4 * (f & 15)]) = xr[z];
        }
#pragma unroll
        for (int z = 0; z < 8; ++z) {
            const int f = lane + 64 * z;
            Yl[(wave * 32 + (f >> 4)) * YS + (f & 15)] = yr[z];
        }
    };

    // wave w owns packed columns [32 w, 32 w + 32): half w / 2, in-chunk columns (w % 2) 32 + 16 cb + i
    const int half = wave >> 1, r0 = (wave & 1) * 32;
    const bool cbok[2] = {r0 < rem, r0 + 16 < rem};                     // a block of 16 columns wholly past 4 D is skipped
    const bool want_bias = it == 0 && wave == 0;
    f32x4 acc[2][2], accb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) { acc[h][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[h][1] = f32x4{0.f, 0.f, 0.f, 0.f}; accb[h] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    load(ubeg);
    for (long long u0 = ubeg; u0 < uend; u0 += 4) {
        __syncthreads();
        store();
        __syncthreads();
        if (u0 + 4 < uend) load(u0 + 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int ms = 0; ms < 4; ++ms) {
                const int m = 4 * ms + kq;
                const float a0 = Yl[(u * 32 + i) * YS + m], a1 = Yl[(u * 32 + 16 + i) * YS + m];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    if (!cbok[cb]) continue;
                    const float bv = T[(u * 17 + m + half) * TD + r0 + 16 * cb + i];
                    acc[0][cb] = mfma4(a0, bv, acc[0][cb]);
                    acc[1][cb] = mfma4(a1, bv, acc[1][cb]);
                }
                if (want_bias) { accb[0] = mfma4(a0, 1.f, accb[0]); accb[1] = mfma4(a1, 1.f, accb[1]); }
            }
        }
    }
    // rows = output channels 16 h + 4 kq + e, columns = packed k
    float* P = p.part + ((long long)s * nit + it) * 4096;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = 16 * h + 4 * kq + e;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
                if (cbok[cb]) P[n * 128 + 32 * wave + 16 * cb + i] = acc[h][cb][e];
            if (want_bias && i == 0) p.partb[s * 32 + n] = accb[h][e];
        }
}

__global__ __launch_bounds__(256) void pc_dw_reduce_kernel(const float* __restrict__ part, const float* __restrict__ partb, float* __restrict__ dw,
                                                           float* __restrict__ db, int D, int nchunk, int slabs) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per = (long long)8 * nchunk * 4096;
    if (t < per) {
        const int col = (int)(t & 127), n = (int)((t >> 7) & 31), it = (int)(t >> 12);
        const int kh = it / nchunk, c = it - kh * nchunk;
        int kw, ci;
        if (!col_tap(col, c, D, kw, ci)) return;
        float v = 0.f;
        for (int s = 0; s < slabs; ++s) v += part[s * per + t];
        dw[(((long long)n * D + ci) * 8 + kh) * 8 + kw] = v;
    } else if (t < per + 32) {
        const int n = (int)(t - per);
        float v = 0.f;
        for (int s = 0; s < slabs; ++s) v += partb[s * 32 + n];
        db[n] = v;
    }
}

__global__ __launch_bounds__(256) void pc_pack_wd_kernel(const float* __restrict__ w, float* __restrict__ Wd, int D, int Dp) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)16 * 128 * Dp) return;
    const int ci = (int)(t % Dp);
    const int k = (int)((t / Dp) & 127), phase = (int)(t / ((long long)Dp * 128));
    const int ph = phase >> 2, pw = phase & 3, tap = k >> 5, n = k & 31, a = tap >> 1, e = tap & 1;
    Wd[t] = ci < D ? w[(((long long)n * D + ci) * 8 + ph + 4 * a) * 8 + pw + 4 * e] : 0.f;
}

template <int NBG>
__global__ __launch_bounds__(256) void pc_dx_kernel(PcDxArgs p) {
    __shared__ float Yl[2 * 32 * YX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int pw = __builtin_amdgcn_readfirstlane(tid >> 6);         // wave = horizontal phase
    const int i = lane & 15, kq = lane >> 4;
    long long t = blockIdx.x;
    const long long grp = t % p.groups; t /= p.groups;
    const int pass = (int)(t % p.passes), ph = (int)(t / p.passes);
    const int cb0 = pass * NBG * 16;                                   // first channel of this pass

    // this wave's phase weights: B operand of k step s is Wd[ph][pw][4 s + kq][channel]
    float wreg[NBG][32];
    {
        const float* wd = p.Wd + ((long long)(ph * 4 + pw) * 128 + kq) * p.Dp + cb0 + i;
#pragma unroll
        for (int s = 0; s < 32; ++s)
#pragma unroll
            for (int blk = 0; blk < NBG; ++blk) wreg[blk][s] = wd[(long long)4 * s * p.Dp + 16 * blk];
    }
    const long long ubeg = grp * p.upw;
    const long long uend = ubeg + p.upw < p.units ? ubeg + p.upw : p.units;
    float yr[5];
    auto load = [&](long long u) {
        long long q = u;
        const int owb0 = (int)(q % p.WT) * 16; q /= p.WT;
        const int ihb = (int)(q % p.HB);
        const long long b = q / p.HB;
#pragma unroll
        for (int z = 0; z < 5; ++z) {
            const int f = tid + 256 * z;
            yr[z] = 0.f;
            if (f < 2 * 32 * YX) {
                const int a = f / (32 * YX), g = f - a * 32 * YX, n = g / YX, x = g - n * YX;
                const int oh = ihb - a, ow = owb0 + x - 1;
                if (oh >= 0 && oh < p.OH && ow >= 0 && ow < p.OW) yr[z] = p.dY[((b * 32 + n) * p.OH + oh) * p.OW + ow];
            }
        }
    };
    load(ubeg);
    for (long long u = ubeg; u < uend; ++u) {
        __syncthreads();
#pragma unroll
        for (int z = 0; z < 5; ++z) {
            const int f = tid + 256 * z;
            if (f < 2 * 32 * YX) Yl[f] = yr[z];
        }
        __syncthreads();
        if (u + 1 < uend) load(u + 1);
        f32x4 acc[NBG];
#pragma unroll
        for (int blk = 0; blk < NBG; ++blk) acc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const int tap = s >> 3, a = tap >> 1, e = tap & 1, n = 4 * (s & 7) + kq;
            const float av = Yl[(a * 32 + n) * YX + i + 1 - e];        // dY[n][ihb - a][owb0 + i - e], 0 outside the map
#pragma unroll
            for (int blk = 0; blk < NBG; ++blk) acc[blk] = mfma4(av, wreg[blk][s], acc[blk]);
        }
        long long q = u;
        const int owb0 = (int)(q % p.WT) * 16; q /= p.WT;
        const int ih = 4 * (int)(q % p.HB) + ph;
        const long long b = q / p.HB;
        if (ih < p.H) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int iw = 4 * (owb0 + 4 * kq + e) + pw;
                if (iw >= p.W) continue;
                float* o = p.dX + ((b * p.H + ih) * p.W + iw) * p.D;
#pragma unroll
                for (int blk = 0; blk < NBG; ++blk) {
                    const int ci = cb0 + 16 * blk + i;
                    if (ci < p.D) o[ci] = acc[blk][e];
                }
            }
        }
    }
}

}  // namespace

PcGeom pc_geom(int B, int H, int W, int D) {
    PcGeom g;
    g.OH = (H - 8) / 4 + 1; g.OW = (W - 8) / 4 + 1;
    g.OWT = (g.OW + 15) / 16;
    g.NG = (4 * D + 15) / 16;
    g.nchunk = (g.NG + 3) / 4;
    g.wp_floats = (size_t)8 * g.nchunk * 4096;
    // weight gradient: up to 16 slabs of (image, output row, 16 columns) units, a multiple of 4 and at least 8 units each
    g.units = (long long)B * g.OH * g.OWT;
    long long su = (g.units + 15) / 16;
    su = (su + 3) & ~3LL;
    if (su < 8) su = 8;
    g.slab_units = (int)su;
    g.slabs = (int)((g.units + su - 1) / su);
    g.part_floats = (size_t)g.slabs * (g.wp_floats + 32);
    // input gradient: passes over at most 5 blocks of 16 channels (the weights of a pass live in registers)
    const int nblk = (D + 15) / 16;
    g.passes = (nblk + 4) / 5;
    g.nbg = (nblk + g.passes - 1) / g.passes;
    g.Dp = g.passes * g.nbg * 16;
    g.wd_floats = (size_t)16 * 128 * g.Dp;
    g.HB = (H + 3) / 4; g.WB = (W + 3) / 4; g.WT = (g.WB + 15) / 16;
    g.dx_units = (long long)B * g.HB * g.WT;
    long long upw = g.dx_units / 128;
    g.upw = (int)(upw < 1 ? 1 : upw > 8 ? 8 : upw);
    return g;
}

int pc_conv1_fwd_launch(const float* X, const float* w, const float* bias, float* Wp, float* Y, int B, int H, int W, int D, hipStream_t st) {
    const PcGeom g = pc_geom(B, H, W, D);
    hipLaunchKernelGGL(pc_pack_w_kernel, dim3(cdiv((long long)g.wp_floats, 256)), dim3(256), 0, st, w, Wp, D, g.nchunk);
    OCRL_CHECK_LAUNCH("pc_pack_w");
    PcFwdArgs a;
    a.X = X; a.Wp = Wp; a.bias = bias; a.Y = Y;
    a.B = B; a.H = H; a.W = W; a.D = D; a.OH = g.OH; a.OW = g.OW; a.OWT = g.OWT; a.nchunk = g.nchunk; a.NG = g.NG;
    const bool vec = ((long long)W * D) % 4 == 0 && ((uintptr_t)X & 15) == 0;
    // two output rows per workgroup once single rows already fill the device several times over: half the weight traffic per output
    const bool two = g.units >= 2048;
    const long long tiles = (long long)B * ((g.OH + (two ? 1 : 0)) / (two ? 2 : 1)) * g.OWT;
    const dim3 grid((unsigned)tiles), block(256);
    if (two) {
        if (vec) hipLaunchKernelGGL((pc_fwd_kernel<2, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((pc_fwd_kernel<2, false>), grid, block, 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((pc_fwd_kernel<1, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((pc_fwd_kernel<1, false>), grid, block, 0, st, a);
    }
    OCRL_CHECK_LAUNCH("pc_fwd");
    return 0;
}

int pc_conv1_dw_launch(const float* X, const float* dY, float* part, int B, int H, int W, int D, hipStream_t st) {
    const PcGeom g = pc_geom(B, H, W, D);
    PcDwArgs a;
    a.X = X; a.dY = dY; a.part = part; a.partb = part + (size_t)g.slabs * g.wp_floats;
    a.B = B; a.H = H; a.W = W; a.D = D; a.OH = g.OH; a.OW = g.OW; a.OWT = g.OWT; a.nchunk = g.nchunk;
    a.units = g.units; a.slab_units = g.slab_units;
    const dim3 grid((unsigned)((long long)g.slabs * 8 * g.nchunk)), block(256);
    if (((long long)W * D) % 4 == 0 && ((uintptr_t)X & 15) == 0) hipLaunchKernelGGL((pc_dw_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((pc_dw_kernel<false>), grid, block, 0, st, a);
    OCRL_CHECK_LAUNCH("pc_dw");
    return 0;
}

int pc_conv1_dw_reduce_launch(const float* part, float* dw, float* db, int B, int H, int W, int D, hipStream_t st) {
    const PcGeom g = pc_geom(B, H, W, D);
    hipLaunchKernelGGL(pc_dw_reduce_kernel, dim3(cdiv((long long)g.wp_floats + 32, 256)), dim3(256), 0, st, part, part + (size_t)g.slabs * g.wp_floats, dw,
                       db, D, g.nchunk, g.slabs);
    OCRL_CHECK_LAUNCH("pc_dw_reduce");
    return 0;
}

int pc_conv1_dx_launch(const float* dY, const float* w, float* Wd, float* dX, int B, int H, int W, int D, hipStream_t st) {
    const PcGeom g = pc_geom(B, H, W, D);
    hipLaunchKernelGGL(pc_pack_wd_kernel, dim3(cdiv((long long)g.wd_floats, 256)), dim3(256), 0, st, w, Wd, D, g.Dp);
    OCRL_CHECK_LAUNCH("pc_pack_wd");
    PcDxArgs a;
    a.dY = dY; a.Wd = Wd; a.dX = dX;
    a.H = H; a.W = W; a.D = D; a.OH = g.OH; a.OW = g.OW; a.HB = g.HB; a.WT = g.WT; a.Dp = g.Dp; a.passes = g.passes;
    a.units = g.dx_units; a.upw = g.upw; a.groups = (g.dx_units + g.upw - 1) / g.upw;
    const dim3 grid((unsigned)(4LL * g.passes * a.groups)), block(256);
    switch (g.nbg) {
        case 1: hipLaunchKernelGGL((pc_dx_kernel<1>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((pc_dx_kernel<2>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((pc_dx_kernel<3>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((pc_dx_kernel<4>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((pc_dx_kernel<5>), grid, block, 0, st, a); break;
    }
    OCRL_CHECK_LAUNCH("pc_dx");
    return 0;
}
