// The encoder's first layer: 5x5, 3 -> 64 channels, stride 1, "same" padding, fp32 on v_mfma_f32_32x32x2_f32 (gfx950), reading the
// observation as the engine receives it ([B,3,H,W], NCHW).  The layer's reduction depth is K = 3 * 25 = 75; the 8-channel instantiation
// of conv.hip pads it to 200 and needs an NHWC8 copy of the observation, and its weight gradient went through a materialised patch
// matrix [B*H*W, 76].  Here k = tap * 3 + ci indexes a planar halo tile in LDS directly.
//
// conv_first_fwd_kernel   — implicit GEMM, M = 4x32 pixels per tile (one image row segment per wave), N = 64, K = 76 (one zero weight
//     row): 38 MFMAs per accumulator.  The packed weights [76][64] live in registers (76 per lane) for all the tiles a workgroup
//     walks; the halo of tile t+1 is loaded while tile t runs.  Bias + ReLU epilogue and float4 NHWC stores as conv_fwd_kernel.
// conv_first_wgrad_kernel — dW[co][k] = sum_pixels dY[p][co] * x[ci(k)][p + tap(k)] with the pixels as the MFMA k dimension: a wave owns
//     one row of the tile and six 32x32 accumulators (2 halves of co x 3 column tiles covering k = 0..95); lanes gather their k's halo
//     element.  The bias gradient is the running sum of the dY fragments.  The four waves are summed in LDS in wave order into one slab
//     [64][96] + [64] per worker; conv_first_wgrad_reduce_kernel sums the slabs in a fixed order into the reference layout [64][3][5][5].
#include "common.h"
#include "kernels.h"

#define TH 4
#define TW 32

namespace {
constexpr int KS = 5, PAD = 2, CI = 3, CO = 64;
constexpr int KR = KS * KS * CI;                    // 75
constexpr int KF = 76;                              // forward depth: even, row 75 of the pack is zero
constexpr int HH = TH + KS - 1, HWD = TW + KS - 1;  // halo 8 x 36 per channel
constexpr int HN = CI * HH * HWD;                   // 864 halo elements
constexpr int NH = (HN + 255) / 256;
// forward: lanes read 32 consecutive pixels of one (channel, row), any pitch is conflict-free
constexpr int FP = HWD, FC = HH * FP;
// weight gradient: lane l of a column tile reads element k = 32 ct + l; with row pitch 47 = 15 (mod 32) and channel pitch 389 = 5 (mod 32)
// the 15 (kx, ci) of one kernel row fall on 15 consecutive banks and the next kernel row on the 15 after them
constexpr int GP = 47, GC = 389;
constexpr int GHALO = CI * GC;
constexpr int KG = 96;                              // weight-gradient columns (three 32-wide tiles; 75 used)
constexpr int SLAB = CO * KG + CO;                  // one worker's partial: dW [64][96], then db [64]
constexpr int WORKERS = 512;                        // two co-resident workgroups per CU
constexpr int RG = 8, RO = 32;                      // reduce: 8 slab groups x 32 outputs per workgroup

__device__ __host__ constexpr int halo_off(int k, int pitch, int cpitch) {
    const int kk = k < KR ? k : KR - 1;             // padding columns re-read the last element (their products are discarded / meet zero weights)
    const int tap = kk / CI, ci = kk - tap * CI, ky = tap / KS, kx = tap - ky * KS;
    return ci * cpitch + ky * pitch + kx;
}

struct Tile { int b, y0, x0; };
__device__ __forceinline__ Tile tile_of(int t, int tiles_x, int tiles_y) {
    Tile r;
    r.x0 = (t % tiles_x) * TW; t /= tiles_x;
    r.y0 = (t % tiles_y) * TH;
    r.b = t / tiles_y;
    return r;
}
// the 3 x 8 x 36 halo of a tile from the NCHW observation (zero outside the image): element idx = threadIdx.x + 256 i
__device__ __forceinline__ void halo_load(float (&hv)[NH], const float* __restrict__ obs, const Tile& q, int H, int W) {
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        const int idx = threadIdx.x + i * 256;
        const int ci = idx / (HH * HWD), rem = idx - ci * (HH * HWD), hy = rem / HWD, hx = rem - hy * HWD;
        const int y = q.y0 - PAD + hy, x = q.x0 - PAD + hx;
        hv[i] = 0.f;
        if (idx < HN && y >= 0 && y < H && x >= 0 && x < W) hv[i] = obs[(((size_t)q.b * CI + ci) * H + y) * W + x];
    }
}
__device__ __forceinline__ void halo_store(const float (&hv)[NH], float* hs, int pitch, int cpitch) {
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        const int idx = threadIdx.x + i * 256;
        const int ci = idx / (HH * HWD), rem = idx - ci * (HH * HWD), hy = rem / HWD, hx = rem - hy * HWD;
        if (idx < HN) hs[ci * cpitch + hy * pitch + hx] = hv[i];
    }
}
}  // namespace

__global__ __launch_bounds__(256, 2) void conv_first_fwd_kernel(const float* __restrict__ obs, const float* __restrict__ Wp, const float* __restrict__ bias,
                                                                float* __restrict__ Y, int B, int H, int W, int relu) {
    __shared__ float hs[CI * FC];
    __shared__ __attribute__((aligned(16))) float patches[4 * 32 * (CO + 4)];
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH, ntiles = tiles_x * tiles_y * B;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;

    // this lane's B fragments of all 38 steps: rows 2s + lh of the pack, columns li and 32 + li
    float wb0[KF / 2], wb1[KF / 2];
#pragma unroll
    for (int s = 0; s < KF / 2; ++s) {
        wb0[s] = Wp[(2 * s + lh) * CO + li];
        wb1[s] = Wp[(2 * s + lh) * CO + 32 + li];
    }
    const int c4 = lane & 15, px0 = lane >> 4;
    const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    float* patch = patches + wave * 32 * (CO + 4);
    const float* arow = hs + wave * FP + li;

    float hv[NH];
    if ((int)blockIdx.x < ntiles) halo_load(hv, obs, tile_of(blockIdx.x, tiles_x, tiles_y), H, W);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();                    // the previous tile's halo has been read by every wave
        halo_store(hv, hs, FP, FC);
        __syncthreads();
        if (t + (int)gridDim.x < ntiles) halo_load(hv, obs, tile_of(t + gridDim.x, tiles_x, tiles_y), H, W);
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < KF / 2; ++s) {
            const float a = arow[lh ? halo_off(2 * s + 1, FP, FC) : halo_off(2 * s, FP, FC)];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb0[s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb1[s], acc1, 0, 0, 0);
        }
        // ---- epilogue through the wave's own LDS patch [32 px][64 + 4]: float4 runs of a pixel's channels (conv_fwd_kernel's form)
        const Tile q = tile_of(t, tiles_x, tiles_y);
        const int y = q.y0 + wave;
        __builtin_amdgcn_wave_barrier();    // the patch reads of the previous tile are done
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int px = (r & 3) + 8 * (r >> 2) + 4 * lh;
            patch[px * (CO + 4) + li] = acc0[r];
            patch[px * (CO + 4) + 32 + li] = acc1[r];
        }
        __builtin_amdgcn_wave_barrier();
        if (y < H) {
#pragma unroll
            for (int ps = 0; ps < 8; ++ps) {
                const int px = ps * 4 + px0, x = q.x0 + px;
                if (x >= W) continue;
                float4 v = *reinterpret_cast<const float4*>(patch + px * (CO + 4) + c4 * 4);
                v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
                if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                *reinterpret_cast<float4*>(Y + (((size_t)q.b * H + y) * W + x) * CO + c4 * 4) = v;
            }
        }
    }
}

// W[co][3][5][5] -> [k = tap * 3 + ci][co], k < 76 (row 75 zero)
__global__ void conv_first_pack_kernel(const float* __restrict__ W, float* __restrict__ pack) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= KF * CO) return;
    const int co = i % CO, k = i / CO, tap = k / CI, ci = k - tap * CI;
    pack[i] = k < KR ? W[((size_t)co * CI + ci) * KS * KS + tap] : 0.f;
}

__global__ __launch_bounds__(256, 2) void conv_first_wgrad_kernel(const float* __restrict__ obs, const float* __restrict__ dY, float* __restrict__ part,
                                                                  int B, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* dYs = smem;                      // [TH*TW][CO]; after the last tile: the workgroup's slab [CO][KG] and the waves' bias sums [4][CO]
    float* hs = smem + TH * TW * CO;        // planar halo, pitches GP / GC
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH, ntiles = tiles_x * tiles_y * B;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;

    f32x16 acc[2][3];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[h][c][r] = 0.f;
    float bs0 = 0.f, bs1 = 0.f;

    constexpr int FY = CO / 4, NDY = TH * TW * FY / 256;
    float4 rdy[NDY];
    float hv[NH];
    auto gload = [&](int t) {
        const Tile q = tile_of(t, tiles_x, tiles_y);
        const float* gy = dY + (size_t)q.b * H * W * CO;
#pragma unroll
        for (int i = 0; i < NDY; ++i) {
            const int idx = threadIdx.x + i * 256;
            const int c4 = idx % FY, pp = idx / FY;
            const int x = q.x0 + (pp % TW), y = q.y0 + (pp / TW);
            rdy[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y < H && x < W) rdy[i] = *reinterpret_cast<const float4*>(gy + ((size_t)y * W + x) * CO + c4 * 4);
        }
        halo_load(hv, obs, q, H, W);
    };
    // this wave's row of the tile; pixel pair j holds pixels 2j + lh
    const float* ay = dYs + (wave * TW + lh) * CO + li;
    const float* b0 = hs + wave * GP + lh + halo_off(li, GP, GC);
    const float* b1 = hs + wave * GP + lh + halo_off(32 + li, GP, GC);
    const float* b2 = hs + wave * GP + lh + halo_off(64 + li, GP, GC);

    if ((int)blockIdx.x < ntiles) gload(blockIdx.x);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();                    // previous tile fully consumed
#pragma unroll
        for (int i = 0; i < NDY; ++i) {
            const int idx = threadIdx.x + i * 256;
            *reinterpret_cast<float4*>(dYs + (idx / FY) * CO + (idx % FY) * 4) = rdy[i];
        }
        halo_store(hv, hs, GP, GC);
        __syncthreads();
        if (t + (int)gridDim.x < ntiles) gload(t + gridDim.x);
#pragma unroll 4
        for (int xx = 0; xx < TW; xx += 2) {
            const float a0 = ay[xx * CO], a1 = ay[xx * CO + 32];
            const float x0 = b0[xx], x1 = b1[xx], x2 = b2[xx];
            bs0 += a0; bs1 += a1;
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, x0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, x0, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, x1, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, x1, acc[1][1], 0, 0, 0);
            acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, x2, acc[0][2], 0, 0, 0);
            acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, x2, acc[1][2], 0, 0, 0);
        }
    }
    // ---- the four waves (tile rows) into one slab, in wave order: ((w0 + w1) + w2) + w3
    float* slab = smem;                     // [CO][KG]
    float* bsw = smem + CO * KG;            // [4][CO]
    const float o0 = __shfl_down(bs0, 32), o1 = __shfl_down(bs1, 32);
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = h * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        float* d = slab + co * KG + c * 32 + li;
                        *d = w == 0 ? acc[h][c][r] : *d + acc[h][c][r];
                    }
            if (lh == 0) { bsw[w * CO + li] = bs0 + o0; bsw[w * CO + 32 + li] = bs1 + o1; }      // even pixels + odd pixels
        }
    }
    __syncthreads();
    float* out = part + (size_t)blockIdx.x * SLAB;
    for (int i = threadIdx.x; i < CO * KG; i += 256) out[i] = slab[i];
    if (threadIdx.x < CO) out[CO * KG + threadIdx.x] = ((bsw[threadIdx.x] + bsw[CO + threadIdx.x]) + bsw[2 * CO + threadIdx.x]) + bsw[3 * CO + threadIdx.x];
}

// dW[co][ci][ky][kx] = sum_slabs part[slab][co][tap * 3 + ci], db[co] = sum_slabs part[slab][CO * KG + co].  A workgroup takes RO outputs;
// its RG thread groups each sum a contiguous run of slabs in slab order, and the RG sums are added in group order.
__global__ __launch_bounds__(256) void conv_first_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dW, float* __restrict__ db,
                                                                      int nslab, int accumulate) {
    __shared__ float red[RG][RO];
    const int o = threadIdx.x % RO, g = threadIdx.x / RO;
    const int i = blockIdx.x * RO + o;                      // output: [0, 64 * 75) dW as (co, k), then 64 of db
    const bool live = i < CO * KR + CO;
    const int co = i < CO * KR ? i / KR : i - CO * KR, k = i < CO * KR ? i - co * KR : 0;
    const int src = i < CO * KR ? co * KG + k : CO * KG + co;
    const int per = (nslab + RG - 1) / RG, s0 = g * per, s1 = s0 + per < nslab ? s0 + per : nslab;
    float s = 0.f;
    if (live)
#pragma unroll 8
        for (int sl = s0; sl < s1; ++sl) s += part[(size_t)sl * SLAB + src];
    red[g][o] = s;
    __syncthreads();
    if (g != 0 || !live) return;
    float v = red[0][o];
#pragma unroll
    for (int j = 1; j < RG; ++j) v += red[j][o];
    float* d;
    if (i < CO * KR) {
        const int tap = k / CI, ci = k - tap * CI;
        d = dW + ((size_t)co * CI + ci) * KS * KS + tap;
    } else {
        if (!db) return;
        d = db + co;
    }
    *d = accumulate ? *d + v : v;
}

size_t conv_first_pack_floats() { return (size_t)KF * CO; }
int conv_first_pack_launch(const float* W, float* pack, hipStream_t st) {
    hipLaunchKernelGGL(conv_first_pack_kernel, GRID1D(KF * CO), 0, st, W, pack);
    OCRL_CHECK_LAUNCH("conv_first_pack");
    return 0;
}

int conv_first_fwd_launch(const float* obs, const float* pack, const float* bias, float* Y, int B, int H, int W, int relu, hipStream_t st) {
    OCRL_REQUIRE(B > 0 && H > 0 && W > 0, "conv first: empty input");
    OCRL_REQUIRE(aligned16(Y, bias), "conv first: Y and bias must be 16-byte aligned");
    OCRL_REQUIRE((long long)B * cdiv(H, TH) * cdiv(W, TW) < (1ll << 31), "conv first: too many tiles");
    // as many workgroups as are co-resident, each walking its tiles with the weights held in registers
    static int resident = 0;
    if (!resident) {
        int dev = 0, cus = 0, per = 0;
        OCRL_HIP(hipGetDevice(&dev));
        OCRL_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        OCRL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, conv_first_fwd_kernel, 256, 0));
        resident = cus * (per > 0 ? per : 1);
    }
    const int ntiles = cdiv(W, TW) * cdiv(H, TH) * B;
    const int grid = ntiles < resident ? ntiles : resident;
    const int pi = prof_begin(PROF_CONV_OTHER, st);
    hipLaunchKernelGGL(conv_first_fwd_kernel, dim3(grid), dim3(256), 0, st, obs, pack, bias, Y, B, H, W, relu);
    prof_end(pi, st);
    OCRL_CHECK_LAUNCH("conv_first_fwd_kernel");
    return 0;
}

int conv_first_wgrad_workers(int B, int H, int W) {
    const long long ntiles = (long long)cdiv(W, TW) * cdiv(H, TH) * B;
    return ntiles < WORKERS ? (int)ntiles : WORKERS;
}
size_t conv_first_wgrad_ws_floats(int B, int H, int W) { return (size_t)conv_first_wgrad_workers(B, H, W) * SLAB; }

int conv_first_wgrad_launch(const float* obs, const float* dY, float* ws, float* dW, float* db, int B, int H, int W, int accumulate, hipStream_t st) {
    OCRL_REQUIRE(B > 0 && H > 0 && W > 0, "conv first wgrad: empty input");
    OCRL_REQUIRE(aligned16(dY), "conv first wgrad: dY must be 16-byte aligned");
    OCRL_REQUIRE((long long)B * cdiv(H, TH) * cdiv(W, TW) < (1ll << 31), "conv first wgrad: too many tiles");
    constexpr int smem = (TH * TW * CO + GHALO) * 4;
    static_assert(TH * TW * CO >= CO * KG + 4 * CO, "the slab and the bias sums reuse the dY tile");
    static bool attr_set = false;
    if (!attr_set) {
        OCRL_HIP(hipFuncSetAttribute((const void*)conv_first_wgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr_set = true;
    }
    const int nw = conv_first_wgrad_workers(B, H, W);
    hipLaunchKernelGGL(conv_first_wgrad_kernel, dim3(nw), dim3(256), smem, st, obs, dY, ws, B, H, W);
    OCRL_CHECK_LAUNCH("conv_first_wgrad_kernel");
    hipLaunchKernelGGL(conv_first_wgrad_reduce_kernel, dim3(cdiv(CO * KR + CO, RO)), dim3(256), 0, st, ws, dW, db, nw, accumulate);
    OCRL_CHECK_LAUNCH("conv_first_wgrad_reduce");
    return 0;
}
