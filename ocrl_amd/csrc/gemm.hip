// fp32 GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, gfx950) with fused epilogues.
//
//   C[m,n] = epi( alpha * sum_k A(m,k) * B(k,n) )
//
// Operand storage is selected per operand:
//   AKC : A stored [M,K] (k contiguous, lda)        else A stored [K,M] (m contiguous, lda)
//   BKC : B stored [N,K] (k contiguous, ldb)        else B stored [K,N] (n contiguous, ldb)
// which covers  y = x W^T (AKC,BKC),  dx = dy W (AKC,!BKC),  dW = dy^T x (!AKC,!BKC).
//
// 256 threads = 4 waves in a 2x2 grid; each wave owns (BM/2)x(BN/2) as 32x32 MFMA tiles.
// K is consumed in 32-wide tiles, double-buffered in LDS with register prefetch (one barrier
// per k-tile).  Within a tile, the k index fed to MFMA step j by lane-half h is  8*c + 4*h + j
// for both operands, so a k-contiguous operand is one ds_read_b128 per 32 rows per 8 k.
// The kernel and its tile dispatch live in gemm_impl.h, compiled per operand-layout family (gemm_tt.hip: A [M,K] x B [N,K];
// gemm_tn.hip: A [M,K] x B [K,N]; gemm_nn.hip: A [K,M]); this file checks the arguments, selects the kernel (gemm_plan) and owns the split-k reduction.
// It also holds the Linear layers every model and unit runs on the GEMM (lin_fwd / lin_bwd_x / lin_bwd_w) and the one rule that splits
// their weight gradients over the rows (lin_splitk_count).
#include "common.h"
#include "kernels.h"
#include "switches.h"

int gemm_launch_tt(const GemmArgs& a, const GemmPlan& p, hipStream_t st);
int gemm_launch_tn(const GemmArgs& a, const GemmPlan& p, hipStream_t st);
int gemm_launch_nn(const GemmArgs& a, const GemmPlan& p, hipStream_t st);

// out[i] = (accumulate ? out[i] : 0) + sum_s part[s*stride + i]   (n % 4 == 0)
// block = 16 float4 columns x 16 split lanes: the slabs are read in parallel and combined through LDS.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, long long n4,
                                                            int splits, long long stride, int accumulate) {
    __shared__ float4 red[16][16];
    const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const long long i = (long long)blockIdx.x * 16 + cl;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n4) {
        int k = sl;
        for (; k + 48 < splits; k += 64) {          // four slabs in flight per thread
            const float4 v0 = *reinterpret_cast<const float4*>(part + (size_t)k * stride + i * 4);
            const float4 v1 = *reinterpret_cast<const float4*>(part + (size_t)(k + 16) * stride + i * 4);
            const float4 v2 = *reinterpret_cast<const float4*>(part + (size_t)(k + 32) * stride + i * 4);
            const float4 v3 = *reinterpret_cast<const float4*>(part + (size_t)(k + 48) * stride + i * 4);
            s.x += (v0.x + v1.x) + (v2.x + v3.x); s.y += (v0.y + v1.y) + (v2.y + v3.y);
            s.z += (v0.z + v1.z) + (v2.z + v3.z); s.w += (v0.w + v1.w) + (v2.w + v3.w);
        }
        for (; k < splits; k += 16) {
            const float4 v = *reinterpret_cast<const float4*>(part + (size_t)k * stride + i * 4);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    red[sl][cl] = s;
    __syncthreads();
    if (sl == 0 && i < n4) {
        float4 t = accumulate ? *reinterpret_cast<const float4*>(out + i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 16; ++k) { t.x += red[k][cl].x; t.y += red[k][cl].y; t.z += red[k][cl].z; t.w += red[k][cl].w; }
        *reinterpret_cast<float4*>(out + i * 4) = t;
    }
}

// development overrides (switches.h): OCRL_GEMM_TILE forces one tile shape where that family builds it, OCRL_GEMM_SB the buffering
static int env_tile() { return (int)sw::process<sw::OCRL_GEMM_TILE>(); }
static int env_sb() { return (int)sw::process<sw::OCRL_GEMM_SB>(); }
// tile shapes instantiated in gemm_impl.h for an operand layout (128x192 only where A is k-contiguous or B is n-contiguous)
static bool tile_built(int tile, int akc, int bkc) {
    return tile == 128128 || tile == 128064 || tile == 64128 || tile == 64064 || (tile == 128192 && (akc || !bkc));
}

int gemm_plan(const GemmArgs& a, GemmPlan* plan) {
    OCRL_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "gemm: empty problem %d %d %d", a.M, a.N, a.K);
    OCRL_REQUIRE(a.batch >= 1 && a.splitk >= 1, "gemm: bad batch/splitk");
    if (a.akc) OCRL_REQUIRE(a.K % 4 == 0 && a.lda % 4 == 0, "gemm: A k-contiguous needs K,lda %% 4 == 0 (K=%d lda=%d)", a.K, a.lda);
    else OCRL_REQUIRE(a.M % 4 == 0 && a.lda % 4 == 0, "gemm: A m-contiguous needs M,lda %% 4 == 0 (M=%d lda=%d)", a.M, a.lda);
    if (a.bkc) OCRL_REQUIRE(a.K % 4 == 0 && a.ldb % 4 == 0, "gemm: B k-contiguous needs K,ldb %% 4 == 0 (K=%d ldb=%d)", a.K, a.ldb);
    else OCRL_REQUIRE(a.N % 4 == 0 && a.ldb % 4 == 0, "gemm: B n-contiguous needs N,ldb %% 4 == 0 (N=%d ldb=%d)", a.N, a.ldb);
    OCRL_REQUIRE(((uintptr_t)a.A & 15) == 0 && ((uintptr_t)a.B & 15) == 0, "gemm: operands must be 16-byte aligned");
    OCRL_REQUIRE((a.sA % 4) == 0 && (a.sB % 4) == 0 && (a.sAi % 4) == 0 && (a.sBi % 4) == 0, "gemm: batch strides must be multiples of 4");
    OCRL_REQUIRE(a.batch_inner >= 1 && a.batch % a.batch_inner == 0, "gemm: batch must be a multiple of batch_inner");
    OCRL_REQUIRE(a.splitk == 1 || a.batch == 1, "gemm: split-k with batches is not supported");
    if (a.splitk > 1) OCRL_REQUIRE(a.sCsplit >= (long long)(a.M - 1) * a.ldc + a.N, "gemm: split-k slab stride too small");
    if (a.adrop_p > 0.f) OCRL_REQUIRE(a.adrop_ld > 0 && a.adrop_ld % 4 == 0 && a.batch == 1, "gemm: A-dropout needs adrop_ld %% 4 == 0 and no batching");
    if (a.bias_out) OCRL_REQUIRE(!a.akc && (a.splitk == 1 || a.sBias >= a.M), "gemm: fused bias gradient needs the dW form");
    OCRL_REQUIRE(!(a.a_mode || a.b_mode) || (a.batch == 1 && a.adrop_p == 0.f && a.x_lse && (a.a_mode != 3 || a.x_tok) &&
                 (a.a_mode == 0 || a.a_mode == 2 || a.a_mode == 3) && (a.b_mode == 0 || a.b_mode == 2)), "gemm: bad operand transform arguments");
    OCRL_REQUIRE(a.force_sb >= -1 && a.force_sb <= 1, "gemm: force_sb must be -1, 0 or 1 (got %d)", a.force_sb);
    GemmPlan p;
    p.layout = 2 * (a.akc ? 1 : 0) + (a.bkc ? 1 : 0);
    if (a.epi_mode) {
        OCRL_REQUIRE(a.akc && a.batch == 1 && a.splitk == 1 && !a.a_mode && !a.b_mode && a.adrop_p == 0.f && a.relu == 0 && a.drop_p == 0.f && !a.resid,
                     "gemm: soft-max epilogue needs a plain k-contiguous A, no split-k / batches / activation");
        OCRL_REQUIRE((a.N & 3) == 0 && (a.ldc & 3) == 0 && (((uintptr_t)a.C) & 15) == 0 && (!a.bias || (((uintptr_t)a.bias) & 15) == 0),
                     "gemm: soft-max epilogue needs N, ldc multiples of 4 and 16-byte aligned C / bias");
        if (a.epi_mode == 1 || a.epi_mode == 2) {
            OCRL_REQUIRE(a.bkc && a.stat && !a.mask && gemm_stat_segments(a.N) <= 64, "gemm: soft-max statistics need a k-contiguous B, a stat buffer and N <= 4096");
            if (a.epi_mode == 2) {
                OCRL_REQUIRE(a.hstat && a.hidx && (a.e1 == nullptr) == (a.e2 == nullptr) && a.ldc == a.N, "gemm: Gumbel head arguments");
                OCRL_REQUIRE(!a.e1 || ((((uintptr_t)a.e1) | ((uintptr_t)a.e2)) & 15) == 0, "gemm: Gumbel noise must be 16-byte aligned");
            }
        } else {
            OCRL_REQUIRE(a.epi_mode == 3 && !a.bkc && a.mask && a.e_lse && a.e_rowvec && !a.bias && (a.ldmask & 3) == 0 && (((uintptr_t)a.mask) & 15) == 0,
                         "gemm: soft-max backward epilogue arguments");
        }
        // the soft-max epilogues are built for single-buffered 128x128 tiles only; the environment overrides do not apply to them
        OCRL_REQUIRE((a.force_tile == 0 || a.force_tile == 128128) && a.force_sb != 0,
                     "gemm: soft-max epilogue %d is built for single-buffered 128x128 tiles only", a.epi_mode);
        p.bm = 128; p.bn = 128; p.sb = 1; p.epi = a.epi_mode;
        *plan = p;
        return 0;
    }
    if (a.a_mode || a.b_mode) {
        OCRL_REQUIRE(a.akc || !a.bkc, "gemm: operand transforms are not built for akc=0 bkc=1");
        p.xf = 2;
    } else if (a.adrop_p > 0.f) {
        p.xf = 1;
    }
    int tile = 0, sb = -1;
    if (a.force_tile) {
        OCRL_REQUIRE(tile_built(a.force_tile, a.akc, a.bkc), "gemm: tile %dx%d is not built for akc=%d bkc=%d", a.force_tile / 1000,
                     a.force_tile % 1000, a.akc, a.bkc);
        tile = a.force_tile;
    } else if (env_tile() && tile_built(env_tile(), a.akc, a.bkc)) {
        tile = env_tile();
    } else if (a.akc && a.N == 192 && a.K >= 1024 && a.M >= 4096) {
        // measured on MI355X (tools/bench_gemm.py): long-K activation x weight products with N = 192 (the model width), e.g. the
        // vocabulary-head dX: one 128x192 tile reads A once and moves 38 FLOP per staged byte instead of 21 (+7 % measured at K = 4096;
        // short K is faster on 128x64)
        tile = 128192;
    } else if (!a.akc && !a.bkc && a.N == 192 && a.K >= 4096) {
        // weight gradients with 192 input features (dW = dY^T X over >= 10^5 rows, split-K): a 128x192 tile reads X once per split
        // (PMC: the 128x64 tiling moved 643 MB per launch for 201 MB of operands); single LDS buffer to keep two workgroups per CU
        tile = 128192;
        sb = 1;
    } else if (a.N % 128 == 0) {
        // 128-wide column tiles only pay when N is a multiple of 128; N = 192 / 64 (projections, weight gradients with 192 inputs)
        // run 10-20 % faster on 128x64 tiles
        tile = a.M > 64 ? 128128 : 64128;
    } else {
        tile = a.M > 64 ? 128064 : 64064;
    }
    if (a.force_sb >= 0) {
        sb = a.force_sb;
    } else if (sb < 0) {
        // measured (tools/bench_gemm.py): a single LDS buffer (twice the resident workgroups) wins for the short-K forward / dX forms
        // (+8..37 %); the long split-K weight-gradient loops keep the double buffer
        const int mode = env_sb();
        sb = (mode == 1 || (mode == 0 && a.akc)) ? 1 : 0;
    }
    p.bm = tile / 1000; p.bn = tile % 1000; p.sb = sb;
    *plan = p;
    return 0;
}

int gemm_launch(const GemmArgs& a, hipStream_t st) {
    GemmPlan p;
    if (gemm_plan(a, &p)) return 1;
    if (a.akc && a.bkc) return gemm_launch_tt(a, p, st);
    if (a.akc) return gemm_launch_tn(a, p, st);
    return gemm_launch_nn(a, p, st);
}

int splitk_reduce_launch(const float* part, float* out, long long n, int splits, long long stride,
                         int accumulate, hipStream_t st) {
    OCRL_REQUIRE(n % 4 == 0 && stride % 4 == 0, "splitk_reduce: n and stride must be multiples of 4");
    const long long n4 = n / 4;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(cdiv(n4, 16)), dim3(256), 0, st, part, out, n4, splits, stride, accumulate);
    OCRL_CHECK_LAUNCH("splitk_reduce");
    return 0;
}

void gemm_splitk_layout(GemmArgs& a, float* ws, long long bslab) {
    const long long slab = (long long)a.M * a.N;
    a.C = ws; a.sCsplit = slab;
    if (a.bias_out) { a.bias_out = ws + a.splitk * slab; a.sBias = bslab; }
}

int gemm_splitk_launch(GemmArgs a, float* ws, long long bslab, int accumulate, hipStream_t st) {
    float* const C = a.C;
    float* const db = a.bias_out;
    gemm_splitk_layout(a, ws, bslab);
    RC(gemm_launch(a, st));
    RC(splitk_reduce_launch(ws, C, a.sCsplit, a.splitk, a.sCsplit, accumulate, st));
    if (db) RC(splitk_reduce_launch(a.bias_out, db, a.M, a.splitk, bslab, 0, st));      // the dW form has M % 4 == 0
    return 0;
}

// ---------------------------------------------------------------------------------------------- Linear layers
static void set_xf(GemmArgs& a, const Xf& xf) {
    a.a_mode = xf.a_mode; a.b_mode = xf.b_mode; a.x_lse = xf.lse; a.x_tok = xf.tok; a.x_scale = xf.scale;
}
static void set_adrop(GemmArgs& a, const Drop& dr, int ld) {
    if (dr.p > 0.f) { a.adrop_p = dr.p; a.adrop_site = dr.site; a.adrop_ld = ld; a.drop_seed = dr.seed; }
}

int lin_fwd(const float* x, int ldx, const float* W, const float* b, float* y, int ldy, long long M, int N, int K, int relu, const float* resid,
            int ldr, hipStream_t st, Drop dr) {
    GemmArgs a;
    a.A = x; a.B = W; a.C = y; a.M = (int)M; a.N = N; a.K = K; a.lda = ldx; a.ldb = K; a.ldc = ldy; a.akc = 1; a.bkc = 1;
    a.bias = b; a.relu = relu; a.resid = resid; a.ldr = ldr; a.drop_p = dr.p; a.drop_seed = dr.seed; a.drop_site = dr.site;
    return gemm_launch(a, st);
}

int lin_bwd_x(const float* dy, int ld_dy, const float* W, float* dx, int ldx, long long M, int N_out, int K_in, const float* mask, int ldmask,
              const float* resid, int ldr, hipStream_t st, Drop dr, Xf xf, float alpha) {
    GemmArgs a;
    a.A = dy; a.B = W; a.C = dx; a.M = (int)M; a.N = K_in; a.K = N_out; a.lda = ld_dy; a.ldb = K_in; a.ldc = ldx; a.akc = 1; a.bkc = 0;
    a.alpha = alpha; a.mask = mask; a.ldmask = ldmask; a.resid = resid; a.ldr = ldr;
    set_adrop(a, dr, N_out);
    set_xf(a, xf);
    return gemm_launch(a, st);
}

// Split count of the weight gradient `a` (the dW form: K = the rows): about 1024 workgroups over the output tiles gemm_plan cuts (measured
// on MI355X: counting the 128x192 tile as three 64-wide ones left 340 workgroups on 256 CUs, 0.95 waves per SIMD), at least 256 rows per
// split, at most max_splits (0: no limit), and no more splits than the scratch holds at one M*N slab plus one bias slab each (reserved
// whether or not the bias gradient is fused, so the count does not depend on it).
static int lin_splitk_count(const GemmArgs& a, size_t sk_floats, int max_splits, int* splits) {
    GemmPlan p;
    RC(gemm_plan(a, &p));
    long long s = 1024 / ((long long)cdiv(a.M, p.bm) * cdiv(a.N, p.bn));
    if (s > a.K / 256) s = a.K / 256;
    if (max_splits > 0 && s > max_splits) s = max_splits;
    const long long per = (long long)a.M * a.N + ((a.M + 3) & ~3);
    if (s * per > (long long)sk_floats) s = (long long)sk_floats / per;
    *splits = s > 1 ? (int)s : 1;
    return 0;
}

int lin_bwd_w(const float* dy, int ld_dy, const float* x, int ldx, float* dW, float* db, long long M, int N_out, int K_in, float alpha, float* sk,
              size_t sk_floats, hipStream_t st, Drop dr, Xf xf, int accumulate, int max_splits) {
    OCRL_REQUIRE(!(db && accumulate), "lin_bwd_w: a fused bias gradient is written, not accumulated");
    GemmArgs a;
    a.A = dy; a.B = x; a.C = dW; a.M = N_out; a.N = K_in; a.K = (int)M; a.lda = ld_dy; a.ldb = ldx; a.ldc = K_in; a.akc = 0; a.bkc = 0;
    a.alpha = alpha; a.bias_out = db;
    set_adrop(a, dr, N_out);
    set_xf(a, xf);
    int splits;
    RC(lin_splitk_count(a, sk_floats, max_splits, &splits));
    if (splits > 1) {
        a.splitk = splits;
        return gemm_splitk_launch(a, sk, (N_out + 3) & ~3, accumulate, st);
    }
    if (accumulate) { a.resid = dW; a.ldr = K_in; }
    return gemm_launch(a, st);
}
