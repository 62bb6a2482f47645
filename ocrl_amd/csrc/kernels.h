// Internal launcher declarations shared by the kernel translation units, the model
// orchestration (slate_model.cpp) and the C ABI (capi.cpp).  Not part of the public ABI.
#pragma once
#include "common.h"
#include "../../include/ocrl_hip.h"

// ------------------------------------------------------------------ prof.cpp
enum { PROF_CONV5 = 0, PROF_CONV_OTHER = 1, PROF_WGRAD = 2, PROF_GEMM = 3, PROF_SA_FWD = 4, PROF_SA_BWD = 5, PROF_ATTN_FWD = 6, PROF_ATTN_BWD = 7, PROF_NTAGS = 8 };
int prof_begin(int tag, hipStream_t st);
void prof_end(int idx, hipStream_t st);

// ------------------------------------------------------------------ gemm.hip
struct GemmArgs {
    const float* A = nullptr;
    const float* B = nullptr;
    float* C = nullptr;
    int M = 0, N = 0, K = 0;
    int lda = 0, ldb = 0, ldc = 0;
    int akc = 1, bkc = 1;                 // operand storage, see gemm.hip
    int batch = 1;                        // total batches; batch index z -> (z / batch_inner, z % batch_inner)
    int batch_inner = 1;
    long long sA = 0, sB = 0, sC = 0;     // outer batch strides (elements)
    long long sAi = 0, sBi = 0, sCi = 0;  // inner batch strides (e.g. attention heads inside a [B,T,d] tensor)
    int splitk = 1;
    long long sCsplit = 0;                // slab stride when splitk > 1 (raw alpha*acc partials)
    // epilogue (ignored when splitk > 1):  v = alpha*acc + bias[n]; relu; dropout; *(mask>0); + resid
    float alpha = 1.f;
    const float* bias = nullptr;
    int relu = 0;                         // 0 none, 1 ReLU, 2 ELU
    float drop_p = 0.f;
    unsigned long long drop_seed = 0;
    unsigned drop_site = 0;
    const float* mask = nullptr; int ldmask = 0; long long sMask = 0;
    int mask_elu = 0;                     // mask holds ELU outputs: v *= (m > 0 ? 1 : m + 1) instead of the ReLU gate
    const float* resid = nullptr; int ldr = 0; long long sR = 0;
    // A-operand dropout (backward of y = x + dropout(branch)): A element (m, n) of the logical row-major [rows, adrop_ld]
    // tensor is multiplied by keep/(1-p) of dropout site adrop_site while it is staged (no separate mask pass)
    float adrop_p = 0.f; unsigned adrop_site = 0; int adrop_ld = 0;
    // fused bias gradient for the dW form (akc == 0): bias_out[m] = sum_k A(m,k)  (partials per split at stride sBias)
    float* bias_out = nullptr; long long sBias = 0;
    // ---- soft-max heads fused into the product (the [rows, vocabulary] tensor is written once and never re-read by an elementwise pass)
    // operand transforms, applied while an operand tile is staged; `row` is the token row (the m index of a k-contiguous A, the k index
    // of an m/n-contiguous A or B), `col` the vocabulary index:
    //   2: exp(x - x_lse[row])                                    (soft-max probabilities rebuilt from the stored scores)
    //   3: (exp(x - x_lse[row]) - [col == x_tok[row]]) * x_scale  (cross-entropy gradient rebuilt from the stored logits; A only)
    int a_mode = 0, b_mode = 0;
    const float* x_lse = nullptr; const int* x_tok = nullptr; float x_scale = 1.f;
    // epilogue modes (128x128 tiles, k-contiguous A, N % 4 == 0, no split-k / batches):
    //   1: C = alpha*acc (+bias) and per (row, 64-column segment) soft-max statistics  stat[(row*nseg + seg)*2 + {0,1}] = (max, sum exp(v - max))
    //   2: Gumbel head: l = acc + bias;  C = (l + g1) * e_scale  with statistics as in 1;  the hard sample's segment maximum of
    //      l + g2 and its column go to hstat / hidx.  g = -log(E + tiny), E from e1 / e2 (injected Exp(1) noise, [M,N]) or
    //      from the counter RNG (e_seed, the same draws as gumbel_softmax_kernel)
    //   3: soft-max backward: C = exp(mask - e_lse[row]) * (acc - e_rowvec[row]) * e_scale   (mask = the stored scores; C may alias mask)
    int epi_mode = 0;
    float* stat = nullptr; float* hstat = nullptr; int* hidx = nullptr;
    const float* e1 = nullptr; const float* e2 = nullptr; unsigned long long e_seed = 0;
    const float* e_lse = nullptr; const float* e_rowvec = nullptr; float e_scale = 1.f;
    // per-call dispatch choice (unit tests; no model call sets them): force_tile 0 = the rule, else BM*1000+BN (as OCRL_GEMM_TILE);
    // force_sb -1 = the rule, 0 = double-buffered LDS, 1 = single.  They take precedence over the environment overrides, and a
    // combination that is not built is an error, never a silent fall-back.
    int force_tile = 0;
    int force_sb = -1;
};
inline int gemm_stat_segments(int N) { return 2 * ((N + 127) / 128); }
// The kernel gemm_launch runs for a set of arguments: gemm_kernel<bm, bn, akc, bkc, sb, xf, epi>, layout = 2*akc + bkc
// (3: A [M,K] x B [N,K], 2: A [M,K] x B [K,N], 1: A [K,M] x B [N,K], 0: A [K,M] x B [K,N]).
struct GemmPlan { int bm = 0, bn = 0, sb = 0, xf = 0, epi = 0, layout = 0; };
// Checks the arguments and selects the kernel (host only); 0, or 1 with the message in ocrl_last_error().  gemm_launch uses it, so
// what it reports is what runs.
int gemm_plan(const GemmArgs& a, GemmPlan* plan);
int gemm_launch(const GemmArgs& a, hipStream_t st);
int splitk_reduce_launch(const float* part, float* out, long long n, int splits, long long stride,
                         int accumulate, hipStream_t st);
// split-k workspace: a.splitk slabs of the raw C [M,N] partials from ws, then (with a fused bias gradient) a.splitk slabs of the bias
// partials at stride bslab: points C / bias_out into ws
void gemm_splitk_layout(GemmArgs& a, float* ws, long long bslab);
// runs a.splitk partial products into that layout, then reduces the slabs into C (added to it when `accumulate`) and the bias partials
// into bias_out.  C must be compact (ldc == N).
int gemm_splitk_launch(GemmArgs a, float* ws, long long bslab, int accumulate, hipStream_t st);

// ---- Linear layers on the GEMM (every model and unit): forward NT, input gradient NN, weight gradient TN split over the rows
// dropout at (seed, site) with probability p: forward on the output, backward on dy as the product stages it
struct Drop { float p = 0.f; unsigned long long seed = 0; unsigned site = 0; };
// soft-max operand transform of a product (GemmArgs::a_mode / b_mode): the operand is rebuilt from stored scores + per-row log-sum-exp
struct Xf { int a_mode = 0, b_mode = 0; const float* lse = nullptr; const int* tok = nullptr; float scale = 1.f; };
// y[M,N] = drop(act(x[M,K] W[N,K]^T + b)) + resid          (act: GemmArgs::relu)
int lin_fwd(const float* x, int ldx, const float* W, const float* b, float* y, int ldy, long long M, int N, int K, int relu, const float* resid,
            int ldr, hipStream_t st, Drop dr = Drop());
// dx[M,K_in] = alpha * (drop(dy)[M,N_out] W[N_out,K_in]) * (mask > 0) + resid
int lin_bwd_x(const float* dy, int ld_dy, const float* W, float* dx, int ldx, long long M, int N_out, int K_in, const float* mask, int ldmask,
              const float* resid, int ldr, hipStream_t st, Drop dr = Drop(), Xf xf = Xf(), float alpha = 1.f);
// dW[N_out,K_in] = alpha * drop(dy)^T x (added to dW when `accumulate`);  db[N_out] = column sums of drop(dy), fused into the product
// (nullptr: none).  Split over the M rows through the scratch (sk, sk_floats) as lin_splitk_count in gemm.hip decides; sk_floats = 0 never splits.
int lin_bwd_w(const float* dy, int ld_dy, const float* x, int ldx, float* dW, float* db, long long M, int N_out, int K_in, float alpha, float* sk,
              size_t sk_floats, hipStream_t st, Drop dr = Drop(), Xf xf = Xf(), int accumulate = 0, int max_splits = 0);

// ------------------------------------------------------------------ pool.hip
int pool_embed_launch(const float* lin, const float* cls, const float* pos, float* x0, int B, int K, int d, hipStream_t st);
int pool_rows_launch(const float* in, float* out, int B, int K, int d, int mode, hipStream_t st);
int pool_attn_launch(const float* qkv, float* P, float* O, const float* dO, float* dqkv, int B, int S, int d, int h, float p, unsigned long long seed,
                     unsigned site, int backward, hipStream_t st);
// host only: every shape limit of pool_attn in one direction (0 = runs; else the reason is the error text), its LDS request, and
// whether the short path runs (K slots of width Din, d_model, nhead) in both directions
int pool_attn_check(int B, int S, int d, int h, int backward);
size_t pool_attn_lds_bytes(int S, int d, int h, int backward);
int pool_short_check(int K, int Din, int d, int h);

// ------------------------------------------------------------------ pool_long.hip (long token sequences: include/ocrl_hip.h ocrl_pool_transformer_long_*)
int pool_cols_launch(const float* src, int lds, float* dst, int ldd, long long rows, int ncols, int ncopy, hipStream_t st);
int pool_cls_drop_launch(const float* x, const float* resid, int ldr, float* out, int B, int N, int S, float p, unsigned long long seed, unsigned site,
                         hipStream_t st);
int pool_cls_add_launch(float* dX, const float* v, int B, int d, int S, hipStream_t st);
int pool_cls_nchunk(int B, int S, int* chunk);     // position chunks per image of the CLS-row attention
struct PoolClsArgs {                                // attention of the CLS row of the last layer over the S rows of X (pool_long.hip)
    const float* X = nullptr;                       // [B][S][d] layer input
    const float* Win = nullptr; const float* bin = nullptr;   // in_proj weight [3d][d], bias [3d]
    const float* q = nullptr;                       // [B][d] query of row 0 (bias included)
    float* U = nullptr;                             // [B][h][d]
    float* part = nullptr;                          // [B][nchunk][h][d + 4] partial blocks (forward), [B][nchunk][h][d] (backward)
    float* z = nullptr;                             // [B][h][d] sum_j p'_hj x_j
    float* stat = nullptr;                          // [B][h][2] (sum_j p'_hj, log-sum-exp of the scores)
    float* o = nullptr;                             // [B][d] attention output (before out_proj)
    const float* dO = nullptr;                      // backward: [B][d] gradient of o
    float* G = nullptr; float* gD = nullptr;        // [B][h][d], [B][h][2]
    float* dX = nullptr;                            // [B][S][d] gradient of X through k and v (row 0's q part is added by the caller)
    float* w = nullptr; float* dq = nullptr;        // [B][h][d] sum_j ds_hj x_j, [B][d]
    const float* x0 = nullptr;                      // [B][d] row 0 of X
    float* dW = nullptr; float* db = nullptr;       // in_proj gradients
    int B = 0, S = 0, d = 0, h = 0;
    float p = 0.f; unsigned long long seed = 0; unsigned site = 0;
};
int pool_cls_attn_fwd_launch(const PoolClsArgs& a, hipStream_t st);
int pool_cls_attn_bwd_launch(const PoolClsArgs& a, hipStream_t st);
// non-causal multi-head attention over all rows: forward O, lse [B*h][S]; backward dqkv from dO (Dd: [B*h][S] scratch)
int pool_flash_launch(const float* qkv, float* O, float* lse, const float* dO, float* Dd, float* dqkv, int B, int S, int d, int h, float p,
                      unsigned long long seed, unsigned site, int backward, hipStream_t st);

// ------------------------------------------------------------------ rn.hip (Relation Network pooling: include/ocrl_hip.h ocrl_pool_rn_*)
int rn_pair_fwd_launch(const float* AB, const float* b1, float* h1, int B, int K, int g, hipStream_t st);
int rn_pair_bwd_launch(const float* dh1, float* dAB, int B, int K, int g, hipStream_t st);
int rn_pairsum_fwd_launch(const float* gL, float* y, int B, int P, int g, hipStream_t st);
int rn_pairsum_bwd_launch(const float* dy, const float* gL, float* dgL, int B, int P, int g, hipStream_t st);

// ------------------------------------------------------------------ naturecnn.hip (NatureCNN / MultipleCNN: include/ocrl_hip.h ocrl_naturecnn_*)
// element offset of (image b, group g, channel c, row h, column w) in a map
struct NcMap { long long sN = 0, sG = 0, sC = 0, sH = 0, sW = 0; };
struct NcFwdArgs {
    const float* X = nullptr; NcMap x;             // layer input, cin channels per group (x.sG = 0: every group reads the same channels)
    float* Y = nullptr; float* Y2 = nullptr; NcMap y;   // relu(conv + bias), cout channels per group; Y2 (optional) gets a second copy
    const float* w[OCRL_NATURECNN_MAX_GROUPS] = {}; const float* bias[OCRL_NATURECNN_MAX_GROUPS] = {};   // [cout, cin, ks, ks], [cout]
    int B = 0, G = 1, cin = 0, cout = 0, H = 0, W = 0, OH = 0, OW = 0, ks = 0, stride = 0;
    int pad = 0;                                   // zero padding on every side (VAE decoder: 3 x 3, pad 1)
};
struct NcBwdArgs {
    const float* X = nullptr; NcMap x;             // layer input; also the ReLU mask of dX
    const float* dY = nullptr; NcMap dy;           // gradient of the pre-activation of this layer
    float* dX = nullptr;                           // masked gradient of the lower layer's pre-activation, layout x (NULL: not wanted)
    float* part = nullptr;                         // [slabs][G][cout][cin ks ks + 1] weight / bias gradient partials
    int slabs = 1, slab_rows = 0;                  // the B OH OW rows in slabs of slab_rows (a multiple of 4)
    const float* w[OCRL_NATURECNN_MAX_GROUPS] = {};
    int B = 0, G = 1, cin = 0, cout = 0, H = 0, W = 0, OH = 0, OW = 0, ks = 0, stride = 0;
    int pad = 0;
    long long dw_tiles = 0, dx_tiles = 0; int dw_blocks = 0;   // set by nc_conv_bwd_launch
};
struct NcReduceLayer { const float* part = nullptr; int slabs = 0, G = 0, cout = 0, K = 0; long long n = 0; };
struct NcReduceArgs {
    NcReduceLayer L[OCRL_NATURECNN_MAX_CONVS];
    float* dw[OCRL_NATURECNN_MAX_CONVS][OCRL_NATURECNN_MAX_GROUPS] = {};
    float* db[OCRL_NATURECNN_MAX_CONVS][OCRL_NATURECNN_MAX_GROUPS] = {};
    int nlayers = 0;
};
int nc_conv_fwd_launch(const NcFwdArgs& a, hipStream_t st);
int nc_conv_bwd_launch(NcBwdArgs a, hipStream_t st);      // dW partials of the layer and, when a.dX, the masked data gradient: one launch
int nc_dw_reduce_launch(const NcReduceArgs& a, hipStream_t st);
int nc_relu_mask_launch(const float* d, const float* act, float* out, long long n, hipStream_t st);

// ------------------------------------------------------------------ pool_cnn.hip (first layer of the CNN pooling heads: include/ocrl_hip.h ocrl_pool_cnn_*)
// Conv2d(D, 32, k 8, s 4) + ReLU over channels-last tokens [B, H, W, D]; output and dY in the [B, 32, OH, OW] layout layer 2 reads
struct PcGeom {
    int OH = 0, OW = 0, OWT = 0;                   // output map; 16-column tiles per output row
    int NG = 0, nchunk = 0;                        // groups of 16 columns per half window row (4 D floats); steps of 4 groups
    size_t wp_floats = 0;                          // packed forward weight [8 nchunk][32][128]
    long long units = 0; int slab_units = 0, slabs = 0; size_t part_floats = 0;   // dW: (image, output row, tile) units in slabs
    int passes = 0, nbg = 0, Dp = 0; size_t wd_floats = 0;                         // dX: channel passes, blocks per pass, padded D
    int HB = 0, WB = 0, WT = 0; long long dx_units = 0; int upw = 0;               // dX: (image, row quad, 16 column quads) units per workgroup
};
PcGeom pc_geom(int B, int H, int W, int D);
struct PcFwdArgs {
    const float* X = nullptr; const float* Wp = nullptr; const float* bias = nullptr; float* Y = nullptr;
    int B = 0, H = 0, W = 0, D = 0, OH = 0, OW = 0, OWT = 0, nchunk = 0, NG = 0;
};
struct PcDwArgs {
    const float* X = nullptr; const float* dY = nullptr; float* part = nullptr; float* partb = nullptr;
    int B = 0, H = 0, W = 0, D = 0, OH = 0, OW = 0, OWT = 0, nchunk = 0, slab_units = 0;
    long long units = 0;
};
struct PcDxArgs {
    const float* dY = nullptr; const float* Wd = nullptr; float* dX = nullptr;
    int H = 0, W = 0, D = 0, OH = 0, OW = 0, HB = 0, WT = 0, Dp = 0, passes = 0, upw = 0;
    long long units = 0, groups = 0;
};
// Wp: pc_geom().wp_floats of scratch (the weight is reordered per call); Y = relu(conv + bias)
int pc_conv1_fwd_launch(const float* X, const float* w, const float* bias, float* Wp, float* Y, int B, int H, int W, int D, hipStream_t st);
// part: pc_geom().part_floats; dY = gradient of the pre-activation; the reduce writes dw [32, D, 8, 8] and db [32]
int pc_conv1_dw_launch(const float* X, const float* dY, float* part, int B, int H, int W, int D, hipStream_t st);
int pc_conv1_dw_reduce_launch(const float* part, float* dw, float* db, int B, int H, int W, int D, hipStream_t st);
// Wd: pc_geom().wd_floats of scratch; dX [B, H, W, D], every element written
int pc_conv1_dx_launch(const float* dY, const float* w, float* Wd, float* dX, int B, int H, int W, int D, hipStream_t st);

// ------------------------------------------------------------------ probe.hip (slot property probe: include/ocrl_hip.h ocrl_probe_*)
#define PROBE_MAX_SLOTS 12      // 2^K assignment states per image in LDS
#define PROBE_MAX_PROPS 8
#define PROBE_MAX_WIDTH 256     // head outputs per slot / state entries per object
// property p reads targets from column t[p] (1 wide; 2 for xy) and head outputs [a[p], b[p]); kind: 0 = categorical, 1 = xy
struct ProbeSchema { int P; int t[PROBE_MAX_PROPS], a[PROBE_MAX_PROPS], b[PROBE_MAX_PROPS], kind[PROBE_MAX_PROPS]; };
int probe_schema_check(const ProbeSchema& sc, int T, int O);
int probe_match_check(int B, int K, int N, int T, int O);
// out[b, s, :] at b * ld_img + s * ld_row (dout alike; only its [K, O] entries are written).  part: [B, P + 2] scratch; metrics: [P + 2] =
// loss, per property acc / R^2, mse_xy.  cost [B, N, K], col [B, N], dout and dloss (device scalar, absent = 1) may be null.
int probe_match_launch(const float* out, int ld_row, long long ld_img, const float* y, const float* dloss, float* cost, int* col, float* part,
                       float* metrics, float* dout, int B, int K, int N, int T, int O, const ProbeSchema& sc, hipStream_t st);
int probe_leaky_fwd_launch(float* x, long long n, float slope, hipStream_t st);
int probe_leaky_bwd_launch(float* dx, const float* h, long long n, float slope, hipStream_t st);

// ------------------------------------------------------------------ vae.hip (VAE module: include/ocrl_hip.h ocrl_vae_*)
// pack = 1: dst (NHWC side) <- src (NCHW side); 0: the reverse.  rows = 1: the C HW index runs over rows of R columns, else columns
int vae_permute_launch(const float* src, float* dst, long long R, int C, int HW, int rows, int pack, hipStream_t st);
int vae_pad_rows_launch(const float* src, float* dst, int rows, int rows_pad, int K, hipStream_t st);
int vae_kl_fwd_launch(const float* ml, const float* eps, float* latent, float* part, float* rep, int B, int L, hipStream_t st);
int vae_loss_launch(const float* part, float* metrics, int B, float kld_weight, hipStream_t st);
int vae_kl_bwd_launch(const float* ml, const float* eps, const float* dlat, const float* drep, const float* dloss, float* dml, int B, int L,
                      float kld_weight, hipStream_t st);
int vae_scale_launch(const float* x, float* y, const float* g, long long n, hipStream_t st);
int vae_recon_nchw_launch(const float* r4, float* out, int B, int C, int HW, hipStream_t st);

// ------------------------------------------------------------------ mae.hip (masked autoencoder: include/ocrl_hip.h ocrl_mae_*)
#define MAE_MAX_PATCHES 1024    // a noise row is ranked in LDS
// ranks of noise [B, L], ties by index: restore [B, L] = rank, keep [B, len_keep] = the indices of ranks < len_keep, mask [B, L] = (rank >=
// len_keep); restore_out / mask_out (optional) get second copies
int mae_rank_launch(const float* noise, int* restore, int* keep, float* mask, int* restore_out, float* mask_out, int B, int L, int len_keep,
                    hipStream_t st);
// out [B n, 3 p p]: patch ids[b, i] (null: i) of obs [B, 3, S, S] in (c, ph, pw) order
int mae_patch_gather_launch(const float* obs, const int* ids, float* out, int B, int n, int S, int p, hipStream_t st, int force_scalar = 0);
// x0 [B, n + 1, D]: row 0 = cls + pos[0], row 1 + i = embed[b, i] + pos[1 + ids[b, i]] (null: i); backward: dembed [B n, D], dcls [D]
int mae_tokens_fwd_launch(const float* embed, const float* cls, const float* pos, const int* ids, float* x0, int B, int n, int D, hipStream_t st);
int mae_tokens_bwd_launch(const float* dx0, float* dembed, float* dcls, int B, int n, int D, hipStream_t st);
// xd [B, L + 1, Dd] from e [B, len_keep + 1, Dd]; backward: de, dmtok [Dd] (part: [B, Dd] scratch)
int mae_unshuffle_fwd_launch(const float* e, const float* mtok, const float* dpos, const int* restore, float* xd, int B, int L, int len_keep, int Dd,
                             hipStream_t st);
int mae_unshuffle_bwd_launch(const float* dxd, const int* keep, const float* mask, float* de, float* dmtok, float* part, int B, int L, int len_keep,
                             int Dd, hipStream_t st);
int mae_gelu_fwd_launch(const float* pre, float* y, long long n, hipStream_t st);
int mae_gelu_bwd_launch(const float* dy, const float* pre, float* dpre, long long n, hipStream_t st);     // dpre may be dy
// LayerNorm of width F % 4 == 0; backward dx = LN'(dy) (+ resid), dg / db [F] through part: mae_ln_chunks(R) * 2 F floats
int mae_ln_fwd_launch(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, long long R, int F, float eps, hipStream_t st);
int mae_ln_chunks(long long R);
int mae_ln_bwd_launch(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, const float* resid, float* dx, float* dg,
                      float* db, float* part, long long R, int F, hipStream_t st);
// pred [B, L, 3 p p] against obs; part [B L] scratch and loss [1] (both null: no loss), dpred [B, L + 1, 3 p p] with a zero CLS row (null: none)
int mae_loss_launch(const float* pred, const float* obs, const float* mask, const float* dloss, float* part, float* loss, float* dpred, int B, int L,
                    int len_keep, int S, int p, hipStream_t st);

// ------------------------------------------------------------------ conv.hip
struct ConvArgs {
    const float* X = nullptr;       // [B,H,W,CIN] NHWC
    const float* Wp = nullptr;      // packed weights [KS*KS][CIN/8][COUT][8]
    float* Y = nullptr;             // [B,H,W,COUT]
    int B = 0, H = 0, W = 0;
    const float* bias = nullptr;    // [COUT]
    int relu = 0;                   // 0 none, 1 ReLU, 2 ELU
    const float* posmap = nullptr;  // [H,W,COUT] added after bias/relu
    const float* mask = nullptr;    // [B,H,W,COUT]: output zeroed where mask <= 0 (ReLU backward)
    int mask_elu = 0;               // mask holds ELU outputs: v *= (m > 0 ? 1 : m + 1)
};
// conv_x3.hip (exploratory): the 5x5 / 64-channel layer on the bf16 matrix pipe with every fp32 operand split exactly into three bf16
size_t conv_x3_pack_floats(int KS = 5);
int conv_pack_x3_launch(const float* W, float* fwd3, float* bwd3, hipStream_t st, int KS = 5);          // W [64][64][KS][KS]; bwd3 may be null
int conv_x3_launch(const ConvArgs& a, const float* pack3, hipStream_t st, int KS = 5);                   // KS = 5 or 3
struct WgradArgs;
int conv_wgrad_x3_stage(const WgradArgs& a, int nchunk, hipStream_t st, int KS = 5);       // first stage of conv_wgrad_launch (same partial slabs)
struct WgradArgs {
    const float* X = nullptr;       // [B,H,W,CIN]
    const float* dY = nullptr;      // [B,H,W,COUT]
    float* part = nullptr;          // workspace, conv_wgrad_ws_floats()
    int B = 0, H = 0, W = 0;
    float* bpart = nullptr;         // bias partials [slab][64] behind the dW slabs (set by conv_wgrad_launch when db is asked for)
};
// low_latency: the caller's grid is small (inference at a few images): 5x5 / 64-channel forward layers whose throughput grid would leave
// most CUs idle go to the k-split kernel (conv_lat_kernel); results differ from the throughput kernel by fp32 summation order
int conv_fwd_launch(const ConvArgs& a, int KS, int CIN, int COUT, hipStream_t st, int low_latency = 0);
// x3: 1 = the split-precision first stage for the 5x5 / 64-channel layer (exploratory), 0 = fp32 MFMA, -1 = by OCRL_CONV_X3
// db (may be null): the bias gradient, summed inside the fp32 kernel from the dY fragments it stages anyway (not with x3 > 0)
int conv_wgrad_launch(const WgradArgs& a, int KS, int CIN, int COUT, int cin_real, float* dW, float* db, int accumulate, hipStream_t st, int x3 = -1);
int conv_wgrad_slabs(int B, int H, int W, int KS, int CIN);       // partial slabs the launch writes (workers, x2 for CIN == 8)
size_t conv_wgrad_ws_floats(int B, int H, int W, int KS, int CIN, bool with_db = true);
int conv_pack_launch(const float* W, float* fwd, float* bwd, int KS, int CIN, int COUT, int cin_real, hipStream_t st);

// ------------------------------------------------------------------ conv_first.hip
// the 5x5 / 3 -> 64 layer on the NCHW observation [B,3,H,W]: Y [B,H,W,64] = relu?(conv + bias) with the weights packed as [76][64]
size_t conv_first_pack_floats();
int conv_first_pack_launch(const float* W, float* pack, hipStream_t st);                       // W [64][3][5][5]
int conv_first_fwd_launch(const float* obs, const float* pack, const float* bias, float* Y, int B, int H, int W, int relu, hipStream_t st);
// its weight gradient dW [64][3][5][5] and bias gradient db [64] (may be null) from dY [B,H,W,64]; ws: conv_first_wgrad_ws_floats()
int conv_first_wgrad_workers(int B, int H, int W);
size_t conv_first_wgrad_ws_floats(int B, int H, int W);
int conv_first_wgrad_launch(const float* obs, const float* dY, float* ws, float* dW, float* db, int B, int H, int W, int accumulate, hipStream_t st);

// ------------------------------------------------------------------ elementwise.hip
int nchw_to_nhwc8_launch(const float* in, float* out, int B, int C, int H, int W, hipStream_t st);
int patchify4_launch(const float* in, float* out, int B, int C, int S, hipStream_t st);
int pixel_shuffle_launch(const float* in, float* out, int B, int h, int w, int Cout, int forward, const float* mask, hipStream_t st);
int layernorm_fwd_launch(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, long long R, int F, hipStream_t st);
int layernorm_bwd_launch(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, float* dx,
                         float* dgb, long long R, int F, int accumulate_dx, int accumulate_dgb, float* ws, size_t ws_floats, hipStream_t st);
int colsum_launch(const float* X, long long ld, float* out, long long R, int F, int accumulate, float scale, float* ws, size_t ws_floats, hipStream_t st);

// ------------------------------------------------------------------ sa_input.hip
// x = W2 relu(W0 LN(e4) + b0) + b2 over [R,64] rows, one kernel per direction (64-row tiles, persistent workgroups, max_wgs 0 = default).
// Forward: mean, rstd, h1, x bitwise as layernorm_fwd_launch + two lin_fwd give them; ln0 (may be null) receives LN(e4).  Backward: de4
// bitwise as the unfused chain's; the six parameter gradients are written (not accumulated) from one partial slab per workgroup in ws.
#define SA_INPUT_SLAB (2 * 4096 + 4 * 64)
void sa_input_plan(long long R, int max_wgs, int out[3]);        // {tile rows, workgroups of the backward (one slab each), slab floats}
int sa_input_fwd_launch(const float* e4, const float* gamma, const float* beta, const float* W0, const float* b0, const float* W2, const float* b2,
                        float* mean, float* rstd, float* ln0, float* h1, float* x, long long R, int max_wgs, hipStream_t st);
int sa_input_bwd_launch(const float* dx, const float* h1, const float* e4, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        const float* W0, const float* W2, float* de4, float* dW0, float* db0, float* dW2, float* db2, float* dgamma, float* dbeta,
                        long long R, int max_wgs, float* ws, size_t ws_floats, hipStream_t st);
int reduce_partials_launch(const float* part, int n, float* out, float scale, int accumulate, hipStream_t st);
int mse_launch(const float* obs, const float* recon, float* drecon, float* out, int B, int C, int H, int W, float* ws, size_t ws_floats, hipStream_t st);
int gumbel_softmax_launch(const float* raw, const float* e1, const float* e2, float* z, int* tokens, long long R, int V, float tau,
                          unsigned long long seed, hipStream_t st, float* zst = nullptr);
int softmax_bwd_rows_launch(const float* z, float* d, long long R, int V, float scale, hipStream_t st);
int softmax_stat_combine_launch(const float* stat, int nseg, long long R, float* lse, const float* hstat, const int* hidx, int* tokens,
                                const float* pred, int ldp, const int* tok, float* out, float scale, float* ws, size_t ws_floats, hipStream_t st,
                                const float* cdf_scores = nullptr, int cdf_V = 0, float cdf_tau = 1.f, unsigned long long cdf_seed = 0);
int exp_rows_launch(const float* y, const float* lse, float* z, long long R, int V, hipStream_t st);
int rowdot_bias64_launch(const float* g, const float* act, const float* bias, long long R, float* out, hipStream_t st);
int embed_fwd_launch(const int* tokens, const float* dict, const float* bos, const float* pe, float* out, int B, int T, int d, float p,
                     unsigned long long seed, hipStream_t st);
size_t embed_bwd_ws_floats(long long BT, int V, int d);
int embed_bwd_launch(float* g, const int* tokens, float* ddict, int B, int T, int V, int d, float p, unsigned long long seed, float* ws,
                     size_t ws_floats, hipStream_t st);
int dropout_apply_launch(const float* x, float* y, long long n, float p, unsigned long long seed, unsigned site, hipStream_t st);
int dropout_mask_launch(float* y, long long n, float p, unsigned long long seed, unsigned site, hipStream_t st);
int obs_u8_to_f32_launch(const unsigned char* in, float* out, int B, int H, int W, int C, hipStream_t st);
int fill_launch(float* x, long long n, float v, hipStream_t st);
int axpy_launch(const float* x, float* y, long long n, float a, hipStream_t st);
int posmap_launch(const float* Wpos, const float* bpos, float* out, int S, int C, hipStream_t st);
int posgrid_launch(float* out, int S, hipStream_t st);
int im2col5_launch(const float* x8, float* col, long long npix, int H, int W, int C, int ldc, hipStream_t st);
int unpack5_launch(const float* dWp, float* dW, int C, int ldc, hipStream_t st);
int pad_cols_launch(const float* in, int ldi, float* out, int ldo, long long R, int C, int Cout, hipStream_t st);

// ------------------------------------------------------------------ xattn.hip: cross attention to the slots, folded (transformer.py:23-50,181-185)
// The folded form's shape rule (host only; the launchers below call it, so what it reports is what runs): KP slots per head after
// padding (8 or 16), NC = h * KP columns, NM = d / 16, lds = dynamic LDS bytes of xattn_launch's kernels.  Returns `supported`;
// an unsupported shape leaves every field zero.
struct XaPlan { bool supported = false; int KP = 0, NC = 0, NM = 0; size_t lds = 0; };
bool xattn_plan(int K, int d, int h, XaPlan* out);
bool xattn_supported(int K, int d, int h);
int xattn_kp(int K, int h);                       // slots per head after padding (8 or 16); columns NC = h * KP
struct XaFoldHost {                               // per-image operands of all decoder blocks from the projected slots, one launch
    const float* mem = nullptr;                   // [B,K,d]
    const float* Wq[8]; const float* Wk[8]; const float* Wv[8]; const float* Wo[8];     // [d,d] (out, in) per block
    float* ck[8]; float* cv[8];                   // [B,K,d]
    float* Ab[8]; float* AbT[8]; float* Vo[8]; float* VoT[8];     // [B,NC,d] / [B,d,NC]; padding columns must be zero (never written)
    int B = 0, K = 0, d = 0, h = 0, nblk = 0;
};
int xattn_fold_fwd_launch(const XaFoldHost& f, hipStream_t st);
struct XaHost {
    const float* x = nullptr;                     // [B,T,d] attention input (LN of the residual stream)
    const float* resid = nullptr;                 // forward: residual stream
    float* y = nullptr;                           // forward: resid + dropout(out);  backward: d x
    float* P = nullptr;                           // [B,h,T,K] probabilities before dropout
    const float *Ab = nullptr, *AbT = nullptr, *Vo = nullptr, *VoT = nullptr;
    const float* gd = nullptr;                    // backward: gradient wrt out
    float *Pd = nullptr, *dS = nullptr;           // backward: [B*T, NC]
    int B = 0, T = 0, K = 0, d = 0, h = 0;
    float p = 0.f; unsigned long long seed = 0; unsigned site_p = 0, site_o = 0;
};
int xattn_launch(const XaHost& h, int backward, hipStream_t st);
struct XaFoldBwdHost {                            // backward of the fold, after xattn_launch(.., 1) of the same block
    const float *Pd = nullptr, *dS = nullptr;     // [B*T,NC] what xattn_launch(.., 1) wrote
    const float *gd = nullptr, *x = nullptr;      // [B,T,d] gradient wrt out; the attention input
    const float *Wq = nullptr, *Wo = nullptr;     // [d,d] (out, in)
    const float *ck = nullptr, *cv = nullptr;     // [B,K,d] from the fold
    float *dVo = nullptr, *dAb = nullptr;         // [B,NC,d] per-image sums over the tokens (written)
    float *dck = nullptr, *dcv = nullptr;         // [B,K,d] (written)
    float *pq = nullptr, *po = nullptr;           // [B,d,d] per-image partials of d Wq / d Wo (written)
    float *dWq = nullptr, *dWo = nullptr;         // [d,d] (written: the partials summed over the images in a fixed order)
    float* ws = nullptr; size_t ws_floats = 0;    // column-sum scratch (colsum_launch: d*d floats serve B <= 64)
    int B = 0, T = 0, K = 0, d = 0, h = 0;
};
int xattn_fold_bwd_launch(const XaFoldBwdHost& f, hipStream_t st);
// the plain form: Q [B,T,d], Km / Vm [B,K,d], P [B,h,T,K] the probabilities before dropout
int cross_attn_fwd_launch(const float* Q, const float* Km, const float* Vm, float* O, float* P, int B, int T, int K, int d, int h, float p,
                          unsigned long long seed, unsigned site, hipStream_t st);
size_t cross_attn_bwd_ws_floats(int B, int T, int K, int d, int h);
int cross_attn_bwd_launch(const float* dO, const float* Q, const float* Km, const float* Vm, const float* P, float* dQ, float* dKm, float* dVm,
                          int B, int T, int K, int d, int h, float p, unsigned long long seed, unsigned site, float* part, size_t part_floats,
                          hipStream_t st);


// ------------------------------------------------------------------ slot_attn.hip
// Packed weight block (built once per step by pack_launch): originals and transposed copies.
struct SaWts {
    int ln_in_g, ln_in_b, ln_s_g, ln_s_b, ln_m_g, ln_m_b;
    int Wq, WqT, Wk, WkT, Wv, WvT, Wih, WihT, Whh, WhhT, bih, bhh, W0, W0T, b0, W2, W2T, b2;
    int total;
};
static inline SaWts sa_wts_layout(int C, int D, int H) {
    SaWts o; int a = 0;
    auto take = [&](int n) { int r = a; a += (n + 3) & ~3; return r; };
    o.ln_in_g = take(C); o.ln_in_b = take(C); o.ln_s_g = take(D); o.ln_s_b = take(D); o.ln_m_g = take(D); o.ln_m_b = take(D);
    o.Wq = take(D * D); o.WqT = take(D * D); o.Wk = take(D * C); o.WkT = take(C * D); o.Wv = take(D * C); o.WvT = take(C * D);
    o.Wih = take(3 * D * D); o.WihT = take(3 * D * D); o.Whh = take(3 * D * D); o.WhhT = take(3 * D * D);
    o.bih = take(3 * D); o.bhh = take(3 * D);
    o.W0 = take(H * D); o.W0T = take(H * D); o.b0 = take(H); o.W2 = take(D * H); o.W2T = take(D * H); o.b2 = take(D);
    o.total = a;
    return o;
}
// Saved-activation matrix: one row per (image, iteration, slot), row = (b*I + t)*K + j, fields at fixed
// column offsets, so every field is a strided [B*I*K, dim] GEMM operand with ld = sa_save_ld().
// With NH attention heads (ocrs/common/slot_attn.py:54-61) the folded query, the weighted means and the weight sums exist per
// (slot, head): qp / up / upn are NH blocks of C columns (head h at + h*C), csum NH values.
struct SaSave { int sprev, sn, q, u, r, z, n, hn, sg, m, hid, qp, up, upn, csum, ld; };
static inline SaSave sa_save_layout(int C, int D, int H, int NH = 1) {
    SaSave o;
    o.sprev = 0; o.sn = D; o.q = 2 * D; o.u = 3 * D; o.r = 4 * D; o.z = 5 * D; o.n = 6 * D; o.hn = 7 * D; o.sg = 8 * D; o.m = 9 * D;
    o.hid = 10 * D; o.qp = 10 * D + H; o.up = o.qp + NH * C; o.upn = o.up + NH * C; o.csum = o.upn + NH * C; o.ld = o.csum + ((NH + 3) & ~3);
    return o;
}
// Gradient rows emitted by the backward kernel (same row index), consumed by the weight-gradient GEMMs.
struct SaGrad { int out, hid, gi, gh, u, q, qp, ld; };
static inline SaGrad sa_grad_layout(int C, int D, int H, int NH = 1) {
    SaGrad o;
    o.out = 0; o.hid = D; o.gi = D + H; o.gh = 4 * D + H; o.u = 7 * D + H; o.q = 8 * D + H; o.qp = 9 * D + H; o.ld = 9 * D + H + NH * C;      // qp: NH blocks of C
    return o;
}
struct SlotAttnArgs {
    int B = 0, N = 0, C = 64, K = 0, D = 0, H = 0, I = 0;
    int NH = 1;                      // attention heads (ocrs/common/slot_attn.py:28): the soft-max runs over NH*K columns; NH*K <= 16, K <= 8 when NH > 1
    float eps = 1e-8f, scale = 1.f;  // scale = (D / NH)^-1/2
    const float* x = nullptr;        // [B,N,C]
    const float* slots0 = nullptr;   // [B,K,D]
    const float* wts = nullptr;      // packed weights, sa_wts_layout
    float* slots = nullptr;          // [B,K,D]
    float* attn = nullptr;           // [B,N,K] (last iteration, pre-eps; summed over the heads), may be null
    float* attn_heads = nullptr;     // NH > 1 and attn wanted: [B,N,NH*K] scratch for the per-head maps
    float* save = nullptr;           // [B*I*K, sa_save_layout().ld], may be null for inference
    const float* dslots = nullptr;   // [B,K,D]
    float* dx = nullptr;             // [B,N,C]
    float* dslots0 = nullptr;        // [B,K,D]
    float* grows = nullptr;          // [B*I*K, sa_grad_layout().ld]
    float* g_small = nullptr;        // [B][4D + 2C]: dgamma/dbeta of norm_slots, norm_mlp, norm_inputs
    // pipelined form (streaming launches with several workgroups per image alternate with slot-side launches): per-image exchange
    // buffer of B * sa_xchg_floats_host() floats and the partial-sum buffer of sa_parts_floats_host() floats; either null = the fused
    // one-workgroup-per-image kernels
    float* xchg = nullptr;
    float* parts = nullptr;
    // forward only: 0 = whole chain; 1 = the preparation launch alone (slots0 -> slots / folded query of iteration 0 in xchg; needs the
    // weights and slots0 but not x, so a caller can issue it long before the features exist); 2 = the chain without that launch
    int phase = 0;
};
size_t sa_xchg_floats_host(int K, int D);      // per image; K = num_slots * heads
size_t sa_parts_floats_host(int B, int K);     // K = num_slots * heads
// what slot_attn_launch runs for (num_slots, slot size, MLP size, heads): G images per slot-side workgroup, NB row blocks of KB rows, the
// dynamic LDS bytes of the forward / backward slot-side kernels, KS = heads * num_slots streaming columns.  Needs no device; non-zero
// (with the error text) for arguments slot_attn_launch refuses.
struct SaPlan { int G, NB, KB, KS; size_t smem_fwd, smem_bwd; };
int sa_plan(int K, int D, int H, int NH, SaPlan* plan);
int slot_attn_launch(const SlotAttnArgs& a, int backward, hipStream_t st);

// generic gather/transposing pack: entry e copies src[rows][cols] to dst + dst_off (transposed if requested)
struct PackEntry { const float* src; int rows, cols, dst_off, transpose; };
int pack_launch(const PackEntry* entries_dev, int n_entries, int max_elems, float* dst, hipStream_t st);

// ------------------------------------------------------------------ optim.hip
int absmax_launch(const float* g, long long n, float* out, float* ws, size_t ws_floats, hipStream_t st);
// g is first scaled by gscale (1/world for data parallel mean), then clipped by the inf-norm in norm[0]*gscale
int clip_adam_launch(float* p, const float* g, float* m, float* v, long long n, const float* norm, float clip, float lr, double b1,
                     double b2, double eps, int step, float gscale, hipStream_t st);
// the same update on 1 .. 3 trailing elements (any alignment)
int clip_adam_tail_launch(float* p, const float* g, float* m, float* v, int n, const float* norm, float clip, float lr, double b1, double b2,
                          double eps, int step, float gscale, hipStream_t st);
// L2-clipped TF-style RMSprop (eps inside the root, sq starts at ones): norm[0] holds ||g||_2; n a multiple of 4, and the 1 .. 3 element tail
int clip_rmsprop_launch(float* p, const float* g, float* sq, long long n, const float* norm, float clip, float lr, double alpha, double eps,
                        hipStream_t st);
int clip_rmsprop_tail_launch(float* p, const float* g, float* sq, int n, const float* norm, float clip, float lr, double alpha, double eps,
                             hipStream_t st);
// The L2 clip + update over up to FLAT_MAX_SEG flat buffers in three launches (partial sums of squares, their fold, the update): the norm
// is that of all the gradients together.  The table travels by value as a kernel argument; the launchers fill blk0 (the prefix of each
// segment's block count, at most FLAT_SEG_BLOCKS each).  s0, s1: m, v (Adam); sq, unused (RMSprop).  Any n >= 1; ws: blk0[nseg] floats,
// at most FLAT_MAX_SEG * FLAT_SEG_BLOCKS.
constexpr int FLAT_MAX_SEG = 8, FLAT_SEG_BLOCKS = 1024;
struct FlatSegs {
    float* p[FLAT_MAX_SEG];
    const float* g[FLAT_MAX_SEG];
    float* s0[FLAT_MAX_SEG];
    float* s1[FLAT_MAX_SEG];
    long long n[FLAT_MAX_SEG];
    int blk0[FLAT_MAX_SEG + 1];
    int nseg;
};
int multi_clip_adam_launch(FlatSegs t, float* norm, float clip, float lr, double b1, double b2, double eps, int step, float* ws, size_t ws_floats,
                           hipStream_t st);
int multi_clip_rmsprop_launch(FlatSegs t, float* norm, float clip, float lr, double alpha, double eps, float* ws, size_t ws_floats, hipStream_t st);
int store_u64_launch(unsigned long long* dst, unsigned long long v, hipStream_t st);
int slot_init_launch(const float* mu, const float* logsig, const float* noise, float* slots0, int BK, int D, unsigned long long seed, hipStream_t st,
                     const unsigned long long* seed_dev = nullptr);
int slot_init_bwd_launch(const float* dslots0, const float* logsig, const float* noise, float* dmu, float* dlogsig, int BK, int D, unsigned long long seed, hipStream_t st);
int copy_launch(const float* src, float* dst, long long n, hipStream_t st);
int argmax_pos_launch(const float* pred, int* tokens, int B, int T, int V, int t, hipStream_t st, int dense_rows = 0);
int embed_step_launch(const int* tokens, const float* dict, const float* bos, const float* pe, float* out, int B, int T, int d, int t, hipStream_t st);
int decode_attn_launch(const float* qkv, float* out, int B, int T, int t, int d, int h, int ld, hipStream_t st);
int onehot_launch(const int* tokens, float* z, long long rows, int V, hipStream_t st);

// ------------------------------------------------------------------ attention.hip
struct AttnArgs {
    const float *q = nullptr, *k = nullptr, *v = nullptr;   // projected (q unscaled), heads side by side, row stride ld (>= d)
    float* o = nullptr;                                     // [B,T,d]
    float* lse = nullptr;                                   // [B,h,T] log-sum-exp of the scaled scores
    int B = 0, T = 0, d = 0, h = 0;
    int ld = 0;                                             // row stride of q,k,v and dq,dk,dv (o, dO are dense [B,T,d])
    float p = 0.f;                                          // dropout on the probabilities
    unsigned long long seed = 0;
    unsigned site = 0;
    const float* dO = nullptr;                              // backward
    float *dq = nullptr, *dk = nullptr, *dv = nullptr, *delta = nullptr;
    // backward, hand-off form: the dK/dV kernel leaves its dS tiles here and the dQ kernel reads them (uninitialised scratch, 16-byte
    // aligned; attn_bwd_ds_floats(B, T, h) holds the whole batch, less makes the launcher walk the batch in image chunks, null or less
    // than one image selects the two-kernel form)
    float* ds = nullptr;
    size_t ds_floats = 0;
    int b0 = 0;                                             // first image of a chunk (set by the launcher: pointers stay those of image 0)
};
int attn_launch(const AttnArgs& a, int mode, hipStream_t st);
size_t attn_bwd_ds_floats(int B, int T, int h);             // 64 x 64 tiles of the causal triangle, per (image, head)
// OCRL_ATTN_BWD as the launcher reads it, at every call: 1 one pass, 2 two kernels, otherwise the hand-off form where a.ds has room
int attn_bwd_form();
// dS floats a model may carve for (B, T, h) under the switches as they are now: min(whole batch, OCRL_ATTN_DS_MB), 0 when the form is 1 or 2
size_t attn_bwd_ds_carve_floats(int B, int T, int h);

// ------------------------------------------------------------------ bcast_l1.hip (first layer of both broadcast decoders: ks = 5 SLATE, 3 IODINE)
enum { BCAST_L1_RELU = 0, BCAST_L1_ELU = 1 };
int bcast_l1_class_sum_launch(const float* in, float* out, long long BK, int ks, int forward, hipStream_t st);
int bcast_l1_fwd_launch(const float* P1, const float* T, const float* bias, float* c1, long long BK, int S, int ks, int act, hipStream_t st);
size_t bcast_l1_bwd_ws_floats(long long BK, int S, int ks);
int bcast_l1_bwd_launch(const float* g, float* dT, long long BK, int S, int ks, float* ws, size_t ws_floats, hipStream_t st);
int bc_posconv_launch(const float* Wc, float* P1, int S, hipStream_t st);
int bc_posconv_bwd_launch(const float* G, float* dWc, int S, hipStream_t st);
int io_p1_launch(const float* Wxy, const float* b1, float* P1, int S, hipStream_t st);
int io_w1_grad_launch(const float* dW1r, const float* G, float* dW1, float* db1, int S, int L, hipStream_t st);

// ------------------------------------------------------------------ bcdec.hip (Slot-Attention broadcast decoder)
int bc_compose_launch(const float* W1, const float* Wpos, const float* bpos, float* Wc, float* W1r, int D, hipStream_t st);
int bc_compose_bwd_launch(const float* W1, const float* Wpos, const float* bpos, const float* dWc, const float* dW1r, float* dW1,
                          float* dWpos, float* dbpos, int D, hipStream_t st);
int bc_c4_pack_launch(const float* W, float* Wk, float* Wb, int co_n, hipStream_t st);
int bc_c4_fwd_launch(const float* X, const float* Wk, const float* bias4, float* Y, int Bn, int S, hipStream_t st);
int bc_c4_bwd_data_launch(const float* dY, const float* Wb, const float* act, float* dX, int Bn, int S, hipStream_t st, int elu = 0);
int bc_c4_wgrad_blocks(int Bn, int S);
int bc_c4_wgrad_launch(const float* X, const float* dY, float* part, int Bn, int S, hipStream_t st, int form = 0);
int bc_mix_launch(const float* out4, const float* obs, float* recon, float* dout4, float* loss_out, int B, int K, int S, int C, float* ws,
                  size_t ws_floats, hipStream_t st);

// ------------------------------------------------------------------ iodine.hip (IODINE: ocrs/iodine/iodine_module.py)
int io_sample_launch(const float* mu, const float* ls, const float* noise, float* eps_out, float* slots, float* kl_out, long long n,
                     unsigned long long seed, unsigned site, float* ws, size_t ws_floats, hipStream_t st);
int io_w1_pack_launch(const float* W1, float* W1r, float* Wxy, int L, hipStream_t st);
int io_elbo_launch(const float* out4, const float* obs, int B, int K, int S, float sigma, float* enc, float* st1, float* dout4, float* part,
                   float* masks_out, float* recon_out, float* rmasked_out, float* ws, size_t ws_floats, hipStream_t st);
int io_enc_norm_launch(float* enc, const float* st1, float* st2, long long BK, int N, float* ws, size_t ws_floats, hipStream_t st);
int io_elbo_bwd_launch(const float* out4, const float* obs, const float* denc, int B, int K, int S, float sigma, float cw, float* dout4, hipStream_t st);
int io_latent_launch(const float* mu, const float* ls, const float* eps, const float* ds, float* latent, long long BK, int L, float beta, int layer_norm,
                     int ld, hipStream_t st);
int io_im2col_launch(const float* x, float* col, long long Bn, int C, int Hi, int Wi, int ldc, hipStream_t st, int force_generic = 0);
int io_col2im_launch(const float* dcol, const float* act, float* dx, long long Bn, int C, int Hi, int Wi, int ldc, hipStream_t st,
                     int force_generic = 0);
int io_refw_pack_launch(const float* W, float* Wp, int C, int ldc, hipStream_t st);
int io_refw_unpack_launch(const float* dWp, float* dW, int C, int ldc, hipStream_t st);
int io_pool_launch(const float* r, float* pool, long long BK, int n, hipStream_t st);
int io_pool_bwd_launch(const float* dpool, const float* r, float* dpre, long long BK, int n, hipStream_t st);
int io_elu2_launch(const float* a, int lda, float* y, int ldy, long long rows, int F, const float* dy, int lddy, hipStream_t st);
int io_lstm_fwd_launch(const float* gates, const float* c0, float* acts, float* c1, float* h1, long long rows, int H, hipStream_t st);
int io_lstm_bwd_launch(const float* acts, const float* c0, const float* c1, const float* dh1, const float* dc1, float* dgates, float* dc0,
                       long long rows, int H, hipStream_t st);
int io_post_grad_launch(const float* mu, const float* ls, const float* eps, const float* ds, const float* dlat, int ldl, float kw, float* gmu,
                        float* gls, long long BK, int L, hipStream_t st);
int io_l2norm_launch(const float* g, long long n, float* out, float* ws, size_t ws_floats, hipStream_t st);
int io_loss_launch(const float* parts, float* metrics, int I, int B, float beta, hipStream_t st);
