// C ABI of the NatureCNN / MultipleCNN encoders (include/ocrl_hip.h: ocrl_naturecnn_*): ocrs/naturecnn/naturecnn_module.py:11-63 and
// ocrs/multiple_cnns/multiple_cnn_module.py:12-38.  G modules (G = 1 for NatureCNN) run side by side as groups of one set of launches:
// the first convolution of all G modules is one launch over the shared image, the deeper ones are grouped convolutions, and the G
// Linears are G GEMMs on the library's GEMM (bias and ReLU in the forward epilogue, the ReLU mask in the dX epilogue, the bias gradient
// through bias_out).
//   forward   L conv launches + G GEMMs (+ 1 copy of the output into ws when saving)          L = 3, or 4 with cnn_feat_size 2
//   backward  1 mask + 2 G GEMMs + L conv launches (dW partials and the masked dX in one) + 1 reduce of every dW / db
// With use_cnn_feat there are no Linears: the last map is written straight to `out` as HWC tokens.  Stateless: the caller owns the
// parameters, their gradients and the workspace; a saving forward leaves every activation the backward needs in `ws`.
#include "../../include/ocrl_hip.h"
#include "kernels.h"

namespace {
struct NcLay {
    int L = 0, G = 1, np = 0, nflat = 0;
    int cin[OCRL_NATURECNN_MAX_CONVS], cout[OCRL_NATURECNN_MAX_CONVS], ks[OCRL_NATURECNN_MAX_CONVS], st[OCRL_NATURECNN_MAX_CONVS];
    int H[OCRL_NATURECNN_MAX_CONVS], W[OCRL_NATURECNN_MAX_CONVS], OH[OCRL_NATURECNN_MAX_CONVS], OW[OCRL_NATURECNN_MAX_CONVS];
    int slabs[OCRL_NATURECNN_MAX_CONVS], slab_rows[OCRL_NATURECNN_MAX_CONVS];
    NcMap xin[OCRL_NATURECNN_MAX_CONVS], yout[OCRL_NATURECNN_MAX_CONVS];
    size_t act[OCRL_NATURECNN_MAX_CONVS], dact[OCRL_NATURECNN_MAX_CONVS], part[OCRL_NATURECNN_MAX_CONVS], lin = 0, dz = 0, total = 0;
};

int check_nc(int B, int H, int W, int cin, int G, int feat, int use_feat, int rep) {
    const int L = feat == 2 ? 4 : 3, minsz = L == 4 ? 52 : 36;
    OCRL_REQUIRE(B >= 1 && cin >= 1, "naturecnn: batch >= 1 and obs_channels >= 1 (got %d, %d)", B, cin);
    OCRL_REQUIRE(H >= minsz && W >= minsz, "naturecnn: the input must be at least %d x %d (got %d x %d): smaller ones leave an empty map", minsz, minsz,
                 H, W);
    OCRL_REQUIRE(G >= 1 && G <= OCRL_NATURECNN_MAX_GROUPS, "naturecnn: 1 <= modules <= %d (got %d)", OCRL_NATURECNN_MAX_GROUPS, G);
    if (use_feat) OCRL_REQUIRE(G == 1 && (feat == 2 || feat == 4), "naturecnn: use_cnn_feat needs one module and cnn_feat_size 2 or 4 (got %d, %d)", G, feat);
    else OCRL_REQUIRE(rep >= 4 && rep % 4 == 0, "naturecnn: rep_dim must be a positive multiple of 4 (got %d)", rep);
    const long long OH1 = (H - 8) / 4 + 1, OW1 = (W - 8) / 4 + 1;
    OCRL_REQUIRE((long long)B * G * 32 * OH1 * OW1 < (1LL << 31) && (long long)B * cin * H * W < (1LL << 31),
                 "naturecnn: batch %d of %d x %d images exceeds the int32 range of one call", B, H, W);
    return 0;
}

NcLay nc_layout(int B, int H, int W, int cin, int G, int feat, int use_feat, int rep) {
    NcLay y;
    WsTake take;
    static const int KS[4] = {8, 4, 3, 3}, ST[4] = {4, 2, 1, 1}, CO[4] = {32, 64, 64, 128};
    y.L = feat == 2 ? 4 : 3;
    y.G = G;
    y.np = 2 * y.L + (use_feat ? 0 : 2);
    int h = H, w = W, c = cin;
    for (int l = 0; l < y.L; ++l) {
        y.cin[l] = c; y.cout[l] = CO[l]; y.ks[l] = KS[l]; y.st[l] = ST[l]; y.H[l] = h; y.W[l] = w;
        y.OH[l] = (h - KS[l]) / ST[l] + 1; y.OW[l] = (w - KS[l]) / ST[l] + 1;
        h = y.OH[l]; w = y.OW[l]; c = CO[l];
    }
    for (int l = 0; l < y.L; ++l) {
        const long long C = y.cout[l], hw = (long long)y.OH[l] * y.OW[l];
        NcMap& o = y.yout[l];
        if (l < y.L - 1) { o.sN = G * C * hw; o.sG = C * hw; o.sC = hw; o.sH = y.OW[l]; o.sW = 1; }          // [B, G C, OH, OW]
        else if (!use_feat) { o.sG = B * C * hw; o.sN = C * hw; o.sC = hw; o.sH = y.OW[l]; o.sW = 1; }      // [G, B, C, OH, OW]
        else { o.sN = hw * C; o.sG = 0; o.sC = 1; o.sH = y.OW[l] * C; o.sW = C; }                              // [B, OH OW, C] tokens
        if (l == 0) { NcMap& x = y.xin[0]; x.sN = (long long)cin * H * W; x.sG = 0; x.sC = (long long)H * W; x.sH = W; x.sW = 1; }   // obs NCHW
        else y.xin[l] = y.yout[l - 1];
        const size_t n = (size_t)B * G * C * hw;
        y.act[l] = take(n); y.dact[l] = take(n);
        // the weight gradient reduces over the B OH OW rows: up to 64 slabs of >= 64 rows, summed in slab order by nc_dw_reduce
        const long long M = (long long)B * hw;
        long long s = (M + 63) / 64;
        if (s > 64) s = 64;
        long long rows = ((M + s - 1) / s + 3) & ~3LL;
        y.slab_rows[l] = (int)rows;
        y.slabs[l] = (int)((M + rows - 1) / rows);
        y.part[l] = take((size_t)y.slabs[l] * G * C * ((size_t)y.cin[l] * KS[l] * KS[l] + 1));
    }
    y.nflat = y.cout[y.L - 1] * y.OH[y.L - 1] * y.OW[y.L - 1];
    if (!use_feat) { y.lin = take((size_t)B * G * rep); y.dz = take((size_t)B * G * rep); }
    y.total = take.end;
    return y;
}
}  // namespace

extern "C" {

size_t ocrl_naturecnn_ws_floats(int B, int H, int W, int cin, int groups, int cnn_feat_size, int use_cnn_feat, int rep_dim) {
    if (check_nc(B, H, W, cin, groups, cnn_feat_size, use_cnn_feat, rep_dim)) return 0;   // the shapes fwd / bwd reject get no workspace
    return nc_layout(B, H, W, cin, groups, cnn_feat_size, use_cnn_feat, rep_dim).total;
}

int ocrl_naturecnn_fwd(const float* obs, const float* const* w, float* out, int B, int H, int W, int cin, int groups, int cnn_feat_size,
                       int use_cnn_feat, int rep_dim, int save, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(obs && w && out && ws, "ocrl_naturecnn_fwd: null argument");
    RC(check_nc(B, H, W, cin, groups, cnn_feat_size, use_cnn_feat, rep_dim));
    const NcLay y = nc_layout(B, H, W, cin, groups, cnn_feat_size, use_cnn_feat, rep_dim);
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_naturecnn_fwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int G = y.G, L = y.L;
    for (int l = 0; l < L; ++l) {
        NcFwdArgs a;
        a.X = l ? ws + y.act[l - 1] : obs; a.x = y.xin[l];
        const bool to_out = use_cnn_feat && l == L - 1;
        a.Y = to_out ? out : ws + y.act[l];
        a.Y2 = to_out && save ? ws + y.act[l] : nullptr;
        a.y = y.yout[l];
        for (int g = 0; g < G; ++g) { a.w[g] = w[g * y.np + 2 * l]; a.bias[g] = w[g * y.np + 2 * l + 1]; }
        a.B = B; a.G = G; a.cin = y.cin[l]; a.cout = y.cout[l]; a.H = y.H[l]; a.W = y.W[l]; a.OH = y.OH[l]; a.OW = y.OW[l];
        a.ks = y.ks[l]; a.stride = y.st[l];
        RC(nc_conv_fwd_launch(a, st));
    }
    if (use_cnn_feat) return 0;
    // module g's Linear: relu(flat_g W_g^T + b_g) -> column block g of [B, G, rep_dim]
    float* lo = save ? ws + y.lin : out;
    for (int g = 0; g < G; ++g)
        RC(lin_fwd(ws + y.act[L - 1] + (size_t)g * B * y.nflat, y.nflat, w[g * y.np + 2 * L], w[g * y.np + 2 * L + 1], lo + (size_t)g * rep_dim,
                   G * rep_dim, B, rep_dim, y.nflat, 1, nullptr, 0, st));
    if (save) RC(copy_launch(lo, out, (long long)B * G * rep_dim, st));
    return 0;
}

int ocrl_naturecnn_bwd(const float* obs, const float* dout, const float* const* w, float* const* dw, int B, int H, int W, int cin, int groups,
                       int cnn_feat_size, int use_cnn_feat, int rep_dim, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(obs && dout && w && dw && ws, "ocrl_naturecnn_bwd: null argument");
    RC(check_nc(B, H, W, cin, groups, cnn_feat_size, use_cnn_feat, rep_dim));
    const NcLay y = nc_layout(B, H, W, cin, groups, cnn_feat_size, use_cnn_feat, rep_dim);
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_naturecnn_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int G = y.G, L = y.L;
    const int last = L - 1;
    if (use_cnn_feat) {
        RC(nc_relu_mask_launch(dout, ws + y.act[last], ws + y.dact[last], (long long)B * y.nflat, st));   // tokens: same layout as out
    } else {
        RC(nc_relu_mask_launch(dout, ws + y.lin, ws + y.dz, (long long)B * G * rep_dim, st));
        for (int g = 0; g < G; ++g) {
            const size_t xo = (size_t)g * B * y.nflat;
            const float* dz = ws + y.dz + (size_t)g * rep_dim;
            const float* flat = ws + y.act[last] + xo;
            // dW_g = dz_g^T flat_g, db_g = column sums of dz_g (B rows: no split-k scratch); d flat_g = (dz_g W_g) * (flat_g > 0)
            RC(lin_bwd_w(dz, G * rep_dim, flat, y.nflat, dw[g * y.np + 2 * L], dw[g * y.np + 2 * L + 1], B, rep_dim, y.nflat, 1.f, nullptr, 0, st));
            RC(lin_bwd_x(dz, G * rep_dim, w[g * y.np + 2 * L], ws + y.dact[last] + xo, y.nflat, B, rep_dim, y.nflat, flat, y.nflat, nullptr, 0, st));
        }
    }
    NcReduceArgs r;
    r.nlayers = L;
    for (int l = last; l >= 0; --l) {
        NcBwdArgs a;
        a.X = l ? ws + y.act[l - 1] : obs; a.x = y.xin[l];
        a.dY = ws + y.dact[l]; a.dy = y.yout[l];
        a.dX = l ? ws + y.dact[l - 1] : nullptr;       // the observation gets no gradient
        a.part = ws + y.part[l]; a.slabs = y.slabs[l]; a.slab_rows = y.slab_rows[l];
        for (int g = 0; g < G; ++g) a.w[g] = w[g * y.np + 2 * l];
        a.B = B; a.G = G; a.cin = y.cin[l]; a.cout = y.cout[l]; a.H = y.H[l]; a.W = y.W[l]; a.OH = y.OH[l]; a.OW = y.OW[l];
        a.ks = y.ks[l]; a.stride = y.st[l];
        RC(nc_conv_bwd_launch(a, st));
        NcReduceLayer& q = r.L[l];
        q.part = ws + y.part[l]; q.slabs = y.slabs[l]; q.G = G; q.cout = y.cout[l]; q.K = y.cin[l] * y.ks[l] * y.ks[l];
        q.n = (long long)G * q.cout * (q.K + 1);
        for (int g = 0; g < G; ++g) { r.dw[l][g] = dw[g * y.np + 2 * l]; r.db[l][g] = dw[g * y.np + 2 * l + 1]; }
    }
    return nc_dw_reduce_launch(r, st);
}

}  // extern "C"
