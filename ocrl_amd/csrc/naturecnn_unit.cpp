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
#include "unit_base.h"

namespace {
struct NcLay {
    int L = 0, G = 1, np = 0, nflat = 0;
    ConvLayer c[OCRL_NATURECNN_MAX_CONVS];
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
    y.L = feat == 2 ? 4 : 3;
    y.G = G;
    y.np = 2 * y.L + (use_feat ? 0 : 2);
    nc_stack(y.c, y.L, B, cin, H, W);
    for (int l = 0; l < y.L; ++l) {
        ConvLayer& c = y.c[l];
        const long long C = c.cout, hw = (long long)c.OH * c.OW;
        NcMap& o = c.y;
        if (l < y.L - 1) { o.sN = G * C * hw; o.sG = C * hw; o.sC = hw; o.sH = c.OW; o.sW = 1; }          // [B, G C, OH, OW]
        else if (!use_feat) { o.sG = B * C * hw; o.sN = C * hw; o.sC = hw; o.sH = c.OW; o.sW = 1; }      // [G, B, C, OH, OW]
        else { o.sN = hw * C; o.sG = 0; o.sC = 1; o.sH = c.OW * C; o.sW = C; }                              // [B, OH OW, C] tokens
        if (l == 0) { c.x.sN = (long long)cin * H * W; c.x.sG = 0; c.x.sC = (long long)H * W; c.x.sH = W; c.x.sW = 1; }   // obs NCHW
        else c.x = y.c[l - 1].y;
        const size_t n = (size_t)B * G * C * hw;
        y.act[l] = take(n); y.dact[l] = take(n);
        y.part[l] = take((size_t)c.slab.slabs * G * C * ((size_t)c.K() + 1));
    }
    y.nflat = y.c[y.L - 1].cout * y.c[y.L - 1].OH * y.c[y.L - 1].OW;
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
    RC(ws_check("ocrl_naturecnn_fwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int G = y.G, L = y.L;
    for (int l = 0; l < L; ++l) {
        const bool to_out = use_cnn_feat && l == L - 1;
        RC(conv_fwd(y.c[l], l ? ws + y.act[l - 1] : obs, to_out ? out : ws + y.act[l], to_out && save ? ws + y.act[l] : nullptr, w + 2 * l, y.np,
                    B, G, st));
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
    RC(ws_check("ocrl_naturecnn_bwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int G = y.G, L = y.L;
    const int last = L - 1;
    if (use_cnn_feat) RC(nc_relu_mask_launch(dout, ws + y.act[last], ws + y.dact[last], (long long)B * y.nflat, st));   // tokens: same layout as out
    else RC(nc_tail_bwd(dout, ws + y.lin, ws + y.dz, ws + y.act[last], ws + y.dact[last], w + 2 * L, dw + 2 * L, y.np, B, G, rep_dim, y.nflat, st));
    NcReduceArgs r;
    for (int l = last; l >= 0; --l) {
        float* dX = l ? ws + y.dact[l - 1] : nullptr;   // the observation gets no gradient
        RC(conv_bwd(y.c[l], l ? ws + y.act[l - 1] : obs, ws + y.dact[l], dX, ws + y.part[l], w + 2 * l, y.np, B, G, st));
        conv_reduce_add(r, l, y.c[l], ws + y.part[l], dw + 2 * l, y.np, G);
    }
    return nc_dw_reduce_launch(r, st);
}

}  // extern "C"
