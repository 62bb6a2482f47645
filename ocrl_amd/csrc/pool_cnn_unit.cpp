// C ABI of the NatureCNN pooling heads (include/ocrl_hip.h: ocrl_pool_cnn_*): poolings/cnn_linear/cnn_linear_module.py:7-14 and the CNN
// front end of poolings/cnn_transformer/cnn_transformer_module.py:12-40, over slot_to_img(tokens) (utils/tools.py:33-36), which for a
// [B, H W, D] token map is a view: the map already is the channels-last image.  The first convolution, its weight gradient and its
// input gradient are pool_cnn.hip; layers 2 and 3, the ReLU masks and the Linear are the launches of the NatureCNN encoder
// (naturecnn.hip, gemm.hip) with one group, through the conv-layer calls of unit_base.h.
//   forward   1 pack + 3 conv launches [+ 1 GEMM (+ 1 copy of the output into ws when saving)]
//   backward  1 mask [+ 2 GEMMs] + 2 conv launches (layers 3, 2: dW partials and the masked dX in one) + the first layer's dW partials
//             + 2 reduces [+ 1 pack + the per-phase dX when the tokens want a gradient]
// Stateless: the caller owns the parameters, their gradients and the workspace.
#include "../../include/ocrl_hip.h"
#include "unit_base.h"

namespace {
struct PcLay {
    PcGeom g;
    ConvLayer c[3];                                // the NatureCNN stack; layer 0 runs on pool_cnn.hip (its slab is g's)
    size_t act[3], dact[3], part[3], wp = 0, wd = 0, lin = 0, dz = 0, total = 0;
    int nflat = 0;
};

int check_pc(int B, int H, int W, int D, int rep) {
    OCRL_REQUIRE(B >= 1 && D >= 1, "pool_cnn: batch >= 1 and token width >= 1 (got %d, %d)", B, D);
    OCRL_REQUIRE(H >= 36 && W >= 36, "pool_cnn: the token map must be at least 36 x 36 (got %d x %d): smaller ones leave an empty map", H, W);
    OCRL_REQUIRE(rep >= 0 && rep % 4 == 0, "pool_cnn: rep_dim must be a non-negative multiple of 4 (got %d)", rep);
    const long long OH1 = (H - 8) / 4 + 1, OW1 = (W - 8) / 4 + 1;
    OCRL_REQUIRE((long long)B * 32 * OH1 * OW1 < (1LL << 31) && (long long)B * D * H * W < (1LL << 31) && (long long)D * 64 * 32 < (1LL << 28),
                 "pool_cnn: batch %d of %d x %d x %d token maps exceeds the int32 range of one call", B, H, W, D);
    return 0;
}

PcLay pc_layout(int B, int H, int W, int D, int rep) {
    PcLay y;
    WsTake take;
    y.g = pc_geom(B, H, W, D);
    nc_stack(y.c, 3, B, D, H, W);
    y.wp = take(y.g.wp_floats);
    y.wd = take(y.g.wd_floats);
    for (int l = 0; l < 3; ++l) {
        ConvLayer& c = y.c[l];
        const long long C = c.cout, hw = (long long)c.OH * c.OW;
        NcMap& o = c.y;
        if (l < 2 || rep > 0) { o.sN = C * hw; o.sG = 0; o.sC = hw; o.sH = c.OW; o.sW = 1; }       // [B, C, OH, OW]; the last one flattens NCHW
        else { o.sN = hw * C; o.sG = 0; o.sC = 1; o.sH = c.OW * C; o.sW = C; }                       // [B, OH OW, C] tokens
        if (l) c.x = y.c[l - 1].y;
        const size_t n = (size_t)B * C * hw;
        y.act[l] = take(n); y.dact[l] = take(n);
        y.part[l] = take(l ? (size_t)c.slab.slabs * C * ((size_t)c.K() + 1) : y.g.part_floats);
    }
    y.nflat = y.c[2].cout * y.c[2].OH * y.c[2].OW;
    if (rep > 0) { y.lin = take((size_t)B * rep); y.dz = take((size_t)B * rep); }
    y.total = take.end;
    return y;
}
}  // namespace

extern "C" {

size_t ocrl_pool_cnn_ws_floats(int B, int H, int W, int D, int rep_dim) {
    if (check_pc(B, H, W, D, rep_dim)) return 0;                      // the shapes fwd / bwd reject get no workspace
    return pc_layout(B, H, W, D, rep_dim).total;
}

int ocrl_pool_cnn_fwd(const float* tokens, const float* const* w, float* out, int B, int H, int W, int D, int rep_dim, int save, float* ws,
                      size_t ws_floats, void* stream) {
    OCRL_REQUIRE(tokens && w && out && ws, "ocrl_pool_cnn_fwd: null argument");
    RC(check_pc(B, H, W, D, rep_dim));
    const PcLay y = pc_layout(B, H, W, D, rep_dim);
    RC(ws_check("ocrl_pool_cnn_fwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    RC(pc_conv1_fwd_launch(tokens, w[0], w[1], ws + y.wp, ws + y.act[0], B, H, W, D, st));
    for (int l = 1; l < 3; ++l) {
        const bool to_out = rep_dim == 0 && l == 2;
        RC(conv_fwd(y.c[l], ws + y.act[l - 1], to_out ? out : ws + y.act[l], to_out && save ? ws + y.act[l] : nullptr, w + 2 * l, 0, B, 1, st));
    }
    if (rep_dim == 0) return 0;
    float* lo = save ? ws + y.lin : out;
    RC(lin_fwd(ws + y.act[2], y.nflat, w[6], w[7], lo, rep_dim, B, rep_dim, y.nflat, 1, nullptr, 0, st));
    if (save) RC(copy_launch(lo, out, (long long)B * rep_dim, st));
    return 0;
}

int ocrl_pool_cnn_bwd(const float* tokens, const float* dout, const float* const* w, float* dtokens, float* const* dw, int B, int H, int W, int D,
                      int rep_dim, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(tokens && dout && w && dw && ws, "ocrl_pool_cnn_bwd: null argument");
    RC(check_pc(B, H, W, D, rep_dim));
    const PcLay y = pc_layout(B, H, W, D, rep_dim);
    RC(ws_check("ocrl_pool_cnn_bwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (rep_dim == 0) RC(nc_relu_mask_launch(dout, ws + y.act[2], ws + y.dact[2], (long long)B * y.nflat, st));      // tokens: same layout as out
    else RC(nc_tail_bwd(dout, ws + y.lin, ws + y.dz, ws + y.act[2], ws + y.dact[2], w + 6, dw + 6, 0, B, 1, rep_dim, y.nflat, st));
    NcReduceArgs r;
    for (int l = 2; l >= 1; --l) {
        RC(conv_bwd(y.c[l], ws + y.act[l - 1], ws + y.dact[l], ws + y.dact[l - 1], ws + y.part[l], w + 2 * l, 0, B, 1, st));
        conv_reduce_add(r, l - 1, y.c[l], ws + y.part[l], dw + 2 * l, 0, 1);
    }
    RC(nc_dw_reduce_launch(r, st));
    // first layer: ws.dact[0] is the gradient of its pre-activation (layer 2's dX applies the mask of act[0])
    RC(pc_conv1_dw_launch(tokens, ws + y.dact[0], ws + y.part[0], B, H, W, D, st));
    RC(pc_conv1_dw_reduce_launch(ws + y.part[0], dw[0], dw[1], B, H, W, D, st));
    if (dtokens) RC(pc_conv1_dx_launch(ws + y.dact[0], w[0], ws + y.wd, dtokens, B, H, W, D, st));
    return 0;
}

}  // extern "C"
