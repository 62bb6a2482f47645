// C ABI of the NatureCNN pooling heads (include/ocrl_hip.h: ocrl_pool_cnn_*): poolings/cnn_linear/cnn_linear_module.py:7-14 and the CNN
// front end of poolings/cnn_transformer/cnn_transformer_module.py:12-40, over slot_to_img(tokens) (utils/tools.py:33-36), which for a
// [B, H W, D] token map is a view: the map already is the channels-last image.  The first convolution, its weight gradient and its
// input gradient are pool_cnn.hip; layers 2 and 3, the ReLU masks and the Linear are the launches of the NatureCNN encoder
// (naturecnn.hip, gemm.hip) with one group.
//   forward   1 pack + 3 conv launches [+ 1 GEMM (+ 1 copy of the output into ws when saving)]
//   backward  1 mask [+ 2 GEMMs] + 2 conv launches (layers 3, 2: dW partials and the masked dX in one) + the first layer's dW partials
//             + 2 reduces [+ 1 pack + the per-phase dX when the tokens want a gradient]
// Stateless: the caller owns the parameters, their gradients and the workspace.
#include "../../include/ocrl_hip.h"
#include "kernels.h"

namespace {
struct PcLay {
    PcGeom g;
    int cin[3], cout[3], ks[3], st[3], H[3], W[3], OH[3], OW[3], slabs[3], slab_rows[3];
    NcMap ymap[3];
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
    static const int KS[3] = {8, 4, 3}, ST[3] = {4, 2, 1}, CO[3] = {32, 64, 64};
    y.g = pc_geom(B, H, W, D);
    int h = H, w = W, c = D;
    for (int l = 0; l < 3; ++l) {
        y.cin[l] = c; y.cout[l] = CO[l]; y.ks[l] = KS[l]; y.st[l] = ST[l]; y.H[l] = h; y.W[l] = w;
        y.OH[l] = (h - KS[l]) / ST[l] + 1; y.OW[l] = (w - KS[l]) / ST[l] + 1;
        h = y.OH[l]; w = y.OW[l]; c = CO[l];
    }
    y.wp = take(y.g.wp_floats);
    y.wd = take(y.g.wd_floats);
    for (int l = 0; l < 3; ++l) {
        const long long C = y.cout[l], hw = (long long)y.OH[l] * y.OW[l];
        NcMap& o = y.ymap[l];
        if (l < 2 || rep > 0) { o.sN = C * hw; o.sG = 0; o.sC = hw; o.sH = y.OW[l]; o.sW = 1; }       // [B, C, OH, OW]; the last one flattens NCHW
        else { o.sN = hw * C; o.sG = 0; o.sC = 1; o.sH = y.OW[l] * C; o.sW = C; }                       // [B, OH OW, C] tokens
        const size_t n = (size_t)B * C * hw;
        y.act[l] = take(n); y.dact[l] = take(n);
        if (l == 0) { y.part[0] = take(y.g.part_floats); continue; }
        // as the NatureCNN encoder: up to 64 slabs of >= 64 of the B OH OW rows, summed in slab order by nc_dw_reduce
        const long long M = (long long)B * hw;
        long long s = (M + 63) / 64;
        if (s > 64) s = 64;
        const long long rows = ((M + s - 1) / s + 3) & ~3LL;
        y.slab_rows[l] = (int)rows;
        y.slabs[l] = (int)((M + rows - 1) / rows);
        y.part[l] = take((size_t)y.slabs[l] * C * ((size_t)y.cin[l] * KS[l] * KS[l] + 1));
    }
    y.nflat = y.cout[2] * y.OH[2] * y.OW[2];
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
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_pool_cnn_fwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    RC(pc_conv1_fwd_launch(tokens, w[0], w[1], ws + y.wp, ws + y.act[0], B, H, W, D, st));
    for (int l = 1; l < 3; ++l) {
        NcFwdArgs a;
        a.X = ws + y.act[l - 1]; a.x = y.ymap[l - 1];
        const bool to_out = rep_dim == 0 && l == 2;
        a.Y = to_out ? out : ws + y.act[l];
        a.Y2 = to_out && save ? ws + y.act[l] : nullptr;
        a.y = y.ymap[l];
        a.w[0] = w[2 * l]; a.bias[0] = w[2 * l + 1];
        a.B = B; a.G = 1; a.cin = y.cin[l]; a.cout = y.cout[l]; a.H = y.H[l]; a.W = y.W[l]; a.OH = y.OH[l]; a.OW = y.OW[l];
        a.ks = y.ks[l]; a.stride = y.st[l];
        RC(nc_conv_fwd_launch(a, st));
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
    OCRL_REQUIRE(ws_floats >= y.total, "ocrl_pool_cnn_bwd: workspace too small (%zu < %zu floats)", ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (rep_dim == 0) {
        RC(nc_relu_mask_launch(dout, ws + y.act[2], ws + y.dact[2], (long long)B * y.nflat, st));      // tokens: same layout as out
    } else {
        RC(nc_relu_mask_launch(dout, ws + y.lin, ws + y.dz, (long long)B * rep_dim, st));
        const float* flat = ws + y.act[2];
        // dW = dz^T flat, db = column sums of dz (B rows: no split-k scratch); d flat = (dz W) * (flat > 0)
        RC(lin_bwd_w(ws + y.dz, rep_dim, flat, y.nflat, dw[6], dw[7], B, rep_dim, y.nflat, 1.f, nullptr, 0, st));
        RC(lin_bwd_x(ws + y.dz, rep_dim, w[6], ws + y.dact[2], y.nflat, B, rep_dim, y.nflat, flat, y.nflat, nullptr, 0, st));
    }
    NcReduceArgs r;
    r.nlayers = 2;
    for (int l = 2; l >= 1; --l) {
        NcBwdArgs a;
        a.X = ws + y.act[l - 1]; a.x = y.ymap[l - 1];
        a.dY = ws + y.dact[l]; a.dy = y.ymap[l];
        a.dX = ws + y.dact[l - 1];
        a.part = ws + y.part[l]; a.slabs = y.slabs[l]; a.slab_rows = y.slab_rows[l];
        a.w[0] = w[2 * l];
        a.B = B; a.G = 1; a.cin = y.cin[l]; a.cout = y.cout[l]; a.H = y.H[l]; a.W = y.W[l]; a.OH = y.OH[l]; a.OW = y.OW[l];
        a.ks = y.ks[l]; a.stride = y.st[l];
        RC(nc_conv_bwd_launch(a, st));
        NcReduceLayer& q = r.L[l - 1];
        q.part = ws + y.part[l]; q.slabs = y.slabs[l]; q.G = 1; q.cout = y.cout[l]; q.K = y.cin[l] * y.ks[l] * y.ks[l];
        q.n = (long long)q.cout * (q.K + 1);
        r.dw[l - 1][0] = dw[2 * l]; r.db[l - 1][0] = dw[2 * l + 1];
    }
    RC(nc_dw_reduce_launch(r, st));
    // first layer: ws.dact[0] is the gradient of its pre-activation (layer 2's dX applies the mask of act[0])
    RC(pc_conv1_dw_launch(tokens, ws + y.dact[0], ws + y.part[0], B, H, W, D, st));
    RC(pc_conv1_dw_reduce_launch(ws + y.part[0], dw[0], dw[1], B, H, W, D, st));
    if (dtokens) RC(pc_conv1_dx_launch(ws + y.dact[0], w[0], ws + y.wd, dtokens, B, H, W, D, st));
    return 0;
}

}  // extern "C"
