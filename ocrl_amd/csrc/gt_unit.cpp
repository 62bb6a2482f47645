// C ABI of the ground-truth-state encoder's per-object MLP (include/ocrl_hip.h: ocrl_gt_mlp_*): ocrs/gt/gt_module.py:14-27.
// Stateless: the caller owns parameters, gradients and the workspace; forward leaves every layer's output in `ws` for the backward.
#include "gt.h"
#include "unit_base.h"

namespace {
struct GtLay {
    size_t h[OCRL_GT_MLP_MAX_LAYERS], part, total;
    int P;                                          // floats of one slab's partial: W0, b0, W1, b1, ..
    GtSlab slab;
};

int check_gt(int M, int D, int nl, const int* dims) {
    OCRL_REQUIRE(M >= 1 && M < (1 << 22), "gt_mlp: 1 <= rows < 2^22 (got %d)", M);
    OCRL_REQUIRE(D >= 1 && D <= 64, "gt_mlp: input width must be 1 .. 64 (got %d)", D);
    OCRL_REQUIRE(nl >= 1 && nl <= OCRL_GT_MLP_MAX_LAYERS && dims, "gt_mlp: 1 <= len(dims) <= %d (got %d)", OCRL_GT_MLP_MAX_LAYERS, nl);
    for (int l = 0; l < nl; ++l)
        OCRL_REQUIRE(dims[l] >= 4 && dims[l] <= 256 && dims[l] % 4 == 0, "gt_mlp: dims[%d] = %d is not a multiple of 4 in 4 .. 256", l, dims[l]);
    return 0;
}

GtLay gt_layout(int M, int D, int nl, const int* dims) {
    GtLay y;
    WsTake take;
    y.P = 0;
    for (int l = 0; l < nl; ++l) {
        y.h[l] = take((size_t)M * dims[l]);
        y.P += dims[l] * (l ? dims[l - 1] : D) + dims[l];
    }
    y.slab = gt_slab(M);
    // sized for the cap, not for the slab count: that one dips where the tiles per slab go up (65 tiles are 33 slabs of 2), and a
    // workspace that shrinks as M grows would surprise a caller who sizes it once for his largest batch
    const int cap = y.slab.tiles < GT_MAX_SLABS ? y.slab.tiles : GT_MAX_SLABS;
    y.part = take(cap > 1 ? (size_t)cap * y.P : 0);
    y.total = take.end;
    return y;
}
}  // namespace

extern "C" {

size_t ocrl_gt_mlp_ws_floats(int M, int D, int nl, const int* dims) {
    if (check_gt(M, D, nl, dims)) return 0;                             // the shapes fwd / bwd reject get no workspace
    return gt_layout(M, D, nl, dims).total;
}

int ocrl_gt_mlp_fwd(const float* x, const float* const* w, float* out, int M, int D, int nl, const int* dims, const int* acts, float* ws,
                    size_t ws_floats, void* stream) {
    OCRL_REQUIRE(x && w && out && acts && ws, "ocrl_gt_mlp_fwd: null argument");
    RC(check_gt(M, D, nl, dims));
    const GtLay y = gt_layout(M, D, nl, dims);
    RC(ws_check("ocrl_gt_mlp_fwd", ws_floats, y.total));
    GtFwdArgs a = {};
    a.x = x; a.out = out; a.M = M; a.D = D; a.nl = nl;
    for (int l = 0; l < nl; ++l) {
        OCRL_REQUIRE(w[2 * l] && w[2 * l + 1], "ocrl_gt_mlp_fwd: null parameter of layer %d", l);
        a.w[l] = w[2 * l]; a.b[l] = w[2 * l + 1]; a.h[l] = ws + y.h[l]; a.dims[l] = dims[l]; a.relu[l] = acts[l] != 0;
    }
    return gt_mlp_fwd_launch(a, static_cast<hipStream_t>(stream));
}

int ocrl_gt_mlp_bwd(const float* x, const float* dout, const float* const* w, float* dx, float* const* dw, int M, int D, int nl, const int* dims,
                    const int* acts, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(x && dout && w && dw && acts && ws, "ocrl_gt_mlp_bwd: null argument");
    RC(check_gt(M, D, nl, dims));
    const GtLay y = gt_layout(M, D, nl, dims);
    RC(ws_check("ocrl_gt_mlp_bwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool direct = y.slab.slabs == 1;                              // one slab: its partial is the gradient
    GtBwdArgs a = {};
    GtReduceArgs r = {};
    a.x = x; a.dout = dout; a.dx = dx; a.M = M; a.D = D; a.nl = nl; a.per_slab = y.slab.per_slab; a.slab_stride = y.P;
    r.part = ws + y.part; r.n = 2 * nl; r.P = y.P; r.slabs = y.slab.slabs;
    int off = 0;
    for (int l = 0; l < nl; ++l) {
        OCRL_REQUIRE(w[2 * l] && dw[2 * l] && dw[2 * l + 1], "ocrl_gt_mlp_bwd: null parameter or gradient of layer %d", l);
        const int nw = dims[l] * (l ? dims[l - 1] : D);
        a.w[l] = w[2 * l]; a.h[l] = ws + y.h[l]; a.dims[l] = dims[l]; a.relu[l] = acts[l] != 0;
        a.dw[l] = direct ? dw[2 * l] : ws + y.part + off;
        a.db[l] = direct ? dw[2 * l + 1] : ws + y.part + off + nw;
        r.dst[2 * l] = dw[2 * l]; r.dst[2 * l + 1] = dw[2 * l + 1];
        r.end[2 * l] = off + nw; r.end[2 * l + 1] = off + nw + dims[l];
        off += nw + dims[l];
    }
    RC(gt_mlp_bwd_launch(a, y.slab.slabs, st));
    return direct ? 0 : gt_mlp_reduce_launch(r, st);
}

}  // extern "C"
