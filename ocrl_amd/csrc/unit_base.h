// What the stateless head units (pool, rn, naturecnn, pool_cnn, vae, probe, mae _unit.cpp) share on the host side, and nothing else.
// Each rule below decides the size of a workspace or the order a sum runs in, so it is written here once and nowhere else:
// the workspace check, the stride-4 padding, the split-k scratch of the Linear weight gradients, and the implicit-GEMM conv layer of
// naturecnn.hip with its weight-gradient slabs.
#pragma once
#include <utility>

#include "kernels.h"

// ---- workspace check: the message every entry point reports an undersized `ws` with
inline int ws_check(const char* entry, size_t have, size_t need) {
    OCRL_REQUIRE(have >= need, "%s: workspace too small (%zu < %zu floats)", entry, have, need);
    return 0;
}

// ---- stride-4 padding: the GEMM reads rows at a stride that is a multiple of 4, so an input of width D with D % 4 != 0 runs as a
// zero-padded copy of width pad4(D) in the workspace (rows and the weight that multiplies them alike), and its gradient lands in a
// padded buffer first and is copied out without the pad columns.  D % 4 == 0 uses the caller's pointers and launches nothing.
inline int pad4(int D) { return (D + 3) & ~3; }
inline size_t pad4_floats(size_t rows, int D) { return D % 4 ? rows * pad4(D) : 0; }      // the padded copy's size; 0 when none is made
// *view = the [rows, pad4(D)] form of src [rows, D]: `buf`, filled here, or src itself
inline int pad4_view(const float* src, int D, float* buf, long long rows, const float** view, hipStream_t st) {
    *view = D % 4 ? buf : src;
    return D % 4 ? pool_cols_launch(src, D, buf, pad4(D), rows, pad4(D), D, st) : 0;
}
// the pointer a product of width pad4(D) uses: the padded buffer, or the caller's own
template <class T> T* pad4_sel(T* own, int D, T* buf) { return D % 4 ? buf : own; }
// the reverse for a gradient written to pad4_sel(dst, D, buf): its D real columns into dst
inline int pad4_unpad(const float* buf, int D, float* dst, long long rows, hipStream_t st) {
    return D % 4 ? pool_cols_launch(buf, pad4(D), dst, D, rows, D, D, st) : 0;
}

// ---- split-k scratch of the Linear weight gradients (lin_bwd_w): the `rows` are the k dimension, split into up to 32 slabs of >= 256
// rows; per_split is the caller's largest weight plus its bias terms.  lin_bwd_w picks its split count from this size, so the
// per_split terms of the units differ on purpose and stay as they are.
inline size_t splitk_scratch_floats(size_t rows, size_t per_split) {
    size_t splits = rows / 256;
    if (splits > 32) splits = 32;
    return splits > 1 ? splits * per_split : 0;
}

// ---- implicit-GEMM conv layers (naturecnn.hip)
// The weight gradient reduces over the M = B OH OW rows: up to 64 slabs of >= 64 rows, the rows of a slab rounded up to 4; nc_dw_reduce
// sums the slabs in slab order.  The partial buffer is slabs * G * cout * (K + 1) floats, K = cin ks ks.
struct ConvSlab { int slabs = 1, rows = 4; };
inline ConvSlab conv_slab(long long M) {
    ConvSlab s;
    long long n = (M + 63) / 64;
    if (n > 64) n = 64;
    const long long rows = ((M + n - 1) / n + 3) & ~3LL;
    s.rows = (int)rows;
    s.slabs = (int)((M + rows - 1) / rows);
    return s;
}

struct ConvLayer {
    int cin = 0, cout = 0, ks = 0, stride = 0, pad = 0, H = 0, W = 0, OH = 0, OW = 0;      // channels per group
    ConvSlab slab;
    NcMap x, y;                                    // layouts of the input and the output map: the unit sets them
    int K() const { return cin * ks * ks; }
};
inline ConvLayer conv_layer(int B, int cin, int cout, int ks, int stride, int pad, int H, int W) {
    ConvLayer c;
    c.cin = cin; c.cout = cout; c.ks = ks; c.stride = stride; c.pad = pad; c.H = H; c.W = W;
    c.OH = (H + 2 * pad - ks) / stride + 1; c.OW = (W + 2 * pad - ks) / stride + 1;
    c.slab = conv_slab((long long)B * c.OH * c.OW);
    return c;
}
// the NatureCNN stack (L = 3, or 4 with cnn_feat_size 2) on an H x W input of cin channels
inline void nc_stack(ConvLayer* c, int L, int B, int cin, int H, int W) {
    static const int KS[4] = {8, 4, 3, 3}, ST[4] = {4, 2, 1, 1}, CO[4] = {32, 64, 64, 128};
    for (int l = 0; l < L; ++l) {
        c[l] = conv_layer(B, cin, CO[l], KS[l], ST[l], 0, H, W);
        H = c[l].OH; W = c[l].OW; cin = CO[l];
    }
}

// The three calls take the layer's parameters as wb: group g's weight is wb[g * np], its bias (or bias gradient) follows it.
// relu(conv(X) + bias) -> Y (and Y2 when given)
inline int conv_fwd(const ConvLayer& c, const float* X, float* Y, float* Y2, const float* const* wb, int np, int B, int G, hipStream_t st) {
    NcFwdArgs a;
    a.X = X; a.x = c.x; a.Y = Y; a.Y2 = Y2; a.y = c.y;
    for (int g = 0; g < G; ++g) { a.w[g] = wb[g * np]; a.bias[g] = wb[g * np + 1]; }
    a.B = B; a.G = G; a.cin = c.cin; a.cout = c.cout; a.H = c.H; a.W = c.W; a.OH = c.OH; a.OW = c.OW; a.ks = c.ks; a.stride = c.stride; a.pad = c.pad;
    return nc_conv_fwd_launch(a, st);
}
// the dW / db slab partials into `part` and, when dX, the gradient of the input masked by X > 0
inline int conv_bwd(const ConvLayer& c, const float* X, const float* dY, float* dX, float* part, const float* const* wb, int np, int B, int G,
                    hipStream_t st) {
    NcBwdArgs a;
    a.X = X; a.x = c.x; a.dY = dY; a.dy = c.y; a.dX = dX; a.part = part; a.slabs = c.slab.slabs; a.slab_rows = c.slab.rows;
    for (int g = 0; g < G; ++g) a.w[g] = wb[g * np];
    a.B = B; a.G = G; a.cin = c.cin; a.cout = c.cout; a.H = c.H; a.W = c.W; a.OH = c.OH; a.OW = c.OW; a.ks = c.ks; a.stride = c.stride; a.pad = c.pad;
    return nc_conv_bwd_launch(a, st);
}
// entry `i` of the one nc_dw_reduce launch that sums this layer's partials into dwb
inline void conv_reduce_add(NcReduceArgs& r, int i, const ConvLayer& c, const float* part, float* const* dwb, int np, int G) {
    NcReduceLayer& q = r.L[i];
    q.part = part; q.slabs = c.slab.slabs; q.G = G; q.cout = c.cout; q.K = c.K();
    q.n = (long long)G * q.cout * (q.K + 1);
    for (int g = 0; g < G; ++g) { r.dw[i][g] = dwb[g * np]; r.db[i][g] = dwb[g * np + 1]; }
    if (i >= r.nlayers) r.nlayers = i + 1;
}

// The Linear tail of the NatureCNN-shaped units, backward: dz = dout * (lin > 0), then per module g (column block g of [B, G rep])
// dW_g = dz_g^T flat_g, db_g = column sums of dz_g (B rows: no split-k scratch), d flat_g = (dz_g W_g) * (flat_g > 0).
inline int nc_tail_bwd(const float* dout, const float* lin, float* dz, const float* flat, float* dflat, const float* const* wb, float* const* dwb,
                       int np, int B, int G, int rep, int nflat, hipStream_t st) {
    RC(nc_relu_mask_launch(dout, lin, dz, (long long)B * G * rep, st));
    for (int g = 0; g < G; ++g) {
        const size_t xo = (size_t)g * B * nflat;
        RC(lin_bwd_w(dz + (size_t)g * rep, G * rep, flat + xo, nflat, dwb[g * np], dwb[g * np + 1], B, rep, nflat, 1.f, nullptr, 0, st));
        RC(lin_bwd_x(dz + (size_t)g * rep, G * rep, wb[g * np], dflat + xo, nflat, B, rep, nflat, flat + xo, nflat, nullptr, 0, st));
    }
    return 0;
}
