// C ABI of the Relation Network pooling head (include/ocrl_hip.h: ocrl_pool_rn_*): poolings/rn/rn_module.py:8-59.
// g = [Linear, ReLU] x ng on every ordered slot pair cat(s_i, s_j), summed over the pairs, then f = [Linear, ReLU] x nf.
// The first g layer is factored: its weight W1 [g1, 2D] splits into U = W1[:, :D] and V = W1[:, D:], and pair row (i, j) is
// relu(U s_i + V s_j + b1).  Both halves are stacked into W1s = [U; V] ([2 g1, Dp], Dp = pad4(rep_dim): unit_base.h), so one
// GEMM over the B K slot rows gives AB = [A | Bq] and rn_pair_fwd expands the pairs with an addition.  The other layers run on the
// library's GEMM (bias and ReLU in the epilogue; the ReLU mask of the backward in the dX epilogue).  Stateless: the caller owns
// parameters, gradients and the workspace; forward leaves what backward needs in `ws`.
#include "../../include/ocrl_hip.h"
#include "unit_base.h"

namespace {
struct RnLay {
    int Dp, P, gmax, fmax;
    size_t sp, dsp, w1s, dw1s, db1s, ab, dab, h[OCRL_POOL_RN_MAX_LAYERS], y, f[OCRL_POOL_RN_MAX_LAYERS], gA, gB, fA, fB, sk, sk_floats, total;
};

int check_rn(int B, int K, int D, int ng, const int* g_dims, int nf, const int* f_dims) {
    OCRL_REQUIRE(B >= 1 && K >= 2 && D >= 1, "pool_rn: batch >= 1, num_slots >= 2 and rep_dim >= 1 (got %d, %d, %d)", B, K, D);
    OCRL_REQUIRE(ng >= 1 && ng <= OCRL_POOL_RN_MAX_LAYERS && nf >= 1 && nf <= OCRL_POOL_RN_MAX_LAYERS && g_dims && f_dims,
                 "pool_rn: 1 <= len(g_dims), len(f_dims) <= %d (got %d, %d)", OCRL_POOL_RN_MAX_LAYERS, ng, nf);
    long long gmax = 0;
    for (int l = 0; l < ng; ++l) {
        OCRL_REQUIRE(g_dims[l] >= 4 && g_dims[l] % 4 == 0, "pool_rn: g_dims[%d] = %d is not a positive multiple of 4", l, g_dims[l]);
        if (g_dims[l] > gmax) gmax = g_dims[l];
    }
    for (int l = 0; l < nf; ++l)
        OCRL_REQUIRE(f_dims[l] >= 4 && f_dims[l] % 4 == 0, "pool_rn: f_dims[%d] = %d is not a positive multiple of 4", l, f_dims[l]);
    // every GEMM extent and element count must stay in the int32 range of the kernels: the pair rows (B K (K-1)) times the widest g
    // layer bound them (a CNN feature map as "slots", K = 4096, is 16.8 M pairs per image and is rejected here)
    const long long BK = (long long)B * K, Dp = pad4(D);
    const long long pairs = BK * (K - 1);
    OCRL_REQUIRE(pairs * gmax < (1LL << 31) && BK * 2 * g_dims[0] < (1LL << 31) && BK * Dp < (1LL << 31),
                 "pool_rn: %lld pair rows of width %lld exceed the int32 range of one call (batch %d, %d slots)", pairs, gmax, B, K);
    return 0;
}

RnLay rn_layout(int B, int K, int D, int ng, const int* g_dims, int nf, const int* f_dims) {
    RnLay y;
    WsTake take;
    y.Dp = pad4(D);
    y.P = K * (K - 1);
    const size_t BK = (size_t)B * K, BP = (size_t)B * y.P, g1 = g_dims[0], gL = g_dims[ng - 1];
    y.gmax = 0; y.fmax = (int)gL;
    for (int l = 0; l < ng; ++l) y.gmax = g_dims[l] > y.gmax ? g_dims[l] : y.gmax;
    for (int l = 0; l < nf; ++l) y.fmax = f_dims[l] > y.fmax ? f_dims[l] : y.fmax;
    y.sp = take(pad4_floats(BK, D)); y.dsp = take(pad4_floats(BK, D));
    y.w1s = take(2 * g1 * y.Dp); y.dw1s = take(2 * g1 * y.Dp); y.db1s = take(2 * g1);
    y.ab = take(BK * 2 * g1); y.dab = take(BK * 2 * g1);
    for (int l = 0; l < ng; ++l) y.h[l] = take(BP * g_dims[l]);
    y.y = take((size_t)B * gL);
    for (int l = 0; l < nf; ++l) y.f[l] = take((size_t)B * f_dims[l]);
    y.gA = take(BP * y.gmax); y.gB = take(BP * y.gmax);
    y.fA = take((size_t)B * y.fmax); y.fB = take((size_t)B * y.fmax);
    // split-k scratch of the weight gradients: the pair rows are their k dimension; the largest weight and the widest bias
    size_t slab = 2 * g1 * y.Dp, bslab = 2 * g1;
    for (int l = 1; l < ng; ++l) slab = (size_t)g_dims[l] * g_dims[l - 1] > slab ? (size_t)g_dims[l] * g_dims[l - 1] : slab;
    for (int l = 0; l < nf; ++l) slab = (size_t)f_dims[l] * (l ? f_dims[l - 1] : gL) > slab ? (size_t)f_dims[l] * (l ? f_dims[l - 1] : gL) : slab;
    if ((size_t)y.gmax > bslab) bslab = y.gmax;
    if ((size_t)y.fmax > bslab) bslab = y.fmax;
    y.sk_floats = splitk_scratch_floats(BP, slab + bslab + 4);
    y.sk = take(y.sk_floats);
    y.total = take.end;
    return y;
}
}  // namespace

extern "C" {

size_t ocrl_pool_rn_ws_floats(int B, int K, int D, int ng, const int* g_dims, int nf, const int* f_dims) {
    if (check_rn(B, K, D, ng, g_dims, nf, f_dims)) return 0;            // the shapes fwd / bwd reject get no workspace
    return rn_layout(B, K, D, ng, g_dims, nf, f_dims).total;
}

int ocrl_pool_rn_fwd(const float* slots, const float* const* w, float* out, int B, int K, int D, int ng, const int* g_dims, int nf, const int* f_dims,
                     float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(slots && w && out && ws, "ocrl_pool_rn_fwd: null argument");
    RC(check_rn(B, K, D, ng, g_dims, nf, f_dims));
    const RnLay y = rn_layout(B, K, D, ng, g_dims, nf, f_dims);
    RC(ws_check("ocrl_pool_rn_fwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Dp = y.Dp, g1 = g_dims[0], gL = g_dims[ng - 1];
    const long long BK = (long long)B * K, BP = (long long)B * y.P;
    const float* xs;
    RC(pad4_view(slots, D, ws + y.sp, BK, &xs, st));
    RC(pool_cols_launch(w[0], 2 * D, ws + y.w1s, Dp, g1, Dp, D, st));                              // U = W1[:, :D]
    RC(pool_cols_launch(w[0] + D, 2 * D, ws + y.w1s + (size_t)g1 * Dp, Dp, g1, Dp, D, st));        // V = W1[:, D:]
    RC(lin_fwd(xs, Dp, ws + y.w1s, nullptr, ws + y.ab, 2 * g1, BK, 2 * g1, Dp, 0, nullptr, 0, st));   // [A | Bq] on the slot rows
    RC(rn_pair_fwd_launch(ws + y.ab, w[1], ws + y.h[0], B, K, g1, st));
    for (int l = 1; l < ng; ++l)
        RC(lin_fwd(ws + y.h[l - 1], g_dims[l - 1], w[2 * l], w[2 * l + 1], ws + y.h[l], g_dims[l], BP, g_dims[l], g_dims[l - 1], 1, nullptr, 0, st));
    RC(rn_pairsum_fwd_launch(ws + y.h[ng - 1], ws + y.y, B, y.P, gL, st));
    const float* const* wf = w + 2 * ng;
    for (int l = 0; l < nf; ++l) {
        const int kin = l ? f_dims[l - 1] : gL;
        RC(lin_fwd(l ? ws + y.f[l - 1] : ws + y.y, kin, wf[2 * l], wf[2 * l + 1], ws + y.f[l], f_dims[l], B, f_dims[l], kin, 1, nullptr, 0, st));
    }
    return copy_launch(ws + y.f[nf - 1], out, (long long)B * f_dims[nf - 1], st);
}

int ocrl_pool_rn_bwd(const float* slots, const float* dout, const float* const* w, float* dslots, float* const* dw, int B, int K, int D, int ng,
                     const int* g_dims, int nf, const int* f_dims, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(slots && dout && w && dw && ws, "ocrl_pool_rn_bwd: null argument");
    RC(check_rn(B, K, D, ng, g_dims, nf, f_dims));
    const RnLay y = rn_layout(B, K, D, ng, g_dims, nf, f_dims);
    RC(ws_check("ocrl_pool_rn_bwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Dp = y.Dp, g1 = g_dims[0], gL = g_dims[ng - 1];
    const long long BK = (long long)B * K, BP = (long long)B * y.P;
    float* sk = ws + y.sk;
    // f: the gradient of each layer's pre-activation; its dX product applies the previous layer's ReLU mask
    const float* const* wf = w + 2 * ng;
    float* const* dwf = dw + 2 * ng;
    float *fc = ws + y.fA, *fn = ws + y.fB;
    RC(rn_pairsum_bwd_launch(dout, ws + y.f[nf - 1], fc, B, 1, f_dims[nf - 1], st));               // dout * (out > 0)
    for (int l = nf - 1; l >= 0; --l) {
        const int kin = l ? f_dims[l - 1] : gL;
        RC(lin_bwd_w(fc, f_dims[l], l ? ws + y.f[l - 1] : ws + y.y, kin, dwf[2 * l], dwf[2 * l + 1], B, f_dims[l], kin, 1.f, sk, y.sk_floats, st));
        RC(lin_bwd_x(fc, f_dims[l], wf[2 * l], fn, kin, B, f_dims[l], kin, l ? ws + y.f[l - 1] : nullptr, kin, nullptr, 0, st));
        std::swap(fc, fn);
    }
    // fc = d loss / d (pair sum); g: broadcast over the pairs under the last layer's ReLU, then layer by layer down to the first
    float *gc = ws + y.gA, *gn = ws + y.gB;
    RC(rn_pairsum_bwd_launch(fc, ws + y.h[ng - 1], gc, B, y.P, gL, st));
    for (int l = ng - 1; l >= 1; --l) {
        RC(lin_bwd_w(gc, g_dims[l], ws + y.h[l - 1], g_dims[l - 1], dw[2 * l], dw[2 * l + 1], BP, g_dims[l], g_dims[l - 1], 1.f, sk, y.sk_floats, st));
        RC(lin_bwd_x(gc, g_dims[l], w[2 * l], gn, g_dims[l - 1], BP, g_dims[l], g_dims[l - 1], ws + y.h[l - 1], g_dims[l - 1], nullptr, 0, st));
        std::swap(gc, gn);
    }
    // the factored first layer: pair gradients -> [dA | dBq] on the slot rows -> dW1 = [dA^T s | dBq^T s], db1 = sum dA, dslots
    RC(rn_pair_bwd_launch(gc, ws + y.dab, B, K, g1, st));
    const float* xs = pad4_sel<const float>(slots, D, ws + y.sp);      // the padded copy the forward left in ws
    RC(lin_bwd_w(ws + y.dab, 2 * g1, xs, Dp, ws + y.dw1s, ws + y.db1s, BK, 2 * g1, Dp, 1.f, sk, y.sk_floats, st));
    RC(pool_cols_launch(ws + y.dw1s, Dp, dw[0], 2 * D, g1, D, D, st));
    RC(pool_cols_launch(ws + y.dw1s + (size_t)g1 * Dp, Dp, dw[0] + D, 2 * D, g1, D, D, st));
    RC(copy_launch(ws + y.db1s, dw[1], g1, st));
    if (dslots) {
        RC(lin_bwd_x(ws + y.dab, 2 * g1, ws + y.w1s, pad4_sel(dslots, D, ws + y.dsp), Dp, BK, 2 * g1, Dp, nullptr, 0, nullptr, 0, st));
        RC(pad4_unpad(ws + y.dsp, D, dslots, BK, st));
    }
    return 0;
}

}  // extern "C"
