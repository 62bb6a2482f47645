// C ABI of the slot property probe (include/ocrl_hip.h: ocrl_probe_*): utils/property_predictor.py:12-189 of the reference.
// Head: nl Linear layers with LeakyReLU between them (model_type linear: nl = 1; mlp3: nl = 4, hidden width 256) on the encoder rows
// ([B K, D] slot rows, or [B, D] rows whose K O outputs are read as K pseudo-slots: the VAE branch), on the library's GEMM.  The input
// width is padded as unit_base.h says; the last layer's output width is zero-padded to a multiple of 4 here (it is 15 wide for the
// default schema; the pad rows of its weight are zero, so are the pad columns of d out).  Then probe.hip: cost matrix, exact
// assignment, loss, metrics, d out.  Stateless: the caller owns parameters, gradients and the workspace; forward leaves what backward
// needs in `ws` (the activations and the unscaled d loss / d out), backward scales by the incoming d loss and walks the layers down.
// The rows get no gradient: the probe reads a detached encoder.
#include <hip/hip_runtime.h>

#include "../../include/ocrl_hip.h"
#include "unit_base.h"

namespace {
struct ProbeLay {
    int Dp, Hp, M;                                         // padded input / head output width, head rows
    size_t xp, wl, bl, dwl, dbl, dw0, h[OCRL_PROBE_MAX_LAYERS], gout, gA, gB, part, sk, sk_floats, total;
};

int check_head(int B, int K, int D, int O, int slot_rows, int nl, const int* dims) {
    OCRL_REQUIRE(B >= 1 && K >= 1 && D >= 1 && O >= 1, "probe: batch, slots, rep_dim and outputs per slot >= 1 (got %d, %d, %d, %d)", B, K, D, O);
    OCRL_REQUIRE(nl >= 1 && nl <= OCRL_PROBE_MAX_LAYERS && dims, "probe: 1 <= layers <= %d (got %d)", OCRL_PROBE_MAX_LAYERS, nl);
    for (int l = 0; l + 1 < nl; ++l)
        OCRL_REQUIRE(dims[l] >= 4 && dims[l] % 4 == 0, "probe: hidden width dims[%d] = %d is not a positive multiple of 4", l, dims[l]);
    const long long want = slot_rows ? O : (long long)K * O;
    OCRL_REQUIRE(dims[nl - 1] == want, "probe: the last layer is %d wide, the schema needs %lld", dims[nl - 1], want);
    long long wmax = pad4(D);
    for (int l = 0; l < nl; ++l) wmax = dims[l] + 3 > wmax ? pad4(dims[l]) : wmax;
    OCRL_REQUIRE((long long)B * (slot_rows ? K : 1) * wmax < (1LL << 31), "probe: %d images exceed the int32 range of one call", B);
    return 0;
}

ProbeLay probe_layout(int B, int K, int N, int D, int slot_rows, int nl, const int* dims, int P) {
    ProbeLay y;
    WsTake take;
    y.Dp = pad4(D);
    y.Hp = pad4(dims[nl - 1]);
    y.M = slot_rows ? B * K : B;
    const size_t M = y.M, kin_last = nl > 1 ? dims[nl - 2] : y.Dp;
    y.xp = take(pad4_floats(M, D));
    y.wl = take((size_t)y.Hp * kin_last); y.bl = take(y.Hp);
    y.dwl = take((size_t)y.Hp * kin_last); y.dbl = take(y.Hp);
    y.dw0 = take(nl > 1 ? pad4_floats(dims[0], D) : 0);
    size_t wmax = y.Hp, slab = (size_t)y.Hp * kin_last;
    for (int l = 0; l < nl; ++l) {
        const size_t wl = l == nl - 1 ? y.Hp : dims[l], kin = l ? dims[l - 1] : y.Dp;
        y.h[l] = take(M * wl);
        wmax = wl > wmax ? wl : wmax;
        slab = wl * kin > slab ? wl * kin : slab;
    }
    y.gout = take(M * y.Hp);
    y.gA = take(M * wmax); y.gB = take(M * wmax);
    y.part = take((size_t)B * (P + 2));
    y.sk_floats = splitk_scratch_floats(M, slab + wmax + 4);      // the head rows are the k dimension of the weight gradients
    y.sk = take(y.sk_floats);
    y.total = take.end;
    return y;
}

int make_schema(int P, const int* tgt_range, const int* out_range, const int* kind, ProbeSchema* sc) {
    OCRL_REQUIRE(P >= 1 && P <= OCRL_PROBE_MAX_PROPS && tgt_range && out_range && kind, "probe: 1 <= properties <= %d with their ranges (got %d)",
                 OCRL_PROBE_MAX_PROPS, P);
    sc->P = P;
    for (int p = 0; p < P; ++p) {
        sc->t[p] = tgt_range[2 * p]; sc->a[p] = out_range[2 * p]; sc->b[p] = out_range[2 * p + 1]; sc->kind[p] = kind[p];
        OCRL_REQUIRE(tgt_range[2 * p + 1] - tgt_range[2 * p] == (kind[p] == 1 ? 2 : 1), "probe: property %d reads %d target columns; xy reads 2, a class 1",
                     p, tgt_range[2 * p + 1] - tgt_range[2 * p]);
    }
    return 0;
}
}  // namespace

static_assert(OCRL_PROBE_MAX_SLOTS == PROBE_MAX_SLOTS && OCRL_PROBE_MAX_PROPS == PROBE_MAX_PROPS, "header and kernel limits differ");

extern "C" {

size_t ocrl_probe_match_ws_floats(int B, int P) {
    if (B < 1 || P < 1 || P > OCRL_PROBE_MAX_PROPS) return 0;
    return (size_t)B * (P + 2);
}

int ocrl_probe_match(const float* out, int ld_row, long long ld_img, const float* y, const float* dloss, float* cost, int* col, float* metrics,
                     float* dout, int B, int K, int N, int T, int O, int P, const int* tgt_range, const int* out_range, const int* kind, float* ws,
                     size_t ws_floats, void* stream) {
    OCRL_REQUIRE(out && y && metrics && ws, "ocrl_probe_match: null argument");
    ProbeSchema sc;
    RC(make_schema(P, tgt_range, out_range, kind, &sc));
    RC(ws_check("ocrl_probe_match", ws_floats, (size_t)B * (P + 2)));
    return probe_match_launch(out, ld_row, ld_img, y, dloss, cost, col, ws, metrics, dout, B, K, N, T, O, sc, static_cast<hipStream_t>(stream));
}

size_t ocrl_probe_ws_floats(int B, int K, int N, int D, int O, int slot_rows, int nl, const int* dims, int P) {
    if (check_head(B, K, D, O, slot_rows, nl, dims) || probe_match_check(B, K, N, 1, O) || P < 1 || P > OCRL_PROBE_MAX_PROPS) return 0;
    return probe_layout(B, K, N, D, slot_rows, nl, dims, P).total;
}

int ocrl_probe_fwd(const float* rows, const float* const* w, const float* y, float* out, float* cost, int* col, float* metrics, int B, int K, int N,
                   int D, int T, int O, int slot_rows, int nl, const int* dims, float slope, int P, const int* tgt_range, const int* out_range,
                   const int* kind, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(rows && w && y && metrics && ws, "ocrl_probe_fwd: null argument");
    RC(check_head(B, K, D, O, slot_rows, nl, dims));
    RC(probe_match_check(B, K, N, T, O));
    ProbeSchema sc;
    RC(make_schema(P, tgt_range, out_range, kind, &sc));
    RC(probe_schema_check(sc, T, O));
    const ProbeLay L = probe_layout(B, K, N, D, slot_rows, nl, dims, P);
    RC(ws_check("ocrl_probe_fwd", ws_floats, L.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long M = L.M;
    const int H = dims[nl - 1], Hp = L.Hp, kin_last = nl > 1 ? dims[nl - 2] : L.Dp;
    const float* x;
    RC(pad4_view(rows, D, ws + L.xp, M, &x, st));
    // the last layer's weight padded to Hp output rows (and, as the only layer, to Dp input columns)
    const int kin_real = nl > 1 ? dims[nl - 2] : D;
    OCRL_HIP(hipMemsetAsync(ws + L.wl, 0, (size_t)Hp * kin_last * sizeof(float), st));
    RC(pool_cols_launch(w[2 * (nl - 1)], kin_real, ws + L.wl, kin_last, H, kin_last, kin_real, st));
    RC(vae_pad_rows_launch(w[2 * (nl - 1) + 1], ws + L.bl, H, Hp, 1, st));
    for (int l = 0; l < nl; ++l) {
        const bool last = l == nl - 1;
        const int kin = l ? dims[l - 1] : L.Dp, wout = last ? Hp : dims[l];
        const float* W = last ? ws + L.wl : w[2 * l];
        const float* bias = last ? ws + L.bl : w[2 * l + 1];
        if (l == 0 && !last) RC(pad4_view(w[0], D, ws + L.dw0, dims[0], &W, st));      // first of several layers: its weight padded in dw0's place
        RC(lin_fwd(l ? ws + L.h[l - 1] : x, kin, W, bias, ws + L.h[l], wout, M, wout, kin, 0, nullptr, 0, st));
        if (!last) RC(probe_leaky_fwd_launch(ws + L.h[l], M * wout, slope, st));
    }
    const float* ho = ws + L.h[nl - 1];                    // [M, Hp]
    if (out) RC(pool_cols_launch(ho, Hp, out, H, M, H, H, st));
    OCRL_HIP(hipMemsetAsync(ws + L.gout, 0, (size_t)M * Hp * sizeof(float), st));
    const int ld_row = slot_rows ? Hp : O;
    const long long ld_img = slot_rows ? (long long)K * Hp : Hp;
    return probe_match_launch(ho, ld_row, ld_img, y, nullptr, cost, col, ws + L.part, metrics, ws + L.gout, B, K, N, T, O, sc, st);
}

int ocrl_probe_bwd(const float* rows, const float* dloss, const float* const* w, float* const* dw, int B, int K, int N, int D, int O, int slot_rows,
                   int nl, const int* dims, float slope, int P, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(rows && w && dw && ws, "ocrl_probe_bwd: null argument");
    RC(check_head(B, K, D, O, slot_rows, nl, dims));
    RC(probe_match_check(B, K, N, 1, O));
    OCRL_REQUIRE(P >= 1 && P <= OCRL_PROBE_MAX_PROPS, "ocrl_probe_bwd: 1 <= properties <= %d (got %d)", OCRL_PROBE_MAX_PROPS, P);
    const ProbeLay L = probe_layout(B, K, N, D, slot_rows, nl, dims, P);
    RC(ws_check("ocrl_probe_bwd", ws_floats, L.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long M = L.M;
    const int H = dims[nl - 1], Hp = L.Hp;
    const float* x = pad4_sel<const float>(rows, D, ws + L.xp);      // the padded copy the forward left in ws
    float *gc = ws + L.gA, *gn = ws + L.gB;
    RC(vae_scale_launch(ws + L.gout, gc, dloss, M * Hp, st));
    for (int l = nl - 1; l >= 0; --l) {
        const bool last = l == nl - 1;
        const int kin = l ? dims[l - 1] : L.Dp, wout = last ? Hp : dims[l];
        const float* xin = l ? ws + L.h[l - 1] : x;
        // padded gradients land in ws first: the last layer's pad rows, the first layer's pad columns
        float* dW = last ? ws + L.dwl : (l ? dw[2 * l] : pad4_sel(dw[0], D, ws + L.dw0));
        float* db = last ? ws + L.dbl : dw[2 * l + 1];
        if (l > 0) RC(lin_bwd_x(gc, wout, last ? ws + L.wl : w[2 * l], gn, kin, M, wout, kin, nullptr, 0, nullptr, 0, st));
        RC(lin_bwd_w(gc, wout, xin, kin, dW, db, M, wout, kin, 1.f, ws + L.sk, L.sk_floats, st));
        if (last) {
            RC(pool_cols_launch(ws + L.dwl, kin, dw[2 * l], l ? kin : D, H, l ? kin : D, l ? kin : D, st));
            RC(copy_launch(ws + L.dbl, dw[2 * l + 1], H, st));
        } else if (l == 0) {
            RC(pad4_unpad(ws + L.dw0, D, dw[0], dims[0], st));
        }
        if (l > 0) {
            RC(probe_leaky_bwd_launch(gn, ws + L.h[l - 1], M * kin, slope, st));
            std::swap(gc, gn);
        }
    }
    return 0;
}

}  // extern "C"
