// C ABI of the VAE representation module (include/ocrl_hip.h: ocrl_vae_*): ocrs/vaes/vae_module.py and ocrs/common/models.py:49-93.
// n = log2(obs_size / cnn_feat_size) stages; every map runs NHWC.
//   encoder   per stage: Conv2dBlock(k 2, s 2) on the naturecnn.hip implicit GEMM (stage 0 reads the NCHW observation), three 1 x 1
//             Conv2dBlocks on the GEMM; then the plain 1 x 1 conv2d (no ReLU).  Its [B, f, f, 64] output is img_to_slot's token order.
//   _mu/_var  one GEMM over [B, f f 64] against both weights stacked, their columns permuted from the NCHW flatten when packed
//   reparam   latent and the per-image KL partials in one kernel (vae.hip)
//   _in_dec   one GEMM whose weight rows and bias are permuted when packed, so its output is the NHWC map
//   decoder   1 x 1 Conv2dBlock, then per stage: 3 x 3 pad 1 (naturecnn.hip below 32 x 32, conv.hip from 32 x 32), three 1 x 1 on the
//             GEMM, PixelShuffle(2); then the 64 -> C conv2d as a 4-wide GEMM into the [B, S, S, 4] layout of mse_launch
// Stateless: the caller owns the parameters (read in torch's layout, packed per call into ws), the gradients and the workspace; the
// forward leaves in ws everything the backward reads.  Sums run in orders fixed by the shapes (no atomics).
#include "../../include/ocrl_hip.h"
#include "unit_base.h"

namespace {
constexpr int CONV_HIP_MIN = 32;      // decoder 3 x 3 maps from this size on run conv.hip's 4 x 32 pixel tiles; smaller ones naturecnn.hip's
constexpr size_t SK_FLOATS = (size_t)1 << 22;

struct VaeLay {
    int n = 0, f = 0, S = 0, C = 0, L = 0, B = 0, full = 0, cnn = 0;
    size_t ea[OCRL_VAE_MAX_STAGES][4] = {}, epart[OCRL_VAE_MAX_STAGES] = {}, e = 0;
    ConvLayer ec[OCRL_VAE_MAX_STAGES];             // the 2 x 2 stride 2 encoder convs
    size_t ml = 0, lat = 0, klp = 0, msews = 0, Wml = 0, bml = 0, Win = 0, bin = 0, Wo4 = 0, bo4 = 0;
    size_t hin = 0, d0 = 0, x3[OCRL_VAE_MAX_STAGES] = {}, y1[OCRL_VAE_MAX_STAGES] = {}, y2[OCRL_VAE_MAX_STAGES] = {},
           y4[OCRL_VAE_MAX_STAGES] = {}, ps[OCRL_VAE_MAX_STAGES] = {}, dpart[OCRL_VAE_MAX_STAGES] = {}, pkf[OCRL_VAE_MAX_STAGES] = {},
           pkb[OCRL_VAE_MAX_STAGES] = {};
    ConvLayer dc[OCRL_VAE_MAX_STAGES];             // the 3 x 3 pad 1 decoder convs below CONV_HIP_MIN
    size_t r4 = 0, dr4 = 0, drs = 0, ge = 0;
    size_t gA = 0, gB = 0, dml = 0, dlat = 0, dWml = 0, dbml = 0, dWin = 0, dbin = 0, dWo4 = 0, dbo4 = 0, sk = 0, sk_floats = 0;
    size_t total = 0;
    // parameter indices in state_dict order (weight; the bias follows)
    int enc(int i, int j) const { return 2 * (4 * i + j); }
    int enc_last() const { return 2 * (4 * n); }
    int mu() const { return 2 * (4 * n + 1); }
    int var() const { return 2 * (4 * n + 2); }
    int in_dec() const { return 2 * (4 * n + 3); }
    int dec0() const { return 2 * (4 * n + 4); }
    int dec(int i, int j) const { return 2 * (4 * n + 5 + 4 * i + j); }
    int out() const { return 2 * (8 * n + 5); }
};

int stages_of(int S, int f) {
    if (f < 1 || S < 2 * f || S % f) return -1;
    const int r = S / f;
    if (r & (r - 1)) return -1;
    int n = 0;
    while ((1 << n) < r) ++n;
    return n;
}

int check_vae(int B, int S, int C, int f, int L) {
    const int n = stages_of(S, f);
    OCRL_REQUIRE(n >= 1 && n <= OCRL_VAE_MAX_STAGES, "vae: obs_size / cnn_feat_size must be a power of two 2 .. 2^%d (got %d / %d)",
                 OCRL_VAE_MAX_STAGES, S, f);
    OCRL_REQUIRE(B >= 1, "vae: batch >= 1 (got %d)", B);
    OCRL_REQUIRE(C >= 1 && C <= 4, "vae: obs_channels must be 1 .. 4 (got %d)", C);
    OCRL_REQUIRE(L >= 4 && L % 4 == 0, "vae: latent_dim must be a positive multiple of 4 (got %d)", L);
    OCRL_REQUIRE((long long)B * S * S * 64 < (1LL << 31), "vae: batch %d of %d x %d images exceeds the int32 range of one call", B, S, S);
    return 0;
}

NcMap nhwc(long long s, int c) { NcMap m; m.sN = s * s * c; m.sG = 0; m.sC = 1; m.sH = s * c; m.sW = c; return m; }
NcMap nchw(long long s, int c) { NcMap m; m.sN = (long long)c * s * s; m.sG = 0; m.sC = s * s; m.sH = s; m.sW = 1; return m; }
size_t part_floats(const ConvLayer& c) { return (size_t)c.slab.slabs * c.cout * (c.K() + 1); }

VaeLay vae_layout(int B, int S, int C, int f, int L, int cnn, int full) {
    VaeLay y;
    WsTake take;
    y.n = stages_of(S, f); y.f = f; y.S = S; y.C = C; y.L = L; y.B = B; y.full = full; y.cnn = cnn;
    const size_t F = (size_t)64 * f * f;
    size_t gmax = (size_t)B * F;
    for (int i = 0; i < y.n; ++i) {
        const long long s = S >> (i + 1), M = (long long)B * s * s;
        for (int j = 0; j < 4; ++j) y.ea[i][j] = take((size_t)M * 64);
        y.ec[i] = conv_layer(B, i ? 64 : C, 64, 2, 2, 0, 2 * (int)s, 2 * (int)s);
        y.ec[i].x = i ? nhwc(2 * s, 64) : nchw(2 * s, C); y.ec[i].y = nhwc(s, 64);
        y.epart[i] = take(part_floats(y.ec[i]));
        if ((size_t)M * 64 > gmax) gmax = (size_t)M * 64;
    }
    y.e = take((size_t)B * F);
    y.ge = take((size_t)B * F);
    y.ml = take((size_t)B * 2 * L);
    y.Wml = take((size_t)2 * L * F);
    y.sk_floats = SK_FLOATS;
    if (full) {
        y.bml = take(2 * L); y.lat = take((size_t)B * L); y.klp = take(B); y.msews = take(1024);
        y.Win = take((size_t)F * L); y.bin = take(F); y.Wo4 = take(4 * 64); y.bo4 = take(4);
        y.hin = take((size_t)B * F); y.d0 = take((size_t)B * F);
        for (int i = 0; i < y.n; ++i) {
            const long long s = (long long)f << i, M = (long long)B * s * s;
            y.x3[i] = take(M * 64); y.y1[i] = take(M * 64); y.y2[i] = take(M * 64); y.y4[i] = take(M * 256); y.ps[i] = take(M * 256);
            if (s < CONV_HIP_MIN) {
                y.dc[i] = conv_layer(B, 64, 64, 3, 1, 1, (int)s, (int)s);
                y.dc[i].x = y.dc[i].y = nhwc(s, 64);
                y.dpart[i] = take(part_floats(y.dc[i]));
            } else {
                y.pkf[i] = take(9 * 64 * 64); y.pkb[i] = take(9 * 64 * 64);
                const size_t wg = conv_wgrad_ws_floats(B, (int)s, (int)s, 3, 64, false);        // db comes from the unit's own column sums
                if (wg > y.sk_floats) y.sk_floats = wg;
            }
            if ((size_t)M * 256 > gmax) gmax = (size_t)M * 256;
        }
        y.r4 = take((size_t)B * S * S * 4); y.dr4 = take((size_t)B * S * S * 4); y.drs = take((size_t)B * S * S * 4);
        y.dml = take((size_t)B * 2 * L); y.dlat = take((size_t)B * L);
        y.dWin = take((size_t)F * L); y.dbin = take(F); y.dWo4 = take(4 * 64); y.dbo4 = take(4);
    }
    y.dWml = take((size_t)2 * L * F); y.dbml = take(2 * L);
    y.gA = take(gmax); y.gB = take(gmax);
    y.sk = take(y.sk_floats);
    y.total = take.end;
    return y;
}

// backward of an implicit-GEMM conv layer (wb / dwb: its weight, the bias follows): dW, db through the slab partials and one reduce and,
// when dx, the gradient masked by x > 0
int nc_bwd(const ConvLayer& c, const float* x, const float* dy, float* dx, const float* const* wb, float* const* dwb, float* part, int B,
           hipStream_t st) {
    RC(conv_bwd(c, x, dy, dx, part, wb, 0, B, 1, st));
    NcReduceArgs r;
    conv_reduce_add(r, 0, c, part, dwb, 0, 1);
    return nc_dw_reduce_launch(r, st);
}

// a 1 x 1 Conv2dBlock / Linear layer's backward: dW, db; then dx = dy W (masked by `mask` > 0, + resid) when dx
int lin_bwd(const float* dy, const float* x, const float* W, float* dW, float* db, float* dx, long long M, int N_out, int K_in, const float* mask,
            const float* resid, const VaeLay& y, float* ws, hipStream_t st) {
    RC(lin_bwd_w(dy, N_out, x, K_in, dW, db, M, N_out, K_in, 1.f, ws + y.sk, y.sk_floats, st));
    if (dx) RC(lin_bwd_x(dy, N_out, W, dx, K_in, M, N_out, K_in, mask, K_in, resid, K_in, st));
    return 0;
}

// the gradients of _in_dec and the decoder when no loss cotangent reaches the backward (dw is overwritten, never accumulated)
int zero_decoder_grads(float* const* dw, const VaeLay& y, hipStream_t st) {
    const long long F = 64LL * y.f * y.f;
    RC(fill_launch(dw[y.in_dec()], F * y.L, 0.f, st));
    RC(fill_launch(dw[y.in_dec() + 1], F, 0.f, st));
    RC(fill_launch(dw[y.dec0()], 64 * 64, 0.f, st));
    RC(fill_launch(dw[y.dec0() + 1], 64, 0.f, st));
    static const int wn[4] = {64 * 64 * 9, 64 * 64, 64 * 64, 256 * 64}, bn[4] = {64, 64, 64, 256};
    for (int i = 0; i < y.n; ++i)
        for (int j = 0; j < 4; ++j) {
            RC(fill_launch(dw[y.dec(i, j)], wn[j], 0.f, st));
            RC(fill_launch(dw[y.dec(i, j) + 1], bn[j], 0.f, st));
        }
    RC(fill_launch(dw[y.out()], (long long)y.C * 64, 0.f, st));
    return fill_launch(dw[y.out() + 1], y.C, 0.f, st);
}

// encoder forward: every activation into ws; the last map into `emap` (ws or the caller's token output)
int enc_fwd(const float* obs, const float* const* w, float* emap, const VaeLay& y, float* ws, hipStream_t st) {
    const int B = y.B;
    for (int i = 0; i < y.n; ++i) {
        const int s = y.S >> (i + 1);
        const long long M = (long long)B * s * s;
        const float* x = i ? ws + y.ea[i - 1][3] : obs;
        RC(conv_fwd(y.ec[i], x, ws + y.ea[i][0], nullptr, w + y.enc(i, 0), 0, B, 1, st));
        for (int j = 1; j < 4; ++j)
            RC(lin_fwd(ws + y.ea[i][j - 1], 64, w[y.enc(i, j)], w[y.enc(i, j) + 1], ws + y.ea[i][j], 64, M, 64, 64, 1, nullptr, 0, st));
    }
    return lin_fwd(ws + y.ea[y.n - 1][3], 64, w[y.enc_last()], w[y.enc_last() + 1], emap, 64, (long long)B * y.f * y.f, 64, 64, 0, nullptr, 0, st);
}

// encoder backward from ge = d (encoder map) [B f f, 64]; ga / gb are scratch maps
int enc_bwd(const float* obs, const float* const* w, float* const* dw, const float* ge, const VaeLay& y, float* ws, hipStream_t st) {
    const int B = y.B;
    float* ga = ws + y.gA;
    float* gb = ws + y.gB;
    const float* last = ws + y.ea[y.n - 1][3];
    RC(lin_bwd(ge, last, w[y.enc_last()], dw[y.enc_last()], dw[y.enc_last() + 1], gb, (long long)B * y.f * y.f, 64, 64, last, nullptr, y, ws, st));
    for (int i = y.n - 1; i >= 0; --i) {
        const int s = y.S >> (i + 1);
        const long long M = (long long)B * s * s;
        for (int j = 3; j >= 1; --j) {                 // gb = d pre-activation of block j
            const float* x = ws + y.ea[i][j - 1];
            RC(lin_bwd(gb, x, w[y.enc(i, j)], dw[y.enc(i, j)], dw[y.enc(i, j) + 1], ga, M, 64, 64, x, nullptr, y, ws, st));
            std::swap(ga, gb);
        }
        const float* x = i ? ws + y.ea[i - 1][3] : obs;
        RC(nc_bwd(y.ec[i], x, gb, i ? ga : nullptr, w + y.enc(i, 0), dw + y.enc(i, 0), ws + y.epart[i], B, st));
        std::swap(ga, gb);
    }
    return 0;
}
}  // namespace

extern "C" {

size_t ocrl_vae_ws_floats(int B, int obs_size, int obs_channels, int cnn_feat_size, int latent_dim, int use_cnn_feat, int full) {
    if (check_vae(B, obs_size, obs_channels, cnn_feat_size, latent_dim)) return 0;   // the shapes fwd / bwd reject get no workspace
    return vae_layout(B, obs_size, obs_channels, cnn_feat_size, latent_dim, use_cnn_feat, full).total;
}

int ocrl_vae_fwd(const float* obs, const float* const* w, const float* eps, float* rep, float* metrics, float* recon, int B, int obs_size,
                 int obs_channels, int cnn_feat_size, int latent_dim, int use_cnn_feat, float kld_weight, int full, float* ws, size_t ws_floats,
                 void* stream) {
    OCRL_REQUIRE(obs && w && rep && ws && (!full || (eps && metrics)), "ocrl_vae_fwd: null argument");
    RC(check_vae(B, obs_size, obs_channels, cnn_feat_size, latent_dim));
    const VaeLay y = vae_layout(B, obs_size, obs_channels, cnn_feat_size, latent_dim, use_cnn_feat, full);
    RC(ws_check("ocrl_vae_fwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int L = y.L, f = y.f, HW = f * f, F = 64 * HW, S = y.S;
    RC(enc_fwd(obs, w, ws + y.e, y, ws, st));
    if (!full && use_cnn_feat) return copy_launch(ws + y.e, rep, (long long)B * F, st);
    // _mu (and _var) weights with their columns moved from the NCHW flatten (c, h, w) to the map's (h, w, c)
    RC(vae_permute_launch(w[y.mu()], ws + y.Wml, L, 64, HW, 0, 1, st));
    if (!full) {
        return lin_fwd(ws + y.e, F, ws + y.Wml, w[y.mu() + 1], rep, L, B, L, F, 0, nullptr, 0, st);
    }
    RC(vae_permute_launch(w[y.var()], ws + y.Wml + (size_t)L * F, L, 64, HW, 0, 1, st));
    RC(copy_launch(w[y.mu() + 1], ws + y.bml, L, st));
    RC(copy_launch(w[y.var() + 1], ws + y.bml + L, L, st));
    RC(lin_fwd(ws + y.e, F, ws + y.Wml, ws + y.bml, ws + y.ml, 2 * L, B, 2 * L, F, 0, nullptr, 0, st));          // [mu | logvar]
    RC(vae_kl_fwd_launch(ws + y.ml, eps, ws + y.lat, ws + y.klp, use_cnn_feat ? nullptr : rep, B, L, st));
    if (use_cnn_feat) RC(copy_launch(ws + y.e, rep, (long long)B * F, st));                                     // img_to_slot order
    // _in_dec with its rows (and bias) moved to the map's (h, w, c) order: its output is the NHWC decoder input
    RC(vae_permute_launch(w[y.in_dec()], ws + y.Win, L, 64, HW, 1, 1, st));
    RC(vae_permute_launch(w[y.in_dec() + 1], ws + y.bin, 1, 64, HW, 1, 1, st));
    RC(lin_fwd(ws + y.lat, L, ws + y.Win, ws + y.bin, ws + y.hin, F, B, F, L, 0, nullptr, 0, st));
    RC(lin_fwd(ws + y.hin, 64, w[y.dec0()], w[y.dec0() + 1], ws + y.d0, 64, (long long)B * HW, 64, 64, 1, nullptr, 0, st));
    const float* x = ws + y.d0;
    for (int i = 0; i < y.n; ++i) {
        const int s = f << i;
        const long long M = (long long)B * s * s;
        const int l3 = y.dec(i, 0);
        if (s < CONV_HIP_MIN) {
            RC(conv_fwd(y.dc[i], x, ws + y.x3[i], nullptr, w + l3, 0, B, 1, st));
        } else {
            RC(conv_pack_launch(w[l3], ws + y.pkf[i], ws + y.pkb[i], 3, 64, 64, 64, st));
            ConvArgs a;
            a.X = x; a.Wp = ws + y.pkf[i]; a.Y = ws + y.x3[i]; a.B = B; a.H = s; a.W = s; a.bias = w[l3 + 1]; a.relu = 1;
            RC(conv_fwd_launch(a, 3, 64, 64, st));
        }
        RC(lin_fwd(ws + y.x3[i], 64, w[y.dec(i, 1)], w[y.dec(i, 1) + 1], ws + y.y1[i], 64, M, 64, 64, 1, nullptr, 0, st));
        RC(lin_fwd(ws + y.y1[i], 64, w[y.dec(i, 2)], w[y.dec(i, 2) + 1], ws + y.y2[i], 64, M, 64, 64, 1, nullptr, 0, st));
        RC(lin_fwd(ws + y.y2[i], 64, w[y.dec(i, 3)], w[y.dec(i, 3) + 1], ws + y.y4[i], 256, M, 256, 64, 1, nullptr, 0, st));
        RC(pixel_shuffle_launch(ws + y.y4[i], ws + y.ps[i], B, s, s, 64, 1, nullptr, st));
        x = ws + y.ps[i];
    }
    // 64 -> C output conv as a 4-wide GEMM (zero rows past C) into the [B, S, S, 4] layout of mse_launch
    RC(vae_pad_rows_launch(w[y.out()], ws + y.Wo4, y.C, 4, 64, st));
    RC(vae_pad_rows_launch(w[y.out() + 1], ws + y.bo4, y.C, 4, 1, st));
    RC(lin_fwd(x, 64, ws + y.Wo4, ws + y.bo4, ws + y.r4, 4, (long long)B * S * S, 4, 64, 0, nullptr, 0, st));
    RC(mse_launch(obs, ws + y.r4, ws + y.dr4, metrics + 1, B, y.C, S, S, ws + y.msews, 1024, st));
    RC(vae_loss_launch(ws + y.klp, metrics, B, kld_weight, st));
    if (recon) RC(vae_recon_nchw_launch(ws + y.r4, recon, B, y.C, S * S, st));
    return 0;
}

int ocrl_vae_bwd(const float* obs, const float* eps, const float* const* w, const float* dloss, const float* drep, float* const* dw, int B,
                 int obs_size, int obs_channels, int cnn_feat_size, int latent_dim, int use_cnn_feat, float kld_weight, int full, float* ws,
                 size_t ws_floats, void* stream) {
    OCRL_REQUIRE(obs && w && dw && ws && (!full || eps) && (full || drep), "ocrl_vae_bwd: null argument");
    RC(check_vae(B, obs_size, obs_channels, cnn_feat_size, latent_dim));
    const VaeLay y = vae_layout(B, obs_size, obs_channels, cnn_feat_size, latent_dim, use_cnn_feat, full);
    RC(ws_check("ocrl_vae_bwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int L = y.L, f = y.f, HW = f * f, F = 64 * HW, S = y.S;
    if (!full) {
        const float* ge = drep;                        // use_cnn_feat: the tokens are the encoder map
        if (!use_cnn_feat) {
            RC(lin_bwd(drep, ws + y.e, ws + y.Wml, ws + y.dWml, dw[y.mu() + 1], ws + y.ge, B, L, F, nullptr, nullptr, y, ws, st));
            RC(vae_permute_launch(ws + y.dWml, dw[y.mu()], L, 64, HW, 0, 0, st));
            ge = ws + y.ge;
        }
        return enc_bwd(obs, w, dw, ge, y, ws, st);
    }
    // no loss cotangent counts as zero: the decoder and KL terms add nothing, and the decoder-side parameters get zero gradients
    if (dloss) {
        // reconstruction: d recon scaled by the loss cotangent; the 64 -> C conv through its 4-wide padded form
        const long long BSS = (long long)B * S * S;
        RC(vae_scale_launch(ws + y.dr4, ws + y.drs, dloss, BSS * 4, st));
        float* ga = ws + y.gA;
        float* gb = ws + y.gB;
        const float* xl = ws + y.ps[y.n - 1];
        RC(lin_bwd(ws + y.drs, xl, ws + y.Wo4, ws + y.dWo4, ws + y.dbo4, ga, BSS, 4, 64, xl, nullptr, y, ws, st));
        RC(copy_launch(ws + y.dWo4, dw[y.out()], (long long)y.C * 64, st));
        RC(copy_launch(ws + y.dbo4, dw[y.out() + 1], y.C, st));
        for (int i = y.n - 1; i >= 0; --i) {               // ga = d (shuffled output of stage i), masked
            const int s = f << i;
            const long long M = (long long)B * s * s;
            RC(pixel_shuffle_launch(ga, gb, B, s, s, 64, 0, nullptr, st));
            RC(lin_bwd(gb, ws + y.y2[i], w[y.dec(i, 3)], dw[y.dec(i, 3)], dw[y.dec(i, 3) + 1], ga, M, 256, 64, ws + y.y2[i], nullptr, y, ws, st));
            RC(lin_bwd(ga, ws + y.y1[i], w[y.dec(i, 2)], dw[y.dec(i, 2)], dw[y.dec(i, 2) + 1], gb, M, 64, 64, ws + y.y1[i], nullptr, y, ws, st));
            RC(lin_bwd(gb, ws + y.x3[i], w[y.dec(i, 1)], dw[y.dec(i, 1)], dw[y.dec(i, 1) + 1], ga, M, 64, 64, ws + y.x3[i], nullptr, y, ws, st));
            const float* x = i ? ws + y.ps[i - 1] : ws + y.d0;
            const int l3 = y.dec(i, 0);
            if (s < CONV_HIP_MIN) {
                RC(nc_bwd(y.dc[i], x, ga, gb, w + l3, dw + l3, ws + y.dpart[i], B, st));
            } else {
                WgradArgs wa;
                wa.X = x; wa.dY = ga; wa.part = ws + y.sk; wa.B = B; wa.H = s; wa.W = s;
                RC(conv_wgrad_launch(wa, 3, 64, 64, 64, dw[l3], nullptr, 0, st, 0));
                RC(colsum_launch(ga, 64, dw[l3 + 1], M, 64, 0, 1.f, ws + y.sk, y.sk_floats, st));
                ConvArgs a;                                // d x = conv(d y, flipped W) masked by x > 0
                a.X = ga; a.Wp = ws + y.pkb[i]; a.Y = gb; a.B = B; a.H = s; a.W = s; a.mask = x;
                RC(conv_fwd_launch(a, 3, 64, 64, st));
            }
            std::swap(ga, gb);
        }
        // ga = d d0 (masked); the decoder's input block, _in_dec, the reparameterisation and KL, _mu / _var
        RC(lin_bwd(ga, ws + y.hin, w[y.dec0()], dw[y.dec0()], dw[y.dec0() + 1], gb, (long long)B * HW, 64, 64, nullptr, nullptr, y, ws, st));
        RC(lin_bwd(gb, ws + y.lat, ws + y.Win, ws + y.dWin, ws + y.dbin, ws + y.dlat, B, F, L, nullptr, nullptr, y, ws, st));
        RC(vae_permute_launch(ws + y.dWin, dw[y.in_dec()], L, 64, HW, 1, 0, st));
        RC(vae_permute_launch(ws + y.dbin, dw[y.in_dec() + 1], 1, 64, HW, 1, 0, st));
    } else {
        RC(zero_decoder_grads(dw, y, st));
    }
    RC(vae_kl_bwd_launch(ws + y.ml, eps, dloss ? ws + y.dlat : nullptr, use_cnn_feat ? nullptr : drep, dloss, ws + y.dml, B, L, kld_weight, st));
    // d (encoder map) = [d mu | d logvar] [W_mu; W_var] (+ d rep: the tokens are the map itself)
    RC(lin_bwd(ws + y.dml, ws + y.e, ws + y.Wml, ws + y.dWml, ws + y.dbml, ws + y.ge, B, 2 * L, F, nullptr, use_cnn_feat ? drep : nullptr, y,
               ws, st));
    RC(vae_permute_launch(ws + y.dWml, dw[y.mu()], L, 64, HW, 0, 0, st));
    RC(vae_permute_launch(ws + y.dWml + (size_t)L * F, dw[y.var()], L, 64, HW, 0, 0, st));
    RC(copy_launch(ws + y.dbml, dw[y.mu() + 1], L, st));
    RC(copy_launch(ws + y.dbml + L, dw[y.var() + 1], L, st));
    return enc_bwd(obs, w, dw, ws + y.ge, y, ws, st);
}

}  // extern "C"
