// C ABI of the IODINE kernels and the broadcast decoder's own kernels, one launcher (sequence) per entry (include/ocrl_hip_iodine.h:
// ocrl_iodine_*, ocrl_bcdec_*).  Stateless: the caller owns every tensor and the scratch.  Each entry refuses, before any launch, what its
// launchers refuse and what would read or write out of bounds; the arithmetic is iodine.hip's and bcdec.hip's, untouched.
#include "../../include/ocrl_hip_iodine.h"
#include "common.h"
#include "kernels.h"

namespace {
constexpr size_t C4_WS_FLOATS = 2 * 9 * 64 * 4;        // Wk [9][64][4] then Wb [9][4][64]
constexpr size_t MIX_WS_FLOATS = 1024;                 // bc_mix's per-block loss partials
constexpr long long MAX_GRID = 0x7fffffffLL;           // blocks of a one-dimensional launch

// 1 <= K <= 16, S % 16 == 0 (a block of the ELBO kernels never straddles two images), a grid that fits
int check_elbo_shape(const char* who, int B, int K, int S) {
    OCRL_REQUIRE(B >= 1, "%s: B >= 1 (got %d)", who, B);
    OCRL_REQUIRE(K >= 1 && K <= 16, "%s: 1 <= K <= 16 (got %d)", who, K);
    OCRL_REQUIRE(S >= 16 && S <= 4096 && (S * S) % 256 == 0, "%s: S %% 16 == 0 in 16 .. 4096 (got %d)", who, S);
    OCRL_REQUIRE((long long)B * K * (S * S / 256) <= MAX_GRID, "%s: B * K * S * S / 256 blocks exceed a grid", who);
    return 0;
}
size_t elbo_ws_floats(int B, int K, int S) {
    const size_t nb = (size_t)S * S / 256, a = (size_t)B * nb * 66, b = (size_t)B * K * nb * 4;      // io_elbo's, io_enc_norm's
    return a > b ? a : b;
}
int check_window(const char* who, long long Bn, int C, int Hi, int Wi, int ldc) {
    OCRL_REQUIRE(Bn >= 1 && C >= 1 && Hi >= 1 && Wi >= 1, "%s: Bn, C, Hi, Wi >= 1 (got %lld, %d, %d, %d)", who, Bn, C, Hi, Wi);
    OCRL_REQUIRE(C <= 4096 && Hi <= 4096 && Wi <= 4096, "%s: C, Hi, Wi <= 4096 (got %d, %d, %d)", who, C, Hi, Wi);
    OCRL_REQUIRE(ldc >= 9 * C, "%s: ldc >= 9 C (got ldc %d, C %d)", who, ldc, C);
    OCRL_REQUIRE(Bn * Hi * Wi * (long long)(ldc > C ? ldc : C) / 256 < MAX_GRID, "%s: the element count exceeds a grid", who);
    return 0;
}
int check_c4_shape(const char* who, int Bn, int S) {
    OCRL_REQUIRE(Bn >= 1 && S >= 1 && S <= 4096, "%s: Bn >= 1 and 1 <= S <= 4096 (got %d, %d)", who, Bn, S);
    OCRL_REQUIRE((long long)cdiv(S, 32) * cdiv(S, 4) * Bn <= MAX_GRID, "%s: the tile count exceeds a grid", who);
    return 0;
}
}  // namespace

extern "C" {

size_t ocrl_iodine_elbo_ws_floats(int B, int K, int S) {
    if (check_elbo_shape("ocrl_iodine_elbo_ws_floats", B, K, S)) return 0;
    return elbo_ws_floats(B, K, S);
}

int ocrl_iodine_elbo(const float* out4, const float* obs, int B, int K, int S, float sigma, int layer_norm, float* enc, float* st1, float* st2,
                     float* dout4, float* part, float* masks, float* recon, float* recons_masked, float* ws, size_t ws_floats, void* stream) {
    RC(check_elbo_shape("ocrl_iodine_elbo", B, K, S));
    OCRL_REQUIRE(out4 && obs && part && ws, "ocrl_iodine_elbo: null argument (out4, obs, part or ws)");
    OCRL_REQUIRE(sigma > 0.f, "ocrl_iodine_elbo: sigma must be positive (got %g)", (double)sigma);
    OCRL_REQUIRE(!enc || st1, "ocrl_iodine_elbo: enc needs st1");
    OCRL_REQUIRE(!enc || !layer_norm || st2, "ocrl_iodine_elbo: enc with layer_norm needs st2");
    OCRL_REQUIRE(aligned16(out4, dout4), "ocrl_iodine_elbo: out4 and dout4 must be 16-byte aligned");
    OCRL_REQUIRE(ws_floats >= elbo_ws_floats(B, K, S), "ocrl_iodine_elbo: workspace too small (%zu < %zu floats)", ws_floats, elbo_ws_floats(B, K, S));
    hipStream_t st = static_cast<hipStream_t>(stream);
    RC(io_elbo_launch(out4, obs, B, K, S, sigma, enc, st1, dout4, part, masks, recon, recons_masked, ws, ws_floats, st));
    if (enc && layer_norm) RC(io_enc_norm_launch(enc, st1, st2, (long long)B * K, S * S, ws, ws_floats, st));
    return 0;
}

int ocrl_iodine_elbo_bwd(const float* out4, const float* obs, const float* denc, int B, int K, int S, float sigma, float cw, float* dout4,
                         void* stream) {
    RC(check_elbo_shape("ocrl_iodine_elbo_bwd", B, K, S));
    OCRL_REQUIRE(out4 && obs && dout4, "ocrl_iodine_elbo_bwd: null argument (out4, obs or dout4)");
    OCRL_REQUIRE(sigma > 0.f, "ocrl_iodine_elbo_bwd: sigma must be positive (got %g)", (double)sigma);
    OCRL_REQUIRE(aligned16(out4, dout4), "ocrl_iodine_elbo_bwd: out4 and dout4 must be 16-byte aligned");
    return io_elbo_bwd_launch(out4, obs, denc, B, K, S, sigma, cw, dout4, static_cast<hipStream_t>(stream));
}

size_t ocrl_iodine_sample_ws_floats(long long n) { return n >= 1 ? (size_t)n : 0; }

int ocrl_iodine_sample(const float* mu, const float* ls, const float* noise, float* eps_out, float* slots, float* kl_out, long long n,
                       unsigned long long seed, unsigned site, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(mu && ls && eps_out && slots && kl_out && ws, "ocrl_iodine_sample: null argument (mu, ls, eps_out, slots, kl_out or ws)");
    OCRL_REQUIRE(n >= 1 && n / 256 < MAX_GRID, "ocrl_iodine_sample: 1 <= n < 2^39 (got %lld)", n);
    OCRL_REQUIRE(ws_floats >= (size_t)n, "ocrl_iodine_sample: workspace too small (%zu < %lld floats)", ws_floats, n);
    return io_sample_launch(mu, ls, noise, eps_out, slots, kl_out, n, seed, site, ws, ws_floats, static_cast<hipStream_t>(stream));
}

int ocrl_iodine_latent(const float* mu, const float* ls, const float* eps, const float* ds, float* latent, long long BK, int L, float beta,
                       int layer_norm, int ld, void* stream) {
    OCRL_REQUIRE(mu && ls && eps && ds && latent, "ocrl_iodine_latent: null argument");
    OCRL_REQUIRE(BK >= 1 && BK / 4 < MAX_GRID, "ocrl_iodine_latent: 1 <= BK < 2^33 (got %lld)", BK);
    OCRL_REQUIRE(L >= 2 && L <= 65536, "ocrl_iodine_latent: 2 <= L <= 65536, the unbiased variance divides by L - 1 (got %d)", L);
    OCRL_REQUIRE(ld >= 4 * L, "ocrl_iodine_latent: ld >= 4 L (got ld %d, L %d)", ld, L);
    return io_latent_launch(mu, ls, eps, ds, latent, BK, L, beta, layer_norm, ld, static_cast<hipStream_t>(stream));
}

int ocrl_iodine_post_grad(const float* mu, const float* ls, const float* eps, const float* ds, const float* dlat, int ldl, float kw, float* gmu,
                          float* gls, long long BK, int L, void* stream) {
    OCRL_REQUIRE(mu && ls && eps && ds && gmu && gls, "ocrl_iodine_post_grad: null argument");
    OCRL_REQUIRE(BK >= 1 && L >= 1 && L <= 65536 && BK * L / 256 < MAX_GRID, "ocrl_iodine_post_grad: BK >= 1, 1 <= L <= 65536 (got %lld, %d)", BK, L);
    OCRL_REQUIRE(!dlat || ldl >= 2 * L, "ocrl_iodine_post_grad: ldl >= 2 L (got ldl %d, L %d)", ldl, L);
    return io_post_grad_launch(mu, ls, eps, ds, dlat, ldl, kw, gmu, gls, BK, L, static_cast<hipStream_t>(stream));
}

int ocrl_iodine_im2col(const float* x, float* col, long long Bn, int C, int Hi, int Wi, int ldc, int force_generic, void* stream) {
    RC(check_window("ocrl_iodine_im2col", Bn, C, Hi, Wi, ldc));
    OCRL_REQUIRE(x && col, "ocrl_iodine_im2col: null argument");
    return io_im2col_launch(x, col, Bn, C, Hi, Wi, ldc, static_cast<hipStream_t>(stream), force_generic ? 1 : 0);
}

int ocrl_iodine_col2im(const float* dcol, const float* act, float* dx, long long Bn, int C, int Hi, int Wi, int ldc, int force_generic,
                       void* stream) {
    RC(check_window("ocrl_iodine_col2im", Bn, C, Hi, Wi, ldc));
    OCRL_REQUIRE(dcol && dx, "ocrl_iodine_col2im: null argument");
    return io_col2im_launch(dcol, act, dx, Bn, C, Hi, Wi, ldc, static_cast<hipStream_t>(stream), force_generic ? 1 : 0);
}

int ocrl_iodine_refw_pack(const float* src, float* dst, int C, int ldc, int backward, void* stream) {
    OCRL_REQUIRE(src && dst, "ocrl_iodine_refw_pack: null argument");
    OCRL_REQUIRE(C >= 1 && C <= 4096 && ldc >= 9 * C && ldc <= (1 << 20), "ocrl_iodine_refw_pack: 1 <= C <= 4096 and 9 C <= ldc <= 2^20 (got C %d, ldc %d)", C, ldc);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return backward ? io_refw_unpack_launch(src, dst, C, ldc, st) : io_refw_pack_launch(src, dst, C, ldc, st);
}

int ocrl_iodine_pool(const float* r, const float* dpool, float* out, long long BK, int n, void* stream) {
    OCRL_REQUIRE(r && out, "ocrl_iodine_pool: null argument");
    OCRL_REQUIRE(BK >= 1 && n >= 1 && BK <= MAX_GRID && BK * n / 4 < MAX_GRID, "ocrl_iodine_pool: BK >= 1 and n >= 1 (got %lld, %d)", BK, n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dpool ? io_pool_bwd_launch(dpool, r, out, BK, n, st) : io_pool_launch(r, out, BK, n, st);
}

int ocrl_iodine_elu2(const float* a, int lda, float* y, int ldy, long long rows, int F, const float* dy, int lddy, void* stream) {
    OCRL_REQUIRE(a && y, "ocrl_iodine_elu2: null argument");
    OCRL_REQUIRE(rows >= 1 && F >= 1 && rows * F / 256 < MAX_GRID, "ocrl_iodine_elu2: rows >= 1 and F >= 1 (got %lld, %d)", rows, F);
    OCRL_REQUIRE(lda >= F && ldy >= F && (!dy || lddy >= F), "ocrl_iodine_elu2: every row stride must be >= F (got lda %d, ldy %d, lddy %d, F %d)", lda,
                 ldy, lddy, F);
    return io_elu2_launch(a, lda, y, ldy, rows, F, dy, lddy, static_cast<hipStream_t>(stream));
}

int ocrl_iodine_lstm(const float* gates, const float* c0, float* acts, float* c1, float* h1, const float* dh1, const float* dc1, float* dgates,
                     float* dc0, long long rows, int H, int backward, void* stream) {
    OCRL_REQUIRE(rows >= 1 && H >= 1 && H <= 65536 && rows * H / 256 < MAX_GRID, "ocrl_iodine_lstm: rows >= 1 and 1 <= H <= 65536 (got %lld, %d)", rows, H);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!backward) {
        OCRL_REQUIRE(gates && c0 && acts && c1 && h1, "ocrl_iodine_lstm: null argument (gates, c0, acts, c1 or h1)");
        return io_lstm_fwd_launch(gates, c0, acts, c1, h1, rows, H, st);
    }
    OCRL_REQUIRE(acts && c0 && c1 && dgates && dc0, "ocrl_iodine_lstm: null argument (acts, c0, c1, dgates or dc0)");
    return io_lstm_bwd_launch(acts, c0, c1, dh1, dc1, dgates, dc0, rows, H, st);
}

size_t ocrl_bcdec_c4_ws_floats(void) { return C4_WS_FLOATS; }

int ocrl_bcdec_c4(const float* W, int co_n, const float* bias, const float* X, const float* act, float* Y, int Bn, int S, int mode, int elu,
                  float* ws, size_t ws_floats, void* stream) {
    RC(check_c4_shape("ocrl_bcdec_c4", Bn, S));
    OCRL_REQUIRE(mode == 0 || mode == 1, "ocrl_bcdec_c4: mode 0 (forward) or 1 (backward data) (got %d)", mode);
    OCRL_REQUIRE(co_n >= 1 && co_n <= 4, "ocrl_bcdec_c4: 1 <= co_n <= 4 (got %d)", co_n);
    OCRL_REQUIRE(W && X && Y && ws && (mode ? act != nullptr : bias != nullptr), "ocrl_bcdec_c4: null argument (W, X, Y, ws, or %s)", mode ? "act" : "bias");
    OCRL_REQUIRE(ws_floats >= C4_WS_FLOATS, "ocrl_bcdec_c4: workspace too small (%zu < %zu floats)", ws_floats, C4_WS_FLOATS);
    OCRL_REQUIRE(aligned16(X, Y, act, ws), "ocrl_bcdec_c4: X, Y, act and ws must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* Wk = ws;
    float* Wb = ws + 9 * 64 * 4;
    RC(bc_c4_pack_launch(W, Wk, Wb, co_n, st));
    if (mode == 0) return bc_c4_fwd_launch(X, Wk, bias, Y, Bn, S, st);
    return bc_c4_bwd_data_launch(X, Wb, act, Y, Bn, S, st, elu ? 1 : 0);
}

int ocrl_bcdec_c4_wgrad_blocks(int Bn, int S) {
    if (check_c4_shape("ocrl_bcdec_c4_wgrad_blocks", Bn, S)) return 0;
    return bc_c4_wgrad_blocks(Bn, S);
}

int ocrl_bcdec_c4_wgrad(const float* X, const float* dY, float* part, size_t part_floats, int Bn, int S, int form, void* stream) {
    RC(check_c4_shape("ocrl_bcdec_c4_wgrad", Bn, S));
    OCRL_REQUIRE(form >= 0 && form <= 2, "ocrl_bcdec_c4_wgrad: form 0 (the switch), 1 (VALU) or 2 (MFMA) (got %d)", form);
    OCRL_REQUIRE(X && dY && part, "ocrl_bcdec_c4_wgrad: null argument");
    OCRL_REQUIRE(aligned16(X, dY), "ocrl_bcdec_c4_wgrad: X and dY must be 16-byte aligned");
    const size_t need = (size_t)bc_c4_wgrad_blocks(Bn, S) * 4 * 64 * 9;
    OCRL_REQUIRE(part_floats >= need, "ocrl_bcdec_c4_wgrad: part too small (%zu < %zu floats)", part_floats, need);
    return bc_c4_wgrad_launch(X, dY, part, Bn, S, static_cast<hipStream_t>(stream), form);
}

size_t ocrl_bcdec_mix_ws_floats(void) { return MIX_WS_FLOATS; }

int ocrl_bcdec_mix(const float* out4, const float* obs, float* recon, float* dout4, float* loss_out, int B, int K, int S, int C, float* ws,
                   size_t ws_floats, void* stream) {
    OCRL_REQUIRE(out4 && obs && loss_out && ws, "ocrl_bcdec_mix: null argument (out4, obs, loss_out or ws)");
    OCRL_REQUIRE(B >= 1 && S >= 1 && S <= 4096, "ocrl_bcdec_mix: B >= 1 and 1 <= S <= 4096 (got %d, %d)", B, S);
    OCRL_REQUIRE(K >= 1 && K <= 16 && C >= 1 && C <= 3, "ocrl_bcdec_mix: 1 <= K <= 16 and 1 <= C <= 3 (got %d, %d)", K, C);
    OCRL_REQUIRE(ws_floats >= MIX_WS_FLOATS, "ocrl_bcdec_mix: workspace too small (%zu < %zu floats)", ws_floats, MIX_WS_FLOATS);
    OCRL_REQUIRE(aligned16(out4, recon, dout4), "ocrl_bcdec_mix: out4, recon and dout4 must be 16-byte aligned");
    return bc_mix_launch(out4, obs, recon, dout4, loss_out, B, K, S, C, ws, ws_floats, static_cast<hipStream_t>(stream));
}

int ocrl_bcdec_compose(const float* W1, const float* Wpos, const float* bpos, float* Wc, float* W1r, int D, void* stream) {
    OCRL_REQUIRE(W1 && Wpos && bpos && Wc && W1r, "ocrl_bcdec_compose: null argument");
    OCRL_REQUIRE(D >= 1 && D <= 65536, "ocrl_bcdec_compose: 1 <= D <= 65536 (got %d)", D);
    return bc_compose_launch(W1, Wpos, bpos, Wc, W1r, D, static_cast<hipStream_t>(stream));
}

int ocrl_bcdec_compose_bwd(const float* W1, const float* Wpos, const float* bpos, const float* dWc, const float* dW1r, float* dW1, float* dWpos,
                           float* dbpos, int D, void* stream) {
    OCRL_REQUIRE(W1 && Wpos && bpos && dWc && dW1r && dW1 && dWpos && dbpos, "ocrl_bcdec_compose_bwd: null argument");
    OCRL_REQUIRE(D >= 1 && D <= 65536, "ocrl_bcdec_compose_bwd: 1 <= D <= 65536 (got %d)", D);
    return bc_compose_bwd_launch(W1, Wpos, bpos, dWc, dW1r, dW1, dWpos, dbpos, D, static_cast<hipStream_t>(stream));
}

}  // extern "C"
