// C ABI of the SLATE token-path and helper kernels, one launcher of elementwise.hip per entry (include/ocrl_hip_slate_kernels.h:
// ocrl_tp_*).  Stateless: the caller owns every tensor and the scratch.  Most of these launchers check little themselves (the model that
// calls them has already fixed the shapes), so each entry refuses, before any launch, what the kernel behind it cannot handle: null
// pointers, sizes below 1, misaligned float4 operands and every shape limit the kernel assumes.  The arithmetic is elementwise.hip's,
// untouched.
#include "../../include/ocrl_hip_slate_kernels.h"
#include "common.h"
#include "kernels.h"

namespace {
constexpr long long MAX_ELEMS = 0x7fffffffLL;          // elements of a one-thread-per-element launch (int indices inside some kernels)
constexpr int MAX_VOCAB_ROWS = 256 * 16;               // gumbel_softmax / softmax_bwd_rows: 16 values per thread of a 256-thread workgroup

int check_vocab(const char* who, long long R, int V) {
    OCRL_REQUIRE(R >= 1 && R <= MAX_ELEMS, "%s: 1 <= R < 2^31 (got %lld)", who, R);
    OCRL_REQUIRE(V >= 256 && V % 256 == 0 && V <= MAX_VOCAB_ROWS, "%s: V %% 256 == 0 in 256 .. %d (got %d)", who, MAX_VOCAB_ROWS, V);
    return 0;
}
int check_prob(const char* who, float p) {
    OCRL_REQUIRE(p >= 0.f && p < 1.f, "%s: 0 <= p < 1 (got %g)", who, (double)p);
    return 0;
}
int check_embed(const char* who, int B, int T, int d) {
    OCRL_REQUIRE(B >= 1 && T >= 1 && d >= 1, "%s: B, T, d >= 1 (got %d, %d, %d)", who, B, T, d);
    OCRL_REQUIRE((long long)B * T * d <= MAX_ELEMS, "%s: B * T * d < 2^31", who);
    return 0;
}
int check_embed_bwd_shape(const char* who, long long BT, int V, int d) {
    OCRL_REQUIRE(BT >= 1 && BT <= MAX_ELEMS, "%s: 1 <= B * T < 2^31 (got %lld)", who, BT);
    OCRL_REQUIRE(d >= 4 && d % 4 == 0 && d <= 1024, "%s: d %% 4 == 0 in 4 .. 1024 (got %d)", who, d);
    OCRL_REQUIRE(V >= 1 && V + 1 <= 16384, "%s: 1 <= V and V + 1 <= 16384 (got %d)", who, V);
    OCRL_REQUIRE(BT * d <= MAX_ELEMS, "%s: B * T * d < 2^31", who);
    return 0;
}
}  // namespace

extern "C" {

int ocrl_tp_gumbel_softmax(const float* raw, const float* e1, const float* e2, float* z, int* tokens, float* zst, long long R, int V, float tau,
                           unsigned long long seed, void* stream) {
    RC(check_vocab("ocrl_tp_gumbel_softmax", R, V));
    OCRL_REQUIRE(raw && z && tokens, "ocrl_tp_gumbel_softmax: null argument (raw, z or tokens)");
    OCRL_REQUIRE((e1 == nullptr) == (e2 == nullptr), "ocrl_tp_gumbel_softmax: give both noise tensors or none");
    OCRL_REQUIRE(tau > 0.f, "ocrl_tp_gumbel_softmax: tau must be positive (got %g)", (double)tau);
    return gumbel_softmax_launch(raw, e1, e2, z, tokens, R, V, tau, seed, static_cast<hipStream_t>(stream), zst);
}

int ocrl_tp_softmax_bwd_rows(const float* z, float* d, long long R, int V, float scale, void* stream) {
    RC(check_vocab("ocrl_tp_softmax_bwd_rows", R, V));
    OCRL_REQUIRE(z && d, "ocrl_tp_softmax_bwd_rows: null argument");
    return softmax_bwd_rows_launch(z, d, R, V, scale, static_cast<hipStream_t>(stream));
}

int ocrl_tp_softmax_stat_combine(const float* stat, int nseg, long long R, float* lse, const float* hstat, const int* hidx, int* tokens,
                                 const float* pred, int ldp, int V, const int* tok, float* out, float scale, float* ws, size_t ws_floats,
                                 void* stream) {
    OCRL_REQUIRE(stat && lse, "ocrl_tp_softmax_stat_combine: null argument (stat or lse)");
    OCRL_REQUIRE(nseg >= 1 && nseg <= 64, "ocrl_tp_softmax_stat_combine: 1 <= nseg <= 64 (got %d)", nseg);
    OCRL_REQUIRE(R >= 1 && R <= MAX_ELEMS, "ocrl_tp_softmax_stat_combine: 1 <= R < 2^31 (got %lld)", R);
    OCRL_REQUIRE((hstat == nullptr) == (hidx == nullptr) && (!hstat || tokens), "ocrl_tp_softmax_stat_combine: the hard sample needs hstat, hidx and tokens");
    if (pred) {
        OCRL_REQUIRE(tok && out && ws, "ocrl_tp_softmax_stat_combine: the cross-entropy needs pred, tok, out and ws");
        OCRL_REQUIRE(V >= 1 && ldp >= V, "ocrl_tp_softmax_stat_combine: ldp >= V >= 1, V = the widest token index + 1 (got ldp %d, V %d)", ldp, V);
        const size_t need = (size_t)((R + 15) / 16);
        OCRL_REQUIRE(ws_floats >= need, "ocrl_tp_softmax_stat_combine: workspace too small (%zu < %zu floats)", ws_floats, need);
    }
    return softmax_stat_combine_launch(stat, nseg, R, lse, hstat, hidx, tokens, pred, ldp, tok, out, scale, ws, ws_floats,
                                       static_cast<hipStream_t>(stream));
}

int ocrl_tp_exp_rows(const float* y, const float* lse, float* z, long long R, int V, void* stream) {
    OCRL_REQUIRE(y && lse && z, "ocrl_tp_exp_rows: null argument");
    OCRL_REQUIRE(R >= 1 && V >= 4 && V % 4 == 0 && R * V <= MAX_ELEMS, "ocrl_tp_exp_rows: R >= 1 and V %% 4 == 0, V >= 4 (got %lld, %d)", R, V);
    OCRL_REQUIRE(aligned16(y, z), "ocrl_tp_exp_rows: y and z must be 16-byte aligned");
    return exp_rows_launch(y, lse, z, R, V, static_cast<hipStream_t>(stream));
}

int ocrl_tp_rowdot_bias64(const float* g, const float* act, const float* bias, long long R, float* out, void* stream) {
    OCRL_REQUIRE(g && act && bias && out, "ocrl_tp_rowdot_bias64: null argument");
    OCRL_REQUIRE(R >= 1 && R <= MAX_ELEMS, "ocrl_tp_rowdot_bias64: 1 <= R < 2^31 (got %lld)", R);
    OCRL_REQUIRE(aligned16(g, act, bias), "ocrl_tp_rowdot_bias64: g, act and bias must be 16-byte aligned");
    return rowdot_bias64_launch(g, act, bias, R, out, static_cast<hipStream_t>(stream));
}

int ocrl_tp_embed_fwd(const int* tokens, const float* dict, const float* bos, const float* pe, float* out, int B, int T, int d, float p,
                      unsigned long long seed, void* stream) {
    RC(check_embed("ocrl_tp_embed_fwd", B, T, d));
    OCRL_REQUIRE(tokens && dict && bos && pe && out, "ocrl_tp_embed_fwd: null argument");
    OCRL_REQUIRE(d % 4 == 0, "ocrl_tp_embed_fwd: d %% 4 == 0 (got %d)", d);
    RC(check_prob("ocrl_tp_embed_fwd", p));
    OCRL_REQUIRE(aligned16(dict, bos, pe, out), "ocrl_tp_embed_fwd: dict, bos, pe and out must be 16-byte aligned");
    return embed_fwd_launch(tokens, dict, bos, pe, out, B, T, d, p, seed, static_cast<hipStream_t>(stream));
}

size_t ocrl_tp_embed_bwd_ws_floats(long long BT, int V, int d) {
    if (check_embed_bwd_shape("ocrl_tp_embed_bwd_ws_floats", BT, V, d)) return 0;
    return embed_bwd_ws_floats(BT, V, d);
}

int ocrl_tp_embed_bwd(float* g, const int* tokens, float* ddict, int B, int T, int V, int d, float p, unsigned long long seed, float* ws,
                      size_t ws_floats, void* stream) {
    OCRL_REQUIRE(B >= 1 && T >= 1, "ocrl_tp_embed_bwd: B, T >= 1 (got %d, %d)", B, T);
    RC(check_embed_bwd_shape("ocrl_tp_embed_bwd", (long long)B * T, V, d));
    OCRL_REQUIRE(g && tokens && ddict && ws, "ocrl_tp_embed_bwd: null argument");
    RC(check_prob("ocrl_tp_embed_bwd", p));
    OCRL_REQUIRE(aligned16(g, ws), "ocrl_tp_embed_bwd: g and ws must be 16-byte aligned");
    const size_t need = embed_bwd_ws_floats((long long)B * T, V, d);
    OCRL_REQUIRE(ws_floats >= need, "ocrl_tp_embed_bwd: workspace too small (%zu < %zu floats)", ws_floats, need);
    return embed_bwd_launch(g, tokens, ddict, B, T, V, d, p, seed, ws, ws_floats, static_cast<hipStream_t>(stream));
}

int ocrl_tp_embed_step(const int* tokens, const float* dict, const float* bos, const float* pe, float* out, int B, int T, int d, int t,
                       void* stream) {
    RC(check_embed("ocrl_tp_embed_step", B, T, d));
    OCRL_REQUIRE(tokens && dict && bos && pe && out, "ocrl_tp_embed_step: null argument");
    OCRL_REQUIRE(t >= 0 && t < T, "ocrl_tp_embed_step: 0 <= t < T (got t %d, T %d)", t, T);
    return embed_step_launch(tokens, dict, bos, pe, out, B, T, d, t, static_cast<hipStream_t>(stream));
}

int ocrl_tp_dropout_apply(const float* x, float* y, long long n, float p, unsigned long long seed, unsigned site, void* stream) {
    OCRL_REQUIRE(x && y, "ocrl_tp_dropout_apply: null argument");
    OCRL_REQUIRE(n >= 4 && n % 4 == 0 && n <= MAX_ELEMS, "ocrl_tp_dropout_apply: n %% 4 == 0 in 4 .. 2^31 (got %lld)", n);
    RC(check_prob("ocrl_tp_dropout_apply", p));
    OCRL_REQUIRE(aligned16(x, y), "ocrl_tp_dropout_apply: x and y must be 16-byte aligned");
    return dropout_apply_launch(x, y, n, p, seed, site, static_cast<hipStream_t>(stream));
}

int ocrl_tp_dropout_mask(float* y, unsigned site, long long n, float p, unsigned long long seed, void* stream) {
    OCRL_REQUIRE(y, "ocrl_tp_dropout_mask: null argument");
    OCRL_REQUIRE(n >= 1 && n <= MAX_ELEMS, "ocrl_tp_dropout_mask: 1 <= n < 2^31 (got %lld)", n);
    RC(check_prob("ocrl_tp_dropout_mask", p));
    return dropout_mask_launch(y, n, p, seed, site, static_cast<hipStream_t>(stream));
}

int ocrl_tp_colsum(const float* X, long long ld, float* out, long long R, int F, int accumulate, float scale, float* ws, size_t ws_floats,
                   void* stream) {
    OCRL_REQUIRE(X && out && ws, "ocrl_tp_colsum: null argument");
    OCRL_REQUIRE(R >= 1 && R <= MAX_ELEMS && F >= 1 && F <= 65536, "ocrl_tp_colsum: 1 <= R < 2^31 and 1 <= F <= 65536 (got %lld, %d)", R, F);
    OCRL_REQUIRE(ld >= F && ld <= MAX_ELEMS, "ocrl_tp_colsum: ld >= F (got ld %lld, F %d)", ld, F);
    OCRL_REQUIRE(aligned16(ws), "ocrl_tp_colsum: ws must be 16-byte aligned");
    return colsum_launch(X, ld, out, R, F, accumulate ? 1 : 0, scale, ws, ws_floats, static_cast<hipStream_t>(stream));
}

int ocrl_tp_mse(const float* obs, const float* recon, float* drecon, float* out, int B, int C, int H, int W, float* ws, size_t ws_floats,
                void* stream) {
    OCRL_REQUIRE(obs && recon && out && ws, "ocrl_tp_mse: null argument (obs, recon, out or ws)");
    OCRL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W * 4 <= MAX_ELEMS, "ocrl_tp_mse: B, H, W >= 1 (got %d, %d, %d)", B, H, W);
    OCRL_REQUIRE(C >= 1 && C <= 4, "ocrl_tp_mse: 1 <= C <= 4 (got %d)", C);
    OCRL_REQUIRE(ws_floats >= 1024, "ocrl_tp_mse: workspace too small (%zu < 1024 floats)", ws_floats);
    OCRL_REQUIRE(aligned16(recon, drecon), "ocrl_tp_mse: recon and drecon must be 16-byte aligned");
    return mse_launch(obs, recon, drecon, out, B, C, H, W, ws, ws_floats, static_cast<hipStream_t>(stream));
}

int ocrl_tp_pixel_shuffle(const float* in, float* out, int B, int h, int w, int Cout, int forward, const float* mask, void* stream) {
    OCRL_REQUIRE(in && out, "ocrl_tp_pixel_shuffle: null argument");
    OCRL_REQUIRE(B >= 1 && h >= 1 && w >= 1 && Cout >= 1, "ocrl_tp_pixel_shuffle: B, h, w, Cout >= 1 (got %d, %d, %d, %d)", B, h, w, Cout);
    OCRL_REQUIRE((long long)B * h * w * Cout * 4 <= MAX_ELEMS, "ocrl_tp_pixel_shuffle: 4 B h w Cout < 2^31");
    OCRL_REQUIRE(!forward || !mask, "ocrl_tp_pixel_shuffle: the mask belongs to the inverse map");
    OCRL_REQUIRE(aligned16(in, out, mask), "ocrl_tp_pixel_shuffle: in, out and mask must be 16-byte aligned");
    return pixel_shuffle_launch(in, out, B, h, w, Cout, forward ? 1 : 0, mask, static_cast<hipStream_t>(stream));
}

int ocrl_tp_nchw_to_nhwc8(const float* in, float* out, int B, int C, int H, int W, void* stream) {
    OCRL_REQUIRE(in && out, "ocrl_tp_nchw_to_nhwc8: null argument");
    OCRL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W * 8 <= MAX_ELEMS, "ocrl_tp_nchw_to_nhwc8: B, H, W >= 1 (got %d, %d, %d)", B, H, W);
    OCRL_REQUIRE(C >= 1 && C <= 8, "ocrl_tp_nchw_to_nhwc8: 1 <= C <= 8 (got %d)", C);
    OCRL_REQUIRE(aligned16(out), "ocrl_tp_nchw_to_nhwc8: out must be 16-byte aligned");
    return nchw_to_nhwc8_launch(in, out, B, C, H, W, static_cast<hipStream_t>(stream));
}

int ocrl_tp_patchify4(const float* in, float* out, int B, int C, int S, void* stream) {
    OCRL_REQUIRE(in && out, "ocrl_tp_patchify4: null argument");
    OCRL_REQUIRE(B >= 1 && C >= 1 && S >= 4 && S % 4 == 0, "ocrl_tp_patchify4: B, C >= 1 and S %% 4 == 0, S >= 4 (got %d, %d, %d)", B, C, S);
    OCRL_REQUIRE((long long)B * C * S * S <= MAX_ELEMS, "ocrl_tp_patchify4: B C S S < 2^31");
    OCRL_REQUIRE(aligned16(in, out), "ocrl_tp_patchify4: in and out must be 16-byte aligned");
    return patchify4_launch(in, out, B, C, S, static_cast<hipStream_t>(stream));
}

int ocrl_tp_pad_cols(const float* in, int ldi, float* out, int ldo, long long R, int C, int Cout, void* stream) {
    OCRL_REQUIRE(in && out, "ocrl_tp_pad_cols: null argument");
    OCRL_REQUIRE(R >= 1 && C >= 1 && Cout >= 1, "ocrl_tp_pad_cols: R, C, Cout >= 1 (got %lld, %d, %d)", R, C, Cout);
    OCRL_REQUIRE(ldo >= Cout && ldi >= C, "ocrl_tp_pad_cols: ldo >= Cout and ldi >= C (got ldo %d, Cout %d, ldi %d, C %d)", ldo, Cout, ldi, C);
    OCRL_REQUIRE(R * (long long)(ldo > ldi ? ldo : ldi) <= MAX_ELEMS, "ocrl_tp_pad_cols: R * ld < 2^31");
    return pad_cols_launch(in, ldi, out, ldo, R, C, Cout, static_cast<hipStream_t>(stream));
}

int ocrl_tp_im2col5(const float* x8, float* col, int B, int H, int W, int C, int ldc, void* stream) {
    OCRL_REQUIRE(x8 && col, "ocrl_tp_im2col5: null argument");
    OCRL_REQUIRE(B >= 1 && H >= 1 && W >= 1, "ocrl_tp_im2col5: B, H, W >= 1 (got %d, %d, %d)", B, H, W);
    OCRL_REQUIRE(C >= 1 && C <= 8, "ocrl_tp_im2col5: 1 <= C <= 8 (got %d)", C);
    OCRL_REQUIRE(ldc >= 25 * C, "ocrl_tp_im2col5: ldc >= 25 C (got ldc %d, C %d)", ldc, C);
    OCRL_REQUIRE((long long)B * H * W * ldc <= MAX_ELEMS, "ocrl_tp_im2col5: B H W ldc < 2^31");
    return im2col5_launch(x8, col, (long long)B * H * W, H, W, C, ldc, static_cast<hipStream_t>(stream));
}

int ocrl_tp_unpack5(const float* dWp, float* dW, int C, int ldc, void* stream) {
    OCRL_REQUIRE(dWp && dW, "ocrl_tp_unpack5: null argument");
    OCRL_REQUIRE(C >= 1 && C <= 8, "ocrl_tp_unpack5: 1 <= C <= 8 (got %d)", C);
    OCRL_REQUIRE(ldc >= 25 * C && ldc <= (1 << 20), "ocrl_tp_unpack5: 25 C <= ldc <= 2^20 (got ldc %d, C %d)", ldc, C);
    return unpack5_launch(dWp, dW, C, ldc, static_cast<hipStream_t>(stream));
}

int ocrl_tp_posmap(const float* Wpos, const float* bpos, float* out, int S, int C, void* stream) {
    OCRL_REQUIRE(Wpos && bpos && out, "ocrl_tp_posmap: null argument");
    OCRL_REQUIRE(S >= 1 && C >= 1 && (long long)S * S * C <= MAX_ELEMS, "ocrl_tp_posmap: S, C >= 1 and S S C < 2^31 (got %d, %d)", S, C);
    return posmap_launch(Wpos, bpos, out, S, C, static_cast<hipStream_t>(stream));
}

int ocrl_tp_posgrid(float* out, int S, void* stream) {
    OCRL_REQUIRE(out, "ocrl_tp_posgrid: null argument");
    OCRL_REQUIRE(S >= 1 && S <= 16384, "ocrl_tp_posgrid: 1 <= S <= 16384 (got %d)", S);
    OCRL_REQUIRE(aligned16(out), "ocrl_tp_posgrid: out must be 16-byte aligned");
    return posgrid_launch(out, S, static_cast<hipStream_t>(stream));
}

int ocrl_tp_onehot(const int* tokens, float* z, long long rows, int V, void* stream) {
    OCRL_REQUIRE(tokens && z, "ocrl_tp_onehot: null argument");
    OCRL_REQUIRE(rows >= 1 && V >= 1 && rows * V <= MAX_ELEMS, "ocrl_tp_onehot: rows, V >= 1 and rows V < 2^31 (got %lld, %d)", rows, V);
    return onehot_launch(tokens, z, rows, V, static_cast<hipStream_t>(stream));
}

int ocrl_tp_slot_init(const float* mu, const float* logsig, const float* noise, float* slots0, int BK, int D, unsigned long long seed,
                      void* stream) {
    OCRL_REQUIRE(mu && logsig && slots0, "ocrl_tp_slot_init: null argument (mu, logsig or slots0)");
    OCRL_REQUIRE(BK >= 1 && D >= 1 && (long long)BK * D <= MAX_ELEMS, "ocrl_tp_slot_init: BK, D >= 1 and BK D < 2^31 (got %d, %d)", BK, D);
    return slot_init_launch(mu, logsig, noise, slots0, BK, D, seed, static_cast<hipStream_t>(stream), nullptr);
}

int ocrl_tp_slot_init_bwd(const float* dslots0, const float* logsig, const float* noise, float* dmu, float* dlogsig, int BK, int D,
                          unsigned long long seed, void* stream) {
    OCRL_REQUIRE(dslots0 && logsig && dmu && dlogsig, "ocrl_tp_slot_init_bwd: null argument (dslots0, logsig, dmu or dlogsig)");
    OCRL_REQUIRE(BK >= 1 && D >= 1 && (long long)BK * D <= MAX_ELEMS, "ocrl_tp_slot_init_bwd: BK, D >= 1 and BK D < 2^31 (got %d, %d)", BK, D);
    return slot_init_bwd_launch(dslots0, logsig, noise, dmu, dlogsig, BK, D, seed, static_cast<hipStream_t>(stream));
}

int ocrl_tp_argmax_pos(const float* pred, int* tokens, int B, int T, int V, int t, int dense_rows, void* stream) {
    OCRL_REQUIRE(pred && tokens, "ocrl_tp_argmax_pos: null argument");
    OCRL_REQUIRE(B >= 1 && T >= 1 && V >= 1 && (long long)B * T * V <= MAX_ELEMS, "ocrl_tp_argmax_pos: B, T, V >= 1 (got %d, %d, %d)", B, T, V);
    OCRL_REQUIRE(t >= 0 && t < T, "ocrl_tp_argmax_pos: 0 <= t < T (got t %d, T %d)", t, T);
    return argmax_pos_launch(pred, tokens, B, T, V, t, static_cast<hipStream_t>(stream), dense_rows ? 1 : 0);
}

int ocrl_tp_decode_attn(const float* qkv, float* out, int B, int T, int t, int d, int h, int ld, void* stream) {
    OCRL_REQUIRE(qkv && out, "ocrl_tp_decode_attn: null argument");
    OCRL_REQUIRE(B >= 1 && T >= 1 && d >= 1 && h >= 1, "ocrl_tp_decode_attn: B, T, d, h >= 1 (got %d, %d, %d, %d)", B, T, d, h);
    OCRL_REQUIRE(d % h == 0 && (d / h) % 4 == 0 && d / h <= 64, "ocrl_tp_decode_attn: d %% h == 0 and a head width that is a multiple of 4, <= 64 (got d %d, h %d)", d, h);
    OCRL_REQUIRE(t >= 0 && t < T, "ocrl_tp_decode_attn: 0 <= t < T (got t %d, T %d)", t, T);
    OCRL_REQUIRE(ld % 4 == 0 && ld >= 3 * (long long)d, "ocrl_tp_decode_attn: ld %% 4 == 0 and ld >= 3 d (got ld %d, d %d)", ld, d);
    OCRL_REQUIRE((long long)B * T * ld <= MAX_ELEMS && (long long)B * h <= MAX_ELEMS, "ocrl_tp_decode_attn: B T ld < 2^31");
    OCRL_REQUIRE(aligned16(qkv), "ocrl_tp_decode_attn: qkv must be 16-byte aligned");
    return decode_attn_launch(qkv, out, B, T, t, d, h, ld, static_cast<hipStream_t>(stream));
}

}  // extern "C"
