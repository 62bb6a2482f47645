// C ABI of the slot-set pooling head (include/ocrl_hip.h: ocrl_pool_transformer_*): poolings/common/transformer.py:9-33
// (Linear -> [CLS; tokens] (+pos) -> nn.TransformerEncoder(num_layers x post-norm TransformerEncoderLayer, ReLU) -> CLS row), the
// consumer of the slots on the RL side (sb3s/ocr_extractor.py:45).  Stateless: the caller owns parameters, gradients and the
// workspace (the parameters belong to the RL policy's optimiser in the reference); forward leaves what backward needs in `ws`.
#include <math.h>

#include "../../include/ocrl_hip.h"
#include "unit_base.h"

namespace {
constexpr unsigned SITE_POOL = 300;      // + 8 * layer + {0: attention weights, 1: dropout1, 2: FFN hidden, 3: dropout2}
constexpr size_t TMP_FLOATS = (size_t)1 << 17;
constexpr int WS_DIN = 256;               // the workspace query has no rep_dim: split-k slabs are sized for rep_dim <= 256 (wider inputs get fewer splits)

// the saved tensors of one full post-norm layer on R = B S rows.  The attention keeps its [B,h,S,S] weights P (short form) or the
// per-row log-sum-exp lse (long form, pool_flash); the other one is empty.
struct LayerLay {
    size_t x, qkv, P, o, lse, y1, mr1, x1, hdn, y2, mr2;      // x = layer input; output = next layer's x
};
// x on R rows, the rest on r rows (r = 0: a layer that saves only its input)
void layer_layout(LayerLay& q, WsTake& take, size_t R, size_t r, int d, int ff, size_t P_floats, size_t lse_floats) {
    q.x = take(R * d); q.qkv = take(r * 3 * d); q.P = take(P_floats); q.o = take(r * d); q.lse = take(lse_floats); q.y1 = take(r * d);
    q.mr1 = take(2 * r); q.x1 = take(r * d); q.hdn = take(r * ff); q.y2 = take(r * d); q.mr2 = take(2 * r);
}
// backward scratch of the full layers, and the split-k scratch: both forms carve these
struct GradLay { size_t gA, gB, dqkv, dhdn, Dd, dgb, dlin, tmp, sk, sk_floats; };
// split-k scratch of the weight gradients (the rows of a PPO minibatch are the k dimension): the largest weight, the widest biases
size_t sk_floats_of(size_t R, int Din, int d, int ff) {
    size_t slab = (size_t)ff * d;
    if ((size_t)3 * d * d > slab) slab = (size_t)3 * d * d;
    if ((size_t)d * Din > slab) slab = (size_t)d * Din;
    return splitk_scratch_floats(R, slab + (size_t)ff + 3 * (size_t)d + 8);
}

struct Lay : GradLay {
    size_t lin, xlast, gC, total;
    LayerLay l[OCRL_POOL_MAX_LAYERS];
};
Lay layout(int B, int K, int Din, int d, int h, int ff, int L) {
    Lay y;
    WsTake take;
    const size_t S = K + 1, R = (size_t)B * S;
    y.lin = take((size_t)B * K * d);
    for (int l = 0; l < L; ++l) layer_layout(y.l[l], take, R, R, d, ff, (size_t)B * h * S * S, 0);
    y.xlast = take(R * d);
    y.gA = take(R * d); y.gB = take(R * d); y.gC = take(R * d);
    y.dqkv = take(R * 3 * d); y.dhdn = take(R * ff); y.dgb = take(2 * (size_t)d); y.dlin = take((size_t)B * K * d);
    y.tmp = take(TMP_FLOATS);
    y.Dd = 0;                                    // the saved P needs no row-dot scratch
    y.sk_floats = sk_floats_of(R, Din, d, ff);
    y.sk = take(y.sk_floats);
    y.total = take.end;
    return y;
}

int check_dims(int B, int K, int Din, int d, int h, int ff, int L) {
    OCRL_REQUIRE(B > 0, "pool_transformer: batch must be >= 1 (got %d)", B);
    // slots, rep_dim, d_model, nhead, the head size and the LDS request of BOTH directions (pool.hip holds them once): a shape whose
    // backward would be refused never runs its forward
    RC(pool_short_check(K, Din, d, h));
    OCRL_REQUIRE(L >= 1 && L <= OCRL_POOL_MAX_LAYERS, "pool_transformer: 1 <= num_layers <= %d (got %d)", OCRL_POOL_MAX_LAYERS, L);
    OCRL_REQUIRE(ff >= 4 && ff % 4 == 0, "pool_transformer: d_model must be a multiple of 64 <= 256, rep_dim/ff multiples of 4");
    return 0;
}

// one call's shape, dropout stream and workspace; flash: the long form's attention (saved lse, Dd scratch) instead of the saved P
struct Enc { int B, S, d, h, ff; float p; unsigned long long seed; bool flash; float* ws; hipStream_t st; };

// full post-norm layer l on the R = B S rows of a.x -> xn
int enc_layer_fwd(const Enc& e, const LayerLay& a, int l, const float* const* q, float* xn) {
    float* ws = e.ws;
    hipStream_t st = e.st;
    const int d = e.d, ff = e.ff;
    const long long R = (long long)e.B * e.S;
    const unsigned site = SITE_POOL + 8 * l;
    RC(lin_fwd(ws + a.x, d, q[0], q[1], ws + a.qkv, 3 * d, R, 3 * d, d, 0, nullptr, 0, st));
    if (e.flash) RC(pool_flash_launch(ws + a.qkv, ws + a.o, ws + a.lse, nullptr, nullptr, nullptr, e.B, e.S, d, e.h, e.p, e.seed, site + 0, 0, st));
    else RC(pool_attn_launch(ws + a.qkv, ws + a.P, ws + a.o, nullptr, nullptr, e.B, e.S, d, e.h, e.p, e.seed, site + 0, 0, st));
    RC(lin_fwd(ws + a.o, d, q[2], q[3], ws + a.y1, d, R, d, d, 0, ws + a.x, d, st, Drop{e.p, e.seed, site + 1}));                 // x + dropout1(attn)
    RC(layernorm_fwd_launch(ws + a.y1, q[8], q[9], ws + a.x1, ws + a.mr1, ws + a.mr1 + R, R, d, st));
    RC(lin_fwd(ws + a.x1, d, q[4], q[5], ws + a.hdn, ff, R, ff, d, 1, nullptr, 0, st, Drop{e.p, e.seed, site + 2}));              // dropout(relu(linear1))
    RC(lin_fwd(ws + a.hdn, ff, q[6], q[7], ws + a.y2, d, R, d, ff, 0, ws + a.x1, d, st, Drop{e.p, e.seed, site + 3}));             // x1 + dropout2(linear2)
    return layernorm_fwd_launch(ws + a.y2, q[10], q[11], xn, ws + a.mr2, ws + a.mr2 + R, R, d, st);
}

// dx of out = LN(y) on R rows (mr = saved mean | rstd); the weight and bias gradients through dgb into dgam, dbeta
int ln_bwd(const float* dout, const float* yv, const float* mr, const float* gam, float* dx, float* dgam, float* dbeta, long long R, int d, float* dgb,
           float* tmp, hipStream_t st) {
    RC(layernorm_bwd_launch(dout, yv, mr, mr + R, gam, dx, dgb, R, d, 0, 0, tmp, TMP_FLOATS, st));
    RC(copy_launch(dgb, dgam, d, st));
    return copy_launch(dgb + d, dbeta, d, st);
}

// its backward: g2 = gradient of the layer's output on entry, of its input on return
int enc_layer_bwd(const Enc& e, const LayerLay& a, const GradLay& y, int l, const float* const* q, float* const* g, float* g2) {
    float* ws = e.ws;
    hipStream_t st = e.st;
    const int d = e.d, ff = e.ff;
    const long long R = (long long)e.B * e.S;
    const unsigned site = SITE_POOL + 8 * l;
    const float inv_keep = e.p > 0.f ? 1.f / (1.f - e.p) : 1.f;
    float *gA = ws + y.gA, *gB = ws + y.gB, *sk = ws + y.sk;
    // x2 = LN2(y2)
    RC(ln_bwd(g2, ws + a.y2, ws + a.mr2, q[10], gA, g[10], g[11], R, d, ws + y.dgb, ws + y.tmp, st));
    // y2 = x1 + dropout2(hdn W2^T + b2),  hdn = dropout(relu(x1 W1^T + b1))
    RC(lin_bwd_w(gA, d, ws + a.hdn, ff, g[6], g[7], R, d, ff, 1.f, sk, y.sk_floats, st, Drop{e.p, e.seed, site + 3}));
    RC(lin_bwd_x(gA, d, q[6], ws + y.dhdn, ff, R, d, ff, ws + a.hdn, ff, nullptr, 0, st, Drop{e.p, e.seed, site + 3}, Xf(), inv_keep));
    RC(lin_bwd_w(ws + y.dhdn, ff, ws + a.x1, d, g[4], g[5], R, ff, d, 1.f, sk, y.sk_floats, st));
    RC(lin_bwd_x(ws + y.dhdn, ff, q[4], gB, d, R, ff, d, nullptr, 0, gA, d, st));                    // + residual
    // x1 = LN1(y1)
    RC(ln_bwd(gB, ws + a.y1, ws + a.mr1, q[8], gA, g[8], g[9], R, d, ws + y.dgb, ws + y.tmp, st));
    // y1 = x + dropout1(o Wo^T + bo)
    RC(lin_bwd_w(gA, d, ws + a.o, d, g[2], g[3], R, d, d, 1.f, sk, y.sk_floats, st, Drop{e.p, e.seed, site + 1}));
    RC(lin_bwd_x(gA, d, q[2], gB, d, R, d, d, nullptr, 0, nullptr, 0, st, Drop{e.p, e.seed, site + 1}));
    if (e.flash) RC(pool_flash_launch(ws + a.qkv, ws + a.o, ws + a.lse, gB, ws + y.Dd, ws + y.dqkv, e.B, e.S, d, e.h, e.p, e.seed, site + 0, 1, st));
    else RC(pool_attn_launch(ws + a.qkv, ws + a.P, nullptr, gB, ws + y.dqkv, e.B, e.S, d, e.h, e.p, e.seed, site + 0, 1, st));
    RC(lin_bwd_w(ws + y.dqkv, 3 * d, ws + a.x, d, g[0], g[1], R, 3 * d, d, 1.f, sk, y.sk_floats, st));
    return lin_bwd_x(ws + y.dqkv, 3 * d, q[0], g2, d, R, 3 * d, d, nullptr, 0, gA, d, st);                  // + residual
}
}  // namespace

extern "C" {

size_t ocrl_pool_transformer_ws_floats(int B, int K, int d, int nhead, int ff, int L) {
    if (L < 1 || L > OCRL_POOL_MAX_LAYERS) return 0;
    return layout(B, K, WS_DIN, d, nhead, ff, L).total;
}

int ocrl_pool_transformer_fwd(const float* slots, const float* const* w, const float* pos, float* out, int B, int K, int Din, int d, int nhead, int ff, int L,
                              float drop_p, unsigned long long seed, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(slots && w && out && ws, "ocrl_pool_transformer_fwd: null argument");
    RC(check_dims(B, K, Din, d, nhead, ff, L));
    const Lay y = layout(B, K, WS_DIN, d, nhead, ff, L);
    RC(ws_check("ocrl_pool_transformer_fwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Enc e{B, K + 1, d, nhead, ff, drop_p, seed, false, ws, st};
    RC(lin_fwd(slots, Din, w[0], w[1], ws + y.lin, d, (long long)B * K, d, Din, 0, nullptr, 0, st));
    RC(pool_embed_launch(ws + y.lin, w[2], pos, ws + y.l[0].x, B, K, d, st));
    for (int l = 0; l < L; ++l) RC(enc_layer_fwd(e, y.l[l], l, w + 3 + 12 * l, ws + (l + 1 < L ? y.l[l + 1].x : y.xlast)));
    RC(pool_rows_launch(ws + y.xlast, out, B, K, d, 2, st));
    return 0;
}

int ocrl_pool_transformer_bwd(const float* slots, const float* dout, const float* const* w, float* dslots, float* const* dw, int B, int K, int Din, int d,
                              int nhead, int ff, int L, float drop_p, unsigned long long seed, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(slots && dout && w && dw && ws, "ocrl_pool_transformer_bwd: null argument");
    RC(check_dims(B, K, Din, d, nhead, ff, L));
    const Lay y = layout(B, K, WS_DIN, d, nhead, ff, L);
    RC(ws_check("ocrl_pool_transformer_bwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = K + 1;
    const Enc e{B, S, d, nhead, ff, drop_p, seed, false, ws, st};
    float *g2 = ws + y.gC, *tmp = ws + y.tmp;
    RC(pool_rows_launch(dout, g2, B, K, d, 1, st));                                                           // only the CLS row is consumed
    for (int l = L - 1; l >= 0; --l) RC(enc_layer_bwd(e, y.l[l], y, l, w + 3 + 12 * l, dw + 3 + 12 * l, g2));
    // x0 = [cls; Linear(slots)] (+pos)
    RC(colsum_launch(g2, (long long)S * d, dw[2], B, d, 0, 1.f, tmp, TMP_FLOATS, st));
    RC(pool_rows_launch(g2, ws + y.dlin, B, K, d, 0, st));
    RC(lin_bwd_w(ws + y.dlin, d, slots, Din, dw[0], dw[1], (long long)B * K, d, Din, 1.f, ws + y.sk, y.sk_floats, st));
    if (dslots) RC(lin_bwd_x(ws + y.dlin, d, w[0], dslots, Din, (long long)B * K, d, Din, nullptr, 0, nullptr, 0, st));
    return 0;
}

// keep-mask of one dropout site (1 = kept), for parity tests: which = 0 attention [B,h,S,S], 1 dropout1 [B,S,d], 2 FFN hidden [B,S,ff], 3 dropout2 [B,S,d]
int ocrl_pool_transformer_dropout_mask(int layer, int which, long long n, float drop_p, unsigned long long seed, float* out, void* stream) {
    OCRL_REQUIRE(out && layer >= 0 && which >= 0 && which < 4, "ocrl_pool_transformer_dropout_mask: bad argument");
    return dropout_mask_launch(out, n, drop_p, seed, SITE_POOL + 8 * layer + which, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// ---------------------------------------------------------------- long token sequences (a CNN feature map: include/ocrl_hip.h ocrl_pool_transformer_long_*)
// Same parameters, dropout sites and element indices as above.  Layers before the last run on all B*S rows (GEMM / LayerNorm family,
// pool_flash attention: the saved log-sum-exp replaces the [B,h,S,S] weights).  The last layer is evaluated for the CLS row only: its
// attention is one pass over the token rows (pool_cls_*, the projections folded), out_proj / LN1 / FFN / LN2 run on B rows.
namespace {
struct LongLay : GradLay {
    int Dp;                                              // rep_dim padded to a multiple of 4
    size_t sp, wp, dwp, dsp, lin;
    LayerLay l[OCRL_POOL_MAX_LAYERS];                    // qkv .. mr2 only for the full layers (l < L-1)
    size_t x0c, q, U, part, z, stat, ov, at, y1, mr1, x1, hdn, y2, mr2;      // last layer (B rows / CLS attention)
    size_t g2, G, gD, w, dq, dO, cA, cB, cAd, chd, total;
};
LongLay long_layout(int B, int K, int Din, int d, int h, int ff, int L) {
    LongLay y;
    WsTake take;
    const size_t S = (size_t)K + 1, R = (size_t)B * S, BK = (size_t)B * K;
    const int nchunk = pool_cls_nchunk(B, (int)S, nullptr);
    y.Dp = pad4(Din);
    y.sp = take(pad4_floats(BK, Din)); y.wp = take(pad4_floats(d, Din)); y.dwp = take(pad4_floats(d, Din)); y.dsp = take(pad4_floats(BK, Din));
    y.lin = take(BK * d);
    for (int l = 0; l < L; ++l) layer_layout(y.l[l], take, R, l + 1 < L ? R : 0, d, ff, 0, l + 1 < L ? (size_t)B * h * S : 0);
    const size_t Bd = (size_t)B * d, Bhd = (size_t)B * h * d;
    y.x0c = take(Bd); y.q = take(Bd); y.U = take(Bhd); y.part = take((size_t)B * nchunk * h * (d + 4)); y.z = take(Bhd); y.stat = take((size_t)2 * B * h);
    y.ov = take(Bd); y.at = take(Bd); y.y1 = take(Bd); y.mr1 = take(2 * (size_t)B); y.x1 = take(Bd); y.hdn = take((size_t)B * ff); y.y2 = take(Bd);
    y.mr2 = take(2 * (size_t)B);
    const size_t rf = L > 1 ? R : 0;                     // gradient buffers of the full layers
    y.g2 = take(R * d); y.gA = take(rf * d); y.gB = take(rf * d); y.dqkv = take(rf * 3 * d); y.dhdn = take(rf * ff); y.Dd = take(L > 1 ? (size_t)B * h * S : 0);
    y.G = take(Bhd); y.gD = take((size_t)2 * B * h); y.w = take(Bhd); y.dq = take(Bd); y.dO = take(Bd);
    y.cA = take(Bd); y.cB = take(Bd); y.cAd = take(Bd); y.chd = take((size_t)B * ff); y.dgb = take(2 * (size_t)d); y.dlin = take(BK * d);
    y.tmp = take(TMP_FLOATS);
    y.sk_floats = sk_floats_of(R, y.Dp, d, ff);
    y.sk = take(y.sk_floats);
    y.total = take.end;
    return y;
}
int check_dims_long(int B, int K, int Din, int d, int h, int ff, int L) {
    OCRL_REQUIRE(B > 0 && K >= 1 && Din >= 1, "pool_transformer_long: batch, tokens and rep_dim must be >= 1 (got %d, %d, %d)", B, K, Din);
    OCRL_REQUIRE(L >= 1 && L <= OCRL_POOL_MAX_LAYERS, "pool_transformer_long: 1 <= num_layers <= %d (got %d)", OCRL_POOL_MAX_LAYERS, L);
    OCRL_REQUIRE(ff >= 4 && ff % 4 == 0 && d % 64 == 0 && d >= 64 && d <= 256, "pool_transformer_long: d_model must be a multiple of 64 <= 256, ff a multiple of 4");
    OCRL_REQUIRE(h >= 1 && d % h == 0 && (d / h == 16 || d / h == 32 || d / h == 48 || d / h == 64),
                 "pool_transformer_long: head size d_model / nhead must be 16, 32, 48 or 64 (got %d / %d)", d, h);
    OCRL_REQUIRE((long long)B * (K + 1) * 3 * d < (1LL << 31) && (L == 1 || (long long)B * (K + 1) * ff < (1LL << 31)),
                 "pool_transformer_long: B * (K + 1) rows too many for one call");
    return 0;
}
}  // namespace

extern "C" {

size_t ocrl_pool_transformer_long_ws_floats(int B, int K, int Din, int d, int nhead, int ff, int L) {
    if (check_dims_long(B, K, Din, d, nhead, ff, L)) return 0;           // the shapes fwd / bwd reject get no workspace
    return long_layout(B, K, Din, d, nhead, ff, L).total;
}

int ocrl_pool_transformer_long_fwd(const float* slots, const float* const* w, const float* pos, float* out, int B, int K, int Din, int d, int nhead, int ff,
                                   int L, float drop_p, unsigned long long seed, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(slots && w && out && ws, "ocrl_pool_transformer_long_fwd: null argument");
    RC(check_dims_long(B, K, Din, d, nhead, ff, L));
    const LongLay y = long_layout(B, K, Din, d, nhead, ff, L);
    RC(ws_check("ocrl_pool_transformer_long_fwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = K + 1, Dp = y.Dp;
    const long long BK = (long long)B * K;
    const Enc e{B, S, d, nhead, ff, drop_p, seed, true, ws, st};
    const float *xs, *w0;                               // the slots and the input Linear's weight at stride Dp
    RC(pad4_view(slots, Din, ws + y.sp, BK, &xs, st));
    RC(pad4_view(w[0], Din, ws + y.wp, d, &w0, st));
    RC(lin_fwd(xs, Dp, w0, w[1], ws + y.lin, d, BK, d, Dp, 0, nullptr, 0, st));
    RC(pool_embed_launch(ws + y.lin, w[2], pos, ws + y.l[0].x, B, K, d, st));
    for (int l = 0; l + 1 < L; ++l) RC(enc_layer_fwd(e, y.l[l], l, w + 3 + 12 * l, ws + y.l[l + 1].x));
    // last layer: the CLS row
    const float* const* q = w + 3 + 12 * (L - 1);
    const unsigned site = SITE_POOL + 8 * (L - 1);
    const float* X = ws + y.l[L - 1].x;
    RC(pool_rows_launch(X, ws + y.x0c, B, K, d, 2, st));
    RC(lin_fwd(ws + y.x0c, d, q[0], q[1], ws + y.q, d, B, d, d, 0, nullptr, 0, st));            // rows 0..d-1 of in_proj: the query
    PoolClsArgs c;
    c.X = X; c.Win = q[0]; c.bin = q[1]; c.q = ws + y.q; c.U = ws + y.U; c.part = ws + y.part; c.z = ws + y.z; c.stat = ws + y.stat; c.o = ws + y.ov;
    c.B = B; c.S = S; c.d = d; c.h = nhead; c.p = drop_p; c.seed = seed; c.site = site + 0;
    RC(pool_cls_attn_fwd_launch(c, st));
    RC(lin_fwd(ws + y.ov, d, q[2], q[3], ws + y.at, d, B, d, d, 0, nullptr, 0, st));
    RC(pool_cls_drop_launch(ws + y.at, ws + y.x0c, d, ws + y.y1, B, d, S, drop_p, seed, site + 1, st));         // x + dropout1(attn)
    RC(layernorm_fwd_launch(ws + y.y1, q[8], q[9], ws + y.x1, ws + y.mr1, ws + y.mr1 + B, B, d, st));
    RC(lin_fwd(ws + y.x1, d, q[4], q[5], ws + y.hdn, ff, B, ff, d, 1, nullptr, 0, st));
    RC(pool_cls_drop_launch(ws + y.hdn, nullptr, 0, ws + y.hdn, B, ff, S, drop_p, seed, site + 2, st));         // dropout(relu(linear1))
    RC(lin_fwd(ws + y.hdn, ff, q[6], q[7], ws + y.at, d, B, d, ff, 0, nullptr, 0, st));
    RC(pool_cls_drop_launch(ws + y.at, ws + y.x1, d, ws + y.y2, B, d, S, drop_p, seed, site + 3, st));          // x1 + dropout2(linear2)
    RC(layernorm_fwd_launch(ws + y.y2, q[10], q[11], out, ws + y.mr2, ws + y.mr2 + B, B, d, st));
    return 0;
}

int ocrl_pool_transformer_long_bwd(const float* slots, const float* dout, const float* const* w, float* dslots, float* const* dw, int B, int K, int Din,
                                   int d, int nhead, int ff, int L, float drop_p, unsigned long long seed, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(slots && dout && w && dw && ws, "ocrl_pool_transformer_long_bwd: null argument");
    RC(check_dims_long(B, K, Din, d, nhead, ff, L));
    const LongLay y = long_layout(B, K, Din, d, nhead, ff, L);
    RC(ws_check("ocrl_pool_transformer_long_bwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = K + 1, Dp = y.Dp;
    const long long BK = (long long)B * K;
    const Enc e{B, S, d, nhead, ff, drop_p, seed, true, ws, st};
    const float inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    float *g2 = ws + y.g2, *tmp = ws + y.tmp, *dgb = ws + y.dgb;
    {   // last layer: B rows, then the CLS attention back to every token row (g2 = gradient of the layer input)
        const float* const* q = w + 3 + 12 * (L - 1);
        float* const* g = dw + 3 + 12 * (L - 1);
        const unsigned site = SITE_POOL + 8 * (L - 1);
        float *cA = ws + y.cA, *cB = ws + y.cB, *cAd = ws + y.cAd;
        RC(ln_bwd(dout, ws + y.y2, ws + y.mr2, q[10], cA, g[10], g[11], B, d, dgb, tmp, st));
        RC(pool_cls_drop_launch(cA, nullptr, 0, cAd, B, d, S, drop_p, seed, site + 3, st));
        RC(lin_bwd_w(cAd, d, ws + y.hdn, ff, g[6], g[7], B, d, ff, 1.f, ws + y.sk, y.sk_floats, st));
        RC(lin_bwd_x(cAd, d, q[6], ws + y.chd, ff, B, d, ff, ws + y.hdn, ff, nullptr, 0, st, Drop(), Xf(), inv_keep));
        RC(lin_bwd_w(ws + y.chd, ff, ws + y.x1, d, g[4], g[5], B, ff, d, 1.f, ws + y.sk, y.sk_floats, st));
        RC(lin_bwd_x(ws + y.chd, ff, q[4], cB, d, B, ff, d, nullptr, 0, cA, d, st));                   // + residual
        RC(ln_bwd(cB, ws + y.y1, ws + y.mr1, q[8], cA, g[8], g[9], B, d, dgb, tmp, st));
        RC(pool_cls_drop_launch(cA, nullptr, 0, cAd, B, d, S, drop_p, seed, site + 1, st));
        RC(lin_bwd_w(cAd, d, ws + y.ov, d, g[2], g[3], B, d, d, 1.f, ws + y.sk, y.sk_floats, st));
        RC(lin_bwd_x(cAd, d, q[2], ws + y.dO, d, B, d, d, nullptr, 0, nullptr, 0, st));
        PoolClsArgs c;
        c.X = ws + y.l[L - 1].x; c.Win = q[0]; c.bin = q[1]; c.q = ws + y.q; c.U = ws + y.U; c.part = ws + y.part; c.z = ws + y.z; c.stat = ws + y.stat;
        c.dO = ws + y.dO; c.G = ws + y.G; c.gD = ws + y.gD; c.dX = g2; c.w = ws + y.w; c.dq = ws + y.dq; c.x0 = ws + y.x0c; c.dW = g[0]; c.db = g[1];
        c.B = B; c.S = S; c.d = d; c.h = nhead; c.p = drop_p; c.seed = seed; c.site = site + 0;
        RC(pool_cls_attn_bwd_launch(c, st));
        RC(lin_bwd_x(ws + y.dq, d, q[0], cB, d, B, d, d, nullptr, 0, cA, d, st));                    // row 0: W_q^T dq + residual
        RC(pool_cls_add_launch(g2, cB, B, d, S, st));
    }
    for (int l = L - 2; l >= 0; --l) RC(enc_layer_bwd(e, y.l[l], y, l, w + 3 + 12 * l, dw + 3 + 12 * l, g2));
    // x0 = [cls; Linear(slots)] (+pos)
    RC(colsum_launch(g2, (long long)S * d, dw[2], B, d, 0, 1.f, tmp, TMP_FLOATS, st));
    RC(pool_rows_launch(g2, ws + y.dlin, B, K, d, 0, st));
    const float *xs, *w0;
    RC(pad4_view(slots, Din, ws + y.sp, BK, &xs, st));
    RC(pad4_view(w[0], Din, ws + y.wp, d, &w0, st));
    RC(lin_bwd_w(ws + y.dlin, d, xs, Dp, pad4_sel(dw[0], Din, ws + y.dwp), dw[1], BK, d, Dp, 1.f, ws + y.sk, y.sk_floats, st));
    RC(pad4_unpad(ws + y.dwp, Din, dw[0], d, st));
    if (dslots) {
        RC(lin_bwd_x(ws + y.dlin, d, w0, pad4_sel(dslots, Din, ws + y.dsp), Dp, BK, d, Dp, nullptr, 0, nullptr, 0, st));
        RC(pad4_unpad(ws + y.dsp, Din, dslots, BK, st));
    }
    return 0;
}

}  // extern "C"
