// C ABI of the masked autoencoder (include/ocrl_hip.h: ocrl_mae_*): ocrs/mae/models_mae.py (MaskedAutoencoderViT) with timm's
// PatchEmbed (Conv2d(3, D, kernel = stride = patch), flattened row-major over the patch grid) and Block
// (x += proj(attn(norm1(x))); x += fc2(GELU(fc1(norm2(x)))); qkv one Linear(D, 3 D) read [B, N, 3, h, hd]).
//   patches   mae_patch_gather: the rows of the patch-embedding GEMM, for all L patches (full = 0) or only the len_keep kept ones (full =
//             1: the embedding is per patch, so gathering first equals "embed all, then gather" at len_keep / L of the GEMM)
//   tokens    cls + pos[0] | embed + pos[1 + id]
//   block     mae_ln, GEMM (qkv), pool_flash attention (no dropout), GEMM (proj, + residual), mae_ln, GEMM (fc1), mae_gelu, GEMM (fc2, +
//             residual); every intermediate stays in ws for the backward
//   decoder   GEMM (decoder_embed), mae_unshuffle (+ mask token, + decoder_pos_embed), blocks, mae_ln, decoder_pred as one GEMM batched over
//             the images whose A operand starts at row 1 of each image (the CLS row is dropped by the pointer offset), mae_loss
// The backward's d pred buffer is [B, L + 1, P] with a zero CLS row, so decoder_pred's two gradient GEMMs run over all B (L + 1) rows.
// Stateless: the caller owns the parameters (torch layout, state_dict order), the gradients and the workspace.  Sums run in orders
// fixed by the shapes (no atomics).
#include "../../include/ocrl_hip.h"
#include "unit_base.h"

namespace {
constexpr size_t SK_FLOATS = (size_t)1 << 25;      // split-k scratch of the weight gradients (fc1 / fc2 of ViT-large: 4 M floats a slab)
constexpr float LN_EPS = 1e-6f;

struct Dims { int B, S, p, D, depth, h, Dd, ddepth, dh, keep, full, G, L, P; };

// one ViT block's saved tensors (float offsets into ws)
struct BlockLay { size_t xn1, mr1, qkv, o, lse, x1, xn2, mr2, hpre, act; };
struct StackLay {
    int N = 0, d = 0, h = 0, depth = 0;
    long long R = 0;
    size_t x[OCRL_MAE_MAX_DEPTH + 1] = {};         // x[i] = input of block i; x[depth] = the stack's output
    BlockLay b[OCRL_MAE_MAX_DEPTH];
};
struct MaeLay {
    StackLay enc, dec;
    size_t restore = 0, keep = 0, mask = 0, patches = 0, emb = 0, lat = 0, mrn = 0, e = 0, xdn = 0, mrd = 0, pred = 0, lpart = 0;
    size_t g[3] = {}, dhid = 0, dqkv = 0, Dd = 0, lnpart = 0, dpred = 0, de = 0, glat = 0, mtpart = 0, sk = 0;
    size_t total = 0;
    // parameter indices in state_dict order (weight; the bias follows)
    int depth = 0, ddepth = 0;
    int blk(int i) const { return 6 + 12 * i; }
    int norm() const { return 6 + 12 * depth; }
    int dembed() const { return norm() + 2; }
    int dblk(int i) const { return norm() + 4 + 12 * i; }
    int dnorm() const { return norm() + 4 + 12 * ddepth; }
    int dpred_() const { return dnorm() + 2; }
};

bool head_ok(int d, int h) { return h >= 1 && d % h == 0 && (d / h == 16 || d / h == 32 || d / h == 48 || d / h == 64); }

int check_mae(const Dims& m) {
    OCRL_REQUIRE(m.B >= 1, "mae: batch >= 1 (got %d)", m.B);
    OCRL_REQUIRE(m.p >= 1 && m.S >= m.p && m.S % m.p == 0, "mae: obs_size must be a multiple of the patch size (got %d / %d)", m.S, m.p);
    OCRL_REQUIRE(m.L <= MAE_MAX_PATCHES, "mae: at most %d patches (got %d)", MAE_MAX_PATCHES, m.L);
    OCRL_REQUIRE(m.P % 4 == 0, "mae: 3 patch^2 must be a multiple of 4 (the GEMM's operand rule; patch %d)", m.p);
    OCRL_REQUIRE(m.D >= 4 && m.D % 4 == 0 && m.Dd >= 4 && m.Dd % 4 == 0, "mae: widths must be multiples of 4 (got %d, %d)", m.D, m.Dd);
    OCRL_REQUIRE(head_ok(m.D, m.h), "mae: encoder head size must be 16, 32, 48 or 64 (got %d / %d)", m.D, m.h);
    OCRL_REQUIRE(head_ok(m.Dd, m.dh), "mae: decoder head size must be 16, 32, 48 or 64 (got %d / %d)", m.Dd, m.dh);
    OCRL_REQUIRE(m.depth >= 1 && m.depth <= OCRL_MAE_MAX_DEPTH && m.ddepth >= 1 && m.ddepth <= OCRL_MAE_MAX_DEPTH,
                 "mae: 1 <= depth <= %d (got %d, %d)", OCRL_MAE_MAX_DEPTH, m.depth, m.ddepth);
    if (m.full) OCRL_REQUIRE(m.keep >= 1 && m.keep <= m.L, "mae: len_keep must be 1 .. %d (got %d)", m.L, m.keep);
    const long long rows = (long long)m.B * (m.L + 1);
    OCRL_REQUIRE(rows * 4 * (m.D > m.Dd ? m.D : m.Dd) < (1LL << 31) && (long long)m.B * 3 * m.S * m.S < (1LL << 31),
                 "mae: batch %d of %d x %d images exceeds the int32 range of one call", m.B, m.S, m.S);
    return 0;
}

Dims dims_of(int B, int S, int p, int D, int depth, int h, int Dd, int ddepth, int dh, int keep, int full) {
    Dims m{B, S, p, D, depth, h, Dd, ddepth, dh, keep, full, 0, 0, 0};
    if (p >= 1 && S >= p) { m.G = S / p; m.L = m.G * m.G; m.P = 3 * p * p; }
    return m;
}

void stack_layout(StackLay& s, WsTake& take, int B, int N, int d, int h, int depth) {
    s.N = N; s.d = d; s.h = h; s.depth = depth; s.R = (long long)B * N;
    const size_t R = (size_t)s.R;
    for (int i = 0; i <= depth; ++i) s.x[i] = take(R * d);
    for (int i = 0; i < depth; ++i) {
        BlockLay& b = s.b[i];
        b.xn1 = take(R * d); b.mr1 = take(2 * R); b.qkv = take(R * 3 * d); b.o = take(R * d); b.lse = take((size_t)B * h * N);
        b.x1 = take(R * d); b.xn2 = take(R * d); b.mr2 = take(2 * R); b.hpre = take(R * 4 * d); b.act = take(R * 4 * d);
    }
}

MaeLay mae_layout(const Dims& m) {
    MaeLay y;
    WsTake take;
    y.depth = m.depth; y.ddepth = m.ddepth;
    const int n = m.full ? m.keep : m.L;               // patches per image through the encoder
    const size_t B = m.B, Re = B * (n + 1), Rd = B * (m.L + 1);
    if (m.full) { y.restore = take(B * m.L); y.keep = take(B * m.keep); y.mask = take(B * m.L); }
    y.patches = take(B * n * m.P); y.emb = take(B * n * m.D);
    stack_layout(y.enc, take, m.B, n + 1, m.D, m.h, m.depth);
    y.lat = take(Re * m.D); y.mrn = take(2 * Re);
    size_t gmax = Re * m.D, wmax = m.D, hmax = (size_t)B * m.h * (n + 1), rmax = Re;
    if (m.full) {
        y.e = take(Re * m.Dd);
        stack_layout(y.dec, take, m.B, m.L + 1, m.Dd, m.dh, m.ddepth);
        y.xdn = take(Rd * m.Dd); y.mrd = take(2 * Rd); y.pred = take(B * m.L * m.P); y.lpart = take(B * m.L);
        y.dpred = take(Rd * m.P); y.de = take(Re * m.Dd); y.glat = take(Re * m.D); y.mtpart = take(B * m.Dd);
        if (Rd * m.Dd > gmax) gmax = Rd * m.Dd;
        if ((size_t)m.Dd > wmax) wmax = m.Dd;
        if ((size_t)B * m.dh * (m.L + 1) > hmax) hmax = (size_t)B * m.dh * (m.L + 1);
        rmax = Rd;
    }
    for (int i = 0; i < 3; ++i) y.g[i] = take(gmax);
    y.dhid = take(4 * gmax); y.dqkv = take(3 * gmax); y.Dd = take(hmax);
    y.lnpart = take((size_t)mae_ln_chunks((long long)rmax) * 2 * wmax + 2 * wmax);
    y.sk = take(SK_FLOATS);
    y.total = take.end;
    return y;
}

int block_fwd(const StackLay& s, int i, const float* const* q, float* ws, int B, hipStream_t st) {
    const BlockLay& b = s.b[i];
    const long long R = s.R;
    const int d = s.d;
    const float* x = ws + s.x[i];
    RC(mae_ln_fwd_launch(x, q[0], q[1], ws + b.xn1, ws + b.mr1, ws + b.mr1 + R, R, d, LN_EPS, st));
    RC(lin_fwd(ws + b.xn1, d, q[2], q[3], ws + b.qkv, 3 * d, R, 3 * d, d, 0, nullptr, 0, st));
    RC(pool_flash_launch(ws + b.qkv, ws + b.o, ws + b.lse, nullptr, nullptr, nullptr, B, s.N, d, s.h, 0.f, 0, 0, 0, st));
    RC(lin_fwd(ws + b.o, d, q[4], q[5], ws + b.x1, d, R, d, d, 0, x, d, st));
    RC(mae_ln_fwd_launch(ws + b.x1, q[6], q[7], ws + b.xn2, ws + b.mr2, ws + b.mr2 + R, R, d, LN_EPS, st));
    RC(lin_fwd(ws + b.xn2, d, q[8], q[9], ws + b.hpre, 4 * d, R, 4 * d, d, 0, nullptr, 0, st));
    RC(mae_gelu_fwd_launch(ws + b.hpre, ws + b.act, R * 4 * d, st));
    return lin_fwd(ws + b.act, 4 * d, q[10], q[11], ws + s.x[i + 1], d, R, d, 4 * d, 0, ws + b.x1, d, st);
}

// g0 = d (block output) -> g0 = d (block input); g1, g2 scratch of the same size
int block_bwd(const StackLay& s, int i, const float* const* q, float* const* g, float* g0, float* g1, float* g2, const MaeLay& y, float* ws, int B,
              hipStream_t st) {
    const BlockLay& b = s.b[i];
    const long long R = s.R;
    const int d = s.d;
    float *dhid = ws + y.dhid, *dqkv = ws + y.dqkv, *sk = ws + y.sk, *lnp = ws + y.lnpart;
    RC(lin_bwd_w(g0, d, ws + b.act, 4 * d, g[10], g[11], R, d, 4 * d, 1.f, sk, SK_FLOATS, st));
    RC(lin_bwd_x(g0, d, q[10], dhid, 4 * d, R, d, 4 * d, nullptr, 0, nullptr, 0, st));
    RC(mae_gelu_bwd_launch(dhid, ws + b.hpre, dhid, R * 4 * d, st));
    RC(lin_bwd_w(dhid, 4 * d, ws + b.xn2, d, g[8], g[9], R, 4 * d, d, 1.f, sk, SK_FLOATS, st));
    RC(lin_bwd_x(dhid, 4 * d, q[8], g1, d, R, 4 * d, d, nullptr, 0, nullptr, 0, st));
    RC(mae_ln_bwd_launch(g1, ws + b.x1, ws + b.mr2, ws + b.mr2 + R, q[6], g0, g2, g[6], g[7], lnp, R, d, st));       // g2 = d x1
    RC(lin_bwd_w(g2, d, ws + b.o, d, g[4], g[5], R, d, d, 1.f, sk, SK_FLOATS, st));
    RC(lin_bwd_x(g2, d, q[4], g1, d, R, d, d, nullptr, 0, nullptr, 0, st));                                            // g1 = d o
    RC(pool_flash_launch(ws + b.qkv, ws + b.o, ws + b.lse, g1, ws + y.Dd, dqkv, B, s.N, d, s.h, 0.f, 0, 0, 1, st));
    RC(lin_bwd_w(dqkv, 3 * d, ws + b.xn1, d, g[2], g[3], R, 3 * d, d, 1.f, sk, SK_FLOATS, st));
    RC(lin_bwd_x(dqkv, 3 * d, q[2], g1, d, R, 3 * d, d, nullptr, 0, nullptr, 0, st));
    return mae_ln_bwd_launch(g1, ws + s.x[i], ws + b.mr1, ws + b.mr1 + R, q[0], g2, g0, g[0], g[1], lnp, R, d, st);
}

int zero_decoder_grads(float* const* dw, const Dims& m, const MaeLay& y, hipStream_t st) {
    const long long Dd = m.Dd;
    RC(fill_launch(dw[2], Dd, 0.f, st));
    RC(fill_launch(dw[y.dembed()], Dd * m.D, 0.f, st));
    RC(fill_launch(dw[y.dembed() + 1], Dd, 0.f, st));
    static const int wr[6] = {1, 3, 1, 1, 4, 1}, wc[6] = {0, 1, 1, 0, 1, 4};      // rows / columns of each weight in units of Dd (0: a vector)
    for (int i = 0; i < m.ddepth; ++i)
        for (int j = 0; j < 6; ++j) {
            RC(fill_launch(dw[y.dblk(i) + 2 * j], wr[j] * Dd * (wc[j] ? wc[j] * Dd : 1), 0.f, st));
            RC(fill_launch(dw[y.dblk(i) + 2 * j + 1], wr[j] * Dd, 0.f, st));
        }
    RC(fill_launch(dw[y.dnorm()], Dd, 0.f, st));
    RC(fill_launch(dw[y.dnorm() + 1], Dd, 0.f, st));
    RC(fill_launch(dw[y.dpred_()], (long long)m.P * Dd, 0.f, st));
    return fill_launch(dw[y.dpred_() + 1], m.P, 0.f, st);
}
}  // namespace

extern "C" {

size_t ocrl_mae_ws_floats(int B, int obs_size, int patch, int D, int depth, int heads, int Dd, int ddepth, int dheads, int len_keep, int full) {
    const Dims m = dims_of(B, obs_size, patch, D, depth, heads, Dd, ddepth, dheads, len_keep, full);
    if (check_mae(m)) return 0;                        // the shapes fwd / bwd reject get no workspace
    return mae_layout(m).total;
}

int ocrl_mae_rank(const float* noise, int* ids_restore, int* ids_keep, float* mask, int B, int L, int len_keep, void* stream) {
    OCRL_REQUIRE(noise && ids_restore && ids_keep && mask, "ocrl_mae_rank: null argument");
    return mae_rank_launch(noise, ids_restore, ids_keep, mask, nullptr, nullptr, B, L, len_keep, static_cast<hipStream_t>(stream));
}

int ocrl_mae_fwd(const float* obs, const float* const* w, const float* noise, float* rep, float* metrics, float* pred, float* mask,
                 int* ids_restore, int B, int obs_size, int patch, int D, int depth, int heads, int Dd, int ddepth, int dheads, int len_keep,
                 int full, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(obs && w && ws && (full ? (noise && metrics) : rep != nullptr), "ocrl_mae_fwd: null argument");
    const Dims m = dims_of(B, obs_size, patch, D, depth, heads, Dd, ddepth, dheads, len_keep, full);
    RC(check_mae(m));
    const MaeLay y = mae_layout(m);
    RC(ws_check("ocrl_mae_fwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = full ? len_keep : m.L, L = m.L, P = m.P;
    const int* keep = nullptr;
    if (full) {
        RC(mae_rank_launch(noise, reinterpret_cast<int*>(ws + y.restore), reinterpret_cast<int*>(ws + y.keep), ws + y.mask, ids_restore, mask, B, L,
                           len_keep, st));
        keep = reinterpret_cast<const int*>(ws + y.keep);
    }
    RC(mae_patch_gather_launch(obs, keep, ws + y.patches, B, n, m.S, m.p, st));
    RC(lin_fwd(ws + y.patches, P, w[4], w[5], ws + y.emb, D, (long long)B * n, D, P, 0, nullptr, 0, st));
    RC(mae_tokens_fwd_launch(ws + y.emb, w[0], w[1], keep, ws + y.enc.x[0], B, n, D, st));
    for (int i = 0; i < depth; ++i) RC(block_fwd(y.enc, i, w + y.blk(i), ws, B, st));
    const long long Re = y.enc.R;
    float* lat = full ? ws + y.lat : rep;
    RC(mae_ln_fwd_launch(ws + y.enc.x[depth], w[y.norm()], w[y.norm() + 1], lat, ws + y.mrn, ws + y.mrn + Re, Re, D, LN_EPS, st));
    if (!full) return 0;
    if (rep) RC(copy_launch(lat, rep, Re * D, st));
    RC(lin_fwd(lat, D, w[y.dembed()], w[y.dembed() + 1], ws + y.e, Dd, Re, Dd, D, 0, nullptr, 0, st));
    RC(mae_unshuffle_fwd_launch(ws + y.e, w[2], w[3], reinterpret_cast<const int*>(ws + y.restore), ws + y.dec.x[0], B, L, len_keep, Dd, st));
    for (int i = 0; i < ddepth; ++i) RC(block_fwd(y.dec, i, w + y.dblk(i), ws, B, st));
    const long long Rd = y.dec.R;
    RC(mae_ln_fwd_launch(ws + y.dec.x[ddepth], w[y.dnorm()], w[y.dnorm() + 1], ws + y.xdn, ws + y.mrd, ws + y.mrd + Rd, Rd, Dd, LN_EPS, st));
    // decoder_pred over rows 1 .. L of every image: one product per image, A starting past the CLS row
    float* pr = ws + y.pred;
    GemmArgs a;
    a.A = ws + y.xdn + Dd; a.B = w[y.dpred_()]; a.C = pr; a.M = L; a.N = P; a.K = Dd; a.lda = Dd; a.ldb = Dd; a.ldc = P; a.akc = 1; a.bkc = 1;
    a.bias = w[y.dpred_() + 1]; a.batch = B; a.sA = (long long)(L + 1) * Dd; a.sC = (long long)L * P;
    RC(gemm_launch(a, st));
    if (pred) RC(copy_launch(pr, pred, (long long)B * L * P, st));
    return mae_loss_launch(pr, obs, ws + y.mask, nullptr, ws + y.lpart, metrics, nullptr, B, L, len_keep, m.S, m.p, st);
}

int ocrl_mae_bwd(const float* obs, const float* const* w, const float* dloss, const float* drep, float* const* dw, int B, int obs_size,
                 int patch, int D, int depth, int heads, int Dd, int ddepth, int dheads, int len_keep, int full, float* ws, size_t ws_floats,
                 void* stream) {
    OCRL_REQUIRE(obs && w && dw && ws && (full ? (dloss || drep) : drep != nullptr), "ocrl_mae_bwd: null argument");
    const Dims m = dims_of(B, obs_size, patch, D, depth, heads, Dd, ddepth, dheads, len_keep, full);
    RC(check_mae(m));
    const MaeLay y = mae_layout(m);
    RC(ws_check("ocrl_mae_bwd", ws_floats, y.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = full ? len_keep : m.L, L = m.L, P = m.P;
    const long long Re = y.enc.R;
    float *g0 = ws + y.g[0], *g1 = ws + y.g[1], *g2 = ws + y.g[2], *sk = ws + y.sk, *lnp = ws + y.lnpart;
    const float* glat = drep;                          // d latent
    if (full && dloss) {
        const long long Rd = y.dec.R;
        RC(mae_loss_launch(ws + y.pred, obs, ws + y.mask, dloss, nullptr, nullptr, ws + y.dpred, B, L, len_keep, m.S, m.p, st));
        RC(lin_bwd_w(ws + y.dpred, P, ws + y.xdn, Dd, dw[y.dpred_()], dw[y.dpred_() + 1], Rd, P, Dd, 1.f, sk, SK_FLOATS, st));
        RC(lin_bwd_x(ws + y.dpred, P, w[y.dpred_()], g1, Dd, Rd, P, Dd, nullptr, 0, nullptr, 0, st));
        RC(mae_ln_bwd_launch(g1, ws + y.dec.x[ddepth], ws + y.mrd, ws + y.mrd + Rd, w[y.dnorm()], nullptr, g0, dw[y.dnorm()], dw[y.dnorm() + 1], lnp,
                             Rd, Dd, st));
        for (int i = ddepth - 1; i >= 0; --i) RC(block_bwd(y.dec, i, w + y.dblk(i), dw + y.dblk(i), g0, g1, g2, y, ws, B, st));
        RC(mae_unshuffle_bwd_launch(g0, reinterpret_cast<const int*>(ws + y.keep), ws + y.mask, ws + y.de, dw[2], ws + y.mtpart, B, L, len_keep, Dd,
                                    st));
        RC(lin_bwd_w(ws + y.de, Dd, ws + y.lat, D, dw[y.dembed()], dw[y.dembed() + 1], Re, Dd, D, 1.f, sk, SK_FLOATS, st));
        RC(lin_bwd_x(ws + y.de, Dd, w[y.dembed()], ws + y.glat, D, Re, Dd, D, nullptr, 0, drep, D, st));            // + d rep
        glat = ws + y.glat;
    } else if (full) {
        RC(zero_decoder_grads(dw, m, y, st));
    }
    const float* lat_in = ws + y.enc.x[depth];
    RC(mae_ln_bwd_launch(glat, lat_in, ws + y.mrn, ws + y.mrn + Re, w[y.norm()], nullptr, g0, dw[y.norm()], dw[y.norm() + 1], lnp, Re, D, st));
    for (int i = depth - 1; i >= 0; --i) RC(block_bwd(y.enc, i, w + y.blk(i), dw + y.blk(i), g0, g1, g2, y, ws, B, st));
    // x0 = [cls + pos[0]; embed + pos]: d embed rows, d cls summed over the images
    float* demb = g1;
    RC(mae_tokens_bwd_launch(g0, demb, dw[0], B, n, D, st));
    return lin_bwd_w(demb, D, ws + y.patches, P, dw[4], dw[5], (long long)B * n, D, P, 1.f, sk, SK_FLOATS, st);
}

}  // extern "C"
