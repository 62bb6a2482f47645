// C ABI of the pooling-Transformer and masked-autoencoder kernels, one launcher of pool.hip, pool_long.hip and mae.hip per entry
// (include/ocrl_hip_vit_kernels.h: ocrl_vit_*).  Stateless: the caller owns every tensor and the scratch.  Most of these launchers check
// little themselves (the model that calls them has already fixed the shapes), so each entry refuses, before any launch, what the kernel
// behind it cannot handle: null pointers, sizes below 1, misaligned float4 operands and every shape limit the kernel assumes.  The
// arithmetic is that of the three kernel files, untouched.
#include "../../include/ocrl_hip_vit_kernels.h"
#include "common.h"
#include "kernels.h"

namespace {
constexpr long long MAX_ELEMS = 0x7fffffffLL;          // elements of one tensor (int indices inside some kernels)
constexpr int MAX_GRID_Y = 65535;                      // images (or image-heads) a two-dimensional launch takes

int check_prob(const char* who, float p) {
    OCRL_REQUIRE(p >= 0.f && p < 1.f, "%s: 0 <= p < 1 (got %g)", who, (double)p);
    return 0;
}
// [B][K + 1][d] rows of the short path's row kernels
int check_rows(const char* who, int B, int K, int d) {
    OCRL_REQUIRE(B >= 1 && K >= 1 && d >= 4, "%s: B, K >= 1 and d >= 4 (got %d, %d, %d)", who, B, K, d);
    OCRL_REQUIRE(d % 4 == 0, "%s: d %% 4 == 0 (got %d)", who, d);
    OCRL_REQUIRE((long long)B * (K + 1LL) * d <= MAX_ELEMS, "%s: B (K + 1) d < 2^31", who);
    return 0;
}
int check_attn(const char* who, int B, int S, int d, int h, float p) {
    OCRL_REQUIRE(B >= 1 && S >= 1 && d >= 1 && h >= 1, "%s: B, S, d, h >= 1 (got %d, %d, %d, %d)", who, B, S, d, h);
    RC(check_prob(who, p));
    return 0;
}
int check_flash(const char* who, int B, int S, int d, int h, float p) {
    RC(check_attn(who, B, S, d, h, p));
    OCRL_REQUIRE(d % h == 0 && (d / h == 16 || d / h == 32 || d / h == 48 || d / h == 64),
                 "%s: head size d / h must be 16, 32, 48 or 64 (got %d / %d)", who, d, h);
    OCRL_REQUIRE((long long)B * h <= MAX_GRID_Y, "%s: B h <= %d (got %lld)", who, MAX_GRID_Y, (long long)B * h);
    OCRL_REQUIRE((long long)B * S * 3 * d <= MAX_ELEMS, "%s: 3 B S d < 2^31", who);
    return 0;
}
int check_cls(const char* who, int B, int S, int d, int h) {
    OCRL_REQUIRE(B >= 1 && S >= 1 && d >= 1 && h >= 1, "%s: B, S, d, h >= 1 (got %d, %d, %d, %d)", who, B, S, d, h);
    OCRL_REQUIRE(d % 4 == 0 && d <= 256 && h <= 16 && (long long)h * d <= 4096 && d % h == 0,
                 "%s: d %% 4 == 0, d <= 256, h <= 16, h d <= 4096 and d %% h == 0 (got d %d, h %d)", who, d, h);
    OCRL_REQUIRE(B <= MAX_GRID_Y, "%s: B <= %d (got %d)", who, MAX_GRID_Y, B);
    OCRL_REQUIRE((long long)B * S * d <= MAX_ELEMS, "%s: B S d < 2^31", who);
    return 0;
}
size_t cls_part_floats(int B, int S, int d, int h, int backward) {
    return (size_t)B * pool_cls_nchunk(B, S, nullptr) * h * (backward ? d : d + 4);
}
// the patch grid of an S x S image: L = (S / p)^2 patches of 3 p p values
int check_patches(const char* who, int B, int S, int p) {
    OCRL_REQUIRE(B >= 1 && S >= 1 && p >= 1, "%s: B, S, p >= 1 (got %d, %d, %d)", who, B, S, p);
    OCRL_REQUIRE(S % p == 0, "%s: S %% p == 0 (got S %d, p %d)", who, S, p);
    OCRL_REQUIRE((S / p) * (long long)(S / p) <= MAE_MAX_PATCHES, "%s: L = (S / p)^2 <= %d (got %lld)", who, MAE_MAX_PATCHES,
                 (S / p) * (long long)(S / p));
    OCRL_REQUIRE((long long)B * 3 * S * S <= MAX_ELEMS, "%s: 3 B S S < 2^31", who);
    return 0;
}
int check_width(const char* who, int D) {
    OCRL_REQUIRE(D >= 4 && D % 4 == 0, "%s: width %% 4 == 0, >= 4 (got %d)", who, D);
    return 0;
}
int check_keep(const char* who, int B, int L, int len_keep, int D) {
    OCRL_REQUIRE(B >= 1 && B <= MAX_GRID_Y, "%s: 1 <= B <= %d (got %d)", who, MAX_GRID_Y, B);
    OCRL_REQUIRE(L >= 1 && L <= MAE_MAX_PATCHES, "%s: 1 <= L <= %d (got %d)", who, MAE_MAX_PATCHES, L);
    OCRL_REQUIRE(len_keep >= 1 && len_keep <= L, "%s: 1 <= len_keep <= L (got %d of %d)", who, len_keep, L);
    RC(check_width(who, D));
    OCRL_REQUIRE((long long)B * (L + 1LL) * D <= MAX_ELEMS, "%s: B (L + 1) D < 2^31", who);
    return 0;
}
int check_ln(const char* who, long long R, int F) {
    OCRL_REQUIRE(R >= 1, "%s: R >= 1 (got %lld)", who, R);
    RC(check_width(who, F));
    OCRL_REQUIRE(R * F <= MAX_ELEMS, "%s: R F < 2^31", who);
    return 0;
}
hipStream_t S_(void* stream) { return static_cast<hipStream_t>(stream); }
}  // namespace

extern "C" {

// ---------------------------------------------------------------- short path (pool.hip)
int ocrl_vit_pool_embed(const float* lin, const float* cls, const float* pos, float* x0, int B, int K, int d, void* stream) {
    RC(check_rows("ocrl_vit_pool_embed", B, K, d));
    OCRL_REQUIRE(lin && cls && x0, "ocrl_vit_pool_embed: null argument (lin, cls or x0)");
    OCRL_REQUIRE(aligned16(lin, cls, pos, x0), "ocrl_vit_pool_embed: lin, cls, pos and x0 must be 16-byte aligned");
    return pool_embed_launch(lin, cls, pos, x0, B, K, d, S_(stream));
}

int ocrl_vit_pool_rows(const float* in, float* out, int B, int K, int d, int mode, void* stream) {
    RC(check_rows("ocrl_vit_pool_rows", B, K, d));
    OCRL_REQUIRE(mode >= 0 && mode <= 2, "ocrl_vit_pool_rows: mode must be 0, 1 or 2 (got %d)", mode);
    OCRL_REQUIRE(in && out, "ocrl_vit_pool_rows: null argument");
    OCRL_REQUIRE(aligned16(in, out), "ocrl_vit_pool_rows: in and out must be 16-byte aligned");
    return pool_rows_launch(in, out, B, K, d, mode, S_(stream));
}

int ocrl_vit_pool_attn_fwd(const float* qkv, float* P, float* O, int B, int S, int d, int h, float p, unsigned long long seed, unsigned site,
                           void* stream) {
    RC(check_attn("ocrl_vit_pool_attn_fwd", B, S, d, h, p));
    RC(pool_attn_check(B, S, d, h, 0));
    OCRL_REQUIRE(qkv && P && O, "ocrl_vit_pool_attn_fwd: null argument");
    OCRL_REQUIRE(aligned16(qkv, O), "ocrl_vit_pool_attn_fwd: qkv and O must be 16-byte aligned");
    return pool_attn_launch(qkv, P, O, nullptr, nullptr, B, S, d, h, p, seed, site, 0, S_(stream));
}

int ocrl_vit_pool_attn_bwd(const float* qkv, const float* P, const float* dO, float* dqkv, int B, int S, int d, int h, float p,
                           unsigned long long seed, unsigned site, void* stream) {
    RC(check_attn("ocrl_vit_pool_attn_bwd", B, S, d, h, p));
    RC(pool_attn_check(B, S, d, h, 1));
    OCRL_REQUIRE(qkv && P && dO && dqkv, "ocrl_vit_pool_attn_bwd: null argument");
    OCRL_REQUIRE(aligned16(qkv, dO, dqkv), "ocrl_vit_pool_attn_bwd: qkv, dO and dqkv must be 16-byte aligned");
    return pool_attn_launch(qkv, const_cast<float*>(P), nullptr, dO, dqkv, B, S, d, h, p, seed, site, 1, S_(stream));
}

int ocrl_vit_pool_short_ok(int K, int Din, int d, int h) { return pool_short_check(K, Din, d, h) == 0; }

// ---------------------------------------------------------------- long path (pool_long.hip)
int ocrl_vit_pool_cols(const float* src, int lds, float* dst, int ldd, long long rows, int ncols, int ncopy, void* stream) {
    OCRL_REQUIRE(src && dst, "ocrl_vit_pool_cols: null argument");
    OCRL_REQUIRE(rows >= 1 && ncols >= 1 && ncopy >= 1, "ocrl_vit_pool_cols: rows, ncols, ncopy >= 1 (got %lld, %d, %d)", rows, ncols, ncopy);
    OCRL_REQUIRE(ncopy <= ncols && lds >= ncopy && ldd >= ncols, "ocrl_vit_pool_cols: ncopy <= ncols, lds >= ncopy and ldd >= ncols (got ncopy %d, ncols %d, lds %d, ldd %d)",
                 ncopy, ncols, lds, ldd);
    OCRL_REQUIRE(rows * (long long)(lds > ldd ? lds : ldd) <= MAX_ELEMS, "ocrl_vit_pool_cols: rows * ld < 2^31");
    return pool_cols_launch(src, lds, dst, ldd, rows, ncols, ncopy, S_(stream));
}

int ocrl_vit_cls_drop(const float* x, const float* resid, int ldr, float* out, int B, int N, int S, float p, unsigned long long seed,
                      unsigned site, void* stream) {
    OCRL_REQUIRE(x && out, "ocrl_vit_cls_drop: null argument (x or out)");
    OCRL_REQUIRE(B >= 1 && N >= 1 && S >= 1, "ocrl_vit_cls_drop: B, N, S >= 1 (got %d, %d, %d)", B, N, S);
    OCRL_REQUIRE(!resid || ldr >= N, "ocrl_vit_cls_drop: ldr >= N with a residual (got ldr %d, N %d)", ldr, N);
    OCRL_REQUIRE((long long)B * (resid && ldr > N ? ldr : N) <= MAX_ELEMS, "ocrl_vit_cls_drop: B * ld < 2^31");
    RC(check_prob("ocrl_vit_cls_drop", p));
    return pool_cls_drop_launch(x, resid, ldr, out, B, N, S, p, seed, site, S_(stream));
}

int ocrl_vit_cls_add(float* dX, const float* v, int B, int d, int S, void* stream) {
    OCRL_REQUIRE(dX && v, "ocrl_vit_cls_add: null argument");
    OCRL_REQUIRE(B >= 1 && d >= 1 && S >= 1, "ocrl_vit_cls_add: B, d, S >= 1 (got %d, %d, %d)", B, d, S);
    OCRL_REQUIRE((long long)B * S * d <= MAX_ELEMS, "ocrl_vit_cls_add: B S d < 2^31");
    return pool_cls_add_launch(dX, v, B, d, S, S_(stream));
}

int ocrl_vit_flash_fwd(const float* qkv, float* O, float* lse, int B, int S, int d, int h, float p, unsigned long long seed, unsigned site,
                       void* stream) {
    RC(check_flash("ocrl_vit_flash_fwd", B, S, d, h, p));
    OCRL_REQUIRE(qkv && O && lse, "ocrl_vit_flash_fwd: null argument");
    OCRL_REQUIRE(aligned16(qkv, O), "ocrl_vit_flash_fwd: qkv and O must be 16-byte aligned");
    return pool_flash_launch(qkv, O, lse, nullptr, nullptr, nullptr, B, S, d, h, p, seed, site, 0, S_(stream));
}

int ocrl_vit_flash_bwd(const float* qkv, const float* O, const float* lse, const float* dO, float* Dd, float* dqkv, int B, int S, int d, int h,
                       float p, unsigned long long seed, unsigned site, void* stream) {
    RC(check_flash("ocrl_vit_flash_bwd", B, S, d, h, p));
    OCRL_REQUIRE(qkv && O && lse && dO && Dd && dqkv, "ocrl_vit_flash_bwd: null argument");
    OCRL_REQUIRE(aligned16(qkv, dO, dqkv), "ocrl_vit_flash_bwd: qkv, dO and dqkv must be 16-byte aligned");
    return pool_flash_launch(qkv, const_cast<float*>(O), const_cast<float*>(lse), dO, Dd, dqkv, B, S, d, h, p, seed, site, 1, S_(stream));
}

int ocrl_vit_cls_nchunk(int B, int S, int* chunk) {
    if (B < 1 || S < 1) {
        if (chunk) *chunk = 0;
        return 0;
    }
    return pool_cls_nchunk(B, S, chunk);
}

size_t ocrl_vit_cls_part_floats(int B, int S, int d, int h, int backward) {
    if (check_cls("ocrl_vit_cls_part_floats", B, S, d, h)) return 0;
    return cls_part_floats(B, S, d, h, backward);
}

int ocrl_vit_cls_attn_fwd(const float* X, const float* Win, const float* bin, const float* q, float* U, float* z, float* stat, float* o,
                          float* part, size_t part_floats, int B, int S, int d, int h, float p, unsigned long long seed, unsigned site,
                          void* stream) {
    RC(check_cls("ocrl_vit_cls_attn_fwd", B, S, d, h));
    RC(check_prob("ocrl_vit_cls_attn_fwd", p));
    OCRL_REQUIRE(X && Win && bin && q && U && z && stat && o && part, "ocrl_vit_cls_attn_fwd: null argument");
    OCRL_REQUIRE(aligned16(X, part), "ocrl_vit_cls_attn_fwd: X and part must be 16-byte aligned");
    const size_t need = cls_part_floats(B, S, d, h, 0);
    OCRL_REQUIRE(part_floats >= need, "ocrl_vit_cls_attn_fwd: part too small (%zu < %zu floats)", part_floats, need);
    PoolClsArgs c;
    c.X = X; c.Win = Win; c.bin = bin; c.q = q; c.U = U; c.part = part; c.z = z; c.stat = stat; c.o = o;
    c.B = B; c.S = S; c.d = d; c.h = h; c.p = p; c.seed = seed; c.site = site;
    return pool_cls_attn_fwd_launch(c, S_(stream));
}

int ocrl_vit_cls_attn_bwd(const float* X, const float* Win, const float* bin, const float* q, const float* U, const float* z, const float* stat,
                          const float* dO, const float* x0, float* G, float* gD, float* dX, float* w, float* dq, float* dW, float* db,
                          float* part, size_t part_floats, int B, int S, int d, int h, float p, unsigned long long seed, unsigned site,
                          void* stream) {
    RC(check_cls("ocrl_vit_cls_attn_bwd", B, S, d, h));
    RC(check_prob("ocrl_vit_cls_attn_bwd", p));
    OCRL_REQUIRE(X && Win && bin && q && U && z && stat && dO && x0 && G && gD && dX && w && dq && dW && db && part,
                 "ocrl_vit_cls_attn_bwd: null argument");
    OCRL_REQUIRE(aligned16(X, dX, part), "ocrl_vit_cls_attn_bwd: X, dX and part must be 16-byte aligned");
    const size_t need = cls_part_floats(B, S, d, h, 1);
    OCRL_REQUIRE(part_floats >= need, "ocrl_vit_cls_attn_bwd: part too small (%zu < %zu floats)", part_floats, need);
    PoolClsArgs c;
    c.X = X; c.Win = Win; c.bin = bin; c.q = q; c.U = const_cast<float*>(U); c.part = part; c.z = const_cast<float*>(z);
    c.stat = const_cast<float*>(stat); c.dO = dO; c.G = G; c.gD = gD; c.dX = dX; c.w = w; c.dq = dq; c.x0 = x0; c.dW = dW; c.db = db;
    c.B = B; c.S = S; c.d = d; c.h = h; c.p = p; c.seed = seed; c.site = site;
    return pool_cls_attn_bwd_launch(c, S_(stream));
}

// ---------------------------------------------------------------- masked autoencoder (mae.hip)
int ocrl_vit_patch_gather(const float* obs, const int* ids, float* out, int B, int n, int S, int p, int force_scalar, void* stream) {
    RC(check_patches("ocrl_vit_patch_gather", B, S, p));
    OCRL_REQUIRE(n >= 1 && n <= (S / p) * (S / p), "ocrl_vit_patch_gather: 1 <= n <= L (got %d of %d)", n, (S / p) * (S / p));
    OCRL_REQUIRE(obs && out, "ocrl_vit_patch_gather: null argument (obs or out)");
    return mae_patch_gather_launch(obs, ids, out, B, n, S, p, S_(stream), force_scalar ? 1 : 0);
}

int ocrl_vit_tokens_fwd(const float* embed, const float* cls, const float* pos, const int* ids, float* x0, int B, int n, int L, int D,
                        void* stream) {
    RC(check_keep("ocrl_vit_tokens_fwd", B, L, n, D));
    OCRL_REQUIRE(embed && cls && pos && x0, "ocrl_vit_tokens_fwd: null argument (embed, cls, pos or x0)");
    OCRL_REQUIRE(aligned16(embed, cls, pos, x0), "ocrl_vit_tokens_fwd: embed, cls, pos and x0 must be 16-byte aligned");
    return mae_tokens_fwd_launch(embed, cls, pos, ids, x0, B, n, D, S_(stream));
}

int ocrl_vit_tokens_bwd(const float* dx0, float* dembed, float* dcls, int B, int n, int D, void* stream) {
    OCRL_REQUIRE(B >= 1 && n >= 1, "ocrl_vit_tokens_bwd: B, n >= 1 (got %d, %d)", B, n);
    RC(check_width("ocrl_vit_tokens_bwd", D));
    OCRL_REQUIRE((long long)B * (n + 1LL) * D <= MAX_ELEMS, "ocrl_vit_tokens_bwd: B (n + 1) D < 2^31");
    OCRL_REQUIRE(dx0 && dembed && dcls, "ocrl_vit_tokens_bwd: null argument");
    OCRL_REQUIRE(aligned16(dx0, dembed), "ocrl_vit_tokens_bwd: dx0 and dembed must be 16-byte aligned");
    return mae_tokens_bwd_launch(dx0, dembed, dcls, B, n, D, S_(stream));
}

int ocrl_vit_unshuffle_fwd(const float* e, const float* mtok, const float* dpos, const int* restore, float* xd, int B, int L, int len_keep,
                           int D, void* stream) {
    RC(check_keep("ocrl_vit_unshuffle_fwd", B, L, len_keep, D));
    OCRL_REQUIRE(e && mtok && dpos && restore && xd, "ocrl_vit_unshuffle_fwd: null argument");
    OCRL_REQUIRE(aligned16(e, mtok, dpos, xd), "ocrl_vit_unshuffle_fwd: e, mtok, dpos and xd must be 16-byte aligned");
    return mae_unshuffle_fwd_launch(e, mtok, dpos, restore, xd, B, L, len_keep, D, S_(stream));
}

int ocrl_vit_unshuffle_bwd(const float* dxd, const int* keep, const float* mask, float* de, float* dmtok, float* part, int B, int L,
                           int len_keep, int D, void* stream) {
    RC(check_keep("ocrl_vit_unshuffle_bwd", B, L, len_keep, D));
    OCRL_REQUIRE(dxd && keep && mask && de && dmtok && part, "ocrl_vit_unshuffle_bwd: null argument");
    OCRL_REQUIRE(aligned16(dxd, de), "ocrl_vit_unshuffle_bwd: dxd and de must be 16-byte aligned");
    return mae_unshuffle_bwd_launch(dxd, keep, mask, de, dmtok, part, B, L, len_keep, D, S_(stream));
}

int ocrl_vit_gelu_fwd(const float* pre, float* y, long long n, void* stream) {
    OCRL_REQUIRE(pre && y, "ocrl_vit_gelu_fwd: null argument");
    OCRL_REQUIRE(n >= 4 && n % 4 == 0, "ocrl_vit_gelu_fwd: n %% 4 == 0, >= 4 (got %lld)", n);
    OCRL_REQUIRE(aligned16(pre, y), "ocrl_vit_gelu_fwd: pre and y must be 16-byte aligned");
    return mae_gelu_fwd_launch(pre, y, n, S_(stream));
}

int ocrl_vit_gelu_bwd(const float* dy, const float* pre, float* dpre, long long n, void* stream) {
    OCRL_REQUIRE(dy && pre && dpre, "ocrl_vit_gelu_bwd: null argument");
    OCRL_REQUIRE(n >= 4 && n % 4 == 0, "ocrl_vit_gelu_bwd: n %% 4 == 0, >= 4 (got %lld)", n);
    OCRL_REQUIRE(aligned16(dy, pre, dpre), "ocrl_vit_gelu_bwd: dy, pre and dpre must be 16-byte aligned");
    return mae_gelu_bwd_launch(dy, pre, dpre, n, S_(stream));
}

int ocrl_vit_ln_chunks(long long R) { return R < 1 ? 0 : mae_ln_chunks(R); }

int ocrl_vit_ln_fwd(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, long long R, int F, float eps,
                    void* stream) {
    RC(check_ln("ocrl_vit_ln_fwd", R, F));
    OCRL_REQUIRE(eps > 0.f, "ocrl_vit_ln_fwd: eps must be positive (got %g)", (double)eps);
    OCRL_REQUIRE(x && g && b && y && mean && rstd, "ocrl_vit_ln_fwd: null argument");
    OCRL_REQUIRE(aligned16(x, g, b, y), "ocrl_vit_ln_fwd: x, g, b and y must be 16-byte aligned");
    return mae_ln_fwd_launch(x, g, b, y, mean, rstd, R, F, eps, S_(stream));
}

int ocrl_vit_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, const float* resid, float* dx,
                    float* dg, float* db, float* part, size_t part_floats, long long R, int F, void* stream) {
    RC(check_ln("ocrl_vit_ln_bwd", R, F));
    OCRL_REQUIRE(dy && x && mean && rstd && g && dx && dg && db && part, "ocrl_vit_ln_bwd: null argument");
    OCRL_REQUIRE(aligned16(dy, x, g, resid, dx), "ocrl_vit_ln_bwd: dy, x, g, resid and dx must be 16-byte aligned");
    const size_t need = (size_t)2 * F * mae_ln_chunks(R);
    OCRL_REQUIRE(part_floats >= need, "ocrl_vit_ln_bwd: part too small (%zu < %zu floats)", part_floats, need);
    return mae_ln_bwd_launch(dy, x, mean, rstd, g, resid, dx, dg, db, part, R, F, S_(stream));
}

int ocrl_vit_loss(const float* pred, const float* obs, const float* mask, const float* dloss, float* part, float* loss, float* dpred, int B,
                  int L, int len_keep, int S, int p, void* stream) {
    RC(check_patches("ocrl_vit_loss", B, S, p));
    OCRL_REQUIRE(B <= MAX_GRID_Y, "ocrl_vit_loss: B <= %d (got %d)", MAX_GRID_Y, B);
    OCRL_REQUIRE(L == (S / p) * (S / p), "ocrl_vit_loss: L == (S / p)^2 (got L %d, S %d, p %d)", L, S, p);
    OCRL_REQUIRE(len_keep >= 1 && len_keep <= L, "ocrl_vit_loss: 1 <= len_keep <= L (got %d of %d)", len_keep, L);
    OCRL_REQUIRE((long long)B * (L + 1LL) * 3 * p * p <= MAX_ELEMS, "ocrl_vit_loss: 3 B (L + 1) p p < 2^31");
    OCRL_REQUIRE(pred && obs && mask, "ocrl_vit_loss: null argument (pred, obs or mask)");
    OCRL_REQUIRE(loss || dpred, "ocrl_vit_loss: nothing to compute (loss and dpred are both null)");
    OCRL_REQUIRE(!loss || part, "ocrl_vit_loss: loss needs part (B L floats of scratch)");
    OCRL_REQUIRE(!dpred || dloss, "ocrl_vit_loss: dpred needs dloss");
    return mae_loss_launch(pred, obs, mask, dloss, loss ? part : nullptr, loss, dpred, B, L, len_keep, S, p, S_(stream));
}

}  // extern "C"
