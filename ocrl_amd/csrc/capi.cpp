// extern "C" boundary of libocrl_hip.so (see include/ocrl_hip.h).
#include <stdarg.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "../../include/ocrl_hip.h"
#include "iodine_model.h"
#include "slate_model.h"

static thread_local char g_err[512] = "";

void ocrl_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

template <class M>
struct Handle {
    using Model = M;
    M* m = nullptr;
};
struct ocrl_slate : Handle<SlateModel> {};
struct ocrl_iodine : Handle<IodineModel> {};

#define ST(s) static_cast<hipStream_t>(s)
#define GUARD(h) \
    if (!(h) || !(h)->m) { ocrl_set_error("null handle"); return 1; }

// ---- the part of a stateful model's ABI that is the same for every model (ModelBase), over the handle type
template <class H, class C>
static int h_create(const C& k, H** out) {
    H* h = new (std::nothrow) H;
    if (!h) { ocrl_set_error("out of memory"); return 1; }
    h->m = new (std::nothrow) typename H::Model(k);
    if (!h->m) { delete h; ocrl_set_error("out of memory"); return 1; }
    if (!h->m->create_error().empty()) {       // a name the constructor could not resolve
        ocrl_set_error("create: %s", h->m->create_error().c_str());
        delete h->m;
        delete h;
        return 1;
    }
    *out = h;
    return 0;
}
template <class H>
static void h_destroy(H* h) {
    if (!h) return;
    delete h->m;
    delete h;
}
template <class H> static int h_param_count(const H* h) { return (h && h->m) ? (int)h->m->params().size() : -1; }
template <class H>
static int h_param_info(const H* h, int i, char* name, int name_cap, int shape[4], int* ndim, long long* offset, long long* numel, int* group) {
    GUARD(h);
    if (i < 0 || i >= (int)h->m->params().size()) { ocrl_set_error("param index out of range"); return 1; }
    const ParamInfo& p = h->m->params()[i];
    if (name && name_cap > 0) { strncpy(name, p.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
    if (ndim) *ndim = p.ndim;
    if (offset) *offset = p.offset;
    if (numel) *numel = p.numel;
    if (group) *group = p.group;
    return 0;
}
template <class H> static long long h_flat_size(const H* h) { return (h && h->m) ? h->m->flat_size() : -1; }
template <class H> static size_t h_workspace_bytes(const H* h) { return (h && h->m) ? h->m->workspace_bytes() : 0; }
template <class H> static int h_bind(H* h, float* p, float* g, float* m, float* v, void* ws, size_t n) { GUARD(h); return h->m->bind(p, g, m, v, ws, n); }
template <class H> static float* h_metrics(const H* h) { return (h && h->m) ? h->m->metrics() : nullptr; }
template <class H> static int h_tensor(const H* h, const char* name, float** ptr, long long* count) { GUARD(h); return h->m->tensor(name, ptr, count); }

extern "C" {

const char* ocrl_last_error(void) { return g_err; }
int ocrl_obs_u8_to_f32(const unsigned char* obs_hwc, float* obs_chw, int B, int H, int W, int C, void* stream) {
    if (!obs_hwc || !obs_chw || B < 1 || H < 1 || W < 1 || C < 1) { ocrl_set_error("ocrl_obs_u8_to_f32: bad arguments"); return 1; }
    return obs_u8_to_f32_launch(obs_hwc, obs_chw, B, H, W, C, ST(stream));
}
int ocrl_abi_version(void) { return OCRL_ABI_VERSION; }

size_t ocrl_slate_config_size(void) { return sizeof(ocrl_slate_config); }

int ocrl_slate_create(const ocrl_slate_config* c, ocrl_slate** out) {
    if (!c || !out) { ocrl_set_error("ocrl_slate_create: null argument"); return 1; }
    if (c->obs_size < 8 || c->obs_size % 4 || c->vocab_size < 256 || c->num_slots < 1 || c->num_iterations < 1 || c->max_batch < 1 ||
        c->num_dec_blocks < 1 || c->num_dec_heads < 1 || c->d_model % c->num_dec_heads) {
        ocrl_set_error("ocrl_slate_create: invalid configuration");
        return 1;
    }
    // T = (obs_size / 4)^2 tokens; the step's kernels are written for T % 4 == 0 (SlateModel::bind checks the same): refuse here,
    // before anything is allocated, instead of at bind time
    if (c->obs_size % 8) {
        const int e = c->obs_size / 4;
        ocrl_set_error("ocrl_slate_create: obs_size %d gives %d tokens per image; the token count must be a multiple of 4 (obs_size a multiple of 8)",
                       c->obs_size, e * e);
        return 1;
    }
    SlateConfig k;
    k.obs_size = c->obs_size; k.obs_channels = c->obs_channels; k.vocab = c->vocab_size; k.d_model = c->d_model;
    k.cnn_hidden = c->cnn_hidden; k.num_slots = c->num_slots; k.num_iters = c->num_iterations; k.slot_size = c->slot_size;
    k.mlp_hidden = c->mlp_hidden; k.num_blocks = c->num_dec_blocks; k.num_heads = c->num_dec_heads; k.dropout = c->dropout;
    k.max_batch = c->max_batch;
    k.hard = c->hard ? 1 : 0; k.use_bcdec = c->use_bcdec ? 1 : 0;
    k.slot_heads = c->num_slot_heads > 0 ? c->num_slot_heads : 1;
    if (k.slot_heads > 1 && (c->num_slots > 8 || k.slot_heads * c->num_slots > 16 || c->slot_size % k.slot_heads || (c->slot_size / k.slot_heads) % 16)) {
        ocrl_set_error("ocrl_slate_create: num_slot_heads %d needs heads * num_slots <= 16, num_slots <= 8 and a head width that is a multiple of 16", k.slot_heads);
        return 1;
    }
    if (k.use_bcdec && (c->num_slots > 16 || c->obs_size < 5)) { ocrl_set_error("ocrl_slate_create: broadcast decoder needs num_slots <= 16 and obs_size >= 5"); return 1; }
    return h_create(k, out);
}
void ocrl_slate_destroy(ocrl_slate* h) { h_destroy(h); }
int ocrl_slate_param_count(const ocrl_slate* h) { return h_param_count(h); }
int ocrl_slate_param_info(const ocrl_slate* h, int i, char* name, int name_cap, int shape[4], int* ndim, long long* offset,
                          long long* numel, int* group) {
    return h_param_info(h, i, name, name_cap, shape, ndim, offset, numel, group);
}
long long ocrl_slate_flat_size(const ocrl_slate* h) { return h_flat_size(h); }
long long ocrl_slate_group_begin(const ocrl_slate* h, int g) { return (h && h->m && g >= 0 && g <= 3) ? h->m->group_begin(g) : -1; }
size_t ocrl_slate_workspace_bytes(const ocrl_slate* h) { return h_workspace_bytes(h); }
int ocrl_slate_bind(ocrl_slate* h, float* p, float* g, float* m, float* v, void* ws, size_t n) { return h_bind(h, p, g, m, v, ws, n); }

int ocrl_slate_forward(ocrl_slate* h, const float* obs, int B, float tau, int train, unsigned long long seed, const float* nz,
                       const float* nzh, const float* ns, void* stream) {
    GUARD(h);
    StepInputs in;
    in.obs = obs; in.B = B; in.tau = tau; in.train = train; in.seed = seed; in.noise_z = nz; in.noise_zh = nzh; in.noise_slots = ns;
    return h->m->forward(in, ST(stream));
}
int ocrl_slate_backward(ocrl_slate* h, void* stream) { GUARD(h); return h->m->backward(ST(stream)); }
int ocrl_slate_encode(ocrl_slate* h, const float* obs, int B, unsigned long long seed, const float* ns, void* stream) {
    GUARD(h);
    StepInputs in;
    in.obs = obs; in.B = B; in.seed = seed; in.noise_slots = ns; in.train = 0;
    return h->m->encode(in, ST(stream));
}
int ocrl_slate_encode_backward(ocrl_slate* h, const float* dslots, void* stream) { GUARD(h); return h->m->encode_backward(dslots, ST(stream)); }
int ocrl_slate_freeze_weights(ocrl_slate* h, int on) { GUARD(h); h->m->freeze_weights(on != 0); return 0; }
int ocrl_slate_generate(ocrl_slate* h, void* stream) { GUARD(h); return h->m->generate(ST(stream)); }
int ocrl_slate_clip_adam(ocrl_slate* h, const float lr[3], float clip, int step, float gscale, void* stream) {
    GUARD(h);
    return h->m->clip_adam(lr, clip, step, gscale, ST(stream));
}
int ocrl_slate_grad_norm(ocrl_slate* h, void* stream) { GUARD(h); return h->m->grad_norm(ST(stream)); }
float* ocrl_slate_metrics(const ocrl_slate* h) { return h_metrics(h); }
int ocrl_slate_tensor(const ocrl_slate* h, const char* name, float** ptr, long long* count) { return h_tensor(h, name, ptr, count); }
int ocrl_slate_soft_z(ocrl_slate* h, void* stream) { GUARD(h); return h->m->soft_z(ST(stream)); }
int ocrl_slate_dropout_mask(const ocrl_slate* h, unsigned site, long long n, float* out, void* stream) {
    GUARD(h);
    return h->m->dropout_mask(site, n, out, ST(stream));
}

// ---------------------------------------------------------------- unit entry points
int ocrl_gemm(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int akc, int bkc, float alpha,
              const float* bias, int relu, const float* mask, int ldmask, const float* resid, int ldr, int splitk, float* ws, void* stream) {
    GemmArgs a;
    a.A = A; a.B = B; a.C = C; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.akc = akc; a.bkc = bkc; a.alpha = alpha;
    a.bias = bias; a.relu = relu; a.mask = mask; a.ldmask = ldmask; a.resid = resid; a.ldr = ldr;
    if (splitk > 1) {
        if (!ws || ldc != N) { ocrl_set_error("ocrl_gemm: split-k needs a workspace and ldc == N"); return 1; }
        a.splitk = splitk;
        return gemm_splitk_launch(a, ws, 0, 0, ST(stream));
    }
    return gemm_launch(a, ST(stream));
}
static GemmArgs gemm_args(const ocrl_gemm_desc& d) {
    GemmArgs a;
    a.A = d.A; a.B = d.B; a.C = d.C; a.M = d.M; a.N = d.N; a.K = d.K; a.lda = d.lda; a.ldb = d.ldb; a.ldc = d.ldc; a.akc = d.akc; a.bkc = d.bkc;
    a.batch = d.batch; a.batch_inner = d.batch_inner; a.sA = d.sA; a.sB = d.sB; a.sC = d.sC; a.sAi = d.sAi; a.sBi = d.sBi; a.sCi = d.sCi;
    a.splitk = d.splitk; a.alpha = d.alpha; a.bias = d.bias; a.relu = d.relu; a.drop_p = d.drop_p; a.drop_seed = d.drop_seed; a.drop_site = d.drop_site;
    a.mask = d.mask; a.ldmask = d.ldmask; a.sMask = d.sMask; a.mask_elu = d.mask_elu; a.resid = d.resid; a.ldr = d.ldr; a.sR = d.sR;
    a.adrop_p = d.adrop_p; a.adrop_site = d.adrop_site; a.adrop_ld = d.adrop_ld; a.bias_out = d.bias_out; a.sBias = d.sBias;
    a.a_mode = d.a_mode; a.b_mode = d.b_mode; a.x_lse = d.x_lse; a.x_tok = d.x_tok; a.x_scale = d.x_scale;
    a.epi_mode = d.epi_mode; a.stat = d.stat; a.hstat = d.hstat; a.hidx = d.hidx; a.e1 = d.e1; a.e2 = d.e2; a.e_seed = d.e_seed;
    a.e_lse = d.e_lse; a.e_rowvec = d.e_rowvec; a.e_scale = d.e_scale; a.force_tile = d.force_tile; a.force_sb = d.force_sb;
    return a;
}
size_t ocrl_gemm_desc_size(void) { return sizeof(ocrl_gemm_desc); }
int ocrl_gemm_plan(const ocrl_gemm_desc* d, int out[6]) {
    if (!d || !out) { ocrl_set_error("ocrl_gemm_plan: null argument"); return 1; }
    GemmArgs a = gemm_args(*d);
    // the workspace as ocrl_gemm_ex lays it out; the plan reads no pointer, so C's address stands in for it
    if (a.splitk > 1) gemm_splitk_layout(a, a.C, a.sBias ? a.sBias : (a.M + 3) & ~3);
    GemmPlan p;
    if (gemm_plan(a, &p)) return 1;
    out[0] = p.bm; out[1] = p.bn; out[2] = p.sb; out[3] = p.xf; out[4] = p.epi; out[5] = p.layout;
    return 0;
}
// split-k as the Linear weight gradients run it (gemm_splitk_launch): raw partial slabs in ws, then one reduction into C (and one into bias_out)
int ocrl_gemm_ex(const ocrl_gemm_desc* d, float* ws, size_t ws_floats, void* stream) {
    if (!d) { ocrl_set_error("ocrl_gemm_ex: null descriptor"); return 1; }
    GemmArgs a = gemm_args(*d);
    if (a.splitk <= 1) return gemm_launch(a, ST(stream));
    const long long slab = (long long)a.M * a.N, bslab = a.sBias ? a.sBias : (a.M + 3) & ~3;
    const size_t need = (size_t)a.splitk * slab + (a.bias_out ? (size_t)a.splitk * bslab : 0);
    if (a.ldc != a.N || !ws || ws_floats < need || bslab % 4) {
        ocrl_set_error("ocrl_gemm_ex: split-k needs ldc == N, sBias %% 4 == 0 and a workspace of %zu floats", need);
        return 1;
    }
    if (a.bias || a.relu || a.drop_p > 0.f || a.mask || a.resid || a.epi_mode) {
        ocrl_set_error("ocrl_gemm_ex: split-k partial products take no epilogue");
        return 1;
    }
    return gemm_splitk_launch(a, ws, bslab, 0, ST(stream));
}
int ocrl_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int cin, int cin_pad, int ks, int relu,
                    float* ws, void* stream) {
    if (conv_pack_launch(w, ws, nullptr, ks, cin_pad, 64, cin, ST(stream))) return 1;
    ConvArgs a;
    a.X = x; a.Wp = ws; a.Y = y; a.B = B; a.H = H; a.W = W; a.bias = bias; a.relu = relu;
    return conv_fwd_launch(a, ks, cin_pad, 64, ST(stream));
}
int ocrl_conv2d_fwd_lowlat(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int cin, int cin_pad, int ks, int relu,
                           float* ws, void* stream) {
    if (conv_pack_launch(w, ws, nullptr, ks, cin_pad, 64, cin, ST(stream))) return 1;
    ConvArgs a;
    a.X = x; a.Wp = ws; a.Y = y; a.B = B; a.H = H; a.W = W; a.bias = bias; a.relu = relu;
    return conv_fwd_launch(a, ks, cin_pad, 64, ST(stream), 1);
}
size_t ocrl_conv2d_x3_ws_floats(void) { return 2 * conv_x3_pack_floats(5); }
int ocrl_conv2d_fwd_x3(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int ks, int relu, float* ws, void* stream) {
    if (ks != 3 && ks != 5) { ocrl_set_error("ocrl_conv2d_fwd_x3: ks must be 3 or 5"); return 1; }
    if (conv_pack_x3_launch(w, ws, nullptr, ST(stream), ks)) return 1;
    ConvArgs a;
    a.X = x; a.Y = y; a.B = B; a.H = H; a.W = W; a.bias = bias; a.relu = relu;
    return conv_x3_launch(a, ws, ST(stream), ks);
}
int ocrl_conv2d_bwd_data_x3(const float* dy, const float* w, const float* mask, float* dx, int B, int H, int W, int ks, float* ws, void* stream) {
    if (ks != 3 && ks != 5) { ocrl_set_error("ocrl_conv2d_bwd_data_x3: ks must be 3 or 5"); return 1; }
    if (conv_pack_x3_launch(w, ws, ws + conv_x3_pack_floats(5), ST(stream), ks)) return 1;
    ConvArgs a;
    a.X = dy; a.Y = dx; a.B = B; a.H = H; a.W = W; a.mask = mask;
    return conv_x3_launch(a, ws + conv_x3_pack_floats(5), ST(stream), ks);
}
int ocrl_conv2d_bwd_data(const float* dy, const float* w, const float* mask, float* dx, int B, int H, int W, int ks, float* ws, void* stream) {
    float* bw = ws + (size_t)ks * ks * 64 * 64;
    if (conv_pack_launch(w, ws, bw, ks, 64, 64, 64, ST(stream))) return 1;
    ConvArgs a;
    a.X = dy; a.Wp = bw; a.Y = dx; a.B = B; a.H = H; a.W = W; a.mask = mask;
    return conv_fwd_launch(a, ks, 64, 64, ST(stream));
}
// the dW slabs plus 65536 floats, which hold the bias partials (64 per slab, at most 204 slabs)
size_t ocrl_conv2d_wgrad_ws_floats(int B, int H, int W, int ks, int cin_pad) {
    const size_t slabs = (size_t)conv_wgrad_slabs(B, H, W, ks, cin_pad);
    return slabs * ks * ks * 64 * cin_pad + (1 << 16);
}
int ocrl_conv2d_bwd_weight(const float* x, const float* dy, float* dw, float* db, int B, int H, int W, int cin, int cin_pad, int ks, float* ws,
                           size_t ws_floats, void* stream) {
    if (ws_floats < ocrl_conv2d_wgrad_ws_floats(B, H, W, ks, cin_pad)) { ocrl_set_error("ocrl_conv2d_bwd_weight: workspace too small"); return 1; }
    WgradArgs a;
    a.X = x; a.dY = dy; a.part = ws; a.B = B; a.H = H; a.W = W;
    return conv_wgrad_launch(a, ks, cin_pad, 64, cin, dw, db, 0, ST(stream), 0);
}
int ocrl_conv2d_bwd_weight_x3(const float* x, const float* dy, float* dw, int B, int H, int W, int ks, float* ws, size_t ws_floats, void* stream) {
    if (ks != 3 && ks != 5) { ocrl_set_error("ocrl_conv2d_bwd_weight_x3: ks must be 3 or 5"); return 1; }
    if (ws_floats < ocrl_conv2d_wgrad_ws_floats(B, H, W, ks, 64)) { ocrl_set_error("ocrl_conv2d_bwd_weight_x3: workspace too small"); return 1; }
    WgradArgs a;
    a.X = x; a.dY = dy; a.part = ws; a.B = B; a.H = H; a.W = W;
    return conv_wgrad_launch(a, ks, 64, 64, 64, dw, nullptr, 0, ST(stream), 1);
}
static bool conv_kernel_built(int ks, int cin_pad) { return (ks == 5 && (cin_pad == 64 || cin_pad == 8)) || (ks == 3 && cin_pad == 64); }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
size_t ocrl_conv_desc_size(void) { return sizeof(ocrl_conv_desc); }
int ocrl_conv2d_ex(const ocrl_conv_desc* d, float* ws, size_t ws_floats, void* stream) {
    if (!d) { ocrl_set_error("ocrl_conv2d_ex: null descriptor"); return 1; }
    if (!d->x || !d->w || !d->y || !ws || d->B < 1 || d->H < 1 || d->W < 1) { ocrl_set_error("ocrl_conv2d_ex: x, w, y, ws and a non-empty image are required"); return 1; }
    if (!conv_kernel_built(d->ks, d->cin_pad)) { ocrl_set_error("ocrl_conv2d_ex: no kernel for ks=%d cin_pad=%d (built: 5/64, 5/8, 3/64)", d->ks, d->cin_pad); return 1; }
    if (d->cin < 1 || d->cin > d->cin_pad) { ocrl_set_error("ocrl_conv2d_ex: cin %d outside 1 .. cin_pad %d", d->cin, d->cin_pad); return 1; }
    if (d->relu < 0 || d->relu > 2) { ocrl_set_error("ocrl_conv2d_ex: relu must be 0, 1 (ReLU) or 2 (ELU), got %d", d->relu); return 1; }
    if (d->mask_elu && !d->mask) { ocrl_set_error("ocrl_conv2d_ex: mask_elu needs a mask"); return 1; }
    if (d->transposed && (d->cin != 64 || d->cin_pad != 64)) { ocrl_set_error("ocrl_conv2d_ex: the transposed (backward-data) form needs cin = cin_pad = 64"); return 1; }
    if (!aligned16(d->x) || !aligned16(d->y) || !aligned16(ws) || !aligned16(d->bias) || !aligned16(d->posmap) || !aligned16(d->mask)) {
        ocrl_set_error("ocrl_conv2d_ex: x, y, ws, bias, posmap and mask must be 16-byte aligned");
        return 1;
    }
    const size_t pack = (size_t)d->ks * d->ks * d->cin_pad * 64, need = d->transposed ? 2 * pack : pack;
    if (ws_floats < need) { ocrl_set_error("ocrl_conv2d_ex: workspace of %zu floats, %zu needed", ws_floats, need); return 1; }
    float* bw = d->transposed ? ws + pack : nullptr;
    if (conv_pack_launch(d->w, ws, bw, d->ks, d->cin_pad, 64, d->cin, ST(stream))) return 1;
    ConvArgs a;
    a.X = d->x; a.Wp = bw ? bw : ws; a.Y = d->y; a.B = d->B; a.H = d->H; a.W = d->W; a.bias = d->bias; a.relu = d->relu;
    a.posmap = d->posmap; a.mask = d->mask; a.mask_elu = d->mask_elu ? 1 : 0;
    return conv_fwd_launch(a, d->ks, d->cin_pad, 64, ST(stream), d->low_latency ? 1 : 0);
}
size_t ocrl_conv_wgrad_desc_size(void) { return sizeof(ocrl_conv_wgrad_desc); }
int ocrl_conv2d_bwd_weight_ex(const ocrl_conv_wgrad_desc* d, float* ws, size_t ws_floats, void* stream) {
    if (!d) { ocrl_set_error("ocrl_conv2d_bwd_weight_ex: null descriptor"); return 1; }
    if (!d->x || !d->dy || !d->dw || !ws || d->B < 1 || d->H < 1 || d->W < 1) { ocrl_set_error("ocrl_conv2d_bwd_weight_ex: x, dy, dw, ws and a non-empty image are required"); return 1; }
    if (!conv_kernel_built(d->ks, d->cin_pad)) { ocrl_set_error("ocrl_conv2d_bwd_weight_ex: no kernel for ks=%d cin_pad=%d (built: 5/64, 5/8, 3/64)", d->ks, d->cin_pad); return 1; }
    if (d->cin < 1 || d->cin > d->cin_pad) { ocrl_set_error("ocrl_conv2d_bwd_weight_ex: cin %d outside 1 .. cin_pad %d", d->cin, d->cin_pad); return 1; }
    if (!aligned16(d->x) || !aligned16(d->dy) || !aligned16(ws)) { ocrl_set_error("ocrl_conv2d_bwd_weight_ex: x, dy and ws must be 16-byte aligned"); return 1; }
    const size_t need = ocrl_conv2d_wgrad_ws_floats(d->B, d->H, d->W, d->ks, d->cin_pad);
    if (ws_floats < need) { ocrl_set_error("ocrl_conv2d_bwd_weight_ex: workspace of %zu floats, %zu needed", ws_floats, need); return 1; }
    const int acc = d->accumulate ? 1 : 0;
    WgradArgs a;
    a.X = d->x; a.dY = d->dy; a.part = ws; a.B = d->B; a.H = d->H; a.W = d->W;
    return conv_wgrad_launch(a, d->ks, d->cin_pad, 64, d->cin, d->dw, d->db, acc, ST(stream), 0);
}
size_t ocrl_conv2d_first_fwd_ws_floats(void) { return conv_first_pack_floats(); }
int ocrl_conv2d_first_fwd(const float* obs, const float* w, const float* bias, float* y, int B, int H, int W, int relu, float* ws, size_t ws_floats,
                          void* stream) {
    if (!obs || !w || !y || !ws || B < 1 || H < 1 || W < 1) { ocrl_set_error("ocrl_conv2d_first_fwd: obs, w, y, ws and a non-empty image are required"); return 1; }
    if (relu < 0 || relu > 1) { ocrl_set_error("ocrl_conv2d_first_fwd: relu must be 0 or 1, got %d", relu); return 1; }
    if (ws_floats < conv_first_pack_floats()) { ocrl_set_error("ocrl_conv2d_first_fwd: workspace of %zu floats, %zu needed", ws_floats, conv_first_pack_floats()); return 1; }
    if (conv_first_pack_launch(w, ws, ST(stream))) return 1;
    return conv_first_fwd_launch(obs, ws, bias, y, B, H, W, relu, ST(stream));
}
size_t ocrl_conv2d_first_wgrad_ws_floats(int B, int H, int W) { return conv_first_wgrad_ws_floats(B, H, W); }
int ocrl_conv2d_first_bwd_weight(const float* obs, const float* dy, float* dw, float* db, int B, int H, int W, int accumulate, float* ws, size_t ws_floats,
                                 void* stream) {
    if (!obs || !dy || !dw || !ws || B < 1 || H < 1 || W < 1) { ocrl_set_error("ocrl_conv2d_first_bwd_weight: obs, dy, dw, ws and a non-empty image are required"); return 1; }
    const size_t need = conv_first_wgrad_ws_floats(B, H, W);
    if (ws_floats < need) { ocrl_set_error("ocrl_conv2d_first_bwd_weight: workspace of %zu floats, %zu needed", ws_floats, need); return 1; }
    return conv_first_wgrad_launch(obs, dy, ws, dw, db, B, H, W, accumulate ? 1 : 0, ST(stream));
}
int ocrl_layernorm_fwd(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, long long R, int F, void* stream) {
    return layernorm_fwd_launch(x, g, b, y, mean, rstd, R, F, ST(stream));
}
int ocrl_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, float* dx, float* dgb, long long R,
                       int F, float* ws, size_t ws_floats, void* stream) {
    return layernorm_bwd_launch(dy, x, mean, rstd, g, dx, dgb, R, F, 0, 0, ws, ws_floats, ST(stream));
}

int ocrl_sa_input_plan(long long R, int out[3]) {
    if (!out || R <= 0) { ocrl_set_error("ocrl_sa_input_plan: needs R > 0 and an output array"); return 1; }
    sa_input_plan(R, 0, out);
    return 0;
}
int ocrl_sa_input_fwd(const float* e4, const float* gamma, const float* beta, const float* W0, const float* b0, const float* W2, const float* b2,
                      float* mean, float* rstd, float* h1, float* x, long long R, int max_wgs, void* stream) {
    return sa_input_fwd_launch(e4, gamma, beta, W0, b0, W2, b2, mean, rstd, nullptr, h1, x, R, max_wgs, ST(stream));
}
int ocrl_sa_input_bwd(const float* dx, const float* h1, const float* e4, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      const float* W0, const float* W2, float* de4, float* dW0, float* db0, float* dW2, float* db2, float* dgamma, float* dbeta,
                      long long R, int max_wgs, float* ws, size_t ws_floats, void* stream) {
    return sa_input_bwd_launch(dx, h1, e4, mean, rstd, gamma, beta, W0, W2, de4, dW0, db0, dW2, db2, dgamma, dbeta, R, max_wgs, ws, ws_floats,
                               ST(stream));
}

int ocrl_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int T, int d, int h, int ld, float p,
                       unsigned long long seed, unsigned site, void* stream) {
    AttnArgs a;
    a.q = q; a.k = k; a.v = v; a.o = o; a.lse = lse; a.B = B; a.T = T; a.d = d; a.h = h; a.ld = ld; a.p = p; a.seed = seed; a.site = site;
    return attn_launch(a, 0, ST(stream));
}
int ocrl_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* dO, float* dq,
                       float* dk, float* dv, float* delta, int B, int T, int d, int h, int ld, float p, unsigned long long seed,
                       unsigned site, void* stream) {
    AttnArgs a;
    a.q = q; a.k = k; a.v = v; a.o = const_cast<float*>(o); a.lse = const_cast<float*>(lse); a.B = B; a.T = T; a.d = d; a.h = h; a.ld = ld;
    a.p = p; a.seed = seed; a.site = site; a.dO = dO; a.dq = dq; a.dk = dk; a.dv = dv; a.delta = delta;
    return attn_launch(a, 1, ST(stream));
}
size_t ocrl_attention_bwd_ds_floats(int B, int T, int h) { return attn_bwd_ds_floats(B, T, h); }
int ocrl_attention_bwd_ws(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* dO, float* dq,
                          float* dk, float* dv, float* delta, int B, int T, int d, int h, int ld, float p, unsigned long long seed,
                          unsigned site, float* ds, size_t ds_floats, void* stream) {
    AttnArgs a;
    a.q = q; a.k = k; a.v = v; a.o = const_cast<float*>(o); a.lse = const_cast<float*>(lse); a.B = B; a.T = T; a.d = d; a.h = h; a.ld = ld;
    a.p = p; a.seed = seed; a.site = site; a.dO = dO; a.dq = dq; a.dk = dk; a.dv = dv; a.delta = delta; a.ds = ds; a.ds_floats = ds_floats;
    return attn_launch(a, 1, ST(stream));
}

// ---- cross attention to the slots: the folded form (xattn.hip) and the plain kernels (elementwise.hip), as the decoder runs them
int ocrl_xattn_plan(int K, int d, int h, int out[5]) {
    if (!out) { ocrl_set_error("ocrl_xattn_plan: null argument"); return 1; }
    XaPlan p;
    if (!xattn_plan(K, d, h, &p)) ocrl_set_error("ocrl_xattn_plan: no folded form for K %d, d %d, heads %d", K, d, h);
    out[0] = p.supported ? 1 : 0; out[1] = p.KP; out[2] = p.NC; out[3] = p.NM; out[4] = (int)p.lds;
    return 0;
}
size_t ocrl_xattn_desc_size(void) { return sizeof(ocrl_xattn_desc); }
static XaHost xattn_host(const ocrl_xattn_desc& d) {
    XaHost hx;
    hx.x = d.x; hx.P = d.P; hx.Ab = d.Ab; hx.AbT = d.AbT; hx.Vo = d.Vo; hx.VoT = d.VoT;
    hx.B = d.B; hx.T = d.T; hx.K = d.K; hx.d = d.d; hx.h = d.h; hx.p = d.p; hx.seed = d.seed; hx.site_p = d.site_p; hx.site_o = d.site_o;
    return hx;
}
int ocrl_xattn_fwd(const ocrl_xattn_desc* d, void* stream) {
    if (!d) { ocrl_set_error("ocrl_xattn_fwd: null descriptor"); return 1; }
    if (!xattn_supported(d->K, d->d, d->h)) { ocrl_set_error("ocrl_xattn_fwd: no folded form for K %d, d %d, heads %d", d->K, d->d, d->h); return 1; }
    if (d->B < 1 || d->T < 1 || !d->x || !d->resid || !d->mem || !d->Wq || !d->Wk || !d->Wv || !d->Wo || !d->ck || !d->cv || !d->Ab || !d->AbT ||
        !d->Vo || !d->VoT || !d->y || !d->P) {
        ocrl_set_error("ocrl_xattn_fwd: null buffer or empty shape");
        return 1;
    }
    XaFoldHost f;
    f.mem = d->mem; f.B = d->B; f.K = d->K; f.d = d->d; f.h = d->h; f.nblk = 1;
    f.Wq[0] = d->Wq; f.Wk[0] = d->Wk; f.Wv[0] = d->Wv; f.Wo[0] = d->Wo;
    f.ck[0] = d->ck; f.cv[0] = d->cv; f.Ab[0] = d->Ab; f.AbT[0] = d->AbT; f.Vo[0] = d->Vo; f.VoT[0] = d->VoT;
    if (xattn_fold_fwd_launch(f, ST(stream))) return 1;
    XaHost hx = xattn_host(*d);
    hx.resid = d->resid; hx.y = d->y;
    return xattn_launch(hx, 0, ST(stream));
}
int ocrl_xattn_bwd(const ocrl_xattn_desc* d, void* stream) {
    if (!d) { ocrl_set_error("ocrl_xattn_bwd: null descriptor"); return 1; }
    if (!xattn_supported(d->K, d->d, d->h)) { ocrl_set_error("ocrl_xattn_bwd: no folded form for K %d, d %d, heads %d", d->K, d->d, d->h); return 1; }
    if (d->B < 1 || d->T < 1 || !d->x || !d->Wq || !d->Wo || !d->ck || !d->cv || !d->Ab || !d->AbT || !d->Vo || !d->VoT || !d->P || !d->gd || !d->Pd ||
        !d->dS || !d->dx || !d->dAb || !d->dVo || !d->dck || !d->dcv || !d->dWq || !d->dWo || !d->pq || !d->po || !d->cs_ws) {
        ocrl_set_error("ocrl_xattn_bwd: null buffer or empty shape");
        return 1;
    }
    if (d->cs_ws_floats < (size_t)d->d * d->d || d->B > 64) { ocrl_set_error("ocrl_xattn_bwd: needs B <= 64 and a column-sum workspace of d * d floats"); return 1; }
    XaHost hx = xattn_host(*d);
    hx.y = d->dx; hx.gd = d->gd; hx.Pd = d->Pd; hx.dS = d->dS;
    if (xattn_launch(hx, 1, ST(stream))) return 1;
    XaFoldBwdHost f;
    f.Pd = d->Pd; f.dS = d->dS; f.gd = d->gd; f.x = d->x; f.Wq = d->Wq; f.Wo = d->Wo; f.ck = d->ck; f.cv = d->cv;
    f.dVo = d->dVo; f.dAb = d->dAb; f.dck = d->dck; f.dcv = d->dcv; f.pq = d->pq; f.po = d->po; f.dWq = d->dWq; f.dWo = d->dWo;
    f.ws = d->cs_ws; f.ws_floats = d->cs_ws_floats; f.B = d->B; f.T = d->T; f.K = d->K; f.d = d->d; f.h = d->h;
    return xattn_fold_bwd_launch(f, ST(stream));
}
int ocrl_cross_attn_fwd(const float* Q, const float* Km, const float* Vm, float* O, float* P, int B, int T, int K, int d, int h, float p,
                        unsigned long long seed, unsigned site, void* stream) {
    if (!Q || !Km || !Vm || !O || !P || B < 1 || T < 1 || h < 1) { ocrl_set_error("ocrl_cross_attn_fwd: null buffer or empty shape"); return 1; }
    return cross_attn_fwd_launch(Q, Km, Vm, O, P, B, T, K, d, h, p, seed, site, ST(stream));
}
size_t ocrl_cross_attn_bwd_ws_floats(int B, int T, int K, int d, int h) {
    if (B < 1 || T < 1 || K < 1 || d < 1 || h < 1 || d % h) { ocrl_set_error("ocrl_cross_attn_bwd_ws_floats: invalid shape"); return 0; }
    return cross_attn_bwd_ws_floats(B, T, K, d, h);
}
int ocrl_cross_attn_bwd(const float* dO, const float* Q, const float* Km, const float* Vm, const float* P, float* dQ, float* dKm, float* dVm, int B,
                        int T, int K, int d, int h, float p, unsigned long long seed, unsigned site, float* ws, size_t ws_floats, void* stream) {
    if (!dO || !Q || !Km || !Vm || !P || !dQ || !dKm || !dVm || B < 1 || T < 1 || h < 1) { ocrl_set_error("ocrl_cross_attn_bwd: null buffer or empty shape"); return 1; }
    return cross_attn_bwd_launch(dO, Q, Km, Vm, P, dQ, dKm, dVm, B, T, K, d, h, p, seed, site, ws, ws_floats, ST(stream));
}


// ---------------------------------------------------------------- IODINE
int ocrl_iodine_create(const ocrl_iodine_config* c, ocrl_iodine** out) {
    if (!c || !out) { ocrl_set_error("ocrl_iodine_create: null argument"); return 1; }
    if (c->obs_size < 16 || c->obs_size % 16 || c->obs_channels != 3 || c->slot_size < 4 || c->slot_size % 4 || c->slot_size > 256 ||
        c->num_iterations < 1 || c->num_slots < 1 || c->num_slots > 16 || c->ref_mlp_hidden < 64 || c->ref_mlp_hidden % 64 || c->max_batch < 1 ||
        !(c->sigma > 0.f)) {
        ocrl_set_error("ocrl_iodine_create: invalid configuration");
        return 1;
    }
    IodineConfig k;
    k.obs_size = c->obs_size; k.obs_channels = c->obs_channels; k.slot_size = c->slot_size; k.num_iters = c->num_iterations;
    k.num_slots = c->num_slots; k.sigma = c->sigma; k.beta = c->beta; k.layer_norm = c->layer_norm; k.ref_mlp_hidden = c->ref_mlp_hidden;
    k.max_batch = c->max_batch;
    return h_create(k, out);
}
void ocrl_iodine_destroy(ocrl_iodine* h) { h_destroy(h); }
int ocrl_iodine_param_count(const ocrl_iodine* h) { return h_param_count(h); }
int ocrl_iodine_param_info(const ocrl_iodine* h, int i, char* name, int name_cap, int shape[4], int* ndim, long long* offset, long long* numel) {
    return h_param_info(h, i, name, name_cap, shape, ndim, offset, numel, nullptr);       // one optimiser group: no `group` out-parameter
}
long long ocrl_iodine_flat_size(const ocrl_iodine* h) { return h_flat_size(h); }
size_t ocrl_iodine_workspace_bytes(const ocrl_iodine* h) { return h_workspace_bytes(h); }
int ocrl_iodine_bind(ocrl_iodine* h, float* p, float* g, float* m, float* v, void* ws, size_t n) { return h_bind(h, p, g, m, v, ws, n); }
int ocrl_iodine_forward(ocrl_iodine* h, const float* obs, int B, unsigned long long seed, const float* noise, void* stream) {
    GUARD(h);
    return h->m->forward(obs, B, seed, noise, ST(stream));
}
int ocrl_iodine_backward(ocrl_iodine* h, void* stream) { GUARD(h); return h->m->backward(ST(stream)); }
int ocrl_iodine_clip_adam(ocrl_iodine* h, float lr, float clip, int step, float gscale, void* stream) {
    GUARD(h);
    return h->m->clip_adam(lr, clip, step, gscale, ST(stream));
}
int ocrl_iodine_grad_norm(ocrl_iodine* h, void* stream) { GUARD(h); return h->m->grad_norm(ST(stream)); }
float* ocrl_iodine_metrics(const ocrl_iodine* h) { return h_metrics(h); }
int ocrl_iodine_tensor(const ocrl_iodine* h, const char* name, float** ptr, long long* count) { return h_tensor(h, name, ptr, count); }
}  // extern "C"
