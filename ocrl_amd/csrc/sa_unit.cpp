// Unit entry points of the slot-attention kernels (include/ocrl_hip.h: ocrl_slot_attention_*): the north-star kernel on its own,
// with the reference's weight tensors as they are (ocrs/common/slot_attn.py:11-45), for parity tests and for hosts that only
// want this operator.  Same code path as the model: pack -> slot_attn_launch -> weight-gradient GEMMs over (image, iteration, slot),
// on the host side too (slot_attn_host.h: the pack table, the buffer sizes, the argument fill and the list of products).
#include <string.h>

#include "../../include/ocrl_hip.h"
#include "slot_attn_host.h"
#include "unit_base.h"

namespace {
constexpr int SA_MAX_SPLITS = 64;        // split-k slabs of a weight gradient over the (image, iteration, slot) rows
constexpr int C = 64;                    // width of the input rows
struct Lay {
    size_t wts, save, grows, small, table, xchg, parts, scratch, scratch_floats, total;
};
Lay layout(int B, int K, int D, int H, int I, int NH) {
    const SaSizes z = sa_sizes(B, K, C, D, H, I, NH);
    Lay l;
    WsTake take;
    l.wts = take(z.wts); l.save = take(z.save); l.grows = take(z.grows); l.small = take(z.small);
    l.table = take(z.table); l.xchg = take(z.xchg); l.parts = take(z.parts);
    l.scratch_floats = (size_t)1024 * 3 * D * D / 4 + (1 << 18);
    l.scratch = take(l.scratch_floats);
    l.total = take.end;
    return l;
}
}  // namespace

extern "C" {

size_t ocrl_slot_attention_ws_floats(int B, int K, int D, int H, int I) { return layout(B, K, D, H, I, 1).total; }
// heads > 1: + the per-head attention maps [B,N,heads*K] behind the single-head layout
size_t ocrl_slot_attention_mh_ws_floats(int B, int N, int K, int D, int H, int I, int heads) {
    return layout(B, K, D, H, I, heads).total + sa_attn_heads_floats(B, N, K, heads);
}

int ocrl_slot_attention_plan(int K, int D, int H, int heads, int* out6) {
    OCRL_REQUIRE(out6, "ocrl_slot_attention_plan: null argument");
    SaPlan pl;
    RC(sa_plan(K, D, H, heads, &pl));
    out6[0] = pl.G; out6[1] = pl.NB; out6[2] = pl.KB; out6[3] = (int)pl.smem_fwd; out6[4] = (int)pl.smem_bwd; out6[5] = pl.KS;
    return 0;
}

int ocrl_slot_attention_fwd(const float* x, const float* slots0, const float* const* w, float* slots, float* attn, int B, int N, int K, int D, int H, int I,
                            float* ws, size_t ws_floats, void* stream) {
    return ocrl_slot_attention_mh_fwd(x, slots0, w, slots, attn, B, N, K, D, H, I, 1, ws, ws_floats, stream);
}
int ocrl_slot_attention_bwd(const float* x, const float* dslots, float* dx, float* dslots0, float* const* dw, int B, int N, int K, int D, int H, int I,
                            float* ws, size_t ws_floats, void* stream) {
    return ocrl_slot_attention_mh_bwd(x, dslots, dx, dslots0, dw, B, N, K, D, H, I, 1, ws, ws_floats, stream);
}

int ocrl_slot_attention_mh_fwd(const float* x, const float* slots0, const float* const* w, float* slots, float* attn, int B, int N, int K, int D, int H, int I,
                               int NH, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(x && slots0 && w && slots && ws, "ocrl_slot_attention_fwd: null argument");
    OCRL_REQUIRE(NH >= 1 && D % NH == 0, "ocrl_slot_attention_fwd: %d heads do not divide the slot size %d", NH, D);
    const Lay l = layout(B, K, D, H, I, NH);
    RC(ws_check("ocrl_slot_attention_fwd", ws_floats, l.total + sa_attn_heads_floats(B, N, K, NH)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PackEntry e[SA_PACK_ENTRIES];
    int mx = 0;
    const int n = sa_pack_table(w, C, D, H, e, &mx);
    OCRL_HIP(hipMemcpyAsync(ws + l.table, e, n * sizeof(PackEntry), hipMemcpyHostToDevice, st));
    OCRL_HIP(hipStreamSynchronize(st));            // `e` lives on this stack frame
    RC(pack_launch(reinterpret_cast<const PackEntry*>(ws + l.table), n, mx, ws + l.wts, st));
    SlotAttnArgs a = sa_args(B, N, K, D, H, I, NH);
    a.x = x; a.slots0 = slots0; a.wts = ws + l.wts; a.slots = slots; a.attn = attn; a.attn_heads = NH > 1 ? ws + l.total : nullptr; a.save = ws + l.save;
    a.xchg = ws + l.xchg; a.parts = ws + l.parts;
    return slot_attn_launch(a, 0, st);
}

int ocrl_slot_attention_mh_bwd(const float* x, const float* dslots, float* dx, float* dslots0, float* const* dw, int B, int N, int K, int D, int H, int I,
                               int NH, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(x && dslots && dx && dslots0 && dw && ws, "ocrl_slot_attention_bwd: null argument");
    OCRL_REQUIRE(NH >= 1 && D % NH == 0, "ocrl_slot_attention_bwd: %d heads do not divide the slot size %d", NH, D);
    const Lay l = layout(B, K, D, H, I, NH);
    RC(ws_check("ocrl_slot_attention_bwd", ws_floats, l.total));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *save = ws + l.save, *grows = ws + l.grows, *small = ws + l.small, *scr = ws + l.scratch;
    SlotAttnArgs a = sa_args(B, N, K, D, H, I, NH);
    a.x = x; a.wts = ws + l.wts; a.save = save; a.dslots = dslots; a.dx = dx; a.dslots0 = dslots0; a.grows = grows; a.g_small = small;
    a.xchg = ws + l.xchg; a.parts = ws + l.parts;
    RC(slot_attn_launch(a, 1, st));
    const long long R = (long long)B * I * K;
    const size_t sf = l.scratch_floats;
    // weight gradient over the R rows (split-k as every Linear, at most SA_MAX_SPLITS slabs); the bias gradient as column sums of dy
    SaWgrad wg[SA_MAX_WGRADS];
    const int nwg = sa_wgrad_list(C, D, H, NH, a.scale, wg);
    for (int i = 0; i < nwg; ++i) {
        const SaWgrad& e = wg[i];
        const float* dy = e.dy.at(save, grows);
        RC(lin_bwd_w(dy, e.dy.ld, e.x.at(save, grows), e.x.ld, dw[e.w] + e.w_off, nullptr, R, e.N_out, e.K_in, e.alpha, scr, sf, st, Drop(), Xf(), 0,
                     SA_MAX_SPLITS));
        if (e.b >= 0) RC(colsum_launch(dy, e.dy.ld, dw[e.b], R, e.N_out, 0, 1.f, scr, sf, st));
    }
    // LayerNorm gammas / betas: per-image partials [B][ln_s (2D) | ln_m (2D) | ln_in (2C)]; weight and bias are separate tensors here
    const int SM = 4 * D + 2 * C;
    RC(colsum_launch(small + 0, SM, dw[SAW_NORM_SLOTS_W], B, D, 0, 1.f, scr, sf, st));
    RC(colsum_launch(small + D, SM, dw[SAW_NORM_SLOTS_B], B, D, 0, 1.f, scr, sf, st));
    RC(colsum_launch(small + 2 * D, SM, dw[SAW_NORM_MLP_W], B, D, 0, 1.f, scr, sf, st));
    RC(colsum_launch(small + 3 * D, SM, dw[SAW_NORM_MLP_B], B, D, 0, 1.f, scr, sf, st));
    RC(colsum_launch(small + 4 * D, SM, dw[SAW_NORM_INPUTS_W], B, C, 0, 1.f, scr, sf, st));
    RC(colsum_launch(small + 4 * D + C, SM, dw[SAW_NORM_INPUTS_B], B, C, 0, 1.f, scr, sf, st));
    return 0;
}

}  // extern "C"
