// The slot-attention module (ocrs/common/slot_attn.py:11-45) as its two hosts see it, SlateModel and the unit entry points of sa_unit.cpp:
// the order of its 17 weights, the pack table, the buffers around slot_attn_launch, the shape fields of its arguments and the column blocks
// that meet in each weight gradient, each written once.  Host only, and no policy: the callers loop over sa_wgrad_list and issue their own
// products, on their stream, with their scratch, split rule and form of bias gradient.  The column sums of the LayerNorm gamma / beta
// partials (g_small, per image [norm_slots 2D | norm_mlp 2D | norm_inputs 2C]) stay with them too: the model sums a weight|bias pair with
// one launch because the two are adjacent in its flat buffer, the unit has six separate tensors -- the destinations differ, not the rule.
#pragma once
#include <math.h>

#include "kernels.h"

// the reference's parameter order: the `w` / `dw` arrays of ocrl_slot_attention_fwd / _bwd (include/ocrl_hip.h)
enum SaWeight {
    SAW_NORM_INPUTS_W, SAW_NORM_INPUTS_B, SAW_NORM_SLOTS_W, SAW_NORM_SLOTS_B, SAW_NORM_MLP_W, SAW_NORM_MLP_B, SAW_Q, SAW_K, SAW_V,
    SAW_GRU_WIH, SAW_GRU_WHH, SAW_GRU_BIH, SAW_GRU_BHH, SAW_MLP0_W, SAW_MLP0_B, SAW_MLP2_W, SAW_MLP2_B, SA_NW
};
inline constexpr const char* SA_WEIGHT_NAMES[SA_NW] = {       // below the module's prefix
    "norm_inputs.weight", "norm_inputs.bias", "norm_slots.weight", "norm_slots.bias", "norm_mlp.weight", "norm_mlp.bias", "project_q.weight", "project_k.weight",
    "project_v.weight", "gru.weight_ih", "gru.weight_hh", "gru.bias_ih", "gru.bias_hh", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"};

// ---- pack table: every weight into its sa_wts_layout slot, the matrices in both tilings (modes 2 and 3).  Returns the entry count;
// *max_elems, the largest entry, sizes pack_launch's grid.
constexpr int SA_PACK_ENTRIES = 24;
inline int sa_pack_table(const float* const w[SA_NW], int C, int D, int H, PackEntry out[SA_PACK_ENTRIES], int* max_elems) {
    const SaWts wo = sa_wts_layout(C, D, H);
    const int t[SA_NW][4] = {      // rows, cols, offset, offset of the transposed copy
        {1, C, wo.ln_in_g, -1}, {1, C, wo.ln_in_b, -1}, {1, D, wo.ln_s_g, -1}, {1, D, wo.ln_s_b, -1}, {1, D, wo.ln_m_g, -1}, {1, D, wo.ln_m_b, -1},
        {D, D, wo.Wq, wo.WqT}, {D, C, wo.Wk, wo.WkT}, {D, C, wo.Wv, wo.WvT}, {3 * D, D, wo.Wih, wo.WihT}, {3 * D, D, wo.Whh, wo.WhhT},
        {1, 3 * D, wo.bih, -1}, {1, 3 * D, wo.bhh, -1}, {H, D, wo.W0, wo.W0T}, {1, H, wo.b0, -1}, {D, H, wo.W2, wo.W2T}, {1, D, wo.b2, -1}};
    int n = 0;
    for (int i = 0; i < SA_NW; ++i) {
        out[n++] = PackEntry{w[i], t[i][0], t[i][1], t[i][2], t[i][3] < 0 ? 0 : 2};
        if (t[i][3] >= 0) out[n++] = PackEntry{w[i], t[i][0], t[i][1], t[i][3], 3};
    }
    *max_elems = 3 * D * D > H * D ? 3 * D * D : H * D;
    return n;
}

// ---- buffers, in floats: packed weights, saved activations and gradient rows (a row per (image, iteration, slot)), the LayerNorm
// partials, the device copy of the pack table (room for 64 entries), the exchange and partial-sum buffers of the pipelined form
struct SaSizes { size_t wts, save, grows, small, table, xchg, parts; };
inline SaSizes sa_sizes(size_t B, int K, int C, int D, int H, int I, int NH) {
    const size_t R = B * I * K;
    return SaSizes{(size_t)sa_wts_layout(C, D, H).total, R * sa_save_layout(C, D, H, NH).ld, R * sa_grad_layout(C, D, H, NH).ld, B * (4 * D + 2 * C),
                   64 * sizeof(PackEntry) / 4 + 64, B * sa_xchg_floats_host(K * NH, D), sa_parts_floats_host((int)B, K * NH)};
}
// SlotAttnArgs::attn_heads, the per-head attention maps [B,N,NH*K]: none with one head
inline size_t sa_attn_heads_floats(size_t B, int N, int K, int NH) { return NH > 1 ? B * N * K * NH : 0; }

// ---- arguments: the shape fields, eps and the soft-max scale; the caller adds its pointers and `phase`
inline SlotAttnArgs sa_args(int B, int N, int K, int D, int H, int I, int NH) {
    SlotAttnArgs a;
    a.B = B; a.N = N; a.K = K; a.D = D; a.H = H; a.I = I; a.NH = NH; a.eps = 1e-8f; a.scale = 1.0f / sqrtf((float)(D / NH));
    return a;
}

// ---- weight gradients: dW[w] + w_off, [N_out, K_in] = alpha * dy^T x over the B*I*K rows; db[b] = column sums of dy (b < 0: none).
// dy and x are column blocks of the gradient rows (sa_grad_layout) or of the saved activations (sa_save_layout).
struct SaCols {
    bool grad; int col, ld;        // of the gradient rows, or else of the saved activations
    const float* at(const float* save, const float* grows) const { return (grad ? grows : save) + col; }
};
struct SaWgrad { SaCols dy, x; int w, b; size_t w_off; int N_out, K_in; float alpha; };
constexpr int SA_MAX_WGRADS = 5 + 2 * 16;        // heads * slots <= 16
inline int sa_wgrad_list(int C, int D, int H, int NH, float scale, SaWgrad out[SA_MAX_WGRADS]) {
    const SaSave so = sa_save_layout(C, D, H, NH);
    const SaGrad go = sa_grad_layout(C, D, H, NH);
    auto S = [&](int col) { return SaCols{false, col, so.ld}; };
    auto G = [&](int col) { return SaCols{true, col, go.ld}; };
    int n = 0;
    out[n++] = SaWgrad{G(go.out), S(so.hid), SAW_MLP2_W, SAW_MLP2_B, 0, D, H, 1.f};
    out[n++] = SaWgrad{G(go.hid), S(so.m), SAW_MLP0_W, SAW_MLP0_B, 0, H, D, 1.f};
    out[n++] = SaWgrad{G(go.gi), S(so.u), SAW_GRU_WIH, SAW_GRU_BIH, 0, 3 * D, D, 1.f};
    out[n++] = SaWgrad{G(go.gh), S(so.sprev), SAW_GRU_WHH, SAW_GRU_BHH, 0, 3 * D, D, 1.f};
    out[n++] = SaWgrad{G(go.q), S(so.sn), SAW_Q, -1, 0, D, D, 1.f};
    for (int h = 0, dh = D / NH; h < NH; ++h) {       // head h: rows h*dh .. of project_v / project_k against that head's weighted means / folded-query gradients
        out[n++] = SaWgrad{G(go.u + h * dh), S(so.up + h * C), SAW_V, -1, (size_t)h * dh * C, dh, C, 1.f};
        out[n++] = SaWgrad{S(so.q + h * dh), G(go.qp + h * C), SAW_K, -1, (size_t)h * dh * C, dh, C, scale};
    }
    return n;
}
