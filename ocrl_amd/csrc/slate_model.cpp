// SLATE training step on the HIP kernels: parameter table, workspace, forward, backward, optimiser.
// Follows the reference's SLATE_Module.get_loss (ocrs/slate/slate_module.py:198-241) and
// Base.update (ocrs/base.py:60-74); maths restated in SURVEY.md Appendix A.
#include "slate_model.h"

#include "switches.h"

#include <math.h>
#include <stdarg.h>
#include <string.h>

static std::string fmt(const char* f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// ---------------------------------------------------------------------------------------------
SlateModel::SlateModel(const SlateConfig& c) : cfg(c) {
    S = c.obs_size; E = S / 4; T = E * E; N = S * S; V = c.vocab; d = c.d_model; C = c.cnn_hidden;
    K = c.num_slots; I = c.num_iters; D = c.slot_size; H = c.mlp_hidden; NB = c.num_blocks; NH = c.num_heads;
    DH = d / NH; Bmax = c.max_batch; SH = c.slot_heads > 0 ? c.slot_heads : 1;
    const int ch = c.obs_channels;
    // group 0: dVAE (ocrs/common/models.py:10-37) — order = reference module.parameters() order
    add_param("_dvae._encoder.0.m.weight", {64, ch, 4, 4}, 0); add_param("_dvae._encoder.0.m.bias", {64}, 0);
    for (int i = 1; i < 7; ++i) { add_param(fmt("_dvae._encoder.%d.m.weight", i), {64, 64, 1, 1}, 0); add_param(fmt("_dvae._encoder.%d.m.bias", i), {64}, 0); }
    add_param("_dvae._encoder.7.weight", {V, 64, 1, 1}, 0); add_param("_dvae._encoder.7.bias", {V}, 0);
    const int di[9] = {0, 1, 2, 3, 4, 6, 7, 8, 9};
    const int dshape[9][4] = {{64, V, 1, 1}, {64, 64, 3, 3}, {64, 64, 1, 1}, {64, 64, 1, 1}, {256, 64, 1, 1},
                              {64, 64, 3, 3}, {64, 64, 1, 1}, {64, 64, 1, 1}, {256, 64, 1, 1}};
    for (int i = 0; i < 9; ++i) {
        add_param(fmt("_dvae._decoder.%d.m.weight", di[i]), {dshape[i][0], dshape[i][1], dshape[i][2], dshape[i][3]}, 0);
        add_param(fmt("_dvae._decoder.%d.m.bias", di[i]), {dshape[i][0]}, 0);
    }
    add_param("_dvae._decoder.11.weight", {ch, 64, 1, 1}, 0); add_param("_dvae._decoder.11.bias", {ch}, 0);
    // group 1
    add_param("_enc._encoder.0.m.weight", {C, ch, 5, 5}, 1); add_param("_enc._encoder.0.m.bias", {C}, 1);
    for (int i = 1; i < 3; ++i) { add_param(fmt("_enc._encoder.%d.m.weight", i), {C, C, 5, 5}, 1); add_param(fmt("_enc._encoder.%d.m.bias", i), {C}, 1); }
    add_param("_enc._encoder.3.weight", {C, C, 5, 5}, 1); add_param("_enc._encoder.3.bias", {C}, 1);
    add_param("_enc_pos.channels_map.weight", {C, 4, 1, 1}, 1); add_param("_enc_pos.channels_map.bias", {C}, 1);
    add_param("_slotattn.slot_mu", {1, 1, D}, 1); add_param("_slotattn.slot_log_sigma", {1, 1, D}, 1);
    add_param("_slotattn.layer_norm.weight", {C}, 1); add_param("_slotattn.layer_norm.bias", {C}, 1);
    add_param("_slotattn.mlp.0.weight", {C, C}, 1); add_param("_slotattn.mlp.0.bias", {C}, 1);
    add_param("_slotattn.mlp.2.weight", {C, C}, 1); add_param("_slotattn.mlp.2.bias", {C}, 1);
    const std::string sa = "_slotattn.slot_attention.";
    add_param(sa + "norm_inputs.weight", {C}, 1); add_param(sa + "norm_inputs.bias", {C}, 1);
    add_param(sa + "norm_slots.weight", {D}, 1); add_param(sa + "norm_slots.bias", {D}, 1);
    add_param(sa + "norm_mlp.weight", {D}, 1); add_param(sa + "norm_mlp.bias", {D}, 1);
    add_param(sa + "project_q.weight", {D, D}, 1); add_param(sa + "project_k.weight", {D, C}, 1); add_param(sa + "project_v.weight", {D, C}, 1);
    add_param(sa + "gru.weight_ih", {3 * D, D}, 1); add_param(sa + "gru.weight_hh", {3 * D, D}, 1);
    add_param(sa + "gru.bias_ih", {3 * D}, 1); add_param(sa + "gru.bias_hh", {3 * D}, 1);
    add_param(sa + "mlp.0.weight", {H, D}, 1); add_param(sa + "mlp.0.bias", {H}, 1);
    add_param(sa + "mlp.2.weight", {D, H}, 1); add_param(sa + "mlp.2.bias", {D}, 1);
    add_param("_slotproj.weight", {d, D}, 1);
    if (c.use_bcdec) {      // ocrs/common/models.py:110-126, appended to the slot-attention group (slate_module.py:96-103)
        add_param("_dec._decoder.0.m.weight", {C, D, 5, 5}, 1); add_param("_dec._decoder.0.m.bias", {C}, 1);
        for (int i = 1; i < 3; ++i) { add_param(fmt("_dec._decoder.%d.m.weight", i), {C, C, 5, 5}, 1); add_param(fmt("_dec._decoder.%d.m.bias", i), {C}, 1); }
        add_param("_dec._decoder.3.weight", {ch + 1, C, 3, 3}, 1); add_param("_dec._decoder.3.bias", {ch + 1}, 1);
        add_param("_dec._pos_emb.channels_map.weight", {D, 4, 1, 1}, 1); add_param("_dec._pos_emb.channels_map.bias", {D}, 1);
    }
    // group 2
    add_param("_dict.dictionary.weight", {V, d}, 2);
    add_param("_bos_token._bos_token", {1, 1, d}, 2);
    add_param("_z_pos.pe", {1, 1 + T, d}, 2);
    for (int b = 0; b < NB; ++b) {
        const std::string p = fmt("_tfdec.blocks.%d.", b);
        add_param(p + "self_attn_layer_norm.weight", {d}, 2); add_param(p + "self_attn_layer_norm.bias", {d}, 2);
        for (const char* q : {"q", "k", "v", "o"}) add_param(p + "self_attn.proj_" + q + ".weight", {d, d}, 2);
        add_param(p + "encoder_decoder_attn_layer_norm.weight", {d}, 2); add_param(p + "encoder_decoder_attn_layer_norm.bias", {d}, 2);
        for (const char* q : {"q", "k", "v", "o"}) add_param(p + "encoder_decoder_attn.proj_" + q + ".weight", {d, d}, 2);
        add_param(p + "ffn_layer_norm.weight", {d}, 2); add_param(p + "ffn_layer_norm.bias", {d}, 2);
        add_param(p + "ffn.0.weight", {4 * d, d}, 2); add_param(p + "ffn.0.bias", {4 * d}, 2);
        add_param(p + "ffn.2.weight", {d, 4 * d}, 2); add_param(p + "ffn.2.bias", {d}, 2);
    }
    add_param("_tfdec.layer_norm.weight", {d}, 2); add_param("_tfdec.layer_norm.bias", {d}, 2);
    add_param("_out.weight", {V, d}, 2);

    finish_params(group_begin_, 3);
    resolve_params();
    blk_.resize(NB);
    // what sizes the workspace is asked once, here: the sizing pass and every bind() lay out the same blocks
    conv_x3_ = (int)sw::model<sw::OCRL_CONV_X3>();
    attn_ds_floats_ = attn_bwd_ds_carve_floats(Bmax, T, NH);
    layout_workspace(false);
}

// every name the step path uses, looked up once (a miss is reported by the create call: ModelBase::ref)
void SlateModel::resolve_params() {
    Weights& w = w_;
    for (int i = 0; i < 8; ++i) w.dvae_enc[i] = ref_pair(fmt(i < 7 ? "_dvae._encoder.%d.m" : "_dvae._encoder.%d", i));
    for (int i = 0; i < 12; ++i)
        if (i != 5 && i != 10) w.dvae_dec[i] = ref_pair(fmt(i < 11 ? "_dvae._decoder.%d.m" : "_dvae._decoder.%d", i));
    for (int i = 0; i < 4; ++i) w.enc[i] = ref_pair(fmt(i < 3 ? "_enc._encoder.%d.m" : "_enc._encoder.%d", i));
    w.enc_pos = ref_pair("_enc_pos.channels_map");
    w.sa.mu = ref("_slotattn.slot_mu"); w.sa.log_sigma = ref("_slotattn.slot_log_sigma");
    w.sa.ln = ref_pair("_slotattn.layer_norm"); w.sa.mlp0 = ref_pair("_slotattn.mlp.0"); w.sa.mlp2 = ref_pair("_slotattn.mlp.2");
    for (int i = 0; i < SA_NW; ++i) w.sa.w[i] = ref(std::string("_slotattn.slot_attention.") + SA_WEIGHT_NAMES[i]);
    w.slotproj = ref("_slotproj.weight");
    if (cfg.use_bcdec) {
        for (int i = 0; i < 4; ++i) w.bc[i] = ref_pair(fmt(i < 3 ? "_dec._decoder.%d.m" : "_dec._decoder.%d", i));
        w.bc_pos = ref_pair("_dec._pos_emb.channels_map");
    }
    w.dict = ref("_dict.dictionary.weight"); w.bos = ref("_bos_token._bos_token"); w.pe = ref("_z_pos.pe");
    w.blk.resize(NB);
    for (int b = 0; b < NB; ++b) {
        const std::string p = fmt("_tfdec.blocks.%d.", b);
        DecBlockW& k = w.blk[b];
        k.ln1 = ref_pair(p + "self_attn_layer_norm"); k.ln2 = ref_pair(p + "encoder_decoder_attn_layer_norm"); k.ln3 = ref_pair(p + "ffn_layer_norm");
        k.qkv = ref(p + "self_attn.proj_q.weight"); k.o = ref(p + "self_attn.proj_o.weight");
        k.cq = ref(p + "encoder_decoder_attn.proj_q.weight"); k.ck = ref(p + "encoder_decoder_attn.proj_k.weight");
        k.cv = ref(p + "encoder_decoder_attn.proj_v.weight"); k.co = ref(p + "encoder_decoder_attn.proj_o.weight");
        k.ffn0 = ref_pair(p + "ffn.0"); k.ffn2 = ref_pair(p + "ffn.2");
    }
    w.lnf = ref_pair("_tfdec.layer_norm"); w.out = ref("_out.weight");
    // the encoder tensors end where the slot projection / broadcast decoder begins
    w.enc_grads_end = group_begin_[2];
    for (const ParamInfo& q : params_)
        if (q.group == 1 && (q.name.rfind("_slotproj.", 0) == 0 || q.name.rfind("_dec.", 0) == 0) && q.offset < w.enc_grads_end) w.enc_grads_end = q.offset;
}

SlateModel::~SlateModel() {
    if (ev_fork_) (void)hipEventDestroy(ev_fork_);
    if (ev_join_) (void)hipEventDestroy(ev_join_);
    if (ev_tokens_) (void)hipEventDestroy(ev_tokens_);
    if (side_) (void)hipStreamDestroy(side_);
    for (auto& kv : enc_graphs_) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    for (hipEvent_t e : ev_dw_) if (e) (void)hipEventDestroy(e);
    if (ev_join2_) (void)hipEventDestroy(ev_join2_);
    if (side2_) (void)hipStreamDestroy(side2_);
    if (cap_) (void)hipStreamDestroy(cap_);
}

void SlateModel::layout_workspace(bool commit) {
    begin_layout(commit);
    x3_of_.clear();
    const size_t B = Bmax, BT = B * T, BN = B * N, BK = B * K;
    metrics_ = carve("metrics", 64);
    // transient scratch: split-k slabs (<= 1024 slabs of the largest weight tile set), wgrad slabs, column sums
    scratch_floats_ = 0;
    {
        size_t need = conv_wgrad_ws_floats((int)(B * (cfg.use_bcdec ? K : 1)), S, S, 5, 64) + (size_t)512 * 2304 * 2;
        if (conv_first_wgrad_ws_floats((int)B, S, S) > need) need = conv_first_wgrad_ws_floats((int)B, S, S);
        size_t sk = (size_t)32 * V * d + (size_t)(1 << 20);        // split-k slabs ([V,d] weights x16; 170 slabs of the [4d,d] FFN weights)
        if (sk > need) need = sk;
        size_t cs = (size_t)N * C * 8 + (size_t)T * d * 8 + (1 << 20);   // column-sum partials (pos map / pe)
        if (cs > need) need = cs;
        if (cfg.use_bcdec && bcast_l1_bwd_ws_floats((long long)BK, S, 5) > need) need = bcast_l1_bwd_ws_floats((long long)BK, S, 5);
        const size_t ca = cross_attn_bwd_ws_floats((int)B, T, K, d, NH), eb = embed_bwd_ws_floats((long long)B * T, V, d);
        if (ca > need) need = ca;
        if (eb > need) need = eb;
        scratch_floats_ = need + (1 << 20);
    }
    scratch_ = carve(nullptr, scratch_floats_);
    scratch2_ = cfg.use_bcdec ? scratch_ : carve(nullptr, scratch_floats_);
    // three channels: the first layer reads the NCHW observation itself (csrc/conv_first.hip); obs_keep_ is the copy its weight gradient
    // reads in the backward, so the caller's buffer is free again once the forward has run.  Other channel counts: the NHWC8 copy.
    obs8_ = first_direct() ? nullptr : carve("obs8", BN * 8);
    obs_keep_ = first_direct() ? carve(nullptr, BN * cfg.obs_channels) : nullptr;
    obs_stage_ = carve(nullptr, (B < 32 ? B : 32) * (size_t)cfg.obs_channels * N);
    seed_dev_ = reinterpret_cast<unsigned long long*>(carve(nullptr, 64));
    e1_ = carve("enc1", BN * 64); e2_ = carve("enc2", BN * 64); e3_ = carve("enc3", BN * 64); e4_ = carve("feats", BN * 64);
    posmap_ = carve(nullptr, (size_t)N * C); gridT_ = carve(nullptr, (size_t)N * 4);
    ln0_ = carve(nullptr, BN * 64); ln0_mean_ = carve(nullptr, BN); ln0_rstd_ = carve(nullptr, BN);
    h1_ = carve("sa_mlp_hidden", BN * 64); x_ = carve("sa_inputs", BN * 64);
    slots0_ = carve("slots0", BK * D); slot_noise_ = carve(nullptr, BK * D); slots_ = carve("slots", BK * D);
    attn_ = carve("attn", BN * K);
    attn_heads_ = SH > 1 ? carve(nullptr, sa_attn_heads_floats(B, N, K, SH)) : nullptr;
    const SaSizes sz = sa_sizes(B, K, C, D, H, I, SH);
    sa_save_ = carve("sa_save", sz.save);
    sa_grows_ = carve(nullptr, sz.grows);
    sa_wts_ = carve(nullptr, sz.wts);
    sa_small_ = carve(nullptr, sz.small);
    sa_xchg_ = carve(nullptr, sz.xchg);
    sa_parts_ = carve(nullptr, sz.parts);
    sa_pack_dev_ = reinterpret_cast<PackEntry*>(carve(nullptr, sz.table));
    for (int i = 0; i < 4; ++i) {
        const int cin = i == 0 ? 8 : 64;
        cw_fwd_[i] = carve(nullptr, (size_t)25 * cin * 64);
        cw_bwd_[i] = i == 0 ? nullptr : carve(nullptr, (size_t)25 * 64 * 64);
        if (conv_x3_ && i > 0) {          // exploratory split-precision packs beside the fp32 ones (csrc/conv_x3.hip)
            float* f3 = carve(nullptr, conv_x3_pack_floats());
            float* b3 = carve(nullptr, conv_x3_pack_floats());
            if (ws_commit_) { x3_of_[cw_fwd_[i]] = f3; x3_of_[cw_bwd_[i]] = b3; }
        }
    }
    gslots_ = carve(nullptr, BK * D); gslots0_ = carve(nullptr, BK * D);
    gA_ = carve(nullptr, BN * 64); gB_ = carve(nullptr, BN * 64); gC_ = cfg.use_bcdec ? gA_ : carve(nullptr, BN * 64);
    gmap_ = carve(nullptr, (size_t)N * C);
    if (cfg.use_bcdec) {
        const size_t BKN = BK * (size_t)N;
        bc_Wc_ = carve(nullptr, 25 * 64 * 5 + 64); bc_W1r_ = carve(nullptr, (size_t)25 * 64 * D); bc_P1_ = carve(nullptr, (size_t)N * 64);
        bc_M_ = carve(nullptr, BK * 1600); bc_T_ = carve(nullptr, BK * 1600);
        bc_c1_ = carve("bc_c1", BKN * 64); bc_c2_ = carve("bc_c2", BKN * 64); bc_c3_ = carve("bc_c3", BKN * 64);
        bc_out4_ = carve(nullptr, BKN * 4); bc_dout4_ = carve(nullptr, BKN * 4);
        bc_gA_ = carve(nullptr, BKN * 64); bc_gB_ = carve(nullptr, BKN * 64);
        for (int i = 0; i < 2; ++i) {
            bc_pk_[i] = carve(nullptr, 25 * 64 * 64); bc_pkb_[i] = carve(nullptr, 25 * 64 * 64);
            if (conv_x3_ > 0) {           // exploratory split-precision packs of the broadcast decoder's 5x5 / 64-channel layers
                float* f3 = carve(nullptr, conv_x3_pack_floats());
                float* b3 = carve(nullptr, conv_x3_pack_floats());
                if (ws_commit_) { x3_of_[bc_pk_[i]] = f3; x3_of_[bc_pkb_[i]] = b3; }
            }
        }
        bc_Wk4_ = carve(nullptr, 9 * 64 * 4); bc_Wb4_ = carve(nullptr, 9 * 64 * 4);
        bc_dW1r_ = carve(nullptr, (size_t)25 * 64 * D); bc_dWc_ = carve(nullptr, 25 * 64 * 5 + 64);
        bc_dT_ = carve(nullptr, BK * 1600); bc_dM_ = carve(nullptr, BK * 1600); bc_G1_ = carve(nullptr, (size_t)N * 64);
        recon_ = carve("recon", BN * 4);
    } else {
    patches_ = carve("patches", BT * 16 * cfg.obs_channels);
    for (int i = 0; i < 7; ++i) de_[i] = carve(fmt("dvae_enc%d", i).c_str(), BT * 64);
    zraw_ = carve("zraw", BT * V);
    z_ = carve("z", BT * V);
    zdec_ = cfg.hard ? carve("z_st", BT * V) : z_;
    tokens_ = reinterpret_cast<int*>(carve("tokens", BT));
    // soft-max heads fused into the vocabulary GEMMs: per-row / per-segment statistics (gemm.hip epi_mode 1-3)
    {
        const size_t nseg = (size_t)gemm_stat_segments(V);
        zstat_ = carve(nullptr, BT * nseg * 2); zhstat_ = carve(nullptr, BT * nseg); zhidx_ = reinterpret_cast<int*>(carve(nullptr, BT * nseg));
        zlse_ = carve("z_lse", BT); zdot_ = carve(nullptr, BT);
        cestat_ = carve(nullptr, BT * nseg * 2); celse_ = carve("ce_lse", BT); cepart_ = carve(nullptr, BT / 16 + 16);
    }
    // post-activation outputs of the dVAE decoder blocks (named: the parity tests read their ReLU masks)
    dd0_ = carve("dvae_dec0", BT * 64); dd1_ = carve("dvae_dec1", BT * 64); dd2_ = carve("dvae_dec2", BT * 64); dd3_ = carve("dvae_dec3", BT * 64);
    dd4_ = carve("dvae_dec4", BT * 256); ps1_ = carve(nullptr, BT * 256);
    dd6_ = carve("dvae_dec6", BT * 256); dd7_ = carve("dvae_dec7", BT * 256); dd8_ = carve("dvae_dec8", BT * 256);
    dd9_ = carve("dvae_dec9", BT * 1024); ps2_ = carve(nullptr, BN * 64);
    recon_ = carve("recon", BN * 4); drecon_ = carve(nullptr, BN * 4);
    for (int i = 0; i < 2; ++i) {
        dw_fwd_[i] = carve(nullptr, 9 * 64 * 64); dw_bwd_[i] = carve(nullptr, 9 * 64 * 64);
        if (conv_x3_ > 0) {           // exploratory split-precision packs of the dVAE decoder's 3x3 / 64-channel layers
            float* f3 = carve(nullptr, conv_x3_pack_floats(3));
            float* b3 = carve(nullptr, conv_x3_pack_floats(3));
            if (ws_commit_) { x3_of_[dw_fwd_[i]] = f3; x3_of_[dw_bwd_[i]] = b3; }
        }
    }
    w11p_ = carve(nullptr, 4 * 64);
    mem_ = carve("mem", BK * d); emb_ = carve("emb", BT * d);
    for (int b = 0; b < NB; ++b) {
        Blk& k = blk_[b];
        k.ln1 = carve(nullptr, BT * d); k.ln1_mean = carve(nullptr, BT); k.ln1_rstd = carve(nullptr, BT);
        k.q = carve(nullptr, BT * 3 * d); k.k = k.q + d; k.v = k.q + 2 * d;      // fused [BT, 3d] projection output
        k.lse = carve(nullptr, B * NH * (size_t)T); k.ao = carve(nullptr, BT * d); k.x1 = carve(nullptr, BT * d);
        k.ln2 = carve(nullptr, BT * d); k.ln2_mean = carve(nullptr, BT); k.ln2_rstd = carve(nullptr, BT);
        k.cq = carve(nullptr, BT * d); k.ck = carve(nullptr, BK * d); k.cv = carve(nullptr, BK * d);
        k.cP = carve(nullptr, B * NH * (size_t)T * K); k.cao = carve(nullptr, BT * d); k.x2 = carve(nullptr, BT * d);
        k.ln3 = carve(nullptr, BT * d); k.ln3_mean = carve(nullptr, BT); k.ln3_rstd = carve(nullptr, BT);
        k.f1 = carve(fmt("blk%d.ffn_hidden", b).c_str(), BT * 4 * d); k.x3 = carve(nullptr, BT * d);
    }
    bg_.resize(NB);
    {   // folded cross attention (xattn.hip)
        const size_t NC = xattn_supported(K, d, NH) ? (size_t)NH * xattn_kp(K, NH) : 16;
        xa_zero_base_ = carve_pos();
        for (int b = 0; b < NB; ++b) {
            Blk& k = blk_[b];
            k.xaAb = carve(nullptr, B * NC * d); k.xaAbT = carve(nullptr, B * NC * d); k.xaVo = carve(nullptr, B * NC * d); k.xaVoT = carve(nullptr, B * NC * d);
        }
        xa_zero_floats_ = (size_t)(carve_pos() - xa_zero_base_);
        for (int b = 0; b < NB; ++b) { bg_[b].xaPd = carve(nullptr, BT * NC); bg_[b].xaDs = carve(nullptr, BT * NC); }
        xa_dAb_ = carve(nullptr, B * NC * d); xa_dVo_ = carve(nullptr, B * NC * d);
        xa_pq_ = carve(nullptr, B * (size_t)d * d); xa_po_ = carve(nullptr, B * (size_t)d * d);
    }
    attn_delta_ = carve(nullptr, B * NH * (size_t)T);
    // dS workspace of the self-attention backward's hand-off form (attn_bwd_ds_carve_floats, csrc/attention.hip), one for the NB blocks,
    // which run in sequence on the main stream: at T = 1024 the whole batch of 128 (1.14 GB) is one chunk, at T = 4096 (136 MB per
    // image) a chunk is 15 images
    attn_ds_ = attn_ds_floats_ ? carve(nullptr, attn_ds_floats_) : nullptr;
    lnf_ =carve("dec_out", BT * d); lnf_mean_ = carve(nullptr, BT); lnf_rstd_ = carve(nullptr, BT);
    pred_ = carve("pred", BT * V);
    gx_ = carve(nullptr, BT * d); gbr_ = carve(nullptr, BT * d); gt1_ = carve(nullptr, BT * d); gt2_ = carve(nullptr, BT * d);
    gt3_ = carve(nullptr, BT * d); gf1_ = carve(nullptr, BT * 4 * d); gqkv_ = carve(nullptr, BT * 3 * d);
    for (int b = 0; b < NB; ++b) {
        BlkG& q = bg_[b];
        if (b == 0) { q.gbr[0] = gbr_; q.gf1 = gf1_; q.gt2 = gt2_; q.gqkv = gqkv_; }
        else { q.gbr[0] = carve(nullptr, BT * d); q.gf1 = carve(nullptr, BT * 4 * d); q.gt2 = carve(nullptr, BT * d); q.gqkv = carve(nullptr, BT * 3 * d); }
        q.gbr[1] = carve(nullptr, BT * d); q.gbr[2] = carve(nullptr, BT * d);
    }
    scratch3_ = carve(nullptr, scratch_floats_);
    gmem_ = carve(nullptr, BK * d); gck_ = carve(nullptr, BK * d); gcv_ = carve(nullptr, BK * d);
    gdA_ = carve(nullptr, BN * 64); gdB_ = carve(nullptr, BN * 64);
    }
    col0_ = dw0p_ = nullptr;
    if (!first_direct()) {      // the first layer's weight gradient as a product with the patch matrix
        const int ldc0 = (25 * cfg.obs_channels + 3) & ~3;
        col0_ = carve(nullptr, BN * ldc0); dw0p_ = carve(nullptr, (size_t)64 * ldc0);
    }
    end_layout();
}

int SlateModel::bind(float* p, float* g, float* m, float* v, void* ws, size_t ws_bytes) {
    RC(check_buffers(p, g, ws, ws_bytes));
    OCRL_REQUIRE(d % 64 == 0 && d <= 256 && D % 64 == 0 && C == 64 && V % 256 == 0 && S % 4 == 0 && d % NH == 0 && DH % 4 == 0 && DH <= 64,
                 "unsupported configuration (d_model/slot_size multiples of 64 <= 256, cnn hidden 64, vocab %% 256, obs_size %% 4)");
    OCRL_REQUIRE(cfg.obs_channels == 3, "obs_channels must be 3");
    OCRL_REQUIRE(T % 4 == 0, "obs_size/4 squared must be a multiple of 4");
    adopt_buffers(p, g, m, v, ws);
    clear_encode_graphs();       // captured against the old buffers
    packs_valid_ = false;
    layout_workspace(true);
    if (!side_) {       // the first bind (a single-stream plan creates nothing, and is asked for again)
        plan_ = stream_plan((int)sw::model<sw::OCRL_OVERLAP>(), (int)sw::model<sw::OCRL_DW_SIDE>(), sw::model<sw::OCRL_TOKENS_LATE>() != 0, cfg.use_bcdec);
        if (plan_.side) {
            OCRL_HIP(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
            OCRL_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
            OCRL_HIP(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
            OCRL_HIP(hipEventCreateWithFlags(&ev_tokens_, hipEventDisableTiming));
            // the weight-gradient products of the transformer decoder leave the main stream: nothing later in the step reads them,
            // while the input-gradient chain they would otherwise interrupt is the step's critical path
            if (plan_.dw) {
                for (hipEvent_t& ev : ev_dw_) OCRL_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                OCRL_HIP(hipEventCreateWithFlags(&ev_join2_, hipEventDisableTiming));
                if (plan_.dw == 2) OCRL_HIP(hipStreamCreateWithFlags(&side2_, hipStreamNonBlocking));
            }
        }
    }
    // the slot-attention input LayerNorm + MLP as one kernel per direction (csrc/sa_input.hip), or the unfused chain: LayerNorm, two
    // GEMMs; five launches and their reduction tails backward
    sa_input_ = (int)sw::model<sw::OCRL_SA_INPUT>();
    xattn_ = !cfg.use_bcdec && xattn_supported(K, d, NH) && sw::model<sw::OCRL_XATTN>() != 0;
    if (!cfg.use_bcdec && xa_zero_floats_) OCRL_HIP(hipMemset(xa_zero_base_, 0, xa_zero_floats_ * sizeof(float)));      // padding columns of the folded operands
    // static tables
    RC(posgrid_launch(gridT_, S, 0));
    RC(fill_launch(recon_, (long long)Bmax * N * 4, 0.f, 0));
    // slot-attention weight pack table
    const float* saw[SA_NW];
    for (int i = 0; i < SA_NW; ++i) saw[i] = P(w_.sa.w[i]);
    PackEntry ent[SA_PACK_ENTRIES];
    sa_pack_n_ = sa_pack_table(saw, C, D, H, ent, &sa_pack_max_);
    OCRL_HIP(hipMemcpy(sa_pack_dev_, ent, sa_pack_n_ * sizeof(PackEntry), hipMemcpyHostToDevice));
    OCRL_HIP(hipDeviceSynchronize());
    have_fwd_ = false;
    return 0;
}

int SlateModel::soft_z(hipStream_t st) {
    if (!fused_heads() || cfg.use_bcdec) return 0;          // z_ is written by the forward itself
    OCRL_REQUIRE(have_scores_, "soft_z: no forward since the last backward (the scores have been overwritten by their gradient)");
    return exp_rows_launch(zraw_, zlse_, z_, (long long)last_.B * T, V, st);
}
int SlateModel::dropout_mask(unsigned site, long long n, float* out, hipStream_t st) const {
    return dropout_mask_launch(out, n, pdrop_, last_.seed, site, st);
}

int SlateModel::conv_layer_fwd(const float* x, const float* pack, const float* bias, float* y, int Bn, int Hh, int Ww, int KS, int CIN,
                               int relu, const float* posmap, const float* mask, const Lane& L) {
    ConvArgs a;
    a.X = x; a.Wp = pack; a.Y = y; a.B = Bn; a.H = Hh; a.W = Ww; a.bias = bias; a.relu = relu; a.posmap = posmap; a.mask = mask;
    if (conv_x3_ > 0 && (KS == 5 || KS == 3) && CIN == 64 && !conv_lowlat_) {
        auto it = x3_of_.find(pack);
        if (it != x3_of_.end()) return conv_x3_launch(a, it->second, L, KS);
    }
    return conv_fwd_launch(a, KS, CIN, 64, L, conv_lowlat_);
}
int SlateModel::conv_layer_wgrad(const float* x, const float* dy, float* dW, float* db, int Bn, int Hh, int Ww, int KS, int CIN,
                                 int cin_real, const Lane& L) {
    WgradArgs a;
    a.X = x; a.dY = dy; a.part = L.scratch; a.B = Bn; a.H = Hh; a.W = Ww;
    OCRL_REQUIRE(conv_wgrad_ws_floats(Bn, Hh, Ww, KS, CIN) <= L.scratch_floats, "conv wgrad: scratch too small");
    // the bias gradient comes out of the weight-gradient kernel (it sums the dY fragments it feeds to the MFMAs); the exploratory
    // split-precision stage has no such sum and keeps the column-sum pass over dY
    const bool x3 = conv_x3_ > 0 && CIN == 64;
    RC(conv_wgrad_launch(a, KS, CIN, 64, cin_real, dW, x3 ? nullptr : db, 0, L, x3 ? 1 : 0));
    if (db && x3) RC(colsum_launch(dy, 64, db, (long long)Bn * Hh * Ww, 64, 0, 1.f, L.scratch, L.scratch_floats, L));
    return 0;
}

int SlateModel::pack_weights(const Lane& L, bool encoder_only) {
    if (first_direct()) RC(conv_first_pack_launch(P(w_.enc[0].w), cw_fwd_[0], L));
    else RC(conv_pack_launch(P(w_.enc[0].w), cw_fwd_[0], nullptr, 5, 8, 64, cfg.obs_channels, L));
    RC(conv_pack_launch(P(w_.enc[1].w), cw_fwd_[1], cw_bwd_[1], 5, 64, 64, 64, L));
    RC(conv_pack_launch(P(w_.enc[2].w), cw_fwd_[2], cw_bwd_[2], 5, 64, 64, 64, L));
    RC(conv_pack_launch(P(w_.enc[3].w), cw_fwd_[3], cw_bwd_[3], 5, 64, 64, 64, L));
    if (conv_x3_ > 0) {
        for (int i = 1; i < 4; ++i) {
            auto f = x3_of_.find(cw_fwd_[i]), b = x3_of_.find(cw_bwd_[i]);
            if (f != x3_of_.end()) RC(conv_pack_x3_launch(P(w_.enc[i].w), const_cast<float*>(f->second), b != x3_of_.end() ? const_cast<float*>(b->second) : nullptr, L));
        }
    }
    if (!cfg.use_bcdec && !encoder_only) {
        RC(conv_pack_launch(P(w_.dvae_dec[1].w), dw_fwd_[0], dw_bwd_[0], 3, 64, 64, 64, L));
        RC(conv_pack_launch(P(w_.dvae_dec[6].w), dw_fwd_[1], dw_bwd_[1], 3, 64, 64, 64, L));
        if (conv_x3_ > 0) {
            for (int i = 0; i < 2; ++i) {
                auto f = x3_of_.find(dw_fwd_[i]), b = x3_of_.find(dw_bwd_[i]);
                if (f != x3_of_.end()) RC(conv_pack_x3_launch(P(w_.dvae_dec[i ? 6 : 1].w), const_cast<float*>(f->second), b != x3_of_.end() ? const_cast<float*>(b->second) : nullptr, L, 3));
            }
        }
        RC(copy_launch(P(w_.dvae_dec[11].w), w11p_, cfg.obs_channels * 64, L));    // [3,64] -> [4,64], row 3 zero
        RC(fill_launch(w11p_ + cfg.obs_channels * 64, (4 - cfg.obs_channels) * 64, 0.f, L));
    }
    RC(pack_launch(sa_pack_dev_, sa_pack_n_, sa_pack_max_, sa_wts_, L));
    RC(posmap_launch(P(w_.enc_pos.w), P(w_.enc_pos.b), posmap_, S, C, L));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// CNN encoder + slot attention (ocrs/common/models.py:96-107, slot_attn.py:147-161)
int SlateModel::fwd_encoder(const StepInputs& in, const Lane& L, FwdDvae fork) {
    const int B = in.B;
    const long long BN = (long long)B * N;
    auto fork_if = [&](FwdDvae here) -> int {
        if (fork != here) return 0;
        RC(after(dvae_lane(), L, ev_fork_));
        return fwd_dvae(in, dvae_lane());
    };
    // slot initialisation and the preparation launch of the slot-attention chain (LayerNorm, q, folded query of iteration 0) need the
    // weights and the noise only: issued first, they run on an otherwise idle machine.  After the fork their whole-CU-LDS workgroups
    // queue behind the Gumbel head's 32 768 small workgroups on the side stream (measured: 1.46 ms instead of 60 us, on the critical
    // path of the decoder)
    RC(slot_init_launch(P(w_.sa.mu), P(w_.sa.log_sigma), in.noise_slots, slots0_, B * K, D, in.seed, L, in.seed_dev));
    SlotAttnArgs a = sa_args(B, N, K, D, H, I, SH);
    a.x = x_; a.slots0 = slots0_; a.wts = sa_wts_; a.slots = slots_; a.attn = attn_; a.attn_heads = attn_heads_; a.save = sa_save_;
    if (conv_lowlat_ && frozen_) a.save = nullptr;       // encode() of a frozen encoder: no backward can follow, the saved-activation rows are not written
    a.xchg = sa_xchg_; a.parts = sa_parts_;
    a.phase = 1;
    RC(slot_attn_launch(a, 0, L));
    RC(fork_if(FwdDvae::AtStart));
    if (first_direct()) {
        RC(conv_first_fwd_launch(in.obs, cw_fwd_[0], P(w_.enc[0].b), e1_, B, S, S, 1, L));
        if (!(conv_lowlat_ && frozen_))       // a backward may follow: it reads the observation again
            OCRL_HIP(hipMemcpyAsync(obs_keep_, in.obs, (size_t)BN * cfg.obs_channels * sizeof(float), hipMemcpyDeviceToDevice, L));
    } else {
        RC(nchw_to_nhwc8_launch(in.obs, obs8_, B, cfg.obs_channels, S, S, L));
        RC(conv_layer_fwd(obs8_, cw_fwd_[0], P(w_.enc[0].b), e1_, B, S, S, 5, 8, 1, nullptr, nullptr, L));
    }
    RC(conv_layer_fwd(e1_, cw_fwd_[1], P(w_.enc[1].b), e2_, B, S, S, 5, 64, 1, nullptr, nullptr, L));
    RC(conv_layer_fwd(e2_, cw_fwd_[2], P(w_.enc[2].b), e3_, B, S, S, 5, 64, 1, nullptr, nullptr, L));
    RC(conv_layer_fwd(e3_, cw_fwd_[3], P(w_.enc[3].b), e4_, B, S, S, 5, 64, 0, posmap_, nullptr, L));
    RC(fork_if(FwdDvae::AfterConvs));
    if (sa_input_ && C == 64 && !(conv_lowlat_ && frozen_)) {
        // LayerNorm and both Linear layers in one pass over the rows (csrc/sa_input.hip): e4 is read, h1 and x are written; the fused
        // backward rebuilds LN(e4) from e4, mean and rstd, so ln0_ is written only for the unfused backward (OCRL_SA_INPUT=2)
        RC(sa_input_fwd_launch(e4_, P(w_.sa.ln.w), P(w_.sa.ln.b), P(w_.sa.mlp0.w),
                               P(w_.sa.mlp0.b), P(w_.sa.mlp2.w), P(w_.sa.mlp2.b), ln0_mean_, ln0_rstd_,
                               sa_input_ == 2 ? ln0_ : nullptr, h1_, x_, BN, 0, L));
    } else {
        RC(layernorm_fwd_launch(e4_, P(w_.sa.ln.w), P(w_.sa.ln.b), ln0_, ln0_mean_, ln0_rstd_, BN, C, L));
        RC(lin_fwd(ln0_, C, P(w_.sa.mlp0.w), P(w_.sa.mlp0.b), h1_, C, BN, C, C, 1, nullptr, 0, 0.f, 0, L));
        RC(lin_fwd(h1_, C, P(w_.sa.mlp2.w), P(w_.sa.mlp2.b), x_, C, BN, C, C, 0, nullptr, 0, 0.f, 0, L));
    }
    RC(fork_if(FwdDvae::AtSlotAttention));
    a.phase = 2;
    RC(slot_attn_launch(a, 0, L));
    return 0;
}

// dVAE encode -> Gumbel softmax -> decode -> reconstruction loss (models.py:14-45, utils.py:75-85)
int SlateModel::fwd_dvae(const StepInputs& in, const Lane& L) {
    const int B = in.B;
    const long long BT = (long long)B * T, BN = (long long)B * N;
    const int ch = cfg.obs_channels;
    RC(patchify4_launch(in.obs, patches_, B, ch, S, L));
    RC(lin_fwd(patches_, 16 * ch, P(w_.dvae_enc[0].w), P(w_.dvae_enc[0].b), de_[0], 64, BT, 64, 16 * ch, 1, nullptr, 0, 0.f, 0, L));
    for (int i = 1; i < 7; ++i)
        RC(lin_fwd(de_[i - 1], 64, P(w_.dvae_enc[i].w), P(w_.dvae_enc[i].b), de_[i], 64, BT, 64, 64, 1, nullptr, 0, 0.f, 0, L));
    if (fused_heads()) {
        // 64 -> vocabulary head with both Gumbel samples in its epilogue (ocrs/slate/slate_module.py:125-127, ocrs/common/utils.py:72-85):
        // zraw_ <- (logits + g1) / tau, the soft sample's scores.  z = softmax(zraw_) is never written: the decoder product and the
        // backward rebuild it from zraw_ and z_lse while staging their operand tiles.  (The reference adds the noise to
        // log_softmax(logits); the row shift cancels in the soft-max and in the argmax.)
        GemmArgs a;
        a.A = de_[6]; a.B = P(w_.dvae_enc[7].w); a.C = zraw_; a.M = (int)BT; a.N = V; a.K = 64; a.lda = 64; a.ldb = 64; a.ldc = V;
        a.bias = P(w_.dvae_enc[7].b);
        a.epi_mode = 2; a.stat = zstat_; a.hstat = zhstat_; a.hidx = zhidx_; a.e1 = in.noise_z; a.e2 = in.noise_zh; a.e_seed = in.seed;
        a.e_scale = 1.0f / in.tau;
        RC(gemm_launch(a, L));
        // hard sample: with injected noise the arg-max of l + g2 (segment maxima from the epilogue); with the device RNG a draw from
        // Categorical(soft-max(l)) by inverse CDF over the segment masses (one pair of uniforms per row instead of a Gumbel draw per entry)
        RC(softmax_stat_combine_launch(zstat_, gemm_stat_segments(V), BT, zlse_, zhstat_, zhidx_, tokens_, nullptr, 0, nullptr, nullptr, 0.f, nullptr, 0, L,
                                       in.noise_z ? nullptr : zraw_, V, in.tau, in.seed));
        have_scores_ = true;
    } else {
    RC(lin_fwd(de_[6], 64, P(w_.dvae_enc[7].w), P(w_.dvae_enc[7].b), zraw_, V, BT, V, 64, 0, nullptr, 0, 0.f, 0, L));
    RC(gumbel_softmax_launch(zraw_, in.noise_z, in.noise_zh, z_, tokens_, BT, V, in.tau, in.seed, L, cfg.hard ? zdec_ : nullptr));
    }
    // the transformer decoder only needs the tokens: it may start on the main stream while the dVAE decoder and the reconstruction loss
    // are still running here (tokens_early mode of forward())
    if (side_ && L.st == side_ && ev_tokens_) OCRL_HIP(hipEventRecord(ev_tokens_, L.st));
    RC(dvae_decode(B, drecon_, L));
    return 0;
}

// dVAE decoder on z_ -> recon_ (ocrs/common/models.py:24-37,44-45) and the reconstruction loss into metrics[0]
int SlateModel::dvae_decode(int B, float* drecon, const Lane& L, const float* zin) {
    const long long BT = (long long)B * T, BN = (long long)B * N;
    const int ch = cfg.obs_channels;
    // decoder
    if (!zin && fused_heads()) {
        GemmArgs a;        // A = softmax(zraw_) rebuilt on the fly
        a.A = zraw_; a.B = P(w_.dvae_dec[0].w); a.C = dd0_; a.M = (int)BT; a.N = 64; a.K = V; a.lda = V; a.ldb = V; a.ldc = 64;
        a.bias = P(w_.dvae_dec[0].b); a.relu = 1; a.a_mode = 2; a.x_lse = zlse_;
        RC(gemm_launch(a, L));
    } else {
    if (!zin) zin = zdec_;
    RC(lin_fwd(zin, V, P(w_.dvae_dec[0].w), P(w_.dvae_dec[0].b), dd0_, 64, BT, 64, V, 1, nullptr, 0, 0.f, 0, L));
    }
    RC(conv_layer_fwd(dd0_, dw_fwd_[0], P(w_.dvae_dec[1].b), dd1_, B, E, E, 3, 64, 1, nullptr, nullptr, L));
    RC(lin_fwd(dd1_, 64, P(w_.dvae_dec[2].w), P(w_.dvae_dec[2].b), dd2_, 64, BT, 64, 64, 1, nullptr, 0, 0.f, 0, L));
    RC(lin_fwd(dd2_, 64, P(w_.dvae_dec[3].w), P(w_.dvae_dec[3].b), dd3_, 64, BT, 64, 64, 1, nullptr, 0, 0.f, 0, L));
    RC(lin_fwd(dd3_, 64, P(w_.dvae_dec[4].w), P(w_.dvae_dec[4].b), dd4_, 256, BT, 256, 64, 1, nullptr, 0, 0.f, 0, L));
    RC(pixel_shuffle_launch(dd4_, ps1_, B, E, E, 64, 1, nullptr, L));
    RC(conv_layer_fwd(ps1_, dw_fwd_[1], P(w_.dvae_dec[6].b), dd6_, B, 2 * E, 2 * E, 3, 64, 1, nullptr, nullptr, L));
    RC(lin_fwd(dd6_, 64, P(w_.dvae_dec[7].w), P(w_.dvae_dec[7].b), dd7_, 64, 4 * BT, 64, 64, 1, nullptr, 0, 0.f, 0, L));
    RC(lin_fwd(dd7_, 64, P(w_.dvae_dec[8].w), P(w_.dvae_dec[8].b), dd8_, 64, 4 * BT, 64, 64, 1, nullptr, 0, 0.f, 0, L));
    RC(lin_fwd(dd8_, 64, P(w_.dvae_dec[9].w), P(w_.dvae_dec[9].b), dd9_, 256, 4 * BT, 256, 64, 1, nullptr, 0, 0.f, 0, L));
    RC(pixel_shuffle_launch(dd9_, ps2_, B, 2 * E, 2 * E, 64, 1, nullptr, L));
    RC(lin_fwd(ps2_, 64, P(w_.dvae_dec[11].w), P(w_.dvae_dec[11].b), recon_, 4, BN, ch, 64, 0, nullptr, 0, 0.f, 0, L));
    RC(mse_launch(last_.obs, recon_, drecon, metrics_ + (drecon ? 0 : 4), B, ch, S, S, L.scratch, L.scratch_floats, L));
    return 0;
}

AttnArgs SlateModel::self_attn_args(int b) const {
    const Blk& k = blk_[b];
    AttnArgs a;
    a.q = k.q; a.k = k.k; a.v = k.v; a.o = k.ao; a.lse = k.lse; a.B = last_.B; a.T = T; a.d = d; a.h = NH; a.ld = 3 * d;
    a.p = pdrop_; a.seed = last_.seed; a.site = SITE_BLK_BASE + 8 * b + 0;
    return a;
}
XaHost SlateModel::xattn_args(int b) const {
    const Blk& k = blk_[b];
    const unsigned site = SITE_BLK_BASE + 8 * b;
    XaHost hx;
    hx.x = k.ln2; hx.P = k.cP; hx.Ab = k.xaAb; hx.AbT = k.xaAbT; hx.Vo = k.xaVo; hx.VoT = k.xaVoT;
    hx.B = last_.B; hx.T = T; hx.K = K; hx.d = d; hx.h = NH; hx.p = pdrop_; hx.seed = last_.seed; hx.site_p = site + 2; hx.site_o = site + 3;
    return hx;
}

// token embedding + transformer decoder + cross entropy (slate_module.py:141-156, transformer.py)
int SlateModel::fwd_decoder(const Lane& L, bool with_ce) {
    const int B = last_.B;
    const long long BT = (long long)B * T;
    const float p = pdrop_;
    RC(lin_fwd(slots_, D, P(w_.slotproj), nullptr, mem_, d, (long long)B * K, d, D, 0, nullptr, 0, 0.f, 0, L));
    RC(embed_fwd_launch(tokens_, P(w_.dict), P(w_.bos), P(w_.pe), emb_, B, T, d, p, last_.seed, L));
    // The fold below only needs the projected slots and is first consumed by block 0's cross attention, after the embedding, a LayerNorm,
    // the q|k|v projection and the self attention: on the (idle) weight-gradient stream it runs beside them
    const Lane F = plan_.dw == 2 ? dw_lane(L) : L;
    if (xattn_) {       // per-image cross-attention operands of every block from the projected slots: one launch
        XaFoldHost f;
        f.mem = mem_; f.B = B; f.K = K; f.d = d; f.h = NH; f.nblk = NB;
        OCRL_REQUIRE(NB <= 8, "more than 8 decoder blocks: set OCRL_XATTN=0");
        for (int b = 0; b < NB; ++b) {
            const DecBlockW& bw = w_.blk[b];
            f.Wq[b] = P(bw.cq); f.Wk[b] = P(bw.ck); f.Wv[b] = P(bw.cv); f.Wo[b] = P(bw.co);
            f.ck[b] = blk_[b].ck; f.cv[b] = blk_[b].cv; f.Ab[b] = blk_[b].xaAb; f.AbT[b] = blk_[b].xaAbT; f.Vo[b] = blk_[b].xaVo; f.VoT[b] = blk_[b].xaVoT;
        }
        RC(after(F, L, ring_event()));
        RC(xattn_fold_fwd_launch(f, F));
    }
    const float* xin = emb_;
    for (int b = 0; b < NB; ++b) {
        Blk& k = blk_[b];
        const DecBlockW& bw = w_.blk[b];
        const unsigned site = SITE_BLK_BASE + 8 * b;
        RC(layernorm_fwd_launch(xin, P(bw.ln1.w), P(bw.ln1.b), k.ln1, k.ln1_mean, k.ln1_rstd, BT, d, L));
        const float* res = (b == 0) ? k.ln1 : xin;      // block 0 normalises the residual stream itself (transformer.py:175-178)
        // proj_q / proj_k / proj_v are adjacent in the flat buffer: one [3d, d] weight, one GEMM
        RC(lin_fwd(k.ln1, d, P(bw.qkv), nullptr, k.q, 3 * d, BT, 3 * d, d, 0, nullptr, 0, 0.f, 0, L));
        {   // causal self attention, flash style (scores never leave the chip)
            const AttnArgs a = self_attn_args(b);
            RC(attn_launch(a, 0, L));
        }
        RC(lin_fwd(k.ao, d, P(bw.o), nullptr, k.x1, d, BT, d, d, 0, res, d, p, site + 1, L));
        // cross attention to the projected slots
        RC(layernorm_fwd_launch(k.x1, P(bw.ln2.w), P(bw.ln2.b), k.ln2, k.ln2_mean, k.ln2_rstd, BT, d, L));
        if (xattn_) {       // folded form: scores, soft-max, dropout, output, dropout and the residual add in one launch (xattn.hip)
            if (b == 0) RC(after(L, F, ev_join2_));       // the folded operands are ready (nothing else went to F since the fold)
            XaHost hx = xattn_args(b);
            hx.resid = k.x1; hx.y = k.x2;
            RC(xattn_launch(hx, 0, L));
        } else {
        RC(lin_fwd(k.ln2, d, P(bw.cq), nullptr, k.cq, d, BT, d, d, 0, nullptr, 0, 0.f, 0, L));
        RC(lin_fwd(mem_, d, P(bw.ck), nullptr, k.ck, d, (long long)B * K, d, d, 0, nullptr, 0, 0.f, 0, L));
        RC(lin_fwd(mem_, d, P(bw.cv), nullptr, k.cv, d, (long long)B * K, d, d, 0, nullptr, 0, 0.f, 0, L));
        RC(cross_attn_fwd_launch(k.cq, k.ck, k.cv, k.cao, k.cP, B, T, K, d, NH, p, last_.seed, site + 2, L));
        RC(lin_fwd(k.cao, d, P(bw.co), nullptr, k.x2, d, BT, d, d, 0, k.x1, d, p, site + 3, L));
        }
        // feed forward
        RC(layernorm_fwd_launch(k.x2, P(bw.ln3.w), P(bw.ln3.b), k.ln3, k.ln3_mean, k.ln3_rstd, BT, d, L));
        RC(lin_fwd(k.ln3, d, P(bw.ffn0.w), P(bw.ffn0.b), k.f1, 4 * d, BT, 4 * d, d, 1, nullptr, 0, 0.f, 0, L));
        RC(lin_fwd(k.f1, 4 * d, P(bw.ffn2.w), P(bw.ffn2.b), k.x3, d, BT, d, 4 * d, 0, k.x2, d, p, site + 4, L));
        xin = k.x3;
    }
    RC(layernorm_fwd_launch(xin, P(w_.lnf.w), P(w_.lnf.b), lnf_, lnf_mean_, lnf_rstd_, BT, d, L));
    if (with_ce) {
        // vocabulary head with the cross-entropy statistics in its epilogue (ocrs/slate/slate_module.py:150-156): pred_ keeps the
        // logits; the gradient (softmax - onehot) / B is rebuilt from pred_ and ce_lse while the backward products stage it
        GemmArgs a;
        a.A = lnf_; a.B = P(w_.out); a.C = pred_; a.M = (int)BT; a.N = V; a.K = d; a.lda = d; a.ldb = d; a.ldc = V;
        a.epi_mode = 1; a.stat = cestat_;
        RC(gemm_launch(a, L));
        RC(softmax_stat_combine_launch(cestat_, gemm_stat_segments(V), BT, celse_, nullptr, nullptr, nullptr, pred_, V, tokens_, metrics_ + 1, 1.0f / B,
                                       cepart_, (size_t)(BT / 16 + 16), L));
    } else RC(lin_fwd(lnf_, d, P(w_.out), nullptr, pred_, V, BT, V, d, 0, nullptr, 0, 0.f, 0, L));
    return 0;
}

int SlateModel::forward(const StepInputs& in, hipStream_t st) {
    OCRL_REQUIRE(p_ && ws_, "forward: model not bound");
    OCRL_REQUIRE(in.B >= 1 && in.B <= Bmax, "forward: batch %d outside [1,%d]", in.B, Bmax);
    OCRL_REQUIRE(in.obs && in.tau > 0.f, "forward: bad inputs");
    last_ = in;
    have_enc_ = false;
    pdrop_ = in.train ? cfg.dropout : 0.f;
    const Lane L = main_lane(st);
    RC(pack_weights(L));
    if (cfg.use_bcdec) {      // slate_module.py:218-225: loss = mse of the broadcast-decoder reconstruction
        RC(fwd_encoder(in, L));
        RC(pack_bcdec(L));
        RC(fwd_bcdec(L));
        RC(fill_launch(metrics_ + 1, 1, 0.f, L));
        RC(copy_launch(metrics_ + 0, metrics_ + 2, 1, L));
        have_fwd_ = true;
        return 0;
    }
    // the dVAE branch (tokens, reconstruction loss) and the CNN encoder + slot attention are independent until the decoder: on the
    // side stream the dVAE fills the CUs the one-workgroup-per-image slot-attention kernel leaves idle.  plan_.fwd_dvae says where it
    // is forked: here, or at one of three points inside the encoder
    if (plan_.fwd_dvae == FwdDvae::Serial) RC(fwd_dvae(in, L));
    if (plan_.fwd_dvae == FwdDvae::BesideEncoder) {
        RC(after(dvae_lane(), L, ev_fork_));
        RC(fwd_dvae(in, dvae_lane()));
    }
    RC(fwd_encoder(in, L, plan_.fwd_dvae));
    // the decoder needs the tokens only: the rest of the dVAE branch (its decoder, the reconstruction loss) may overlap it
    if (plan_.tokens_early) OCRL_HIP(hipStreamWaitEvent(L, ev_tokens_, 0));
    else if (plan_.side) RC(after(L, dvae_lane(), ev_join_));
    RC(fwd_decoder(L));
    if (plan_.tokens_early) RC(after(L, dvae_lane(), ev_join_));
    RC(copy_launch(metrics_ + 0, metrics_ + 2, 1, L));
    RC(axpy_launch(metrics_ + 1, metrics_ + 2, 1, 1.f, L));      // loss = dvae_mse + cross_entropy
    have_fwd_ = true;
    return 0;
}

int SlateModel::encode(const StepInputs& in, hipStream_t st) {
    OCRL_REQUIRE(p_ && ws_, "encode: model not bound");
    OCRL_REQUIRE(in.B >= 1 && in.B <= Bmax && in.obs, "encode: bad inputs");
    last_ = in;
    pdrop_ = 0.f;
    have_fwd_ = false;
    have_enc_ = true;
    const Lane L = main_lane(st);
    // measured (tools/bench_encode.py, B = 1 / 8 / 32 at 64x64): 0.457 / 0.483 / 1.006 ms replayed against 0.450 / 0.473 / 0.988 ms eager -- the
    // call is bound by its chain of ~30 dependent small kernels on the GPU, not by the host's launches, so the replay is opt-in
    if (enc_graph_mode_ < 0) enc_graph_mode_ = (int)sw::model<sw::OCRL_ENCODE_GRAPH>();
    const bool graph = enc_graph_mode_ && in.B <= 32 && !in.noise_slots && obs_stage_;
    // frozen weights (ocrl_slate_freeze_weights: serving with a pre-trained encoder): the derived weight images -- convolution packs,
    // slot-attention block, position map; 8 launches, ~45 us of a 0.47 ms call at B = 1 -- are built once
    const bool need_pack = !(frozen_ && packs_valid_);
    struct LowLat { int& f; LowLat(int& x) : f(x) { f = 1; } ~LowLat() { f = 0; } } lowlat(conv_lowlat_);      // for every fwd_encoder below
    if (!graph) {
        if (need_pack) RC(pack_weights(L, true));
        packs_valid_ = frozen_;
        return fwd_encoder(in, L);
    }
    EncGraph& eg = enc_graphs_[in.B];
    if (!eg.warm || need_pack) {            // first call at this batch size runs eagerly: one-time kernel attributes are set outside the capture
        eg.warm = 1;
        if (need_pack) RC(pack_weights(L, true));
        packs_valid_ = frozen_;
        return fwd_encoder(in, L);
    }
    const size_t bytes = (size_t)in.B * cfg.obs_channels * N * sizeof(float);
    OCRL_HIP(hipMemcpyAsync(obs_stage_, in.obs, bytes, hipMemcpyDeviceToDevice, L));
    RC(store_u64_launch(seed_dev_, in.seed, L));
    if (!eg.exec) {
        StepInputs gi = in;
        gi.obs = obs_stage_; gi.seed_dev = seed_dev_;
        hipGraph_t g = nullptr;
        // captured on a stream of its own (the caller's may be the legacy default stream, which cannot capture); replayed on the caller's
        if (!cap_) OCRL_HIP(hipStreamCreateWithFlags(&cap_, hipStreamNonBlocking));
        OCRL_HIP(hipStreamBeginCapture(cap_, hipStreamCaptureModeThreadLocal));
        const Lane cap = main_lane(cap_);       // the capture stream stands in for the caller's
        int rc = frozen_ ? 0 : pack_weights(cap, true);
        if (!rc) rc = fwd_encoder(gi, cap);
        const hipError_t ce = hipStreamEndCapture(cap_, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        OCRL_HIP(ce);
        OCRL_HIP(hipGraphInstantiate(&eg.exec, g, nullptr, nullptr, 0));
        OCRL_HIP(hipGraphDestroy(g));
    }
    OCRL_HIP(hipGraphLaunch(eg.exec, L));
    return 0;
}

void SlateModel::clear_encode_graphs() {
    for (auto& kv : enc_graphs_) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    enc_graphs_.clear();
}

// Fine-tuning the encoder through a downstream loss (poolings/base.py:53-55, learn_downstream_loss: the slots reach the pooling head
// undetached): d loss / d slots of the last encode() -> gradients of the CNN encoder, the positional embedding and the slot-attention
// module.  Every other tensor of the flat gradient buffer is zero and is skipped by the next clip_adam(), as torch's Adam skips
// parameters whose .grad is None.
int SlateModel::encode_backward(const float* dslots, hipStream_t st) {
    OCRL_REQUIRE(have_enc_, "encode_backward: call encode first (its activations are what is differentiated)");
    OCRL_REQUIRE(!frozen_, "encode_backward: the weights are frozen (ocrl_slate_freeze_weights): encode() kept no activations");
    OCRL_REQUIRE(g_ && dslots, "encode_backward: no gradient buffer bound / null dslots");
    const Lane L = main_lane(st);
    RC(fill_launch(g_, flat_size_, 0.f, L));
    RC(copy_launch(dslots, gslots_, (long long)last_.B * K * D, L));
    RC(bwd_encoder(L));
    have_enc_ = false;
    enc_only_grads_ = true;
    return 0;
}

// SLATE_Module._gen_imgs (slate_module.py:163-179): greedy autoregressive token decode from the projected slots, then the dVAE
// decoder.  The reference re-runs the whole decoder on the growing prefix for every token (O(T^2) decoder rows); the causal mask makes
// the rows of earlier positions independent of later tokens, so here every step pushes ONE new row per image through the blocks and
// attends to the keys / values of the earlier rows kept in the fused q|k|v buffer of each block (KV cache): T steps of B rows instead
// of T passes of up to B*T rows.  Clobbers the decoder activations: no backward() afterwards.  metrics[4] = mse of the generated image.
int SlateModel::generate(hipStream_t st) {
    OCRL_REQUIRE(!cfg.use_bcdec, "generate: the autoregressive decoder is not part of the use_bcdec configuration");
    OCRL_REQUIRE(last_.B > 0 && last_.obs, "generate: run forward or encode first");
    have_enc_ = false;
    const int B = last_.B;
    const long long BK = (long long)B * K;
    pdrop_ = 0.f;
    have_fwd_ = false;
    const Lane L = main_lane(st);
    OCRL_HIP(hipMemsetAsync(tokens_, 0, sizeof(int) * (size_t)B * T, L));
    // slot side, once: projected slots and every block's cross-attention keys / values
    RC(lin_fwd(slots_, D, P(w_.slotproj), nullptr, mem_, d, BK, d, D, 0, nullptr, 0, 0.f, 0, L));
    for (int b = 0; b < NB; ++b) {
        const DecBlockW& bw = w_.blk[b];
        RC(lin_fwd(mem_, d, P(bw.ck), nullptr, blk_[b].ck, d, BK, d, d, 0, nullptr, 0, 0.f, 0, L));
        RC(lin_fwd(mem_, d, P(bw.cv), nullptr, blk_[b].cv, d, BK, d, d, 0, nullptr, 0, 0.f, 0, L));
    }
    float* x0 = emb_;           // [B, d] rows of the current step (the first rows of the full-size training buffers)
    for (int t = 0; t < T; ++t) {
        RC(embed_step_launch(tokens_, P(w_.dict), P(w_.bos), P(w_.pe), x0, B, T, d, t, L));
        const float* xin = x0;
        for (int b = 0; b < NB; ++b) {
            Blk& k = blk_[b];
            const DecBlockW& bw = w_.blk[b];
            RC(layernorm_fwd_launch(xin, P(bw.ln1.w), P(bw.ln1.b), k.ln1, k.ln1_mean, k.ln1_rstd, B, d, L));
            const float* res = (b == 0) ? k.ln1 : xin;
            // q | k | v of the new row go straight into row t of each image's cache: output row m lives at (m*T + t) * 3d
            RC(lin_fwd(k.ln1, d, P(bw.qkv), nullptr, k.q + (size_t)t * 3 * d, T * 3 * d, B, 3 * d, d, 0, nullptr, 0, 0.f, 0, L));
            RC(decode_attn_launch(k.q, k.ao, B, T, t, d, NH, 3 * d, L));
            RC(lin_fwd(k.ao, d, P(bw.o), nullptr, k.x1, d, B, d, d, 0, res, d, 0.f, 0, L));
            RC(layernorm_fwd_launch(k.x1, P(bw.ln2.w), P(bw.ln2.b), k.ln2, k.ln2_mean, k.ln2_rstd, B, d, L));
            RC(lin_fwd(k.ln2, d, P(bw.cq), nullptr, k.cq, d, B, d, d, 0, nullptr, 0, 0.f, 0, L));
            RC(cross_attn_fwd_launch(k.cq, k.ck, k.cv, k.cao, k.cP, B, 1, K, d, NH, 0.f, 0, 0, L));
            RC(lin_fwd(k.cao, d, P(bw.co), nullptr, k.x2, d, B, d, d, 0, k.x1, d, 0.f, 0, L));
            RC(layernorm_fwd_launch(k.x2, P(bw.ln3.w), P(bw.ln3.b), k.ln3, k.ln3_mean, k.ln3_rstd, B, d, L));
            RC(lin_fwd(k.ln3, d, P(bw.ffn0.w), P(bw.ffn0.b), k.f1, 4 * d, B, 4 * d, d, 1, nullptr, 0, 0.f, 0, L));
            RC(lin_fwd(k.f1, 4 * d, P(bw.ffn2.w), P(bw.ffn2.b), k.x3, d, B, d, 4 * d, 0, k.x2, d, 0.f, 0, L));
            xin = k.x3;
        }
        RC(layernorm_fwd_launch(xin, P(w_.lnf.w), P(w_.lnf.b), lnf_, lnf_mean_, lnf_rstd_, B, d, L));
        RC(lin_fwd(lnf_, d, P(w_.out), nullptr, pred_, V, B, V, d, 0, nullptr, 0, 0.f, 0, L));
        RC(argmax_pos_launch(pred_, tokens_, B, T, V, t, L, 1));
    }
    RC(onehot_launch(tokens_, z_, (long long)B * T, V, L));
    RC(dvae_decode(B, nullptr, L, z_));
    return 0;
}

// ---------------------------------------------------------------------------------------------
int SlateModel::bwd_decoder(const Lane& L) {
    const int B = last_.B;
    const long long BT = (long long)B * T, BK = (long long)B * K;
    const float p = pdrop_;
    // The weight-gradient products go to their own lane W (OCRL_DW_SIDE, dw_lane): after(W, L, ..) makes it wait for everything the main
    // stream has enqueued so far.  Without OCRL_DW_SIDE W is the main lane and the ordering calls do nothing.
    const Lane W = dw_lane(L);
    const bool dws = plan_.dw != 0;
    // output head: d loss / d pred = (softmax(pred_) - onehot(tokens)) / B, rebuilt from the logits as both products stage their A tiles
    Xf ce; ce.a_mode = 3; ce.lse = celse_; ce.tok = tokens_; ce.scale = 1.0f / last_.B;
    RC(after(W, L, ring_event()));
    RC(lin_bwd_w(pred_, V, lnf_, d, G(w_.out), nullptr, BT, V, d, 1.f, W, ce));
    RC(lin_bwd_x(pred_, V, P(w_.out), gt1_, d, BT, V, d, nullptr, 0, nullptr, 0, L, Drop(), ce));
    const float* xlast = blk_[NB - 1].x3;
    RC(layernorm_bwd_launch(gt1_, xlast, lnf_mean_, lnf_rstd_, P(w_.lnf.w), gx_, G(w_.lnf.w), BT, d, 0, 0,
                            L.scratch, L.scratch_floats, L));
    RC(fill_launch(gmem_, BK * d, 0.f, L));
    for (int b = NB - 1; b >= 0; --b) {
        Blk& k = blk_[b];
        const BlkG& q = bg_[dws ? b : 0];
        const DecBlockW& bw = w_.blk[b];
        const unsigned site = SITE_BLK_BASE + 8 * b;
        const float* xin = (b == 0) ? emb_ : blk_[b - 1].x3;
        // ---- feed forward:  x3 = x2 + drop(W2 relu(W1 ln3 + b1) + b2)
        // the gradient entering a residual branch is dropout-backward(gx) of the branch's site: applied once into a buffer of its own and
        // fed to both the weight-gradient and the input-gradient product (drawing the mask inside the products made each 40-90 % slower).
        // With the weight gradients on the side stream the copy is also taken when there is no dropout: gx_ itself moves on.
        const float* gd = gx_;
        auto drop_gx = [&](unsigned s_, float* into) -> int {
            gd = gx_;
            if (p > 0.f || dws) { RC(dropout_apply_launch(gx_, into, BT * d, p, last_.seed, s_, L)); gd = into; }
            return 0;
        };
        RC(drop_gx(site + 4, q.gbr[0]));
        RC(lin_bwd_x(gd, d, P(bw.ffn2.w), q.gf1, 4 * d, BT, d, 4 * d, k.f1, 4 * d, nullptr, 0, L));
        RC(after(W, L, ring_event()));
        RC(lin_bwd_w(gd, d, k.f1, 4 * d, G(bw.ffn2.w), G(bw.ffn2.b), BT, d, 4 * d, 1.f, W));
        RC(lin_bwd_w(q.gf1, 4 * d, k.ln3, d, G(bw.ffn0.w), G(bw.ffn0.b), BT, 4 * d, d, 1.f, W));
        RC(lin_bwd_x(q.gf1, 4 * d, P(bw.ffn0.w), gt1_, d, BT, 4 * d, d, nullptr, 0, nullptr, 0, L));
        RC(layernorm_bwd_launch(gt1_, k.x2, k.ln3_mean, k.ln3_rstd, P(bw.ln3.w), gx_, G(bw.ln3.w), BT, d, 1, 0,
                                L.scratch, L.scratch_floats, L));
        // ---- cross attention
        RC(drop_gx(site + 3, q.gbr[1]));
        const float* gd_co = gd;
        if (xattn_) {
            // folded backward (xattn.hip): d probabilities, soft-max backward and d LN(x) in one launch; the per-image sums
            // d Vo_b = Pd^T d out and d A_b = dS^T LN(x) are two batched products; a per-image kernel takes them back to the projection
            // weights (partials summed over the images in a fixed order) and to d ck / d cv
            XaHost hx = xattn_args(b);
            hx.y = gt1_; hx.gd = gd_co; hx.Pd = q.xaPd; hx.dS = q.xaDs;
            RC(xattn_launch(hx, 1, L));                                                                                  // gt1 = d ln2
            // everything below feeds weight gradients and d mem only: it runs on the weight-gradient stream lane (W), in order
            RC(after(W, L, ring_event()));
            XaFoldBwdHost f;      // the per-image sums, back through the fold to d ck / d cv, and the images' d Wq / d Wo partials summed
            f.Pd = q.xaPd; f.dS = q.xaDs; f.gd = gd_co; f.x = k.ln2; f.Wq = P(bw.cq); f.Wo = P(bw.co); f.ck = k.ck; f.cv = k.cv;
            f.dVo = xa_dVo_; f.dAb = xa_dAb_; f.dck = gck_; f.dcv = gcv_; f.pq = xa_pq_; f.po = xa_po_; f.dWq = G(bw.cq); f.dWo = G(bw.co);
            f.ws = W.scratch; f.ws_floats = W.scratch_floats; f.B = B; f.T = T; f.K = K; f.d = d; f.h = NH;
            RC(xattn_fold_bwd_launch(f, W));
        } else {
        RC(lin_bwd_x(gd, d, P(bw.co), gt1_, d, BT, d, d, nullptr, 0, nullptr, 0, L));   // d cao
        RC(cross_attn_bwd_launch(gt1_, k.cq, k.ck, k.cv, k.cP, q.gt2, gck_, gcv_, B, T, K, d, NH, p, last_.seed, site + 2, L.scratch, L.scratch_floats, L));   // gt2 = d cq
        RC(after(W, L, ring_event()));
        RC(lin_bwd_w(gd_co, d, k.cao, d, G(bw.co), nullptr, BT, d, d, 1.f, W));
        RC(lin_bwd_w(q.gt2, d, k.ln2, d, G(bw.cq), nullptr, BT, d, d, 1.f, W));
        RC(lin_bwd_x(q.gt2, d, P(bw.cq), gt1_, d, BT, d, d, nullptr, 0, nullptr, 0, L));   // d ln2
        }
        {   // slot-side projections k / v: their weight gradients and d mem (accumulated over the blocks)
            const Lane& X = xattn_ ? W : L;      // in the folded form d ck / d cv were produced on the weight-gradient lane
            RC(lin_bwd_w(gck_, d, mem_, d, G(bw.ck), nullptr, BK, d, d, 1.f, X));
            RC(lin_bwd_w(gcv_, d, mem_, d, G(bw.cv), nullptr, BK, d, d, 1.f, X));
            RC(lin_bwd_x(gck_, d, P(bw.ck), gmem_, d, BK, d, d, nullptr, 0, gmem_, d, X));
            RC(lin_bwd_x(gcv_, d, P(bw.cv), gmem_, d, BK, d, d, nullptr, 0, gmem_, d, X));
        }
        RC(layernorm_bwd_launch(gt1_, k.x1, k.ln2_mean, k.ln2_rstd, P(bw.ln2.w), gx_,
                                G(bw.ln2.w), BT, d, 1, 0, L.scratch, L.scratch_floats, L));
        // ---- causal self attention
        RC(drop_gx(site + 1, q.gbr[2]));
        const float* gd_o = gd;
        RC(lin_bwd_x(gd, d, P(bw.o), gt1_, d, BT, d, d, nullptr, 0, nullptr, 0, L));   // gt1 = d ao
        {
            AttnArgs a = self_attn_args(b);
            a.dO = gt1_; a.dq = q.gqkv; a.dk = q.gqkv + d; a.dv = q.gqkv + 2 * d; a.delta = attn_delta_;
            a.ds = attn_ds_; a.ds_floats = attn_ds_floats_;
            RC(attn_launch(a, 1, L));
        }
        // fused [3d, d] weight: dW = [dq|dk|dv]^T ln1 ;  d ln1 = [dq|dk|dv] W
        RC(after(W, L, ring_event()));
        RC(lin_bwd_w(gd_o, d, k.ao, d, G(bw.o), nullptr, BT, d, d, 1.f, W));
        RC(lin_bwd_w(q.gqkv, 3 * d, k.ln1, d, G(bw.qkv), nullptr, BT, 3 * d, d, 1.f, W));
        RC(lin_bwd_x(q.gqkv, 3 * d, P(bw.qkv), gt1_, d, BT, 3 * d, d, nullptr, 0, nullptr, 0, L));      // gt1 = d ln1
        if (b == 0) {
            // ln1 is both the attention input and the residual stream: d ln1_total = gx + gt2, then LN backward to emb
            RC(axpy_launch(gx_, gt1_, BT * d, 1.f, L));
            RC(layernorm_bwd_launch(gt1_, xin, k.ln1_mean, k.ln1_rstd, P(bw.ln1.w), gx_,
                                    G(bw.ln1.w), BT, d, 0, 0, L.scratch, L.scratch_floats, L));
        } else {
            RC(layernorm_bwd_launch(gt1_, xin, k.ln1_mean, k.ln1_rstd, P(bw.ln1.w), gx_,
                                    G(bw.ln1.w), BT, d, 1, 0, L.scratch, L.scratch_floats, L));
        }
    }
    // ---- embedding: gx_ = d emb (after dropout);  dictionary (rows sorted by token, summed in a fixed order), pe / bos (sum over the batch)
    RC(embed_bwd_launch(gx_, tokens_, G(w_.dict), B, T, V, d, p, last_.seed, L.scratch, L.scratch_floats, L));
    RC(fill_launch(G(w_.pe), (long long)(T + 1) * d, 0.f, L));
    RC(colsum_launch(gx_, (long long)T * d, G(w_.pe), B, T * d, 0, 1.f, L.scratch, L.scratch_floats, L));
    RC(copy_launch(G(w_.pe), G(w_.bos), d, L));
    // ---- slot projection (d mem was accumulated on the weight-gradient stream in the folded cross-attention form)
    if (xattn_) RC(after(L, W, ring_event()));
    RC(lin_bwd_w(gmem_, d, slots_, D, G(w_.slotproj), nullptr, BK, d, D, 1.f, L));
    RC(lin_bwd_x(gmem_, d, P(w_.slotproj), gslots_, D, BK, d, D, nullptr, 0, nullptr, 0, L));
    return 0;
}

int SlateModel::bwd_encoder(const Lane& L, BwdDvae fork) {
    const bool fork_dvae = fork == BwdDvae::AtSlotAttention;
    const int B = last_.B;
    const long long BN = (long long)B * N, R = (long long)B * I * K;
    const SlotAttnW& sa = w_.sa;
    SlotAttnArgs a = sa_args(B, N, K, D, H, I, SH);
    a.x = x_; a.wts = sa_wts_; a.save = sa_save_; a.dslots = gslots_; a.dx = gA_; a.dslots0 = gslots0_; a.grows = sa_grows_; a.g_small = sa_small_;
    a.xchg = sa_xchg_; a.parts = sa_parts_;
    if (fork_dvae) {
        RC(after(dvae_lane(), L, ev_fork_));
        RC(bwd_dvae(dvae_lane()));
    }
    RC(slot_attn_launch(a, 1, L));
    // Everything below that only consumes the slot-attention backward's outputs (gradient rows, dx) and feeds no later kernel of the
    // step -- the slot-side weight gradients, the LayerNorm partials, the slot-initialisation gradients and the weight gradient of the
    // input MLP's second layer -- goes to the side stream; the main stream continues with the input-gradient chain towards the
    // convolutions.  Joined before the convolutions.
    const bool side_w = plan_.sa_wgrads_on_side;       // never together with fork_dvae: the plan puts the dVAE backward elsewhere then
    const Lane W = side_w ? dvae_lane() : L;
    if (side_w) RC(after(W, L, ev_fork_));
    const bool sa_in_bwd = sa_input_ == 1 && C == 64;          // the input LayerNorm + MLP backward as one kernel on the main stream
    // weight gradients: contract the emitted gradient rows with the saved activations over (image, iteration, slot), the bias gradient
    // out of the same product
    SaWgrad wg[SA_MAX_WGRADS];
    const int nwg = sa_wgrad_list(C, D, H, SH, a.scale, wg);
    for (int i = 0; i < nwg; ++i) {
        const SaWgrad& e = wg[i];
        RC(lin_bwd_w(e.dy.at(sa_save_, sa_grows_), e.dy.ld, e.x.at(sa_save_, sa_grows_), e.x.ld, G(sa.w[e.w]) + e.w_off,
                     e.b < 0 ? nullptr : G(sa.w[e.b]), R, e.N_out, e.K_in, e.alpha, W));
    }
    // LayerNorm gammas / betas: weight and bias are adjacent in the flat buffer, one column sum over each pair
    const int SM = 4 * D + 2 * C;
    RC(colsum_launch(sa_small_ + 0, SM, G(sa.w[SAW_NORM_SLOTS_W]), B, 2 * D, 0, 1.f, W.scratch, W.scratch_floats, W));
    RC(colsum_launch(sa_small_ + 2 * D, SM, G(sa.w[SAW_NORM_MLP_W]), B, 2 * D, 0, 1.f, W.scratch, W.scratch_floats, W));
    RC(colsum_launch(sa_small_ + 4 * D, SM, G(sa.w[SAW_NORM_INPUTS_W]), B, 2 * C, 0, 1.f, W.scratch, W.scratch_floats, W));
    RC(slot_init_bwd_launch(gslots0_, P(w_.sa.log_sigma), last_.noise_slots, G(w_.sa.mu), G(w_.sa.log_sigma),
                            B * K, D, last_.seed, W));
    // ---- input MLP: x = W2 relu(W0 LN(e4) + b0) + b2 ; gA = dx
    if (!sa_in_bwd) RC(lin_bwd_w(gA_, C, h1_, C, G(w_.sa.mlp2.w), G(w_.sa.mlp2.b), BN, C, C, 1.f, W));
    // the first convolution's weight gradient is a product with im2col(obs): the patch matrix only needs the observation
    if (side_w && !first_direct()) RC(im2col5_launch(obs8_, col0_, BN, S, S, cfg.obs_channels, (25 * cfg.obs_channels + 3) & ~3, W));
    if (sa_in_bwd) {
        // reads dx (gA_), h1, e4; writes d e4 (gB_) and the six parameter gradients from one partial slab per workgroup (csrc/sa_input.hip)
        const size_t slabs = L.scratch_floats / SA_INPUT_SLAB;
        OCRL_REQUIRE(slabs >= 1, "bwd_encoder: scratch too small for the input-chain slabs");
        RC(sa_input_bwd_launch(gA_, h1_, e4_, ln0_mean_, ln0_rstd_, P(w_.sa.ln.w), P(w_.sa.ln.b),
                               P(w_.sa.mlp0.w), P(w_.sa.mlp2.w), gB_, G(w_.sa.mlp0.w), G(w_.sa.mlp0.b),
                               G(w_.sa.mlp2.w), G(w_.sa.mlp2.b), G(w_.sa.ln.w), G(w_.sa.ln.b),
                               BN, slabs < 512 ? (int)slabs : 0, L.scratch, L.scratch_floats, L));
    } else {
        RC(lin_bwd_x(gA_, C, P(w_.sa.mlp2.w), gB_, C, BN, C, C, h1_, C, nullptr, 0, L));              // gB = d h1 (pre-relu)
        RC(lin_bwd_w(gB_, C, ln0_, C, G(w_.sa.mlp0.w), G(w_.sa.mlp0.b), BN, C, C, 1.f, L));
        // d ln0 goes to gC_ when the side stream may still be reading gA_ (= dx) for the second layer's weight gradient
        float* gL = side_w ? gC_ : gA_;
        RC(lin_bwd_x(gB_, C, P(w_.sa.mlp0.w), gL, C, BN, C, C, nullptr, 0, nullptr, 0, L));            // gL = d ln0
        RC(layernorm_bwd_launch(gL, e4_, ln0_mean_, ln0_rstd_, P(w_.sa.ln.w), gB_, G(w_.sa.ln.w), BN, C, 0, 0,
                                L.scratch, L.scratch_floats, L));                                                      // gB = d e4
    }
    // ---- positional embedding (added to every image): d map = sum over images
    RC(colsum_launch(gB_, (long long)N * C, gmap_, B, N * C, 0, 1.f, L.scratch, L.scratch_floats, L));
    RC(lin_bwd_w(gmap_, C, gridT_, 4, G(w_.enc_pos.w), G(w_.enc_pos.b), N, C, 4, 1.f, L));
    if (fork_dvae || side_w) RC(after(L, dvae_lane(), ev_join_));      // the side stream has read gA_ (= dx): the convolution chain may reuse it
    if (plan_.dw == 2) RC(after(L, dw_lane(L), ev_join2_));      // ... and the decoder's weight gradients are done: the convolutions run alone
    // ---- CNN encoder, last layer first
    // the last layer's bias gradient is the column sum of the per-position sums gmap_ just taken for the positional embedding (4 MB),
    // not another pass over the [B*N, 64] gradient (537 MB)
    RC(colsum_launch(gmap_, C, G(w_.enc[3].b), N, C, 0, 1.f, L.scratch, L.scratch_floats, L));
    RC(conv_layer_wgrad(e3_, gB_, G(w_.enc[3].w), nullptr, B, S, S, 5, 64, 64, L));
    RC(conv_layer_fwd(gB_, cw_bwd_[3], nullptr, gA_, B, S, S, 5, 64, 0, nullptr, e3_, L));                       // gA = d e3 (pre-relu)
    RC(conv_layer_wgrad(e2_, gA_, G(w_.enc[2].w), G(w_.enc[2].b), B, S, S, 5, 64, 64, L));
    RC(conv_layer_fwd(gA_, cw_bwd_[2], nullptr, gB_, B, S, S, 5, 64, 0, nullptr, e2_, L));
    RC(conv_layer_wgrad(e1_, gB_, G(w_.enc[1].w), G(w_.enc[1].b), B, S, S, 5, 64, 64, L));
    RC(conv_layer_fwd(gB_, cw_bwd_[1], nullptr, gA_, B, S, S, 5, 64, 0, nullptr, e1_, L));
    // first layer: three channels go through the kernel that gathers the patches from the observation's halo tiles and sums the bias
    // gradient on the way (csrc/conv_first.hip); any other count as dW = dY^T im2col(obs), one [64 x 25 ch] split-K product over the pixels
    if (first_direct()) {
        OCRL_REQUIRE(conv_first_wgrad_ws_floats(B, S, S) <= L.scratch_floats, "first conv wgrad: scratch too small");
        RC(conv_first_wgrad_launch(obs_keep_, gA_, L.scratch, G(w_.enc[0].w), G(w_.enc[0].b), B, S, S, 0, L));
    } else {
        const int ch = cfg.obs_channels, ldc0 = (25 * ch + 3) & ~3;
        if (!side_w) RC(im2col5_launch(obs8_, col0_, BN, S, S, ch, ldc0, L));
        RC(lin_bwd_w(gA_, 64, col0_, ldc0, dw0p_, G(w_.enc[0].b), BN, 64, ldc0, 1.f, L));
        RC(unpack5_launch(dw0p_, G(w_.enc[0].w), ch, ldc0, L));
    }
    return 0;
}

int SlateModel::bwd_dvae(const Lane& L) {
    const int B = last_.B;
    const long long BT = (long long)B * T, BN = (long long)B * N;
    const int ch = cfg.obs_channels;
    // ---- output conv 64 -> 3 (padded to 4 columns): dW through a [4,64] scratch
    float* w4 = L.scratch + L.scratch_floats - 1024;      // tail of the scratch region, not touched by split-k / colsum
    {
        GemmArgs a;
        a.A = drecon_; a.B = ps2_; a.C = w4; a.M = 4; a.N = 64; a.K = (int)BN; a.lda = 4; a.ldb = 64; a.ldc = 64; a.akc = 0; a.bkc = 0;
        long long splits = BN / 512; if (splits > 512) splits = 512; if (splits < 1) splits = 1;
        if (splits > 1) {
            a.splitk = (int)splits; a.C = L.scratch; a.sCsplit = 256;
            RC(gemm_launch(a, L));
            RC(splitk_reduce_launch(L.scratch, w4, 256, (int)splits, 256, 0, L));
        } else RC(gemm_launch(a, L));
        RC(copy_launch(w4, G(w_.dvae_dec[11].w), ch * 64, L));
        // bias gradient: the padded rows are summed as float4 (the 3-wide scalar form ran one 64-lane column group at 0.05 TB/s)
        RC(colsum_launch(drecon_, 4, w4 + 256, BN, 4, 0, 1.f, L.scratch, L.scratch_floats - 1024, L));
        RC(copy_launch(w4 + 256, G(w_.dvae_dec[11].b), ch, L));
    }
    RC(lin_bwd_x(drecon_, 4, w11p_, gdA_, 64, BN, 4, 64, nullptr, 0, nullptr, 0, L));                            // gdA = d ps2
    RC(pixel_shuffle_launch(gdA_, gdB_, B, 2 * E, 2 * E, 64, 0, dd9_, L));                                        // gdB = d dd9 (pre-relu) [4BT,256]
    RC(lin_bwd_w(gdB_, 256, dd8_, 64, G(w_.dvae_dec[9].w), G(w_.dvae_dec[9].b), 4 * BT, 256, 64, 1.f, L));
    RC(lin_bwd_x(gdB_, 256, P(w_.dvae_dec[9].w), gdA_, 64, 4 * BT, 256, 64, dd8_, 64, nullptr, 0, L));
    RC(lin_bwd_w(gdA_, 64, dd7_, 64, G(w_.dvae_dec[8].w), G(w_.dvae_dec[8].b), 4 * BT, 64, 64, 1.f, L));
    RC(lin_bwd_x(gdA_, 64, P(w_.dvae_dec[8].w), gdB_, 64, 4 * BT, 64, 64, dd7_, 64, nullptr, 0, L));
    RC(lin_bwd_w(gdB_, 64, dd6_, 64, G(w_.dvae_dec[7].w), G(w_.dvae_dec[7].b), 4 * BT, 64, 64, 1.f, L));
    RC(lin_bwd_x(gdB_, 64, P(w_.dvae_dec[7].w), gdA_, 64, 4 * BT, 64, 64, dd6_, 64, nullptr, 0, L));   // gdA = d dd6 (pre-relu)
    RC(conv_layer_wgrad(ps1_, gdA_, G(w_.dvae_dec[6].w), G(w_.dvae_dec[6].b), B, 2 * E, 2 * E, 3, 64, 64, L));
    RC(conv_layer_fwd(gdA_, dw_bwd_[1], nullptr, gdB_, B, 2 * E, 2 * E, 3, 64, 0, nullptr, ps1_, L));             // gdB = d ps1 (relu mask of dd4)
    RC(pixel_shuffle_launch(gdB_, gdA_, B, E, E, 64, 0, nullptr, L));                                             // gdA = d dd4 (pre-relu) [BT,256]
    RC(lin_bwd_w(gdA_, 256, dd3_, 64, G(w_.dvae_dec[4].w), G(w_.dvae_dec[4].b), BT, 256, 64, 1.f, L));
    RC(lin_bwd_x(gdA_, 256, P(w_.dvae_dec[4].w), gdB_, 64, BT, 256, 64, dd3_, 64, nullptr, 0, L));
    RC(lin_bwd_w(gdB_, 64, dd2_, 64, G(w_.dvae_dec[3].w), G(w_.dvae_dec[3].b), BT, 64, 64, 1.f, L));
    RC(lin_bwd_x(gdB_, 64, P(w_.dvae_dec[3].w), gdA_, 64, BT, 64, 64, dd2_, 64, nullptr, 0, L));
    RC(lin_bwd_w(gdA_, 64, dd1_, 64, G(w_.dvae_dec[2].w), G(w_.dvae_dec[2].b), BT, 64, 64, 1.f, L));
    RC(lin_bwd_x(gdA_, 64, P(w_.dvae_dec[2].w), gdB_, 64, BT, 64, 64, dd1_, 64, nullptr, 0, L));       // gdB = d dd1 (pre-relu)
    RC(conv_layer_wgrad(dd0_, gdB_, G(w_.dvae_dec[1].w), G(w_.dvae_dec[1].b), B, E, E, 3, 64, 64, L));
    RC(conv_layer_fwd(gdB_, dw_bwd_[0], nullptr, gdA_, B, E, E, 3, 64, 0, nullptr, dd0_, L));                     // gdA = d dd0 (pre-relu)
    float* dz = zraw_;      // the logits / scores are not needed any more: d raw = d logp is built in their place
    have_scores_ = false;
    if (fused_heads()) {
        Xf zx; zx.b_mode = 2; zx.lse = zlse_;
        RC(lin_bwd_w(gdA_, 64, zraw_, V, G(w_.dvae_dec[0].w), G(w_.dvae_dec[0].b), BT, 64, V, 1.f, L, zx));
        // Gumbel soft-max backward in the epilogue of the dz product: d = z (dz - sum_v z_v dz_v) / tau with
        // sum_v z_v dz_v = sum_c g_c (z W^T)_c = sum_c g_c (dd0 - bias)_c  (g = gdA_ is zero where the ReLU of dd0 is closed)
        RC(rowdot_bias64_launch(gdA_, dd0_, P(w_.dvae_dec[0].b), BT, zdot_, L));
        GemmArgs a;
        a.A = gdA_; a.B = P(w_.dvae_dec[0].w); a.C = dz; a.M = (int)BT; a.N = V; a.K = 64; a.lda = 64; a.ldb = V; a.ldc = V; a.bkc = 0;
        a.epi_mode = 3; a.mask = zraw_; a.ldmask = V; a.e_lse = zlse_; a.e_rowvec = zdot_; a.e_scale = 1.0f / last_.tau;
        RC(gemm_launch(a, L));
    } else {
    RC(lin_bwd_w(gdA_, 64, zdec_, V, G(w_.dvae_dec[0].w), G(w_.dvae_dec[0].b), BT, 64, V, 1.f, L));
    RC(lin_bwd_x(gdA_, 64, P(w_.dvae_dec[0].w), dz, V, BT, 64, V, nullptr, 0, nullptr, 0, L));
    // ---- Gumbel softmax + log_softmax backward (row sums of the soft-max gradient vanish, so d raw = d logp)
    RC(softmax_bwd_rows_launch(z_, dz, BT, V, 1.0f / last_.tau, L));
    }
    // ---- encoder
    RC(lin_bwd_w(dz, V, de_[6], 64, G(w_.dvae_enc[7].w), G(w_.dvae_enc[7].b), BT, V, 64, 1.f, L));
    RC(lin_bwd_x(dz, V, P(w_.dvae_enc[7].w), gdA_, 64, BT, V, 64, de_[6], 64, nullptr, 0, L));
    float* cur = gdA_;
    float* oth = gdB_;
    for (int i = 6; i >= 1; --i) {
        RC(lin_bwd_w(cur, 64, de_[i - 1], 64, G(w_.dvae_enc[i].w), G(w_.dvae_enc[i].b), BT, 64, 64, 1.f, L));
        RC(lin_bwd_x(cur, 64, P(w_.dvae_enc[i].w), oth, 64, BT, 64, 64, de_[i - 1], 64, nullptr, 0, L));
        float* t = cur; cur = oth; oth = t;
    }
    RC(lin_bwd_w(cur, 64, patches_, 16 * ch, G(w_.dvae_enc[0].w), G(w_.dvae_enc[0].b), BT, 64, 16 * ch, 1.f, L));
    return 0;
}

int SlateModel::backward(hipStream_t st) {
    OCRL_REQUIRE(have_fwd_, "backward: call forward first");
    OCRL_REQUIRE(g_, "backward: no gradient buffer bound");
    enc_only_grads_ = false;
    const Lane L = main_lane(st);
    if (cfg.use_bcdec) {
        RC(fill_launch(g_, flat_size_, 0.f, L));       // dVAE / transformer / slotproj parameters get no gradient in this mode
        RC(bwd_bcdec(L));
        RC(bwd_encoder(L));
        have_fwd_ = false;
        return 0;
    }
    // the dVAE backward only needs the forward's reconstruction gradient; plan_.bwd_dvae says what it runs beside
    const BwdDvae at = plan_.bwd_dvae;
    if (at == BwdDvae::BesideAll || at == BwdDvae::BesideDecoder) {
        RC(after(dvae_lane(), L, ev_fork_));
        RC(bwd_dvae(dvae_lane()));
    }
    RC(bwd_decoder(L));
    // with the decoder's weight gradients on lanes of their own the dVAE lane may still be busy: it is joined inside bwd_encoder, before
    // the convolutions, so the slot-attention backward and the input MLP overlap what is left of it
    if (at == BwdDvae::BesideDecoder && !plan_.dw) RC(after(L, dvae_lane(), ev_join_));
    RC(bwd_encoder(L, at));
    if (at == BwdDvae::BesideAll) RC(after(L, dvae_lane(), ev_join_));
    if (at == BwdDvae::SerialLast) RC(bwd_dvae(L));
    have_fwd_ = false;
    return 0;
}

int SlateModel::after(const Lane& waiter, const Lane& producer, hipEvent_t ev) {
    if (waiter.st == producer.st) return 0;        // one stream orders itself (a switch put both roles on the same lane)
    OCRL_HIP(hipEventRecord(ev, producer.st));
    OCRL_HIP(hipStreamWaitEvent(waiter.st, ev, 0));
    return 0;
}

int SlateModel::grad_norm(hipStream_t st) {
    const Lane L = main_lane(st);
    return absmax_launch(g_, flat_size_, metrics_ + 3, L.scratch, L.scratch_floats, L);
}

int SlateModel::clip_adam(const float lr[3], float clip, int step, float gscale, hipStream_t st) {
    OCRL_REQUIRE(m_ && v_, "clip_adam: optimiser state not bound");
    packs_valid_ = false;
    RC(grad_norm(st));
    if (enc_only_grads_) {       // after encode_backward(): the encoder tensors only (group 1 up to the slot projection / broadcast decoder)
        const long long b0 = group_begin_[1], end = w_.enc_grads_end;
        return clip_adam_launch(p_ + b0, g_ + b0, m_ + b0, v_ + b0, end - b0, metrics_ + 3, clip, lr[1], 0.9, 0.999, 1e-8, step, gscale, st);
    }
    for (int g = 0; g < 3; ++g) {
        if (cfg.use_bcdec && g != 1) continue;      // parameters without gradients are skipped, as torch's Adam does
        const long long b0 = group_begin_[g], n = group_begin_[g + 1] - b0;
        RC(clip_adam_launch(p_ + b0, g_ + b0, m_ + b0, v_ + b0, n, metrics_ + 3, clip, lr[g], 0.9, 0.999, 1e-8, step, gscale, st));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Slot-Attention configuration: spatial-broadcast decoder (ocrs/common/models.py:110-141)
int SlateModel::pack_bcdec(const Lane& L) {
    RC(bc_compose_launch(P(w_.bc[0].w), P(w_.bc_pos.w), P(w_.bc_pos.b), bc_Wc_,
                         bc_W1r_, D, L));
    RC(conv_pack_launch(P(w_.bc[1].w), bc_pk_[0], bc_pkb_[0], 5, 64, 64, 64, L));
    RC(conv_pack_launch(P(w_.bc[2].w), bc_pk_[1], bc_pkb_[1], 5, 64, 64, 64, L));
    if (conv_x3_ > 0) {
        for (int i = 0; i < 2; ++i) {
            auto f = x3_of_.find(bc_pk_[i]), b = x3_of_.find(bc_pkb_[i]);
            if (f != x3_of_.end()) RC(conv_pack_x3_launch(P(w_.bc[i + 1].w), const_cast<float*>(f->second), b != x3_of_.end() ? const_cast<float*>(b->second) : nullptr, L));
        }
    }
    RC(bc_c4_pack_launch(P(w_.bc[3].w), bc_Wk4_, bc_Wb4_, cfg.obs_channels + 1, L));
    return 0;
}

int SlateModel::fwd_bcdec(const Lane& L) {
    const int B = last_.B, BK = B * K;
    RC(bc_posconv_launch(bc_Wc_, bc_P1_, S, L));
    RC(lin_fwd(slots_, D, bc_W1r_, nullptr, bc_M_, 1600, BK, 1600, D, 0, nullptr, 0, 0.f, 0, L));       // M[bk][tap][co] = W_tap s
    RC(bcast_l1_class_sum_launch(bc_M_, bc_T_, BK, 5, 1, L));
    RC(bcast_l1_fwd_launch(bc_P1_, bc_T_, P(w_.bc[0].b), bc_c1_, BK, S, 5, BCAST_L1_RELU, L));
    RC(conv_layer_fwd(bc_c1_, bc_pk_[0], P(w_.bc[1].b), bc_c2_, BK, S, S, 5, 64, 1, nullptr, nullptr, L));
    RC(conv_layer_fwd(bc_c2_, bc_pk_[1], P(w_.bc[2].b), bc_c3_, BK, S, S, 5, 64, 1, nullptr, nullptr, L));
    RC(bc_c4_fwd_launch(bc_c3_, bc_Wk4_, P(w_.bc[3].b), bc_out4_, BK, S, L));
    RC(bc_mix_launch(bc_out4_, last_.obs, recon_, bc_dout4_, metrics_ + 0, B, K, S, cfg.obs_channels, L.scratch, L.scratch_floats, L));
    return 0;
}

int SlateModel::bwd_bcdec(const Lane& L) {
    const int B = last_.B, BK = B * K;
    const long long BKN = (long long)BK * N;
    // output conv 64 -> 4
    const int nb = bc_c4_wgrad_blocks(BK, S);
    RC(bc_c4_wgrad_launch(bc_c3_, bc_dout4_, L.scratch, BK, S, L));
    RC(colsum_launch(L.scratch, 4 * 64 * 9, G(w_.bc[3].w), nb, 4 * 64 * 9, 0, 1.f, L.scratch + (size_t)nb * 2304, L.scratch_floats - (size_t)nb * 2304, L));
    RC(colsum_launch(bc_dout4_, 4, G(w_.bc[3].b), BKN, cfg.obs_channels + 1, 0, 1.f, L.scratch, L.scratch_floats, L));
    RC(bc_c4_bwd_data_launch(bc_dout4_, bc_Wb4_, bc_c3_, bc_gA_, BK, S, L));                                      // gA = d c3 (pre-relu)
    RC(conv_layer_wgrad(bc_c2_, bc_gA_, G(w_.bc[2].w), G(w_.bc[2].b), BK, S, S, 5, 64, 64, L));
    RC(conv_layer_fwd(bc_gA_, bc_pkb_[1], nullptr, bc_gB_, BK, S, S, 5, 64, 0, nullptr, bc_c2_, L));               // gB = d c2 (pre-relu)
    RC(conv_layer_wgrad(bc_c1_, bc_gB_, G(w_.bc[1].w), G(w_.bc[1].b), BK, S, S, 5, 64, 64, L));
    RC(conv_layer_fwd(bc_gB_, bc_pkb_[0], nullptr, bc_gA_, BK, S, S, 5, 64, 0, nullptr, bc_c1_, L));               // gA = d c1 (pre-relu)
    // first layer through the shortcut
    RC(bcast_l1_bwd_launch(bc_gA_, bc_dT_, BK, S, 5, L.scratch, L.scratch_floats, L));
    RC(colsum_launch(bc_dT_, 64, G(w_.bc[0].b), (long long)BK * 25, 64, 0, 1.f, L.scratch, L.scratch_floats, L));
    RC(bcast_l1_class_sum_launch(bc_dT_, bc_dM_, BK, 5, 0, L));
    RC(lin_bwd_x(bc_dM_, 1600, bc_W1r_, gslots_, D, BK, 1600, D, nullptr, 0, nullptr, 0, L));                      // d slots
    RC(lin_bwd_w(bc_dM_, 1600, slots_, D, bc_dW1r_, nullptr, BK, 1600, D, 1.f, L));
    RC(colsum_launch(bc_gA_, (long long)N * 64, bc_G1_, BK, N * 64, 0, 1.f, L.scratch, L.scratch_floats, L));        // sum over (image, slot)
    RC(bc_posconv_bwd_launch(bc_G1_, bc_dWc_, S, L));
    RC(bc_compose_bwd_launch(P(w_.bc[0].w), P(w_.bc_pos.w), P(w_.bc_pos.b), bc_dWc_,
                             bc_dW1r_, G(w_.bc[0].w), G(w_.bc_pos.w), G(w_.bc_pos.b), D, L));
    return 0;
}
