// SLATE training-step orchestration over the HIP kernels (host code).  One object per process
// per GPU; not thread-safe; every launch goes to the caller's stream or to a side stream ordered against it (Lane).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#include "model_base.h"
#include "slot_attn_host.h"
#include "stream_plan.h"

struct SlateConfig {
    int obs_size = 64, obs_channels = 3, vocab = 4096, d_model = 192, cnn_hidden = 64;
    int num_slots = 5, num_iters = 3, slot_size = 192, mlp_hidden = 192;
    int num_blocks = 4, num_heads = 4;
    float dropout = 0.1f;
    int max_batch = 1;
    int use_bcdec = 0;      // Slot-Attention configuration: spatial-broadcast decoder instead of dVAE + transformer
    int hard = 0;           // ocr_config.hard: straight-through Gumbel sample for the dVAE decoder (utils.py:81-83)
    int slot_heads = 1;     // ocr_config.slotattr.num_slot_heads (ocrs/common/slot_attn.py:28)
};

struct StepInputs {
    const float* obs = nullptr;        // [B,3,S,S] NCHW fp32 in [0,1]
    int B = 0;
    float tau = 1.f;
    int train = 1;                     // dropout on/off
    unsigned long long seed = 0;       // device RNG stream for this step (noise + dropout)
    const float* noise_z = nullptr;    // optional injected Exp(1) draws [B,T,V] (both or none)
    const float* noise_zh = nullptr;
    const float* noise_slots = nullptr;  // optional injected N(0,1) [B,K,D]
    const unsigned long long* seed_dev = nullptr;   // internal: the slot-noise seed read from device memory (captured encode graphs)
};

// A lane is a stream together with the transient scratch (split-k slabs, column-sum partials, wgrad slabs) that launches on it may
// use: lanes run concurrently, so each has a region of its own, and every launcher that needs scratch takes it from the lane it
// launches on.  Passed where a launcher expects the stream.
struct Lane {
    hipStream_t st = nullptr;
    float* scratch = nullptr;
    size_t scratch_floats = 0;
    operator hipStream_t() const { return st; }
};

class SlateModel : public ModelBase {
public:
    explicit SlateModel(const SlateConfig& c);
    ~SlateModel();
    long long group_begin(int g) const { return group_begin_[g]; }   // group g = [begin(g), begin(g+1))
    int bind(float* p, float* g, float* m, float* v, void* ws, size_t ws_bytes);
    int forward(const StepInputs& in, hipStream_t st);          // loss terms -> metrics()
    int backward(hipStream_t st);                               // fills the flat gradient buffer
    int encode(const StepInputs& in, hipStream_t st);           // slots + attention only (inference path)
    void freeze_weights(bool on) { frozen_ = on; packs_valid_ = false; clear_encode_graphs(); }
    void clear_encode_graphs();
    int encode_backward(const float* dslots, hipStream_t st);   // gradient of the last encode() wrt the encoder's parameters (downstream fine-tuning)
    int generate(hipStream_t st);                               // greedy autoregressive image from the last step's slots
    int clip_adam(const float lr[3], float clip, int step, float gscale, hipStream_t st);
    int grad_norm(hipStream_t st);                              // metrics()[3] = max |g|
    // metrics(): dvae_mse, ce, loss, grad absmax
    int dropout_mask(unsigned site, long long n, float* out, hipStream_t st) const;
    // writes the soft sample z = softmax(scores) of the last forward into the named tensor "z" (the fused heads keep only the scores;
    // valid between forward and backward -- the backward builds d logits in place of the scores)
    int soft_z(hipStream_t st);
    const SlateConfig cfg;

private:
    void layout_workspace(bool commit);
    // the Linear helpers of gemm.hip with this step's dropout seed and the lane's scratch (lin_bwd_x is used as it is)
    int lin_fwd(const float* x, int ldx, const float* W, const float* b, float* y, int ldy, long long M, int N, int K, int relu,
                const float* resid, int ldr, float drop_p, unsigned site, hipStream_t st) {
        return ::lin_fwd(x, ldx, W, b, y, ldy, M, N, K, relu, resid, ldr, st, Drop{drop_p, last_.seed, site});
    }
    int lin_bwd_w(const float* dy, int ld_dy, const float* x, int ldx, float* dW, float* db, long long M, int N_out, int K_in,
                  float alpha, const Lane& L, Xf xf = Xf()) {
        return ::lin_bwd_w(dy, ld_dy, x, ldx, dW, db, M, N_out, K_in, alpha, L.scratch, L.scratch_floats, L.st, Drop(), xf);
    }
    // the Gumbel / cross-entropy soft-max heads live in the vocabulary GEMMs (soft samples; the straight-through `hard` form keeps z)
    bool fused_heads() const { return !cfg.hard; }
    int conv_layer_fwd(const float* x, const float* pack, const float* bias, float* y, int Bn, int Hh, int Ww, int KS, int CIN, int relu,
                       const float* posmap, const float* mask, const Lane& L);
    int conv_layer_wgrad(const float* x, const float* dy, float* dW, float* db, int Bn, int Hh, int Ww, int KS, int CIN, int cin_real,
                         const Lane& L);
    int pack_weights(const Lane& L, bool encoder_only = false);
    // fork: the plan's placement of the step's dVAE forward; the three placements inside the encoder fork it there.  encode() and the
    // use_bcdec step, which run no dVAE branch, leave the default (as do forward()'s own two placements)
    int fwd_encoder(const StepInputs& in, const Lane& L, FwdDvae fork = FwdDvae::Serial);
    int fwd_dvae(const StepInputs& in, const Lane& L);
    int fwd_decoder(const Lane& L, bool with_ce = true);
    int dvae_decode(int B, float* drecon, const Lane& L, const float* zin = nullptr);
    int bwd_decoder(const Lane& L);
    int bwd_encoder(const Lane& L, BwdDvae fork = BwdDvae::SerialLast);      // AtSlotAttention forks (and joins) the step's dVAE backward here
    int bwd_dvae(const Lane& L);
    int pack_bcdec(const Lane& L);
    int fwd_bcdec(const Lane& L);
    int bwd_bcdec(const Lane& L);
    AttnArgs self_attn_args(int b) const;          // the fields of block b's causal self attention that forward and backward share
    XaHost xattn_args(int b) const;                // the same for its folded cross attention

    // ---- the three lanes.  The scratch pointers are assigned in layout_workspace and nowhere else.
    Lane main_lane(hipStream_t st) const { return Lane{st, scratch_, scratch_floats_}; }      // the caller's stream
    Lane dvae_lane() const { return Lane{side_, scratch2_, scratch_floats_}; }                // the dVAE branch (under use_bcdec, which has none, scratch2_ == scratch_)
    // The decoder's weight-gradient products: a stream of their own (OCRL_DW_SIDE=2), the dVAE lane (1) or the main lane (0).  The
    // operands such a product reads are never rewritten by the main stream during this backward: saved activations, and the per-block
    // gradient temporaries bg_[b] (bwd_decoder selects bg_[b] when this lane is not the main one, bg_[0] otherwise).
    Lane dw_lane(const Lane& main) const { return plan_.dw == 2 ? Lane{side2_, scratch3_, scratch_floats_} : plan_.dw ? dvae_lane() : main; }
    // The one ordering primitive: everything enqueued on `producer` so far happens before whatever is enqueued on `waiter` from now
    // on (records `ev` on producer.st, makes waiter.st wait for it; nothing when both are the same stream).  Each call site passes the
    // event object it has always used -- ev_fork_ (main -> dVAE lane), ev_join_ (dVAE lane -> main), ev_join2_ (weight-gradient stream
    // -> main), the ring (main -> weight-gradient lane, and back at the end of bwd_decoder) -- so a step issues the same record / wait
    // pairs in the same order as when they were written out at each site (one record moved: the cross-attention fold's ev_join2_ is
    // recorded where it is awaited, in fwd_decoder, not right after the fold -- nothing is enqueued on that stream in between, so it
    // marks the same point).  ev_tokens_ alone is recorded in one place (fwd_dvae, in the middle of the dVAE lane's work) and awaited
    // in another (forward).
    int after(const Lane& waiter, const Lane& producer, hipEvent_t ev);
    hipEvent_t ring_event() { return ev_dw_[ev_dw_next_++ & 7]; }

    // ---- parameters, resolved once by the constructor (resolve_params)
    struct DecBlockW { ParamPair ln1, ln2, ln3, ffn0, ffn2; ParamRef qkv, o, cq, ck, cv, co; };     // qkv: proj_q, with proj_k / proj_v behind it
    struct SlotAttnW {
        ParamRef mu, log_sigma;
        ParamPair ln, mlp0, mlp2;          // the input LayerNorm + MLP
        ParamRef w[SA_NW];                 // the slot-attention module's own weights, by SaWeight (slot_attn_host.h)
    };
    struct Weights {
        ParamPair dvae_enc[8], dvae_dec[12];       // by the reference's Sequential index (decoder 5 and 10 are pixel shuffles)
        ParamPair enc[4], enc_pos;                 // CNN encoder, positional map
        SlotAttnW sa;
        ParamPair bc[4], bc_pos;                   // broadcast decoder (use_bcdec)
        ParamRef slotproj, dict, bos, pe, out;
        ParamPair lnf;
        std::vector<DecBlockW> blk;
        long long enc_grads_end = 0;               // encode_backward() fills [group_begin(1), enc_grads_end): group 1 up to the slot projection / broadcast decoder
    } w_;
    void resolve_params();

    long long group_begin_[4] = {0, 0, 0, 0};

    // dims
    int S, E, T, N, V, d, C, K, I, D, H, NB, NH, DH, Bmax;
    int SH = 1;             // slot-attention heads
    // last step
    StepInputs last_;
    float pdrop_ = 0.f;
    bool have_fwd_ = false;
    int conv_lowlat_ = 0;           // set around the encoder of encode(): small grids take the low-latency convolution
    bool frozen_ = false, packs_valid_ = false;   // freeze_weights(): encode() re-uses the derived weight images (serving: the parameters do not change)
    bool have_enc_ = false;         // the last call was encode(): its activations are what encode_backward() differentiates
    bool enc_only_grads_ = false;   // the gradient buffer holds an encode_backward(): only the encoder tensors have gradients
    bool have_scores_ = false;        // zraw_ holds the Gumbel scores of last_ (not yet overwritten by their gradient)

    // ---- workspace tensors
    float *scratch_ = nullptr;            // transient: split-k slabs, column-sum partials, wgrad slabs (main lane)
    size_t scratch_floats_ = 0;
    float* scratch2_ = nullptr;           // scratch of the dVAE lane
    StreamPlan plan_;                     // what OCRL_OVERLAP / OCRL_DW_SIDE / OCRL_TOKENS_LATE decide (stream_plan.h), built where the streams are created: the first bind
    hipStream_t side_ = nullptr;          // dVAE forward / backward overlap the encoder + decoder work (independent branches)
    hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr, ev_tokens_ = nullptr;
    float *zstat_ = nullptr, *zhstat_ = nullptr, *zlse_ = nullptr, *zdot_ = nullptr, *cestat_ = nullptr, *celse_ = nullptr, *cepart_ = nullptr;
    int* zhidx_ = nullptr;
    float *obs8_, *patches_, *de_[7], *zraw_, *z_, *zdec_;      // zdec_: what the dVAE decoder consumes (z_ or its straight-through form)
    int* tokens_;
    float *dd0_, *dd1_, *dd2_, *dd3_, *dd4_, *ps1_, *dd6_, *dd7_, *dd8_, *dd9_, *ps2_, *recon_, *drecon_;
    float *e1_, *e2_, *e3_, *e4_, *posmap_, *gridT_, *ln0_, *ln0_mean_, *ln0_rstd_, *h1_, *x_;
    float *slots0_, *slot_noise_, *slots_, *attn_, *sa_save_, *sa_wts_, *sa_grows_, *sa_small_, *sa_xchg_;
    float* attn_heads_ = nullptr;         // [B,N,SH*K] per-head attention maps (SH > 1 only)
    float* sa_parts_;
    PackEntry* sa_pack_dev_ = nullptr;    // sa_pack_table on the device
    int sa_pack_n_ = 0, sa_pack_max_ = 0;
    float *cw_fwd_[4], *cw_bwd_[4];       // CNN encoder conv packs
    int conv_x3_ = 0;                     // OCRL_CONV_X3=1 (exploratory): the 5x5 / 64-channel layers on the split-precision bf16 kernel
    std::map<const float*, const float*> x3_of_;      // fp32 pack -> its split-precision pack
    float *dw_fwd_[2], *dw_bwd_[2];       // dVAE decoder 3x3 conv packs
    float *w11p_;                         // [4,64] padded copy of the dVAE output conv
    float *mem_, *emb_;
    struct Blk {
        float *ln1, *ln1_mean, *ln1_rstd, *q, *k, *v, *lse, *ao, *x1;
        float *ln2, *ln2_mean, *ln2_rstd, *cq, *ck, *cv, *cP, *cao, *x2;
        float *ln3, *ln3_mean, *ln3_rstd, *f1, *x3;
        float *xaAb, *xaAbT, *xaVo, *xaVoT;       // folded cross-attention operands per image (xattn.hip): [B,NC,d], [B,d,NC], [B,NC,d], [B,d,NC]
    };
    int sa_input_ = 1;                    // OCRL_SA_INPUT (default 1): 1 fused input LayerNorm + MLP both ways, 2 forward only, 0 the unfused chain
    bool xattn_ = false;                  // OCRL_XATTN (default 1): cross attention in its folded form (one launch per block and direction)
    float *xa_dAb_ = nullptr, *xa_dVo_ = nullptr, *xa_pq_ = nullptr, *xa_po_ = nullptr;
    size_t xa_zero_floats_ = 0;           // the per-block operand buffers form one contiguous region that bind() zeroes (padding columns)
    float* xa_zero_base_ = nullptr;
    std::vector<Blk> blk_;
    // per-block gradient temporaries that a weight-gradient product on the side stream may still be reading while the main stream has
    // moved on: the dropout-backward copies of the residual gradient at the three branch outputs, d ffn-hidden, d cross-attention query,
    // d q|k|v (OCRL_DW_SIDE; without it every block uses the first set)
    struct BlkG { float *gbr[3], *gf1, *gt2, *gqkv, *xaPd, *xaDs; };
    std::vector<BlkG> bg_;
    // inference path of the RL feature extractor (sb3s/ocr_extractor.py:45) at tiny batches: the ~30 launches of encode() are captured once
    // per batch size into a hipGraph and replayed (OCRL_ENCODE_GRAPH=1, opt-in: measured no faster; B <= 32, device RNG).  The observation is staged into a
    // fixed buffer and the seed passed through device memory, so a replay sees new inputs.
    struct EncGraph { hipGraphExec_t exec = nullptr; int warm = 0; };
    std::map<int, EncGraph> enc_graphs_;
    int enc_graph_mode_ = -1;
    hipStream_t cap_ = nullptr;
    float* obs_stage_ = nullptr;
    unsigned long long* seed_dev_ = nullptr;
    hipStream_t side2_ = nullptr;         // the decoder's weight-gradient products when plan_.dw == 2
    float* scratch3_ = nullptr;           // scratch of the weight-gradient stream
    hipEvent_t ev_dw_[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_join2_ = nullptr;
    int ev_dw_next_ = 0;
    float *attn_delta_;                   // [B,h,T] scratch of the attention backward
    float *attn_ds_ = nullptr;            // dS tiles of its hand-off form (null: the two-kernel form)
    size_t attn_ds_floats_ = 0;           // attn_bwd_ds_carve_floats at max_batch, asked once by the constructor: the sizing pass and bind() lay out the same workspace
    float *lnf_, *lnf_mean_, *lnf_rstd_, *pred_;
    // gradient temporaries
    float *gqkv_;                         // [BT, 3d] fused dq|dk|dv
    float *gx_, *gbr_, *gt1_, *gt2_, *gt3_, *gf1_, *gmem_, *gck_, *gcv_, *gslots_, *gslots0_;
    float *gA_, *gB_, *gC_;               // [B*N,64] (CNN encoder / slot-attention input gradients)
    float *gdA_, *gdB_;                   // dVAE decoder gradient ping-pong (up to [B*4T,256])
    float *gmap_;
    float *col0_, *dw0p_;                 // first conv layer, obs_channels != 3: im2col of the observation and the [64, 25*ch (+pad)] gradient product
    float* obs_keep_ = nullptr;           // obs_channels == 3: the observation as given (NCHW), kept for the first layer's weight gradient
    bool first_direct() const { return cfg.obs_channels == 3; }       // first layer on csrc/conv_first.hip
    // broadcast decoder (use_bcdec)
    float *bc_Wc_, *bc_W1r_, *bc_P1_, *bc_M_, *bc_T_, *bc_c1_, *bc_c2_, *bc_c3_, *bc_out4_, *bc_dout4_, *bc_gA_, *bc_gB_;
    float *bc_pk_[2], *bc_pkb_[2], *bc_Wk4_, *bc_Wb4_, *bc_dW1r_, *bc_dWc_, *bc_dT_, *bc_dM_, *bc_G1_;
};
