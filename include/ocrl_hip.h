/* ocrl_hip — C ABI of the MI355X-native SLATE / Slot-Attention pre-training path.
 *
 * The reference (ugadiarov-la-phystech-edu/OCRL) is pure Python and has no native boundary of
 * its own; each entry point below names the reference function(s) whose arithmetic it replaces.
 * Conventions: every function returns 0 on success, non-zero on error with a thread-local message
 * from ocrl_last_error(); nothing throws across the ABI.  All pointers are DEVICE pointers to
 * fp32 (unless noted), 16-byte aligned, caller-owned; `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  No call synchronises the device unless stated.  One handle per
 * process per GPU; calls on a handle are not thread-safe.
 */
#ifndef OCRL_HIP_H
#define OCRL_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCRL_ABI_VERSION 5

const char* ocrl_last_error(void);
int ocrl_abi_version(void);

/* ---- model handle: SLATE_Module + SLATE/Base optimiser (ocrs/slate/slate_module.py:23-121,
 *      ocrs/slate/slate.py:13-34, ocrs/base.py:8-25) */
typedef struct ocrl_slate ocrl_slate;
typedef struct ocrl_slate_config {
    int obs_size, obs_channels;                 /* env_config.obs_size / obs_channels */
    int vocab_size, d_model;                    /* ocr_config.dvae.* */
    int cnn_hidden;                             /* ocr_config.cnn.hidden_size (must be 64) */
    int num_slots, num_iterations, slot_size, mlp_hidden;   /* ocr_config.slotattr.* */
    int num_dec_blocks, num_dec_heads;          /* ocr_config.tfdec.* */
    float dropout;                              /* ocr_config.learning.dropout */
    int max_batch;                              /* workspace is sized for this many images */
    int use_bcdec;                              /* ocr_config.use_bcdec: Slot-Attention configuration (broadcast decoder) */
    int hard;                                   /* ocr_config.hard: straight-through Gumbel sample into the dVAE decoder */
    int num_slot_heads;                         /* ocr_config.slotattr.num_slot_heads (ocrs/common/slot_attn.py:28,54-92); 0 is read as 1.
                                                 * heads > 1: heads * num_slots <= 16, num_slots <= 8, (slot_size / heads) % 16 == 0 */
} ocrl_slate_config;

/* sizeof(ocrl_slate_config) as this library was built: a binding checks its own struct against it before ocrl_slate_create */
size_t ocrl_slate_config_size(void);
int ocrl_slate_create(const ocrl_slate_config* cfg, ocrl_slate** out);
void ocrl_slate_destroy(ocrl_slate* h);

/* Parameter inventory in the reference's state_dict names and optimiser-group order
 * (slate_module.py:94-121): group 0 dvae, 1 enc/enc_pos/slotattn/slotproj, 2 dict/bos/pos/tfdec/out.
 * offset/numel are in floats inside the flat buffers handed to ocrl_slate_bind; every tensor
 * starts 16-byte aligned (gaps are zero and inert). */
int ocrl_slate_param_count(const ocrl_slate* h);
int ocrl_slate_param_info(const ocrl_slate* h, int i, char* name, int name_cap, int shape[4], int* ndim,
                          long long* offset, long long* numel, int* group);
long long ocrl_slate_flat_size(const ocrl_slate* h);
long long ocrl_slate_group_begin(const ocrl_slate* h, int group);      /* group in 0..3 (3 = end) */
size_t ocrl_slate_workspace_bytes(const ocrl_slate* h);

/* Adopt caller-allocated (e.g. torch) flat parameter / gradient / Adam-moment buffers of
 * ocrl_slate_flat_size() floats and a workspace of ocrl_slate_workspace_bytes() bytes, all
 * 256-byte aligned.  m/v may be NULL for inference.  Synchronises the device once. */
int ocrl_slate_bind(ocrl_slate* h, float* params, float* grads, float* adam_m, float* adam_v, void* workspace, size_t workspace_bytes);

/* SLATE_Module.get_loss (slate_module.py:198-241), masks=None path.  obs: [B,3,S,S] NCHW in [0,1].
 * noise_z / noise_zh: optional injected Exp(1) draws laid out [B,T,V] (the reference's two
 * torch.empty_like(logits).exponential_() tensors permuted to channel-last, utils.py:77);
 * noise_slots: optional injected N(0,1) [B,K,D] (slot_attn.py:155).  NULL = draw on device from
 * `seed`.  train != 0 enables dropout (masks derived from `seed`).  Results: ocrl_slate_metrics. */
int ocrl_slate_forward(ocrl_slate* h, const float* obs, int B, float tau, int train, unsigned long long seed,
                       const float* noise_z, const float* noise_zh, const float* noise_slots, void* stream);
/* loss.backward() of the last forward: fills the flat gradient buffer (overwrites). */
int ocrl_slate_backward(ocrl_slate* h, void* stream);
/* SLATE_Module.forward (slate_module.py:181-196): slots [B,K,D] and attention [B,N,K] only. */
int ocrl_slate_encode(ocrl_slate* h, const float* obs, int B, unsigned long long seed, const float* noise_slots, void* stream);
/* Backward of the last ocrl_slate_encode for a downstream loss (poolings/base.py:53-55, learn_downstream_loss=True: the slots enter the
 * pooling head undetached): dslots [B,K,D] -> the flat gradient buffer, overwritten: gradients of the CNN encoder, the positional
 * embedding and the slot-attention module; zeros elsewhere.  The next ocrl_slate_clip_adam then steps those tensors only (learning rate
 * lr[1]), as torch's Adam skips parameters without a gradient. */
int ocrl_slate_encode_backward(ocrl_slate* h, const float* dslots, void* stream);
/* Serving with a frozen encoder (sb3s/ocr_extractor.py:33-36 with a pre-trained checkpoint and finetuning off): on != 0 promises that
 * the parameters do not change until the next call with on = 0 (or a clip_adam / bind), so ocrl_slate_encode builds the derived
 * weight images once instead of at every call.  Writing the flat parameter buffer while frozen leaves them stale. */
int ocrl_slate_freeze_weights(ocrl_slate* h, int on);
/* SLATE_Module._gen_imgs (slate_module.py:163-179): greedy autoregressive token decode from the slots of the last
 * forward/encode, then dVAE decode into the "recon" tensor; metrics[4] = sum (obs - recon_tf)^2 / B.  Destroys the
 * activations of the last forward (no ocrl_slate_backward afterwards). */
int ocrl_slate_generate(ocrl_slate* h, void* stream);
/* clip_grad_norm_(params, clip, "inf") + Adam(3 groups).step() (base.py:65-72, slate.py:19-34):
 * grads are first scaled by grad_scale (1/world_size after an all-reduce sum), clip <= 0 disables
 * clipping, `step` is the 1-based Adam step count.  metrics[3] receives max|g| before scaling. */
int ocrl_slate_clip_adam(ocrl_slate* h, const float lr[3], float clip, int step, float grad_scale, void* stream);
int ocrl_slate_grad_norm(ocrl_slate* h, void* stream);
/* device float[8]: [0] dvae_mse (mse with use_bcdec), [1] cross_entropy, [2] loss, [3] max|grad|, [4] mse of ocrl_slate_generate */
float* ocrl_slate_metrics(const ocrl_slate* h);
/* Named tensors of the last step ("slots" [B,K,D], "attn" [B,N,K], "recon" [B,S,S,4], "tokens"
 * (int32) [B,T], "zraw" [B,T,V] (soft models: the Gumbel scores (logits + g)/tau until the backward overwrites them with d logits;
 * hard=True: the raw logits), "z" [B,T,V] (see ocrl_slate_soft_z), "z_lse"/"ce_lse" [B,T], "feats" [B,N,64], "dec_out" [B,T,d],
 * "pred" (the output-head logits), "mem", "emb",
 * "slots0", "sa_inputs") or any parameter name; count = capacity in elements at max_batch. */
int ocrl_slate_tensor(const ocrl_slate* h, const char* name, float** ptr, long long* count);
/* The soft Gumbel sample z = softmax((logits + g) / tau) of the last forward (ocrs/slate/slate_module.py:126, the `z` that
 * get_loss(with_rep=True) returns, :239-241) written into the named tensor "z".  The training step itself never materialises it:
 * the vocabulary products rebuild it from the stored scores ("zraw") and their row log-sum-exp ("z_lse").  Call between forward and
 * backward; a no-op for hard=True models, whose forward writes "z" / "z_st" itself. */
int ocrl_slate_soft_z(ocrl_slate* h, void* stream);
/* The keep-mask (float 0/1) the kernels used for a dropout site in the last forward; site ids:
 * 1 = z_pos, 16 + 8*block + {0 self.attn, 1 self.out, 2 cross.attn, 3 cross.out, 4 ffn}. */
int ocrl_slate_dropout_mask(const ocrl_slate* h, unsigned site, long long n, float* out, void* stream);

/* ---- unit entry points (parity tests of the MFMA kernels)
 * C[M,N] = alpha * op(A) op(B) (+bias[n]) (relu) (* (mask>0)) (+resid); akc/bkc select storage:
 * akc=1: A is [M,K] row-major, else [K,M]; bkc=1: B is [N,K] row-major (torch Linear weight), else [K,N].
 * splitk > 1 needs ws of splitk*M*N floats and ldc == N. */
int ocrl_gemm(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int akc, int bkc,
              float alpha, const float* bias, int relu, const float* mask, int ldmask, const float* resid, int ldr,
              int splitk, float* ws, void* stream);
/* The same GEMM with every argument the kernel takes (unit tests of each instantiation; csrc/kernels.h GemmArgs documents the fields).
 * Fields left zero by memset are the defaults except alpha, x_scale and e_scale (set them to 1), batch, batch_inner and splitk (>= 1)
 * and force_sb (-1 = the dispatch rule, 0 = double-buffered LDS, 1 = single).  force_tile: 0 = the rule, else BM*1000 + BN; a forced
 * combination that is not built is an error.  splitk > 1 needs ldc == N and no epilogue; ws then holds splitk*M*N floats of partial
 * products, plus splitk*sBias floats of bias partials when bias_out is set (sBias 0: M rounded up to 4); both are summed into C and
 * bias_out.  ocrl_gemm_plan reports the kernel the arguments select, out = {BM, BN, single_buffer, xf, epi, 2*akc + bkc} (xf: 0 plain
 * operands, 1 A-operand dropout, 2 soft-max operand transforms; epi = epi_mode); host only, pointers are only checked for alignment. */
typedef struct ocrl_gemm_desc {
    const float* A; const float* B; float* C;
    int M, N, K, lda, ldb, ldc;
    int akc, bkc;
    int batch, batch_inner;
    long long sA, sB, sC, sAi, sBi, sCi;
    int splitk; float alpha;
    const float* bias; int relu;
    float drop_p; unsigned long long drop_seed; unsigned drop_site;
    const float* mask; int ldmask; long long sMask; int mask_elu;
    const float* resid; int ldr; long long sR;
    float adrop_p; unsigned adrop_site; int adrop_ld;
    float* bias_out; long long sBias;
    int a_mode, b_mode; const float* x_lse; const int* x_tok; float x_scale;
    int epi_mode; float* stat; float* hstat; int* hidx; const float* e1; const float* e2; unsigned long long e_seed;
    const float* e_lse; const float* e_rowvec; float e_scale;
    int force_tile, force_sb;
} ocrl_gemm_desc;
size_t ocrl_gemm_desc_size(void);
int ocrl_gemm_ex(const ocrl_gemm_desc* d, float* ws, size_t ws_floats, void* stream);
int ocrl_gemm_plan(const ocrl_gemm_desc* d, int out[6]);
/* F.conv2d(x, w, b, stride 1, padding ks/2) on NHWC x [B,H,W,cin_pad] (cin_pad = 8 or 64; channels >= cin are
 * zero) with the reference-layout weight w [64,cin,ks,ks]; y [B,H,W,64] NHWC.  ws: ks*ks*cin_pad*64 floats. */
int ocrl_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int cin, int cin_pad, int ks,
                    int relu, float* ws, void* stream);
/* The same convolution for a few images at a time (the RL extractor's encode(): sb3s/ocr_extractor.py:45 at num_envs images): 5x5 /
 * 64-channel layers whose grid would leave most of the GPU idle run a kernel that splits one output tile over four waves and two
 * workgroups (k-split, ordered sum).  Same arguments and result up to fp32 summation order; other shapes take the kernel above. */
int ocrl_conv2d_fwd_lowlat(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int cin, int cin_pad, int ks,
                           int relu, float* ws, void* stream);
/* EXPLORATORY, not on any default path: the ks x ks (5 or 3) / 64 -> 64 layer (forward, and backward-data with the ReLU mask) on the bf16
 * matrix pipe, every fp32 operand split exactly into three bf16 numbers and six products accumulated in fp32 (csrc/conv_x3.hip).  NHWC
 * [B,H,W,64], reference-layout weight [64,64,ks,ks]; ws: ocrl_conv2d_x3_ws_floats() floats. */
size_t ocrl_conv2d_x3_ws_floats(void);
int ocrl_conv2d_fwd_x3(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int ks, int relu, float* ws, void* stream);
int ocrl_conv2d_bwd_data_x3(const float* dy, const float* w, const float* mask, float* dx, int B, int H, int W, int ks, float* ws, void* stream);
/* its weight gradient [64,64,ks,ks]; ws from ocrl_conv2d_wgrad_ws_floats(B, H, W, ks, 64) */
int ocrl_conv2d_bwd_weight_x3(const float* x, const float* dy, float* dw, int B, int H, int W, int ks, float* ws, size_t ws_floats, void* stream);
/* grad wrt input of the same conv (square 64->64 layers): dx = conv_transpose(dy, w) * (mask > 0 if mask). ws: 2*ks*ks*64*64 floats. */
int ocrl_conv2d_bwd_data(const float* dy, const float* w, const float* mask, float* dx, int B, int H, int W, int ks, float* ws, void* stream);
/* grad wrt weight (reference layout [64,cin,ks,ks]) and bias [64] (may be NULL); ws from ocrl_conv2d_wgrad_ws_floats: the kernel's
 * partial dW slabs, then 65536 floats that hold its bias partials (64 per slab). */
size_t ocrl_conv2d_wgrad_ws_floats(int B, int H, int W, int ks, int cin_pad);
int ocrl_conv2d_bwd_weight(const float* x, const float* dy, float* dw, float* db, int B, int H, int W, int cin, int cin_pad, int ks,
                           float* ws, size_t ws_floats, void* stream);
/* The same convolution kernels with every argument they take (unit tests of each instantiation and epilogue; csrc/kernels.h ConvArgs
 * documents the fields).  x [B,H,W,cin_pad], y [B,H,W,64] NHWC, w [64,cin,ks,ks] in the reference layout; (ks, cin_pad) is (5, 64),
 * (5, 8) or (3, 64).  Epilogue in this order: + bias[co]; relu = 1 ReLU, 2 ELU; + posmap [H,W,64]; mask [B,H,W,64]: v where m > 0,
 * else 0, or v * (m + 1) with mask_elu (m = the ELU output of the layer below, so m + 1 = ELU'(pre-activation)).  transposed = 1 packs
 * the flipped taps with ci / co swapped, the backward-data form (x = dy, y = dx; needs cin = cin_pad = 64).  low_latency = 1 asks for the
 * k-split kernel, which serves 5x5 / 64 channels, relu <= 1, no mask, at most 160 tiles; every other request runs the throughput kernel.
 * ws: ks*ks*cin_pad*64 floats, twice that when transposed (the packs, laid out as ocrl_conv2d_fwd / ocrl_conv2d_bwd_data lay them out).
 * Every pointer 16-byte aligned; fields left zero by memset are "absent".  An unsupported combination is an error, never another kernel. */
typedef struct ocrl_conv_desc {
    const float* x; const float* w; float* y;
    int B, H, W, cin, cin_pad, ks;
    const float* bias; int relu;
    const float* posmap; const float* mask; int mask_elu;
    int transposed, low_latency;
} ocrl_conv_desc;
size_t ocrl_conv_desc_size(void);
int ocrl_conv2d_ex(const ocrl_conv_desc* d, float* ws, size_t ws_floats, void* stream);
/* ocrl_conv2d_bwd_weight with the accumulate switch of the model paths: accumulate = 1 gives dw += and db += (IODINE sums the decoder's
 * weight gradients over its refinement iterations), 0 overwrites.  db may be NULL; ws from ocrl_conv2d_wgrad_ws_floats. */
typedef struct ocrl_conv_wgrad_desc {
    const float* x; const float* dy; float* dw; float* db;
    int B, H, W, cin, cin_pad, ks;
    int accumulate;
} ocrl_conv_wgrad_desc;
size_t ocrl_conv_wgrad_desc_size(void);
int ocrl_conv2d_bwd_weight_ex(const ocrl_conv_wgrad_desc* d, float* ws, size_t ws_floats, void* stream);
/* The encoder's first layer alone: 5x5, 3 -> 64 channels, stride 1, padding 2, on the NCHW observation obs [B,3,H,W] (no channel padding,
 * no NHWC copy).  y [B,H,W,64] = conv(obs, w [64,3,5,5]) + bias (may be NULL), ReLU if relu = 1.  An image's result does not depend on B. */
size_t ocrl_conv2d_first_fwd_ws_floats(void);
int ocrl_conv2d_first_fwd(const float* obs, const float* w, const float* bias, float* y, int B, int H, int W, int relu, float* ws, size_t ws_floats,
                          void* stream);
/* its weight gradient dw [64,3,5,5] and bias gradient db [64] (may be NULL) from dy [B,H,W,64], without a patch matrix; accumulate = 1 adds
 * to dw / db.  The workspace holds one partial of 64 * 96 + 64 floats per worker (at most 512, one per 4 x 32 pixel tile below that). */
size_t ocrl_conv2d_first_wgrad_ws_floats(int B, int H, int W);
int ocrl_conv2d_first_bwd_weight(const float* obs, const float* dy, float* dw, float* db, int B, int H, int W, int accumulate, float* ws, size_t ws_floats,
                                 void* stream);
/* nn.LayerNorm(F) forward / backward over R rows (F in {64,128,192,256}); dgb = [dgamma | dbeta]. */
int ocrl_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long long R, int F, void* stream);
int ocrl_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx, float* dgb,
                       long long R, int F, float* ws, size_t ws_floats, void* stream);

/* The slot-attention input chain x = W2 relu(W0 LN(e4) + b0) + b2 over R rows of 64 (SlotAttentionModule: layer_norm, mlp), one kernel per
 * direction.  Forward: mean, rstd [R], h1, x [R,64] are bitwise what ocrl_layernorm_fwd followed by two ocrl_gemm_ex (bias, ReLU) give.
 * Backward: de4 is bitwise the unfused chain's; dW0, db0, dW2, db2, dgamma, dbeta are written from one partial slab per workgroup, summed
 * in a fixed order (no atomics).  ws: workgroups * slab floats, both reported by ocrl_sa_input_plan, out = {tile rows, workgroups of the
 * backward at max_wgs = 0 (one slab each), slab floats}; max_wgs > 0 caps the workgroups of either direction (they walk the tiles with
 * that stride).  All tensors 16-byte aligned. */
int ocrl_sa_input_plan(long long R, int out[3]);
int ocrl_sa_input_fwd(const float* e4, const float* gamma, const float* beta, const float* W0, const float* b0, const float* W2, const float* b2,
                      float* mean, float* rstd, float* h1, float* x, long long R, int max_wgs, void* stream);
int ocrl_sa_input_bwd(const float* dx, const float* h1, const float* e4, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      const float* W0, const float* W2, float* de4, float* dW0, float* db0, float* dW2, float* db2, float* dgamma, float* dbeta,
                      long long R, int max_wgs, float* ws, size_t ws_floats, void* stream);

/* Causal multi-head self-attention core of MultiHeadAttention.forward (ocrs/common/transformer.py:31-47): q,k,v are the
 * projected [B,T,d] tensors (row stride ld >= d, heads side by side, q unscaled); o = dropout(softmax(mask(q k^T / sqrt(dh)))) v
 * as [B,T,d]; lse [B,h,T] is saved for the backward.  Dropout decisions come from (seed, site) as in ocrl_slate_forward: the
 * probability of (b, head, query, key) is element ((b*h + head)*T + query)*T4 + key of the site's stream, T4 = T rounded up to a
 * multiple of 4 (the site's mask dump is [B,h,T,T4], of which [..., :T] is used; dense [B,h,T,T] when T % 4 == 0).
 * Every output element is written, none is read: o, lse, dq, dk, dv and delta need no initialisation. */
int ocrl_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int T, int d, int h, int ld,
                       float p, unsigned long long seed, unsigned site, void* stream);
/* gradients dq,dk,dv (row stride ld) from dO [B,T,d]; delta is scratch [B,h,T]. */
int ocrl_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* dO,
                       float* dq, float* dk, float* dv, float* delta, int B, int T, int d, int h, int ld,
                       float p, unsigned long long seed, unsigned site, void* stream);
/* The same backward with a dS workspace (hand-off form: the dK/dV kernel stores the score gradients it forms, the dQ kernel is the one
 * product dS K that reads them; dk and dv are bit for bit those of ocrl_attention_bwd's two-kernel form).  ds is uninitialised scratch,
 * 16-byte aligned; ocrl_attention_bwd_ds_floats(B, T, h) floats hold the whole batch, a smaller ds_floats makes the call walk the batch
 * in chunks of floor(ds_floats / ocrl_attention_bwd_ds_floats(1, T, h)) images with the same results, and with room for less than one
 * image (or ds null) the call is ocrl_attention_bwd's two-kernel form.  OCRL_ATTN_BWD unset or 3 runs this form; 1 and 2 keep their
 * meanings (the one-pass and the two-kernel form). */
size_t ocrl_attention_bwd_ds_floats(int B, int T, int h);
int ocrl_attention_bwd_ws(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* dO,
                          float* dq, float* dk, float* dv, float* delta, int B, int T, int d, int h, int ld,
                          float p, unsigned long long seed, unsigned site, float* ds, size_t ds_floats, void* stream);

/* ---- Cross attention of a decoder block to the K projected slots (MultiHeadAttention.forward, ocrs/common/transformer.py:23-50, as
 * TransformerDecoderBlock.forward :181-185 calls it with k = v = the slot memory), in the two forms the decoder runs.
 *
 * Folded form (csrc/xattn.hip): y = resid + dropout_o(softmax_dropout_p(x Wq^T (mem Wk^T)^T / sqrt(d/h)) (mem Wv^T) Wo^T) with the two
 * projections around the attention folded into per-image operands.  ocrl_xattn_plan reports the form a shape runs, host only:
 * out = {supported (0/1), KP, NC, NM, dynamic LDS bytes of the forward / backward kernel}.  Supported: 1 <= K <= 16, d in {64, 128, 192,
 * 256}, h | d, (d/h) % 4 == 0 and NC = h * KP in {16, 32, 64}, where KP (slots per head after padding) is 8 for K <= 8 and h > 1, else
 * 16; NM = d / 16.  That is h in {1, 2, 4, 8} at K <= 8 and h in {1, 2, 4} at K > 8; an unsupported shape gives out = {0, 0, 0, 0, 0} (the
 * model then runs the plain form), and _fwd / _bwd refuse it with a message and launch nothing.
 * Column layout of the padded operands: col = head * KP + slot.
 *   ocrl_xattn_fwd: the fold (ck, cv [B,K,d] = mem Wk^T, mem Wv^T; Ab [B,NC,d], AbT [B,d,NC], Vo [B,NC,d], VoT [B,d,NC]), then the
 *     attention: y [B,T,d] and P [B,h,T,K] (probabilities before dropout).  ck, cv, y, P are written in full and need no initialisation.
 *     Of Ab / AbT / Vo / VoT only the columns of real slots are written: the CALLER ZEROES these four buffers once, and the padding columns
 *     (slot >= K of every head) stay zero through every call.
 *   ocrl_xattn_bwd (after _fwd, same descriptor): from gd [B,T,d], the gradient wrt the attention branch's output after the output
 *     dropout's backward (gd = dy * keep_o / (1 - p)), it writes Pd [B*T,NC] = P * keep_p / (1 - p) and dS [B*T,NC] (score gradients;
 *     padding columns of both are written as zero), dx [B,T,d] (gradient wrt x through the attention branch only), the per-image sums
 *     dVo, dAb [B,NC,d], then dck, dcv [B,K,d], the per-image partials pq, po [B,d,d] and dWq, dWo [d,d] (the partials summed over the
 *     images in a fixed order).  Every one of them is written, none is added to.  cs_ws: scratch of cs_ws_floats >= d * d floats; B <= 64.
 * Dropout index contract (seed as in ocrl_slate_forward): the keep decision of probability (b, head, t, slot) is element
 * ((b*h + head)*T + t)*K + slot of site_p's stream (K % 4 != 0 included: rows then start off the group of four); that of output element
 * (b, t, o) is element (b*T + t)*d + o of site_o's stream.  Results are bitwise reproducible, and an image's results do not depend on B. */
typedef struct ocrl_xattn_desc {
    const float* x; const float* resid; const float* mem;            /* [B,T,d] LN output, [B,T,d] residual stream, [B,K,d] projected slots */
    const float* Wq; const float* Wk; const float* Wv; const float* Wo;      /* [d,d] (out, in) */
    float* ck; float* cv; float* Ab; float* AbT; float* Vo; float* VoT; float* y; float* P;
    const float* gd;
    float* Pd; float* dS; float* dx; float* dAb; float* dVo; float* dck; float* dcv; float* dWq; float* dWo;
    float* pq; float* po; float* cs_ws; size_t cs_ws_floats;
    int B, T, K, d, h;
    float p; unsigned long long seed; unsigned site_p, site_o;
} ocrl_xattn_desc;
size_t ocrl_xattn_desc_size(void);
int ocrl_xattn_plan(int K, int d, int h, int out[5]);
int ocrl_xattn_fwd(const ocrl_xattn_desc* d, void* stream);
int ocrl_xattn_bwd(const ocrl_xattn_desc* d, void* stream);
/* Plain form (csrc/elementwise.hip), the attention core alone: Q [B,T,d] (projected, unscaled), Km, Vm [B,K,d], heads side by side;
 * O [B,T,d] = dropout(softmax(Q Km^T / sqrt(d/h))) Vm and P [B,h,T,K] (before dropout) are written.  1 <= K <= 16 (K <= 8 and K > 8 run
 * different instantiations), (d/h) % 4 == 0, d/h <= 64.  Dropout as site_p above.  _bwd writes dQ [B,T,d], dKm, dVm [B,K,d] (none is
 * added to); ws: ocrl_cross_attn_bwd_ws_floats floats (one partial per (image, head, block of 256 queries), summed in a fixed order). */
int ocrl_cross_attn_fwd(const float* Q, const float* Km, const float* Vm, float* O, float* P, int B, int T, int K, int d, int h, float p,
                        unsigned long long seed, unsigned site, void* stream);
size_t ocrl_cross_attn_bwd_ws_floats(int B, int T, int K, int d, int h);
int ocrl_cross_attn_bwd(const float* dO, const float* Q, const float* Km, const float* Vm, const float* P, float* dQ, float* dKm, float* dVm,
                        int B, int T, int K, int d, int h, float p, unsigned long long seed, unsigned site, float* ws, size_t ws_floats,
                        void* stream);

/* ---- optional HIP-event timing of kernel families on the launch stream (bench.py's roofline line).
 * tag bits: 0 conv5x5/64ch fwd+bwd-data, 1 other convs, 2 conv weight-grad, 3 gemm, 4 slot-attn fwd, 5 slot-attn bwd,
 * 6 self-attention fwd, 7 self-attention bwd.
 * ocrl_prof_collect synchronises the device and returns total milliseconds / launch counts per tag. */
/* Input pipeline on the device: utils/datasets.py:13-24 (`torch.Tensor(obss[i]).permute(2, 0, 1) / 255.0`) + to_device
 * (utils/tools.py:182-191, train_ocr.py:52-53).  The host uploads the dataset's uint8 HWC images as they are (a quarter of the
 * fp32 bytes over PCIe); obs_chw = obs_hwc / 255 as correctly rounded fp32, bit-identical to the reference's conversion. */
int ocrl_obs_u8_to_f32(const unsigned char* obs_hwc, float* obs_chw, int B, int H, int W, int C, void* stream);

int ocrl_prof_enable(unsigned tag_mask);
int ocrl_prof_collect(double* ms, long long* count, int ntags);

/* ---- the slot-attention loop on its own (SlotAttention.forward, ocrs/common/slot_attn.py:47-102; single head) ----
 * x [B,N,64] inputs (before norm_inputs), slots0 [B,K,D]; `w` = 17 device pointers in the reference's parameter order:
 * norm_inputs.{weight,bias}, norm_slots.{weight,bias}, norm_mlp.{weight,bias}, project_q / project_k / project_v .weight,
 * gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh, mlp.0.{weight,bias}, mlp.2.{weight,bias}.
 * Outputs: slots [B,K,D], attn [B,N,K] (last iteration, before the epsilon; may be NULL).  The workspace keeps the saved
 * activations: call _bwd with the same ws right after _fwd.  _bwd: dslots [B,K,D] -> dx [B,N,64], dslots0 [B,K,D] and the
 * 17 weight gradients `dw` (same order and shapes).  Slot / MLP widths: multiples of 64 up to 256; 1 <= K <= 16. */
size_t ocrl_slot_attention_ws_floats(int B, int K, int D, int H, int I);
int ocrl_slot_attention_fwd(const float* x, const float* slots0, const float* const* w, float* slots, float* attn, int B, int N, int K, int D,
                            int H, int I, float* ws, size_t ws_floats, void* stream);
int ocrl_slot_attention_bwd(const float* x, const float* dslots, float* dx, float* dslots0, float* const* dw, int B, int N, int K, int D, int H,
                            int I, float* ws, size_t ws_floats, void* stream);
/* the same with `heads` attention heads (ocrs/common/slot_attn.py:28,54-92: q / k / v split into heads, soft-max over heads * K columns,
 * attn = sum over the heads): heads * K <= 16, K <= 8 and (D / heads) % 16 == 0 when heads > 1; heads = 1 is the pair above. */
size_t ocrl_slot_attention_mh_ws_floats(int B, int N, int K, int D, int H, int I, int heads);
int ocrl_slot_attention_mh_fwd(const float* x, const float* slots0, const float* const* w, float* slots, float* attn, int B, int N, int K, int D,
                               int H, int I, int heads, float* ws, size_t ws_floats, void* stream);
int ocrl_slot_attention_mh_bwd(const float* x, const float* dslots, float* dx, float* dslots0, float* const* dw, int B, int N, int K, int D, int H,
                               int I, int heads, float* ws, size_t ws_floats, void* stream);
/* the form _fwd / _bwd run for these sizes, from the host function their launch path dispatches on (no device needed):
 * out = {G images per slot-side workgroup, NB row blocks, KB rows per block, dynamic LDS bytes of the forward slot-side kernel, of the
 * backward one, KS = heads * K soft-max columns of the streaming kernels}.  heads = 1, K <= 8: G = 16 / K while both LDS requests fit
 * the 163,584 bytes a workgroup may take, else G = 1 (KB = G * K rows fill the 16-row matrix tile); K > 8: G = 1, NB = 2 blocks of
 * KB = (K + 1) / 2 rows; heads > 1: G = 1, KB = K.  Non-zero, with ocrl_last_error(), for sizes _fwd / _bwd refuse. */
int ocrl_slot_attention_plan(int K, int D, int H, int heads, int* out6);

/* ---- slot-set pooling head: poolings/common/transformer.py:9-33 (Transformer: Linear -> [CLS; tokens] (+pos) ->
 * nn.TransformerEncoder of post-norm ReLU layers -> CLS row), as built by poolings/transformer/transformer_module.py:27-117 with its
 * default switches; the consumer of the slots in sb3s/ocr_extractor.py:45.  SURVEY.md §8(f) rank 4.
 * slots [B,K,Din]; `w` = 3 + 12 L device pointers in the module's state_dict order: _linear.{weight [d,Din], bias},
 * _cls_token._cls_token [d], then per layer self_attn.in_proj_{weight [3d,d], bias}, self_attn.out_proj.{weight,bias},
 * linear1.{weight [ff,d], bias}, linear2.{weight [d,ff], bias}, norm1.{weight,bias}, norm2.{weight,bias}.
 * pos: [K+1,d] positional table added to the token sequence (the reference's `pe` buffers), or NULL (pos_emb "None").
 * out [B,d] = encoder output of the CLS token.  drop_p = nn.TransformerEncoderLayer's dropout in train mode (0 in eval); the keep
 * decisions are a pure function of (seed, layer, site, element) so _bwd regenerates them: pass the same drop_p and seed.
 * _bwd: dout [B,d] -> dw (same order / shapes as w; every entry is overwritten) and dslots [B,K,Din] (NULL = the slots are detached,
 * poolings/base.py:53).  Call it with the same ws right after _fwd.  d_model: multiple of 64 up to 256; K + 1 <= 32. */
#define OCRL_POOL_MAX_LAYERS 8
size_t ocrl_pool_transformer_ws_floats(int B, int K, int d, int nhead, int ff, int L);
int ocrl_pool_transformer_fwd(const float* slots, const float* const* w, const float* pos, float* out, int B, int K, int Din, int d, int nhead,
                              int ff, int L, float drop_p, unsigned long long seed, float* ws, size_t ws_floats, void* stream);
int ocrl_pool_transformer_bwd(const float* slots, const float* dout, const float* const* w, float* dslots, float* const* dw, int B, int K, int Din,
                              int d, int nhead, int ff, int L, float drop_p, unsigned long long seed, float* ws, size_t ws_floats, void* stream);
/* keep-mask (1 = kept) of one dropout site, for parity tests: which = 0 attention weights [B,h,S,S], 1 dropout1 [B,S,d],
 * 2 FFN hidden [B,S,ff], 3 dropout2 [B,S,d]; n = element count. */
int ocrl_pool_transformer_dropout_mask(int layer, int which, long long n, float drop_p, unsigned long long seed, float* out, void* stream);
/* The same head over long token sequences (the encoder's CNN feature map as tokens: K = H*W, rep_dim = channels + 3, as SLATE with
 * use_cnn_feat returns them).  Arguments, `w` order, dropout sites and keep decisions as in ocrl_pool_transformer_*; any K >= 1, any
 * Din >= 1, d_model a multiple of 64 up to 256, head size 16, 32, 48 or 64.  The workspace is linear in K: layers before the last keep
 * the log-sum-exp of their attention instead of the weights, and the last layer is evaluated for the CLS row only. */
size_t ocrl_pool_transformer_long_ws_floats(int B, int K, int Din, int d, int nhead, int ff, int L);
int ocrl_pool_transformer_long_fwd(const float* slots, const float* const* w, const float* pos, float* out, int B, int K, int Din, int d, int nhead,
                                   int ff, int L, float drop_p, unsigned long long seed, float* ws, size_t ws_floats, void* stream);
int ocrl_pool_transformer_long_bwd(const float* slots, const float* dout, const float* const* w, float* dslots, float* const* dw, int B, int K,
                                   int Din, int d, int nhead, int ff, int L, float drop_p, unsigned long long seed, float* ws, size_t ws_floats,
                                   void* stream);

/* ---- Relation Network pooling head: poolings/rn/rn_module.py:8-59 (RN_Module.forward: every ordered slot pair cat(s_i, s_j) in
 * itertools.permutations order (:33-47) -> g = [Linear, ReLU] x len(g_dims) -> sum over the K (K-1) pairs (:57) -> f = [Linear, ReLU] x
 * len(f_dims)), as built by poolings/rn/rn.py:6-9 with configs/pooling/rn.yaml; the consumer of the slots in sb3s/ocr_extractor.py:45.
 * slots [B,K,D]; `w` = 2 (ng + nf) device pointers in the module's state_dict order: _g.0.{weight [g_dims[0], 2D], bias},
 * _g.2.{weight, bias}, ..., _f.0.{weight [f_dims[0], g_dims[ng-1]], bias}, ...  out [B, f_dims[nf-1]].
 * _bwd: dout [B, f_dims[nf-1]] -> dw (same order / shapes as w; every entry is overwritten) and dslots [B,K,D] (NULL = the slots are
 * detached, poolings/base.py:53).  Call it with the same ws right after _fwd.  K >= 2; every g / f width a multiple of 4; any D >= 1;
 * 1 <= ng, nf <= OCRL_POOL_RN_MAX_LAYERS.  Shapes whose pair rows (B K (K-1)) times the widest g layer leave the int32 range of one GEMM
 * are rejected (a CNN feature map as slots).  Rejected shapes get ws_floats == 0; _fwd / _bwd return non-zero for them. */
#define OCRL_POOL_RN_MAX_LAYERS 16
size_t ocrl_pool_rn_ws_floats(int B, int K, int D, int ng, const int* g_dims, int nf, const int* f_dims);
int ocrl_pool_rn_fwd(const float* slots, const float* const* w, float* out, int B, int K, int D, int ng, const int* g_dims, int nf, const int* f_dims,
                     float* ws, size_t ws_floats, void* stream);
int ocrl_pool_rn_bwd(const float* slots, const float* dout, const float* const* w, float* dslots, float* const* dw, int B, int K, int D, int ng,
                     const int* g_dims, int nf, const int* f_dims, float* ws, size_t ws_floats, void* stream);

/* ---- NatureCNN / MultipleCNN encoders: ocrs/naturecnn/naturecnn_module.py:11-63 (configs/ocr/naturecnn.yaml) and
 * ocrs/multiple_cnns/multiple_cnn_module.py:12-38 (G = num_modules NatureCNN modules on the same image, stacked on axis 1).
 * Per module: Conv2d(cin, 32, 8, s 4) ReLU  Conv2d(32, 64, 4, s 2) ReLU  Conv2d(64, 64, 3, s 1) ReLU  [Conv2d(64, 128, 3, s 1) ReLU when
 * cnn_feat_size == 2], all padding 0; then, without use_cnn_feat, Flatten (NCHW order) and Linear(n_flatten, rep_dim) ReLU.
 * obs [B, cin, H, W] (NCHW).  out: [B, G, rep_dim] without use_cnn_feat ([B, rep_dim] for G = 1); [B, OH OW, C] (HWC tokens) with it.
 * `w` = the parameters in state_dict order, module-major for G > 1: _cnn.0.{weight, bias}, _cnn.2.*, _cnn.4.*[, _cnn.6.*][, _linear.0.*].
 * They are read on every call (nothing is packed or cached).  save != 0 leaves in ws what _bwd needs; _bwd (called with the same ws right
 * after a saving _fwd): dout (out's shape) -> dw (same order / shapes as w; every entry is overwritten, not accumulated).  The
 * observation gets no gradient.  Rejected shapes get ws_floats == 0 and fail in _fwd / _bwd: B < 1, an input below 36 x 36 (52 x 52
 * with the 4th conv), rep_dim not a positive multiple of 4, G outside 1 .. OCRL_NATURECNN_MAX_GROUPS, use_cnn_feat with G > 1. */
#define OCRL_NATURECNN_MAX_GROUPS 16
#define OCRL_NATURECNN_MAX_CONVS 4
size_t ocrl_naturecnn_ws_floats(int B, int H, int W, int cin, int groups, int cnn_feat_size, int use_cnn_feat, int rep_dim);
int ocrl_naturecnn_fwd(const float* obs, const float* const* w, float* out, int B, int H, int W, int cin, int groups, int cnn_feat_size,
                       int use_cnn_feat, int rep_dim, int save, float* ws, size_t ws_floats, void* stream);
int ocrl_naturecnn_bwd(const float* obs, const float* dout, const float* const* w, float* const* dw, int B, int H, int W, int cin, int groups,
                       int cnn_feat_size, int use_cnn_feat, int rep_dim, float* ws, size_t ws_floats, void* stream);

/* ---- NatureCNN pooling heads: poolings/cnn_linear/cnn_linear_module.py:7-14 (CNN_Linear) and the CNN front end of
 * poolings/cnn_transformer/cnn_transformer_module.py:12-40 (CNN_Transformer), both over slot_to_img(tokens) (utils/tools.py:33-36;
 * configs/pooling/cnn_linear.yaml, cnn_transformer.yaml).  poolings/common/naturecnn.py:10-29: Conv2d(D, 32, 8, s 4) ReLU
 * Conv2d(32, 64, 4, s 2) ReLU  Conv2d(64, 64, 3, s 1) ReLU, all padding 0; then, with rep_dim > 0, Flatten (NCHW order) and
 * Linear(64 OH OW, rep_dim) ReLU.  tokens [B, H W, D]: the channels-last H x W map that SLATE with use_cnn_feat returns (D = channels + 3);
 * slot_to_img is a view of it, nothing is permuted.  out: [B, rep_dim] with rep_dim > 0 (CNN_Linear); [B, OH OW, 64] (the last map as HWC
 * tokens, the pooling transformer's input) with rep_dim == 0.  `w` = the parameters in state_dict order: _net.0.{weight [32, D, 8, 8],
 * bias}, _net.2.*, _net.4.*[, _net.7.{weight [rep_dim, 64 OH OW], bias}], in torch's layouts; they are read on every call (the first
 * layer's weight is reordered into ws per call, nothing is cached).  The Linear's input width is derived from H and W.  save != 0 leaves
 * in ws what _bwd needs; _bwd (called with the same ws right after a saving _fwd): dout (out's shape) -> dw (same order / shapes as w;
 * every entry is overwritten, not accumulated) and dtokens [B, H W, D] (NULL = the tokens are detached, poolings/base.py:53; every
 * element is written, 0 at border pixels that no window covers).  Rejected shapes get ws_floats == 0 and fail in _fwd / _bwd: B < 1,
 * D < 1, a map below 36 x 36, rep_dim not a non-negative multiple of 4, index ranges past int32. */
size_t ocrl_pool_cnn_ws_floats(int B, int H, int W, int D, int rep_dim);
int ocrl_pool_cnn_fwd(const float* tokens, const float* const* w, float* out, int B, int H, int W, int D, int rep_dim, int save, float* ws,
                      size_t ws_floats, void* stream);
int ocrl_pool_cnn_bwd(const float* tokens, const float* dout, const float* const* w, float* dtokens, float* const* dw, int B, int H, int W, int D,
                      int rep_dim, float* ws, size_t ws_floats, void* stream);

/* ---- VAE representation module: ocrs/vaes/vae_module.py, ocrs/common/models.py:49-93 (VAEEncoder / VAEDecoder), configs/ocr/vae.yaml.
 * n = log2(obs_size / cnn_feat_size) stages (1 .. OCRL_VAE_MAX_STAGES), f = cnn_feat_size, L = latent_dim (a multiple of 4), C =
 * obs_channels (1 .. 4).  obs [B, C, S, S] (NCHW).  `w` = every parameter in state_dict order: _enc._encoder.{0 .. 4n - 1}.m.*,
 * _enc._encoder.4n.*, _mu.*, _var.*, _in_dec.*, _dec._decoder.0.m.*, the 4n Conv2dBlocks of the decoder stages (the PixelShuffle slots
 * have no parameters), _dec._decoder.(5n + 1).*: 2 (8n + 6) tensors, read in torch's layout on every call (packed into ws per call).
 * full = 0 (encoder only, the rollout): rep = mu [B, L], or with use_cnn_feat the encoder map as img_to_slot tokens [B, f f, 64];
 *   eps, metrics and recon are not read; only the encoder's and _mu's entries of dw are written by _bwd (the others may be NULL).
 * full = 1 (get_loss): also eps [B, L] (the reparameterisation noise), metrics [3] = (loss, mse, kld) with
 *   kld = mean_B(-0.5 sum(1 + logvar - mu^2 - exp(logvar))) (the reference's metric is -kld), recon [B, C, S, S] when not NULL.
 * _bwd (called with the same ws right after _fwd, same arguments): dloss (device scalar) is the cotangent of loss, drep (same shape as
 * rep; required when full = 0) the cotangent of rep; they are summed, and a NULL one counts as zero (dloss NULL: the decoder and KL
 * terms are skipped and the decoder-side entries of dw are zeroed).  dw: same order / shapes as w, overwritten.
 * The observation gets no gradient.  Rejected shapes get ws_floats == 0 and fail in _fwd / _bwd. */
#define OCRL_VAE_MAX_STAGES 6
size_t ocrl_vae_ws_floats(int B, int obs_size, int obs_channels, int cnn_feat_size, int latent_dim, int use_cnn_feat, int full);
int ocrl_vae_fwd(const float* obs, const float* const* w, const float* eps, float* rep, float* metrics, float* recon, int B, int obs_size,
                 int obs_channels, int cnn_feat_size, int latent_dim, int use_cnn_feat, float kld_weight, int full, float* ws, size_t ws_floats,
                 void* stream);
int ocrl_vae_bwd(const float* obs, const float* eps, const float* const* w, const float* dloss, const float* drep, float* const* dw, int B,
                 int obs_size, int obs_channels, int cnn_feat_size, int latent_dim, int use_cnn_feat, float kld_weight, int full, float* ws,
                 size_t ws_floats, void* stream);

/* ---- Masked autoencoder (MAE, a ViT encoder and a lighter ViT decoder): ocrs/mae/models_mae.py, mae_module.py, configs/ocr/mae.yaml.
 * obs [B, 3, S, S]; patch p, L = (S / p)^2 patches (<= 1024), P = 3 p p.  Encoder width D, `depth` blocks of `heads` heads; decoder
 * width Dd, `ddepth` blocks of `dheads` heads; MLP ratio 4, LayerNorm eps 1e-6, exact GELU, no dropout.  Head sizes 16 / 32 / 48 / 64;
 * D, Dd and P multiples of 4.  `w` = every parameter in state_dict order: cls_token [D], pos_embed [L + 1, D], mask_token [Dd],
 * decoder_pos_embed [L + 1, Dd], patch_embed.proj.{weight [D, 3, p, p], bias}, per block {norm1, attn.qkv, attn.proj, norm2, mlp.fc1,
 * mlp.fc2}.{weight, bias}, norm.*, decoder_embed.*, the decoder blocks, decoder_norm.*, decoder_pred.*: 14 + 12 (depth + ddepth) tensors.
 * The two position tables are inputs without a gradient (their dw entries are not written and may be NULL).
 * full = 0 (encode_full_patches, the rollout): all L patches; rep [B, L + 1, D] (the CLS row first) is the final norm's output.  noise,
 *   metrics, pred, mask, ids_restore and len_keep are not read; _bwd starts from drep and writes the encoder-side entries of dw
 *   (cls_token, patch_embed, blocks, norm).
 * full = 1 (the masked pre-training loss): noise [B, L] is ranked per image (ties by index), the len_keep patches of the lowest noise
 *   are embedded and encoded; rep [B, len_keep + 1, D] is the latent (may be NULL).  The decoder runs on L + 1 tokens.  metrics [2] =
 *   (loss, mse), both sum(mask mean_j (pred - target)^2) / sum(mask), as the reference reports them; pred [B, L, P] in patchify's
 *   (ph, pw, c) order, mask [B, L] (0 kept, 1 removed), ids_restore [B, L] (int) may each be NULL.  At len_keep == L no patch is removed,
 *   the divisor is zero and the loss is NaN, as in the reference; pred is still valid.
 * _bwd (same ws right after _fwd, same arguments): dloss (device scalar) the cotangent of the loss, drep that of rep; summed, a NULL one
 *   counts as zero (dloss NULL: the decoder is skipped and the decoder-side entries of dw are zeroed); full = 0 requires drep.
 * The observation gets no gradient.  Rejected shapes get ws_floats == 0 and fail in _fwd / _bwd. */
#define OCRL_MAE_MAX_DEPTH 32
size_t ocrl_mae_ws_floats(int B, int obs_size, int patch, int D, int depth, int heads, int Dd, int ddepth, int dheads, int len_keep, int full);
int ocrl_mae_fwd(const float* obs, const float* const* w, const float* noise, float* rep, float* metrics, float* pred, float* mask,
                 int* ids_restore, int B, int obs_size, int patch, int D, int depth, int heads, int Dd, int ddepth, int dheads, int len_keep,
                 int full, float* ws, size_t ws_floats, void* stream);
int ocrl_mae_bwd(const float* obs, const float* const* w, const float* dloss, const float* drep, float* const* dw, int B, int obs_size,
                 int patch, int D, int depth, int heads, int Dd, int ddepth, int dheads, int len_keep, int full, float* ws, size_t ws_floats,
                 void* stream);
/* mae_rank alone (tests): ids_restore [B, L], ids_keep [B, len_keep] (int), mask [B, L] of noise [B, L] */
int ocrl_mae_rank(const float* noise, int* ids_restore, int* ids_keep, float* mask, int B, int L, int len_keep, void* stream);

/* ---- Slot property probe: utils/property_predictor.py:12-189 (configs/train_property_predictor.yaml) ----
 * A head (nl Linear layers, LeakyReLU(slope) between them; `linear`: nl = 1, `mlp3`: nl = 4 with dims = {256, 256, 256, O}) reads the
 * detached encoder rows and predicts, per slot, O = sum of the property widths.  slot_rows != 0: rows [B K, D], dims[nl-1] == O
 * (SLATE, Slot-Attention, IODINE).  slot_rows == 0: rows [B, D], dims[nl-1] == K O, the outputs are read as K pseudo-slots (VAE).
 * Targets y [B, N, T], fp32; property p reads the target columns [tgt_range[2p], tgt_range[2p+1]) and the outputs
 * [out_range[2p], out_range[2p+1]) (ascending, not overlapping); kind[p] = 0: a class index, cost -log_softmax(softmax(out))[class] (the
 * reference takes the soft-max twice); kind[p] = 1: xy, two outputs, cost mean((out - y)^2); at most one xy property.
 * cost [B, N, K] (object, slot) sums the properties; col [B, N] is the exact minimum-cost assignment of the N objects to N distinct
 * slots, N <= K <= OCRL_PROBE_MAX_SLOTS (dynamic programme over slot bit-masks; ties: the lowest slot index, so two runs agree bit for
 * bit); above the limit the calls return non-zero and launch nothing.
 * metrics [P + 2]: [0] loss = sum over images and objects of cost[o, col[o]] (a sum, not a mean); [1 + p] acc of a class property
 * (argmax of the raw outputs) or the reference's R^2_xy (||out - mean(y)||^2 / ||y - mean(y)||^2, mean over images and coordinates);
 * [P + 1] mse_xy = mean Euclidean distance of the matched xy outputs (the reference's definition, despite the name).
 * A class index outside its property's range gives a NaN loss (the reference raises).
 * `w` / `dw`: the head's parameters in state_dict order (0.weight, 0.bias, 2.weight, ...); dw is overwritten, the rows get no gradient.
 * _fwd leaves in ws what _bwd needs; _bwd (same ws, same shapes) scales by the device scalar dloss (null = 1).
 * out [B, K, O], cost and col of _fwd may be null.  _match takes head outputs directly: out[b, s, :] at b * ld_img + s * ld_row, dout
 * alike (only its [K, O] entries are written; null = no gradient), ws of _match_ws_floats(B, P).  Rejected shapes get ws_floats == 0. */
#define OCRL_PROBE_MAX_SLOTS 12
#define OCRL_PROBE_MAX_PROPS 8
#define OCRL_PROBE_MAX_LAYERS 8
size_t ocrl_probe_ws_floats(int B, int K, int N, int D, int O, int slot_rows, int nl, const int* dims, int P);
int ocrl_probe_fwd(const float* rows, const float* const* w, const float* y, float* out, float* cost, int* col, float* metrics, int B, int K, int N,
                   int D, int T, int O, int slot_rows, int nl, const int* dims, float slope, int P, const int* tgt_range, const int* out_range,
                   const int* kind, float* ws, size_t ws_floats, void* stream);
int ocrl_probe_bwd(const float* rows, const float* dloss, const float* const* w, float* const* dw, int B, int K, int N, int D, int O, int slot_rows,
                   int nl, const int* dims, float slope, int P, float* ws, size_t ws_floats, void* stream);
size_t ocrl_probe_match_ws_floats(int B, int P);
int ocrl_probe_match(const float* out, int ld_row, long long ld_img, const float* y, const float* dloss, float* cost, int* col, float* metrics,
                     float* dout, int B, int K, int N, int T, int O, int P, const int* tgt_range, const int* out_range, const int* kind, float* ws,
                     size_t ws_floats, void* stream);

/* ---- Segmentation ARI counts: utils/tools.py:309-320 (calculate_ari) with the masking of slate_module.py:211-213 /
 * iodine_module.py:263-265 folded in ----
 * Two stacks of per-pixel channel scores, each addressed by ELEMENT strides (batch, channel, pixel), so [B, C, N] and [B, N, C] are both
 * read in place; no alignment is required (pixel-contiguous, 16-byte aligned stacks take 16-byte loads).  Per image:
 *   true label  t = first maximum over the Ct channels of `truth`, predicted label p = first maximum over Cp channels (torch.argmax:
 *               a NaN is the maximum, the first NaN wins)
 *   fuse_fg = 0: `pred` holds the Cp channels.  fuse_fg = 1: `pred` holds K = Cp - 1 channels; with fg = 1 - truth[Ct-1] (one fp32
 *               subtract) channel k < K scores pred_k * fg (one fp32 multiply) and channel K scores fg, which is
 *               torch.cat([attns * fg_mask, fg_mask], dim=1) bit for bit, ties included
 *   table [B, Ct, Cp] int32   pixels per (t, p); zeroed by the call
 *   sums  [B, 3]      int64   sum_ij C(n_ij), sum_i C(a_i) (row sums), sum_j C(b_j) (column sums), C(x) = x (x - 1) / 2
 * Exact integers: the result does not depend on the order of the additions.  1 <= Ct, Cp <= OCRL_ARI_MAX_CHANNELS, B >= 1,
 * 1 <= N < 2^31; anything else is rejected ("invalid ...") before any memory is touched.  The zeroing and both kernels go on `stream`. */
#define OCRL_ARI_MAX_CHANNELS 32
int ocrl_ari_counts(const float* truth, long long t_sb, long long t_sc, long long t_sn, int Ct, const float* pred, long long p_sb,
                    long long p_sc, long long p_sn, int Cp, int fuse_fg, int B, long long N, int* table, long long* sums, void* stream);

/* ---- actor-critic head, PPO minibatch step and A2C step: sb3s/custom_acnets.py:8-96 (CustomNetwork: shared_net, then policy_net and value_net,
 *      each [Linear, ReLU | Tanh] x n, the configs/sb3_acnet files) with the heads its ActorCriticPolicy (custom_acnets.py:99-128) inherits
 *      from stable-baselines3: action_net = Linear(latent_dim_pi, A), value_net = Linear(latent_dim_vf, 1), a categorical distribution,
 *      and the losses of PPO.train (configs/sb3/ppo.yaml; clip_range_vf = None) and A2C.train (configs/sb3/a2c.yaml).  The heads and the losses are restated from the published
 *      algorithm, not from an import.
 * Stateless; fp32 device pointers; everything is enqueued on `stream` with no host synchronisation.
 * desc: B rows of F features, A actions (A == 0: the trunks alone, no heads), trunk t = 0 shared, 1 policy, 2 value with n[t] layers of
 *   widths dims[t][] and activations acts[t][] (0 none, 1 ReLU, 2 tanh).  Supported: B >= 1, F >= 1, B * max(F, widths) < 2^31, widths
 *   multiples of 4 up to 256, at most OCRL_ACNET_MAX_LAYERS layers per trunk (any trunk may be empty), 1 <= A <= 64 (or 0).  Anything
 *   else is rejected: ws_floats == 0, the other entry points return non-zero with a message.
 * w / dw: state_dict order: shared_net, policy_net, value_net as (weight [out, in], bias) per layer, then with A > 0 action_net.weight
 *   [A, latent_pi], action_net.bias, value_net.weight [1, latent_vf], value_net.bias.
 * _fwd: latent_pi [B, latent_dim_pi], latent_vf [B, latent_dim_vf], logits [B, A], values [B]; each may be NULL.  One kernel launch.
 *   save != 0 leaves every trunk layer's output in ws for _bwd (ws may be NULL otherwise).
 * _bwd: after a _fwd with save != 0 on the same features and ws.  Any of dlatent_pi, dlatent_vf, dlogits, dvalues may be NULL (zero).
 *   Overwrites every entry of dw and, unless NULL (detached features), dfeatures [B, F].
 * _ppo_fwd_bwd: the whole minibatch step.  actions: int64 [B] in [0, A) (clamped into the range); scalars [6] = loss, policy_loss,
 *   value_loss, entropy_loss, approx_kl, clip_fraction; dw, dfeatures = gradients of `loss`.  With normalize_advantage the advantages
 *   become (adv - mean) / (std + 1e-8), unbiased std; B == 1 is then rejected.  At most three launches.
 * _a2c_fwd_bwd: the whole-batch A2C step with the same descriptor, w / dw order, workspace and reduction.  Per row, with lse, q_a =
 *   exp(z_a - lse) and H = -sum_a q_a (z_a - lse) computed as in _ppo_fwd_bwd: policy_loss = -mean(adv * log_prob), value_loss =
 *   mean((values - returns)^2), entropy_loss = -mean(H), loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss;
 *   scalars [4] = loss, policy_loss, value_loss, entropy_loss; dw, dfeatures (may be NULL) = gradients of `loss`.  actions are clamped
 *   into [0, A); normalize_advantage as above (B == 1 is then rejected); A == 0 is rejected.  At most three launches (the advantage
 *   statistics run only with normalize_advantage).
 * _act: the rollout's step: _fwd (save = 0, no workspace) with the action and its log-probability in the same single launch.  Needs the
 *   heads (A >= 1; A == 0 is rejected).  actions int64 [B], values [B], log_prob [B]; logits [B, A] may be NULL.  The sampling rule:
 *     u in [0, 1) is a 24-bit uniform (k / 2^24): uniforms[r] when `uniforms` is given, else a pure function of (seed, row_offset + r)
 *       from the library's counter RNG, so a row's result depends neither on B nor on its position in the batch;
 *     lse = max + log(sum_j exp(logits_j - max)), p_j = exp(logits_j - lse), c_a = p_0 + ... + p_a, all fp32, summed in index order;
 *     action = the number of a in [0, A - 2] with c_a <= u: the last action absorbs the rounding of the sum, the result is in [0, A);
 *     deterministic != 0: action = the lowest index of the maximum logit (torch.argmax), no draw;
 *     log_prob = logits[action] - lse either way.
 *   _act_uniforms writes out[i] = the uniform of row row_offset + i of the stream `seed`, i < n: exactly what _act draws.
 * Bit-reproducible: no atomics; per-tile partial gradients are summed in a fixed order; a row's outputs do not depend on its position. */
#define OCRL_ACNET_MAX_LAYERS 8
typedef struct {
    int B, F, A;
    int n[3];
    int dims[3][OCRL_ACNET_MAX_LAYERS];
    int acts[3][OCRL_ACNET_MAX_LAYERS];
} ocrl_acnet_desc;
size_t ocrl_acnet_desc_size(void);
size_t ocrl_acnet_ws_floats(const ocrl_acnet_desc* d);
int ocrl_acnet_fwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, float* latent_pi, float* latent_vf, float* logits,
                   float* values, int save, float* ws, size_t ws_floats, void* stream);
int ocrl_acnet_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const float* dlatent_pi, const float* dlatent_vf,
                   const float* dlogits, const float* dvalues, float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream);
int ocrl_acnet_ppo_fwd_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const long long* actions,
                           const float* old_log_prob, const float* advantages, const float* returns, float clip_range, float vf_coef,
                           float ent_coef, int normalize_advantage, float* scalars, float* dfeatures, float* const* dw, float* ws,
                           size_t ws_floats, void* stream);
int ocrl_acnet_a2c_fwd_bwd(const ocrl_acnet_desc* d, const float* features, const float* const* w, const long long* actions,
                           const float* advantages, const float* returns, float vf_coef, float ent_coef, int normalize_advantage,
                           float* scalars, float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream);
int ocrl_acnet_act(const ocrl_acnet_desc* d, const float* features, const float* const* w, unsigned long long seed,
                   unsigned long long row_offset, const float* uniforms /* NULL = draw */, int deterministic, long long* actions, float* values,
                   float* log_prob, float* logits /* may be NULL */, void* stream);
int ocrl_acnet_act_uniforms(unsigned long long seed, unsigned long long row_offset, long long n, float* out, void* stream);
/* Generalised advantage estimation as stable-baselines3's RolloutBuffer.compute_returns_and_advantage: rewards, values, episode_starts
 * [T, E], last_values, dones [E] -> advantages, returns [T, E]; one thread per environment walks T backwards. */
int ocrl_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values, const float* dones,
             float* advantages, float* returns, int T, int E, float gamma, float gae_lambda, void* stream);

/* ---- sprite environments: the Target and Odd-One-Out tasks (envs/synthetic_envs/base.py:81-151, 291-360, target.py:16-57 and
 *      oddoneout.py:19-126, restated) as a vectorised environment whose state, transition, reward, auto-reset and frames stay on the device.  Stateless: the caller owns `state`
 *      (ocrl_sprite_env_state_floats floats, 256-byte aligned, zero before the first reset) and every output; everything is enqueued on
 *      `stream` with no host synchronisation, no atomics and no unbounded loop; reset and step run one thread per environment.
 * desc: E environments, H x H frames (H a multiple of 4 in [8, 512]); num_objects_range [lo, hi], 1 <= lo <= hi <= 15 (easy mode: within
 *   [2, 4]; normal mode: [4, 4], the modes' boxes); colour ids 0..6 = blue, green, yellow, red, cyan, pink, brown; shape ids = the names' indices
 *   in the reference's SHAPES list, of which six are drawn: 0 square, 1 triangle, 2 star_4, 3 circle, 7 star_5, 9 spoke_4 (ids 4, 5, 6, 8, 10, 11,
 *   the list's other names, and anything outside the list are rejected with "shape id <N>"); scales in (0, 1).  Anything else
 *   is rejected: state_floats == 0, the other entry points return non-zero, with a message.
 * state: rows [E, hi + 1, 5] fp32 = (colour id, shape id, scale, x, y): objects 0..n-1, the agent in row n, zero rows after it; then,
 *   at the next multiple of 64 floats, 8 int32 words per environment: n, target index, step_count, episode index, episode length, the
 *   unique property kind of an Odd-One-Out episode (0 colour, 1 shape, 2 scale; 0 for Target), and the episode's return so far as one
 *   double.
 * The draws.  u(seed, e, k, j) = the top 24 bits of the library's counter RNG at site 500 and counter (e << 44) | ((k mod 2^24) << 20) | j:
 *   draw j of episode k of environment e is a function of (seed, e, k, j) alone, whatever E is and whenever the episode began.  An integer
 *   in [0, m) is (bits24 * m) >> 24; a position in [a, b] is a + (b - a) * (bits24 / 2^24), each operation rounded to fp32 (no FMA).
 *   An episode draws, with j counting up from 0: n in [lo, hi]; the target index in [0, n); for every other object in index order its
 *   (colour, shape, scale) as indices into the desc's lists, redrawn while the triple equals the target's (after 64 tries the last one
 *   stands); then positions for i = 0..n-1, x then y: uniform in [lo_i + r + dist_wall, hi_i - r - dist_wall] of the object's box (easy
 *   mode: [lo_i, hi_i]; an interval with lo_i == hi_i yields lo_i without a draw), r = scale / 2, rejected while the centre is closer than
 *   a threshold to an object placed before it (r + r_j + dist_objs) or to the agent (r + r_agent + dist_agent), 0.15 for both with
 *   `occlusion`.  An object takes at most 256 candidates; then the whole placement starts over on the draws that follow, at most 8
 *   times, and on the last attempt the 256th candidate stands.  The agent starts at agent_x, agent_y (hard mode) or (0.5, 0.5).
 * The Odd-One-Out episode (task 1; target_* is ignored).  One object, `target`, carries a value u of one property kind T that no other
 *   object has; every other value of every kind is shared by at least two objects.  below(m) is the integer draw in [0, m) above and takes
 *   exactly one draw, also when m = 1; list_K / n_K are the desc's COLORS, SHAPES, SCALES in the order colour, shape, scale.  The draws:
 *   1. n = lo + below(hi - lo + 1).
 *   2. target = below(n); in an unseen mode target = 0 and no draw is taken.
 *   3. kinds = the K with n_K > 1, in order; T = kinds[below(len(kinds))].
 *   4. u = list_T[below(n_T)]; in unseen test mode u = unseen_colors[below(2)].  Object `target` gets u in kind T.
 *   5. with obj_comp: for each K != T in order, v_K = list_K[below(n_K)] is given to all n objects.
 *   6. for K = colour, shape, scale: fill the objects without a value of kind K: for K = T all but `target`; for K != T all n, or none
 *      under obj_comp (no draw then).  The admissible list A is list_K in desc order; for K = T without u, in unseen train mode with u
 *      one of the two unseen colours also without the other one, and in unseen test mode exactly the other one.  While z objects are
 *      unfilled, z > 0: v = A[below(len(A))], g = 2 + below(z - 1), then g times v goes to the below(z')-th still unfilled object in
 *      index order (z' the count at that moment); if exactly one object is then left, it takes v too, without a draw.
 *   7. positions exactly as in the Target episode.
 *   These are the reference's distributions with its rejection loops written as draws from the admissible set, so every loop is bounded
 *   (at most 6 + 6 n draws before the positions).  Rejected for task 1: lo < 3, no list with more than one entry, equal entries within a
 *   list; for an unseen mode also n_shapes != 1, n_scales != 1, n_colors < 3, and unseen colours that are equal or not both in COLORS
 *   (the reference's unseen modes do not terminate when the unique kind is not the colour).  Task 0 takes no obj_comp or unseen_mode.
 * _reset: every environment, or those with mask[e] != 0.  episode >= 0 starts that episode index, -1 the one after the state's own.
 * _step: actions int64 [E]: 0 y += step_size, 1 x -= step_size, 2 y -= step_size, 3 x += step_size, anything else no move; x, y clipped
 *   to [r_agent, 1 - r_agent]; step_count + 1 >= max_steps ends the episode; rew_type 2 (dense) pays +-0.01 by whether the distance to the
 *   target shrank; the first object in index order whose centre is closer than agent_scale ends it: reward 1 and success for the target,
 *   else 0.1 under rew_type 1 (normal) and 0 otherwise.  rewards fp32, dones and success bytes, ep_return (double; the rewards summed in
 *   double in step order) and ep_length of the episode that ended with this step (0 elsewhere), all [E].  A finished environment starts
 *   its next episode in the same launch.
 * _render: rows [E, R, 5] of any origin, R <= 16, painted in row order (a later row overwrites; a row is painted when its colour id is in
 *   0..6, its shape id, truncated to an integer, is one of the six drawn ones and its scale > 0: colour -1, any other shape id and an empty
 *   row are not drawn) on black with the shape predicates of the pre-training scenes and, for ids 7 and 9, star_5 (a ten-vertex star, tips
 *   at 1.25 r, 72 degrees apart from straight up, notches at 0.63 r halfway between them; r = scale / 2, up = -y) and spoke_4 (an upright
 *   Greek cross, bars of half width 0.4 r and half length 1.25 r), pixel centre (i + 0.5) / H, the row index growing with y.
 *   mode 0: uint8 [E, 3, H, W]; 1: [E, H, W, 3]; 2: masks [E, R + 1, H, W, 1] of 0 / 1: each row alone and unoccluded, the background
 *   (no row covers the pixel) last.
 * _state_obs: the observation of render_mode "state" (base.py:365-394) of rows [E, R, 5], R <= 16 -> out fp32 [E, R, 5]: columns 0, 1, 3, 4
 *   copied; column 2 the index of the scale in the reference's global list [0.15, 0.22]: 0 for (float)0.15 and for an all-zero row (the
 *   padding), 1 for (float)0.22, -1 for any other scale; a row whose colour is -1 becomes (-1, -1, -1, 0, 0).  One thread per row.
 * _uniforms: out [n_envs, n] = bits24 / 2^24 of draws first .. first + n - 1 of episode `episode` of environments env0 .. */
#define OCRL_SPRITE_MAX_OBJECTS 15
typedef struct {
    int E, H;
    int lo, hi;
    int mode;                                   /* 0 easy, 1 normal, 2 hard */
    int rew_type;                               /* 0 sparse, 1 normal, 2 dense */
    int occlusion, max_steps;
    int n_colors, n_shapes, n_scales;
    int colors[8], shapes[8];
    float scales[8];
    int target_color, target_shape;
    float target_scale;
    int agent_color, agent_shape;
    float agent_scale, agent_x, agent_y;
    float step_size, dist_agent, dist_objs, dist_wall;
    int task;                                   /* 0 Target, 1 Odd-One-Out; a zeroed tail from here on is the Target task */
    int obj_comp;                               /* Odd-One-Out: the kinds other than the unique one are constant over the objects */
    int unseen_mode;                            /* 0 none, 1 train (never the unseen pair), 2 test (always the unseen pair) */
    int unseen_colors[2];                       /* colour ids of the unseen combination */
} ocrl_sprite_env_desc;
size_t ocrl_sprite_env_desc_size(void);
size_t ocrl_sprite_env_state_floats(const ocrl_sprite_env_desc* d);
int ocrl_sprite_env_reset(const ocrl_sprite_env_desc* d, float* state, unsigned long long seed, const unsigned char* mask /* [E] or NULL */,
                          long long episode, void* stream);
int ocrl_sprite_env_step(const ocrl_sprite_env_desc* d, float* state, unsigned long long seed, const long long* actions, float* rewards,
                         unsigned char* dones, unsigned char* success, double* ep_return, int* ep_length, void* stream);
int ocrl_sprite_render(const float* rows, int E, int R, int H, int mode, unsigned char* out, void* stream);
int ocrl_sprite_state_obs(const float* rows, int E, int R, float* out, void* stream);
int ocrl_sprite_env_uniforms(unsigned long long seed, long long env0, int n_envs, long long episode, int first, int n, float* out, void* stream);

/* ---- pre-training scenes: the RandomObjs episode of the pre-training dataset (ocrl_amd/utils/data.py:random_sprite_scenes: K sprites on
 *      black, occlusion allowed, no agent) made on the device, batch by batch.  Scene i of a seed is a function of (seed, i) alone: the
 *      same whichever batch it is in, at whichever position, and whichever outputs are asked for.  Stateless: the caller owns every
 *      buffer (obs and masks 16-byte aligned, obs_u8 4-byte aligned); everything is enqueued on `stream` with no host synchronisation, no
 *      atomics and no unbounded loop.  One launch per call.
 * desc: H x H frames, H a multiple of 4 in [8, 512]; K objects, 1 <= K <= 15.  indices: device int64 [B], B >= 1, the scene indices
 *   of the batch; an index outside [0, 2^40) is masked to its low 40 bits inside the kernel.  Rejected, non-zero with a message: a null
 *   descriptor, H or K outside their ranges, B < 1, null indices, all four outputs null, misaligned outputs, a batch beyond the grid limit.
 * The draws.  u(seed, i, j) = the top 24 bits of the library's counter RNG at site 510 and counter (i << 16) | j.  below(m) =
 *   (bits24 * m) >> 24 and u01() = bits24 / 2^24 as in the sprite environments.  Scene i takes j = 0, 1, .. in order; for k = 0 .. K-1:
 *   1. s = below(2); r = SCALES[s] * 0.5f, SCALES = {0.15f, 0.22f}.
 *   2. a = r + 0.08f; b = (1.0f - r) - 0.08f.  At most 64 candidates, each x = a + (b - a) * u01(), then y likewise, every operation
 *      rounded to fp32 (no FMA); a candidate is rejected when its distance (sqrtf(dx * dx + dy * dy)) to (0.5, 0.5) or to an earlier
 *      object's centre is < 0.15f.  The 64th candidate stands whatever it is.
 *   3. shape = below(4): square, triangle, star_4, circle.
 *   4. colour = below(4): blue, green, yellow, red.
 *   This is the distribution and the draw order of random_sprite_scenes, not numpy's bit stream.
 * The pixels are those of ocrl_sprite_render: pixel centre (i + 0.5) / H, its shape predicates with r = scale / 2, object k + 1 painted
 *   over object k, on black.
 * Outputs, each may be NULL: obs_u8 [B, H, W, 3] the bytes; obs [B, 3, H, W] what ocrl_obs_u8_to_f32 gives for them (0.0f or 1.0f:
 *   only the bytes 0 and 255 occur); masks [B, K + 1, H, W]: plane k is 1.0f where object k is the last one covering the pixel, plane K
 *   where none does, 0.0f elsewhere; objs [B, K, 5] = (colour index, shape index, scale index, x, y).
 * _uniforms: out [n] = bits24 / 2^24 of draws first .. first + n - 1 (all below 2^16) of scene `index` (masked as above). */
typedef struct {
    int H;
    int K;
} ocrl_scenes_desc;
int ocrl_scenes_batch(const ocrl_scenes_desc* d, unsigned long long seed, const long long* indices /* device int64 [B] */, int B,
                      float* obs /* [B,3,H,W] or NULL */, unsigned char* obs_u8 /* [B,H,W,3] or NULL */, float* masks /* [B,K+1,H,W] or NULL */,
                      float* objs /* [B,K,5] or NULL */, void* stream);
int ocrl_scenes_uniforms(unsigned long long seed, long long index, int first, int n, float* out /* [n] */, void* stream);

/* ---- task scenes: the first frames of the sprite tasks' episodes as a pre-training dataset (the reference collects its target-* and
 *      odd-one-out-* datasets from the environments with only_initial: True), made on the device, batch by batch.  Scene i of a seed is a
 *      function of (desc, seed, i) alone, and it is the environment's own episode: the kernel runs the episode function of
 *      ocrl_sprite_env_reset.  Stateless: the caller owns every buffer (obs and masks 16-byte aligned, obs_u8 4-byte aligned); everything
 *      is enqueued on `stream` with no host synchronisation, no atomics and no unbounded loop.  One launch per call.
 * desc: a sprite environment's descriptor, validated exactly as by ocrl_sprite_env_reset (tasks 0 and 1); E and max_steps are not used
 *   but must be valid; frames are H x H.  indices: device int64 [B], B >= 1.  An index is masked to its low 44 bits inside the kernel:
 *   scene i is episode k = i & 0xFFFFFF of environment e = i >> 24 of the site-500 stream ("The draws" above), so scene (e << 24) | k
 *   under a seed is what an environment of that seed shows when its environment e starts its episode k, and a plain dataset index
 *   i < 2^24 is episode i of environment 0.
 * Outputs, each may be NULL.  With R = hi + 1 rows (objects 0..n-1, the agent in row n, zero rows after it):
 *   obs_u8 [B, H, W, 3]: the pixels of ocrl_sprite_render mode 1 of the rows: painter's order over rows 0..hi, the agent included, on black;
 *   obs [B, 3, H, W] fp32: byte / 255.0f, what ocrl_obs_u8_to_f32 gives for those bytes;
 *   masks [B, R + 1, H, W] fp32 of 0 / 1: ocrl_sprite_render mode 2 (the reference's render(mode="mask") with its zero padding): plane j is
 *     row j alone and unoccluded, the planes of empty rows are zero, the last plane is 1 where no row covers the pixel.  (Not the
 *     "last object covering" planes of ocrl_scenes_batch: where sprites overlap, the planes here overlap too.)
 *   objs [B, R, 5] fp32: what ocrl_sprite_state_obs gives for the rows, the scale as its index in [0.15, 0.22];
 *   labels [B] int64: the target's row index.
 * Rejected, non-zero with a message: a null or invalid descriptor, B < 1, null indices, all five outputs null, misaligned outputs, a
 *   batch beyond the grid limit. */
int ocrl_task_scenes_batch(const ocrl_sprite_env_desc* d, unsigned long long seed, const long long* indices /* device int64 [B] */, int B,
                           float* obs /* [B,3,H,W] or NULL */, unsigned char* obs_u8 /* [B,H,W,3] or NULL */, float* masks /* [B,hi+2,H,W] or NULL */,
                           float* objs /* [B,hi+1,5] or NULL */, long long* labels /* [B] or NULL */, void* stream);

/* ---- the per-object MLP of the ground-truth-state encoder (ocrs/gt/gt_module.py:14-27): x [M, D] through nl layers
 *      h_l = act_l(h_{l-1} W_l^T + b_l), W_l [dims[l], dims[l-1]] (torch layout), acts[l] != 0: ReLU, 0: none.  M = batch x objects rows
 *      (1 <= M < 2^22), 1 <= D <= 64, 1 <= nl <= 4, every dims[l] a multiple of 4 in 4 .. 256; anything else: ws_floats == 0 and the
 *      other entries return non-zero, with a message.  w = {W_0, b_0, W_1, b_1, ..}, dw likewise.  Stateless: the caller owns parameters,
 *      gradients and `ws` (ocrl_gt_mlp_ws_floats floats, 256-byte aligned); _fwd leaves every layer's output there and _bwd reads them
 *      (the ReLU mask is output > 0), so `ws` lives from the one to the other.
 * _fwd: one launch; a workgroup takes 16 rows, the activations stay in LDS from layer to layer.  out [M, dims[nl-1]].
 * _bwd: dout [M, dims[nl-1]] -> dw (written, not accumulated) and, when dx is not NULL, dx [M, D].  One launch down the chain: the
 *   16-row tiles are split into at most 64 slabs, a workgroup adds its slab's tiles in order into the slab's partial; a second launch
 *   sums the partials in slab order (none when M <= 16 rows make one slab).  No atomics: the result depends on the inputs and M alone
 *   and is the same bit for bit from run to run. */
#define OCRL_GT_MLP_MAX_LAYERS 4
size_t ocrl_gt_mlp_ws_floats(int M, int D, int nl, const int* dims);
int ocrl_gt_mlp_fwd(const float* x, const float* const* w, float* out, int M, int D, int nl, const int* dims, const int* acts, float* ws,
                    size_t ws_floats, void* stream);
int ocrl_gt_mlp_bwd(const float* x, const float* dout, const float* const* w, float* dx /* may be NULL */, float* const* dw, int M, int D, int nl,
                    const int* dims, const int* acts, float* ws, size_t ws_floats, void* stream);

/* ---- L2 gradient clip + Adam on caller-owned flat fp32 buffers p, g, m, v [n] (16-byte aligned), as PPO.train applies
 *      torch.nn.utils.clip_grad_norm_ and torch.optim.Adam to the policy.  Stateless, no host synchronisation, no atomics:
 *      norm = ||g||_2 over the whole buffer (per-block sums of squares folded in a fixed order; written to norm_out, 1 device float),
 *      coef = min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: no clipping; norm_out is still written), then the bias-corrected Adam
 *      update of p, m, v with g * coef; `step` counts from 1.  n >= 1, any tail; ws: ocrl_flat_clip_adam_ws_floats() floats.
 *      Four small launches (three of the norm, one update), five when n is not a multiple of 4. */
size_t ocrl_flat_clip_adam_ws_floats(void);
int ocrl_flat_clip_adam_l2(float* p, const float* g, float* m, float* v, long long n, float max_norm, float lr, float beta1, float beta2,
                           float eps, int step, float* norm_out /* device, 1 float */, float* ws, size_t ws_floats, void* stream);

/* ---- L2 gradient clip + TF-style RMSprop on caller-owned flat fp32 buffers p, g, sq [n] (16-byte aligned), as A2C.train applies
 *      torch.nn.utils.clip_grad_norm_ and stable-baselines3's RMSpropTFLike (momentum 0, not centred, no weight decay) to the policy.
 *      norm and coef exactly as in ocrl_flat_clip_adam_l2 (a NaN norm reaches every weight); with g' = coef * g:
 *        sq <- alpha * sq + (1 - alpha) * g'^2,   p <- p - lr * g' / sqrt(sq + eps)
 *      Two things set this apart from torch.optim.RMSprop: the epsilon is INSIDE the square root, and the caller initialises sq to
 *      ONES, not zeros.  1 - alpha is taken in double from the decimal `alpha` stands for and rounded once.  Rejected before any launch:
 *      null arguments, n < 1, misaligned p / g / sq, ws_floats < ocrl_flat_clip_rmsprop_ws_floats(), alpha outside (0, 1), eps <= 0.
 *      Four small launches (three of the norm, one update), five when n is not a multiple of 4. */
size_t ocrl_flat_clip_rmsprop_ws_floats(void);
int ocrl_flat_clip_rmsprop_l2(float* p, const float* g, float* sq, long long n, float max_norm, float lr, float alpha, float eps,
                              float* norm_out /* device, 1 float */, float* ws, size_t ws_floats, void* stream);

/* ---- The same two steps over several flat buffers at once, as stable-baselines3 clips and steps a policy whose encoder keeps its
 *      parameters in a buffer of its own: the semantics are those of ocrl_flat_clip_adam_l2 / ocrl_flat_clip_rmsprop_l2 applied to the
 *      concatenation of the segments.  norm = ||g||_2 over every segment's g together (written to norm_out), one coef for all, then the
 *      same update of every segment; a NaN norm reaches every weight of every segment; g is never written.  No atomics, no host
 *      synchronisation: block partial sums of squares are folded in a fixed order (segment order, then block order), so the result is a
 *      function of the inputs and the segment lengths alone, the same bit for bit from run to run.  `seg` is HOST memory, read during the
 *      call and handed to the kernels by value: no upload, copy or allocation.  Three launches whatever nseg is (partial sums, their
 *      fold, the update); a segment's last n % 4 elements are taken inside them.  p, g, s0, s1 16-byte aligned; n >= 1, any tail.
 *      A segment whose g is all zero and whose m = v = 0 comes back with p, m, v unchanged bit for bit (Adam).
 *      Rejected before any launch: nseg outside [1, OCRL_FLAT_MAX_SEGMENTS]; a null seg, p, g, s0 (s1 for Adam), norm_out or ws;
 *      n < 1; a misaligned pointer; ws_floats < ocrl_flat_clip_multi_ws_floats(); step < 1; alpha outside (0, 1) or eps <= 0 (RMSprop). */
#define OCRL_FLAT_MAX_SEGMENTS 8
typedef struct { float* p; const float* g; float* s0; float* s1; long long n; } ocrl_flat_segment;   /* s0, s1: m, v (Adam); sq, unused (RMSprop) */
size_t ocrl_flat_clip_multi_ws_floats(void);
int ocrl_flat_clip_adam_l2_multi(const ocrl_flat_segment* seg, int nseg, float max_norm, float lr, float beta1, float beta2, float eps,
                                 int step, float* norm_out /* device, 1 float */, float* ws, size_t ws_floats, void* stream);
int ocrl_flat_clip_rmsprop_l2_multi(const ocrl_flat_segment* seg, int nseg, float max_norm, float lr, float alpha, float eps,
                                    float* norm_out /* device, 1 float */, float* ws, size_t ws_floats, void* stream);

/* ---- IODINE (ocrs/iodine/iodine_module.py:14-271, ocrs/iodine/iodine.py:4-14, ocrs/base.py:60-74): SURVEY.md §8 row a20 ----
 * Same conventions as the SLATE handle: flat fp32 parameter / gradient / Adam buffers in the reference's
 * _module.parameters() order and state_dict names, adopted from the caller; one workspace; all work on the caller's stream. */
typedef struct ocrl_iodine ocrl_iodine;
typedef struct ocrl_iodine_config {
    int obs_size, obs_channels;                 /* env_config.obs_size / obs_channels (3) */
    int slot_size, num_iterations, num_slots;   /* ocr_config.slot_size / num_iterations / num_slots */
    float sigma, beta;                          /* ocr_config.sigma / beta */
    int layer_norm;                             /* ocr_config.layer_norm */
    int ref_mlp_hidden;                         /* ocr_config.ref_mlp_hidden_size; conv widths 64, 4 layers, 3x3 (stride 2 / 1) are fixed */
    int max_batch;
} ocrl_iodine_config;
int ocrl_iodine_create(const ocrl_iodine_config* cfg, ocrl_iodine** out);
void ocrl_iodine_destroy(ocrl_iodine* h);
int ocrl_iodine_param_count(const ocrl_iodine* h);
int ocrl_iodine_param_info(const ocrl_iodine* h, int i, char* name, int name_cap, int shape[4], int* ndim, long long* offset, long long* numel);
long long ocrl_iodine_flat_size(const ocrl_iodine* h);
size_t ocrl_iodine_workspace_bytes(const ocrl_iodine* h);
int ocrl_iodine_bind(ocrl_iodine* h, float* params, float* grads, float* adam_m, float* adam_v, void* workspace, size_t workspace_bytes);
/* Iodine_Module._forward (iodine_module.py:79-252): obs [B,3,S,S] NCHW; noise: optional injected N(0,1) draws of the
 * per-iteration rsample, [I,B,K,L] (NULL = device RNG stream `seed`).  Results: ocrl_iodine_metrics / ocrl_iodine_tensor
 * ("slots" [B,K,L], "masks" [B,K,S,S], "recon" [B,3,S,S], "recons_masked" [B,K,3,S,S], "out4" [B*K,S,S,4]). */
int ocrl_iodine_forward(ocrl_iodine* h, const float* obs, int B, unsigned long long seed, const float* noise, void* stream);
/* loss.backward() of the last forward (loss = -sum_i (i+1)/I ELBO_i) into the flat gradient buffer */
int ocrl_iodine_backward(ocrl_iodine* h, void* stream);
/* clip_grad_norm_(params, clip, 2.0) + Adam(lr) (base.py:60-74); gscale = 1/world for a data-parallel mean */
int ocrl_iodine_clip_adam(ocrl_iodine* h, float lr, float clip, int step, float gscale, void* stream);
int ocrl_iodine_grad_norm(ocrl_iodine* h, void* stream);
/* device float[8]: [0] loss, [1] mse (last iteration), [2] kld (last iteration), [3] gradient L2 norm */
float* ocrl_iodine_metrics(const ocrl_iodine* h);
int ocrl_iodine_tensor(const ocrl_iodine* h, const char* name, float** ptr, long long* count);

/* ---- data-parallel exchange: one in-place SUM all-reduce of a flat fp32 gradient buffer per step over RCCL
 * (xGMI); pass gscale = 1/world to ocrl_*_clip_adam for the mean.  For hosts without torch.distributed; librccl is opened
 * lazily (dlopen).  unique id: 128 bytes produced on rank 0 and broadcast by the host's own means (as ncclGetUniqueId). */
typedef struct ocrl_comm ocrl_comm;
int ocrl_comm_unique_id(void* out128, size_t cap);
int ocrl_comm_init(ocrl_comm** out, int rank, int world, const void* unique_id128);   /* current HIP device = this rank's GPU */
int ocrl_comm_allreduce(ocrl_comm* c, float* device_buf, long long n, void* stream);
int ocrl_comm_world(const ocrl_comm* c);
void ocrl_comm_destroy(ocrl_comm* c);

#ifdef __cplusplus
}
#endif
#endif
