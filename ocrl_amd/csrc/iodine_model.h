// IODINE training-step orchestration over the HIP kernels (host code): reference ocrs/iodine/iodine_module.py:79-252 and
// ocrs/base.py:60-74.  One object per process per GPU; not thread-safe; every launch goes to the caller's stream.
#pragma once
#include <string>
#include <vector>

#include "kernels.h"
#include "model_base.h"

struct IodineConfig {
    int obs_size = 64, obs_channels = 3, slot_size = 64, num_iters = 5, num_slots = 7;
    float sigma = 0.35f, beta = 1.f;
    int layer_norm = 1;
    int ref_mlp_hidden = 256;     // refinement MLP / LSTM width; the convolution widths are fixed at 64 (reference configs)
    int max_batch = 1;
};

class IodineModel : public ModelBase {
public:
    explicit IodineModel(const IodineConfig& c);
    int bind(float* p, float* g, float* m, float* v, void* ws, size_t ws_bytes);
    // obs [B,3,S,S] NCHW; noise: optional injected N(0,1) draws [I,B,K,L] (else the device RNG stream `seed`)
    int forward(const float* obs, int B, unsigned long long seed, const float* noise, hipStream_t st);
    int backward(hipStream_t st);
    int grad_norm(hipStream_t st);                                       // metrics()[3] = ||g||_2
    int clip_adam(float lr, float clip, int step, float gscale, hipStream_t st);
    // metrics(): loss, mse, kld, grad norm
    const IodineConfig cfg;

private:
    void layout_workspace(bool commit);
    int pack_weights(hipStream_t st);
    int decoder_fwd(int i, hipStream_t st);
    int decoder_bwd(int i, const float* dout4, bool weights, hipStream_t st);      // -> dslots_
    int refine_fwd(int i, hipStream_t st);
    int refine_bwd(int i, hipStream_t st);                                         // -> denc_, dxin_ (latent part)

    // parameters, resolved once by the constructor
    struct Weights {
        ParamRef mean_init, logsig_init, lstm_wih, lstm_whh, lstm_bih, lstm_bhh;
        ParamPair ref_conv[4], ref_mlp, mean_update, logsig_update, dec_conv[4], dec_out;
        long long skip_begin = 0, skip_end = 0;       // `slot_init`, which the optimiser leaves alone
    } w_;

    int S, N, K, I, L, Hm, Bmax, XW;          // XW = Hm + 4L (LSTM input width)
    int rs_[5];                               // spatial side of the refinement feature maps: S, S/2, ...
    int B_ = 0;
    const float* obs_ = nullptr;
    bool have_fwd_ = false;

    float *scratch_ = nullptr; size_t scratch_floats_ = 0;
    int conv_x3_ = 0;                     // OCRL_CONV_X3=1 (exploratory): the decoder's 3x3 / 64-channel layers on the split-precision bf16 kernels
    float *pk3_[3] = {nullptr, nullptr, nullptr}, *pkb3_[3] = {nullptr, nullptr, nullptr};
    float* parts_ = nullptr;                  // [I][4]: ll, mse, kl sums
    float *st1_, *st2_;
    std::vector<float*> mu_, ls_, eps_, slots_, c_[4], out4_;
    std::vector<float*> enc_, r_[4], pool_, mlpa_, xin_, acts_, cst_, hst_;
    float *zero_state_, *M_, *T_, *P1_, *W1r_, *Wxy_, *pk_[3], *pkb_[3], *Wk4_, *Wb4_, *Wp_[4], *dWp_[4];
    float *col_, *dcol_, *gates_, *dgates_, *dxin_, *dslots_, *gmu_, *gls_, *dh_, *dc_, *dcH_, *dpool_, *da_, *dr_[2], *denc_, *dout4_, *gA_, *gB_;
    float *G1_, *dW1r_, *masks_, *recon_, *rmasked_;
    int ldc_[4];
};
