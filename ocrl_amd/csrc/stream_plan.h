// The stream schedule of the SLATE training step as data: what OCRL_OVERLAP, OCRL_DW_SIDE and OCRL_TOKENS_LATE (switches.h) decide,
// worked out once, when SlateModel creates its streams.  Plain C++, no HIP types (tests/test_stream_plan_cpu.py compiles it alone).
//
// The step has two branches that are independent between the observation and the transformer decoder: the CNN encoder + slot attention,
// and the dVAE (tokens, reconstruction loss) -- many short 64-wide products that do not fill the machine.  The plan says where the dVAE
// branch is forked to the side stream and joined again, in each direction, and where the weight-gradient products go that nothing later
// in the step reads.  The use_bcdec configuration has no dVAE branch: it ignores both placements and keeps everything on the main stream.
#pragma once

enum class FwdDvae {
    Serial,             // overlap 0: on the main stream, before the encoder
    BesideEncoder,      // 1: forked before the encoder, joined before the decoder
    AtSlotAttention,    // 2, 3: forked inside the encoder, right before the slot-attention iterations
    AtStart,            // 4: forked inside the encoder after the slot preparation launch, beside the convolutions
    AfterConvs,         // 5: forked after the encoder convolutions, beside the input LayerNorm / MLP and the slot-attention chain
};
enum class BwdDvae {
    SerialLast,         // overlap 0: on the main stream, after decoder and encoder
    BesideAll,          // 1: forked first, beside decoder + encoder, joined at the end (per-kernel timings of both branches stop being comparable)
    AtSlotAttention,    // 2: forked inside the encoder backward at the slot-attention launch, joined before the 5x5 convolutions
    BesideDecoder,      // >= 3: forked first, beside the decoder backward; joined before the encoder backward when dw == 0, else inside
                        //       it, before the convolutions, which then have the machine to themselves (their timings stay comparable)
};

struct StreamPlan {
    bool side = false;                          // a side stream exists (the dVAE lane)
    int dw = 0;                                 // lane of the decoder's weight-gradient products: 0 main, 1 the dVAE lane (behind the dVAE backward), 2 a stream of their own
    FwdDvae fwd_dvae = FwdDvae::Serial;         // forward placement of the dVAE branch
    bool tokens_early = false;                  // the decoder waits for the dVAE's tokens only; the rest of that branch is joined before the losses are added
    BwdDvae bwd_dvae = BwdDvae::SerialLast;     // backward placement of the dVAE branch
    bool sa_wgrads_on_side = false;             // what only consumes the slot-attention backward's outputs runs on the dVAE lane (idle by then), joined before the convolutions
};

// overlap outside 0..5 falls where the comparisons it replaces put it: below 2 as 1, above 5 as 3; dw_side other than 0 / 2 as 1
inline StreamPlan stream_plan(int overlap, int dw_side, bool tokens_late, bool use_bcdec) {
    StreamPlan p;
    p.side = overlap != 0;
    p.dw = (overlap >= 3 && !use_bcdec) ? (dw_side == 2 ? 2 : dw_side ? 1 : 0) : 0;
    p.fwd_dvae = overlap == 0 ? FwdDvae::Serial : overlap < 2 ? FwdDvae::BesideEncoder : overlap == 4 ? FwdDvae::AtStart
               : overlap == 5 ? FwdDvae::AfterConvs : FwdDvae::AtSlotAttention;
    p.tokens_early = overlap >= 3 && !tokens_late;
    p.bwd_dvae = overlap == 0 ? BwdDvae::SerialLast : overlap < 2 ? BwdDvae::BesideAll : overlap == 2 ? BwdDvae::AtSlotAttention
               : BwdDvae::BesideDecoder;
    p.sa_wgrads_on_side = overlap >= 3 && !use_bcdec;
    return p;
}
