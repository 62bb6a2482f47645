// The OCRL_* environment switches of the library: one table, and the only place in csrc/ that reads the environment.  All are optional
// development / comparison knobs; none changes a result beyond fp32 summation order (OCRL_CONV_X3: beyond fp32 rounding).  Host only, no
// HIP types.  INTEGRATION.md carries the same table for users (tests/test_switches_cpu.py holds the two together).
//
// A row: name, default (what an unset variable gives), the moment it is read, meaning with its values.
//   PROCESS  read at the first use and kept for the life of the process      sw::process<sw::name>()
//   MODEL    read when a model object asks; the object stores the value      sw::model<sw::name>()
//   CALL     read at every call                                              sw::call<sw::name>()
// The reader is chosen at the site and checked against the row when the site is compiled.  A set variable is parsed with atoi(), so
// text that is no number gives 0, with three exceptions written out in sw::parse below.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#define OCRL_SWITCHES(X)                                                                                                                \
    X(OCRL_GEMM_TILE, 0, PROCESS, "BMxBN (e.g. 128x64) forces that GEMM tile where the operand layout builds it; read as BM * 1000 + BN, 0 (unset, or no such text) = the dispatch rule") \
    X(OCRL_GEMM_SB, 0, PROCESS, "GEMM LDS buffering: 0 = the buffering rule, 1 = always single, 2 = always double")                          \
    X(OCRL_CONV_LAT, 1, PROCESS, "0 keeps the small grids of encode() on the throughput convolution; 1 = the low-latency kernel below ~0.6 workgroups per CU") \
    X(OCRL_BC_WGRAD, 2, PROCESS, "weight gradient of the broadcast decoder's output convolution: 1 = the VALU form, anything else = the MFMA form") \
    X(OCRL_SA_GROUP, 1, PROCESS, "0 = one image per slot-side workgroup (development comparison); otherwise 16 / num_slots images where the LDS allows") \
    X(OCRL_SA_WGS, 0, PROCESS, "n > 0 = streaming slot-attention workgroups per CU per launch; 0 = the kernel's own launch bound")           \
    X(OCRL_SA_FWD, 2, PROCESS, "1 = the earlier streaming forward (slots on the lanes); otherwise positions on the lanes")                   \
    X(OCRL_SA_BWD, 2, PROCESS, "1 = the earlier streaming backward; otherwise positions on the lanes")                                       \
    X(OCRL_CONV_X3, 0, MODEL, "1 = the 5x5 and 3x3 64-channel convolutions on the split-precision bf16 kernels (exploratory), read when a model is created; conv_wgrad_launch callers that pass x3 < 0 get a value read once per process") \
    X(OCRL_ENCODE_GRAPH, 0, MODEL, "1 = encode() at B <= 32 replays a captured hipGraph (measured no faster); read at a model's first encode()") \
    X(OCRL_ATTN_DS_MB, 2048, MODEL, "cap in megabytes of the dS workspace a model carves for the hand-off attention backward: min(whole batch, cap); 0 or negative = none (the two-kernel form)") \
    X(OCRL_OVERLAP, 5, MODEL, "stream plan of the SLATE step (stream_plan.h), read at the first bind: 0 = single stream, 1 = dVAE branch beside encoder and decoder, 2 = beside slot attention, 3 / 4 / 5 = backward beside the decoder backward and forward forked at slot attention / at the start / after the encoder convolutions") \
    X(OCRL_DW_SIDE, 2, MODEL, "the decoder's weight-gradient products under OVERLAP >= 3: 0 = main stream, 1 = the dVAE side stream, 2 = a stream of their own; read with OVERLAP") \
    X(OCRL_TOKENS_LATE, 0, MODEL, "set (to anything) = the main stream joins the whole dVAE forward before the decoder instead of waiting for its tokens only (OVERLAP >= 3); read with OVERLAP") \
    X(OCRL_SA_INPUT, 1, MODEL, "slot-attention input LayerNorm + MLP: 1 = one fused kernel per direction, 2 = fused forward only, 0 = the unfused chain; read at every bind") \
    X(OCRL_XATTN, 1, MODEL, "0 = the unfused cross-attention kernels instead of the folded form; read at every bind")                        \
    X(OCRL_ATTN_BWD, 0, CALL, "self-attention backward: 1 = one pass, 2 = two kernels, 3 or 0 (unset) = dS hand-off when the caller gave a workspace, else two kernels") \
    X(OCRL_SA_NS, 0, CALL, "n > 0 = that many streaming workgroups per image, so a small batch sums like a large one; 0 = sized to the GPU")

namespace sw {

enum Moment { PROCESS, MODEL, CALL };
enum Switch {
#define X(name, def, when, meaning) name,
    OCRL_SWITCHES(X)
#undef X
        COUNT
};
struct Row { const char* name; long long def; Moment when; const char* meaning; };
constexpr Row TABLE[COUNT] = {
#define X(name, def, when, meaning) {#name, def, when, meaning},
    OCRL_SWITCHES(X)
#undef X
};

inline long long parse(Switch s, const char* text) {
    if (s == OCRL_GEMM_TILE) { int bm = 0, bn = 0; return sscanf(text, "%dx%d", &bm, &bn) == 2 ? bm * 1000 + bn : 0; }
    if (s == OCRL_TOKENS_LATE) return 1;             // its presence is the switch
    if (s == OCRL_ATTN_DS_MB) return atoll(text);    // megabytes, multiplied out to bytes by its reader
    return atoi(text);
}
inline long long read(Switch s) {
    const char* e = getenv(TABLE[s].name);
    return e ? parse(s, e) : TABLE[s].def;
}

// OCRL_CONV_X3 is the one name with two moments (its row says where)
constexpr bool read_at(Switch s, Moment m) { return TABLE[s].when == m || (s == OCRL_CONV_X3 && m == PROCESS); }

template <Switch S>
long long process() {
    static_assert(read_at(S, PROCESS), "this switch is not read once per process (switches.h)");
    static const long long v = read(S);
    return v;
}
template <Switch S>
long long model() {
    static_assert(read_at(S, MODEL), "this switch is not read per model (switches.h)");
    return read(S);
}
template <Switch S>
long long call() {
    static_assert(read_at(S, CALL), "this switch is not read at every call (switches.h)");
    return read(S);
}

}  // namespace sw
