// C ABI of the stateless optimiser steps (include/ocrl_hip.h: ocrl_flat_clip_adam_*, ocrl_flat_clip_rmsprop_*):
// torch.nn.utils.clip_grad_norm_ (L2) followed by torch.optim.Adam, as PPO.train applies them to the policy, or by the TF-style RMSprop
// of A2C.train, on caller-owned flat fp32 buffers.  The norm is IODINE's io_l2norm_launch (iodine.hip: per-block sums of squares, folded
// in a fixed order) and the updates optim.hip's clip_adam / clip_rmsprop kernels.  The _multi entry points take the same step over several
// such buffers under one joint norm (optim.hip's multi_* kernels: three launches whatever the number of segments).
#include "../../include/ocrl_hip.h"
#include "common.h"
#include "kernels.h"
#include <cstdio>
#include <cstdlib>

namespace {
constexpr size_t WS_FLOATS = 1024;      // io_l2norm's per-block partial sums
constexpr size_t MULTI_WS_FLOATS = (size_t)FLAT_MAX_SEG * FLAT_SEG_BLOCKS;      // the multi step's: every segment's blocks
static_assert(FLAT_MAX_SEG == OCRL_FLAT_MAX_SEGMENTS, "kernels.h and ocrl_hip.h disagree on the segment count");
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// The decimal a float argument stands for: the shortest one that rounds to it (0.999f -> 0.999, not 0.99900001287).  optim.hip takes
// 1 - beta and the bias corrections in double from the decimal betas, as torch.optim.Adam does; 1 - 0.999f is 4.7e-5 off 0.001.
double decimal(float x) {
    char buf[32];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(buf, sizeof buf, "%.*g", digits, (double)x);
        if (strtof(buf, nullptr) == x) return strtod(buf, nullptr);
    }
    return (double)x;
}
}  // namespace

extern "C" {

size_t ocrl_flat_clip_adam_ws_floats(void) { return WS_FLOATS; }

int ocrl_flat_clip_adam_l2(float* p, const float* g, float* m, float* v, long long n, float max_norm, float lr, float beta1, float beta2, float eps,
                           int step, float* norm_out, float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(p && g && m && v && norm_out && ws, "ocrl_flat_clip_adam_l2: null argument");
    OCRL_REQUIRE(n >= 1, "ocrl_flat_clip_adam_l2: n >= 1 (got %lld)", n);
    OCRL_REQUIRE(step >= 1, "ocrl_flat_clip_adam_l2: step counts from 1 (got %d)", step);
    OCRL_REQUIRE(ws_floats >= WS_FLOATS, "ocrl_flat_clip_adam_l2: workspace too small (%zu < %zu floats)", ws_floats, WS_FLOATS);
    OCRL_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), "ocrl_flat_clip_adam_l2: p, g, m and v must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RC(io_l2norm_launch(g, n, norm_out, ws, ws_floats, st));
    const double b1 = decimal(beta1), b2 = decimal(beta2), e = decimal(eps);
    const long long n4 = n & ~3LL;
    if (n4) RC(clip_adam_launch(p, g, m, v, n4, norm_out, max_norm, lr, b1, b2, e, step, 1.f, st));
    if (n > n4) RC(clip_adam_tail_launch(p + n4, g + n4, m + n4, v + n4, (int)(n - n4), norm_out, max_norm, lr, b1, b2, e, step, 1.f, st));
    return 0;
}

size_t ocrl_flat_clip_rmsprop_ws_floats(void) { return WS_FLOATS; }

int ocrl_flat_clip_rmsprop_l2(float* p, const float* g, float* sq, long long n, float max_norm, float lr, float alpha, float eps, float* norm_out,
                              float* ws, size_t ws_floats, void* stream) {
    OCRL_REQUIRE(p && g && sq && norm_out && ws, "ocrl_flat_clip_rmsprop_l2: null argument (p, g, sq, norm_out or ws)");
    OCRL_REQUIRE(n >= 1, "ocrl_flat_clip_rmsprop_l2: n >= 1 (got %lld)", n);
    OCRL_REQUIRE(alpha > 0.f && alpha < 1.f, "ocrl_flat_clip_rmsprop_l2: alpha must lie in (0, 1) (got %g)", (double)alpha);
    OCRL_REQUIRE(eps > 0.f, "ocrl_flat_clip_rmsprop_l2: eps must be positive (got %g)", (double)eps);
    OCRL_REQUIRE(ws_floats >= WS_FLOATS, "ocrl_flat_clip_rmsprop_l2: workspace too small (%zu < %zu floats)", ws_floats, WS_FLOATS);
    OCRL_REQUIRE(aligned16(p) && aligned16(g) && aligned16(sq), "ocrl_flat_clip_rmsprop_l2: p, g and sq must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RC(io_l2norm_launch(g, n, norm_out, ws, ws_floats, st));
    const double a = decimal(alpha), e = decimal(eps);
    const long long n4 = n & ~3LL;
    if (n4) RC(clip_rmsprop_launch(p, g, sq, n4, norm_out, max_norm, lr, a, e, st));
    if (n > n4) RC(clip_rmsprop_tail_launch(p + n4, g + n4, sq + n4, (int)(n - n4), norm_out, max_norm, lr, a, e, st));
    return 0;
}

size_t ocrl_flat_clip_multi_ws_floats(void) { return MULTI_WS_FLOATS; }

// everything the two multi entry points check alike, and the table their kernels take; `who` names the entry point, need_s1: Adam
static int multi_table(const char* who, const ocrl_flat_segment* seg, int nseg, bool need_s1, const float* norm_out, const float* ws,
                       size_t ws_floats, FlatSegs* out) {
    OCRL_REQUIRE(nseg >= 1 && nseg <= OCRL_FLAT_MAX_SEGMENTS, "%s: nseg must lie in [1, %d] (got %d)", who, OCRL_FLAT_MAX_SEGMENTS, nseg);
    OCRL_REQUIRE(seg && norm_out && ws, "%s: null argument (seg, norm_out or ws)", who);
    OCRL_REQUIRE(ws_floats >= MULTI_WS_FLOATS, "%s: workspace too small (%zu < %zu floats)", who, ws_floats, MULTI_WS_FLOATS);
    FlatSegs t = {};
    t.nseg = nseg;
    for (int s = 0; s < nseg; ++s) {
        const ocrl_flat_segment& q = seg[s];
        OCRL_REQUIRE(q.p && q.g && q.s0 && (q.s1 || !need_s1), "%s: segment %d: null pointer (p, g, s0%s)", who, s, need_s1 ? " or s1" : "");
        OCRL_REQUIRE(q.n >= 1, "%s: segment %d: n >= 1 (got %lld)", who, s, q.n);
        OCRL_REQUIRE(aligned16(q.p) && aligned16(q.g) && aligned16(q.s0) && (!need_s1 || aligned16(q.s1)),
                     "%s: segment %d: p, g, s0%s must be 16-byte aligned", who, s, need_s1 ? " and s1" : "");
        t.p[s] = q.p; t.g[s] = q.g; t.s0[s] = q.s0; t.s1[s] = need_s1 ? q.s1 : nullptr; t.n[s] = q.n;
    }
    *out = t;
    return 0;
}

int ocrl_flat_clip_adam_l2_multi(const ocrl_flat_segment* seg, int nseg, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                                 float* norm_out, float* ws, size_t ws_floats, void* stream) {
    FlatSegs t;
    RC(multi_table("ocrl_flat_clip_adam_l2_multi", seg, nseg, true, norm_out, ws, ws_floats, &t));
    OCRL_REQUIRE(step >= 1, "ocrl_flat_clip_adam_l2_multi: step counts from 1 (got %d)", step);
    return multi_clip_adam_launch(t, norm_out, max_norm, lr, decimal(beta1), decimal(beta2), decimal(eps), step, ws, ws_floats,
                                  static_cast<hipStream_t>(stream));
}

int ocrl_flat_clip_rmsprop_l2_multi(const ocrl_flat_segment* seg, int nseg, float max_norm, float lr, float alpha, float eps, float* norm_out,
                                    float* ws, size_t ws_floats, void* stream) {
    FlatSegs t;
    RC(multi_table("ocrl_flat_clip_rmsprop_l2_multi", seg, nseg, false, norm_out, ws, ws_floats, &t));
    OCRL_REQUIRE(alpha > 0.f && alpha < 1.f, "ocrl_flat_clip_rmsprop_l2_multi: alpha must lie in (0, 1) (got %g)", (double)alpha);
    OCRL_REQUIRE(eps > 0.f, "ocrl_flat_clip_rmsprop_l2_multi: eps must be positive (got %g)", (double)eps);
    return multi_clip_rmsprop_launch(t, norm_out, max_norm, lr, decimal(alpha), decimal(eps), ws, ws_floats, static_cast<hipStream_t>(stream));
}

}  // extern "C"
