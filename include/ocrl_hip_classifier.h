/* C ABI of the MLP classifier's gradient step in libocrl_hip.so (gfx950): the head, the soft-max cross-entropy, the accuracy and the
 * backward in one entry point.  A seventh header beside ocrl_hip.h, ocrl_hip_dqn.h, ocrl_hip_rollout.h, ocrl_hip_replay.h,
 * ocrl_hip_c51.h and ocrl_hip_noisy.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads them all); the conventions are
 * ocrl_hip_dqn.h's: the entry is stateless and takes device pointers (fp32 unless said otherwise), returns 0 on success and leaves the
 * message of a failure in ocrl_last_error(), checks its arguments before any launch, enqueues on `stream` (a hipStream_t) without
 * synchronising with the host, uses no atomics, bounds every loop and is bit-reproducible.
 *
 * The head is ocrl_hip_dqn.h's chain with A = the number of classes: features [B, F] -> n x [Linear(dims[l]), acts[l]] -> Linear(last, A)
 *   = z [B, A].  `d` points to an ocrl_qnet_desc of ocrl_hip_dqn.h (this header stays self-contained and declares no struct of its own:
 *   the pointer is a `const void*` here); the limits, the arithmetic and the order of w / dw (2 (n + 1) device pointers in state_dict
 *   order) are those of ocrl_qnet_*.
 *
 * ocrl_clf_ce_fwd_bwd: per row b, with y = labels[b] (int64):
 *     y outside [0, A):  the row contributes nothing to any sum or gradient (its dfeatures are 0); its logits are still written
 *     m     = max_a z[b, a]
 *     lse   = m + log(sum_a exp(z[b, a] - m))
 *     l_b   = lse - z[b, y]
 *     dz[b, a] = (exp(z[b, a] - lse) - [a == y]) / B
 *     hit_b = (the lowest index of the maximum of z[b, :] == y)
 *   scalars [3] = sum_b l_b / B, sum_b hit_b / B, the number of rows whose label was in range (exact below 2^24 rows).  The denominators
 *   stay B whatever the third scalar says: no tile depends on another, and the caller who wants the mean over the valid rows divides.
 *   logits [B, A] (may be NULL) = z, the bits ocrl_qnet_fwd writes.
 *   dw, and dfeatures [B, F] when given, are the gradients of scalars[0], overwritten, not accumulated.
 *   dw == NULL evaluates: no backward, dfeatures must be NULL too, the same scalars and logits bit for bit.
 *   Three launches (the tiles' forward + loss + backward with z and the layer cotangents in LDS, the fold of the partial dw, the fold of
 *   the scalars in slab order), two when evaluating.  A tile's terms are added in row order, the tiles of a slab in tile order, the slabs
 *   in slab order.  A row's logits do not depend on its position in the batch or on B.
 *   ws_floats >= ocrl_qnet_ws_floats(d), evaluating too (the scalars' partial sums live there).
 *   Rejected before any launch: a null d / features / w / labels / scalars / ws, a null entry of w or dw, dfeatures without dw, a
 *   workspace below ocrl_qnet_ws_floats(d), and every descriptor ocrl_qnet_ws_floats rejects. */
#ifndef OCRL_HIP_CLASSIFIER_H
#define OCRL_HIP_CLASSIFIER_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int ocrl_clf_ce_fwd_bwd(const void* d /* an ocrl_qnet_desc */, const float* features, const float* const* w, const long long* labels,
                        float* scalars /* [3] */, float* logits /* [B, A] or NULL */, float* dfeatures /* [B, F] or NULL */,
                        float* const* dw /* NULL: evaluation */, float* ws, size_t ws_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
