// C ABI of the MLP classifier's step (include/ocrl_hip_classifier.h: ocrl_clf_ce_fwd_bwd).  Stateless: the caller owns parameters,
// gradients and the workspace.  The head's host side (limits, workspace layout, the tile code's arguments, the fold of dw) is
// dqn_unit.cpp's.
#include "../../include/ocrl_hip_classifier.h"
#include "classifier.h"

using namespace qnet;

extern "C" {

int ocrl_clf_ce_fwd_bwd(const void* dv, const float* features, const float* const* w, const long long* labels, float* scalars, float* logits,
                        float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_clf_ce_fwd_bwd";
    const ocrl_qnet_desc* d = static_cast<const ocrl_qnet_desc*>(dv);
    RC(check_qnet(d, who));
    const QLay y = q_layout(d);
    OCRL_REQUIRE(features && w && labels && scalars && ws, "%s: null argument", who);
    RC(check_ptrs((const void* const*)w, y.np, who));
    OCRL_REQUIRE(dw || !dfeatures, "%s: dfeatures without dw (a null dw evaluates: there is no backward to take them from)", who);
    if (dw) RC(check_ptrs((const void* const*)dw, y.np, who));
    OCRL_REQUIRE(ws_floats >= y.total, "%s: workspace too small (%zu < %zu floats)", who, ws_floats, y.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    fill_args(a, d, y, features, w, ws, dw != nullptr);
    a.logits = logits;
    a.dx = dfeatures;
    const ClfCeArgs s{labels, dw != nullptr};
    RC(clf_ce_launch(a, s, st));
    if (dw) RC(reduce_dw(a, y, dw, st));
    return clf_scalars_launch(a.scal_slab, y.S, d->B, scalars, st);
}

}  // extern "C"
