// C ABI of the MLP classifier's step (include/ocrl_hip_classifier.h: ocrl_clf_ce_fwd_bwd).  Stateless: the caller owns parameters,
// gradients and the workspace.  The head's host side (limits, workspace layout, the tile code's arguments, the fold of dw) is
// acnet_host.h's Q head.
#include "../../include/ocrl_hip_classifier.h"
#include "acnet_host.h"
#include "classifier.h"

extern "C" {

int ocrl_clf_ce_fwd_bwd(const void* dv, const float* features, const float* const* w, const long long* labels, float* scalars, float* logits,
                        float* dfeatures, float* const* dw, float* ws, size_t ws_floats, void* stream) {
    const char* who = "ocrl_clf_ce_fwd_bwd";
    const ocrl_qnet_desc* d = static_cast<const ocrl_qnet_desc*>(dv);
    RC(check_qnet(d, who));
    const HeadSpec s = qnet_spec(d);
    const HeadLay y = head_layout(s);
    OCRL_REQUIRE(features && w && labels && scalars && ws, "%s: null argument", who);
    OCRL_REQUIRE(dw || !dfeatures, "%s: dfeatures without dw (a null dw evaluates: there is no backward to take them from)", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AcnetArgs a;
    RC(head_begin(a, s, y, who, features, w, dw, ws, ws_floats, dw != nullptr));
    a.logits = logits;
    a.dx = dfeatures;
    const ClfCeArgs t{labels, dw != nullptr};
    RC(clf_ce_launch(a, t, st));
    if (dw) RC(reduce_dw(a, y, dw, st));
    return head_scalars_launch(a.scal_slab, y.S, d->B, true, scalars, st);
}

}  // extern "C"
