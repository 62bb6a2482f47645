// gemm_kernel instantiations for m-contiguous A (weight gradients dW = dy^T x, split-k); see gemm_impl.h
#include "gemm_impl.h"

int gemm_launch_nn(const GemmArgs& a, const GemmPlan& p, hipStream_t st) {
    if (!a.bkc) return launch_family<false, false>(a, p, st);
    return launch_family<false, true>(a, p, st);
}
