// gemm_kernel instantiations for k-contiguous A and B (y = x W^T and the vocabulary heads with soft-max epilogues); see gemm_impl.h
#include "gemm_impl.h"

int gemm_launch_tt(const GemmArgs& a, const GemmPlan& p, hipStream_t st) { return launch_family<true, true>(a, p, st); }
