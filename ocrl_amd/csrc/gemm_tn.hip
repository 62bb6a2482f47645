// gemm_kernel instantiations for k-contiguous A, n-contiguous B (dx = dy W and the soft-max backward epilogue); see gemm_impl.h
#include "gemm_impl.h"

int gemm_launch_tn(const GemmArgs& a, const GemmPlan& p, hipStream_t st) { return launch_family<true, false>(a, p, st); }
