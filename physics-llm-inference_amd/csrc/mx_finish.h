// The finishing expressions of the block-scaled GEMMs, shared by gemm_fp8.hip,
// gemm_mxfp4.hip and gemm_mx_splitk.hip: every kernel of a format applies the
// same expression to its fp32 sum, so two kernels agree bit for bit wherever
// their sums do.
#pragma once

#include <hip/hip_runtime.h>

namespace pli {

// W8A8: both row scales folded in after the sum
__device__ __forceinline__ float fp8a_finish(float sum, float xs, float ws) { return sum * (xs * ws); }
// W4A8: the weight's scales went into the sum.  Bitwise fp8a_finish(sum, xs,
// 1.0f): xs * 1.0f is exact, NaN and infinity included.
__device__ __forceinline__ float mxfp4a_finish(float sum, float xs) { return sum * xs; }

}  // namespace pli
