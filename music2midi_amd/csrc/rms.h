// The piece of RMSNorm that rmsnorm_kernel (enc_kernels.hip) and the fused norm_gemm_kernel (enc_gemm.hip) must share to the bit.
#pragma once
#include <hip/hip_runtime.h>

namespace m2m {

// Sum of squares of one 16-byte chunk of a row, every product and every sum rounded on its own (no FMA contraction): x^2 + y^2, + z^2,
// + w^2.  Compiled with contraction OFF because rmsnorm_kernel and the fused norm_gemm_kernel must produce the
// SAME bits: left to the compiler, one context gave packed multiplies + adds (this form), another a chain of fused multiply-adds — one
// ulp apart in rstd, which flips a bf16 rounding of the normalised row about once per 10^5 elements (found by the bit-identity test).
__device__ inline float rms_sumsq4(const float4& v) {
#pragma clang fp contract(off)      // (HIP's __fmul_rn / __fadd_rn are plain * and +: they do not stop the contraction)
  const float a = v.x * v.x, b = v.y * v.y, c = v.z * v.z, d = v.w * v.w;
  return ((a + b) + c) + d;
}

}  // namespace m2m
