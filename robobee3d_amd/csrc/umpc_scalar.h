// Scalar wrappers shared by every device header: one overload per scalar type, each a single instruction or a short
// fixed sequence. No generated code, no other project header.
#pragma once
#include <hip/hip_runtime.h>

namespace umpc {

// |v| as a source modifier (c_absval of glob_opts.h:91; identical for every non-NaN value)
__device__ __forceinline__ float umpc_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double umpc_abs(double v) { return __builtin_fabs(v); }
// max/min of non-NaN values (c_max / c_min of glob_opts.h:95-99): one v_max / v_min
__device__ __forceinline__ float umpc_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ float umpc_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double umpc_max(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ double umpc_min(double a, double b) { return __builtin_fmin(a, b); }
// 1/sqrt(v): the reference does sqrtf then 1.0f/ (two roundings, scaling.c:98-103). fp32 uses the
// hardware v_rsq_f32 (1 ulp, one quarter-rate instruction instead of ~20). fp64: v_rsq_f64 (~2^-24) + two Newton
// steps (error squares each step -> rounding level, within ~2 ulp of the reference's two-rounding value) in 9
// instructions where the correctly rounded sqrt followed by the IEEE divide expands to ~35; the Ruiz passes take
// 840 of them per step. Arguments are limit_scaling()'d: finite, in [1e-4, 1e4].
__device__ __forceinline__ float umpc_rsqrt(float v) { return __builtin_amdgcn_rsqf(v); }
__device__ __forceinline__ double umpc_rsqrt(double v) {
  double y = __builtin_amdgcn_rsq(v);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double e = __builtin_fma(-(v * y), y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
  }
  return y;
}
// 1/v for finite, normal, nonzero v: fp32 IEEE divide; fp64 v_rcp_f64 + two Newton steps (5 instructions against ~25)
__device__ __forceinline__ float umpc_recip(float v) { return 1.0f / v; }
__device__ __forceinline__ double umpc_recip(double v) {
  double y = __builtin_amdgcn_rcp(v);
#pragma unroll
  for (int k = 0; k < 2; ++k) y = __builtin_fma(y, __builtin_fma(-v, y, 1.0), y);
  return y;
}
// 1/v where only residual NORMS consume the result
__device__ __forceinline__ float umpc_rcp_fast(float v) { return __builtin_amdgcn_rcpf(v); }
__device__ __forceinline__ double umpc_rcp_fast(double v) { return umpc_recip(v); }
__device__ __forceinline__ float umpc_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double umpc_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float umpc_sqrt(float v) { return __fsqrt_rn(v); }
__device__ __forceinline__ float umpc_sqrt_fast(float v) { return __builtin_amdgcn_sqrtf(v); }   // v_sqrt_f32, 1 ulp
__device__ __forceinline__ double umpc_sqrt_fast(double v) { return __dsqrt_rn(v); }
__device__ __forceinline__ double umpc_sqrt(double v) { return __dsqrt_rn(v); }
__device__ __forceinline__ float umpc_sin(float v) { return sinf(v); }
__device__ __forceinline__ double umpc_sin(double v) { return sin(v); }
__device__ __forceinline__ float umpc_cos(float v) { return cosf(v); }
__device__ __forceinline__ double umpc_cos(double v) { return cos(v); }

}  // namespace umpc
