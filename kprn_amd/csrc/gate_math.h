// Gate functions of the recurrent cells (sigmoid, tanh) on v_exp_f32 / v_rcp_f32 (1 ulp each) instead of libm's ~40-instruction
// expf / tanhf.  Two families with distinct names; tests/test_gpu_gate_math.py runs every finite float32 through both (and through the
// fused kernels' fast_sigmoid / fast_tanh, lstm_fused_common.h) against double precision on the device and pins the bounds below.
#pragma once
#include <hip/hip_runtime.h>

// ---- fp32-accurate: exp_fast / sigm / tanh_fast (gemm_tiled.hip, layer_f32_persist.hip) -----------------------------------------------
// The tiled step kernel's cell epilogue evaluates 80 of them per thread and 128 x 32-unit tile, which with libm cost a quarter of the
// tile's MFMA time.  e^x = 2^t (1 + ln2 (x log2e - t)): the product's rounding residual (and log2e's low word) is folded back in, so
// the result stays within ~2 ulp for |x| <= 88.72; 1 / (1 + e^-x) and tanh x = (1 - e^-2|x|) / (1 + e^-2|x|) then have ABSOLUTE
// error <= 1.5e-7 for every finite x (measured over all of them: 1.10e-7 / 1.25e-7).
// The argument is clamped to [-88.72, 88.72] first (one v_med3_f32): from 128 ln2 = 88.7228 up v_exp_f32 returns +inf and the
// residual term fma(inf, lo, inf) is NaN whenever lo <= 0 (sigm(x) was NaN for a third of the x in [-130, -88.72]); from
// |x| = 2.4e38 on, t itself overflows to -inf and fma(0, inf, 0) is NaN.  exp_fast saturates at e^88.72 = 3.39e38 instead.
// Wherever the unclamped form was finite, the clamp changes no bit of sigm(x) for x >= -88.72 and none of tanh_fast(x): beyond the
// clamp, 1 + e^-88.72 and 1 - e^-88.72 round to 1 exactly as the smaller e^x they replace did.
// (The bound goes through an empty asm so that both ends are ONE scalar register, the lower one by a negation modifier: a VOP3 on
// gfx950 reads one scalar operand and no literal, so two distinct constants cost a vector register -- which spilled in the
// persistent layer kernels, layer_f32_persist.hip.)
__device__ __forceinline__ float exp_fast(float x) {
  float c = 88.72f;
  asm("" : "+s"(c));
  x = __builtin_amdgcn_fmed3f(x, -c, c);
  const float t = x * 1.4426950408889634f;
  const float lo = __builtin_fmaf(x, 1.9259629911e-8f, __builtin_fmaf(x, 1.4426950408889634f, -t));
  const float e = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(e, lo * 0.6931471805599453f, e);
}
__device__ __forceinline__ float sigm(float x) { return __builtin_amdgcn_rcpf(1.0f + exp_fast(-x)); }
__device__ __forceinline__ float tanh_fast(float x) {
  const float t = exp_fast(-2.0f * __builtin_fabsf(x));
  return __builtin_copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), x);
}

// ---- one exp2 + one rcp: sigm_e2 / tanh_e2 (the bf16 pipelines: lstm_bf16.hip, lstm_bf16_persist.hip, lstm_bf16_bwd_persist.hip) ----
// At bf16 precision the cell's transcendental functions, not the MFMAs, were most of those kernels' time with libm.  No residual
// term: exp2 of a huge argument gives inf or 0 and rcp of inf gives 0, so both are finite everywhere.  Absolute error over every
// finite float32: sigm_e2 <= 1.2e-7, tanh_e2 <= 2.3e-7 (measured 1.108e-7 at x = 3.63 / 2.216e-7 at x = 1.82).
__device__ __forceinline__ float sigm_e2(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
__device__ __forceinline__ float tanh_e2(float x) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.8853900817779268f * x)) - 1.0f; }
