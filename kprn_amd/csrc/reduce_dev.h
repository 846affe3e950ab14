// The reducer over a pair's paths as device functions, shared by the pooling / loss kernels (loss_stage.hip) and the explanation stage
// (explain_paths.hip): one definition, so that both produce the same bits for the same pair.
#pragma once
#include "kprn_internal.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// LogSumExp under the pooling temperature (include/kprn.h "pooling temperature"; ig = (float)(1 / gamma), formed on the host): the exponent of path q is
// (s_q - m) * ig and the pooled value log(sum) + m * ig.  At ig == 1.0f both products are exact and exp / log are the library's expf / logf, so the results
// are the bits of the plain LogSumExp.  m * ig is rounded on its own, never contracted into the sum.
//
// Under a temperature (ig != 1.0f; wave-uniform) exp and log are exp_shared / log_shared below instead: the device's expf / logf and the host's are different
// implementations that differ in the last places, and kprn_host_explain_gamma is the BIT-EXACT host statement of the rule.  Both are plain fp32 arithmetic --
// explicit fmaf, IEEE division, rintf / frexpf / ldexpf (exact), no contraction left to a compiler -- so the kernels and the host twin give the same bits.
//   exp_shared: n = rint(x log2 e), r = x - n ln 2 (two-part), Taylor to r^7 on |r| <= 0.3466 (truncation 5e-9 relative), 2^n p.  Below -87 the result is 0
//               (no denormal is ever formed), above 88 +inf; about 1 unit in the last place.
//   log_shared: x = 2^e m, m in [sqrt(1/2), sqrt 2), s = f / (2 + f) with f = m - 1, 2 atanh(s) by its series to s^11 (|s| <= 0.1716: truncation 2e-9
//               relative), e ln 2 in two parts; about 2 units in the last place.  x is a sum of exponentials whose largest is 1: finite x >= 1, or NaN.
__host__ __device__ inline float exp_shared(float x) {
#pragma clang fp contract(off)
  if (x != x) return x;
  if (!(x > -87.0f)) return 0.f;
  if (x > 88.0f) return INFINITY;
  const float n = rintf(x * 1.44269504f);
  float r = fmaf(n, -0.693145752f, x);
  r = fmaf(n, -1.42860677e-6f, r);
  float p = 1.0f / 5040.0f;
  p = fmaf(p, r, 1.0f / 720.0f);
  p = fmaf(p, r, 1.0f / 120.0f);
  p = fmaf(p, r, 1.0f / 24.0f);
  p = fmaf(p, r, 1.0f / 6.0f);
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  return ldexpf(p, (int)n);
}
__host__ __device__ inline float log_shared(float x) {
#pragma clang fp contract(off)
  if (!(x > 0.f) || x > 3.0e38f) return x != x ? x : (x > 0.f ? INFINITY : (x == 0.f ? -INFINITY : NAN));
  int e;
  float m = frexpf(x, &e);   // [0.5, 1)
  if (m < 0.70710678f) { m = m * 2.0f; e -= 1; }
  const float f = m - 1.0f;
  const float s = f / (2.0f + f);
  const float z = s * s;
  float q = 1.0f / 11.0f;
  q = fmaf(q, z, 1.0f / 9.0f);
  q = fmaf(q, z, 1.0f / 7.0f);
  q = fmaf(q, z, 0.2f);
  q = fmaf(q, z, 1.0f / 3.0f);
  const float s2 = s + s;
  const float l1p = fmaf(s2 * z, q, s2);
  const float fe = (float)e;
  return fmaf(fe, 0.693145752f, fmaf(fe, 1.42860677e-6f, l1p));
}
// exp of path q's exponent, and the pooled value
__host__ __device__ __forceinline__ float lse_exponent(float v, float m, float ig) { return (v - m) * ig; }
__host__ __device__ __forceinline__ float lse_term(float v, float m, float ig) {
  const float t = lse_exponent(v, m, ig);
  return ig == 1.0f ? expf(t) : exp_shared(t);
}
__host__ __device__ __forceinline__ float lse_finish(float sum, float m, float ig) {
#pragma clang fp contract(off)
  const float mi = m * ig;
  return (ig == 1.0f ? logf(sum) : log_shared(sum)) + mi;
}
// nn.Sigmoid on a pooled value: the library's expf at ig == 1.0f (sigmoidf_'s bits on the device), exp_shared under a temperature
__host__ __device__ __forceinline__ float pool_sigmoid_of(float y, float ig) { return 1.0f / (1.0f + (ig == 1.0f ? expf(-y) : exp_shared(-y))); }

// ---------------------------------------------------------------------------------------
// reducer over the P paths of a pair + nn.Sigmoid (OneModel.lua:284-294):
//   2: module/LogSumExp.lua:13-27 (under ig)   0: nn.Max(2)   1: module/TopK.lua:17-24 + nn.Mean(2)   (Max and TopK never see ig)
__device__ float reduce_col(const float* s, int P, int C, int reducer, int K, float ig) {
  if (reducer == 2) {
    float m = s[0];
    for (int p = 1; p < P; ++p) m = fmaxf(m, s[(int64_t)p * C]);
    float sum = 0.f;
    for (int p = 0; p < P; ++p) sum += lse_term(s[(int64_t)p * C], m, ig);
    return lse_finish(sum, m, ig);
  } else if (reducer == 0) {
    float m = s[0];
    for (int p = 1; p < P; ++p) m = fmaxf(m, s[(int64_t)p * C]);
    return m;
  } else {
    int kk = K < P ? K : P;
    // k largest by repeated selection with an exclusion bound (value, index) -- P is small (<= 28)
    float acc = 0.f;
    float last_v = INFINITY; int last_i = -1;
    for (int q = 0; q < kk; ++q) {
      float best = -INFINITY; int bi = -1;
      for (int p = 0; p < P; ++p) {
        float v = s[(int64_t)p * C];
        bool after = (v < last_v) || (v == last_v && p > last_i);
        if (after && (bi < 0 || v > best)) { best = v; bi = p; }
      }
      acc += best; last_v = best; last_i = bi;
    }
    return acc / (float)kk;
  }
}

__device__ __forceinline__ int64_t seg_begin(const int32_t* __restrict__ off, int P, int b) { return off ? (int64_t)off[b] : (int64_t)b * P; }
__device__ __forceinline__ int seg_count(const int32_t* __restrict__ off, int P, int b) { return off ? off[b + 1] - off[b] : P; }

__device__ __forceinline__ float wave_all_max(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float wave_all_sum(float v) {  // a + b == b + a bit for bit: both partners of every exchange hold the same sum
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// best (value, index) of the wave: the larger value, the lower index among equal values (TopK's tie rule, nn.Max's first maximum); i < 0 = none
__device__ __forceinline__ void wave_all_best(float& v, int& i) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const float ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
  }
}
// this lane's best candidate behind the exclusion bound (last_v, last_i), among the paths lane, lane + 64, ...
__device__ __forceinline__ void lane_best(const float* __restrict__ s, int cnt, int C, int lane, float last_v, int last_i, float& best, int& bi) {
  best = -INFINITY; bi = -1;
  for (int p = lane; p < cnt; p += 64) {
    const float v = s[(int64_t)p * C];
    const bool after = (v < last_v) || (v == last_v && p > last_i);
    if (after && (bi < 0 || v > best)) { best = v; bi = p; }
  }
}

// the reducer over one pair by one wave (cnt > RAGGED_THREAD_MAX); every lane returns the same value.  LogSumExp: two passes (max, sum of exp)
__device__ float reduce_col_wave(const float* __restrict__ s, int cnt, int C, int reducer, int K, float ig, int lane) {
  if (reducer != 1) {
    float m = -INFINITY;
    for (int p = lane; p < cnt; p += 64) m = fmaxf(m, s[(int64_t)p * C]);
    m = wave_all_max(m);
    if (reducer == 0) return m;
    float sum = 0.f;
    for (int p = lane; p < cnt; p += 64) sum += lse_term(s[(int64_t)p * C], m, ig);
    return lse_finish(wave_all_sum(sum), m, ig);
  }
  const int kk = K < cnt ? K : cnt;
  float acc = 0.f, last_v = INFINITY;
  int last_i = -1;
  for (int q = 0; q < kk; ++q) {
    float best; int bi;
    lane_best(s, cnt, C, lane, last_v, last_i, best, bi);
    wave_all_best(best, bi);
    acc += best; last_v = best; last_i = bi;
  }
  return acc / (float)kk;
}

__device__ __forceinline__ float reduce_seg(const float* __restrict__ s, int cnt, int C, int reducer, int K, float ig, int wave_mode, int lane) {
  return (wave_mode && cnt > kk::RAGGED_THREAD_MAX) ? reduce_col_wave(s, cnt, C, reducer, K, ig, lane) : reduce_col(s, cnt, C, reducer, K, ig);
}

}  // namespace
