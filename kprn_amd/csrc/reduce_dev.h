// The reducer over a pair's paths as device functions, shared by the pooling / loss kernels (loss_stage.hip) and the explanation stage
// (explain_paths.hip): one definition, so that both produce the same bits for the same pair.
#pragma once
#include "kprn_internal.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------------------
// reducer over the P paths of a pair + nn.Sigmoid (OneModel.lua:284-294):
//   2: module/LogSumExp.lua:13-27   0: nn.Max(2)   1: module/TopK.lua:17-24 + nn.Mean(2)
__device__ float reduce_col(const float* s, int P, int C, int reducer, int K) {
  if (reducer == 2) {
    float m = s[0];
    for (int p = 1; p < P; ++p) m = fmaxf(m, s[(int64_t)p * C]);
    float sum = 0.f;
    for (int p = 0; p < P; ++p) sum += expf(s[(int64_t)p * C] - m);
    return logf(sum) + m;
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
__device__ float reduce_col_wave(const float* __restrict__ s, int cnt, int C, int reducer, int K, int lane) {
  if (reducer != 1) {
    float m = -INFINITY;
    for (int p = lane; p < cnt; p += 64) m = fmaxf(m, s[(int64_t)p * C]);
    m = wave_all_max(m);
    if (reducer == 0) return m;
    float sum = 0.f;
    for (int p = lane; p < cnt; p += 64) sum += expf(s[(int64_t)p * C] - m);
    return logf(wave_all_sum(sum)) + m;
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

__device__ __forceinline__ float reduce_seg(const float* __restrict__ s, int cnt, int C, int reducer, int K, int wave_mode, int lane) {
  return (wave_mode && cnt > kk::RAGGED_THREAD_MAX) ? reduce_col_wave(s, cnt, C, reducer, K, lane) : reduce_col(s, cnt, C, reducer, K);
}

}  // namespace
