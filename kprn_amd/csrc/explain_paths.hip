// Explanation stage (include/kprn.h "explaining a recommendation"): the M strongest paths behind a pair's pooled score, each with the share it takes of that
// score: the path's normalised share of the pooled value (for LogSumExp at pooling temperature 1 that is d pooled / d s_q, the factor the loss stage multiplies
// dy by; under a temperature gamma the derivative is the share / gamma and the share is what is reported).  Forward only; reads column cid of the mapper output S [N][C] in
// place (stride C), writes no float atomics, uses no LDS.
//
// One definition of the rule serves the kernels and the host twin (namespace ex, __host__ __device__):
//   order   score descending, then path index ascending among equal scores (plain fp32 > / ==; -0 == +0); a NaN sorts after every number, lower index
//           first.  Found by repeated selection with an exclusion bound (the last selected (score, index)), as reduce_col's TopK branch does.
//   weight  LogSumExp: expf((s_q - m) ig) / sum_p expf((s_p - m) ig), ig = 1 / gamma (option "pool_gamma"; reduce_dev.h lse_term);  Max: 1 at place 0;  TopK + Mean: 1 / kk at the places < kk = min(K, cnt)
// Two forms, as for the ragged reducer (kernels_basic.hip):
//   k_explain_thread  one thread per explained pair; every pair of the batch has at most RAGGED_THREAD_MAX paths.  m and the sum are formed in reduce_col's order.
//   k_explain_wave    one 64-lane wave per explained pair, four to a workgroup.  A pair of at most RAGGED_THREAD_MAX paths is still done by one lane in the
//                     thread form's order (same bits in either launch); a longer one by the wave: lanes stride the segment, m / sum / every selection
//                     finish with a __shfl_xor butterfly (every lane ends with the same bits).
// pooled / prob come from reduce_col / reduce_col_wave (reduce_dev.h) chosen as the batch's pooling kernel chooses them, then sigmoidf_: the bits of a scoring pass.
// The pair list is device memory: the caller's pairs, or (goff != null) the top-K rows the ranking kernel wrote: item i = place i % per_group of group i / per_group.
#include "kprn_internal.h"
#include "reduce_dev.h"

#include <cmath>
#include <cstring>

namespace ex {

// (v, p) comes after the exclusion bound (lv, li) in the order
__host__ __device__ static inline bool after(float v, int p, float lv, int li) {
  if (lv != lv) return v != v && p > li;
  return v != v || v < lv || (v == lv && p > li);
}
// (v, p) comes before the candidate (b, bi); bi < 0 = no candidate yet
__host__ __device__ static inline bool before(float v, int p, float b, int bi) {
  if (bi < 0) return true;
  if (v != v) return b != b && p < bi;
  if (b != b) return true;
  return v > b || (v == b && p < bi);
}
// the first path behind the bound among p0, p0 + step, ...
__host__ __device__ static inline void next_best(const float* __restrict__ s, int cnt, int C, int p0, int step, float lv, int li, float& best, int& bi) {
  best = -INFINITY; bi = -1;
  for (int p = p0; p < cnt; p += step) {
    const float v = s[(int64_t)p * C];
    if (after(v, p, lv, li) && before(v, p, best, bi)) { best = v; bi = p; }
  }
}
__host__ __device__ static inline float place_weight(int reducer, int kk, int place, float v, float m, float sum, float ig) {
  if (reducer == 2) return lse_term(v, m, ig) / sum;
  if (reducer == 0) return place == 0 ? 1.f : 0.f;
  return place < kk ? 1.f / (float)kk : 0.f;
}
__host__ __device__ static inline void empty_place(int32_t* idx, float* score, float* weight, int r) { idx[r] = -1; score[r] = 0.f; weight[r] = 0.f; }

// m and sum of the LogSumExp weights in reduce_col's order (cnt <= RAGGED_THREAD_MAX on the device)
__host__ __device__ static inline void lse_serial(const float* __restrict__ s, int cnt, int C, float ig, float& m, float& sum) {
  m = s[0];
  for (int p = 1; p < cnt; ++p) m = fmaxf(m, s[(int64_t)p * C]);
  sum = 0.f;
  for (int p = 0; p < cnt; ++p) sum += lse_term(s[(int64_t)p * C], m, ig);
}
// the M places of one pair by one thread (m, sum: LogSumExp only)
__host__ __device__ static inline void places_serial(const float* __restrict__ s, int cnt, int C, int reducer, int K, int M, float m, float sum, float ig,
                                                     int32_t* idx, float* score, float* weight) {
  const int kk = K < cnt ? K : cnt;
  float lv = INFINITY;
  int li = -1;
  for (int r = 0; r < M; ++r) {
    if (r >= cnt) { empty_place(idx, score, weight, r); continue; }
    float best; int bi;
    next_best(s, cnt, C, 0, 1, lv, li, best, bi);
    idx[r] = bi; score[r] = best; weight[r] = place_weight(reducer, kk, r, best, m, sum, ig);
    lv = best; li = bi;
  }
}

__device__ static inline int pair_of(const Args& a, int64_t i) {
  int p = a.pairs ? a.pairs[i] : (int)i;
  if (a.goff) p = p < 0 ? -1 : (int)a.goff[i / a.per_group] + p;
  return p;
}
__device__ static inline void emit_pooled(const Args& a, int64_t i, float y) {
  if (a.pooled) a.pooled[i] = y;
  if (a.prob) a.prob[i] = pool_sigmoid_of(y, a.ig);
}
__device__ static inline void pair_serial(const Args& a, int64_t i, const float* __restrict__ s, int cnt) {
  float m = 0.f, sum = 1.f;
  if (a.reducer == 2) lse_serial(s, cnt, a.C, a.ig, m, sum);
  places_serial(s, cnt, a.C, a.reducer, a.K, a.M, m, sum, a.ig, a.idx + i * a.M, a.score + i * a.M, a.weight + i * a.M);
  if (a.pooled || a.prob) emit_pooled(a, i, reduce_col(s, cnt, a.C, a.reducer, a.K, a.ig));
}

__global__ __launch_bounds__(256) void k_explain_thread(Args a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int pair = pair_of(a, i);
  if (pair < 0) {   // (a place past the end of a ranked group)
    for (int r = 0; r < a.M; ++r) empty_place(a.idx + i * a.M, a.score + i * a.M, a.weight + i * a.M, r);
    emit_pooled(a, i, 0.f);
    return;
  }
  pair_serial(a, i, a.S + seg_begin(a.off, a.P, pair) * a.C + a.cid, seg_count(a.off, a.P, pair));
}

// the wave's first path behind the bound; every lane ends with the same (v, i)
__device__ __forceinline__ void wave_best(float& v, int& i) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const float ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    if (oi >= 0 && before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

__global__ __launch_bounds__(256) void k_explain_wave(Args a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;   // (the whole wave leaves)
  const int pair = pair_of(a, i);
  int32_t* idx = a.idx + i * a.M;
  float* score = a.score + i * a.M;
  float* weight = a.weight + i * a.M;
  if (pair < 0) {
    if (lane < a.M) empty_place(idx, score, weight, lane);
    if (lane == 0) emit_pooled(a, i, 0.f);
    return;
  }
  const int cnt = seg_count(a.off, a.P, pair);
  const float* __restrict__ s = a.S + seg_begin(a.off, a.P, pair) * a.C + a.cid;
  if (cnt <= kk::RAGGED_THREAD_MAX) {
    if (lane == 0) pair_serial(a, i, s, cnt);
    return;
  }
  const int C = a.C;
  float m = 0.f, sum = 1.f;
  if (a.reducer == 2) {
    m = -INFINITY;
    for (int p = lane; p < cnt; p += 64) m = fmaxf(m, s[(int64_t)p * C]);
    m = wave_all_max(m);
    sum = 0.f;
    for (int p = lane; p < cnt; p += 64) sum += lse_term(s[(int64_t)p * C], m, a.ig);
    sum = wave_all_sum(sum);
  }
  const int kk = a.K < cnt ? a.K : cnt;
  float lv = INFINITY;
  int li = -1;
  for (int r = 0; r < a.M; ++r) {
    if (r >= cnt) {
      if (lane == 0) empty_place(idx, score, weight, r);
      continue;
    }
    float best; int bi;
    next_best(s, cnt, C, lane, 64, lv, li, best, bi);
    wave_best(best, bi);
    if (lane == 0) { idx[r] = bi; score[r] = best; weight[r] = place_weight(a.reducer, kk, r, best, m, sum, a.ig); }
    lv = best; li = bi;
  }
  if (a.pooled || a.prob) {   // (a rectangular batch pools every pair in reduce_col's order, whatever its P: k_pool<false, ..>)
    const float y = a.seg_wave ? reduce_col_wave(s, cnt, C, a.reducer, a.K, a.ig, lane) : reduce_col(s, cnt, C, a.reducer, a.K, a.ig);
    if (lane == 0) emit_pooled(a, i, y);
  }
}

int validate(int32_t B, const int32_t* pairs, int64_t n, int32_t M, std::string* why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (M < 1 || M > KPRN_EXPLAIN_MAX_M) return bad(KPRN_E_ARG, "M must be in 1..32");
  if (B < 1 || n < 1) return bad(KPRN_E_ARG, "no pairs to explain");
  if (!pairs) return n == B ? KPRN_OK : bad(KPRN_E_ARG, "pairs is NULL (= every pair): n_pairs must be the batch's pair count");
  for (int64_t i = 0; i < n; ++i)
    if (pairs[i] < 0 || pairs[i] >= B) return bad(KPRN_E_INDEX, "a pair is outside 0..B-1");
  return KPRN_OK;
}

void launch(hipStream_t s, const Args& a, int max_cnt) {
  if (max_cnt <= kk::RAGGED_THREAD_MAX) hipLaunchKernelGGL(k_explain_thread, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_explain_wave, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
}

}  // namespace ex

// The host twin.  A pair of more than RAGGED_THREAD_MAX paths sums its exponentials the way the wave does (64 strided partial sums, then the butterfly's
// tree), so that the same error bound holds for both; the selection is the shared rule.  gamma: the pooling temperature with the refusals of option
// "pool_gamma" (include/kprn.h "pooling temperature"); the exponents and the pooled value are formed by reduce_dev.h's lse_term / lse_finish / pool_sigmoid_of, as on the
// device: under a temperature their exp and log are exp_shared / log_shared, plain fp32 arithmetic that gives the kernels' bits on the host.
extern "C" int kprn_host_explain_gamma(const float* path_scores, const int32_t* offsets, int32_t B, int32_t C, int32_t class_id, int32_t reducer,
                                       int32_t K_reducer, const int32_t* pairs, int32_t n_pairs, int32_t M, int32_t* path_idx, float* path_score,
                                       float* path_weight, float* pooled, float* probs, float gamma) {
  if (!path_scores || !offsets || !path_idx || !path_score || !path_weight) return KPRN_E_ARG;
  if (C < 1 || class_id < 1 || class_id > C || reducer < 0 || reducer > 2 || (reducer == 1 && K_reducer < 1)) return KPRN_E_ARG;
  if (!kk::pool_gamma_ok((double)gamma)) return KPRN_E_ARG;
  if (gamma != 1.0f && reducer != 2) return KPRN_E_UNSUPPORTED;
  const float ig = kk::pool_ig_of(gamma);
  const int rc = ex::validate(B, pairs, n_pairs, M, nullptr);
  if (rc != KPRN_OK) return rc;
  if (offsets[0] < 0) return KPRN_E_ARG;
  for (int32_t b = 0; b < B; ++b) {
    const int64_t c = (int64_t)offsets[b + 1] - offsets[b];
    if (c < 1 || c > kk::RAGGED_MAX_SEG) return KPRN_E_ARG;
  }
  for (int32_t i = 0; i < n_pairs; ++i) {
    const int b = pairs ? pairs[i] : i;
    const int cnt = offsets[b + 1] - offsets[b];
    const float* s = path_scores + (int64_t)offsets[b] * C + (class_id - 1);
    float m = 0.f, sum = 1.f;
    if (reducer == 2) {
      if (cnt <= kk::RAGGED_THREAD_MAX) ex::lse_serial(s, cnt, C, ig, m, sum);
      else {
        m = -INFINITY;
        for (int p = 0; p < cnt; ++p) m = fmaxf(m, s[(int64_t)p * C]);
        float lanes[64];
        for (int l = 0; l < 64; ++l) {
          float a = 0.f;
          for (int p = l; p < cnt; p += 64) a += lse_term(s[(int64_t)p * C], m, ig);
          lanes[l] = a;
        }
        for (int w = 32; w > 0; w >>= 1)
          for (int l = 0; l < w; ++l) lanes[l] += lanes[l + w];   // (lane 0's operands in the butterfly, level by level)
        sum = lanes[0];
      }
    }
    ex::places_serial(s, cnt, C, reducer, K_reducer, M, m, sum, ig, path_idx + (int64_t)i * M, path_score + (int64_t)i * M, path_weight + (int64_t)i * M);
    if (pooled || probs) {
      float y;
      if (reducer == 2) y = lse_finish(sum, m, ig);
      else {
        const int kk = reducer == 0 ? 1 : (K_reducer < cnt ? K_reducer : cnt);
        float acc = 0.f, lv = INFINITY;
        int li = -1;
        for (int q = 0; q < kk; ++q) {
          float best; int bi;
          ex::next_best(s, cnt, C, 0, 1, lv, li, best, bi);
          acc += best; lv = best; li = bi;
        }
        y = reducer == 0 ? acc : acc / (float)kk;
      }
      if (pooled) pooled[i] = y;
      if (probs) probs[i] = pool_sigmoid_of(y, ig);
    }
  }
  return KPRN_OK;
}

extern "C" int kprn_host_explain(const float* path_scores, const int32_t* offsets, int32_t B, int32_t C, int32_t class_id, int32_t reducer, int32_t K_reducer,
                                 const int32_t* pairs, int32_t n_pairs, int32_t M, int32_t* path_idx, float* path_score, float* path_weight, float* pooled,
                                 float* probs) {
  return kprn_host_explain_gamma(path_scores, offsets, B, C, class_id, reducer, K_reducer, pairs, n_pairs, M, path_idx, path_score, path_weight, pooled, probs, 1.0f);
}
