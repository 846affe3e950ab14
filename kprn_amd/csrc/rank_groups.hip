// Ranking stage (include/kprn.h "ranking"): groups of candidate scores -> rank of the positive, top-K list, rank histogram, under the rule of the
// reference's evaluation chain (eval/combine_result.py, eval_score.py: printed "%.5f" scores, first seen wins a tie, an all-zero group is a miss).
//
// One definition of the order serves the device kernels and the host twin (rk::composite): every member gets ONE unique 64-bit integer
//   (key << 12) | (4095 - index)      key = 0 for an invalid member, else 1 + the "%.5f" integer (mode 0) or 1.. from the fp32 order (mode 1)
// and a member's place is the number of members with a larger integer.  The kernels find it by COUNTING: the group's integers are staged in LDS once, every
// lane holds a few members and compares them with each staged integer (a wave-uniform LDS read: a broadcast, no bank conflict).  O(n^2 / lanes) per group:
//   k_rank_wave   n <= 256: one 64-lane wave per group, 4 groups per 256-thread workgroup (1, 2 or 4 members per lane; the 101-candidate evaluation is 2)
//   k_rank_block  n <= 4096: one 256-thread workgroup per group, 32 KB of LDS; below Args::sort_min members by counting (2 .. 16 members per thread), from
//                 there on by a bitonic sort of the staged integers in LDS, place = position (option "rank_sort_min", default 512: counting is faster at
//                 257 members, the sort from 512 on and 9 x at 4096; profiles/rank/README.md, comparison 3)
// Both are launched over all groups and leave the groups of the other size class alone.  Histogram counters are int64 in global memory, bumped with one
// integer atomicAdd per group: the sums do not depend on the order of arrival.
#include "kprn_internal.h"
#include "rank_key.h"   // rk::key_of / composite / printed_positive: the order, shared with select_hardest.hip

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rk {

__device__ static inline int64_t line_of(const Args& a, int64_t o, int i) { return a.members ? a.members[o + i] : o + i; }

// the group's integers -> LDS; returns this thread's invalid members, sets *any when one of its members prints above zero
template <int NT>
__device__ static inline int stage(const Args& a, int64_t o, int n, int tid, uint64_t* keys, bool* any) {
  int inv = 0;
  for (int i = tid; i < n; i += NT) {
    const uint64_t c = composite(a.scores[line_of(a, o, i)], i, a.mode);
    keys[i] = c;
    inv += (c >> 12) == 0u;
    *any = *any || printed_positive(c);
  }
  return inv;
}

// places by counting; winners write the top-K row, the positive's holder the rank and the histogram
template <int NT, int MPL>
__device__ static inline void count_emit(const Args& a, int g, int64_t o, int n, int tid, const uint64_t* keys, bool zero_group) {
  uint64_t mine[MPL];
  int cnt[MPL];
#pragma unroll
  for (int r = 0; r < MPL; ++r) {
    const int i = tid + NT * r;
    mine[r] = i < n ? keys[i] : ~0ull;
    cnt[r] = 0;
  }
  for (int j = 0; j < n; ++j) {
    const uint64_t cj = keys[j];   // (wave-uniform address)
#pragma unroll
    for (int r = 0; r < MPL; ++r) cnt[r] += cj > mine[r];
  }
  const int p = a.pos ? a.pos[g] : 0;
#pragma unroll
  for (int r = 0; r < MPL; ++r) {
    const int i = tid + NT * r;
    if (i >= n) continue;
    if (a.tk_idx && cnt[r] < a.K) {
      a.tk_idx[(int64_t)g * a.K + cnt[r]] = i;
      a.tk_score[(int64_t)g * a.K + cnt[r]] = a.scores[line_of(a, o, i)];
    }
    if (i == p) {
      const int rank = zero_group ? KPRN_RANK_ZERO_GROUP : cnt[r];
      if (a.ranks) a.ranks[g] = rank;
      if (a.hist) atomicAdd(a.hist + (rank < 0 ? a.hist_len + 1 : (rank < a.hist_len ? rank : a.hist_len)), 1ull);
    }
  }
  if (a.tk_idx)
    for (int s = n + tid; s < a.K; s += NT) { a.tk_idx[(int64_t)g * a.K + s] = -1; a.tk_score[(int64_t)g * a.K + s] = 0.f; }
  if (p < 0 && tid == 0) {
    if (a.ranks) a.ranks[g] = KPRN_RANK_NO_POSITIVE;
    if (a.hist) atomicAdd(a.hist + a.hist_len + 2, 1ull);
  }
}

// large groups: the staged integers are sorted in LDS (bitonic, descending, padded with 0 to a power of two: every member's integer is >= 1 unless the group
// has all 4096 members, and then nothing is padded); place = position.  O(n log^2 n / 256) per thread against O(n^2 / 256) for counting.
__device__ static inline void sort_emit(const Args& a, int g, int64_t o, int n, int tid, uint64_t* keys, bool zero_group) {
  int np2 = 512;
  while (np2 < n) np2 <<= 1;
  for (int i = n + tid; i < np2; i += 256) keys[i] = 0ull;
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (np2 >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t x = keys[i], y = keys[l];
        if ((x < y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
      }
      __syncthreads();
    }
  const int p = a.pos ? a.pos[g] : 0;
  if (a.tk_idx)
    for (int s = tid; s < a.K; s += 256) {
      const int i = s < n ? 4095 - (int)(keys[s] & 4095ull) : -1;
      a.tk_idx[(int64_t)g * a.K + s] = i;
      a.tk_score[(int64_t)g * a.K + s] = i < 0 ? 0.f : a.scores[line_of(a, o, i)];
    }
  if (p >= 0) {
    for (int s = tid; s < n; s += 256)
      if ((int)(keys[s] & 4095ull) == 4095 - p) {
        const int rank = zero_group ? KPRN_RANK_ZERO_GROUP : s;
        if (a.ranks) a.ranks[g] = rank;
        if (a.hist) atomicAdd(a.hist + (rank < 0 ? a.hist_len + 1 : (rank < a.hist_len ? rank : a.hist_len)), 1ull);
      }
  } else if (tid == 0) {
    if (a.ranks) a.ranks[g] = KPRN_RANK_NO_POSITIVE;
    if (a.hist) atomicAdd(a.hist + a.hist_len + 2, 1ull);
  }
}

constexpr int WAVE_MAX = 256;   // longest group a single wave ranks (4 members per lane)

__global__ __launch_bounds__(256) void k_rank_wave(Args a) {
  __shared__ uint64_t keys[4][WAVE_MAX];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t gl = (int64_t)blockIdx.x * 4 + wave;
  const int g = (int)gl;
  int n = 0;
  int64_t o = 0;
  if (gl < a.G) {
    o = a.goff[g];
    n = (int)(a.goff[g + 1] - o);
    if (n > WAVE_MAX) n = 0;   // (k_rank_block's)
  }
  bool any = false;
  const int inv = stage<64>(a, o, n, lane, keys[wave], &any);
  __syncthreads();   // (every wave of the workgroup arrives, with or without a group)
  if (n == 0) return;
  int n_inv = inv;
  if (__ballot(inv > 0) != 0ull)
    for (int d = 32; d > 0; d >>= 1) n_inv += __shfl_xor(n_inv, d);
  const bool zero_group = a.mode == 0 && __ballot(any) == 0ull;
  if (n_inv && lane == 0 && a.hist) atomicAdd(a.hist + a.hist_len + 3, (unsigned long long)n_inv);
  if (n <= 64) count_emit<64, 1>(a, g, o, n, lane, keys[wave], zero_group);
  else if (n <= 128) count_emit<64, 2>(a, g, o, n, lane, keys[wave], zero_group);
  else count_emit<64, 4>(a, g, o, n, lane, keys[wave], zero_group);
}

__global__ __launch_bounds__(256) void k_rank_block(Args a) {
  __shared__ uint64_t keys[4096];
  __shared__ int red[2];   // {invalid members, a member prints above zero}
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t o = a.goff[g];
  const int n = (int)(a.goff[g + 1] - o);
  if (n <= WAVE_MAX) return;   // (k_rank_wave's; the whole workgroup leaves)
  if (tid < 2) red[tid] = 0;
  __syncthreads();
  bool any = false;
  const int inv = stage<256>(a, o, n, tid, keys, &any);
  if (inv) atomicAdd(&red[0], inv);
  if (any) red[1] = 1;
  __syncthreads();
  const bool zero_group = a.mode == 0 && red[1] == 0;
  if (tid == 0 && red[0] && a.hist) atomicAdd(a.hist + a.hist_len + 3, (unsigned long long)red[0]);
  if (n >= a.sort_min) sort_emit(a, g, o, n, tid, keys, zero_group);   // (uniform over the workgroup)
  else if (n <= 512) count_emit<256, 2>(a, g, o, n, tid, keys, zero_group);
  else if (n <= 1024) count_emit<256, 4>(a, g, o, n, tid, keys, zero_group);
  else if (n <= 2048) count_emit<256, 8>(a, g, o, n, tid, keys, zero_group);
  else count_emit<256, 16>(a, g, o, n, tid, keys, zero_group);
}

// the refusals both entry points share; *max_n = longest group
int validate(int64_t n_scores, const int64_t* members, const int64_t* goff, const int32_t* pos, int32_t G, int32_t mode, int32_t K, int32_t hist_len,
             int* max_n, std::string* why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (!goff || G < 1) return bad(KPRN_E_ARG, "group_offsets is NULL or G < 1");
  if (mode != KPRN_RANK_PRINTED && mode != KPRN_RANK_RAW) return bad(KPRN_E_ARG, "mode must be KPRN_RANK_PRINTED or KPRN_RANK_RAW");
  if (K < 1 || K > KPRN_RANK_MAX_K) return bad(KPRN_E_ARG, "K must be in 1..64");
  if (hist_len < 1 || hist_len > KPRN_RANK_MAX_GROUP) return bad(KPRN_E_ARG, "hist_len must be in 1..4096");
  const char* text = "";
  const int rc = validate_groups(n_scores, members, goff, pos, G, max_n, &text);   // (rank_key.h: the groups, pos and the members)
  return rc == KPRN_OK ? rc : bad(rc, text);
}

void launch(hipStream_t s, const Args& a, int max_n) {
  hipLaunchKernelGGL(k_rank_wave, dim3((a.G + 3) / 4), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  if (max_n > WAVE_MAX) {
    hipLaunchKernelGGL(k_rank_block, dim3(a.G), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
  }
}

}  // namespace rk

extern "C" int kprn_host_rank_groups(const float* scores, int64_t n_scores, const int64_t* members, const int64_t* group_offsets, const int32_t* pos, int32_t G,
                                     int32_t mode, int32_t K, int32_t* ranks, int32_t* topk_idx, float* topk_score, int64_t* hist, int32_t hist_len) {
  if (!scores || n_scores < 0) return KPRN_E_ARG;
  if ((topk_idx == nullptr) != (topk_score == nullptr)) return KPRN_E_ARG;
  const int rc = rk::validate(n_scores, members, group_offsets, pos, G, mode, K, hist_len, nullptr, nullptr);
  if (rc != KPRN_OK) return rc;
  if (hist) memset(hist, 0, (size_t)(hist_len + 4) * sizeof(int64_t));
  std::vector<uint64_t> c;
  for (int32_t g = 0; g < G; ++g) {
    const int64_t o = group_offsets[g];
    const int n = (int)(group_offsets[g + 1] - o);
    auto line = [&](int i) { return members ? members[o + i] : o + i; };
    const int p = pos ? pos[g] : 0;
    c.resize(n);
    bool any = false;
    int64_t inv = 0;
    uint64_t cp = 0;
    for (int i = 0; i < n; ++i) {
      c[i] = rk::composite(scores[line(i)], i, mode);
      inv += (c[i] >> 12) == 0u;
      any = any || rk::printed_positive(c[i]);
      if (i == p) cp = c[i];
    }
    if (hist) hist[hist_len + 3] += inv;
    int rank = KPRN_RANK_NO_POSITIVE;
    if (p >= 0) {
      rank = 0;
      for (int i = 0; i < n; ++i) rank += c[i] > cp;
      if (mode == KPRN_RANK_PRINTED && !any) rank = KPRN_RANK_ZERO_GROUP;
    }
    if (ranks) ranks[g] = rank;
    if (hist) hist[p < 0 ? hist_len + 2 : (rank < 0 ? hist_len + 1 : (rank < hist_len ? rank : hist_len))] += 1;
    if (topk_idx) {
      const int k = std::min<int>(K, n);
      std::partial_sort(c.begin(), c.begin() + k, c.end(), std::greater<uint64_t>());
      for (int s = 0; s < K; ++s) {
        const int i = s < k ? 4095 - (int)(c[s] & 4095u) : -1;
        topk_idx[(int64_t)g * K + s] = i;
        topk_score[(int64_t)g * K + s] = i < 0 ? 0.f : scores[line(i)];
      }
    }
  }
  return KPRN_OK;
}
