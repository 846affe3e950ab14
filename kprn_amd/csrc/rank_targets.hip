// Ranking targets in groups of any size (include/kprn.h "ranking targets in groups of any size"): the held-out items of a user among everything the user
// reaches.  The order is the ranking stage's -- key descending, first seen first -- as one 64-bit integer per member with a 32-bit index
// (rank_targets_host.h), and a target's place is the number of NON-target members with a larger integer.
//
//   k_rank_targets   one 256-thread workgroup per group, any n < 2^31 and any nt <= n in one body.  The members are never staged: up to CHUNK = 1024 target
//                    integers are staged in LDS and sorted descending (the bitonic form of rank_groups.hip's sort_emit, with the target's ordinal riding
//                    along), then the members are STREAMED past them (coalesced loads through line_of): each member finds by binary search b = the number of
//                    staged targets >= itself and adds 1 to bucket[b]; the group's targets -- all of them, not only the staged ones -- are streamed the same
//                    way and subtract 1.  The inclusive prefix sum over the buckets at a staged target s is then
//                      (members larger than s) - (targets larger than s) = place(s),
//                    whichever chunk the larger targets are in.  A group of more than 1024 targets streams its members once per chunk.
// Two buckets never see an add: b = 0 (larger than every staged target) is counted in a register and added once per thread, and b = cnt (not larger than
// any) enters no prefix.  So a group with one target issues no LDS atomic inside the stream at all.
// The same pass counts the invalid members and the members / targets that print above zero (mode 0's zero samples).  Everything is integer adds in LDS
// and int64 adds in global memory: no result depends on the order of arrival.  LDS: 8 KB integers + 2 KB ordinals + 4 KB buckets, whatever n is.
#include "kprn_internal.h"
#include "rank_targets_host.h"

namespace rt {

constexpr int CHUNK = 1024;   // targets staged at a time
constexpr int NT = 256;       // threads of a workgroup; each owns CHUNK / NT consecutive buckets in the prefix sum
constexpr int PER = CHUNK / NT;
constexpr int LOADS = 4;      // member scores a thread has in flight in the stream

__device__ static inline int64_t line_of(const Args& a, int64_t o, int64_t i) { return a.members ? a.members[o + i] : o + i; }

// b = the number of staged integers >= c; st [np2] is sorted descending and padded with 0 (no member's integer is 0), np2 a power of two
__device__ static inline int staged_not_below(const uint64_t* st, int np2, uint64_t c) {
  int b = 0;
  for (int step = np2 >> 1; step > 0; step >>= 1)
    if (st[b + step - 1] >= c) b += step;
  return b + (st[b] >= c);   // (b <= np2 - 1 here)
}

__global__ __launch_bounds__(NT) void k_rank_targets(Args a) {
  __shared__ uint64_t st[CHUNK];
  __shared__ int bucket[CHUNK];
  __shared__ uint16_t ord[CHUNK];
  __shared__ unsigned red[3];   // {invalid members, members that print above zero, targets that print above zero}
  __shared__ int wave_sum[NT / 64];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t o = a.goff[g], n = a.goff[g + 1] - o;
  const int64_t to = a.toff[g], nt = a.toff[g + 1] - to;
  const int64_t chunks = nt ? (nt + CHUNK - 1) / CHUNK : 1;   // (a group without targets still has its invalid members counted)
  for (int64_t ch = 0; ch < chunks; ++ch) {   // every bound below is uniform over the workgroup
    const int64_t k0 = ch * CHUNK;
    const int cnt = (int)(nt - k0 < CHUNK ? nt - k0 : CHUNK);
    int np2 = 1;
    while (np2 < cnt) np2 <<= 1;
    for (int s = tid; s < np2; s += NT) {
      uint64_t c = 0ull;
      if (s < cnt) {
        const int32_t i = a.targets[to + k0 + s];
        c = composite(a.scores[line_of(a, o, i)], i, a.mode);
      }
      st[s] = c;
      ord[s] = (uint16_t)s;
      bucket[s] = 0;
    }
    if (tid < 3) red[tid] = 0u;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (np2 >> 1); t += NT) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const uint64_t x = st[i], y = st[l];
          if ((x < y) == ((i & k) == 0)) {
            st[i] = y; st[l] = x;
            const uint16_t q = ord[i]; ord[i] = ord[l]; ord[l] = q;
          }
        }
        __syncthreads();
      }
    // the members, then the targets, past the staged integers
    int top = 0;   // bucket[0]'s share of this thread
    unsigned inv = 0u, pos_all = 0u, pos_t = 0u;
    for (int64_t i0 = tid; i0 < n; i0 += LOADS * NT) {   // LOADS loads in flight per thread, each a coalesced row of the workgroup
      float p[LOADS];
#pragma unroll
      for (int r = 0; r < LOADS; ++r) {
        const int64_t i = i0 + r * NT;
        p[r] = i < n ? a.scores[line_of(a, o, i)] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < LOADS; ++r) {
        const int64_t i = i0 + r * NT;
        if (i >= n) break;
        const uint64_t c = composite(p[r], i, a.mode);
        inv += invalid(c);
        pos_all += printed_positive(c);
        const int b = cnt ? staged_not_below(st, np2, c) : 1;
        if (b == 0) ++top;
        else if (b < cnt) atomicAdd(&bucket[b], 1);
      }
    }
    for (int64_t k = tid; k < nt; k += NT) {
      const int32_t i = a.targets[to + k];
      const uint64_t c = composite(a.scores[line_of(a, o, i)], i, a.mode);
      pos_t += printed_positive(c);
      const int b = staged_not_below(st, np2, c);
      if (b == 0) --top;
      else if (b < cnt) atomicAdd(&bucket[b], -1);
    }
    if (top) atomicAdd(&bucket[0], top);
    if (inv) atomicAdd(&red[0], inv);
    if (pos_all) atomicAdd(&red[1], pos_all);
    if (pos_t) atomicAdd(&red[2], pos_t);
    __syncthreads();
    // inclusive prefix sum over the buckets: PER consecutive ones per thread, a shuffle scan in the wave, the waves' totals through LDS
    int mine[PER];
    int sum = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int s = tid * PER + r;
      sum += s < cnt ? bucket[s] : 0;
      mine[r] = sum;
    }
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = incl - sum;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    const bool others_zero = a.mode == KPRN_RANK_PRINTED && red[1] == red[2];   // no non-target member prints above zero
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int s = tid * PER + r;
      if (s >= cnt) continue;
      const int32_t place = others_zero && !printed_positive(st[s]) ? KPRN_RANK_ZERO_GROUP : before + mine[r];
      a.places[to + k0 + ord[s]] = place;
      atomicAdd(a.hist + hist_slot(place, a.hist_len), 1ull);
    }
    if (ch == 0 && tid == 0 && red[0]) atomicAdd(a.hist + a.hist_len + 3, (unsigned long long)red[0]);
    __syncthreads();   // (the next chunk restages st / ord / bucket / red)
  }
}

void launch(hipStream_t s, const Args& a) {
  hipLaunchKernelGGL(k_rank_targets, dim3(a.G), dim3(NT), 0, s, a);
  HIP_TRY(hipGetLastError());
}

}  // namespace rt

extern "C" int kprn_host_rank_targets(const float* scores, int64_t n_scores, const int64_t* members, const int64_t* group_offsets, const int64_t* target_offsets,
                                      const int32_t* targets, int32_t G, int32_t mode, int32_t* places, int64_t* hist, int32_t hist_len) {
  return rt::host_rank_targets(scores, n_scores, members, group_offsets, target_offsets, targets, G, mode, places, hist, hist_len);
}
