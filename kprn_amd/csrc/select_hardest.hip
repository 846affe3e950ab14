// Hard negatives, the selection (include/kprn.h "hard negatives"): groups of board scores -> a keep mask over their members: each group's positive and the
// n_keep non-positive members that score highest under the RAW order of the ranking stage.  The rule, its refusals and the host twin are select_hardest.h's;
// the order is rank_key.h's rk::composite, the one rank_groups.hip ranks by.
//
// ONE launch serves every group size.  The host cuts the groups into workgroups (sh::plan): up to four consecutive groups of at most 256 members go to one
// 256-thread workgroup, a 64-lane wave each (1, 2 or 4 members per lane); a longer group (up to 4096 members) has a workgroup to itself (2 .. 16 members per
// thread).  Either way the group's staged integers go to LDS once and every thread compares its members with each of them (a wave-uniform LDS read: a
// broadcast, no bank conflict) -- places by COUNTING, as k_rank_wave and k_rank_block form them; O(n^2 / lanes) per group.  The positive's staged integer is 0:
// it is never counted.  Every member's byte of the mask is written by the one thread that owns the member: no atomics but the integer add of the invalid
// count, so nothing depends on timing.
#include "kprn_internal.h"
#include "select_hardest.h"

namespace sh {

struct Args {   // device pointers; members / pos / n_invalid may be null
  const float* scores; const int64_t* members; const int64_t* goff; const int32_t* pos; const int32_t* wg;
  int64_t base;   // goff[0]: members and keep are the slices from there on
  int n_keep;
  unsigned char* keep; unsigned long long* n_invalid;
};

// the group's staged integers -> LDS; returns this thread's invalid non-positive members
template <int NT>
__device__ static inline int stage(const Args& a, int64_t o, int n, int p, int tid, uint64_t* keys) {
  int inv = 0;
  for (int i = tid; i < n; i += NT) {
    const uint64_t c = staged(a.scores[a.members ? a.members[o - a.base + i] : o + i], i, p);
    keys[i] = c;
    inv += invalid(c, i, p);
  }
  return inv;
}

template <int NT, int MPL>
__device__ static inline void count_emit(const Args& a, int64_t o, int n, int p, int tid, const uint64_t* keys) {
  uint64_t mine[MPL];
  int cnt[MPL];
#pragma unroll
  for (int r = 0; r < MPL; ++r) {
    const int i = tid + NT * r;
    mine[r] = i < n ? keys[i] : ~0ull;
    cnt[r] = 0;
  }
  count_above<MPL>(keys, n, mine, cnt);
#pragma unroll
  for (int r = 0; r < MPL; ++r) {
    const int i = tid + NT * r;
    if (i < n) a.keep[o - a.base + i] = kept(i, p, cnt[r], a.n_keep) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_select_hardest(Args a) {
  __shared__ uint64_t keys[KPRN_RANK_MAX_GROUP];   // a long group's integers, or WG_GROUPS x WAVE_MAX: a wave's group each
  __shared__ int red;                              // a long group's invalid members
  const int tid = threadIdx.x, g0 = a.wg[blockIdx.x], g1 = a.wg[blockIdx.x + 1];
  if (g1 - g0 == 1 && a.goff[g0 + 1] - a.goff[g0] > WAVE_MAX) {   // (uniform over the workgroup)
    const int64_t o = a.goff[g0];
    const int n = (int)(a.goff[g0 + 1] - o), p = a.pos ? a.pos[g0] : -1;
    if (tid == 0) red = 0;
    __syncthreads();
    const int inv = stage<256>(a, o, n, p, tid, keys);
    if (inv) atomicAdd(&red, inv);
    __syncthreads();
    if (tid == 0 && red && a.n_invalid) atomicAdd(a.n_invalid, (unsigned long long)red);
    if (n <= 512) count_emit<256, 2>(a, o, n, p, tid, keys);
    else if (n <= 1024) count_emit<256, 4>(a, o, n, p, tid, keys);
    else if (n <= 2048) count_emit<256, 8>(a, o, n, p, tid, keys);
    else count_emit<256, 16>(a, o, n, p, tid, keys);
    return;
  }
  const int wave = tid >> 6, lane = tid & 63, g = g0 + wave;
  int n = 0, p = -1;
  int64_t o = 0;
  if (g < g1) {
    o = a.goff[g];
    n = (int)(a.goff[g + 1] - o);
    p = a.pos ? a.pos[g] : -1;
  }
  uint64_t* mykeys = keys + wave * WAVE_MAX;
  const int inv = stage<64>(a, o, n, p, lane, mykeys);
  __syncthreads();   // (every wave of the workgroup arrives, with or without a group)
  if (n == 0) return;
  int n_inv = inv;
  if (__ballot(inv > 0) != 0ull)
    for (int d = 32; d > 0; d >>= 1) n_inv += __shfl_xor(n_inv, d);
  if (n_inv && lane == 0 && a.n_invalid) atomicAdd(a.n_invalid, (unsigned long long)n_inv);
  if (n <= 64) count_emit<64, 1>(a, o, n, p, lane, mykeys);
  else if (n <= 128) count_emit<64, 2>(a, o, n, p, lane, mykeys);
  else count_emit<64, 4>(a, o, n, p, lane, mykeys);
}

}  // namespace sh

extern "C" {

// arguments up into the ranking stage's call block, ONE launch, results down, one wait
int kprn_select_hardest(kprn_handle* h, const int64_t* members, const int64_t* group_offsets, const int32_t* pos, int32_t G, int32_t n_keep, unsigned char* keep,
                        int64_t* n_invalid) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->board, KPRN_E_ARG, "no board: call kprn_board_reserve first");
  KPRN_REQUIRE(keep, KPRN_E_ARG, "keep is NULL");
  const char* why = "";
  const int rc = sh::validate(h->board_n, members, group_offsets, pos, G, n_keep, nullptr, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  score::join_put(h);
  std::vector<int32_t> wg;
  sh::plan(group_offsets, G, &wg);
  const int n_wg = (int)wg.size() - 1;
  const int64_t m0 = group_offsets[0], M = group_offsets[G] - m0;
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t o_goff = 0, o_mem = o_goff + up((size_t)(G + 1) * 8), o_inv = o_mem + up(members ? (size_t)M * 8 : 0), o_pos = o_inv + 16,
               o_wg = o_pos + up(pos ? (size_t)G * 4 : 0), o_keep = o_wg + up((size_t)(n_wg + 1) * 4), total = o_keep + up((size_t)M);
  hipStream_t s = h->stream;
  char* base = (char*)grow_call_block(s, h->rank_buf, h->rank_buf_bytes, total);
  HIP_TRY(hipMemcpyAsync(base + o_goff, group_offsets, (size_t)(G + 1) * 8, hipMemcpyHostToDevice, s));
  if (members) HIP_TRY(hipMemcpyAsync(base + o_mem, members + m0, (size_t)M * 8, hipMemcpyHostToDevice, s));
  if (pos) HIP_TRY(hipMemcpyAsync(base + o_pos, pos, (size_t)G * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(base + o_wg, wg.data(), (size_t)(n_wg + 1) * 4, hipMemcpyHostToDevice, s));
  if (n_invalid) HIP_TRY(hipMemsetAsync(base + o_inv, 0, 8, s));
  sh::Args a;
  a.scores = h->board; a.members = members ? (const int64_t*)(base + o_mem) : nullptr; a.goff = (const int64_t*)(base + o_goff);
  a.pos = pos ? (const int32_t*)(base + o_pos) : nullptr; a.wg = (const int32_t*)(base + o_wg);
  a.base = m0; a.n_keep = n_keep;
  a.keep = (unsigned char*)(base + o_keep); a.n_invalid = n_invalid ? (unsigned long long*)(base + o_inv) : nullptr;
  {
    ProfScope ps(h, "select_hardest");
    hipLaunchKernelGGL(sh::k_select_hardest, dim3((unsigned)n_wg), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
  }
  // (into buffers of the call's own: a failed wait leaves the caller's arrays untouched)
  std::vector<unsigned char> got((size_t)M);
  int64_t inv = 0;
  HIP_TRY(hipMemcpyAsync(got.data(), base + o_keep, (size_t)M, hipMemcpyDeviceToHost, s));
  if (n_invalid) HIP_TRY(hipMemcpyAsync(&inv, base + o_inv, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));   // (also covers wg, the source of a pageable copy)
  memcpy(keep + m0, got.data(), (size_t)M);
  if (n_invalid) *n_invalid = inv;
  prof_drain(h);
  API_END(h)
}

int kprn_host_select_hardest(const float* scores, int64_t n_scores, const int64_t* members, const int64_t* group_offsets, const int32_t* pos, int32_t G,
                             int32_t n_keep, unsigned char* keep, int64_t* n_invalid) {
  try {
    return sh::host_select(scores, n_scores, members, group_offsets, pos, G, n_keep, keep, n_invalid);
  } catch (...) { return KPRN_E_NOMEM; }
}

}  // extern "C"
