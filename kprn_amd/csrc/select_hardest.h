// Hard negatives (include/kprn.h "hard negatives"): which members of a board group to keep -- the positive and the n_keep non-positive members that score
// highest.  What the device kernel (select_hardest.hip) and the host twin share, in plain C++ so that the twin also compiles without the HIP headers.
//
// The order is the RAW order of "ranking" and nothing else: rk::composite(score, index, KPRN_RANK_RAW) from rank_key.h.  The positive is EXCLUDED from the
// counting: its staged integer is 0, and 0 is larger than nothing, so no member ever counts it -- it is not subtracted afterwards (its own integer may tie
// nothing and still sit above or below the cut).  Every other member's place is the number of staged integers larger than its own; it is kept iff that
// number is below n_keep.  Kernel and twin form the places with the same count_above over the same staged integers.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/kprn.h"
#include "rank_key.h"

namespace sh {

constexpr int MAX_KEEP = 256;   // n_keep's upper end: the negative sampler's n_neg limit
constexpr int WAVE_MAX = 256;   // longest group a single wave selects in (4 members per lane)
constexpr int WG_GROUPS = 4;    // groups of at most WAVE_MAX members per 256-thread workgroup, one per wave

RK_HD static inline uint64_t staged(float score, int i, int pos) { return i == pos ? 0ull : rk::composite(score, i, KPRN_RANK_RAW); }
// an invalid NON-positive member (NaN: a board entry nothing wrote)
RK_HD static inline bool invalid(uint64_t staged_key, int i, int pos) { return i != pos && (staged_key >> 12) == 0u; }
// cnt[r] += the staged integers larger than mine[r], r < MPL
template <int MPL>
RK_HD static inline void count_above(const uint64_t* keys, int n, const uint64_t* mine, int* cnt) {
  for (int j = 0; j < n; ++j) {
    const uint64_t cj = keys[j];   // (on the device: a wave-uniform LDS address, a broadcast)
#pragma unroll
    for (int r = 0; r < MPL; ++r) cnt[r] += cj > mine[r];
  }
}
RK_HD static inline bool kept(int i, int pos, int above, int n_keep) { return i == pos || above < n_keep; }

// the refusals both entry points share, on host arrays: n_keep's range, then kprn_rank_groups' own for the groups, pos and the members; *max_n = longest group
static inline int validate(int64_t n_scores, const int64_t* members, const int64_t* goff, const int32_t* pos, int32_t G, int32_t n_keep, int* max_n,
                           const char** why) {
  if (n_keep < 1 || n_keep > MAX_KEEP) { if (why) *why = "n_keep must be in 1..256"; return KPRN_E_ARG; }
  return rk::validate_groups(n_scores, members, goff, pos, G, max_n, why);
}

// the single launch's workgroup table: wg [n_wg + 1], workgroup w owns the groups wg[w] .. wg[w + 1] - 1 -- up to WG_GROUPS consecutive groups of at most
// WAVE_MAX members (a wave each), or one longer group (the whole workgroup)
static inline void plan(const int64_t* goff, int32_t G, std::vector<int32_t>* wg) {
  wg->clear();
  wg->push_back(0);
  int run = 0;
  for (int32_t g = 0; g < G; ++g) {
    if (goff[g + 1] - goff[g] > WAVE_MAX) {
      if (run) wg->push_back(g);
      wg->push_back(g + 1);
      run = 0;
    } else {
      if (run == WG_GROUPS) { wg->push_back(g); run = 0; }
      ++run;
    }
  }
  if (run) wg->push_back(G);
}

// the rule on the host cores.  keep [goff[G]] is written in goff[0] .. goff[G] - 1 only
static inline int host_select(const float* scores, int64_t n_scores, const int64_t* members, const int64_t* goff, const int32_t* pos, int32_t G, int32_t n_keep,
                              unsigned char* keep, int64_t* n_invalid) {
  if (!scores || n_scores < 0 || !keep) return KPRN_E_ARG;
  const int rc = validate(n_scores, members, goff, pos, G, n_keep, nullptr, nullptr);
  if (rc != KPRN_OK) return rc;
  std::vector<uint64_t> c;
  int64_t inv = 0;
  for (int32_t g = 0; g < G; ++g) {
    const int64_t o = goff[g];
    const int n = (int)(goff[g + 1] - o), p = pos ? pos[g] : -1;
    c.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
      c[(size_t)i] = staged(scores[members ? members[o + i] : o + i], i, p);
      inv += invalid(c[(size_t)i], i, p);
    }
    for (int i = 0; i < n; ++i) {
      int above = 0;
      count_above<1>(c.data(), n, &c[(size_t)i], &above);
      keep[o + i] = kept(i, p, above, n_keep) ? 1 : 0;
    }
  }
  if (n_invalid) *n_invalid = inv;
  return KPRN_OK;
}

}  // namespace sh
