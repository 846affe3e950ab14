// Ranking targets in groups of any size (include/kprn.h): what the device kernel (rank_targets.hip) and the host twin share, in plain C++ so that the twin
// also compiles without the HIP headers (tests/rank_targets_san_main.cpp builds it into a stand-alone program under the host sanitizers).
//
// The order is rank_groups.hip's -- key descending, first seen first -- with the member index in 32 bits instead of 12:
//   (key << 32) | (0xFFFFFFFF - index)      key = rk::key_of's: 0 for an invalid member, else 1 + the "%.5f" integer (mode 0) or 1.. from the fp32 order (mode 1)
// key_of is restated here (rk::key_of lives in rank_key.h; this file keeps its own copy, written when rank_groups.hip held rk's as a file-local);
// tests/test_rank_targets_host.py holds the two equal through every score class (the single-target cases must give kprn_host_rank_groups' ranks).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/kprn.h"

#if defined(__HIPCC__)
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

namespace rt {

RT_HD static inline uint32_t key_of(float p, int mode) {
  if (mode == 0) {
    if (!(p >= 0.f && p <= 1.f)) return 0u;   // (NaN included)
    return 1u + (uint32_t)(int32_t)rint((double)p * 1e5);
  }
  if (p != p) return 0u;
  if (p == 0.f) p = 0.f;   // (-0 and +0 are one value)
  uint32_t u;
  memcpy(&u, &p, 4);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // fp32 order -> unsigned order; -inf -> 0x007fffff, never 0
  return u;
}
// never 0: index < 2^31, so the low word is >= 0x80000000 (the sort pads with 0)
RT_HD static inline uint64_t composite(float p, int64_t i, int mode) { return ((uint64_t)key_of(p, mode) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i); }
RT_HD static inline bool invalid(uint64_t c) { return (c >> 32) == 0u; }
// mode 0: a member whose printed score is above zero (key >= 2)
RT_HD static inline bool printed_positive(uint64_t c) { return (c >> 32) >= 2u; }
RT_HD static inline int64_t hist_slot(int32_t place, int32_t hist_len) { return place < 0 ? hist_len + 1 : (place < hist_len ? place : hist_len); }

// the refusals both entry points share, on host arrays: KPRN_OK, or the status with its text in *why
static inline int validate(int64_t n_scores, const int64_t* members, const int64_t* goff, const int64_t* toff, const int32_t* targets, int32_t G, int32_t mode,
                           int32_t hist_len, const char** why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (!goff || !toff || G < 1) return bad(KPRN_E_ARG, "group_offsets or target_offsets is NULL, or G < 1");
  if (mode != KPRN_RANK_PRINTED && mode != KPRN_RANK_RAW) return bad(KPRN_E_ARG, "mode must be KPRN_RANK_PRINTED or KPRN_RANK_RAW");
  if (hist_len < 1 || hist_len > KPRN_RANK_MAX_GROUP) return bad(KPRN_E_ARG, "hist_len must be in 1..4096");
  if (goff[0] < 0) return bad(KPRN_E_ARG, "group_offsets[0] < 0");
  if (toff[0] != 0) return bad(KPRN_E_ARG, "target_offsets[0] must be 0");
  for (int32_t g = 0; g < G; ++g) {
    const int64_t n = goff[g + 1] - goff[g], nt = toff[g + 1] - toff[g];
    if (n < 1 || n > 0x7fffffffll) return bad(KPRN_E_ARG, "a group must have 1..2^31-1 members");
    if (nt < 0 || nt > n) return bad(KPRN_E_ARG, "a group must have 0..n targets");
  }
  if (toff[G] < 1) return bad(KPRN_E_ARG, "no targets at all");
  if (!targets) return bad(KPRN_E_ARG, "targets is NULL");
  for (int32_t g = 0; g < G; ++g) {
    const int64_t n = goff[g + 1] - goff[g];
    for (int64_t k = toff[g]; k < toff[g + 1]; ++k)
      if (targets[k] < 0 || targets[k] >= n || (k > toff[g] && targets[k] <= targets[k - 1]))
        return bad(KPRN_E_ARG, "targets must be strictly ascending indices within their group");
  }
  if (members) {
    for (int64_t m = goff[0]; m < goff[G]; ++m)
      if (members[m] < 0 || members[m] >= n_scores) return bad(KPRN_E_INDEX, "a member is outside the scores");
  } else if (goff[G] > n_scores) return bad(KPRN_E_INDEX, "a group runs past the end of the scores");
  return KPRN_OK;
}

// the rule by sorting: a target's count of larger members (of larger targets) is its distance from the end of the sorted members (targets)
static inline int host_rank_targets(const float* scores, int64_t n_scores, const int64_t* members, const int64_t* goff, const int64_t* toff, const int32_t* targets,
                                    int32_t G, int32_t mode, int32_t* places, int64_t* hist, int32_t hist_len) {
  if (!scores || n_scores < 0 || !places || !hist) return KPRN_E_ARG;
  const int rc = validate(n_scores, members, goff, toff, targets, G, mode, hist_len, nullptr);
  if (rc != KPRN_OK) return rc;
  memset(hist, 0, (size_t)(hist_len + 4) * sizeof(int64_t));
  std::vector<uint64_t> all, tc, ts;
  for (int32_t g = 0; g < G; ++g) {
    const int64_t o = goff[g], n = goff[g + 1] - o, to = toff[g], nt = toff[g + 1] - to;
    all.resize((size_t)n);
    int64_t inv = 0, pos_all = 0, pos_t = 0;
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t c = composite(scores[members ? members[o + i] : o + i], i, mode);
      all[(size_t)i] = c;
      inv += invalid(c);
      pos_all += printed_positive(c);
    }
    hist[hist_len + 3] += inv;
    if (nt == 0) continue;
    tc.resize((size_t)nt);
    for (int64_t k = 0; k < nt; ++k) {
      tc[(size_t)k] = all[(size_t)targets[to + k]];
      pos_t += printed_positive(tc[(size_t)k]);
    }
    ts = tc;
    std::sort(all.begin(), all.end());
    std::sort(ts.begin(), ts.end());
    for (int64_t k = 0; k < nt; ++k) {
      const uint64_t c = tc[(size_t)k];
      const int64_t above = all.end() - std::upper_bound(all.begin(), all.end(), c), above_t = ts.end() - std::upper_bound(ts.begin(), ts.end(), c);
      int32_t place = (int32_t)(above - above_t);
      if (mode == KPRN_RANK_PRINTED && !printed_positive(c) && pos_all == pos_t) place = KPRN_RANK_ZERO_GROUP;   // (no non-target prints above zero either)
      places[to + k] = place;
      hist[hist_slot(place, hist_len)] += 1;
    }
  }
  return KPRN_OK;
}

}  // namespace rt
