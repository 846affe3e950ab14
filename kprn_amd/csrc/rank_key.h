// The order of the ranking stage (include/kprn.h "ranking"), defined once for everything that ranks board groups of at most 4096 members: the kernels and the
// host twin of rank_groups.hip, and the selection of select_hardest.hip / select_hardest.h.  Plain C++, so that a host twin that includes it also compiles
// without the HIP headers.  Every member gets ONE unique 64-bit integer
//   (key << 12) | (4095 - index)      key = 0 for an invalid member, else 1 + the "%.5f" integer (mode 0) or 1.. from the fp32 order (mode 1)
// and a member's place is the number of members with a larger integer: key descending, the lower index first among equal keys.
// validate_groups holds the refusals those calls share for their groups, positives and members.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/kprn.h"

#if defined(__HIPCC__)
#define RK_HD __host__ __device__
#else
#define RK_HD
#endif

namespace rk {

// mode 0: the integer "%.5f" prints, times 1e5: the product of a 24-bit and a 17-bit significand is exact in double, rint rounds half to even as printf does
RK_HD static inline uint32_t key_of(float p, int mode) {
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
RK_HD static inline uint64_t composite(float p, int i, int mode) { return ((uint64_t)key_of(p, mode) << 12) | (uint64_t)(4095 - i); }
// mode 0: a member whose printed score is above zero (key >= 2)
RK_HD static inline bool printed_positive(uint64_t c) { return (c >> 12) >= 2u; }

// the refusals every call over board groups of at most 4096 members shares, on host arrays: KPRN_OK, or the status with its text in *why; *max_n = longest group
static inline int validate_groups(int64_t n_scores, const int64_t* members, const int64_t* goff, const int32_t* pos, int32_t G, int* max_n, const char** why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (!goff || G < 1) return bad(KPRN_E_ARG, "group_offsets is NULL or G < 1");
  if (goff[0] < 0) return bad(KPRN_E_ARG, "group_offsets[0] < 0");
  int mx = 0;
  for (int32_t g = 0; g < G; ++g) {
    const int64_t n = goff[g + 1] - goff[g];
    if (n < 1 || n > KPRN_RANK_MAX_GROUP) return bad(KPRN_E_ARG, "a group must have 1..4096 members");
    if (pos && (pos[g] < -1 || pos[g] >= n)) return bad(KPRN_E_ARG, "pos must be in -1..n-1");
    if (n > mx) mx = (int)n;
  }
  if (members) {
    for (int64_t m = goff[0]; m < goff[G]; ++m)
      if (members[m] < 0 || members[m] >= n_scores) return bad(KPRN_E_INDEX, "a member is outside the scores");
  } else if (goff[G] > n_scores) return bad(KPRN_E_INDEX, "a group runs past the end of the scores");
  if (max_n) *max_n = mx;
  return KPRN_OK;
}

}  // namespace rk
