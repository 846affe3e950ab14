// Sampled evaluation groups (include/kprn.h "sampled evaluation groups"): what the device stage (eval_sample.hip) and the host twin share, in plain C++ so
// that the twin also compiles without the HIP headers (tests/eval_sample_san_main.cpp builds it into a stand-alone program under the host sanitizers).
//
// One definition of the rule serves the kernels and the twin (namespace es):
//   key     ((uint64)w0 << 32) | (uint32)c, w0 = word 0 of Philox4x32-10 with key (seed low, seed high) and counter (c, i, u, draw): a function of ids only
//   find    position of an id in an ascending run of list rows (the item column, stride 2) or of target ids (stride 1) by binary search, -1 = not there
// The twin takes the n_neg smallest keys of D by a partial sort; the kernel finds the same cut by a radix select (keys are distinct: c is).
// Integers only.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/kprn.h"
#include "philox_dev.h"

namespace es {

typedef unsigned long long u64;

struct Seed { uint32_t k0, k1, draw; };   // seed & 0xffffffff, seed >> 32, draw
static inline Seed seed_of(uint64_t seed, unsigned int draw) { return Seed{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)draw}; }

KPRN_HD u64 key(const Seed& s, int32_t u, int32_t i, int32_t c) {
  uint32_t w[4];
  philox::philox4x32_10((uint32_t)c, (uint32_t)i, (uint32_t)u, s.draw, s.k0, s.k1, w);
  return ((u64)w[0] << 32) | (u64)(uint32_t)c;
}

// position of id among a[0], a[stride], ..., a[(n - 1) stride] (ascending), -1 = not there
KPRN_HD int64_t find(const int32_t* a, int64_t n, int stride, int32_t id) {
  int64_t l = 0, r = n;
  while (l < r) { const int64_t m = l + ((r - l) >> 1); if (a[m * stride] < id) l = m + 1; else r = m; }
  return (l < n && a[l * stride] == id) ? l : -1;
}

// the refusals both entry points share, on host arrays (the list itself is the caller's to vouch for): KPRN_OK, or the status with its text in *why
static inline int validate(const int32_t* group_counts, int32_t B, int64_t total, const int64_t* toff, const int32_t* titems, int32_t n_neg, int32_t Ve,
                           const void* o1, const void* o2, const void* o3, const void* o4, const void* o5, const char** why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (!group_counts || !toff || !titems || B < 1) return bad(KPRN_E_ARG, "group_counts, target_offsets or target_items is NULL, or B < 1");
  if (!o1 || !o2 || !o3 || !o4 || !o5) return bad(KPRN_E_ARG, "an output is NULL");
  if (n_neg < 1 || n_neg > KPRN_RANK_MAX_GROUP - 1) return bad(KPRN_E_ARG, "n_neg must be in 1..4095");
  int64_t sum = 0;
  for (int32_t b = 0; b < B; ++b) {
    if (group_counts[b] < 0) return bad(KPRN_E_ARG, "a group count is negative");
    sum += group_counts[b];
  }
  if (sum != total) return bad(KPRN_E_ARG, "group_counts do not add up to the candidate list's total");
  if (toff[0] != 0) return bad(KPRN_E_ARG, "target_offsets[0] must be 0");
  for (int32_t b = 0; b < B; ++b)
    if (toff[b + 1] < toff[b]) return bad(KPRN_E_ARG, "target_offsets must not decrease");
  const int64_t NT = toff[B];
  if (NT < 1) return bad(KPRN_E_ARG, "no targets at all");
  if (NT * (int64_t)(n_neg + 1) > 0x7fffffffLL) return bad(KPRN_E_ARG, "NT * (n_neg + 1) must stay below 2^31");
  for (int64_t k = 0; k < NT; ++k)
    if (titems[k] < 1 || titems[k] >= Ve) return bad(KPRN_E_INDEX, "a target item is outside 1..Ve-1");
  for (int32_t b = 0; b < B; ++b)
    for (int64_t k = toff[b] + 1; k < toff[b + 1]; ++k)
      if (titems[k] <= titems[k - 1]) return bad(KPRN_E_ARG, "target items must be strictly ascending within a user");
  return KPRN_OK;
}

// the rule on the host cores.  new_list [new_total][2] or NULL; everything is formed in buffers of the call's own and copied out at the end
static inline int host_sample(const int32_t* list, int64_t total, int32_t Ve, const int32_t* group_counts, int32_t B, const int64_t* toff, const int32_t* titems,
                              int32_t n_neg, uint64_t seed, unsigned int draw, int32_t* new_group_counts, int64_t* new_total, int32_t* target_rows,
                              int32_t* neg_rows, int32_t* n_drawn, int32_t* new_list) {
  if (total < 0 || total > 0x7fffffffLL || (total > 0 && !list)) return KPRN_E_ARG;
  const int rc = validate(group_counts, B, total, toff, titems, n_neg, Ve, new_group_counts, new_total, target_rows, neg_rows, n_drawn, nullptr);
  if (rc != KPRN_OK) return rc;
  {   // the list's own shape: one user per group, items strictly ascending within it, ids in 1..Ve-1
    int64_t r = 0;
    for (int32_t b = 0; b < B; ++b)
      for (int64_t j = 0; j < group_counts[b]; ++j, ++r) {
        if (list[2 * r] < 1 || list[2 * r] >= Ve || list[2 * r + 1] < 1 || list[2 * r + 1] >= Ve) return KPRN_E_INDEX;
        if (j > 0 && (list[2 * r] != list[2 * r - 2] || list[2 * r + 1] <= list[2 * r - 1])) return KPRN_E_ARG;
      }
  }
  const Seed sd = seed_of(seed, draw);
  const int64_t NT = toff[B];
  std::vector<int32_t> trow((size_t)NT, -1), nd((size_t)NT, 0), neg((size_t)NT * n_neg, -1), ngc((size_t)B, 0), to_new((size_t)total, -1);
  std::vector<unsigned char> kept((size_t)total, 0);
  std::vector<std::pair<u64, int64_t>> keys;
  int64_t r0 = 0;
  for (int32_t b = 0; b < B; ++b) {
    const int64_t n = group_counts[b], t0 = toff[b], nt = toff[b + 1] - t0;
    const int32_t* rows = list + 2 * r0;
    for (int64_t k = t0; k < t0 + nt; ++k) {
      const int32_t i = titems[k];
      const int64_t at = find(rows + 1, n, 2, i);
      if (at < 0) continue;   // unreachable: draws nothing
      const int32_t u = rows[0];
      trow[(size_t)k] = (int32_t)(r0 + at);
      kept[(size_t)(r0 + at)] = 1;
      keys.clear();
      for (int64_t j = 0; j < n; ++j) {
        const int32_t c = rows[2 * j + 1];
        if (find(titems + t0, nt, 1, c) < 0) keys.emplace_back(key(sd, u, i, c), r0 + j);
      }
      if ((int64_t)keys.size() > n_neg) {
        std::nth_element(keys.begin(), keys.begin() + n_neg, keys.end());
        keys.resize((size_t)n_neg);
      }
      std::sort(keys.begin(), keys.end(), [](const std::pair<u64, int64_t>& x, const std::pair<u64, int64_t>& y) { return x.second < y.second; });
      nd[(size_t)k] = (int32_t)keys.size();
      for (size_t q = 0; q < keys.size(); ++q) {
        neg[(size_t)k * n_neg + q] = (int32_t)keys[q].second;
        kept[(size_t)keys[q].second] = 1;
      }
    }
    r0 += n;
  }
  // the kept rows in the old order, and every old row's new one
  int64_t at = 0;
  r0 = 0;
  for (int32_t b = 0; b < B; ++b) {
    const int64_t before = at;
    for (int64_t j = 0; j < group_counts[b]; ++j)
      if (kept[(size_t)(r0 + j)]) to_new[(size_t)(r0 + j)] = (int32_t)at++;
    ngc[(size_t)b] = (int32_t)(at - before);
    r0 += group_counts[b];
  }
  for (int32_t& v : trow) if (v >= 0) v = to_new[(size_t)v];
  for (int32_t& v : neg) if (v >= 0) v = to_new[(size_t)v];
  if (new_list)
    for (int64_t r = 0; r < total; ++r)
      if (kept[(size_t)r]) { new_list[2 * (int64_t)to_new[(size_t)r]] = list[2 * r]; new_list[2 * (int64_t)to_new[(size_t)r] + 1] = list[2 * r + 1]; }
  std::copy(ngc.begin(), ngc.end(), new_group_counts);
  *new_total = at;
  std::copy(trow.begin(), trow.end(), target_rows);
  std::copy(neg.begin(), neg.end(), neg_rows);
  std::copy(nd.begin(), nd.end(), n_drawn);
  return KPRN_OK;
}

}  // namespace es
