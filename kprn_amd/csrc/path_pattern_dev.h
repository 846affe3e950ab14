// Meta-paths (include/kprn.h "meta-paths"): a graph's pattern set as the table the path finder, its sampled hops and the candidates read, and the match
// itself.  Plain C++ (no HIP headers needed), so that the host twins and a stand-alone program compile it too; the kernels see the same functions as
// __host__ __device__ code.
//   match [k][r]  (uint32, k < 5, r <= Vr, row stride Vr + 1): bit p is set iff position k of pattern p admits relation r; positions k >= hops[p] give 0
//   len [h]       (h = 1..5): the patterns of h hops
// A path of h hops carries alive = len[h] & match[0][r_0] & match[1][r_1] & ...; it matches iff alive != 0 after its last edge, and a prefix whose alive is 0
// cannot be completed: the walk leaves it there.
#pragma once
#include <stdint.h>

#include "../../include/kprn.h"
#include "philox_dev.h"   // KPRN_HD

namespace pat {

constexpr int MAX_HOPS = 5;

// the table as the kernels take it (by value); match == NULL only where no kernel with patterns is launched
struct Table {
  const uint32_t* match;
  int stride;                  // Vr + 1
  uint32_t len[MAX_HOPS + 1];  // [0] unused
};

static inline int64_t table_words(int32_t Vr) { return (int64_t)MAX_HOPS * ((int64_t)Vr + 1); }

// bit h - 1: some pattern has h hops (the hop mask a call's asked hops are cut to)
KPRN_HD int hops_mask(const Table& t) {
  int m = 0;
  for (int h = 1; h <= MAX_HOPS; ++h) if (t.len[h]) m |= 1 << (h - 1);
  return m;
}

// the patterns still alive after an edge of relation r at position k
KPRN_HD uint32_t step(const Table& t, uint32_t alive, int k, int r) { return alive & t.match[k * t.stride + r]; }

// a whole relation sequence
KPRN_HD bool matches(const Table& t, const int32_t* rels, int h) {
  if (h < 1 || h > MAX_HOPS) return false;
  uint32_t alive = t.len[h];
  for (int k = 0; k < h; ++k) alive = step(t, alive, k, rels[k]);
  return alive != 0;
}

// the refusals of a pattern set, before anything is written
static inline int validate(const int32_t* hops, const int64_t* set_offsets, const int32_t* set_rels, int32_t n, int32_t Vr, const char** why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (n < 0 || n > KPRN_PATTERN_MAX) return bad(KPRN_E_ARG, "the number of patterns must be in 0..32");
  if (n == 0) return KPRN_OK;
  if (!hops || !set_offsets) return bad(KPRN_E_ARG, "hops / set_offsets is NULL with n > 0");
  int64_t S = 0;
  for (int32_t p = 0; p < n; ++p) {
    if (hops[p] < 1 || hops[p] > MAX_HOPS) return bad(KPRN_E_ARG, "a pattern's hop count must be in 1..5");
    S += hops[p];
  }
  if (set_offsets[0] != 0) return bad(KPRN_E_ARG, "set_offsets must ascend from 0");
  for (int64_t s = 0; s < S; ++s)
    if (set_offsets[s + 1] < set_offsets[s]) return bad(KPRN_E_ARG, "set_offsets must ascend from 0");
  if (set_offsets[S] > 0 && !set_rels) return bad(KPRN_E_ARG, "set_rels is NULL");
  for (int64_t k = 0; k < set_offsets[S]; ++k)
    if (set_rels[k] < 1 || set_rels[k] > Vr) return bad(KPRN_E_INDEX, "a pattern's relation is outside 1..Vr");
  return KPRN_OK;
}

// a validated set -> match [5 (Vr + 1)] and len [6]; column r = 0 (no relation) stays 0
static inline void build(const int32_t* hops, const int64_t* set_offsets, const int32_t* set_rels, int32_t n, int32_t Vr, uint32_t* match, uint32_t* len) {
  const int64_t stride = (int64_t)Vr + 1;
  for (int64_t k = 0; k < table_words(Vr); ++k) match[k] = 0u;
  for (int h = 0; h <= MAX_HOPS; ++h) len[h] = 0u;
  int64_t s = 0;
  for (int32_t p = 0; p < n; ++p) {
    const uint32_t bit = (uint32_t)1 << p;
    len[hops[p]] |= bit;
    for (int k = 0; k < hops[p]; ++k, ++s) {
      if (set_offsets[s] == set_offsets[s + 1]) {   // the empty set: any relation
        for (int32_t r = 1; r <= Vr; ++r) match[k * stride + r] |= bit;
      } else {
        for (int64_t q = set_offsets[s]; q < set_offsets[s + 1]; ++q) match[k * stride + set_rels[q]] |= bit;
      }
    }
  }
}

}  // namespace pat
