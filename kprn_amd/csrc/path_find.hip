// Path finder (include/kprn.h "finding a pair's paths"): a knowledge graph as CSR in HBM, and for B (user, item) pairs every path of min_hops .. max_hops <= 3
// hops between them, laid out as the rows of a ragged kprn_batch; the sampled paths of 4 and 5 hops that may follow them in a pair's rows are path_walk.hip's.  Integers only; no float, no atomics that hand out output slots, no LDS beyond the
// workgroup's scan.
//
// One definition of the rule serves the kernels and the host twin (namespace pf, __host__ __device__):
//   graph   edges sorted by (src, dst, rel), exact duplicates and self-loops dropped; rowptr [Ve + 1] by 1-based node id
//   path    u = n0 -> n1 -> ... -> nh = i over edges, all nodes pairwise distinct (u == i: none); two relations between the same nodes are two paths
//   order   hops ascending, then (n1, r0, n2, r1, ..., r_{h-1}) lexicographically = the depth-first order of the sorted CSR.  The paths of h >= 2 hops are
//           grouped by their first edge e0 (u's adjacency, in order): subtree_count gives the group's sizes, subtree_fill writes its rows in order
//   rank    of a path = (paths of fewer hops) + (paths of the same hops under earlier first edges) + its place under its own first edge
// Device: one 256-thread workgroup per pair.  In a user-item graph u's adjacency is short and n1's (a popular item's raters) is long, so the 3-hop work is
// spread over the SECOND edges: every closing-edge search (edge_range of n2 -> i) is one lane's.
//   k_count   the pair's totals per hop -> tot [B][4] = {1 hop, 2 hops, 3 hops, found}: 2 hops a thread per first edge, 3 hops a wave per first edge with its
//             lanes over the second edges.  The host turns them into counts = min(found, max_paths), compacts the pairs that have paths and scans the
//             counts into each pair's first row
//   k_fill    ranks by prefix sums in the workgroup (Hillis-Steele in LDS, int64): 2 hops over 256 first edges at a time; 3 hops first edge by first edge,
//             256 second edges at a time, a running rank carried from chunk to chunk.  Which ranks are kept is path_find_dev.h's Keep: the first counts[b]
//             (a thread writes the rows of its own first / second edge at their ranks while rank < counts[b], and a hop's chunks stop once the running rank
//             reaches it: with a cap of 28 the fill pass touches a few chunks, whatever found is), or, under option "path_cap" = "spread", the ranks k_cap_ranks
//             drew (a path of rank r goes to kept row j iff r is the pair's j-th kept rank; the chunks run on to the last kept rank).  The rows a workgroup
//             placed are summed and compared with the kept ranks below the pair's exhaustive total (the rest, where sampled rows follow, path_walk.hip places
//             and checks the same way): a disagreement between the passes sets the flag (KPRN_E_DEVICE), and no write leaves the pair's range either way.
// Meta-paths (include/kprn.h "meta-paths"; path_pattern_dev.h): a graph with a pattern set launches the PAT = true instantiations, which count and place only
// the paths whose relation sequence matches a pattern (close_count / close_edge over the closing multi-edge); PAT = false is the rule above, unchanged.
// The host twin walks the same primitives (edge_range, mid_range, write_row) pair by pair on its threads.  The graph, the CSR view and edge_range are in
// path_find_dev.h, shared with neg_sample.hip; find_staged runs the two passes over a pair list that is staged into HBM by its caller.
#include "path_find_dev.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

namespace pf {

// the closing edges of the 3-hop paths u -> n1 -> col[e1] -> i: their number, the range in [lo, hi); none when the middle node repeats u, i or n1.  PAT: a0 =
// the patterns of 3 hops that admit the first edge; alive = those that also admit e1 -- none: no search is made -- and the number counts the admitted closes
template <bool PAT>
__host__ __device__ static inline int mid_range(const Csr& g, const pat::Table& pt, uint32_t a0, int u, int i, int n1, int e1, int& lo, int& hi, uint32_t& alive) {
  const int n2 = g.col[e1];
  lo = 0; hi = 0; alive = a0;
  if (n2 == u || n2 == i || n2 == n1) return 0;
  if (PAT) { alive = pat::step(pt, a0, 1, g.rel[e1]); if (!alive) return 0; }
  edge_range(g, n2, i, lo, hi);
  return close_count<PAT>(g, pt, alive, 2, lo, hi);
}

// paths of 2 / 3 hops whose first edge is e0 (want2 / want3: the hop is asked for)
template <bool PAT>
__host__ __device__ static inline void subtree_count(const Csr& g, const pat::Table& pt, int u, int i, int e0, bool want2, bool want3, int64_t& c2, int64_t& c3) {
  c2 = 0; c3 = 0;
  const int n1 = g.col[e0];
  if (n1 == u || n1 == i) return;
  uint32_t a2 = 0, a3 = 0, a;
  if (PAT) {   // a first edge no pattern of that length admits: its whole fan of second edges is left alone
    a2 = pat::step(pt, pt.len[2], 0, g.rel[e0]); a3 = pat::step(pt, pt.len[3], 0, g.rel[e0]);
    want2 = want2 && a2; want3 = want3 && a3;
  }
  int lo, hi;
  if (want2) { edge_range(g, n1, i, lo, hi); c2 = close_count<PAT>(g, pt, a2, 1, lo, hi); }
  if (!want3) return;
  const int end = g.rowptr[n1 + 1];
  for (int e1 = g.rowptr[n1]; e1 < end; ++e1) c3 += mid_range<PAT>(g, pt, a3, u, i, n1, e1, lo, hi, a);
}

// the paths of 1 hop: the admitted edges of [lo, hi)
template <bool PAT>
__host__ __device__ static inline int hop1_count(const Csr& g, const pat::Table& pt, int lo, int hi) { return close_count<PAT>(g, pt, pt.len[1], 0, lo, hi); }

// the kept paths of 1 hop (ranks 0 .. n - 1 = the admitted edges of [lo, hi), n of them) among the pair's rows first, first + step, ..; out = the pair's rows;
// returns the rows written
template <bool PAT>
__host__ __device__ static inline int hop1_fill(const Csr& g, const pat::Table& pt, const Fmt& f, int u, int i, int lo, int hi, int n, int first, int step,
                                                const Keep& keep, int32_t* out) {
  int placed = 0;
  const int64_t row = (int64_t)f.T * f.F;
  for (int64_t j = first; j < keep.cap && keep_rank(keep, j) < n; j += step) {
    const int nodes[2] = {u, i}, rels[1] = {g.rel[close_edge<PAT>(g, pt, pt.len[1], 0, lo, hi, keep_rank(keep, j))]};
    write_row(f, out + j * row, 1, nodes, rels);
    ++placed;
  }
  return placed;
}

// the kept rows of first edge e0: its paths of 2 hops have the ranks from r2 on, those of 3 hops from r3 on (< 0: that hop is not looked at); out = the pair's
// rows; returns the rows written
template <bool PAT>
__host__ __device__ static inline int subtree_fill(const Csr& g, const pat::Table& pt, const Fmt& f, int u, int i, int e0, const Keep& keep, int64_t r2, int64_t r3,
                                                   int32_t* out) {
  const int n1 = g.col[e0];
  if (n1 == u || n1 == i) return 0;
  const int64_t row = (int64_t)f.T * f.F;
  int placed = 0, lo, hi;
  uint32_t a2 = 0, a3 = 0, a;
  if (PAT) { a2 = pat::step(pt, pt.len[2], 0, g.rel[e0]); a3 = pat::step(pt, pt.len[3], 0, g.rel[e0]); }
  int64_t j = r2 >= 0 ? keep_lower(keep, r2) : keep.cap;
  if (j < keep.cap) {
    edge_range(g, n1, i, lo, hi);
    const int c = close_count<PAT>(g, pt, a2, 1, lo, hi);
    for (; j < keep.cap && keep_rank(keep, j) - r2 < c; ++j) {
      const int nodes[3] = {u, n1, i}, rels[2] = {g.rel[e0], g.rel[close_edge<PAT>(g, pt, a2, 1, lo, hi, keep_rank(keep, j) - r2)]};
      write_row(f, out + j * row, 2, nodes, rels);
      ++placed;
    }
  }
  if (r3 >= 0) {
    const int end = g.rowptr[n1 + 1];
    j = keep_lower(keep, r3);
    for (int e1 = g.rowptr[n1]; e1 < end && j < keep.cap; ++e1) {
      const int c = mid_range<PAT>(g, pt, a3, u, i, n1, e1, lo, hi, a);
      for (; j < keep.cap && keep_rank(keep, j) - r3 < c; ++j) {
        const int nodes[4] = {u, n1, g.col[e1], i}, rels[3] = {g.rel[e0], g.rel[e1], g.rel[close_edge<PAT>(g, pt, a, 2, lo, hi, keep_rank(keep, j) - r3)]};
        write_row(f, out + j * row, 3, nodes, rels);
        ++placed;
      }
      r3 += c;
    }
  }
  return placed;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------------
// PAT (every kernel below that walks edges): the graph has a pattern set and pt is its table; PAT = false never reads pt, and the match folds out of the code.
// The match sits inside a lane's own count; what surrounds a barrier or a workgroup sum stays workgroup-uniform (hmask, the first edge's relation)
template <bool PAT>
__global__ __launch_bounds__(TPB) void k_count(Csr g, pat::Table pt, const int32_t* __restrict__ pairs, int hmask, int64_t* __restrict__ tot) {
  __shared__ int64_t sh[TPB];
  const int b = blockIdx.x, u = pairs[2 * b], i = pairs[2 * b + 1];
  int64_t c1 = 0, c2 = 0, c3 = 0;
  if (u != i) {   // (workgroup-uniform)
    int lo, hi;
    if (hmask & 1) { edge_range(g, u, i, lo, hi); c1 = hop1_count<PAT>(g, pt, lo, hi); }
    const int end = g.rowptr[u + 1];
    if (hmask & 2) {   // a thread per first edge: one search each
      for (int e0 = g.rowptr[u] + threadIdx.x; e0 < end; e0 += TPB) {
        int64_t a2, a3;
        subtree_count<PAT>(g, pt, u, i, e0, true, false, a2, a3);
        c2 += a2;
      }
      c2 = block_sum(c2, sh);
    }
    if (hmask & 4) {   // a wave per first edge, its lanes over the second edges: the long adjacency of a popular n1 is 64 searches wide
      const int lane = threadIdx.x & 63;
      for (int e0 = g.rowptr[u] + (threadIdx.x >> 6); e0 < end; e0 += TPB / 64) {
        const int n1 = g.col[e0];
        if (n1 == u || n1 == i) continue;   // (wave-uniform)
        uint32_t a3 = 0, a;
        if (PAT) { a3 = pat::step(pt, pt.len[3], 0, g.rel[e0]); if (!a3) continue; }   // (wave-uniform: the fan of a first edge no pattern admits is skipped)
        const int end1 = g.rowptr[n1 + 1];
        for (int e1 = g.rowptr[n1] + lane; e1 < end1; e1 += 64) { int lo, hi; c3 += mid_range<PAT>(g, pt, a3, u, i, n1, e1, lo, hi, a); }
      }
      c3 = block_sum(c3, sh);
    }
  }
  if (threadIdx.x == 0) { tot[4 * (int64_t)b] = c1; tot[4 * (int64_t)b + 1] = c2; tot[4 * (int64_t)b + 2] = c3; tot[4 * (int64_t)b + 3] = c1 + c2 + c3; }
}

// the kept ranks of every pair under CAP_SPREAD, a thread per kept row (64-thread workgroups: a cap of 28 is one wave): ranks [first[b] + j] = cap_rank of
// the pair's found = its exhaustive total + its sampled sums (wsum == NULL: no sampled hops).  Plain stores; rebuilt by every call, read by the fill kernels
__global__ __launch_bounds__(64) void k_cap_ranks(const int64_t* __restrict__ tot, const int64_t* __restrict__ wsum, const int64_t* __restrict__ first,
                                                  const int32_t* __restrict__ cnt, int max_paths, Sampling sm, int64_t* __restrict__ ranks) {
  const int b = blockIdx.x;
  const int64_t off = first[b];
  if (off < 0) return;
  const int64_t found = tot[4 * (int64_t)b + 3] + (wsum ? wsum[2 * (int64_t)b] + wsum[2 * (int64_t)b + 1] : 0);
  for (int j = threadIdx.x; j < cnt[b]; j += 64) ranks[off + j] = cap_rank(found, max_paths, j, b, sm.k0, sm.k1, sm.draw);
}

// first [b]: the pair's first row in idx (-1: the pair has no paths and owns nothing); cnt [b]: the rows it was allotted; ranks (or NULL = the first cnt[b]):
// k_cap_ranks' array.  nxt = the first kept row whose rank is not behind the running rank: a hop's chunks stop once it reaches cnt[b], a chunk without a kept
// rank writes nothing, and a thread looks its own ranks up from nxt on (all three workgroup-uniform: every thread reads the same ranks).  SPREAD = false: ranks
// is not looked at, and the rank lookups fold into the comparisons with cnt[b] that the kernel made before there was a cap mode
template <bool SPREAD, bool PAT>
__global__ __launch_bounds__(TPB) void k_fill(Csr g, pat::Table pt, Fmt f, const int32_t* __restrict__ pairs, int hmask, const int64_t* __restrict__ tot,
                                              const int64_t* __restrict__ first, const int32_t* __restrict__ cnt, const int64_t* __restrict__ ranks,
                                              int32_t* __restrict__ idx, int32_t* flag) {
  __shared__ int64_t sh[TPB];
  const int b = blockIdx.x;
  const int64_t off = first[b];
  if (off < 0) return;   // (workgroup-uniform)
  const int u = pairs[2 * b], i = pairs[2 * b + 1];
  const int64_t cap = cnt[b], row = (int64_t)f.T * f.F;
  const Keep keep{SPREAD ? ranks + off : nullptr, cap};
  const int64_t base2 = tot[4 * (int64_t)b], base3 = base2 + tot[4 * (int64_t)b + 1];
  int32_t* out = idx + off * row;
  int64_t placed = 0;
  if (hmask & 1) {
    int lo, hi;
    edge_range(g, u, i, lo, hi);
    placed += hop1_fill<PAT>(g, pt, f, u, i, lo, hi, PAT ? (int)base2 : hi - lo, threadIdx.x, TPB, keep, out);   // (tot[0] = the hop's count)
  }
  const int end = g.rowptr[u + 1];
  // 2 hops: a thread per first edge, 256 first edges at a time; run2 = rank of the next chunk's first path (workgroup-uniform, like every loop bound below)
  if (hmask & 2) {
    int64_t run2 = base2, nxt = keep_lower(keep, run2);
    for (int e_base = g.rowptr[u]; e_base < end && nxt < cap; e_base += TPB) {
      const int e0 = e_base + threadIdx.x;
      int64_t c2 = 0, c3, sum2;
      if (e0 < end) subtree_count<PAT>(g, pt, u, i, e0, true, false, c2, c3);
      const int64_t r2 = run2 + block_scan_excl(c2, sh, sum2);
      // (every row written is a kept row j < cap: out + j * row stays inside the pair's range)
      if (c2 && keep_rank(keep, nxt) < run2 + sum2) placed += subtree_fill<PAT>(g, pt, f, u, i, e0, keep, r2, -1, out);
      run2 += sum2;
      nxt = keep_lower(keep, run2, nxt);
    }
  }
  // 3 hops: the first edges in order, the workgroup's threads over the second edges 256 at a time; a thread writes the kept paths through its second edge
  if (hmask & 4) {
    int64_t run3 = base3, nxt = keep_lower(keep, run3);   // rank of the next chunk's first path
    for (int e0 = g.rowptr[u]; e0 < end && nxt < cap; ++e0) {
      const int n1 = g.col[e0];
      if (n1 == u || n1 == i) continue;
      uint32_t a3 = 0, a = 0;
      if (PAT) { a3 = pat::step(pt, pt.len[3], 0, g.rel[e0]); if (!a3) continue; }   // (workgroup-uniform)
      const int end1 = g.rowptr[n1 + 1];
      for (int e1_base = g.rowptr[n1]; e1_base < end1 && nxt < cap; e1_base += TPB) {
        const int e1 = e1_base + threadIdx.x;
        int lo = 0, hi = 0;
        const int64_t c = e1 < end1 ? mid_range<PAT>(g, pt, a3, u, i, n1, e1, lo, hi, a) : 0;
        int64_t sum3;
        const int64_t r3 = run3 + block_scan_excl(c, sh, sum3);
        if (c && keep_rank(keep, nxt) < run3 + sum3)
          for (int64_t j = keep_lower(keep, r3, nxt); j < cap && keep_rank(keep, j) - r3 < c; ++j) {
            const int nodes[4] = {u, n1, g.col[e1], i}, rels[3] = {g.rel[e0], g.rel[e1], g.rel[close_edge<PAT>(g, pt, a, 2, lo, hi, keep_rank(keep, j) - r3)]};
            write_row(f, out + j * row, 3, nodes, rels);
            ++placed;
          }
        run3 += sum3;
        nxt = keep_lower(keep, run3, nxt);
      }
    }
  }
  placed = block_sum(placed, sh);
  // the kept ranks below the exhaustive total are this kernel's (the rest, where sampled paths follow, are path_walk.hip's)
  if (threadIdx.x == 0 && placed != keep_lower(keep, tot[4 * (int64_t)b + 3])) atomicOr(flag, 1);
}

// ---- graph build -----------------------------------------------------------------------------------------------------------------------------
__global__ void k_edge_keys(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t E, unsigned long long* __restrict__ key) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) key[e] = ((unsigned long long)(uint32_t)src[e] << 32) | (uint32_t)dst[e];
}
// keep [e]: edge e of the sorted list is no self-loop and differs from the one before it; col [e] = its destination
__global__ void k_keep(const unsigned long long* __restrict__ key, const int32_t* __restrict__ rel, int64_t E, int32_t* __restrict__ keep, int32_t* __restrict__ col) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const unsigned long long k = key[e];
  const bool loop = (uint32_t)(k >> 32) == (uint32_t)k;
  const bool dup = e > 0 && key[e - 1] == k && rel[e - 1] == rel[e];
  keep[e] = (!loop && !dup) ? 1 : 0;
  col[e] = (int32_t)(uint32_t)k;
}
// rowptr [n] = the first stored edge whose source is >= n, n = 0 .. Ve
__global__ void k_rowptr(const unsigned long long* __restrict__ key, int64_t E, int32_t Ve, int32_t* __restrict__ rowptr) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n > Ve) return;
  const unsigned long long want = (unsigned long long)n << 32;
  int64_t l = 0, r = E;
  while (l < r) { const int64_t m = l + ((r - l) >> 1); if (key[m] < want) l = m + 1; else r = m; }
  rowptr[n] = (int32_t)l;
}

static int bits_for(int64_t v) { int b = 1; while (b < 63 && ((int64_t)1 << b) <= v) ++b; return b; }

// The build's order and its dedupe over E edges already in HBM (shared with graph_update.hip, which runs it over a delta's additions): on return, once the
// stream has drained, *n_out [0] = the edges kept = the input's less self-loops and exact duplicates, in (src, dst, rel) order: *key_out [k] = src << 32 | dst,
// d_src [k] = the destination, d_dst [k] = the relation (the inputs are consumed).  Every block comes from tmp
void sort_dedupe(Tmp& tmp, hipStream_t s, int32_t* d_src, int32_t* d_dst, int32_t* d_rel, int64_t E, int32_t Ve, int32_t Vr, unsigned long long** key_out,
                 int32_t** n_out) {
  unsigned long long* key0 = tmp.get<unsigned long long>(E); unsigned long long* key1 = tmp.get<unsigned long long>(E);
  unsigned long long* key2 = tmp.get<unsigned long long>(E);
  int32_t* rel1 = tmp.get<int32_t>(E); int32_t* rel2 = tmp.get<int32_t>(E);
  int32_t* keep = tmp.get<int32_t>(E); int32_t* col2 = tmp.get<int32_t>(E);
  int32_t* d_n = tmp.get<int32_t>(4);
  hipLaunchKernelGGL(k_edge_keys, dim3(blocks_for(E)), dim3(TPB), 0, s, d_src, d_dst, E, key0);
  HIP_TRY(hipGetLastError());
  // (src, dst, rel) order from two stable passes: by relation, then by (src, dst)
  const int rbits = bits_for(Vr), kbits = 32 + bits_for(Ve);
  size_t need1 = 0, need2 = 0, need3 = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, need1, (uint32_t*)d_rel, (uint32_t*)rel1, key0, key1, (size_t)E, 0, rbits, s));
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, need2, key1, key2, rel1, rel2, (size_t)E, 0, kbits, s));
  HIP_TRY(rocprim::select(nullptr, need3, key2, keep, key0, d_n, (size_t)E, s));
  size_t need4 = 0;
  HIP_TRY(rocprim::select(nullptr, need4, col2, keep, d_src, d_n, (size_t)E, s));
  const size_t need = std::max(std::max(need1, need2), std::max(need3, need4));
  char* work = tmp.get<char>((int64_t)need);
  size_t nb = need;
  HIP_TRY(rocprim::radix_sort_pairs(work, nb, (uint32_t*)d_rel, (uint32_t*)rel1, key0, key1, (size_t)E, 0, rbits, s));
  nb = need;
  HIP_TRY(rocprim::radix_sort_pairs(work, nb, key1, key2, rel1, rel2, (size_t)E, 0, kbits, s));
  hipLaunchKernelGGL(k_keep, dim3(blocks_for(E)), dim3(TPB), 0, s, key2, rel2, E, keep, col2);
  HIP_TRY(hipGetLastError());
  // compaction: the stored key (for rowptr), destination and relation of every kept edge (d_src / d_dst are free again)
  nb = need; HIP_TRY(rocprim::select(work, nb, key2, keep, key0, d_n, (size_t)E, s));
  nb = need; HIP_TRY(rocprim::select(work, nb, col2, keep, d_src, d_n, (size_t)E, s));
  nb = need; HIP_TRY(rocprim::select(work, nb, rel2, keep, d_dst, d_n, (size_t)E, s));
  *key_out = key0; *n_out = d_n;
}

// the refusals shared by kprn_graph_create and the host twin
static int validate_graph(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr, int32_t Vt,
                          int32_t nT, int32_t end_rel, std::string* why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (E < 0 || E > 0x7fffffffLL) return bad(KPRN_E_ARG, "E must be in 0 .. 2^31 - 1");
  if ((E > 0 && (!src || !dst || !rel)) || !node_types) return bad(KPRN_E_ARG, "src / dst / rel / node_types is NULL");
  if (Ve < 2 || Vr < 1 || Vt < 1 || nT < 1) return bad(KPRN_E_ARG, "the vocabularies need Ve >= 2, Vr >= 1, Vt >= 1, num_types >= 1");
  if (end_rel < 1 || end_rel > Vr) return bad(KPRN_E_INDEX, "end_relation is outside 1..Vr");
  for (int64_t e = 0; e < E; ++e) {
    if (src[e] < 1 || src[e] >= Ve || dst[e] < 1 || dst[e] >= Ve) return bad(KPRN_E_INDEX, "an edge's node is outside 1..Ve-1 (Ve is the pad row)");
    if (rel[e] < 1 || rel[e] > Vr) return bad(KPRN_E_INDEX, "an edge's relation is outside 1..Vr");
  }
  for (int64_t k = 0; k < (int64_t)(Ve - 1) * nT; ++k)
    if (node_types[k] < 1 || node_types[k] > Vt) return bad(KPRN_E_INDEX, "a type id is outside 1..Vt");
  return KPRN_OK;
}
int validate_find_limits(int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, const Sampling* sm, std::string* why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (B < 1) return bad(KPRN_E_ARG, "pairs is NULL or B < 1");
  if (!sm && (min_hops < 1 || min_hops > max_hops || max_hops > 3)) return bad(KPRN_E_ARG, "hops: 1 <= min_hops <= max_hops <= 3");
  if (sm && (min_hops < 1 || min_hops > max_hops || max_hops > 5)) return bad(KPRN_E_ARG, "hops: 1 <= min_hops <= max_hops <= 5");
  if (sm && max_hops > 3 && (sm->walks < 1 || sm->walks > MAX_WALKS)) return bad(KPRN_E_ARG, "walks must be in 1..256 when max_hops > 3");
  if (max_paths < 1 || max_paths > kk::RAGGED_MAX_SEG) return bad(KPRN_E_ARG, "max_paths must be in 1..4096");
  if (T < max_hops + 1) return bad(KPRN_E_ARG, "T must be at least max_hops + 1");
  return KPRN_OK;
}
int validate_find(const int32_t* pairs, int32_t B, int32_t Ve, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, const Sampling* sm, std::string* why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (!pairs) return bad(KPRN_E_ARG, "pairs is NULL or B < 1");
  const int rc = validate_find_limits(B, min_hops, max_hops, max_paths, T, sm, why);
  if (rc != KPRN_OK) return rc;
  for (int64_t k = 0; k < 2 * (int64_t)B; ++k)
    if (pairs[k] < 1 || pairs[k] >= Ve) return bad(KPRN_E_INDEX, "a pair's node is outside 1..Ve-1");
  return KPRN_OK;
}

static kprn_graph* build_graph(kprn_handle* h, const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t end_rel) {
  const kprn_config& c = h->cfg;
  hipStream_t s = h->stream;
  kprn_graph* g = new kprn_graph();
  g->Ve = c.Ve; g->Vr = c.Vr; g->Vt = c.Vt; g->nT = c.num_types; g->end_rel = end_rel;
  try {
    g->rowptr = dalloc<int32_t>((int64_t)c.Ve + 1);
    g->types = dalloc<int32_t>((int64_t)c.Ve * c.num_types);
    HIP_TRY(hipMemcpyAsync(g->types, node_types, (size_t)c.Ve * c.num_types * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (E == 0) {
      HIP_TRY(hipMemsetAsync(g->rowptr, 0, ((size_t)c.Ve + 1) * sizeof(int32_t), s));
      g->col = dalloc<int32_t>(1); g->rel = dalloc<int32_t>(1);
      HIP_TRY(hipStreamSynchronize(s));
      return g;
    }
    Tmp tmp;
    int32_t* d_src = tmp.get<int32_t>(E); int32_t* d_dst = tmp.get<int32_t>(E); int32_t* d_rel = tmp.get<int32_t>(E);
    HIP_TRY(hipMemcpyAsync(d_src, src, (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_dst, dst, (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_rel, rel, (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, s));
    unsigned long long* key0 = nullptr;
    int32_t* d_n = nullptr;
    sort_dedupe(tmp, s, d_src, d_dst, d_rel, E, c.Ve, c.Vr, &key0, &d_n);
    int32_t n_kept = 0;
    HIP_TRY(hipMemcpyAsync(&n_kept, d_n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    KPRN_REQUIRE(n_kept >= 0 && n_kept <= E, KPRN_E_DEVICE, "graph build: the compaction returned an impossible edge count");
    g->E = n_kept;
    g->col = dalloc<int32_t>(n_kept); g->rel = dalloc<int32_t>(n_kept);
    if (n_kept > 0) {
      HIP_TRY(hipMemcpyAsync(g->col, d_src, (size_t)n_kept * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(g->rel, d_dst, (size_t)n_kept * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(k_rowptr, dim3(blocks_for((int64_t)c.Ve + 1)), dim3(TPB), 0, s, key0, (int64_t)n_kept, c.Ve, g->rowptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
  } catch (...) {
    dfree(g->rowptr); dfree(g->col); dfree(g->rel); dfree(g->types);
    delete g;
    throw;
  }
  return g;
}

static void free_graph(kprn_graph* g) {
  dfree(g->rowptr); dfree(g->col); dfree(g->rel); dfree(g->types); dfree(g->pat_match);
  delete g;
}

void release_all(kprn_handle* h) {
  for (kprn_graph* g : h->graphs) free_graph(g);
  h->graphs.clear();
  if (h->pf_buf) { hipFree(h->pf_buf); h->pf_buf = nullptr; h->pf_buf_bytes = 0; }
  if (h->pf_keep) { hipFree(h->pf_keep); h->pf_keep = nullptr; h->pf_keep_bytes = 0; }
}

// ---- host twin: the same rule over the host CSR (path_find_dev.h) ---------------------------------------------------------------------------
template <bool PAT>
static void host_pair_totals(const Csr& g, const pat::Table& pt, int u, int i, int hmask, int64_t* t4) {
  int64_t c1 = 0, c2 = 0, c3 = 0;
  if (u != i) {
    int lo, hi;
    if (hmask & 1) { edge_range(g, u, i, lo, hi); c1 = hop1_count<PAT>(g, pt, lo, hi); }
    if (hmask & 6)
      for (int e0 = g.rowptr[u]; e0 < g.rowptr[u + 1]; ++e0) {
        int64_t a2, a3;
        subtree_count<PAT>(g, pt, u, i, e0, (hmask & 2) != 0, (hmask & 4) != 0, a2, a3);
        c2 += a2; c3 += a3;
      }
  }
  t4[0] = c1; t4[1] = c2; t4[2] = c3; t4[3] = c1 + c2 + c3;
}

template <bool PAT>
static int64_t host_pair_fill(const Csr& g, const pat::Table& pt, const Fmt& f, int u, int i, int hmask, const int64_t* t4, const Keep& keep, int32_t* out) {
  const int64_t base2 = t4[0], base3 = t4[0] + t4[1];
  int64_t placed = 0, done2 = 0, done3 = 0;
  int lo, hi;
  if (hmask & 1) { edge_range(g, u, i, lo, hi); placed += hop1_fill<PAT>(g, pt, f, u, i, lo, hi, (int)t4[0], 0, 1, keep, out); }
  for (int e0 = g.rowptr[u]; e0 < g.rowptr[u + 1]; ++e0) {
    const bool go2 = (hmask & 2) && keep_lower(keep, base2 + done2) < keep.cap, go3 = (hmask & 4) && keep_lower(keep, base3 + done3) < keep.cap;
    if (!go2 && !go3) break;
    int64_t c2, c3;
    subtree_count<PAT>(g, pt, u, i, e0, go2, go3, c2, c3);
    placed += subtree_fill<PAT>(g, pt, f, u, i, e0, keep, c2 ? base2 + done2 : -1, c3 ? base3 + done3 : -1, out);
    done2 += c2; done3 += c3;
  }
  return placed;
}

void find_staged(kprn_handle* h, const kprn_graph* g, const StagePairs& stage, const float* labels, int32_t B, int32_t min_hops, int32_t max_hops,
                 int32_t max_paths, int32_t T, const Sampling* sm, int32_t* pairs_out, int32_t* counts, int64_t* found, kprn_batch** out) {
  const kprn_config& c = h->cfg;
  KPRN_REQUIRE(c.F >= c.num_types + 2, KPRN_E_ARG, "F must hold num_types + 2 columns");
  hipStream_t s = h->stream;
  // with a pattern set, an asked hop count that no pattern has yields no paths: it leaves the mask here, and its kernels' work with it
  const bool pat_on = g->n_pat > 0;
  const pat::Table pt = table_of(g);
  const int hmask = hop_mask(min_hops, max_hops) & (pat_on ? pat::hops_mask(pt) : ~0);
  const bool sampled = (hmask & HOPS_SAMPLED) != 0;   // (validated: sm is there)
  const bool spread = sm && sm->cap_mode == CAP_SPREAD;
  const size_t n_wc = sampled ? (size_t)2 * B * sm->walks : 0;
  // device arguments of the two passes: pairs [2B] | cnt [B] | flag [4] (int32), then tot [4B] | first [B] (int64); sampled hops add wsum [2B] | wc [B][2][walks]
  const size_t w32 = ((size_t)3 * B + 4 + 1) & ~(size_t)1, total = w32 * 4 + ((size_t)(sampled ? 7 : 5) * B + n_wc) * 8;
  grow_call_block(s, h->pf_buf, h->pf_buf_bytes, total);
  int32_t* d_pairs = (int32_t*)h->pf_buf;
  int32_t* d_cnt = d_pairs + 2 * (size_t)B;
  int32_t* d_flag = d_cnt + B;
  int64_t* d_tot = (int64_t*)((char*)h->pf_buf + w32 * 4);
  int64_t* d_first = d_tot + 4 * (size_t)B;
  int64_t* d_wsum = d_first + B;
  int64_t* d_wc = d_wsum + 2 * (size_t)B;
  const Csr csr{g->rowptr, g->col, g->rel};
  stage(d_pairs, s);
  {
    ProfScope ps(h, "find_paths_count");
    hipLaunchKernelGGL(pat_on ? k_count<true> : k_count<false>, dim3((unsigned)B), dim3(TPB), 0, s, csr, pt, d_pairs, hmask, d_tot);
    HIP_TRY(hipGetLastError());
  }
  std::vector<int64_t> tot((size_t)4 * B), first((size_t)B), wsum(sampled ? (size_t)2 * B : 0);
  if (sampled) {
    ProfScope ps(h, "find_paths_walk_count");
    walk_count_launch(csr, d_pairs, B, hmask, *sm, d_wc, d_wsum, s, pat_on ? &pt : nullptr);
    HIP_TRY(hipMemcpyAsync(wsum.data(), d_wsum, wsum.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipMemcpyAsync(tot.data(), d_tot, tot.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  if (pairs_out) HIP_TRY(hipMemcpyAsync(pairs_out, d_pairs, (size_t)2 * B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // the scan over the pairs: counts, the pairs that have paths, each one's first row
  std::vector<int32_t> cnt((size_t)B), kept;
  std::vector<int64_t> fnd((size_t)B);
  std::vector<float> lab;
  int64_t N = 0;
  for (int32_t b = 0; b < B; ++b) {
    const int64_t fx = tot[4 * (size_t)b + 3], fs = sampled ? wsum[2 * (size_t)b] + wsum[2 * (size_t)b + 1] : 0, f = fx + fs;
    KPRN_REQUIRE(fx >= 0 && fs >= 0 && (!sampled || (wsum[2 * (size_t)b] >= 0 && wsum[2 * (size_t)b + 1] >= 0)), KPRN_E_DEVICE,
                 "find_paths: the counting pass returned a negative count");
    KPRN_REQUIRE(!spread || f < CAP_MAX_FOUND, KPRN_E_ARG, "find_paths: path_cap = spread takes pairs of fewer than 2^51 paths");
    fnd[b] = f;
    cnt[b] = (int32_t)std::min<int64_t>(f, max_paths);
    first[b] = cnt[b] > 0 ? N : -1;
    if (cnt[b] > 0) { kept.push_back(cnt[b]); if (labels) lab.push_back(labels[b]); }
    N += cnt[b];
  }
  if (!kept.empty()) {
    HIP_TRY(hipMemcpyAsync(d_cnt, cnt.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_first, first.data(), (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
    const Fmt fmt{g->types, g->nT, g->Vt, g->Ve, g->Vr, T, c.F, g->end_rel};
    // spread: every pair's kept ranks, one int64 per row of the batch, at the pair's first row (a block of its own: its size is known only now)
    int64_t* d_keep = spread ? (int64_t*)grow_call_block(s, h->pf_keep, h->pf_keep_bytes, (size_t)N * sizeof(int64_t)) : nullptr;
    const slots::DeviceFill fill = [&](int32_t* idx_dev, hipStream_t st) {
      if (spread) {
        ProfScope pr(h, "find_paths_cap_ranks", st);
        hipLaunchKernelGGL(k_cap_ranks, dim3((unsigned)B), dim3(64), 0, st, d_tot, sampled ? d_wsum : nullptr, d_first, d_cnt, max_paths, *sm, d_keep);
        HIP_TRY(hipGetLastError());
      }
      {
        ProfScope ps(h, "find_paths_fill", st);
        const auto kern = pat_on ? (spread ? k_fill<true, true> : k_fill<false, true>) : (spread ? k_fill<true, false> : k_fill<false, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(TPB), 0, st, csr, pt, fmt, d_pairs, hmask, d_tot, d_first, d_cnt, d_keep, idx_dev, d_flag);
        HIP_TRY(hipGetLastError());
      }
      if (sampled) {
        ProfScope pw(h, "find_paths_walk_fill", st);
        walk_fill_launch(csr, fmt, d_pairs, B, *sm, d_tot, d_wc, d_first, d_cnt, d_keep, idx_dev, d_flag, st, pat_on ? &pt : nullptr);
      }
    };
    kprn_batch* nb = nullptr;
    slots::create(h, nullptr, kept.data(), labels ? lab.data() : nullptr, (int32_t)kept.size(), 0, N, T, c.F, &nb, &fill);
    int32_t flag = 0;
    const hipError_t e = hipMemcpy(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost);   // (create has drained the stream)
    if (e != hipSuccess || flag != 0) {
      kprn_batch_destroy(h, nb);
      HIP_TRY(e);
      throw KprnError{KPRN_E_DEVICE, "find_paths: the fill pass placed a different number of paths than the counting pass allotted"};
    }
    *out = nb;
  }
  for (int32_t b = 0; b < B; ++b) {
    if (counts) counts[b] = cnt[b];
    if (found) found[b] = fnd[b];
  }
}

int host_find(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr, int32_t Vt, int32_t num_types,
              int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, int32_t F, const Sampling* sm,
              int32_t threads, int32_t* counts, int64_t* found, int32_t* idx, const pat::Table* ptp) {
  int rc = pf::validate_graph(src, dst, rel, E, node_types, Ve, Vr, Vt, num_types, end_relation, nullptr);
  if (rc != KPRN_OK) return rc;
  rc = pf::validate_find(pairs, B, Ve, min_hops, max_hops, max_paths, T, sm, nullptr);
  if (rc != KPRN_OK) return rc;
  if (F < num_types + 2 || !counts) return KPRN_E_ARG;
  try {
    const pf::HostCsr hg = pf::host_csr(src, dst, rel, E, Ve);
    const pf::Csr g{hg.rowptr.data(), hg.col.data(), hg.rel.data()};
    const pf::Fmt f{node_types, num_types, Vt, Ve, Vr, T, F, end_relation};
    const pat::Table none{nullptr, 0, {0, 0, 0, 0, 0, 0}};
    const pat::Table& pt = ptp ? *ptp : none;
    const int hmask = pf::hop_mask(min_hops, max_hops) & (ptp ? pat::hops_mask(pt) : ~0);
    const bool sampled = (hmask & HOPS_SAMPLED) != 0;
    const bool spread = sm && sm->cap_mode == CAP_SPREAD;
    const size_t per = sampled ? (size_t)2 * sm->walks : 0;   // a pair's per-walk counts
    std::vector<int64_t> tot((size_t)4 * B), first((size_t)B), fnd((size_t)B), wc(per * B), wsum(sampled ? (size_t)2 * B : 0);
    pf::parallel_pairs(B, threads, [&](int32_t b) {
      if (ptp) pf::host_pair_totals<true>(g, pt, pairs[2 * b], pairs[2 * b + 1], hmask, &tot[4 * (size_t)b]);
      else pf::host_pair_totals<false>(g, pt, pairs[2 * b], pairs[2 * b + 1], hmask, &tot[4 * (size_t)b]);
      if (sampled) host_walk_counts(g, pairs[2 * b], pairs[2 * b + 1], b, hmask, *sm, &wc[per * b], &wsum[2 * (size_t)b], ptp);
    });
    int64_t N = 0;
    for (int32_t b = 0; b < B; ++b) {
      const int64_t f = tot[4 * (size_t)b + 3] + (sampled ? wsum[2 * (size_t)b] + wsum[2 * (size_t)b + 1] : 0);
      if (spread && f >= CAP_MAX_FOUND) return KPRN_E_ARG;
      counts[b] = (int32_t)std::min<int64_t>(f, max_paths);
      fnd[(size_t)b] = f;
      if (found) found[b] = f;
      first[b] = N;
      N += counts[b];
    }
    if (!idx) return KPRN_OK;
    std::atomic<int> wrong{0};
    pf::parallel_pairs(B, threads, [&](int32_t b) {
      if (counts[b] == 0) return;
      int32_t* rows = idx + first[b] * T * F;
      std::vector<int64_t> ranks;   // (spread, a pair over the cap: its kept ranks; every other pair keeps the first counts[b])
      if (spread && fnd[(size_t)b] > max_paths) {
        ranks.resize((size_t)counts[b]);
        for (int32_t j = 0; j < counts[b]; ++j) ranks[(size_t)j] = cap_rank(fnd[(size_t)b], max_paths, j, b, sm->k0, sm->k1, sm->draw);
      }
      const Keep keep{ranks.empty() ? nullptr : ranks.data(), counts[b]};
      int64_t placed = ptp ? pf::host_pair_fill<true>(g, pt, f, pairs[2 * b], pairs[2 * b + 1], hmask, &tot[4 * (size_t)b], keep, rows)
                           : pf::host_pair_fill<false>(g, pt, f, pairs[2 * b], pairs[2 * b + 1], hmask, &tot[4 * (size_t)b], keep, rows);
      if (sampled) placed += host_walk_fill(g, f, pairs[2 * b], pairs[2 * b + 1], b, *sm, &wc[per * b], tot[4 * (size_t)b + 3], keep, rows, ptp);
      if (placed != counts[b]) wrong = 1;
    });
    if (wrong) return KPRN_E_DEVICE;
  } catch (...) { return KPRN_E_NOMEM; }
  return KPRN_OK;
}

}  // namespace pf

extern "C" {

int kprn_graph_create(kprn_handle* h, const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t end_relation,
                      kprn_graph** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out, KPRN_E_ARG, "out is NULL");
  *out = nullptr;
  std::string why;
  const int rc = pf::validate_graph(src, dst, rel, E, node_types, h->cfg.Ve, h->cfg.Vr, h->cfg.Vt, h->cfg.num_types, end_relation, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  kprn_graph* g = pf::build_graph(h, src, dst, rel, E, node_types, end_relation);
  h->graphs.push_back(g);
  *out = g;
  API_END(h)
}

void kprn_graph_destroy(kprn_handle* h, kprn_graph* g) {
  if (!h || !g) return;
  auto it = std::find(h->graphs.begin(), h->graphs.end(), g);
  if (it == h->graphs.end()) return;   // (not this handle's, or destroyed already)
  hipSetDevice(h->cfg.device_id);
  sync_stream(h->stream, /*nothrow=*/true);   // (a finder launch may still read it)
  h->graphs.erase(it);
  pf::free_graph(g);
}

int kprn_graph_num_edges(kprn_handle* h, const kprn_graph* g, int64_t* n) {
  API_BEGIN(h)
  KPRN_REQUIRE(g && n, KPRN_E_ARG, "NULL argument");
  *n = g->E;
  API_END(h)
}

int kprn_graph_set_patterns(kprn_handle* h, kprn_graph* g, const int32_t* hops, const int64_t* set_offsets, const int32_t* set_rels, int32_t n) {
  API_BEGIN(h)
  KPRN_REQUIRE(g && std::find(h->graphs.begin(), h->graphs.end(), g) != h->graphs.end(), KPRN_E_ARG, "g is not a graph of this handle");
  const char* why = "";
  const int rc = pat::validate(hops, set_offsets, set_rels, n, g->Vr, &why);   // (every refusal, before anything is written)
  if (rc != KPRN_OK) throw KprnError{rc, why};
  if (n > 0) {
    std::vector<uint32_t> match((size_t)pat::table_words(g->Vr));
    uint32_t len[pat::MAX_HOPS + 1];
    pat::build(hops, set_offsets, set_rels, n, g->Vr, match.data(), len);
    if (!g->pat_match) g->pat_match = dalloc<uint32_t>(pat::table_words(g->Vr));
    HIP_TRY(hipStreamSynchronize(h->stream));   // (a launch still queued reads the old table)
    HIP_TRY(hipMemcpyAsync(g->pat_match, match.data(), match.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // (match leaves scope)
    std::copy(len, len + pat::MAX_HOPS + 1, g->pat_len);
  }
  g->n_pat = n;
  API_END(h)
}

int kprn_graph_num_patterns(kprn_handle* h, const kprn_graph* g, int32_t* n) {
  API_BEGIN(h)
  KPRN_REQUIRE(g && n, KPRN_E_ARG, "NULL argument");
  *n = g->n_pat;
  API_END(h)
}

}  // extern "C"

// kprn_find_paths (sm == NULL: no seed, the first paths are kept whatever option "path_cap" says) and kprn_find_paths_sampled
static int find_paths(kprn_handle* h, const kprn_graph* g, const int32_t* pairs, const float* labels, int32_t B, int32_t min_hops, int32_t max_hops,
                      int32_t max_paths, int32_t T, const pf::Sampling* sm, uint64_t seed, uint32_t draw, int32_t* counts, int64_t* found, kprn_batch** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out, KPRN_E_ARG, "out is NULL");
  *out = nullptr;
  KPRN_REQUIRE(g && std::find(h->graphs.begin(), h->graphs.end(), g) != h->graphs.end(), KPRN_E_ARG, "g is not a graph of this handle");
  std::string why;
  const int rc = pf::validate_find(pairs, B, g->Ve, min_hops, max_hops, max_paths, T, sm, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  const pf::StagePairs stage = [&](int32_t* d_pairs, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(d_pairs, pairs, (size_t)2 * B * sizeof(int32_t), hipMemcpyHostToDevice, s));
  };
  pf::Sampling spread;
  pf::find_staged(h, g, stage, labels, B, min_hops, max_hops, max_paths, T, sm ? pf::with_cap(h, sm, seed, draw, spread) : nullptr, nullptr, counts, found, out);
  API_END(h)
}

extern "C" {

int kprn_find_paths(kprn_handle* h, const kprn_graph* g, const int32_t* pairs, const float* labels, int32_t B, int32_t min_hops, int32_t max_hops,
                    int32_t max_paths, int32_t T, int32_t* counts, int64_t* found, kprn_batch** out) {
  return find_paths(h, g, pairs, labels, B, min_hops, max_hops, max_paths, T, nullptr, 0, 0, counts, found, out);
}

int kprn_find_paths_sampled(kprn_handle* h, const kprn_graph* g, const int32_t* pairs, const float* labels, int32_t B, int32_t min_hops, int32_t max_hops,
                            int32_t max_paths, int32_t T, int32_t walks, uint64_t seed, unsigned int draw, int32_t* counts, int64_t* found, kprn_batch** out) {
  const pf::Sampling sm = pf::sampling_of(walks, seed, draw);
  return find_paths(h, g, pairs, labels, B, min_hops, max_hops, max_paths, T, &sm, seed, draw, counts, found, out);
}

int kprn_host_find_paths(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr, int32_t Vt,
                         int32_t num_types, int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths,
                         int32_t T, int32_t F, int32_t threads, int32_t* counts, int64_t* found, int32_t* idx) {
  return pf::host_find(src, dst, rel, E, node_types, Ve, Vr, Vt, num_types, end_relation, pairs, B, min_hops, max_hops, max_paths, T, F, nullptr, threads, counts, found,
                       idx);
}

int kprn_host_find_paths_sampled(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr,
                                 int32_t Vt, int32_t num_types, int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops,
                                 int32_t max_paths, int32_t T, int32_t F, int32_t walks, uint64_t seed, unsigned int draw, int32_t threads, int32_t* counts,
                                 int64_t* found, int32_t* idx) {
  return kprn_host_find_paths_cap(src, dst, rel, E, node_types, Ve, Vr, Vt, num_types, end_relation, pairs, B, min_hops, max_hops, max_paths, T, F, walks, seed, draw,
                                  pf::CAP_FIRST, threads, counts, found, idx);
}

int kprn_host_find_paths_cap(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr, int32_t Vt,
                             int32_t num_types, int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths,
                             int32_t T, int32_t F, int32_t walks, uint64_t seed, unsigned int draw, int32_t cap_mode, int32_t threads, int32_t* counts,
                             int64_t* found, int32_t* idx) {
  if (cap_mode != pf::CAP_FIRST && cap_mode != pf::CAP_SPREAD) return KPRN_E_ARG;
  const pf::Sampling sm = pf::sampling_of(walks, seed, draw, cap_mode);
  return pf::host_find(src, dst, rel, E, node_types, Ve, Vr, Vt, num_types, end_relation, pairs, B, min_hops, max_hops, max_paths, T, F, &sm, threads, counts, found,
                       idx);
}

int kprn_host_find_paths_patterns(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr, int32_t Vt,
                                  int32_t num_types, int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths,
                                  int32_t T, int32_t F, int32_t walks, uint64_t seed, unsigned int draw, int32_t cap_mode, int32_t threads, int32_t* counts,
                                  int64_t* found, int32_t* idx, const int32_t* hops, const int64_t* set_offsets, const int32_t* set_rels, int32_t n_pat) {
  if (cap_mode != pf::CAP_FIRST && cap_mode != pf::CAP_SPREAD) return KPRN_E_ARG;
  if (Vr < 1) return KPRN_E_ARG;
  const pf::Sampling sm = pf::sampling_of(walks, seed, draw, cap_mode);
  try {
    pf::HostPat hp;
    const int rc = hp.set(hops, set_offsets, set_rels, n_pat, Vr);
    if (rc != KPRN_OK) return rc;
    return pf::host_find(src, dst, rel, E, node_types, Ve, Vr, Vt, num_types, end_relation, pairs, B, min_hops, max_hops, max_paths, T, F, &sm, threads, counts, found,
                         idx, hp.on ? &hp.t : nullptr);
  } catch (...) { return KPRN_E_NOMEM; }
}

int kprn_host_cap_select(int64_t found, int32_t max_paths, int32_t b, uint64_t seed, unsigned int draw, int64_t* ranks) {
  if (found < 0 || found >= pf::CAP_MAX_FOUND || max_paths < 1 || max_paths > kk::RAGGED_MAX_SEG || b < 0 || (found > 0 && !ranks)) return KPRN_E_ARG;
  const pf::Sampling sm = pf::sampling_of(0, seed, draw, pf::CAP_SPREAD);
  const int64_t n = std::min<int64_t>(found, max_paths);
  for (int64_t j = 0; j < n; ++j) ranks[j] = pf::cap_rank(found, max_paths, j, b, sm.k0, sm.k1, sm.draw);
  return KPRN_OK;
}

}  // extern "C"
