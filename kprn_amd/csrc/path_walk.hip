// Sampled paths of four and five hops (include/kprn.h "sampled paths of four and five hops"): what the finder (path_find.hip) appends to a pair's exhaustive
// paths of 1..3 hops when max_hops > 3.  A path of h in {4, 5} hops = a random prefix of h - 2 hops out of the user, then every way to close the last two hops
// into the item.  Integers only; no atomic hands out a slot or a rank; the only atomic is the flag's.
//
// One definition of the rule serves the kernels and the host twin (namespace pf, __host__ __device__):
//   walk     w = 0 .. walks - 1 of hop count h of pair-list row b: four Philox words addressed by (w, 65536 + h, b, draw); word k picks edge
//            rowptr[n_k] + mulhi32(word, degree) of the node reached so far.  Dead: a node without edges, or a node that repeats u, i or the prefix
//   dropped  a live walk whose edge sequence an earlier walk of the same h has: distinct prefixes give distinct paths, so nothing is found twice
//   paths    of a live walk: (e, c), e an edge n_{h-2} -> m with m off the prefix and != i, c an edge m -> i; e ascending, then c (close_range)
//   rank     of a path = (the pair's exhaustive paths) + (paths of the walks before it: 4 hops' walks, then 5 hops', by walk index) + its place in its walk
// Device: one 256-thread workgroup per pair, beside k_count / k_fill.
//   k_walk_count  a thread per walk forms the prefix (one Philox call) and puts its edges into LDS, seq [2][256][3]; a thread marks its walk dropped after
//                 comparing it with the earlier ones (every lane reads the same LDS words: broadcasts).  Then a wave per live walk, its lanes over the
//                 last node's adjacency, one closing search (edge_range m -> i) per lane: a popular node is 64 searches wide.  Per-walk counts -> wc
//                 [B][2][walks], their sums -> wsum [B][2]; the host adds them to found and caps
//   k_walk_fill   one workgroup scan over the pair's 2 * walks stored counts gives every walk its first rank.  A wave per walk whose first rank is below
//                 the pair's allotment and whose rank range holds a kept rank (path_find_dev.h Keep: the first counts[b] ranks, or the drawn ones of option
//                 "path_cap" = "spread") regenerates the prefix from its Philox words (a dropped walk has count 0 and is never looked at) and walks the
//                 closing adjacency 64 edges at a time, a wave prefix sum (shuffles) per chunk and the running rank carried along, until the walk's last kept
//                 rank is behind it; no workgroup barrier in that loop.  A path goes to kept row j iff its rank is the pair's j-th kept rank; the rows placed
//                 are summed and compared with the kept ranks at or above the exhaustive total (the finder's flag)
// Meta-paths (PAT = true; path_pattern_dev.h): the walks are drawn as above, a walk's paths are its closes whose whole relation sequence matches a pattern, and
// a live walk whose prefix no pattern admits counts 0 without walking its closes.
// Control flow around every shuffle and barrier is wave- / workgroup-uniform: the loop bounds and branch conditions there are kernel arguments, values
// every lane reads from the same address, or results of the cross-lane operations themselves.
#include "path_find_dev.h"

namespace pf {

constexpr int WAVES = TPB / 64;
static_assert(MAX_WALKS <= TPB, "k_walk_count forms one walk per thread");

// walk w of h hops of row b: its prefix's edges e [h - 2] (the other places stay as they are), nodes n [h - 1] = (u, n_1, .., n_{h-2}) and relations r [h - 2];
// false = the walk is dead
__host__ __device__ static inline bool walk_prefix(const Csr& g, const Sampling& sm, int u, int i, int b, int w, int h, int* e, int* n, int* r) {
  uint32_t word[4];
  philox::philox4x32_10((uint32_t)w, 65536u + (uint32_t)h, (uint32_t)b, sm.draw, sm.k0, sm.k1, word);
  n[0] = u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k > h - 3) break;
    const int lo = g.rowptr[n[k]], deg = g.rowptr[n[k] + 1] - lo;
    if (deg == 0) return false;
    e[k] = lo + (int)philox::mulhi32(word[k], (uint32_t)deg);
    const int nx = g.col[e[k]];
    if (nx == i) return false;
#pragma unroll
    for (int j = 0; j <= k; ++j) if (nx == n[j]) return false;
    n[k + 1] = nx; r[k] = g.rel[e[k]];
  }
  return true;
}

// the patterns of h hops that admit a walk's prefix relations r [h - 2]
__host__ __device__ static inline uint32_t prefix_alive(const pat::Table& pt, const int* r, int h) {
  uint32_t a = pt.len[h];
  for (int k = 0; k <= h - 3; ++k) a = pat::step(pt, a, k, r[k]);
  return a;
}

// the closing edges of the paths through edge e of the prefix's last node: their number, the range in [lo, hi); none when col[e] is i or on the prefix.
// PAT: a0 = prefix_alive; alive = the patterns that also admit e -- none: no search is made -- and the number counts the admitted closes
template <bool PAT>
__host__ __device__ static inline int close_range(const Csr& g, const pat::Table& pt, uint32_t a0, const int* n, int h, int i, int e, int& lo, int& hi,
                                                  uint32_t& alive) {
  const int m = g.col[e];
  lo = 0; hi = 0; alive = a0;
  if (m == i) return 0;
  for (int j = 0; j <= h - 2; ++j) if (m == n[j]) return 0;
  if (PAT) { alive = pat::step(pt, a0, h - 2, g.rel[e]); if (!alive) return 0; }
  edge_range(g, m, i, lo, hi);
  return close_count<PAT>(g, pt, alive, h - 1, lo, hi);
}

// the row of the path prefix -> col[e] -> i over edges e and c
__host__ __device__ static inline void walk_row(const Csr& g, const Fmt& f, int32_t* row, const int* n, const int* r, int h, int i, int e, int c) {
  int nodes[6], rels[5];
  for (int k = 0; k <= h - 2; ++k) nodes[k] = n[k];
  for (int k = 0; k <= h - 3; ++k) rels[k] = r[k];
  nodes[h - 1] = g.col[e]; nodes[h] = i;
  rels[h - 2] = g.rel[e]; rels[h - 1] = g.rel[c];
  write_row(f, row, h, nodes, rels);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------------
__device__ static inline int64_t wave_sum(int64_t v) {
  for (int d = 32; d > 0; d >>= 1) v += (int64_t)__shfl_xor((long long)v, d);
  return v;
}

template <bool PAT>
__global__ __launch_bounds__(TPB) void k_walk_count(Csr g, pat::Table pt, const int32_t* __restrict__ pairs, int hmask, Sampling sm, int64_t* __restrict__ wc,
                                                    int64_t* __restrict__ wsum) {
  __shared__ int32_t seq[2][MAX_WALKS][3];   // a walk's edges; [0] = -1: dead or dropped
  __shared__ int64_t sh[TPB];
  const int b = blockIdx.x, u = pairs[2 * b], i = pairs[2 * b + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool pair_ok = u != i && i != 0;
  int64_t sum[2] = {0, 0};   // lane 0 of a wave: the paths of its walks
  for (int s = 0; s < 2; ++s) {
    const int h = 4 + s;
    const bool asked = pair_ok && ((hmask >> (h - 1)) & 1);   // (workgroup-uniform)
    if (asked) {
      int e[3] = {0, 0, 0};
      bool live = false;
      if (tid < sm.walks) {
        int n[4], r[3];
        live = walk_prefix(g, sm, u, i, b, tid, h, e, n, r);
        seq[s][tid][0] = live ? e[0] : -1; seq[s][tid][1] = e[1]; seq[s][tid][2] = e[2];
      }
      __syncthreads();
      bool dup = false;
      for (int v = 0; v < sm.walks; ++v)   // (every lane reads walk v's words: a broadcast)
        dup = dup || (v < tid && seq[s][v][0] == e[0] && seq[s][v][1] == e[1] && seq[s][v][2] == e[2]);
      __syncthreads();   // (the marks below change what the loop above reads)
      if (live && dup) seq[s][tid][0] = -1;
      __syncthreads();
    }
    for (int w = wave; w < sm.walks; w += WAVES) {
      int64_t c = 0;
      if (asked && seq[s][w][0] >= 0) {   // (wave-uniform: one LDS word)
        int n[4], r[3];
        n[0] = u;
        for (int k = 0; k <= h - 3; ++k) { n[k + 1] = g.col[seq[s][w][k]]; if (PAT) r[k] = g.rel[seq[s][w][k]]; }
        const uint32_t a0 = PAT ? prefix_alive(pt, r, h) : 0u;   // (wave-uniform: LDS words every lane reads)
        uint32_t a;
        const int last = n[h - 2], end = !PAT || a0 ? g.rowptr[last + 1] : 0;   // a prefix no pattern admits: its closes are not walked, the sum is 0
        for (int e = g.rowptr[last] + lane; e < end; e += 64) { int lo, hi; c += close_range<PAT>(g, pt, a0, n, h, i, e, lo, hi, a); }
        c = wave_sum(c);
      }
      if (lane == 0) { wc[((int64_t)b * 2 + s) * sm.walks + w] = c; sum[s] += c; }
    }
  }
  const int64_t s4 = block_sum(sum[0], sh), s5 = block_sum(sum[1], sh);
  if (tid == 0) { wsum[2 * (int64_t)b] = s4; wsum[2 * (int64_t)b + 1] = s5; }
}

// tot [b][3]: the pair's exhaustive paths = the rank of its first sampled path; first / cnt / ranks / flag as k_fill's.  nxt = the first kept row whose rank
// is not behind the running rank (wave-uniform: every lane reads the same ranks); SPREAD as k_fill's
template <bool SPREAD, bool PAT>
__global__ __launch_bounds__(TPB) void k_walk_fill(Csr g, pat::Table pt, Fmt f, const int32_t* __restrict__ pairs, Sampling sm, const int64_t* __restrict__ tot,
                                                   const int64_t* __restrict__ wc, const int64_t* __restrict__ first, const int32_t* __restrict__ cnt,
                                                   const int64_t* __restrict__ ranks, int32_t* __restrict__ idx, int32_t* flag) {
  __shared__ int64_t sh[TPB];
  __shared__ int64_t wbase[2 * MAX_WALKS];   // rank of a walk's first path
  const int b = blockIdx.x;
  const int64_t off = first[b];
  if (off < 0) return;   // (workgroup-uniform)
  const int64_t cap = cnt[b], base = tot[4 * (int64_t)b + 3], row = (int64_t)f.T * f.F;
  const Keep keep{SPREAD ? ranks + off : nullptr, cap};
  const int64_t row0 = keep_lower(keep, base);   // the kept rows before it are the exhaustive paths'
  if (row0 >= cap) return;   // the exhaustive paths fill the allotment
  const int u = pairs[2 * b], i = pairs[2 * b + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nw = 2 * sm.walks;   // the pair's walks in rank order: 4 hops' then 5 hops'
  const int64_t* mine = wc + (int64_t)b * nw;
  int32_t* out = idx + off * row;
  const int64_t c0 = 2 * tid < nw ? mine[2 * tid] : 0, c1 = 2 * tid + 1 < nw ? mine[2 * tid + 1] : 0;
  int64_t all;
  const int64_t ex = base + block_scan_excl(c0 + c1, sh, all);
  wbase[2 * tid] = ex; wbase[2 * tid + 1] = ex + c0;
  __syncthreads();
  int64_t placed = 0;
  for (int fl = wave; fl < nw; fl += WAVES) {   // (what decides the branches below is read by every lane from one address)
    int64_t run = wbase[fl];   // rank of the next chunk's first path
    const int64_t wend = run + mine[fl];
    int64_t nxt = keep_lower(keep, run, row0);
    if (nxt >= cap) break;     // (the ranks ascend)
    if (keep_rank(keep, nxt) >= wend) continue;   // no kept rank in the walk (an empty walk among them): its prefix is not regenerated
    const int s = fl >= sm.walks ? 1 : 0, w = fl - s * sm.walks, h = 4 + s;
    int e[3], n[4], r[3];
    if (!walk_prefix(g, sm, u, i, b, w, h, e, n, r)) continue;   // (never: a dead walk's count is 0; the sum below would tell)
    const uint32_t a0 = PAT ? prefix_alive(pt, r, h) : 0u;
    uint32_t a = 0;
    const int last = n[h - 2], end = g.rowptr[last + 1];
    for (int e_base = g.rowptr[last]; e_base < end && nxt < cap && keep_rank(keep, nxt) < wend; e_base += 64) {
      const int e1 = e_base + lane;
      int lo = 0, hi = 0;
      const int c = e1 < end ? close_range<PAT>(g, pt, a0, n, h, i, e1, lo, hi, a) : 0;
      int incl = c;
      for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
      const int chunk = __shfl(incl, 63);
      const int64_t r0 = run + incl - c;
      if (c && keep_rank(keep, nxt) < run + chunk)
        for (int64_t j = keep_lower(keep, r0, nxt); j < cap && keep_rank(keep, j) - r0 < c; ++j) {
          walk_row(g, f, out + j * row, n, r, h, i, e1, close_edge<PAT>(g, pt, a, h - 1, lo, hi, keep_rank(keep, j) - r0));
          ++placed;
        }
      run += chunk;
      nxt = keep_lower(keep, run, nxt);
    }
  }
  placed = block_sum(placed, sh);
  if (tid == 0 && placed != cap - row0) atomicOr(flag, 1);
}

void walk_count_launch(const Csr& g, const int32_t* d_pairs, int32_t B, int hmask, const Sampling& sm, int64_t* d_wc, int64_t* d_wsum, hipStream_t s,
                       const pat::Table* pt) {
  const pat::Table none{nullptr, 0, {0, 0, 0, 0, 0, 0}};
  hipLaunchKernelGGL(pt ? k_walk_count<true> : k_walk_count<false>, dim3((unsigned)B), dim3(TPB), 0, s, g, pt ? *pt : none, d_pairs, hmask, sm, d_wc, d_wsum);
  HIP_TRY(hipGetLastError());
}

void walk_fill_launch(const Csr& g, const Fmt& f, const int32_t* d_pairs, int32_t B, const Sampling& sm, const int64_t* d_tot, const int64_t* d_wc,
                      const int64_t* d_first, const int32_t* d_cnt, const int64_t* d_keep, int32_t* idx, int32_t* d_flag, hipStream_t s, const pat::Table* pt) {
  const pat::Table none{nullptr, 0, {0, 0, 0, 0, 0, 0}};
  const auto kern = pt ? (d_keep ? k_walk_fill<true, true> : k_walk_fill<false, true>) : (d_keep ? k_walk_fill<true, false> : k_walk_fill<false, false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(TPB), 0, s, g, pt ? *pt : none, f, d_pairs, sm, d_tot, d_wc, d_first, d_cnt, d_keep, idx, d_flag);
  HIP_TRY(hipGetLastError());
}

// ---- host twin -------------------------------------------------------------------------------------------------------------------------------
template <bool PAT>
static void host_walk_counts_t(const Csr& g, const pat::Table& pt, int u, int i, int b, int hmask, const Sampling& sm, int64_t* wc, int64_t* s2) {
  std::vector<int> seq((size_t)3 * sm.walks);
  for (int s = 0; s < 2; ++s) {
    const int h = 4 + s;
    s2[s] = 0;
    int64_t* mine = wc + (size_t)s * sm.walks;
    std::fill(mine, mine + sm.walks, 0);
    if (u == i || i == 0 || !((hmask >> (h - 1)) & 1)) continue;
    for (int w = 0; w < sm.walks; ++w) {
      int* e = &seq[(size_t)3 * w];
      int n[4], r[3];
      e[0] = e[1] = e[2] = 0;
      if (!walk_prefix(g, sm, u, i, b, w, h, e, n, r)) { e[0] = -1; continue; }
      bool dup = false;
      for (int v = 0; v < w && !dup; ++v) dup = std::equal(e, e + 3, &seq[(size_t)3 * v]);   // (a dropped walk equals a kept one before it)
      if (dup) continue;
      const int last = n[h - 2];
      const uint32_t a0 = PAT ? prefix_alive(pt, r, h) : 0u;
      uint32_t a;
      for (int e1 = g.rowptr[last]; e1 < g.rowptr[last + 1]; ++e1) { int lo, hi; mine[w] += close_range<PAT>(g, pt, a0, n, h, i, e1, lo, hi, a); }
      s2[s] += mine[w];
    }
  }
}
void host_walk_counts(const Csr& g, int u, int i, int b, int hmask, const Sampling& sm, int64_t* wc, int64_t* s2, const pat::Table* pt) {
  const pat::Table none{nullptr, 0, {0, 0, 0, 0, 0, 0}};
  if (pt) host_walk_counts_t<true>(g, *pt, u, i, b, hmask, sm, wc, s2);
  else host_walk_counts_t<false>(g, none, u, i, b, hmask, sm, wc, s2);
}

template <bool PAT>
static int64_t host_walk_fill_t(const Csr& g, const pat::Table& pt, const Fmt& f, int u, int i, int b, const Sampling& sm, const int64_t* wc, int64_t base,
                                const Keep& keep, int32_t* out) {
  const int64_t row = (int64_t)f.T * f.F, cap = keep.cap;
  int64_t run = base, placed = 0, j = keep_lower(keep, base);   // j: the next kept row
  for (int fl = 0; fl < 2 * sm.walks && j < cap; run += wc[fl], ++fl) {
    if (keep_rank(keep, j) >= run + wc[fl]) continue;
    const int s = fl >= sm.walks ? 1 : 0, w = fl - s * sm.walks, h = 4 + s;
    int e[3], n[4], r[3];
    if (!walk_prefix(g, sm, u, i, b, w, h, e, n, r)) continue;
    const int last = n[h - 2];
    const uint32_t a0 = PAT ? prefix_alive(pt, r, h) : 0u;
    uint32_t a;
    int64_t r0 = run;
    for (int e1 = g.rowptr[last]; e1 < g.rowptr[last + 1] && j < cap; ++e1) {
      int lo, hi;
      const int c = close_range<PAT>(g, pt, a0, n, h, i, e1, lo, hi, a);
      for (; j < cap && keep_rank(keep, j) - r0 < c; ++j) {
        walk_row(g, f, out + j * row, n, r, h, i, e1, close_edge<PAT>(g, pt, a, h - 1, lo, hi, keep_rank(keep, j) - r0));
        ++placed;
      }
      r0 += c;
    }
  }
  return placed;
}
int64_t host_walk_fill(const Csr& g, const Fmt& f, int u, int i, int b, const Sampling& sm, const int64_t* wc, int64_t base, const Keep& keep, int32_t* out,
                       const pat::Table* pt) {
  const pat::Table none{nullptr, 0, {0, 0, 0, 0, 0, 0}};
  return pt ? host_walk_fill_t<true>(g, *pt, f, u, i, b, sm, wc, base, keep, out) : host_walk_fill_t<false>(g, none, f, u, i, b, sm, wc, base, keep, out);
}

}  // namespace pf
