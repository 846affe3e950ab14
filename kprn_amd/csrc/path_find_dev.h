// What the path finder (path_find.hip), its sampled hops (path_walk.hip), the negative sampler (neg_sample.hip) and the candidates (candidates.hip) share: the graph in HBM, the CSR view they
// walk and a path's row (namespace pf, __host__ __device__), the closing multi-edge under a pattern set (close_count / close_edge; path_pattern_dev.h), the
// workgroup's sums, the host CSR of the twins and their thread loop.
#pragma once
#include "kprn_internal.h"
#include "philox_dev.h"
#include "path_pattern_dev.h"

#include <algorithm>
#include <atomic>
#include <thread>
#include <tuple>

struct kprn_graph {
  int32_t Ve = 0, Vr = 0, Vt = 0, nT = 0, end_rel = 0;
  int64_t E = 0;                 // stored edges (after duplicates and self-loops are gone)
  int32_t* rowptr = nullptr;     // device [Ve + 1]: edges of node n = rowptr[n] .. rowptr[n + 1] - 1 (n = 0 has none)
  int32_t* col = nullptr;        // device [E] destination
  int32_t* rel = nullptr;        // device [E] relation
  int32_t* types = nullptr;      // device [Ve][nT]: row e - 1 = the type slots of entity e
  // the pattern set (include/kprn.h "meta-paths"; path_pattern_dev.h): n_pat == 0 = no filter.  The table's block is made by the first set and kept
  int32_t n_pat = 0;
  uint32_t* pat_match = nullptr; // device [5][Vr + 1]
  uint32_t pat_len[pat::MAX_HOPS + 1] = {0, 0, 0, 0, 0, 0};
};

struct kprn_sampler {
  int32_t M = 0;
  int32_t* items = nullptr;            // device [M] ascending entity ids: the negative sampler's candidate list and the catalogue of candidates.hip
  unsigned long long* thr = nullptr;   // device [M], thr[M - 1] = 2^32
};

namespace ns {   // (neg_sample.hip) the refusals of an item list and of a user list, shared with candidates.hip
int validate_table(const int32_t* items, const float* weights, int64_t M, int32_t Ve, std::string* why);
int validate_users(const int32_t* users, int64_t n, int32_t Ve, std::string* why);
}  // namespace ns

namespace pf {

struct Csr { const int32_t* rowptr; const int32_t* col; const int32_t* rel; };

// the edges n -> target: [lo, hi) (contiguous, relation ascending)
__host__ __device__ static inline void edge_range(const Csr& g, int n, int target, int& lo, int& hi) {
  const int a = g.rowptr[n], b = g.rowptr[n + 1];
  int l = a, r = b;
  while (l < r) { const int m = l + ((r - l) >> 1); if (g.col[m] < target) l = m + 1; else r = m; }
  lo = l;
  r = b;
  while (l < r) { const int m = l + ((r - l) >> 1); if (g.col[m] <= target) l = m + 1; else r = m; }
  hi = l;
}

// ---- meta-paths: the closing multi-edge [lo, hi) under a pattern set.  PAT = false is the unfiltered rule: every edge of the range, the j-th one at lo + j ----
// alive: the patterns the path's earlier edges left; k: the closing edge's position
template <bool PAT>
__host__ __device__ static inline int close_count(const Csr& g, const pat::Table& pt, uint32_t alive, int k, int lo, int hi) {
  if (!PAT) return hi - lo;
  int c = 0;
  for (int e = lo; e < hi; ++e) c += pat::step(pt, alive, k, g.rel[e]) != 0;
  return c;
}
// the j-th admitted edge of the range, j < close_count (hi - 1 otherwise: never past the range)
template <bool PAT>
__host__ __device__ static inline int close_edge(const Csr& g, const pat::Table& pt, uint32_t alive, int k, int lo, int hi, int64_t j) {
  if (!PAT) return lo + (int)j;
  int e = lo;
  for (; e < hi - 1; ++e)
    if (pat::step(pt, alive, k, g.rel[e]) != 0 && j-- == 0) break;
  return e;
}
// a graph's table as the kernels take it, and the hop mask of a call on it: with patterns, an asked hop count that no pattern has yields no paths
static inline pat::Table table_of(const kprn_graph* g) {
  pat::Table t{g->pat_match, g->Vr + 1, {0, 0, 0, 0, 0, 0}};
  for (int h = 0; h <= pat::MAX_HOPS; ++h) t.len[h] = g->n_pat > 0 ? g->pat_len[h] : 0u;
  return t;
}
// a pattern set on the host (the twins): the table built from the four pattern arguments; n == 0: none
struct HostPat {
  std::vector<uint32_t> match;
  pat::Table t{nullptr, 0, {0, 0, 0, 0, 0, 0}};
  bool on = false;
  int set(const int32_t* hops, const int64_t* set_offsets, const int32_t* set_rels, int32_t n, int32_t Vr) {
    const int rc = pat::validate(hops, set_offsets, set_rels, n, Vr, nullptr);
    if (rc != KPRN_OK || n == 0) return rc;
    match.resize((size_t)pat::table_words(Vr));
    pat::build(hops, set_offsets, set_rels, n, Vr, match.data(), t.len);
    t.match = match.data(); t.stride = Vr + 1; on = true;
    return KPRN_OK;
  }
};

struct Fmt { const int32_t* types; int nT, Vt, Ve, Vr, T, F, end_rel; };
constexpr int TPB = 256;

// one path's [T][F] row: left padding (Vt .., Ve, Vr), then (types of n_k, n_k, r_k), the last step with #END_RELATION; leading columns = Vt
__host__ __device__ static inline void write_row(const Fmt& f, int32_t* row, int h, const int* nodes, const int* rels) {
  const int pad = f.T - (h + 1), lead = f.F - f.nT - 2;
  for (int t = 0; t < f.T; ++t) {
    int32_t* s = row + t * f.F;
    const int k = t - pad;
    for (int c = 0; c < lead; ++c) s[c] = f.Vt;
    if (k < 0) {
      for (int c = 0; c < f.nT; ++c) s[lead + c] = f.Vt;
      s[f.F - 2] = f.Ve; s[f.F - 1] = f.Vr;
    } else {
      const int n = nodes[k];
      for (int c = 0; c < f.nT; ++c) s[lead + c] = f.types[(int64_t)(n - 1) * f.nT + c];
      s[f.F - 2] = n; s[f.F - 1] = k < h ? rels[k] : f.end_rel;
    }
  }
}

// sum over the workgroup; every thread gets it.  sh [TPB]
__device__ static inline int64_t block_sum(int64_t v, int64_t* sh) {
  __syncthreads();   // (sh may still be read from the previous use)
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int d = TPB / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  return sh[0];
}
// exclusive prefix over the workgroup in thread order; total = the sum.  sh [TPB]
__device__ static inline int64_t block_scan_excl(int64_t v, int64_t* sh, int64_t& total) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int d = 1; d < TPB; d <<= 1) {
    const int64_t t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  total = sh[TPB - 1];
  return sh[threadIdx.x] - v;
}

// ---- the cap (include/kprn.h "finding a pair's paths", cap) ----------------------------------------------------------------------------------
// Which min(found, max_paths) ranks of a pair's path sequence are kept.  CAP_FIRST: the first ones.  CAP_SPREAD: one rank drawn in each of max_paths strata
// of [0, found), addressed by the pair-list row and the stratum, so any selection can be rebuilt anywhere.  One definition serves the rank kernel
// (path_find.hip k_cap_ranks), the fill kernels and the host twin.
constexpr int CAP_FIRST = 0, CAP_SPREAD = 1;
constexpr uint32_t CAP_COUNTER = 131072u;              // second counter word: apart from the negative sampler's n <= 255 and the walks' 65536 + h
constexpr int64_t CAP_MAX_FOUND = (int64_t)1 << 51;    // j * found stays below 2^63 for j <= 4096

KPRN_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the rank kept row j holds, of a pair in row b with F paths under a cap of K: j itself while everything fits, else the draw of stratum j
KPRN_HD int64_t cap_rank(int64_t F, int64_t K, int64_t j, int b, uint32_t k0, uint32_t k1, uint32_t draw) {
  if (F <= K) return j;
  const int64_t lo = j * F / K, hi = (j + 1) * F / K;
  uint32_t w[4];
  philox::philox4x32_10((uint32_t)(j >> 1), CAP_COUNTER, (uint32_t)b, draw, k0, k1, w);
  const uint64_t x = ((uint64_t)w[2 * (j & 1)] << 32) | w[2 * (j & 1) + 1];
  return lo + (int64_t)mulhi64(x, (uint64_t)(hi - lo));
}

// a pair's kept ranks as the fill passes see them: ranks [cap] strictly ascending, kept row j = the path of rank ranks[j]; ranks == NULL: row j = rank j
struct Keep { const int64_t* ranks; int64_t cap; };
KPRN_HD int64_t keep_rank(const Keep& k, int64_t j) { return k.ranks ? k.ranks[j] : j; }
// the first kept row at or after row `from` whose rank is >= r; cap: none.  A run of c paths from rank r on owns the rows from there while keep_rank < r + c
KPRN_HD int64_t keep_lower(const Keep& k, int64_t r, int64_t from = 0) {
  if (!k.ranks) return r < k.cap ? (r > from ? r : from) : k.cap;
  int64_t l = from, h = k.cap;
  while (l < h) { const int64_t m = l + ((h - l) >> 1); if (k.ranks[m] < r) l = m + 1; else h = m; }
  return l;
}

// ---- the build's pieces that an update of the graph runs again over its delta (path_find.hip; graph_update.hip) ----
static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }
// temporaries of one build or update, freed whatever happens
struct Tmp {
  std::vector<void*> v;
  ~Tmp() { for (void* p : v) hipFree(p); }
  template <typename T> T* get(int64_t n) {
    void* p = nullptr;
    if (kprn_dev_malloc(&p, (size_t)std::max<int64_t>(n, 1) * sizeof(T)) != hipSuccess) throw KprnError{KPRN_E_NOMEM, "hipMalloc failed (graph build)"};
    v.push_back(p);
    return (T*)p;
  }
};
// the build's order and dedupe over E >= 1 edges already in HBM: see path_find.hip
void sort_dedupe(Tmp& tmp, hipStream_t s, int32_t* d_src, int32_t* d_dst, int32_t* d_rel, int64_t E, int32_t Ve, int32_t Vr, unsigned long long** key_out,
                 int32_t** n_out);

// ---- host twins: the same rule over a CSR built by std::sort --------------------------------------------------------------------------------
// the build rule: the edges less self-loops and exact duplicates, ascending by (src, dst, rel)
typedef std::tuple<int32_t, int32_t, int32_t> HostEdge;
static inline std::vector<HostEdge> host_edges(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E) {
  std::vector<HostEdge> ed;
  ed.reserve((size_t)E);
  for (int64_t e = 0; e < E; ++e) if (src[e] != dst[e]) ed.emplace_back(src[e], dst[e], rel[e]);
  std::sort(ed.begin(), ed.end());
  ed.erase(std::unique(ed.begin(), ed.end()), ed.end());
  return ed;
}
struct HostCsr { std::vector<int32_t> rowptr, col, rel; };
static inline HostCsr host_csr(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve) {
  const std::vector<HostEdge> ed = host_edges(src, dst, rel, E);
  HostCsr g;
  g.rowptr.assign((size_t)Ve + 2, 0);
  g.col.resize(ed.size() + 1); g.rel.resize(ed.size() + 1);
  for (size_t e = 0; e < ed.size(); ++e) { g.rowptr[(size_t)std::get<0>(ed[e]) + 1]++; g.col[e] = std::get<1>(ed[e]); g.rel[e] = std::get<2>(ed[e]); }
  for (size_t n = 0; n + 1 < g.rowptr.size(); ++n) g.rowptr[n + 1] += g.rowptr[n];
  return g;
}

template <class Fn>
static void parallel_pairs(int32_t B, int threads, Fn&& fn) {
  const int nth = std::max(1, std::min(threads, (int)B));
  if (nth == 1) { for (int32_t b = 0; b < B; ++b) fn(b); return; }
  std::atomic<int32_t> next{0};   // (which thread takes a pair changes nothing a pair computes)
  std::vector<std::thread> th;
  for (int t = 0; t < nth; ++t)
    th.emplace_back([&] { for (int32_t b = next.fetch_add(1); b < B; b = next.fetch_add(1)) fn(b); });
  for (auto& t : th) t.join();
}

// The finder's two passes over B pairs whose list stage(d_pairs, s) queues into HBM on the handle's stream -- a copy from the host (kprn_find_paths) or the
// kernels that form it there (kprn_find_training_paths); a pair's item may be 0 = no item (the pair counts no paths), its user is a node.  pairs_out
// (or NULL): the list back on the host, [B][2].  Everything else as kprn_find_paths.
// sm (or NULL = hops 1..3 only, the first paths kept): the sampled hops 4 and 5 (path_walk.hip) follow the exhaustive ones in every pair's rows where the
// hops ask for them, and sm->cap_mode says which paths the cap keeps.
typedef std::function<void(int32_t* d_pairs, hipStream_t s)> StagePairs;
// walks per pair and hop count; Philox key = the seed's halves; cap_mode: which of a pair's paths the cap keeps (CAP_FIRST | CAP_SPREAD, below)
struct Sampling { int32_t walks; uint32_t k0, k1, draw; int32_t cap_mode; };
static inline Sampling sampling_of(int32_t walks, uint64_t seed, uint32_t draw, int32_t cap_mode = 0) {
  return Sampling{walks, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), draw, cap_mode};
}
constexpr int MAX_WALKS = 256, HOPS_SAMPLED = 8 | 16;   // (bits of the hop mask: bit h - 1 = paths of h hops are asked for)
static inline int hop_mask(int min_hops, int max_hops) { int m = 0; for (int h = min_hops; h <= max_hops; ++h) m |= 1 << (h - 1); return m; }
void find_staged(kprn_handle* h, const kprn_graph* g, const StagePairs& stage, const float* labels, int32_t B, int32_t min_hops, int32_t max_hops,
                 int32_t max_paths, int32_t T, const Sampling* sm, int32_t* pairs_out, int32_t* counts, int64_t* found, kprn_batch** out);
// hops / max_paths / T of a find call (KPRN_E_ARG), before anything is staged; sm == NULL: max_hops <= 3, else max_hops <= 5 and walks in 1..256 past 3 hops
int validate_find_limits(int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, const Sampling* sm, std::string* why);
int validate_find(const int32_t* pairs, int32_t B, int32_t Ve, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, const Sampling* sm, std::string* why);
// the host twin's body (kprn_host_find_paths and kprn_host_find_paths_sampled)
int host_find(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr, int32_t Vt, int32_t num_types,
              int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, int32_t F, const Sampling* sm,
              int32_t threads, int32_t* counts, int64_t* found, int32_t* idx, const pat::Table* pt = nullptr);
// what a device find call hands find_staged: the caller's sampling (or NULL) where the handle keeps the first paths, else `spread` = the same walks, seed and
// draw with the cap mode of option "path_cap"
static inline const Sampling* with_cap(const kprn_handle* h, const Sampling* sm, uint64_t seed, uint32_t draw, Sampling& spread) {
  if (h->path_cap == CAP_FIRST) return sm;
  spread = sampling_of(sm ? sm->walks : 0, seed, draw, h->path_cap);
  return &spread;
}

// ---- the sampled hops (path_walk.hip; include/kprn.h "sampled paths of four and five hops") ----
// pt (or NULL = no patterns): the graph's table; a walk's paths are then those of its closes that match
// per-walk path counts wc [B][2][walks] (slot 0 = 4 hops, 1 = 5 hops; 0 for a dead or dropped walk or a hop count hmask leaves out) and their sums wsum [B][2]
void walk_count_launch(const Csr& g, const int32_t* d_pairs, int32_t B, int hmask, const Sampling& sm, int64_t* d_wc, int64_t* d_wsum, hipStream_t s,
                       const pat::Table* pt);
// the kept sampled rows of every pair, ranks from tot[4 b + 3] (the pair's exhaustive paths) on; d_keep (or NULL = the first cnt[b] ranks): every pair's kept
// ranks at its first row; flag as k_fill's
void walk_fill_launch(const Csr& g, const Fmt& f, const int32_t* d_pairs, int32_t B, const Sampling& sm, const int64_t* d_tot, const int64_t* d_wc,
                      const int64_t* d_first, const int32_t* d_cnt, const int64_t* d_keep, int32_t* idx, int32_t* d_flag, hipStream_t s, const pat::Table* pt);
// the same on the host for row b: wc [2][walks] -> the two sums in s2; the kept rows of rank base and above -> the rows written
void host_walk_counts(const Csr& g, int u, int i, int b, int hmask, const Sampling& sm, int64_t* wc, int64_t* s2, const pat::Table* pt);
int64_t host_walk_fill(const Csr& g, const Fmt& f, int u, int i, int b, const Sampling& sm, const int64_t* wc, int64_t base, const Keep& keep, int32_t* out,
                       const pat::Table* pt);

}  // namespace pf
