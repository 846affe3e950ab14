// What the path finder (path_find.hip) and the negative sampler (neg_sample.hip) share: the graph in HBM, the CSR view both walk (namespace pf,
// __host__ __device__), the host CSR of the twins and their thread loop.
#pragma once
#include "kprn_internal.h"

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
};

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

// ---- host twins: the same rule over a CSR built by std::sort --------------------------------------------------------------------------------
struct HostCsr { std::vector<int32_t> rowptr, col, rel; };
static inline HostCsr host_csr(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve) {
  std::vector<std::tuple<int32_t, int32_t, int32_t>> ed;
  ed.reserve((size_t)E);
  for (int64_t e = 0; e < E; ++e) if (src[e] != dst[e]) ed.emplace_back(src[e], dst[e], rel[e]);
  std::sort(ed.begin(), ed.end());
  ed.erase(std::unique(ed.begin(), ed.end()), ed.end());
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
typedef std::function<void(int32_t* d_pairs, hipStream_t s)> StagePairs;
void find_staged(kprn_handle* h, const kprn_graph* g, const StagePairs& stage, const float* labels, int32_t B, int32_t min_hops, int32_t max_hops,
                 int32_t max_paths, int32_t T, int32_t* pairs_out, int32_t* counts, int64_t* found, kprn_batch** out);
// hops / max_paths / T of a find call (KPRN_E_ARG), before anything is staged
int validate_find_limits(int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, std::string* why);

}  // namespace pf
