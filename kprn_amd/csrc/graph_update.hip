// Graph update (include/kprn.h "updating a graph in place"): a stored graph S, the removals D and the additions A of one call -> the CSR kprn_graph_create would
// store for (S \ D) u A, bit for bit, by merging the small sorted delta into the large sorted CSR: one streaming pass over E instead of the build's sorts over E.
// Integers only; plain vector stores; every destination is a rank from two prefix sums, never an atomic counter: nothing depends on timing.
//   additions   uploaded, put in the build's (src, dst, rel) order and deduped by the build's own passes (path_find.hip sort_dedupe) over n_add elements
//   k_mark_removed        a thread per removal: pf::edge_range on the stored CSR, then the relation inside the range (rel == 0: the whole range) -> dead [e] = 1
//                         (several threads may store the same 1 into the same byte)
//   k_adds_against_graph  a later launch, a thread per distinct addition: the same search.  pos [j] = the stored edges whose key is below the addition's (its
//                         lower bound in the CSR: non-decreasing in j).  Found stored at e: dead [e] is cleared -- removals first, then additions: an edge
//                         named in both is stored afterwards -- readd [j] = what dead [e] was, and the addition is dropped from the merge; else keep_add [j] = 1
//   scans       alive_prefix [E + 1] over !dead and add_prefix [nA + 1] over keep_add (rocprim exclusive scans; the last entries are the totals)
//   k_merge     the only pass over E, a thread per stored edge and then a thread per addition:
//                 a surviving stored edge e -> alive_prefix [e] + (kept additions with a smaller key).  A kept addition's key is no stored key, so it is smaller
//                 than e's exactly when pos [j] <= e: the count is add_prefix [first j with pos [j] > e], a search over pos by the edge's OWN INDEX.  The stored
//                 edges' sources are never needed, so neither a search in rowptr nor a walk by rows is made.  A workgroup's 256 consecutive edges search only
//                 the window of pos between the bounds of its first and last edge, which two threads find first: with a delta of 1 % that window holds a few entries
//                 a kept addition j -> add_prefix [j] + alive_prefix [pos [j]]
//               col / rel are read in order (coalesced); the destinations of consecutive threads ascend.  A destination outside [0, E_new) is not written and sets
//               the flag; every workgroup stores the number of edges it placed, and their sum must be E_new (else KPRN_E_DEVICE, the old arrays stay)
//   k_rowptr_update       a thread per node: rowptr' [n] = alive_prefix [rowptr [n]] + add_prefix [first addition whose source is >= n]
// The host twin applies the same rule with std::sort and std::set_union over tuples (no handle, no GPU).
#include "path_find_dev.h"

#include <climits>
#include <iterator>

#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace pf {

struct NotDead { __host__ __device__ int32_t operator()(uint8_t d) const { return d ? 0 : 1; } };

// the first edge of [lo, hi) (relations ascending) whose relation is >= r
__host__ __device__ static inline int rel_lower(const Csr& g, int lo, int hi, int r) {
  int l = lo, h = hi;
  while (l < h) { const int m = l + ((h - l) >> 1); if (g.rel[m] < r) l = m + 1; else h = m; }
  return l;
}

__global__ __launch_bounds__(TPB) void k_mark_removed(Csr g, const int32_t* __restrict__ ds, const int32_t* __restrict__ dd, const int32_t* __restrict__ dr,
                                                      int64_t n, uint8_t* __restrict__ dead) {
  const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (j >= n) return;
  int lo, hi;
  edge_range(g, ds[j], dd[j], lo, hi);
  const int r = dr[j];
  if (r == 0) { for (int e = lo; e < hi; ++e) dead[e] = 1; return; }
  const int e = rel_lower(g, lo, hi, r);
  if (e < hi && g.rel[e] == r) dead[e] = 1;
}

// akey / arel [nA]: the distinct additions in the build's order; keep_add has nA + 1 entries (the last one 0: the scan's total lands behind it)
__global__ __launch_bounds__(TPB) void k_adds_against_graph(Csr g, const unsigned long long* __restrict__ akey, const int32_t* __restrict__ arel, int64_t nA,
                                                            uint8_t* __restrict__ dead, int32_t* __restrict__ pos, int32_t* __restrict__ keep_add,
                                                            int32_t* __restrict__ readd) {
  const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (j > nA) return;
  if (j == nA) { keep_add[j] = 0; return; }
  const unsigned long long k = akey[j];
  int lo, hi;
  edge_range(g, (int)(uint32_t)(k >> 32), (int)(uint32_t)k, lo, hi);
  const int r = arel[j], e = rel_lower(g, lo, hi, r);
  const bool stored = e < hi && g.rel[e] == r;
  pos[j] = e;
  readd[j] = stored ? (int32_t)dead[e] : 0;
  keep_add[j] = stored ? 0 : 1;
  if (stored) dead[e] = 0;   // (distinct additions name distinct edges: no two threads meet here)
}

// the first j of [l, h) with pos [j] > e (h: none)
__device__ static inline int64_t pos_upper(const int32_t* __restrict__ pos, int64_t l, int64_t h, int64_t e) {
  while (l < h) { const int64_t m = l + ((h - l) >> 1); if (pos[m] <= e) l = m + 1; else h = m; }
  return l;
}

__global__ __launch_bounds__(TPB) void k_merge(Csr g, int64_t E, const uint8_t* __restrict__ dead, const int32_t* __restrict__ alive_prefix,
                                               const unsigned long long* __restrict__ akey, const int32_t* __restrict__ arel, const int32_t* __restrict__ pos,
                                               const int32_t* __restrict__ keep_add, const int32_t* __restrict__ add_prefix, int64_t nA, int64_t E_new,
                                               int32_t* __restrict__ col2, int32_t* __restrict__ rel2, int64_t* __restrict__ placed_blk, int32_t* flag) {
  __shared__ int64_t sh[TPB];
  __shared__ int64_t win[2];
  const int64_t first = (int64_t)blockIdx.x * TPB, t = first + threadIdx.x;
  // the window of pos this workgroup's stored edges fall into (workgroup-uniform; a workgroup behind E has none)
  if (first < E && threadIdx.x < 2) win[threadIdx.x] = pos_upper(pos, 0, nA, threadIdx.x == 0 ? first - 1 : (first + TPB < E ? first + TPB : E) - 1);
  __syncthreads();
  int64_t placed = 0, d = -1;
  int32_t c = 0, r = 0;
  if (t < E) {
    if (!dead[t]) { d = (int64_t)alive_prefix[t] + add_prefix[pos_upper(pos, win[0], win[1], t)]; c = g.col[t]; r = g.rel[t]; }
  } else if (t - E < nA) {
    const int64_t j = t - E;
    if (keep_add[j]) { d = (int64_t)add_prefix[j] + alive_prefix[pos[j]]; c = (int32_t)(uint32_t)akey[j]; r = arel[j]; }
  }
  if (d >= 0) {
    if (d < E_new) { col2[d] = c; rel2[d] = r; placed = 1; }
    else atomicOr(flag, 1);
  }
  placed = block_sum(placed, sh);
  if (threadIdx.x == 0) placed_blk[blockIdx.x] = placed;
}

__global__ __launch_bounds__(TPB) void k_rowptr_update(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ alive_prefix,
                                                       const unsigned long long* __restrict__ akey, const int32_t* __restrict__ add_prefix, int64_t nA, int32_t Ve,
                                                       int32_t* __restrict__ rowptr2) {
  const int64_t n = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (n > Ve) return;
  const unsigned long long want = (unsigned long long)n << 32;
  int64_t l = 0, h = nA;
  while (l < h) { const int64_t m = l + ((h - l) >> 1); if (akey[m] < want) l = m + 1; else h = m; }
  rowptr2[n] = alive_prefix[rowptr[n]] + add_prefix[l];
}

// entity ent [k]'s type row <- rows [k]
__global__ __launch_bounds__(TPB) void k_set_types(const int32_t* __restrict__ ent, const int32_t* __restrict__ rows, int64_t n, int nT, int32_t* __restrict__ types) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= n * nT) return;
  types[(int64_t)(ent[t / nT] - 1) * nT + t % nT] = rows[t];
}

// ---- the refusals of a delta, shared by kprn_graph_update and the host twin ----
static int validate_delta(const int32_t* as, const int32_t* ad, const int32_t* ar, int64_t n_add, const int32_t* ds, const int32_t* dd, const int32_t* dr,
                          int64_t n_del, int32_t Ve, int32_t Vr, std::string* why) {
  auto bad = [&](int code, const char* t) { if (why) *why = t; return code; };
  if (n_add < 0 || n_add > 0x7fffffffLL || n_del < 0 || n_del > 0x7fffffffLL) return bad(KPRN_E_ARG, "n_add and n_del must be in 0 .. 2^31 - 1");
  if ((n_add > 0 && (!as || !ad || !ar)) || (n_del > 0 && (!ds || !dd || !dr))) return bad(KPRN_E_ARG, "a delta array is NULL with a positive count");
  for (int64_t k = 0; k < n_add; ++k) {
    if (as[k] < 1 || as[k] >= Ve || ad[k] < 1 || ad[k] >= Ve) return bad(KPRN_E_INDEX, "an added edge's node is outside 1..Ve-1 (Ve is the pad row)");
    if (ar[k] < 1 || ar[k] > Vr) return bad(KPRN_E_INDEX, "an added edge's relation is outside 1..Vr");
  }
  for (int64_t k = 0; k < n_del; ++k) {
    if (ds[k] < 1 || ds[k] >= Ve || dd[k] < 1 || dd[k] >= Ve) return bad(KPRN_E_INDEX, "a removed edge's node is outside 1..Ve-1 (Ve is the pad row)");
    if (dr[k] < 0 || dr[k] > Vr) return bad(KPRN_E_INDEX, "a removed edge's relation is outside 0..Vr (0 = every relation)");
  }
  return KPRN_OK;
}

template <typename T>
static T* upload(Tmp& tmp, const T* src, int64_t n, hipStream_t s) {
  T* d = tmp.get<T>(n);
  if (n > 0) HIP_TRY(hipMemcpyAsync(d, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, s));
  return d;
}

static void update_graph(kprn_handle* h, kprn_graph* g, const int32_t* as, const int32_t* ad, const int32_t* ar, int64_t n_add, const int32_t* ds,
                         const int32_t* dd, const int32_t* dr, int64_t n_del, int64_t* n_added, int64_t* n_removed) {
  hipStream_t s = h->stream;
  const int64_t E = g->E;
  sync_all_streams(h);   // (nothing queued anywhere reads the arrays that are about to be replaced)
  Tmp tmp;
  const Csr csr{g->rowptr, g->col, g->rel};
  // 1. the additions in the build's order, deduped; nothing touches E yet
  int64_t nA = 0;
  unsigned long long* akey = nullptr;
  int32_t* acol = nullptr; int32_t* arel = nullptr;
  if (n_add > 0) {
    acol = upload(tmp, as, n_add, s); arel = upload(tmp, ad, n_add, s);
    int32_t* d_rel = upload(tmp, ar, n_add, s);
    int32_t* d_n = nullptr;
    sort_dedupe(tmp, s, acol, arel, d_rel, n_add, g->Ve, g->Vr, &akey, &d_n);   // (acol = destinations, arel = relations from here on)
    int32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, d_n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    KPRN_REQUIRE(n >= 0 && n <= n_add, KPRN_E_DEVICE, "graph update: the compaction returned an impossible number of additions");
    nA = n;
  } else {
    akey = tmp.get<unsigned long long>(1); arel = tmp.get<int32_t>(1);
  }
  // 2. / 3. removals, then additions against the stored graph
  uint8_t* dead = tmp.get<uint8_t>(E + 1);
  int32_t* pos = tmp.get<int32_t>(nA); int32_t* keep_add = tmp.get<int32_t>(nA + 1); int32_t* readd = tmp.get<int32_t>(nA);
  int32_t* alive_prefix = tmp.get<int32_t>(E + 1); int32_t* add_prefix = tmp.get<int32_t>(nA + 1);
  int64_t* d_sum = tmp.get<int64_t>(2);
  int32_t* d_flag = tmp.get<int32_t>(1);
  if (E > 0) HIP_TRY(hipMemsetAsync(dead, 0, (size_t)E, s));
  HIP_TRY(hipMemsetAsync(dead + E, 1, 1, s));            // (the entry behind the last edge counts as not alive: alive_prefix [E] = the total)
  HIP_TRY(hipMemsetAsync(d_sum, 0, 2 * sizeof(int64_t), s));
  HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
  if (n_del > 0) {
    const int32_t* d_ds = upload(tmp, ds, n_del, s); const int32_t* d_dd = upload(tmp, dd, n_del, s); const int32_t* d_dr = upload(tmp, dr, n_del, s);
    hipLaunchKernelGGL(k_mark_removed, dim3(blocks_for(n_del)), dim3(TPB), 0, s, csr, d_ds, d_dd, d_dr, n_del, dead);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_adds_against_graph, dim3(blocks_for(nA + 1)), dim3(TPB), 0, s, csr, akey, arel, nA, dead, pos, keep_add, readd);
  HIP_TRY(hipGetLastError());
  // 4. the two scans, and the additions that put a removed edge back
  const rocprim::transform_iterator<const uint8_t*, NotDead, int32_t> alive(dead, NotDead());
  size_t need1 = 0, need2 = 0, need3 = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, need1, alive, alive_prefix, (int32_t)0, (size_t)E + 1, rocprim::plus<int32_t>(), s));
  HIP_TRY(rocprim::exclusive_scan(nullptr, need2, keep_add, add_prefix, (int32_t)0, (size_t)nA + 1, rocprim::plus<int32_t>(), s));
  HIP_TRY(rocprim::reduce(nullptr, need3, readd, d_sum, (int64_t)0, (size_t)std::max<int64_t>(nA, 1), rocprim::plus<int64_t>(), s));
  const unsigned mblocks = blocks_for(E + nA);
  int64_t* placed_blk = tmp.get<int64_t>(mblocks);
  size_t need4 = 0;
  HIP_TRY(rocprim::reduce(nullptr, need4, placed_blk, d_sum + 1, (int64_t)0, (size_t)std::max(mblocks, 1u), rocprim::plus<int64_t>(), s));
  const size_t need = std::max(std::max(need1, need2), std::max(need3, need4));
  char* work = tmp.get<char>((int64_t)need);
  size_t nb = need;
  HIP_TRY(rocprim::exclusive_scan(work, nb, alive, alive_prefix, (int32_t)0, (size_t)E + 1, rocprim::plus<int32_t>(), s));
  nb = need;
  HIP_TRY(rocprim::exclusive_scan(work, nb, keep_add, add_prefix, (int32_t)0, (size_t)nA + 1, rocprim::plus<int32_t>(), s));
  if (nA > 0) { nb = need; HIP_TRY(rocprim::reduce(work, nb, readd, d_sum, (int64_t)0, (size_t)nA, rocprim::plus<int64_t>(), s)); }
  int32_t n_alive = 0, n_kept = 0;
  int64_t n_readd = 0;
  HIP_TRY(hipMemcpyAsync(&n_alive, alive_prefix + E, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&n_kept, add_prefix + nA, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&n_readd, d_sum, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  KPRN_REQUIRE(n_alive >= 0 && n_alive <= E && n_kept >= 0 && n_kept <= nA && n_readd >= 0 && n_readd <= nA - n_kept, KPRN_E_DEVICE,
               "graph update: the counting pass returned an impossible count");
  const int64_t E_new = (int64_t)n_alive + n_kept;
  KPRN_REQUIRE(E_new <= 0x7fffffffLL, KPRN_E_ARG, "graph update: the updated graph would hold more than 2^31 - 1 edges");
  // 5. - 7. the merge into fresh arrays, the row pointers, the swap
  int32_t* col2 = nullptr; int32_t* rel2 = nullptr; int32_t* rowptr2 = nullptr;
  try {
    col2 = dalloc<int32_t>(std::max<int64_t>(E_new, 1)); rel2 = dalloc<int32_t>(std::max<int64_t>(E_new, 1)); rowptr2 = dalloc<int32_t>((int64_t)g->Ve + 1);
    int64_t placed = 0;
    int32_t flag = 0;
    if (mblocks > 0) {
      hipLaunchKernelGGL(k_merge, dim3(mblocks), dim3(TPB), 0, s, csr, E, dead, alive_prefix, akey, arel, pos, keep_add, add_prefix, nA, E_new, col2, rel2,
                         placed_blk, d_flag);
      HIP_TRY(hipGetLastError());
      nb = need; HIP_TRY(rocprim::reduce(work, nb, placed_blk, d_sum + 1, (int64_t)0, (size_t)mblocks, rocprim::plus<int64_t>(), s));
    }
    hipLaunchKernelGGL(k_rowptr_update, dim3(blocks_for((int64_t)g->Ve + 1)), dim3(TPB), 0, s, g->rowptr, alive_prefix, akey, add_prefix, nA, g->Ve, rowptr2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&placed, d_sum + 1, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    KPRN_REQUIRE(flag == 0 && placed == E_new, KPRN_E_DEVICE, "graph update: the merge placed a different number of edges than the counting pass found");
  } catch (...) {
    dfree(col2); dfree(rel2); dfree(rowptr2);
    throw;
  }
  std::swap(g->col, col2); std::swap(g->rel, rel2); std::swap(g->rowptr, rowptr2);
  g->E = E_new;
  dfree(col2); dfree(rel2); dfree(rowptr2);   // (the old arrays: the streams were drained, and this call's kernels have finished)
  if (n_added) *n_added = (int64_t)n_kept + n_readd;
  if (n_removed) *n_removed = (E - n_alive) + n_readd;
}

// ---- host twin ----
static int host_update(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, int32_t Vr, const int32_t* as, const int32_t* ad,
                       const int32_t* ar, int64_t n_add, const int32_t* ds, const int32_t* dd, const int32_t* dr, int64_t n_del, int32_t* rowptr, int32_t* col,
                       int32_t* rel_out, int64_t* E_out, int64_t* n_added, int64_t* n_removed) {
  if (E < 0 || E > 0x7fffffffLL || (E > 0 && (!src || !dst || !rel)) || Ve < 2 || Vr < 1 || !rowptr || !col || !rel_out || !E_out) return KPRN_E_ARG;
  for (int64_t e = 0; e < E; ++e)
    if (src[e] < 1 || src[e] >= Ve || dst[e] < 1 || dst[e] >= Ve || rel[e] < 1 || rel[e] > Vr) return KPRN_E_INDEX;
  const int rc = validate_delta(as, ad, ar, n_add, ds, dd, dr, n_del, Ve, Vr, nullptr);
  if (rc != KPRN_OK) return rc;
  try {
    const std::vector<HostEdge> S = host_edges(src, dst, rel, E), A = host_edges(as, ad, ar, n_add);
    std::vector<char> dead(S.size(), 0);
    for (int64_t k = 0; k < n_del; ++k) {   // rel == 0: the run of (s, d, *); else the one edge
      auto lo = std::lower_bound(S.begin(), S.end(), HostEdge(ds[k], dd[k], dr[k] == 0 ? INT32_MIN : dr[k]));
      auto hi = std::upper_bound(lo, S.end(), HostEdge(ds[k], dd[k], dr[k] == 0 ? INT32_MAX : dr[k]));
      std::fill(dead.begin() + (lo - S.begin()), dead.begin() + (hi - S.begin()), 1);
    }
    std::vector<HostEdge> alive, out;
    for (size_t e = 0; e < S.size(); ++e) if (!dead[e]) alive.push_back(S[e]);
    std::set_union(alive.begin(), alive.end(), A.begin(), A.end(), std::back_inserter(out));
    if (out.size() > (size_t)0x7fffffff) return KPRN_E_ARG;
    for (int32_t n = 0; n <= Ve; ++n) rowptr[n] = 0;
    for (size_t e = 0; e < out.size(); ++e) { col[e] = std::get<1>(out[e]); rel_out[e] = std::get<2>(out[e]); if (std::get<0>(out[e]) < Ve) rowptr[std::get<0>(out[e]) + 1]++; }
    for (int32_t n = 0; n < Ve; ++n) rowptr[n + 1] += rowptr[n];
    *E_out = (int64_t)out.size();
    if (n_added) *n_added = (int64_t)(out.size() - alive.size());
    if (n_removed) *n_removed = (int64_t)(S.size() - alive.size());
  } catch (...) { return KPRN_E_NOMEM; }
  return KPRN_OK;
}

}  // namespace pf

static bool graph_of(kprn_handle* h, const kprn_graph* g) { return g && std::find(h->graphs.begin(), h->graphs.end(), g) != h->graphs.end(); }

extern "C" {

int kprn_graph_update(kprn_handle* h, kprn_graph* g, const int32_t* add_src, const int32_t* add_dst, const int32_t* add_rel, int64_t n_add,
                      const int32_t* del_src, const int32_t* del_dst, const int32_t* del_rel, int64_t n_del, int64_t* n_added, int64_t* n_removed) {
  API_BEGIN(h)
  KPRN_REQUIRE(graph_of(h, g), KPRN_E_ARG, "g is not a graph of this handle");
  std::string why;
  const int rc = pf::validate_delta(add_src, add_dst, add_rel, n_add, del_src, del_dst, del_rel, n_del, g->Ve, g->Vr, &why);   // (before anything is queued)
  if (rc != KPRN_OK) throw KprnError{rc, why};
  if (n_add == 0 && n_del == 0) {
    if (n_added) *n_added = 0;
    if (n_removed) *n_removed = 0;
  } else {
    pf::update_graph(h, g, add_src, add_dst, add_rel, n_add, del_src, del_dst, del_rel, n_del, n_added, n_removed);
  }
  API_END(h)
}

int kprn_graph_read(kprn_handle* h, const kprn_graph* g, int32_t* rowptr, int32_t* col, int32_t* rel) {
  API_BEGIN(h)
  KPRN_REQUIRE(graph_of(h, g), KPRN_E_ARG, "g is not a graph of this handle");
  KPRN_REQUIRE(rowptr && (g->E == 0 || (col && rel)), KPRN_E_ARG, "rowptr / col / rel is NULL");
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(rowptr, g->rowptr, ((size_t)g->Ve + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (g->E > 0) {
    HIP_TRY(hipMemcpyAsync(col, g->col, (size_t)g->E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(rel, g->rel, (size_t)g->E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  API_END(h)
}

int kprn_graph_set_node_types(kprn_handle* h, kprn_graph* g, const int32_t* entities, const int32_t* rows, int64_t n) {
  API_BEGIN(h)
  KPRN_REQUIRE(graph_of(h, g), KPRN_E_ARG, "g is not a graph of this handle");
  KPRN_REQUIRE(n >= 0 && n < g->Ve && (n == 0 || (entities && rows)), KPRN_E_ARG, "entities / rows is NULL, or n is outside 0..Ve-1");
  for (int64_t k = 0; k < n; ++k) KPRN_REQUIRE(entities[k] >= 1 && entities[k] < g->Ve, KPRN_E_INDEX, "an entity is outside 1..Ve-1 (Ve is the pad row)");
  for (int64_t k = 0; k < n * g->nT; ++k) KPRN_REQUIRE(rows[k] >= 1 && rows[k] <= g->Vt, KPRN_E_INDEX, "a type id is outside 1..Vt");
  std::vector<int32_t> seen(entities, entities + n);
  std::sort(seen.begin(), seen.end());
  KPRN_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), KPRN_E_ARG, "an entity is listed twice");
  if (n > 0) {
    hipStream_t s = h->stream;
    pf::Tmp tmp;
    const int32_t* d_ent = pf::upload(tmp, entities, n, s);
    const int32_t* d_rows = pf::upload(tmp, rows, n * g->nT, s);
    hipLaunchKernelGGL(pf::k_set_types, dim3(pf::blocks_for(n * g->nT)), dim3(pf::TPB), 0, s, d_ent, d_rows, n, g->nT, g->types);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));   // (the staged copies leave scope)
  }
  API_END(h)
}

int kprn_host_graph_update(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, int32_t Vr, const int32_t* add_src,
                           const int32_t* add_dst, const int32_t* add_rel, int64_t n_add, const int32_t* del_src, const int32_t* del_dst, const int32_t* del_rel,
                           int64_t n_del, int32_t* rowptr, int32_t* col, int32_t* rel_out, int64_t* E_out, int64_t* n_added, int64_t* n_removed) {
  return pf::host_update(src, dst, rel, E, Ve, Vr, add_src, add_dst, add_rel, n_add, del_src, del_dst, del_rel, n_del, rowptr, col, rel_out, E_out, n_added,
                         n_removed);
}

}  // extern "C"
