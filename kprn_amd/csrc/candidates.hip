// Candidates of a user (include/kprn.h "candidates of a user"): for B users, the members of a catalogue (a kprn_sampler's item list) that a path of
// min_hops .. max_hops <= 3 hops reaches from the user, less the user itself and -- on request -- the items the user is adjacent to; the (user, item) rows
// stay in HBM as the handle's candidate list, which kprn_find_paths_of_candidates hands to the finder's two passes (path_find_dev.h find_staged) without a
// trip to the host.  Integers only.
//
// One definition of the rule serves the kernels and the host twin (namespace cd, __host__ __device__):
//   walk    stored edges hold no self-loops, so "all nodes pairwise distinct" reduces to: 1 hop u -> c; 2 hops u -> a -> c, c != u; 3 hops u -> a -> b -> c,
//           b != u, c != u, c != a.  The walk runs from the user outward: deg(u) * deg(a) * deg(b) steps, whatever the catalogue's size
//   member  position of c in items [M] (ascending) by binary search, -1 = not in the catalogue
// Device: one 256-thread workgroup per user and a bitmap of W = ceil(M / 32) words per user, zeroed by a memset queued before the first kernel.
//   k_mark   the walk, spread as the finder's k_count: hops 1 and 2 a thread per first edge, hop 3 a wave per first edge with its lanes over the second edges.
//            Every end node that is a member sets its bit: a plain load first (most marks of a 3-hop walk are repeats), atomicOr where the bit is not
//            yet seen.  The result is a set: the order of the atomics cannot show, and no atomic hands out a slot or a rank
//   k_count  a thread per word: the user's own bit and, with exclude_adjacent, the bits of the members u has an edge to (edge_range per set bit) are cleared
//            and the word stored back; popcounts summed over the workgroup -> counts [B].  The host scans them into each user's first row
//   k_fill   the words 256 at a time, ranks by the workgroup's exclusive scan with the running rank carried from chunk to chunk; a thread writes the rows of
//            its own word while rank < counts[b].  The rows a workgroup placed are summed and compared with counts[b]: a disagreement sets the flag
//            (KPRN_E_DEVICE), and no write leaves the user's rows either way.
//
// The N strongest candidates of a user (include/kprn.h "the N strongest candidates of a user"; kprn_find_candidates_top): the same walk counts its marks, so
// every member gets n_paths = the finder's `found` for (u, c), and a user keeps its `cap` best by (n_paths descending, id ascending), laid out by id.  A tally
// of M 64-bit words per user takes the bitmap's place, zeroed by a memset queued before the first kernel:
//   k_tally   k_mark's spread; an end node that is a member adds 1 to its word (relaxed, agent scope).  Integer adds commute: the sums do not depend on order
//   k_settle  a thread per entry: the user's own entry and, with exclude_adjacent, the adjacent members' are zeroed with plain stores; the non-zero entries
//             summed over the workgroup -> ncand [B]
//   k_select  a user with more than cap candidates: v = its cap-th largest count by a radix select from the most significant non-zero byte of the workgroup's
//             maximum down, one 256-bin LDS histogram per byte; quota = cap - #(entries > v) of the entries equal to v are kept, lowest ids first.  Otherwise
//             v = 0: every non-zero entry is kept.  counts [B] = min(cap, ncand) goes to the host
//   k_fill_top  the entries 256 at a time, one exclusive scan per chunk over (entries > v, entries == v) packed in the halves of an int64, the rank among
//             kept rows and the rank among ties carried from chunk to chunk; a thread writes its own row and n_paths entry while rank < counts[b]; the rows
//             placed are checked against counts[b] as k_fill does.
// Meta-paths (PAT = true; path_pattern_dev.h): k_mark and k_tally mark only the ends of walks whose relation sequence matches a pattern of the graph's set.
#include "path_find_dev.h"

namespace cd {

using pf::Csr;
using pf::TPB;

__host__ __device__ static inline int member(const int32_t* items, int M, int c) {
  int l = 0, r = M;
  while (l < r) { const int m = l + ((r - l) >> 1); if (items[m] < c) l = m + 1; else r = m; }
  return (l < M && items[l] == c) ? l : -1;
}

// the end nodes of the 2-hop walks through first edge e0 (want2) and of the 3-hop walks through its second edges e1_first, e1_first + e1_step, ... (want3).
// PAT (include/kprn.h "meta-paths"): the walk carries the patterns its edges left alive, leaves an edge none of them admits -- a first edge with its whole fan --
// and marks only the ends of matching walks; PAT = false never reads pt
template <bool PAT, class Mark>
__host__ __device__ static inline void walk_edge(const Csr& g, const pat::Table& pt, int u, int e0, bool want2, bool want3, int e1_first, int e1_step, Mark&& mark) {
  const int a = g.col[e0];   // (a != u: no self-loops)
  uint32_t a2 = 0, a3 = 0;
  if (PAT) {
    a2 = pat::step(pt, pt.len[2], 0, g.rel[e0]); a3 = pat::step(pt, pt.len[3], 0, g.rel[e0]);
    want2 = want2 && a2; want3 = want3 && a3;
    if (!want2 && !want3) return;
  }
  const int end1 = g.rowptr[a + 1];
  if (want2 && e1_first == 0)
    for (int e1 = g.rowptr[a]; e1 < end1; ++e1) { const int c = g.col[e1]; if (c != u && (!PAT || pat::step(pt, a2, 1, g.rel[e1]))) mark(c); }
  if (!want3) return;
  for (int e1 = g.rowptr[a] + e1_first; e1 < end1; e1 += e1_step) {
    const int b = g.col[e1];
    if (b == u) continue;
    uint32_t al = 0;
    if (PAT) { al = pat::step(pt, a3, 1, g.rel[e1]); if (!al) continue; }
    const int end2 = g.rowptr[b + 1];
    for (int e2 = g.rowptr[b]; e2 < end2; ++e2) { const int c = g.col[e2]; if (c != u && c != a && (!PAT || pat::step(pt, al, 2, g.rel[e2]))) mark(c); }
  }
}
// the 1-hop walk over first edge e0 marks its end
template <bool PAT>
__host__ __device__ static inline bool hop1_ok(const Csr& g, const pat::Table& pt, int e0) { return !PAT || pat::step(pt, pt.len[1], 0, g.rel[e0]) != 0; }

// the walk of one user on the host: every first edge in order
template <bool PAT, class Mark>
static inline void host_walk(const Csr& g, const pat::Table& pt, int u, int hmask, Mark&& mark) {
  for (int e0 = g.rowptr[u]; e0 < g.rowptr[u + 1]; ++e0) {
    if ((hmask & 1) && hop1_ok<PAT>(g, pt, e0)) mark(g.col[e0]);
    if (hmask & 6) walk_edge<PAT>(g, pt, u, e0, (hmask & 2) != 0, (hmask & 4) != 0, 0, 1, mark);
  }
}

template <bool PAT>
__global__ __launch_bounds__(TPB) void k_mark(Csr g, pat::Table pt, const int32_t* __restrict__ items, int M, int W, const int32_t* __restrict__ users, int hmask,
                                              uint32_t* bits_all) {
  const int u = users[blockIdx.x];
  uint32_t* bits = bits_all + (int64_t)blockIdx.x * W;
  auto mark = [&](int c) {
    const int j = member(items, M, c);
    if (j < 0) return;
    const uint32_t m = 1u << (j & 31);
    if (!(bits[j >> 5] & m)) atomicOr(&bits[j >> 5], m);   // (a stale load only repeats an atomic: bits are set, never cleared, in this launch)
  };
  const int beg = g.rowptr[u], end = g.rowptr[u + 1];
  if (hmask & 1)
    for (int e0 = beg + threadIdx.x; e0 < end; e0 += TPB) if (hop1_ok<PAT>(g, pt, e0)) mark(g.col[e0]);
  if (hmask & 2)   // a thread per first edge
    for (int e0 = beg + threadIdx.x; e0 < end; e0 += TPB) walk_edge<PAT>(g, pt, u, e0, true, false, 0, 1, mark);
  if (hmask & 4) { // a wave per first edge, its lanes over the second edges
    const int lane = threadIdx.x & 63;
    for (int e0 = beg + (threadIdx.x >> 6); e0 < end; e0 += TPB / 64) walk_edge<PAT>(g, pt, u, e0, false, true, lane, 64, mark);
  }
}

__global__ __launch_bounds__(TPB) void k_count(Csr g, const int32_t* __restrict__ items, int M, int W, const int32_t* __restrict__ users, int exclude,
                                               uint32_t* bits_all, int32_t* __restrict__ counts) {
  __shared__ int64_t sh[TPB];
  const int u = users[blockIdx.x];
  uint32_t* bits = bits_all + (int64_t)blockIdx.x * W;
  const int ju = member(items, M, u);
  int64_t n = 0;
  for (int w = threadIdx.x; w < W; w += TPB) {   // a thread owns its words: plain loads and stores
    uint32_t word = bits[w];
    if (ju >= 0 && (ju >> 5) == w) word &= ~(1u << (ju & 31));
    if (exclude)
      for (uint32_t rest = word; rest; rest &= rest - 1) {
        const int bit = __ffs(rest) - 1;
        int lo, hi;
        pf::edge_range(g, u, items[32 * w + bit], lo, hi);
        if (lo != hi) word &= ~(1u << bit);
      }
    bits[w] = word;
    n += __popc(word);
  }
  n = pf::block_sum(n, sh);
  if (threadIdx.x == 0) counts[blockIdx.x] = (int32_t)n;
}

// first [b]: the user's first row in list; counts [b]: the rows it was allotted
__global__ __launch_bounds__(TPB) void k_fill(const int32_t* __restrict__ items, int W, const int32_t* __restrict__ users, const uint32_t* __restrict__ bits_all,
                                              const int64_t* __restrict__ first, const int32_t* __restrict__ counts, int32_t* __restrict__ list, int32_t* flag) {
  __shared__ int64_t sh[TPB];
  const int u = users[blockIdx.x];
  const uint32_t* bits = bits_all + (int64_t)blockIdx.x * W;
  const int64_t cap = counts[blockIdx.x];
  int32_t* out = list + 2 * first[blockIdx.x];
  int64_t run = 0, placed = 0;   // run: the rank of the next chunk's first row (workgroup-uniform, like the loop bound)
  for (int base = 0; base < W; base += TPB) {
    const int w = base + threadIdx.x;
    const uint32_t word = w < W ? bits[w] : 0u;
    int64_t sum;
    int64_t r = run + pf::block_scan_excl(__popc(word), sh, sum);
    for (uint32_t rest = word; rest && r < cap; rest &= rest - 1, ++r) {   // (out + 2 r is formed only for a rank below the cap)
      out[2 * r] = u;
      out[2 * r + 1] = items[32 * w + (__ffs(rest) - 1)];
      ++placed;
    }
    run += sum;
  }
  placed = pf::block_sum(placed, sh);
  if (threadIdx.x == 0 && placed != cap) atomicOr(flag, 1);
}

// ---- the N strongest candidates ----------------------------------------------------------------------------------------------------------------
typedef unsigned long long u64;

template <bool PAT>
__global__ __launch_bounds__(TPB) void k_tally(Csr g, pat::Table pt, const int32_t* __restrict__ items, int M, const int32_t* __restrict__ users, int hmask, u64* tally_all) {
  const int u = users[blockIdx.x];
  u64* tally = tally_all + (int64_t)blockIdx.x * M;
  auto mark = [&](int c) {
    const int j = member(items, M, c);
    if (j >= 0) __hip_atomic_fetch_add(&tally[j], (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  const int beg = g.rowptr[u], end = g.rowptr[u + 1];
  if (hmask & 1)
    for (int e0 = beg + threadIdx.x; e0 < end; e0 += TPB) if (hop1_ok<PAT>(g, pt, e0)) mark(g.col[e0]);
  if (hmask & 2)   // a thread per first edge
    for (int e0 = beg + threadIdx.x; e0 < end; e0 += TPB) walk_edge<PAT>(g, pt, u, e0, true, false, 0, 1, mark);
  if (hmask & 4) { // a wave per first edge, its lanes over the second edges
    const int lane = threadIdx.x & 63;
    for (int e0 = beg + (threadIdx.x >> 6); e0 < end; e0 += TPB / 64) walk_edge<PAT>(g, pt, u, e0, false, true, lane, 64, mark);
  }
}

__global__ __launch_bounds__(TPB) void k_settle(Csr g, const int32_t* __restrict__ items, int M, const int32_t* __restrict__ users, int exclude, u64* tally_all,
                                                int32_t* __restrict__ ncand) {
  __shared__ int64_t sh[TPB];
  const int u = users[blockIdx.x];
  u64* tally = tally_all + (int64_t)blockIdx.x * M;
  int64_t n = 0;
  for (int j = threadIdx.x; j < M; j += TPB) {   // a thread owns its entries: plain loads and stores
    if (tally[j] == 0) continue;
    const int c = items[j];
    bool out = c == u;
    if (!out && exclude) {
      int lo, hi;
      pf::edge_range(g, u, c, lo, hi);
      out = lo != hi;
    }
    if (out) tally[j] = 0; else ++n;
  }
  n = pf::block_sum(n, sh);
  if (threadIdx.x == 0) ncand[blockIdx.x] = (int32_t)n;
}

// maximum over the workgroup; every thread gets it.  sh [TPB]
__device__ static inline u64 block_max(u64 v, u64* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int d = TPB / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d && sh[threadIdx.x + d] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + d];
    __syncthreads();
  }
  return sh[0];
}

// counts [b] = min(cap, ncand [b]); cut [b] = v and quota [b]: an entry t is kept iff t > v, or t == v && t > 0 and it is among the first quota such entries
__global__ __launch_bounds__(TPB) void k_select(int M, int cap, const u64* __restrict__ tally_all, const int32_t* __restrict__ ncand, int32_t* __restrict__ counts,
                                                u64* __restrict__ cut, int32_t* __restrict__ quota) {
  __shared__ int64_t sh[TPB];
  __shared__ int hist[256];
  static_assert(TPB == 256, "one thread zeroes one bin");
  const u64* tally = tally_all + (int64_t)blockIdx.x * M;
  const int n = ncand[blockIdx.x];   // (one address for all lanes: the branches and loop bounds below are workgroup-uniform)
  if (n <= cap) {
    if (threadIdx.x == 0) { counts[blockIdx.x] = n; cut[blockIdx.x] = 0; quota[blockIdx.x] = 0; }
    return;
  }
  u64 top = 0;
  for (int j = threadIdx.x; j < M; j += TPB) top = tally[j] > top ? tally[j] : top;
  top = block_max(top, (u64*)sh);
  int d = 7;
  while (d > 0 && (top >> (8 * d)) == 0) --d;   // the bytes above the maximum's top byte are 0 in every entry
  u64 v = 0;      // the digits found so far, in place
  int k = cap;    // v is the k-th largest of the entries that agree with it above digit d (cap < n: there are at least k, and the k-th is not 0)
  for (; d >= 0; --d) {
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < M; j += TPB) {
      const u64 t = tally[j];
      if (d == 7 || (t >> (8 * (d + 1))) == (v >> (8 * (d + 1)))) atomicAdd(&hist[(int)((t >> (8 * d)) & 255)], 1);   // (integer LDS adds: any order, one sum)
    }
    __syncthreads();
    int bin = 255, above = 0;
    for (; bin > 0; --bin) {   // every thread reads the same bins: the same digit in all of them
      const int c = hist[bin];
      if (above + c >= k) break;
      above += c;
    }
    k -= above;
    v |= (u64)bin << (8 * d);
    __syncthreads();   // (hist is zeroed again by the next pass)
  }
  int64_t n_gt = 0;
  for (int j = threadIdx.x; j < M; j += TPB) n_gt += tally[j] > v;
  n_gt = pf::block_sum(n_gt, sh);
  if (threadIdx.x == 0) { counts[blockIdx.x] = cap; cut[blockIdx.x] = v; quota[blockIdx.x] = (int32_t)(cap - n_gt); }
}

// first [b]: the user's first row in list and paths; counts [b]: the rows it was allotted
__global__ __launch_bounds__(TPB) void k_fill_top(const int32_t* __restrict__ items, int M, const int32_t* __restrict__ users, const u64* __restrict__ tally_all,
                                                  const int64_t* __restrict__ first, const int32_t* __restrict__ counts, const u64* __restrict__ cut,
                                                  const int32_t* __restrict__ quota, int32_t* __restrict__ list, int64_t* __restrict__ paths, int32_t* flag) {
  __shared__ int64_t sh[TPB];
  const int u = users[blockIdx.x];
  const u64* tally = tally_all + (int64_t)blockIdx.x * M;
  const int64_t cap = counts[blockIdx.x], q = quota[blockIdx.x];
  const u64 v = cut[blockIdx.x];
  int32_t* out = list + 2 * first[blockIdx.x];
  int64_t* np = paths + first[blockIdx.x];
  int64_t run = 0, ties = 0, placed = 0;   // run: the rank of the next chunk's first kept row; ties: the entries == v before the chunk (both workgroup-uniform)
  for (int base = 0; base < M; base += TPB) {
    const int j = base + threadIdx.x;
    const u64 t = j < M ? tally[j] : 0;
    const bool gt = t > v, tie = t == v && t > 0;
    int64_t sum;
    const int64_t ex = pf::block_scan_excl((int64_t)gt | ((int64_t)tie << 32), sh, sum);   // low half: entries > v before mine; high half: ties before mine
    const int64_t tie_rank = ties + (ex >> 32), kept_ties = ties < q ? ties : q;
    if (gt || (tie && tie_rank < q)) {
      const int64_t r = run + (ex & 0xffffffffLL) + ((tie_rank < q ? tie_rank : q) - kept_ties);
      if (r < cap) {   // (out + 2 r and np + r are formed only for a rank below the cap)
        out[2 * r] = u;
        out[2 * r + 1] = items[j];
        np[r] = (int64_t)t;
        ++placed;
      }
    }
    ties += sum >> 32;
    run += (sum & 0xffffffffLL) + ((ties < q ? ties : q) - kept_ties);
  }
  placed = pf::block_sum(placed, sh);
  if (threadIdx.x == 0 && placed != cap) atomicOr(flag, 1);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
static int bad(std::string* why, int code, const char* t) { if (why) *why = t; return code; }

// the refusals shared by kprn_find_candidates and the host twin (the users' ids: ns::validate_users)
static int validate_limits(int64_t M, int32_t B, int32_t min_hops, int32_t max_hops, std::string* why) {
  if (min_hops < 1 || min_hops > max_hops || max_hops > 3) return bad(why, KPRN_E_ARG, "hops: 1 <= min_hops <= max_hops <= 3");
  if (B < 1) return bad(why, KPRN_E_ARG, "B < 1");
  if ((int64_t)B * ((M + 31) / 32) > 0x7fffffffLL) return bad(why, KPRN_E_ARG, "B * ceil(M / 32) must stay below 2^31");
  return KPRN_OK;
}

// kprn_find_candidates_top's and its twin's, on top of validate_limits
static int validate_top(int64_t M, int32_t B, int32_t cap, std::string* why) {
  if (cap < 1) return bad(why, KPRN_E_ARG, "cap < 1");
  if ((int64_t)B * M >= (1LL << 28)) return bad(why, KPRN_E_ARG, "B * M must stay below 2^28");
  return KPRN_OK;
}

void release_all(kprn_handle* h) {
  dfree(h->cand_list);
  dfree(h->cand_paths);
  h->cand_total = -1;
  if (h->cand_buf) { hipFree(h->cand_buf); h->cand_buf = nullptr; h->cand_buf_bytes = 0; }
}

}  // namespace cd

extern "C" {

int kprn_find_candidates(kprn_handle* h, const kprn_graph* g, const kprn_sampler* catalogue, const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops,
                         int32_t exclude_adjacent, int32_t* group_counts, int64_t* total) {
  API_BEGIN(h)
  KPRN_REQUIRE(g && std::find(h->graphs.begin(), h->graphs.end(), g) != h->graphs.end(), KPRN_E_ARG, "g is not a graph of this handle");
  KPRN_REQUIRE(catalogue && std::find(h->samplers.begin(), h->samplers.end(), catalogue) != h->samplers.end(), KPRN_E_ARG,
               "catalogue is not a sampler of this handle");
  KPRN_REQUIRE(group_counts && total, KPRN_E_ARG, "group_counts or total is NULL");
  const int M = catalogue->M, W = (M + 31) / 32;
  std::string why;
  int rc = cd::validate_limits(M, B, min_hops, max_hops, &why);
  if (rc == KPRN_OK) rc = ns::validate_users(users, B, g->Ve, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  hipStream_t s = h->stream;
  // device arguments: first [B] (int64), then users [B] | counts [B] | flag [4] (int32) | the bitmaps [B][W] (uint32)
  const size_t n_bits = (size_t)B * W, bytes = (size_t)B * 8 + ((size_t)2 * B + 4 + n_bits) * 4;
  grow_call_block(s, h->cand_buf, h->cand_buf_bytes, bytes);
  int64_t* d_first = (int64_t*)h->cand_buf;
  int32_t* d_users = (int32_t*)(d_first + B);
  int32_t* d_counts = d_users + B;
  int32_t* d_flag = d_counts + B;
  uint32_t* d_bits = (uint32_t*)(d_flag + 4);
  const pf::Csr csr{g->rowptr, g->col, g->rel};
  // with a pattern set, an asked hop count that no pattern has reaches nobody
  const bool pat_on = g->n_pat > 0;
  const pat::Table pt = pf::table_of(g);
  const int hmask = pf::hop_mask(min_hops, max_hops) & (pat_on ? pat::hops_mask(pt) : ~0);
  HIP_TRY(hipMemcpyAsync(d_users, users, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_bits, 0, n_bits * sizeof(uint32_t), s));
  {
    ProfScope ps(h, "candidates_mark");
    hipLaunchKernelGGL(pat_on ? cd::k_mark<true> : cd::k_mark<false>, dim3((unsigned)B), dim3(cd::TPB), 0, s, csr, pt, catalogue->items, M, W, d_users, hmask, d_bits);
    HIP_TRY(hipGetLastError());
  }
  {
    ProfScope ps(h, "candidates_count");
    hipLaunchKernelGGL(cd::k_count, dim3((unsigned)B), dim3(cd::TPB), 0, s, csr, catalogue->items, M, W, d_users, exclude_adjacent != 0 ? 1 : 0, d_bits, d_counts);
    HIP_TRY(hipGetLastError());
  }
  std::vector<int32_t> cnt((size_t)B);
  std::vector<int64_t> first((size_t)B);
  HIP_TRY(hipMemcpyAsync(cnt.data(), d_counts, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));   // the wait for the list's size
  int64_t n = 0;
  for (int32_t b = 0; b < B; ++b) {
    KPRN_REQUIRE(cnt[b] >= 0 && cnt[b] <= M, KPRN_E_DEVICE, "find_candidates: the counting pass returned an impossible count");
    first[b] = n;
    n += cnt[b];
  }
  KPRN_REQUIRE(n <= 0x7fffffffLL, KPRN_E_ARG, "the candidate list must stay below 2^31 rows");
  int32_t* list = nullptr;
  if (n > 0) {
    list = dalloc<int32_t>(2 * n);
    try {
      HIP_TRY(hipMemcpyAsync(d_first, first.data(), (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
      {
        ProfScope ps(h, "candidates_fill");
        hipLaunchKernelGGL(cd::k_fill, dim3((unsigned)B), dim3(cd::TPB), 0, s, catalogue->items, W, d_users, d_bits, d_first, d_counts, list, d_flag);
        HIP_TRY(hipGetLastError());
      }
      int32_t flag = 0;
      HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));   // (the fill pass's verdict, before the list replaces the handle's)
      KPRN_REQUIRE(flag == 0, KPRN_E_DEVICE, "find_candidates: the fill pass placed a different number of rows than the counting pass allotted");
    } catch (...) {
      hipStreamSynchronize(s);
      dfree(list);
      throw;
    }
  }
  dfree(h->cand_list);   // (the stream is drained: nothing queued reads the old list)
  dfree(h->cand_paths);  // (a list of this call has no path counts)
  h->cand_list = list; h->cand_total = n; h->cand_Ve = g->Ve;
  std::copy(cnt.begin(), cnt.end(), group_counts);
  *total = n;
  API_END(h)
}

int kprn_find_candidates_top(kprn_handle* h, const kprn_graph* g, const kprn_sampler* catalogue, const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops,
                             int32_t exclude_adjacent, int32_t cap, int32_t* group_counts, int64_t* total) {
  API_BEGIN(h)
  KPRN_REQUIRE(g && std::find(h->graphs.begin(), h->graphs.end(), g) != h->graphs.end(), KPRN_E_ARG, "g is not a graph of this handle");
  KPRN_REQUIRE(catalogue && std::find(h->samplers.begin(), h->samplers.end(), catalogue) != h->samplers.end(), KPRN_E_ARG,
               "catalogue is not a sampler of this handle");
  KPRN_REQUIRE(group_counts && total, KPRN_E_ARG, "group_counts or total is NULL");
  const int M = catalogue->M;
  std::string why;
  int rc = cd::validate_limits(M, B, min_hops, max_hops, &why);
  if (rc == KPRN_OK) rc = cd::validate_top(M, B, cap, &why);
  if (rc == KPRN_OK) rc = ns::validate_users(users, B, g->Ve, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  hipStream_t s = h->stream;
  // device arguments: first [B] (int64) | cut [B] | the tallies [B][M] (uint64), then users [B] | counts [B] | ncand [B] | quota [B] | flag [4] (int32)
  const size_t n_tally = (size_t)B * M, bytes = ((size_t)2 * B + n_tally) * 8 + ((size_t)4 * B + 4) * 4;
  grow_call_block(s, h->cand_buf, h->cand_buf_bytes, bytes);
  int64_t* d_first = (int64_t*)h->cand_buf;
  cd::u64* d_cut = (cd::u64*)(d_first + B);
  cd::u64* d_tally = d_cut + B;
  int32_t* d_users = (int32_t*)(d_tally + n_tally);
  int32_t* d_counts = d_users + B;
  int32_t* d_ncand = d_counts + B;
  int32_t* d_quota = d_ncand + B;
  int32_t* d_flag = d_quota + B;
  const pf::Csr csr{g->rowptr, g->col, g->rel};
  // with a pattern set, an asked hop count that no pattern has reaches nobody
  const bool pat_on = g->n_pat > 0;
  const pat::Table pt = pf::table_of(g);
  const int hmask = pf::hop_mask(min_hops, max_hops) & (pat_on ? pat::hops_mask(pt) : ~0);
  HIP_TRY(hipMemcpyAsync(d_users, users, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_tally, 0, n_tally * sizeof(cd::u64), s));   // (the block is grow-only: an earlier call's sums lie in it)
  {
    ProfScope ps(h, "candidates_tally");
    hipLaunchKernelGGL(pat_on ? cd::k_tally<true> : cd::k_tally<false>, dim3((unsigned)B), dim3(cd::TPB), 0, s, csr, pt, catalogue->items, M, d_users, hmask, d_tally);
    HIP_TRY(hipGetLastError());
  }
  {
    ProfScope ps(h, "candidates_settle");
    hipLaunchKernelGGL(cd::k_settle, dim3((unsigned)B), dim3(cd::TPB), 0, s, csr, catalogue->items, M, d_users, exclude_adjacent != 0 ? 1 : 0, d_tally, d_ncand);
    HIP_TRY(hipGetLastError());
  }
  {
    ProfScope ps(h, "candidates_select");
    hipLaunchKernelGGL(cd::k_select, dim3((unsigned)B), dim3(cd::TPB), 0, s, M, cap, d_tally, d_ncand, d_counts, d_cut, d_quota);
    HIP_TRY(hipGetLastError());
  }
  std::vector<int32_t> cnt((size_t)B);
  std::vector<int64_t> first((size_t)B);
  HIP_TRY(hipMemcpyAsync(cnt.data(), d_counts, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));   // the wait for the list's size
  int64_t n = 0;
  for (int32_t b = 0; b < B; ++b) {
    KPRN_REQUIRE(cnt[b] >= 0 && cnt[b] <= std::min(M, cap), KPRN_E_DEVICE, "find_candidates_top: the selecting pass returned an impossible count");
    first[b] = n;
    n += cnt[b];
  }
  KPRN_REQUIRE(n <= 0x7fffffffLL, KPRN_E_ARG, "the candidate list must stay below 2^31 rows");
  int32_t* list = nullptr;
  int64_t* paths = dalloc<int64_t>(n);   // (never NULL: a list with counts, even an empty one)
  try {
    if (n > 0) {
      list = dalloc<int32_t>(2 * n);
      HIP_TRY(hipMemcpyAsync(d_first, first.data(), (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
      {
        ProfScope ps(h, "candidates_fill_top");
        hipLaunchKernelGGL(cd::k_fill_top, dim3((unsigned)B), dim3(cd::TPB), 0, s, catalogue->items, M, d_users, d_tally, d_first, d_counts, d_cut, d_quota, list,
                           paths, d_flag);
        HIP_TRY(hipGetLastError());
      }
      int32_t flag = 0;
      HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));   // (the fill pass's verdict, before the list replaces the handle's)
      KPRN_REQUIRE(flag == 0, KPRN_E_DEVICE, "find_candidates_top: the fill pass placed a different number of rows than the selecting pass allotted");
    }
  } catch (...) {
    hipStreamSynchronize(s);
    dfree(list);
    dfree(paths);
    throw;
  }
  dfree(h->cand_list);   // (the stream is drained: nothing queued reads the old list)
  dfree(h->cand_paths);
  h->cand_list = list; h->cand_paths = paths; h->cand_total = n; h->cand_Ve = g->Ve;
  std::copy(cnt.begin(), cnt.end(), group_counts);
  *total = n;
  API_END(h)
}

int kprn_read_candidate_paths(kprn_handle* h, int64_t* n_paths_out, int64_t total) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->cand_total >= 0 && h->cand_paths, KPRN_E_ARG, "the handle's candidate list has no path counts");
  KPRN_REQUIRE(total == h->cand_total, KPRN_E_ARG, "total is not the candidate list's");
  if (total > 0) {
    KPRN_REQUIRE(n_paths_out, KPRN_E_ARG, "n_paths_out is NULL");
    HIP_TRY(hipMemcpyAsync(n_paths_out, h->cand_paths, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  API_END(h)
}

int kprn_read_candidates(kprn_handle* h, int32_t* pairs_out, int64_t total) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->cand_total >= 0, KPRN_E_ARG, "the handle has no candidate list");
  KPRN_REQUIRE(total == h->cand_total, KPRN_E_ARG, "total is not the candidate list's");
  if (total > 0) {
    KPRN_REQUIRE(pairs_out, KPRN_E_ARG, "pairs_out is NULL");
    HIP_TRY(hipMemcpyAsync(pairs_out, h->cand_list, (size_t)2 * total * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  API_END(h)
}

int kprn_find_paths_of_candidates(kprn_handle* h, const kprn_graph* g, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, int32_t walks,
                                  uint64_t seed, unsigned int draw, int32_t* counts, int64_t* found, kprn_batch** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out, KPRN_E_ARG, "out is NULL");
  *out = nullptr;
  KPRN_REQUIRE(g && std::find(h->graphs.begin(), h->graphs.end(), g) != h->graphs.end(), KPRN_E_ARG, "g is not a graph of this handle");
  KPRN_REQUIRE(h->cand_total >= 0, KPRN_E_ARG, "the handle has no candidate list");
  const pf::Sampling sampling = pf::sampling_of(walks, seed, draw);
  const pf::Sampling* sm = walks != 0 ? &sampling : nullptr;
  const int32_t B = (int32_t)h->cand_total;
  std::string why;
  const int rc = pf::validate_find_limits(std::max(B, 1), min_hops, max_hops, max_paths, T, sm, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  KPRN_REQUIRE(g->Ve == h->cand_Ve, KPRN_E_INDEX, "the graph's Ve differs from the candidate list's: a pair's node may be outside 1..Ve-1");
  if (B > 0) {
    const int32_t* list = h->cand_list;
    const pf::StagePairs stage = [&](int32_t* d_pairs, hipStream_t s) {
      HIP_TRY(hipMemcpyAsync(d_pairs, list, (size_t)2 * B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    };
    pf::Sampling spread;
    pf::find_staged(h, g, stage, nullptr, B, min_hops, max_hops, max_paths, T, pf::with_cap(h, sm, seed, draw, spread), nullptr, counts, found, out);
  }
  API_END(h)
}

}  // extern "C"

static int host_candidates(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, int64_t M,
                              const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t threads,
                              int32_t* group_counts, int32_t* cand, const pat::Table* ptp) {
  if (E < 0 || E > 0x7fffffffLL || (E > 0 && (!src || !dst || !rel)) || !group_counts) return KPRN_E_ARG;
  int rc = ns::validate_table(items, nullptr, M, Ve, nullptr);
  if (rc == KPRN_OK) rc = cd::validate_limits(M, B, min_hops, max_hops, nullptr);
  if (rc == KPRN_OK) rc = ns::validate_users(users, B, Ve, nullptr);
  if (rc != KPRN_OK) return rc;
  for (int64_t e = 0; e < E; ++e)
    if (src[e] < 1 || src[e] >= Ve || dst[e] < 1 || dst[e] >= Ve) return KPRN_E_INDEX;
  try {
    const pf::HostCsr hg = pf::host_csr(src, dst, rel, E, Ve);
    const pf::Csr g{hg.rowptr.data(), hg.col.data(), hg.rel.data()};
    const pat::Table none{nullptr, 0, {0, 0, 0, 0, 0, 0}};
    const pat::Table& pt = ptp ? *ptp : none;
    const int hmask = pf::hop_mask(min_hops, max_hops) & (ptp ? pat::hops_mask(pt) : ~0);
    std::vector<std::vector<int32_t>> mine((size_t)B);
    pf::parallel_pairs(B, threads, [&](int32_t b) {
      std::vector<int32_t>& v = mine[(size_t)b];
      const int u = users[b];
      auto mark = [&](int c) { if (cd::member(items, (int)M, c) >= 0) v.push_back(c); };
      if (ptp) cd::host_walk<true>(g, pt, u, hmask, mark); else cd::host_walk<false>(g, pt, u, hmask, mark);
      std::sort(v.begin(), v.end());
      v.erase(std::unique(v.begin(), v.end()), v.end());
      v.erase(std::remove_if(v.begin(), v.end(), [&](int32_t c) {
        if (c == u) return true;
        if (!exclude_adjacent) return false;
        int lo, hi;
        pf::edge_range(g, u, c, lo, hi);
        return lo != hi;
      }), v.end());
    });
    int64_t n = 0;
    for (const auto& v : mine) n += (int64_t)v.size();
    if (n > 0x7fffffffLL) return KPRN_E_ARG;
    int32_t* to = cand;
    for (int32_t b = 0; b < B; ++b) {
      group_counts[b] = (int32_t)mine[(size_t)b].size();
      if (cand) to = std::copy(mine[(size_t)b].begin(), mine[(size_t)b].end(), to);
    }
  } catch (...) { return KPRN_E_NOMEM; }
  return KPRN_OK;
}

static int host_candidates_top(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, int64_t M,
                                  const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t cap, int32_t threads,
                                  int32_t* group_counts, int32_t* cand, int64_t* n_paths, const pat::Table* ptp) {
  if (E < 0 || E > 0x7fffffffLL || (E > 0 && (!src || !dst || !rel)) || !group_counts) return KPRN_E_ARG;
  int rc = ns::validate_table(items, nullptr, M, Ve, nullptr);
  if (rc == KPRN_OK) rc = cd::validate_limits(M, B, min_hops, max_hops, nullptr);
  if (rc == KPRN_OK) rc = cd::validate_top(M, B, cap, nullptr);
  if (rc == KPRN_OK) rc = ns::validate_users(users, B, Ve, nullptr);
  if (rc != KPRN_OK) return rc;
  for (int64_t e = 0; e < E; ++e)
    if (src[e] < 1 || src[e] >= Ve || dst[e] < 1 || dst[e] >= Ve) return KPRN_E_INDEX;
  try {
    const pf::HostCsr hg = pf::host_csr(src, dst, rel, E, Ve);
    const pf::Csr g{hg.rowptr.data(), hg.col.data(), hg.rel.data()};
    const pat::Table none{nullptr, 0, {0, 0, 0, 0, 0, 0}};
    const pat::Table& pt = ptp ? *ptp : none;
    const int hmask = pf::hop_mask(min_hops, max_hops) & (ptp ? pat::hops_mask(pt) : ~0);
    std::vector<std::vector<std::pair<int32_t, int64_t>>> mine((size_t)B);   // per user: (member's position, n_paths), positions ascending
    pf::parallel_pairs(B, threads, [&](int32_t b) {
      auto& v = mine[(size_t)b];
      const int u = users[b];
      std::vector<int64_t> tally((size_t)M, 0);
      auto mark = [&](int c) { const int j = cd::member(items, (int)M, c); if (j >= 0) ++tally[(size_t)j]; };
      if (ptp) cd::host_walk<true>(g, pt, u, hmask, mark); else cd::host_walk<false>(g, pt, u, hmask, mark);
      for (int32_t j = 0; j < (int32_t)M; ++j) {
        if (tally[(size_t)j] == 0 || items[j] == u) continue;
        if (exclude_adjacent) {
          int lo, hi;
          pf::edge_range(g, u, items[j], lo, hi);
          if (lo != hi) continue;
        }
        v.emplace_back(j, tally[(size_t)j]);
      }
      if ((int64_t)v.size() > cap) {   // the cap best by (n_paths descending, id ascending), then back in id order
        std::nth_element(v.begin(), v.begin() + cap, v.end(),
                         [](const std::pair<int32_t, int64_t>& x, const std::pair<int32_t, int64_t>& y) { return x.second != y.second ? x.second > y.second : x.first < y.first; });
        v.resize((size_t)cap);
        std::sort(v.begin(), v.end());
      }
    });
    int64_t n = 0;
    for (const auto& v : mine) n += (int64_t)v.size();
    if (n > 0x7fffffffLL) return KPRN_E_ARG;
    int64_t at = 0;
    for (int32_t b = 0; b < B; ++b) {
      group_counts[b] = (int32_t)mine[(size_t)b].size();
      for (const auto& p : mine[(size_t)b]) {
        if (cand) cand[at] = items[p.first];
        if (n_paths) n_paths[at] = p.second;
        ++at;
      }
    }
  } catch (...) { return KPRN_E_NOMEM; }
  return KPRN_OK;
}

extern "C" {

int kprn_host_find_candidates(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, int64_t M,
                              const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t threads,
                              int32_t* group_counts, int32_t* cand) {
  return host_candidates(src, dst, rel, E, Ve, items, M, users, B, min_hops, max_hops, exclude_adjacent, threads, group_counts, cand, nullptr);
}

int kprn_host_find_candidates_top(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, int64_t M,
                                  const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t cap, int32_t threads,
                                  int32_t* group_counts, int32_t* cand, int64_t* n_paths) {
  return host_candidates_top(src, dst, rel, E, Ve, items, M, users, B, min_hops, max_hops, exclude_adjacent, cap, threads, group_counts, cand, n_paths, nullptr);
}

// The candidates twins take no Vr: the table's columns reach the largest relation the edges or the sets name, and a relation below 1 is KPRN_E_INDEX
int kprn_host_find_candidates_patterns(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, int64_t M,
                                       const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t cap, int32_t threads,
                                       int32_t* group_counts, int32_t* cand, int64_t* n_paths, const int32_t* hops, const int64_t* set_offsets,
                                       const int32_t* set_rels, int32_t n_pat) {
  if (n_pat == 0) return host_candidates_top(src, dst, rel, E, Ve, items, M, users, B, min_hops, max_hops, exclude_adjacent, cap, threads, group_counts, cand, n_paths, nullptr);
  if (E < 0 || E > 0x7fffffffLL || (E > 0 && (!src || !dst || !rel))) return KPRN_E_ARG;
  try {
    int rc = pat::validate(hops, set_offsets, set_rels, n_pat, 0x7fffffff, nullptr);   // (the shape, and no relation below 1)
    if (rc != KPRN_OK) return rc;
    int32_t Vr = 1;
    for (int64_t e = 0; e < E; ++e) { if (rel[e] < 1) return KPRN_E_INDEX; Vr = std::max(Vr, rel[e]); }
    int64_t S = 0;
    for (int32_t p = 0; p < n_pat; ++p) S += hops[p];
    for (int64_t k = 0; k < set_offsets[S]; ++k) Vr = std::max(Vr, set_rels[k]);
    if (Vr > (1 << 24)) return KPRN_E_INDEX;   // (a table of 5 (Vr + 1) words)
    pf::HostPat hp;
    rc = hp.set(hops, set_offsets, set_rels, n_pat, Vr);
    if (rc != KPRN_OK) return rc;
    return host_candidates_top(src, dst, rel, E, Ve, items, M, users, B, min_hops, max_hops, exclude_adjacent, cap, threads, group_counts, cand, n_paths, &hp.t);
  } catch (...) { return KPRN_E_NOMEM; }
}

}  // extern "C"
