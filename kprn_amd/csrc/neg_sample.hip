// Negative sampler (include/kprn.h "sampling negatives"): for B user slots, n_neg distinct items per slot drawn from a weighted candidate list, none of
// them the user or adjacent to the user in the stored graph -- and kprn_find_training_paths, which forms the (positive, negatives) pair list in HBM and
// hands it to the finder's two passes (path_find_dev.h find_staged) without a trip to the host.  Integers only behind the thresholds; no atomics.
//
// One definition of the rule serves the kernel and the host twin (namespace ns, __host__ __device__):
//   table   items [M] ascending, thr [M] (uint64, built on the host in double): pick(r) = the number of j with thr[j] <= r
//   word    Philox4x32-10, key = the seed's halves, counter = (a / 4, n, b, draw), word a % 4: attempt a of negative n of slot b
//   test    a candidate c passes the graph tests when c != u and the CSR holds no edge u -> c (edge_range empty)
//   settle  n = 0 .. n_neg - 1 in order: negative n = the candidate of its first attempt that passes the graph tests and is not on the slot's accepted list
// Device: one wave per slot, 4 slots per 256-thread workgroup.  A pass covers 64 / max_attempts negatives: lane l forms the candidate of attempt l % A of
// negative n0 + l / A and its graph tests on its own (Philox, two binary searches), then checks it against the accepted list in LDS (every lane reads the
// same word: a broadcast).  The negatives of the pass are settled one after the other: a 64-bit ballot over the lanes of negative n that are still
// valid, the first set bit wins, its candidate is broadcast, the later negatives' lanes that hold the same item drop out, lane 0 extends the list and
// stores the result.  The wave's control flow between its cross-lane operations is uniform (loop bounds are kernel arguments and ballot results), a wave
// never waits for another, and a wave writes its own slot's outputs only.
#include "path_find_dev.h"

#include <cmath>

namespace ns {

constexpr int TPB = 256, WAVES = TPB / 64, MAX_NEG = 256, MAX_ATTEMPTS = 64;

struct Table { const int32_t* items; const unsigned long long* thr; int M; };
struct Rng { uint32_t k0, k1, draw; };

// the number of j with thr[j] <= r (thr[M - 1] = 2^32 > r: the result is an index)
__host__ __device__ static inline int pick(const Table& t, uint32_t r) {
  int l = 0, h = t.M;
  while (l < h) { const int m = l + ((h - l) >> 1); if (t.thr[m] <= (unsigned long long)r) l = m + 1; else h = m; }
  return l < t.M ? l : t.M - 1;
}
__host__ __device__ static inline uint32_t attempt_word(const Rng& g, uint32_t a, uint32_t n, uint32_t b) {
  uint32_t w[4];
  philox::philox4x32_10(a >> 2, n, b, g.draw, g.k0, g.k1, w);
  const uint32_t lo = (a & 1) ? w[1] : w[0], hi = (a & 1) ? w[3] : w[2];
  return (a & 2) ? hi : lo;
}
__host__ __device__ static inline int candidate(const Table& t, const Rng& g, int a, int n, int b) { return t.items[pick(t, attempt_word(g, a, n, b))]; }
// c may be u's negative as far as the graph goes
__host__ __device__ static inline bool graph_ok(const pf::Csr& g, int u, int c) {
  if (c == u) return false;
  int lo, hi;
  pf::edge_range(g, u, c, lo, hi);
  return lo == hi;
}

// users [B] at users[b * ustride].  neg [B][n_neg] / n_found [B] (either may be null).  pairs (or null) [B * (1 + n_neg)][2]: the slot's rows of the training
// pair list, (u, users[b * ustride + 1]) and then (u, negative n) -- ustride = 2 then, the positives.  n_neg <= MAX_NEG, 1 <= A <= 64.
__global__ __launch_bounds__(TPB) void k_sample(pf::Csr g, Table t, Rng rng, const int32_t* __restrict__ users, int ustride, int B, int n_neg, int A,
                                                int32_t* __restrict__ neg, int32_t* __restrict__ n_found, int32_t* __restrict__ pairs) {
  __shared__ int32_t accepted[WAVES][MAX_NEG];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * WAVES + wave;
  if (b >= B) return;   // (the whole wave; nothing below waits for another wave)
  int32_t* acc = accepted[wave];
  const int u = users[(int64_t)b * ustride];
  int32_t* out_pairs = pairs ? pairs + 2 * (int64_t)b * (1 + n_neg) : nullptr;
  int32_t* out_neg = neg ? neg + (int64_t)b * n_neg : nullptr;
  if (out_pairs && lane == 0) { out_pairs[0] = u; out_pairs[1] = users[(int64_t)b * ustride + 1]; }
  const int per_pass = 64 / A;                    // negatives whose attempts share the wave's lanes
  const int grp = lane / A, a = lane - grp * A;   // this lane: attempt a of the pass's negative grp
  int cnt = 0;                                    // accepted so far (wave-uniform)
  for (int n0 = 0; n0 < n_neg; n0 += per_pass) {
    const int in_pass = min(per_pass, n_neg - n0);
    int c = 0;
    bool ok = false;
    if (grp < in_pass) {
      c = candidate(t, rng, a, n0 + grp, b);
      ok = graph_ok(g, u, c);
      for (int j = 0; ok && j < cnt; ++j) ok = acc[j] != c;   // the list as the earlier passes left it
    }
    for (int k = 0; k < in_pass; ++k) {
      const unsigned long long valid = __ballot(ok && grp == k);
      const int first = valid ? __ffsll(valid) - 1 : 0;
      int sel = __shfl(c, first);
      sel = valid ? sel : 0;
      if (valid) {   // (wave-uniform)
        if (grp > k && c == sel) ok = false;
        if (lane == 0) acc[cnt] = sel;
        ++cnt;
      }
      if (lane == 0) {
        if (out_neg) out_neg[n0 + k] = sel;
        if (out_pairs) { out_pairs[2 * (1 + n0 + k)] = u; out_pairs[2 * (1 + n0 + k) + 1] = sel; }
      }
    }
    // lane 0's list entries before the next pass's reads by every lane (one wave: program order in the LDS queue; this keeps the compiler to it)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (n_found && lane == 0) n_found[b] = cnt;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
static int bad(std::string* why, int code, const char* t) { if (why) *why = t; return code; }

int validate_table(const int32_t* items, const float* weights, int64_t M, int32_t Ve, std::string* why) {
  if (!items || M < 1 || M > 0x7fffffffLL) return bad(why, KPRN_E_ARG, "items is NULL or M is outside 1 .. 2^31 - 1");
  if (Ve < 2) return bad(why, KPRN_E_ARG, "Ve must be at least 2");
  bool any = weights == nullptr;
  for (int64_t j = 0; j < M; ++j) {
    if (items[j] < 1 || items[j] >= Ve) return bad(why, KPRN_E_INDEX, "a candidate item is outside 1..Ve-1");
    if (j > 0 && items[j] <= items[j - 1]) return bad(why, KPRN_E_ARG, "items must be strictly ascending");
    if (weights) {
      if (!std::isfinite(weights[j]) || weights[j] < 0.f) return bad(why, KPRN_E_ARG, "a weight is negative or not finite");
      any = any || weights[j] > 0.f;
    }
  }
  if (!any) return bad(why, KPRN_E_ARG, "every weight is 0");
  return KPRN_OK;
}

// thr[j] = floor(cum_j / cum_{M-1} * 2^32), cum in double in index order
static std::vector<unsigned long long> thresholds(const float* weights, int64_t M) {
  double total = 0.0;
  for (int64_t j = 0; j < M; ++j) total = total + (weights ? (double)weights[j] : 1.0);
  std::vector<unsigned long long> thr((size_t)M);
  double cum = 0.0;
  for (int64_t j = 0; j < M; ++j) {
    cum = cum + (weights ? (double)weights[j] : 1.0);
    thr[(size_t)j] = (unsigned long long)std::floor(cum / total * 4294967296.0);
  }
  return thr;
}

static int validate_limits(int64_t B, int32_t n_neg, int32_t max_attempts, std::string* why) {
  if (B < 1) return bad(why, KPRN_E_ARG, "B < 1");
  if (n_neg < 1 || n_neg > MAX_NEG) return bad(why, KPRN_E_ARG, "n_neg must be in 1..256");
  if (max_attempts < 1 || max_attempts > MAX_ATTEMPTS) return bad(why, KPRN_E_ARG, "max_attempts must be in 1..64");
  if (B * (1 + (int64_t)n_neg) > 0x7fffffffLL) return bad(why, KPRN_E_ARG, "B * (1 + n_neg) must stay below 2^31");
  return KPRN_OK;
}
int validate_users(const int32_t* users, int64_t n, int32_t Ve, std::string* why) {
  if (!users) return bad(why, KPRN_E_ARG, "users is NULL");
  for (int64_t k = 0; k < n; ++k)
    if (users[k] < 1 || users[k] >= Ve) return bad(why, KPRN_E_INDEX, "a user (or a positive's item) is outside 1..Ve-1");
  return KPRN_OK;
}

static Rng rng_of(uint64_t seed, uint32_t draw) { return Rng{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), draw}; }

// grow-only device block of the sampling calls (the stream is drained before it is replaced)
static void* reserve(kprn_handle* h, size_t bytes) { return grow_call_block(h->stream, h->ns_buf, h->ns_buf_bytes, bytes); }

static void launch(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s, const Rng& rng, const int32_t* d_users, int ustride, int32_t B, int32_t n_neg,
                   int32_t max_attempts, int32_t* d_neg, int32_t* d_found, int32_t* d_pairs, hipStream_t st) {
  ProfScope ps(h, "sample_negatives", st);
  const pf::Csr csr{g->rowptr, g->col, g->rel};
  const Table t{s->items, s->thr, s->M};
  hipLaunchKernelGGL(k_sample, dim3((unsigned)((B + WAVES - 1) / WAVES)), dim3(TPB), 0, st, csr, t, rng, d_users, ustride, B, n_neg, max_attempts, d_neg, d_found,
                     d_pairs);
  HIP_TRY(hipGetLastError());
}

static void free_sampler(kprn_sampler* s) {
  dfree(s->items); dfree(s->thr);
  delete s;
}

void release_all(kprn_handle* h) {
  for (kprn_sampler* s : h->samplers) free_sampler(s);
  h->samplers.clear();
  if (h->ns_buf) { hipFree(h->ns_buf); h->ns_buf = nullptr; h->ns_buf_bytes = 0; }
}

static void require_ours(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s) {
  KPRN_REQUIRE(g && std::find(h->graphs.begin(), h->graphs.end(), g) != h->graphs.end(), KPRN_E_ARG, "g is not a graph of this handle");
  KPRN_REQUIRE(s && std::find(h->samplers.begin(), h->samplers.end(), s) != h->samplers.end(), KPRN_E_ARG, "s is not a sampler of this handle");
}

}  // namespace ns

extern "C" {

int kprn_sampler_create(kprn_handle* h, const int32_t* items, const float* weights, int64_t M, kprn_sampler** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out, KPRN_E_ARG, "out is NULL");
  *out = nullptr;
  std::string why;
  const int rc = ns::validate_table(items, weights, M, h->cfg.Ve, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  const std::vector<unsigned long long> thr = ns::thresholds(weights, M);
  kprn_sampler* s = new kprn_sampler();
  s->M = (int32_t)M;
  try {
    s->items = dalloc<int32_t>(M);
    s->thr = dalloc<unsigned long long>(M);
    HIP_TRY(hipMemcpyAsync(s->items, items, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s->thr, thr.data(), (size_t)M * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  } catch (...) {
    ns::free_sampler(s);
    throw;
  }
  h->samplers.push_back(s);
  *out = s;
  API_END(h)
}

void kprn_sampler_destroy(kprn_handle* h, kprn_sampler* s) {
  if (!h || !s) return;
  auto it = std::find(h->samplers.begin(), h->samplers.end(), s);
  if (it == h->samplers.end()) return;   // (not this handle's, or destroyed already)
  hipSetDevice(h->cfg.device_id);
  sync_stream(h->stream, /*nothrow=*/true);   // (a sampling launch may still read it)
  h->samplers.erase(it);
  ns::free_sampler(s);
}

int kprn_sample_negatives(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s, const int32_t* users, int32_t B, int32_t n_neg, int32_t max_attempts,
                          uint64_t seed, unsigned int draw, int32_t* neg, int32_t* n_found) {
  API_BEGIN(h)
  ns::require_ours(h, g, s);
  KPRN_REQUIRE(neg, KPRN_E_ARG, "neg is NULL");
  std::string why;
  int rc = ns::validate_limits(B, n_neg, max_attempts, &why);
  if (rc == KPRN_OK) rc = ns::validate_users(users, B, g->Ve, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  hipStream_t st = h->stream;
  // users [B] | neg [B][n_neg] | n_found [B]
  const size_t n_out = (size_t)B * n_neg;
  int32_t* d_users = (int32_t*)ns::reserve(h, ((size_t)2 * B + n_out) * sizeof(int32_t));
  int32_t* d_neg = d_users + B;
  int32_t* d_found = d_neg + n_out;
  HIP_TRY(hipMemcpyAsync(d_users, users, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
  ns::launch(h, g, s, ns::rng_of(seed, draw), d_users, 1, B, n_neg, max_attempts, d_neg, d_found, nullptr, st);
  // (through vectors: a failed copy or wait leaves the caller's arrays as they were)
  std::vector<int32_t> out(n_out), nf((size_t)B);
  HIP_TRY(hipMemcpyAsync(out.data(), d_neg, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(nf.data(), d_found, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::copy(out.begin(), out.end(), neg);
  if (n_found) std::copy(nf.begin(), nf.end(), n_found);
  API_END(h)
}

}  // extern "C"

// kprn_find_training_paths (sm == NULL) and kprn_find_training_paths_sampled
static int find_training_paths(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s, const int32_t* pos, int32_t B, int32_t n_neg, int32_t max_attempts,
                               uint64_t seed, unsigned int draw, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, const pf::Sampling* sm,
                               int32_t* pairs_out, int32_t* counts, int64_t* found, kprn_batch** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out, KPRN_E_ARG, "out is NULL");
  *out = nullptr;
  ns::require_ours(h, g, s);
  std::string why;
  int rc = ns::validate_limits(B, n_neg, max_attempts, &why);
  if (rc == KPRN_OK) rc = ns::validate_users(pos, 2 * (int64_t)B, g->Ve, &why);
  const int32_t n_pairs = rc == KPRN_OK ? B * (1 + n_neg) : 0;
  if (rc == KPRN_OK) rc = pf::validate_find_limits(n_pairs, min_hops, max_hops, max_paths, T, sm, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  int32_t* d_pos = (int32_t*)ns::reserve(h, (size_t)2 * B * sizeof(int32_t));
  std::vector<float> labels((size_t)n_pairs, 0.f);
  for (int32_t b = 0; b < B; ++b) labels[(size_t)b * (1 + n_neg)] = 1.f;
  const ns::Rng rng = ns::rng_of(seed, draw);
  // the pair list is formed where the finder reads it: each wave writes its slot's 1 + n_neg rows
  const pf::StagePairs stage = [&](int32_t* d_pairs, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(d_pos, pos, (size_t)2 * B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    ns::launch(h, g, s, rng, d_pos, 2, B, n_neg, max_attempts, nullptr, nullptr, d_pairs, st);
  };
  pf::Sampling spread;   // (option "path_cap": the seed and draw of the negatives serve the cap too; their counters differ)
  pf::find_staged(h, g, stage, labels.data(), n_pairs, min_hops, max_hops, max_paths, T, pf::with_cap(h, sm, seed, draw, spread), pairs_out, counts, found, out);
  API_END(h)
}

extern "C" {

int kprn_find_training_paths(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s, const int32_t* pos, int32_t B, int32_t n_neg, int32_t max_attempts,
                             uint64_t seed, unsigned int draw, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, int32_t* pairs_out,
                             int32_t* counts, int64_t* found, kprn_batch** out) {
  return find_training_paths(h, g, s, pos, B, n_neg, max_attempts, seed, draw, min_hops, max_hops, max_paths, T, nullptr, pairs_out, counts, found, out);
}

int kprn_find_training_paths_sampled(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s, const int32_t* pos, int32_t B, int32_t n_neg,
                                     int32_t max_attempts, uint64_t seed, unsigned int draw, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T,
                                     int32_t walks, int32_t* pairs_out, int32_t* counts, int64_t* found, kprn_batch** out) {
  const pf::Sampling sm = pf::sampling_of(walks, seed, draw);   // (one seed and draw for the negatives and the walks: their counters differ)
  return find_training_paths(h, g, s, pos, B, n_neg, max_attempts, seed, draw, min_hops, max_hops, max_paths, T, &sm, pairs_out, counts, found, out);
}

int kprn_host_sample_negatives(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, const float* weights,
                               int64_t M, const int32_t* users, int32_t B, int32_t n_neg, int32_t max_attempts, uint64_t seed, unsigned int draw,
                               int32_t threads, int32_t* neg, int32_t* n_found) {
  if (E < 0 || E > 0x7fffffffLL || (E > 0 && (!src || !dst || !rel)) || !neg) return KPRN_E_ARG;
  int rc = ns::validate_table(items, weights, M, Ve, nullptr);
  if (rc == KPRN_OK) rc = ns::validate_limits(B, n_neg, max_attempts, nullptr);
  if (rc == KPRN_OK) rc = ns::validate_users(users, B, Ve, nullptr);
  if (rc != KPRN_OK) return rc;
  for (int64_t e = 0; e < E; ++e)
    if (src[e] < 1 || src[e] >= Ve || dst[e] < 1 || dst[e] >= Ve) return KPRN_E_INDEX;
  try {
    const pf::HostCsr hg = pf::host_csr(src, dst, rel, E, Ve);
    const pf::Csr g{hg.rowptr.data(), hg.col.data(), hg.rel.data()};
    const std::vector<unsigned long long> thr = ns::thresholds(weights, M);
    const ns::Table t{items, thr.data(), (int)M};
    const ns::Rng rng = ns::rng_of(seed, draw);
    std::vector<int32_t> out((size_t)B * n_neg, 0), nf((size_t)B, 0);
    pf::parallel_pairs(B, threads, [&](int32_t b) {
      int32_t* mine = &out[(size_t)b * n_neg];
      int32_t acc[ns::MAX_NEG];
      int cnt = 0;
      const int u = users[b];
      for (int n = 0; n < n_neg; ++n)
        for (int a = 0; a < max_attempts; ++a) {
          const int c = ns::candidate(t, rng, a, n, b);
          if (!ns::graph_ok(g, u, c) || std::find(acc, acc + cnt, c) != acc + cnt) continue;
          mine[n] = acc[cnt++] = c;
          break;
        }
      nf[(size_t)b] = cnt;
    });
    std::copy(out.begin(), out.end(), neg);
    if (n_found) std::copy(nf.begin(), nf.end(), n_found);
  } catch (...) { return KPRN_E_NOMEM; }
  return KPRN_OK;
}

}  // extern "C"
