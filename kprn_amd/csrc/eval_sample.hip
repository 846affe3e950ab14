// Sampled evaluation groups (include/kprn.h "sampled evaluation groups"): for every held pair (u, i) of B users, up to n_neg negatives drawn from the
// user's rows of the handle's candidate list, the list cut down to the rows some sample needs, and the rows of every group in the new list -- the list never
// visits the host.  The rule (key, find), its refusals and the host twin are eval_sample_host.h's.  Integers only.
//
// Device: 256-thread workgroups; a bitmap of ceil(rows / 32) words per user, zeroed by a memset queued before the first kernel.
//   k_draw   one workgroup per target.  Every thread finds the target's row by the same binary search in the user's rows (a uniform result: the early return
//            of an unreachable target is taken by the whole workgroup).  d = the rows whose item is no target of the user, counted.  d > n_neg: the n_neg-th
//            smallest key over those rows by a radix select from byte 7 down, one 256-bin LDS histogram per byte (integer LDS adds: any order, one sum) --
//            keys are distinct, so exactly n_neg keys are <= the cut.  The selected rows are written in row order, 256 rows at a time, by the workgroup's
//            exclusive scan with the running rank carried from chunk to chunk; each sets its bit, and the target its own, in the user's bitmap: a plain
//            load first, atomicOr where the bit is not yet seen.  The bitmap is a set: several targets of a user set the same bits in any order
//   k_count  a thread per word, popcounts summed over the workgroup -> the user's rows in the new list.  The host scans them into each user's first row
//   k_fill   the words 256 at a time, ranks by the exclusive scan; a thread copies the rows of its own word into the new block while rank < the count and
//            notes the new row of each in the old-row -> new-row table.  The rows placed are compared with the count: a disagreement sets the flag
//   k_remap  target_rows and neg_rows, written by k_draw as rows of the old list, through that table
// No atomic hands out a slot or a rank, and no workgroup waits for another.
#include "path_find_dev.h"
#include "eval_sample_host.h"

namespace es {

using pf::TPB;

struct Args {   // device pointers
  const int32_t* list;     // the old list [total][2]
  const int64_t* first;    // [B + 1]: user b's rows are first[b] .. first[b + 1] - 1
  const int64_t* toff;     // [B + 1]
  const int64_t* woff;     // [B + 1]: user b's bitmap words
  const int32_t* tslot;    // [NT]: the user slot of every target
  const int32_t* titems;   // [NT]
  Seed sd;
  int n_neg;
  int32_t* trow;           // [NT]
  int32_t* neg;            // [NT][n_neg], -1 everywhere before the launch
  int32_t* ndrawn;         // [NT]
  uint32_t* bits;
  int32_t* flag;
};

__device__ static inline void mark(uint32_t* bits, int64_t j) {
  const uint32_t m = 1u << (j & 31);
  if (!(bits[j >> 5] & m)) atomicOr(&bits[j >> 5], m);   // (a stale load only repeats an atomic: bits are set, never cleared, in this launch)
}

__global__ __launch_bounds__(TPB) void k_draw(Args a) {
  __shared__ int64_t sh[TPB];
  __shared__ int hist[256];
  static_assert(TPB == 256, "one thread zeroes one bin");
  const int k = blockIdx.x, b = a.tslot[k];
  const int64_t r0 = a.first[b], n = a.first[b + 1] - r0, t0 = a.toff[b], nt = a.toff[b + 1] - t0;
  const int32_t* rows = a.list + 2 * r0;
  const int32_t* mine = a.titems + t0;   // H, ascending
  const int32_t i = a.titems[k];
  const int64_t at = find(rows + 1, n, 2, i);   // (the same loads in every thread: the branches and loop bounds below are workgroup-uniform)
  if (at < 0) {
    if (threadIdx.x == 0) { a.trow[k] = -1; a.ndrawn[k] = 0; }
    return;
  }
  const int32_t u = rows[0];
  uint32_t* bits = a.bits + a.woff[b];
  int64_t d = 0;
  for (int64_t j = threadIdx.x; j < n; j += TPB) d += find(mine, nt, 1, rows[2 * j + 1]) < 0;
  d = pf::block_sum(d, sh);
  u64 v = ~0ull;   // the cut: a row of D is drawn iff its key <= v
  if (d > a.n_neg) {
    v = 0;           // the digits found so far, in place
    int kk = a.n_neg;   // v is the kk-th smallest of the keys that agree with it above digit dg
    for (int dg = 7; dg >= 0; --dg) {
      hist[threadIdx.x] = 0;
      __syncthreads();
      for (int64_t j = threadIdx.x; j < n; j += TPB) {
        const int32_t c = rows[2 * j + 1];
        if (find(mine, nt, 1, c) >= 0) continue;
        const u64 t = key(a.sd, u, i, c);
        if (dg == 7 || (t >> (8 * (dg + 1))) == (v >> (8 * (dg + 1)))) atomicAdd(&hist[(int)((t >> (8 * dg)) & 255)], 1);
      }
      __syncthreads();
      int bin = 0, below = 0;
      for (; bin < 255; ++bin) {   // every thread reads the same bins: the same digit in all of them
        const int c = hist[bin];
        if (below + c >= kk) break;
        below += c;
      }
      kk -= below;
      v |= (u64)bin << (8 * dg);
      __syncthreads();   // (hist is zeroed again by the next pass)
    }
  }
  int32_t* out = a.neg + (int64_t)k * a.n_neg;
  int64_t run = 0;   // the rank of the next chunk's first drawn row (workgroup-uniform, like the loop bound)
  for (int64_t base = 0; base < n; base += TPB) {
    const int64_t j = base + threadIdx.x;
    bool sel = false;
    if (j < n) {
      const int32_t c = rows[2 * j + 1];
      sel = find(mine, nt, 1, c) < 0 && key(a.sd, u, i, c) <= v;
    }
    int64_t sum;
    const int64_t r = run + pf::block_scan_excl(sel ? 1 : 0, sh, sum);
    if (sel && r < a.n_neg) {   // (out + r is formed only for a rank below n_neg)
      out[r] = (int32_t)(r0 + j);
      mark(bits, j);
    }
    run += sum;
  }
  if (threadIdx.x == 0) {
    a.trow[k] = (int32_t)(r0 + at);
    mark(bits, at);
    a.ndrawn[k] = (int32_t)(run < a.n_neg ? run : a.n_neg);
    if (run != (d < a.n_neg ? d : a.n_neg)) atomicOr(a.flag, 2);   // the cut kept another number of rows than it was found for
  }
}

__global__ __launch_bounds__(TPB) void k_count(const int64_t* __restrict__ woff, const uint32_t* __restrict__ bits_all, int32_t* __restrict__ counts) {
  __shared__ int64_t sh[TPB];
  const uint32_t* bits = bits_all + woff[blockIdx.x];
  const int64_t W = woff[blockIdx.x + 1] - woff[blockIdx.x];
  int64_t n = 0;
  for (int64_t w = threadIdx.x; w < W; w += TPB) n += __popc(bits[w]);
  n = pf::block_sum(n, sh);
  if (threadIdx.x == 0) counts[blockIdx.x] = (int32_t)n;
}

// nfirst [b]: the user's first row in the new list; counts [b]: the rows it was allotted
__global__ __launch_bounds__(TPB) void k_fill(const int32_t* __restrict__ list, const int64_t* __restrict__ first, const int64_t* __restrict__ woff,
                                              const uint32_t* __restrict__ bits_all, const int64_t* __restrict__ nfirst, const int32_t* __restrict__ counts,
                                              int32_t* __restrict__ new_list, int32_t* __restrict__ to_new, int32_t* flag) {
  __shared__ int64_t sh[TPB];
  const int b = blockIdx.x;
  const uint32_t* bits = bits_all + woff[b];
  const int64_t W = woff[b + 1] - woff[b], r0 = first[b], n = first[b + 1] - r0, o = nfirst[b], cap = counts[b];
  int64_t run = 0, placed = 0;   // run: the rank of the next chunk's first row (workgroup-uniform, like the loop bound)
  for (int64_t base = 0; base < W; base += TPB) {
    const int64_t w = base + threadIdx.x;
    const uint32_t word = w < W ? bits[w] : 0u;
    int64_t sum;
    int64_t r = run + pf::block_scan_excl(__popc(word), sh, sum);
    for (uint32_t rest = word; rest && r < cap; rest &= rest - 1, ++r) {   // (new_list + 2 (o + r) is formed only for a rank below the count)
      const int64_t j = 32 * w + (__ffs(rest) - 1);
      if (j >= n) break;   // (no bit past the user's rows is ever set)
      new_list[2 * (o + r)] = list[2 * (r0 + j)];
      new_list[2 * (o + r) + 1] = list[2 * (r0 + j) + 1];
      to_new[r0 + j] = (int32_t)(o + r);
      ++placed;
    }
    run += sum;
  }
  placed = pf::block_sum(placed, sh);
  if (threadIdx.x == 0 && placed != cap) atomicOr(flag, 1);
}

// x [n]: rows of the old list (every one of them kept, so its entry of the table is written), -1 stays
__global__ __launch_bounds__(TPB) void k_remap(int32_t* __restrict__ x, int64_t n, const int32_t* __restrict__ to_new) {
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < n; q += (int64_t)gridDim.x * TPB) {
    const int32_t v = x[q];
    if (v >= 0) x[q] = to_new[v];
  }
}

}  // namespace es

extern "C" {

int kprn_sample_eval_groups(kprn_handle* h, const int32_t* group_counts, int32_t B, const int64_t* target_offsets, const int32_t* target_items, int32_t n_neg,
                            uint64_t seed, unsigned int draw, int32_t* new_group_counts, int64_t* new_total, int32_t* target_rows, int32_t* neg_rows,
                            int32_t* n_drawn) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->cand_total >= 0, KPRN_E_ARG, "the handle has no candidate list");
  const char* why = "";
  const int rc = es::validate(group_counts, B, h->cand_total, target_offsets, target_items, n_neg, h->cand_Ve, new_group_counts, new_total, target_rows, neg_rows,
                              n_drawn, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  const int64_t total = h->cand_total, NT = target_offsets[B], n_out = NT * (int64_t)(n_neg + 1);
  std::vector<int64_t> first((size_t)B + 1), woff((size_t)B + 1), nfirst((size_t)B);
  std::vector<int32_t> tslot((size_t)NT);
  first[0] = woff[0] = 0;
  for (int32_t b = 0; b < B; ++b) {
    first[(size_t)b + 1] = first[(size_t)b] + group_counts[b];
    woff[(size_t)b + 1] = woff[(size_t)b] + (group_counts[b] + 31) / 32;
    for (int64_t k = target_offsets[b]; k < target_offsets[b + 1]; ++k) tslot[(size_t)k] = b;
  }
  const int64_t Wt = woff[(size_t)B];
  hipStream_t s = h->stream;
  // device arguments: first [B + 1] | toff [B + 1] | woff [B + 1] | nfirst [B] (int64), then tslot [NT] | titems [NT] | ndrawn [NT] | counts [B] | flag [4] |
  // the bitmaps [Wt] | the old-row -> new-row table [total] | target_rows [NT] and neg_rows [NT][n_neg], one run (int32)
  const size_t n64 = (size_t)4 * B + 3, n32 = (size_t)3 * NT + B + 4 + (size_t)Wt + (size_t)total + (size_t)n_out;
  grow_call_block(s, h->cand_buf, h->cand_buf_bytes, n64 * 8 + n32 * 4);
  int64_t* d_first = (int64_t*)h->cand_buf;
  int64_t* d_toff = d_first + B + 1;
  int64_t* d_woff = d_toff + B + 1;
  int64_t* d_nfirst = d_woff + B + 1;
  int32_t* d_tslot = (int32_t*)(d_nfirst + B);
  int32_t* d_titems = d_tslot + NT;
  int32_t* d_ndrawn = d_titems + NT;
  int32_t* d_counts = d_ndrawn + NT;
  int32_t* d_flag = d_counts + B;
  uint32_t* d_bits = (uint32_t*)(d_flag + 4);
  int32_t* d_to_new = (int32_t*)(d_bits + Wt);
  int32_t* d_rows = d_to_new + total;   // target_rows, then neg_rows
  HIP_TRY(hipMemcpyAsync(d_first, first.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_toff, target_offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_woff, woff.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_tslot, tslot.data(), (size_t)NT * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_titems, target_items, (size_t)NT * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
  if (Wt > 0) HIP_TRY(hipMemsetAsync(d_bits, 0, (size_t)Wt * sizeof(uint32_t), s));   // (the block is grow-only: an earlier call's words lie in it)
  HIP_TRY(hipMemsetAsync(d_rows, 0xFF, (size_t)n_out * sizeof(int32_t), s));          // -1: unreachable, and the padding of a short sample
  es::Args a;
  a.list = h->cand_list; a.first = d_first; a.toff = d_toff; a.woff = d_woff; a.tslot = d_tslot; a.titems = d_titems;
  a.sd = es::seed_of(seed, draw); a.n_neg = n_neg;
  a.trow = d_rows; a.neg = d_rows + NT; a.ndrawn = d_ndrawn; a.bits = d_bits; a.flag = d_flag;
  {
    ProfScope ps(h, "eval_sample_draw");
    hipLaunchKernelGGL(es::k_draw, dim3((unsigned)NT), dim3(es::TPB), 0, s, a);
    HIP_TRY(hipGetLastError());
  }
  {
    ProfScope ps(h, "eval_sample_count");
    hipLaunchKernelGGL(es::k_count, dim3((unsigned)B), dim3(es::TPB), 0, s, d_woff, d_bits, d_counts);
    HIP_TRY(hipGetLastError());
  }
  std::vector<int32_t> cnt((size_t)B), rows_out((size_t)n_out), nd((size_t)NT);
  int32_t flag = 0;
  HIP_TRY(hipMemcpyAsync(cnt.data(), d_counts, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));   // the wait for the new list's size (also covers first, woff and tslot, the sources of pageable copies)
  KPRN_REQUIRE(flag == 0, KPRN_E_DEVICE, "sample_eval_groups: a draw kept another number of rows than its cut was found for");
  int64_t n = 0;
  for (int32_t b = 0; b < B; ++b) {
    KPRN_REQUIRE(cnt[(size_t)b] >= 0 && cnt[(size_t)b] <= group_counts[b], KPRN_E_DEVICE, "sample_eval_groups: the counting pass returned an impossible count");
    nfirst[(size_t)b] = n;
    n += cnt[(size_t)b];
  }
  int32_t* list = nullptr;
  try {
    if (n > 0) {
      list = dalloc<int32_t>(2 * n);
      HIP_TRY(hipMemcpyAsync(d_nfirst, nfirst.data(), (size_t)B * 8, hipMemcpyHostToDevice, s));
      {
        ProfScope ps(h, "eval_sample_fill");
        hipLaunchKernelGGL(es::k_fill, dim3((unsigned)B), dim3(es::TPB), 0, s, h->cand_list, d_first, d_woff, d_bits, d_nfirst, d_counts, list, d_to_new, d_flag);
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));   // (the fill pass's verdict, before the table is read and the list replaces the handle's)
      KPRN_REQUIRE(flag == 0, KPRN_E_DEVICE, "sample_eval_groups: the fill pass placed a different number of rows than the counting pass allotted");
      {
        ProfScope ps(h, "eval_sample_remap");
        const unsigned grid = (unsigned)std::min<int64_t>((n_out + es::TPB - 1) / es::TPB, 2048);
        hipLaunchKernelGGL(es::k_remap, dim3(grid), dim3(es::TPB), 0, s, d_rows, n_out, d_to_new);
        HIP_TRY(hipGetLastError());
      }
    }
    // (into buffers of the call's own: a failed wait leaves the caller's arrays untouched)
    HIP_TRY(hipMemcpyAsync(rows_out.data(), d_rows, (size_t)n_out * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nd.data(), d_ndrawn, (size_t)NT * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  } catch (...) {
    hipStreamSynchronize(s);
    dfree(list);
    throw;
  }
  dfree(h->cand_list);   // (the stream is drained: nothing queued reads the old list)
  dfree(h->cand_paths);  // (the cut list has no path counts)
  h->cand_list = list; h->cand_total = n;
  std::copy(cnt.begin(), cnt.end(), new_group_counts);
  *new_total = n;
  std::copy(rows_out.begin(), rows_out.begin() + NT, target_rows);
  std::copy(rows_out.begin() + NT, rows_out.end(), neg_rows);
  std::copy(nd.begin(), nd.end(), n_drawn);
  API_END(h)
}

int kprn_host_sample_eval_groups(const int32_t* list, int64_t total, int32_t Ve, const int32_t* group_counts, int32_t B, const int64_t* target_offsets,
                                 const int32_t* target_items, int32_t n_neg, uint64_t seed, unsigned int draw, int32_t* new_group_counts, int64_t* new_total,
                                 int32_t* target_rows, int32_t* neg_rows, int32_t* n_drawn, int32_t* new_list) {
  try {
    return es::host_sample(list, total, Ve, group_counts, B, target_offsets, target_items, n_neg, seed, draw, new_group_counts, new_total, target_rows, neg_rows,
                           n_drawn, new_list);
  } catch (...) { return KPRN_E_NOMEM; }
}

}  // extern "C"
