// A batch from the kept pairs of a batch (include/kprn.h "hard negatives", kprn_batch_subset): the kept pairs' rows are taken from the source batch where
// they lie in HBM -- nothing is found, sampled or uploaded again, so the rows trained on are the rows that were scored.
//
// The new batch goes through slots::create with a DeviceFill, as the path finder's does: its counts come from the host (the source's ragged plan, or P), the
// fill is k_gather_rows below, and create derives validation, the identical-prefix plan, the occurrence index and the ragged plan as for any batch.  The
// labels follow by k_gather_labels on the same stream behind create (create uploads zeros into the label block first), so the call has create's one wait.
//
// k_gather_rows is flat over the OUTPUT's 32-bit words: thread w writes word w, adjacent threads read adjacent words of a source row (rows are T * F words,
// any number: nothing assumes a multiple of 4).  The output path of a word is w / (T F); its pair is found by bisection in the output's pair offsets (at most
// 12 steps over a table that stays in cache), and the source row is the pair's first source row plus the path's index within the pair.  Word indices are
// 32-bit unless a batch's N T F needs more.
#include "kprn_internal.h"

namespace bsub {

// dst_off [Bk + 1]: first output path of every kept pair; src_first [Bk]: its first path in the source
template <typename IX>
__global__ __launch_bounds__(256) void k_gather_rows(const int32_t* __restrict__ src, const int32_t* __restrict__ dst_off, const int32_t* __restrict__ src_first,
                                                     int Bk, IX row_words, IX n_words, int32_t* __restrict__ dst) {
  const IX w = (IX)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_words) return;
  const IX path = w / row_words, col = w - path * row_words;
  int lo = 0, hi = Bk;   // the last pair whose first path is <= path
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((IX)dst_off[mid] <= path) lo = mid; else hi = mid;
  }
  const IX from = (IX)src_first[lo] + (path - (IX)dst_off[lo]);
  dst[w] = src[from * row_words + col];
}

__global__ __launch_bounds__(256) void k_gather_labels(const float* __restrict__ src, const int32_t* __restrict__ kept_pair, int Bk, float* __restrict__ dst) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < Bk) dst[b] = src[kept_pair[b]];
}

}  // namespace bsub

extern "C" int kprn_batch_subset(kprn_handle* h, const kprn_batch* src, const unsigned char* keep, kprn_batch** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out, KPRN_E_ARG, "out is NULL");
  *out = nullptr;
  KPRN_REQUIRE(src && keep, KPRN_E_ARG, "NULL argument");
  slots::ready(h, src);   // (a fed slot nobody used yet is waited for; KPRN_E_INDEX for contents with a bad id, or for a slot without contents)
  KPRN_REQUIRE(src->idx_valid, KPRN_E_ARG, "kprn_batch_subset: the batch does not hold its ids in the caller's order (a label-less fed batch with a plan)");
  const int32_t B = src->B, T = src->T, F = src->F;
  const bool ragged = src->off != nullptr;
  // the kept pairs: counts, first paths in the output and in the source
  std::vector<int32_t> counts, dst_off(1, 0), src_first, kept_pair;
  int64_t N = 0;
  for (int32_t b = 0; b < B; ++b) {
    if (!keep[b]) continue;
    const int32_t first = ragged ? src->hrag[(size_t)b] : b * src->P, cnt = ragged ? src->hrag[(size_t)b + 1] - first : src->P;
    counts.push_back(cnt); src_first.push_back(first); kept_pair.push_back(b);
    N += cnt;
    dst_off.push_back((int32_t)N);   // (N <= the source's paths, which fit 32 bits)
  }
  const int32_t Bk = (int32_t)counts.size();
  if (Bk > 0) {
    hipStream_t s = h->stream;
    // device arguments: dst_off [Bk + 1] | src_first [Bk] | kept_pair [Bk]
    const size_t w_off = ((size_t)Bk + 1 + 3) & ~(size_t)3, w_first = ((size_t)Bk + 3) & ~(size_t)3, total = (w_off + 2 * w_first) * 4;
    int32_t* d_off = (int32_t*)grow_call_block(s, h->sub_buf, h->sub_buf_bytes, total);
    int32_t* d_first = d_off + w_off;
    int32_t* d_pair = d_first + w_first;
    HIP_TRY(hipMemcpyAsync(d_off, dst_off.data(), (size_t)(Bk + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_first, src_first.data(), (size_t)Bk * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_pair, kept_pair.data(), (size_t)Bk * 4, hipMemcpyHostToDevice, s));
    const int64_t row_words = (int64_t)T * F, n_words = N * row_words;
    const bool wide = std::max(src->N, N) * row_words > 0xffffffffll;   // (a word index of either batch leaves 32 bits)
    const slots::DeviceFill fill = [&](int32_t* idx_dev, hipStream_t st) {
      ProfScope ps(h, "batch_subset_gather", st);
      const unsigned grid = (unsigned)((n_words + 255) / 256);
      if (wide) hipLaunchKernelGGL(bsub::k_gather_rows<int64_t>, dim3(grid), dim3(256), 0, st, src->idx, d_off, d_first, Bk, row_words, n_words, idx_dev);
      else hipLaunchKernelGGL(bsub::k_gather_rows<uint32_t>, dim3(grid), dim3(256), 0, st, src->idx, d_off, d_first, Bk, (uint32_t)row_words, (uint32_t)n_words, idx_dev);
      HIP_TRY(hipGetLastError());
    };
    const std::vector<float> zeros(src->labels ? (size_t)Bk : 0, 0.f);   // (create sizes and fills the label block; the labels themselves follow below)
    kprn_batch* nb = nullptr;
    slots::create(h, nullptr, counts.data(), src->labels ? zeros.data() : nullptr, Bk, 0, N, T, F, &nb, &fill);   // (drains the stream: the locals above were read)
    if (src->labels) {
      hipLaunchKernelGGL(bsub::k_gather_labels, dim3((unsigned)((Bk + 255) / 256)), dim3(256), 0, s, src->labels, d_pair, Bk, nb->labels);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) { kprn_batch_destroy(h, nb); HIP_TRY(e); }
    }
    *out = nb;
  }
  API_END(h)
}
