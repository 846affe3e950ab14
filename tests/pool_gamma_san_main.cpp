// The host twin of the explanation stage under a pooling temperature (kprn_host_explain_gamma, kprn_amd/csrc/explain_paths.hip) as a stand-alone program, for
// tests/test_pool_gamma_host.py to build with the host sanitizers (address, undefined) and run: every array is a heap block of exactly its size, so a read
// or write past an end is reported.  The program never touches a GPU.
//   pool_gamma_san IN OUT
// IN:  int32 {N, C, B, class_id, reducer, K_reducer, n_pairs, M, have_pairs}, float gamma, float scores[N * C], int32 offsets[B + 1], int32 pairs[n_pairs]
//      (only if have_pairs)
// OUT: int32 status, int32 path_idx[n * m], float path_score[n * m], float path_weight[n * m], float pooled[n], float probs[n], with n = max(n_pairs, 0)
//      and m = max(M, 1)  (all poisoned with -77 before the call)
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "kprn.h"

template <typename T> static T* take(FILE* f, int64_t n) {
  T* p = (T*)malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0 && fread(p, sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short input\n"); exit(2); }
  return p;
}
template <typename T> static T* poisoned(int64_t n) {
  T* p = (T*)malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  for (int64_t i = 0; i < n; ++i) p[i] = (T)-77;
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t* hd = take<int32_t>(f, 9);
  const int32_t N = hd[0], C = hd[1], B = hd[2], class_id = hd[3], reducer = hd[4], K = hd[5], n_pairs = hd[6], M = hd[7], have_pairs = hd[8];
  float* gamma = take<float>(f, 1);
  float* scores = take<float>(f, (int64_t)N * C);
  int32_t* off = take<int32_t>(f, (int64_t)B + 1);
  int32_t* pairs = have_pairs ? take<int32_t>(f, n_pairs) : nullptr;
  fclose(f);
  const int64_t n = n_pairs > 0 ? n_pairs : 0, m = M > 1 ? M : 1;
  int32_t* idx = poisoned<int32_t>(n * m);
  float* score = poisoned<float>(n * m);
  float* weight = poisoned<float>(n * m);
  float* pooled = poisoned<float>(n);
  float* probs = poisoned<float>(n);
  const int32_t rc = kprn_host_explain_gamma(scores, off, B, C, class_id, reducer, K, pairs, n_pairs, M, idx, score, weight, pooled, probs, *gamma);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(&rc, 4, 1, o);
  fwrite(idx, 4, (size_t)(n * m), o);
  fwrite(score, 4, (size_t)(n * m), o);
  fwrite(weight, 4, (size_t)(n * m), o);
  fwrite(pooled, 4, (size_t)n, o);
  fwrite(probs, 4, (size_t)n, o);
  fclose(o);
  free(hd); free(gamma); free(scores); free(off); free(pairs); free(idx); free(score); free(weight); free(pooled); free(probs);
  return 0;
}
