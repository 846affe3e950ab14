// The host twin of kprn_rank_targets (kprn_amd/csrc/rank_targets_host.h) as a stand-alone program, for tests/test_rank_targets_host.py to build with
// -fsanitize=address,undefined and run: every array is a heap block of exactly its size, so a read or write past an end is reported.
//   rank_targets_san IN OUT
// IN:  int64 {n_scores, G, M (-1: members NULL), NT, mode, hist_len}, float scores[n_scores], int64 members[M], int64 group_offsets[G + 1],
//      int64 target_offsets[G + 1], int32 targets[NT]
// OUT: int64 status, int32 places[NT], int64 hist[hist_len + 4]  (both poisoned with -77 before the call)
#include <cstdio>
#include <cstdlib>

#include "rank_targets_host.h"

template <typename T> static T* take(FILE* f, int64_t n) {
  T* p = (T*)malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0 && fread(p, sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short input\n"); exit(2); }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t* hd = take<int64_t>(f, 6);
  const int64_t n_scores = hd[0], G = hd[1], M = hd[2], NT = hd[3], mode = hd[4], hist_len = hd[5];
  float* scores = take<float>(f, n_scores);
  int64_t* members = M >= 0 ? take<int64_t>(f, M) : nullptr;
  int64_t* goff = take<int64_t>(f, G + 1);
  int64_t* toff = take<int64_t>(f, G + 1);
  int32_t* targets = take<int32_t>(f, NT);
  fclose(f);
  const int64_t nh = hist_len >= 0 ? hist_len + 4 : 4;
  int32_t* places = (int32_t*)malloc(NT > 0 ? (size_t)NT * 4 : 1);
  int64_t* hist = (int64_t*)malloc((size_t)nh * 8);
  for (int64_t i = 0; i < NT; ++i) places[i] = -77;
  for (int64_t i = 0; i < nh; ++i) hist[i] = -77;
  const int64_t rc = rt::host_rank_targets(scores, n_scores, members, goff, toff, targets, (int32_t)G, (int32_t)mode, places, hist, (int32_t)hist_len);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(&rc, 8, 1, o);
  if (NT > 0) fwrite(places, 4, (size_t)NT, o);
  fwrite(hist, 8, (size_t)nh, o);
  fclose(o);
  free(hd); free(scores); free(members); free(goff); free(toff); free(targets); free(places); free(hist);
  return 0;
}
