// The host twin of kprn_select_hardest (kprn_amd/csrc/select_hardest.h) as a stand-alone program, for tests/test_select_hardest_host.py to build with
// -fsanitize=address,undefined and run: every array is a heap block of exactly its size, so a read or write past an end is reported.
//   select_hardest_san IN OUT
// IN:  int64 {n_scores, G, M (-1: members NULL), has_pos, n_keep, keep_len}, float scores[n_scores], int64 members[M], int64 group_offsets[G + 1],
//      int32 pos[G] (when has_pos)
// OUT: int64 status, int64 n_invalid, uint8 keep[keep_len]  (poisoned with -77 / 77 before the call)
#include <cstdio>
#include <cstdlib>

#include "select_hardest.h"

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
  const int64_t n_scores = hd[0], G = hd[1], M = hd[2], has_pos = hd[3], n_keep = hd[4], keep_len = hd[5];
  float* scores = take<float>(f, n_scores);
  int64_t* members = M >= 0 ? take<int64_t>(f, M) : nullptr;
  int64_t* goff = take<int64_t>(f, G + 1);
  int32_t* pos = has_pos ? take<int32_t>(f, G) : nullptr;
  fclose(f);
  unsigned char* keep = (unsigned char*)malloc(keep_len > 0 ? (size_t)keep_len : 1);
  for (int64_t i = 0; i < keep_len; ++i) keep[i] = 77;
  int64_t n_invalid = -77;
  const int64_t rc = sh::host_select(scores, n_scores, members, goff, pos, (int32_t)G, (int32_t)n_keep, keep, &n_invalid);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(&rc, 8, 1, o);
  fwrite(&n_invalid, 8, 1, o);
  if (keep_len > 0) fwrite(keep, 1, (size_t)keep_len, o);
  fclose(o);
  free(hd); free(scores); free(members); free(goff); free(pos); free(keep);
  return 0;
}
