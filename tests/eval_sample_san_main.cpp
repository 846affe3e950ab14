// The host twin of kprn_sample_eval_groups (kprn_amd/csrc/eval_sample_host.h) as a stand-alone program, for tests/test_eval_sample_host.py to build with
// -fsanitize=address,undefined and run: every array is a heap block of exactly its size, so a read or write past an end is reported.
//   eval_sample_san IN OUT
// IN:  int64 {total, Ve, B, NT, n_neg, seed, draw}, int32 list[2 total], int32 group_counts[B], int64 target_offsets[B + 1], int32 target_items[NT]
// OUT: int64 {status, new_total}, int32 new_group_counts[B], target_rows[NT], neg_rows[NT n_neg], n_drawn[NT] (all poisoned with -77 before the call), and
//      after a successful call int32 new_list[2 new_total]: the twin is called once without the rows, then again with a block of exactly new_total rows
#include <cstdio>
#include <cstdlib>

#include "eval_sample_host.h"

template <typename T> static T* take(FILE* f, int64_t n) {
  T* p = (T*)malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0 && fread(p, sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short input\n"); exit(2); }
  return p;
}
static int32_t* poisoned(int64_t n) {
  int32_t* p = (int32_t*)malloc(n > 0 ? (size_t)n * 4 : 1);
  for (int64_t i = 0; i < n; ++i) p[i] = -77;
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t* hd = take<int64_t>(f, 7);
  const int64_t total = hd[0], Ve = hd[1], B = hd[2], NT = hd[3], n_neg = hd[4], seed = hd[5], draw = hd[6];
  int32_t* list = take<int32_t>(f, 2 * total);
  int32_t* gc = take<int32_t>(f, B);
  int64_t* toff = take<int64_t>(f, B + 1);
  int32_t* titems = take<int32_t>(f, NT);
  fclose(f);
  const int64_t nn = n_neg > 0 ? NT * n_neg : 0;
  int32_t *ngc = poisoned(B), *trow = poisoned(NT), *neg = poisoned(nn), *nd = poisoned(NT), *new_list = nullptr;
  int64_t new_total = -77;
  int64_t rc = es::host_sample(list, total, (int32_t)Ve, gc, (int32_t)B, toff, titems, (int32_t)n_neg, (uint64_t)seed, (unsigned int)draw, ngc, &new_total, trow,
                               neg, nd, nullptr);
  if (rc == KPRN_OK) {
    new_list = poisoned(2 * new_total);
    rc = es::host_sample(list, total, (int32_t)Ve, gc, (int32_t)B, toff, titems, (int32_t)n_neg, (uint64_t)seed, (unsigned int)draw, ngc, &new_total, trow, neg, nd,
                         new_list);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(&rc, 8, 1, o);
  fwrite(&new_total, 8, 1, o);
  if (B > 0) fwrite(ngc, 4, (size_t)B, o);
  if (NT > 0) fwrite(trow, 4, (size_t)NT, o);
  if (nn > 0) fwrite(neg, 4, (size_t)nn, o);
  if (NT > 0) fwrite(nd, 4, (size_t)NT, o);
  if (new_list && new_total > 0) fwrite(new_list, 4, (size_t)(2 * new_total), o);
  fclose(o);
  free(hd); free(list); free(gc); free(toff); free(titems); free(ngc); free(trow); free(neg); free(nd); free(new_list);
  return 0;
}
