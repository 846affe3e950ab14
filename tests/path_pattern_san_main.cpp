// The table builder and the match of the meta-paths (kprn_amd/csrc/path_pattern_dev.h) as a stand-alone program, for tests/test_meta_path_host.py to build
// with -fsanitize=address,undefined and run: every array is a heap block of exactly its size, so a read or write past an end is reported.
//   path_pattern_san IN OUT
// IN:  int64 {Vr, n_seq, seq_len}, int64 {n, n_rels}, then (n > 0) int32 hops[n], int64 set_offsets[sum(hops) + 1], int32 set_rels[n_rels]; then
//      int32 seqs[seq_len]: n_seq times (h, r_0 .. r_{h-1})
// OUT: uint8 status (the validation's), uint8 match[n_seq]  (poisoned with 77 before the calls)
#include <cstdio>
#include <cstdlib>

#include "path_pattern_dev.h"

template <typename T> static T* take(FILE* f, int64_t n) {
  T* p = (T*)malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0 && fread(p, sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short input\n"); exit(2); }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t* hd = take<int64_t>(f, 3);
  const int64_t Vr = hd[0], n_seq = hd[1], seq_len = hd[2];
  int64_t* ph = take<int64_t>(f, 2);
  const int64_t n = ph[0], n_rels = ph[1];
  int32_t* hops = n > 0 ? take<int32_t>(f, n) : nullptr;
  int64_t S = 0;
  for (int64_t p = 0; p < n; ++p) S += hops[p];
  int64_t* offs = n > 0 ? take<int64_t>(f, S + 1) : nullptr;
  int32_t* rels = n > 0 && n_rels > 0 ? take<int32_t>(f, n_rels) : nullptr;
  int32_t* seqs = take<int32_t>(f, seq_len);
  fclose(f);
  unsigned char* out = (unsigned char*)malloc((size_t)n_seq + 1);
  for (int64_t k = 0; k <= n_seq; ++k) out[k] = 77;
  const int rc = pat::validate(hops, offs, rels, (int32_t)n, (int32_t)Vr, nullptr);
  out[0] = (unsigned char)(rc == KPRN_OK ? 0 : 1);
  uint32_t* match = (uint32_t*)malloc((size_t)pat::table_words((int32_t)Vr) * sizeof(uint32_t));   // exactly 5 (Vr + 1) words
  pat::Table t{match, (int)Vr + 1, {0, 0, 0, 0, 0, 0}};
  if (rc == KPRN_OK) {
    pat::build(hops, offs, rels, (int32_t)n, (int32_t)Vr, match, t.len);
    int64_t at = 0;
    for (int64_t k = 0; k < n_seq; ++k) {
      const int h = seqs[at];
      int32_t* one = (int32_t*)malloc((size_t)h * sizeof(int32_t));   // a block of the sequence's own size
      for (int j = 0; j < h; ++j) one[j] = seqs[at + 1 + j];
      out[1 + k] = pat::matches(t, one, h) ? 1 : 0;
      free(one);
      at += 1 + h;
    }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(out, 1, (size_t)n_seq + 1, o);
  fclose(o);
  free(hd); free(ph); free(hops); free(offs); free(rels); free(seqs); free(out); free(match);
  return 0;
}
