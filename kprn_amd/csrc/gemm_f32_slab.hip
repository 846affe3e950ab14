// Option "deterministic" = "2" (DESIGN.md 3.11): the slab forms of gemm_f32.hip's two untiled kernels -- the same tiles, grids and K ranges as the split-K launch
// with atomics, but split s plain-stores its partial product into slab s of a scratch [splits][M][N], and kk::slab_join, the launch behind, adds the slabs to C
// in split order.  A translation unit of its own: gemm_f32.hip keeps the kernels it always had.
#include "gemm_f32_kernels.h"

namespace gemm {

// kchunk / split_k: as gemm::run derived them (split_k > 1, fp32 products)
void run_untiled_slab(hipStream_t s, const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc, int64_t M, int N,
                      int64_t K, int64_t kchunk, int split_k, DetScratch* det) {
  float* const slabs = kk::det_reserve(det, s, (int64_t)split_k * M * N);
  const bool akc = (sAk == 1), bnc = (sBn == 1);
  const bool big = (M >= 100 && N >= 100);
  if (big) kchunk = ((kchunk + GK - 1) / GK) * GK;
  const dim3 grid = big ? dim3((unsigned)((M + GM - 1) / GM), (unsigned)((N + GN - 1) / GN), (unsigned)split_k)
                        : dim3((unsigned)((M + BM - 1) / BM), (unsigned)((N + BN - 1) / BN), (unsigned)split_k);
  const float* const nobias = nullptr;
#define LAUNCHS(AK, BNC)                                                                                                                                    \
  do {                                                                                                                                                      \
    if (big) hipLaunchKernelGGL((gemm_kernel_big<AK, BNC, false, true>), grid, dim3(256), 0, s, A, sAm, sAk, B, sBk, sBn, slabs, (int64_t)N, M, N, K, 0, nobias, kchunk, 0);  \
    else hipLaunchKernelGGL((gemm_kernel<AK, BNC, false, true>), grid, dim3(256), 0, s, A, sAm, sAk, B, sBk, sBn, slabs, (int64_t)N, M, N, K, 0, nobias, kchunk, 0);          \
  } while (0)
  if (akc && bnc) LAUNCHS(true, true);
  else if (akc && !bnc) LAUNCHS(true, false);
  else if (!akc && bnc) LAUNCHS(false, true);
  else LAUNCHS(false, false);
#undef LAUNCHS
  HIP_TRY(hipGetLastError());
  kk::slab_join(s, slabs, split_k, M * N, M, N, C, ldc);
}

}  // namespace gemm
