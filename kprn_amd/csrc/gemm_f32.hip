// Generic GEMM on the gfx950 MFMA: fp32 (v_mfma_f32_16x16x4_f32, exact f32, 157 TF peak) or, compute_dtype = bf16,
// bf16 products with fp32 accumulation (v_mfma_f32_16x16x16_bf16; operands stay fp32 in HBM / LDS and are rounded to
// nearest-even bf16 as the fragments are formed -- BASELINE.json configs[3] "bf16 MFMA LSTM", first step: the
// arithmetic; bf16 storage and a fused bf16 kernel are later rounds).
//
// This is the shape-agnostic fallback of the engine: any M, N, K, any operand strides
// (so A*B^T, A*B and A^T*B are one kernel), boundary-checked, optional split-K.  The
// fused LSTM kernels (lstm_fused_*.hip) replace it on the shapes they cover; it stays the
// reference GPU path for odd sizes (e.g. the shipped config's H=250, D=200,
// release/songPathRnn/run_scripts/config.sh:20-23).
//
// Replaces the TH/THC BLAS calls under nn.Linear / FastLSTM's i2g,o2g
// (release/songPathRnn/model/OneModel.lua:236,275).
#include <stdlib.h>

#include <algorithm>

#include "gemm_f32_kernels.h"

namespace gemm {

void run(hipStream_t s, const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C,
         int64_t ldc, int64_t M, int N, int64_t K, bool accumulate, const float* bias, int split_k, bool bf16, bool untiled, DetScratch* det) {
  if (M <= 0 || N <= 0) return;
  if (split_k < 1) split_k = 1;
  KPRN_REQUIRE(!(det && bf16), KPRN_E_UNSUPPORTED, "deterministic: the bf16 products have no slab form");
  if (det && !accumulate) det = nullptr;   // (a stored product has one split: nothing to join)
  static const bool no_tiled = getenv("KPRN_NO_TILED_GEMM") != nullptr;  // (measurement: the round-1 kernels)
  if (!bf16 && !no_tiled && !untiled && run_tiled(s, A, sAm, sAk, B, sBk, sBn, C, ldc, M, N, K, accumulate, bias, split_k, det)) return;
  if (det) split_k = (int)std::max<int64_t>(1, std::min<int64_t>(split_k, DET_SLAB_FLOATS / (M * N)));   // (a function of the shape only)
  int64_t kchunk = (K + split_k - 1) / split_k;
  kchunk = ((kchunk + BK - 1) / BK) * BK;
  if (kchunk <= 0) kchunk = BK;
  split_k = (int)((K + kchunk - 1) / kchunk);
  if (split_k < 1) split_k = 1;
  KPRN_REQUIRE(!(split_k > 1 && !accumulate), KPRN_E_ARG, "gemm: split-K needs accumulate mode");
  const int use_atomic = split_k > 1 ? 1 : 0;
  const bool akc = (sAk == 1), bnc = (sBn == 1);
  const bool big = (M >= 100 && N >= 100);
  if (det && split_k > 1) {   // deterministic mode: the same grid and K ranges, the partials into slabs, joined in split order (gemm_f32_slab.hip)
    run_untiled_slab(s, A, sAm, sAk, B, sBk, sBn, C, ldc, M, N, K, kchunk, split_k, det);
    return;
  }
  if (big) {
    kchunk = ((kchunk + GK - 1) / GK) * GK;
    dim3 grid((unsigned)((M + GM - 1) / GM), (unsigned)((N + GN - 1) / GN), (unsigned)split_k);
#define LAUNCHB(AK, BNC)                                                                                           \
  do {                                                                                                             \
    if (bf16)                                                                                                      \
      hipLaunchKernelGGL((gemm_kernel_big<AK, BNC, true>), grid, dim3(256), 0, s, A, sAm, sAk, B, sBk, sBn, C, ldc, M, N, K, \
                         accumulate ? 1 : 0, bias, kchunk, use_atomic);                                            \
    else                                                                                                           \
      hipLaunchKernelGGL((gemm_kernel_big<AK, BNC, false>), grid, dim3(256), 0, s, A, sAm, sAk, B, sBk, sBn, C, ldc, M, N, K, \
                         accumulate ? 1 : 0, bias, kchunk, use_atomic);                                            \
  } while (0)
    if (akc && bnc) LAUNCHB(true, true);
    else if (akc && !bnc) LAUNCHB(true, false);
    else if (!akc && bnc) LAUNCHB(false, true);
    else LAUNCHB(false, false);
#undef LAUNCHB
    HIP_TRY(hipGetLastError());
    return;
  }
  dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((N + BN - 1) / BN), (unsigned)split_k);
#define LAUNCH(AK, BNC)                                                                                            \
  do {                                                                                                             \
    if (bf16)                                                                                                      \
      hipLaunchKernelGGL((gemm_kernel<AK, BNC, true>), grid, dim3(256), 0, s, A, sAm, sAk, B, sBk, sBn, C, ldc, M, N, K, \
                         accumulate ? 1 : 0, bias, kchunk, use_atomic);                                            \
    else                                                                                                           \
      hipLaunchKernelGGL((gemm_kernel<AK, BNC, false>), grid, dim3(256), 0, s, A, sAm, sAk, B, sBk, sBn, C, ldc, M, N, K, \
                         accumulate ? 1 : 0, bias, kchunk, use_atomic);                                            \
  } while (0)
  if (akc && bnc) LAUNCH(true, true);
  else if (akc && !bnc) LAUNCH(true, false);
  else if (!akc && bnc) LAUNCH(false, true);
  else LAUNCH(false, false);
#undef LAUNCH
  HIP_TRY(hipGetLastError());
}

}  // namespace gemm
