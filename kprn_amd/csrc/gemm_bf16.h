// What the bf16 pipeline (lstm_bf16.hip) uses of the bf16 products (gemm_bf16.hip).  Every product takes the handle's A/B switches (Bf16GemmOpts, by value)
// and `zero`: >= 16 zero bytes on the launch's device, the source of every out-of-range LDS-DMA piece (owned by the pipeline's State).
#pragma once
#include "kprn_internal.h"

namespace bf16p {

typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16 tobf(float x) { return (bf16)x; }   // round to nearest even

struct GArgs {
  const bf16* A; int64_t lda; const bf16* B; int64_t ldb; int64_t K;
  const bf16* A2; int64_t lda2; const bf16* B2; int64_t ldb2; int64_t K2;   // second K segment (recurrent half)
  float* C; int64_t ldc; int64_t M; int N; const float* bias;
  int64_t kchunk; int use_atomic; int nsplit;
  int64_t mtiles; int ntiles;
  // EPI_LSTM: N = 4H gate-major rows of B; a column tile = 32 hidden units x 4 gates
  int H; const float* cprev; float* cout; bf16* hout; int64_t ldh; bf16* act; float* hout_f32;
};

// what a launcher ran (host code only; filled where a caller passes one: kprn_debug_gemm16_run).  kernel: the KPRN_GEMM16_* of include/kprn.h
struct Ran { int kernel = KPRN_GEMM16_DECLINED; int nsplit = 0; int64_t kchunk = 0; };

// C[M][N] (fp32) = or += A[M][K] B[N][K]^T; K, lda, ldb multiples of 8 elements, 16-byte aligned pointers
void gemm16(hipStream_t s, Bf16GemmOpts o, const bf16* zero, const bf16* A, int64_t lda, const bf16* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int64_t K,
            bool accumulate, const float* bias, int split_k, Ran* ran = nullptr);
// what gemm16 runs after gemm16x declines: k_gemm16 alone (any M, N; a bias with the storing form only)
void gemm16_plain(hipStream_t s, const bf16* A, int64_t lda, const bf16* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int64_t K,
                  bool accumulate, const float* bias, int split_k, Ran* ran = nullptr);
// the same on the LDS-DMA kernels alone; false = shape not covered.  Rows n >= n_lo of B are known to be zero for k < k_lo; at least sx_min K ranges per XCD
bool gemm16x(hipStream_t s, Bf16GemmOpts o, const bf16* zero, const bf16* A, int64_t lda, const bf16* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int64_t K,
             bool accumulate, int split_k, int n_lo = 0, int64_t k_lo = 0, int sx_min = 1, Ran* ran = nullptr);
// C[(step, path)][N] (fp32) = sum_k AT[k][step Np + path] B[n][k]: the k-major A operand (gx::k_gemm16xt); false = shape not covered
bool gemm16xt(hipStream_t s, const bf16* zero, const bf16* AT, int64_t ldat, const bf16* B, int64_t ldb, float* C, int64_t ldc, int64_t Mp, int N, int64_t K, int64_t Np, int64_t Nv,
              Ran* ran = nullptr);
bool dx_from_transposed_ok(int64_t Mp, int N, int64_t K, int64_t Np);   // (the BPTT launch asks before it drops its row-major copy of dA)
// one FastLSTM step, the cell as the product's epilogue: the caller fills the operands, M, H, bias and the cell's planes; the tile geometry is chosen here
void lstm_step16(hipStream_t s, GArgs a);
// lstm_bf16.hip: y[0 .. n) = bf16(x) (debug_gemm16's operands)
void cvt16(hipStream_t s, const float* x, bf16* y, int64_t n);

}  // namespace bf16p
