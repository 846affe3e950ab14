// The bf16 products of the bf16 pipeline (lstm_bf16.hip; gemm_bf16.h is what it sees of this file): C[M,N] (fp32) = or += A[M,K] B[N,K]^T on bf16
// operands with fp32 accumulation.  gfx950 only.
//
// k_gemm16: both operands k-contiguous bf16 (16-byte = 8-element global loads, LDS tiles [128][64 + 8], one ds_read_b128 per MFMA operand of
// v_mfma_f32_16x16x32_bf16), 128 x 128 x 64 or 256 x 256 x 64 tiles, XCD-aware order; its epilogues store, accumulate (split-K) or run the FastLSTM cell
// (the forward's step kernel).  namespace gx: the same product on 256 x 128 x 64 tiles of v_mfma_f32_32x32x16_bf16 with LDS-DMA operand staging
// (k_gemm16x), with a k-major A operand (k_gemm16xt), and the two measured alternatives of the split-K launch that option keys and tests still reach
// (k_gemm16r, k_gemm16p).  Behind the kernels: their launchers, the split-K planner and the predicate of the k-major product.
#include <string.h>

#include <algorithm>

#include "gate_math.h"
#include "gemm_bf16.h"

namespace bf16p {

constexpr int TK = 64, LDB = TK + 8;   // LDS row pitch in elements (144 bytes)

// gate functions: sigm_e2 / tanh_e2 of gate_math.h (v_exp_f32 / v_rcp_f32: at bf16 precision the cell's transcendental functions,
// not the MFMAs, were most of this kernel's time with libm's expf / tanhf, ~40 instructions each against ~17 cycles per 16 KFLOP MFMA)
enum { EPI_STORE = 0, EPI_ACCUM = 1, EPI_LSTM = 2 };

// Tile geometry. BIG = 0: 128 x 128 block, 4 waves (2 x 2), 64 x 64 per wave, two blocks per CU.
// BIG = 1: 256 x 256 block, 8 waves (2 x 4), 128 x 64 per wave, one block per CU (half the L2 -> LDS bytes and LDS reads per MFMA).
// Measured on the configs[3] step GEMM (65 536 x 1 536 x 768, 0.27 ms either way, profiles/r02/README.md): the launch is not bound
// by the matrix cores (compiling the MFMAs out saves 6 %) but by the un-overlapped sum of the operand stream, the cell epilogue
// (10 transcendentals per cell, c_prev read) and the h / c / gate stores -- 0.5 GB of HBM traffic per launch against 62 us of MFMA
// work. The 256-wide geometry is therefore only taken for plain GEMMs with >= 512 such tiles, where it trims the operand re-reads.
template <int BIG> struct Geo {
  static constexpr int TMx = BIG ? 256 : 128, TNx = TMx, NT = BIG ? 512 : 256;
  static constexpr int RSTEP = NT / 8;            // tile rows covered by one 16-byte load of every thread
  static constexpr int WN = BIG ? 4 : 2;          // waves along the columns
  static constexpr int FI = BIG ? 8 : 4;          // 16-row fragments per wave
  static constexpr int HC = TNx / 4;              // EPI_LSTM: hidden units per block (x 4 gates = TNx columns)
  static constexpr int TILE = TMx * LDB;          // elements of one operand tile in LDS
};

// pieces of one [TMx][64] bf16 tile: running pointers, clamped loads, zeroing at the LDS write (as gemm_tiled.hip's TileLoader)
template <int RSTEP>
struct Loader {
  const bf16* p[4]; const bf16* safe; bool rok[4]; int kq;
  __device__ __forceinline__ void init(const bf16* __restrict__ P, int64_t ld, int64_t r0, int64_t rmax, int64_t k0, const int* rowmap) {
    const int tid = threadIdx.x;
    safe = P; kq = (tid & 7) * 8;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = (tid >> 3) + RSTEP * e;
      int64_t gr = r0 + row;
      bool ok = gr < rmax;
      if (rowmap) { const int mr = rowmap[row]; ok = mr >= 0; gr = mr; }
      rok[e] = ok;
      p[e] = P + (ok ? gr : 0) * ld + k0 + kq;
    }
  }
  __device__ __forceinline__ unsigned load(int64_t k0, int64_t kend, bf16x8 (&v)[4]) {
    unsigned mask = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = rok[e] && (k0 + kq < kend);
      v[e] = *(const bf16x8*)(ok ? p[e] : safe);
      mask |= ok ? (1u << e) : 0u;
      p[e] += TK;
    }
    return mask;
  }
};
template <int RSTEP>
__device__ __forceinline__ void tile_store(bf16* __restrict__ T, const bf16x8 (&v)[4], unsigned mask) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bf16x8 x = v[e];
    if (!((mask >> e) & 1u)) {
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = (bf16)0.f;
    }
    *(bf16x8*)(T + ((tid >> 3) + RSTEP * e) * LDB + (tid & 7) * 8) = x;
  }
}

// The MFMA takes the B fragment as its first operand and the A fragment as its second: the 16 x 16 result block then comes out
// transposed in the lanes -- lane (arow, ag) holds C[row = arow][col = 4 ag .. 4 ag + 3] -- so every lane owns FOUR CONSECUTIVE
// COLUMNS of one row and the epilogues store 8 / 16 bytes per lane (h, the gate activations, c) instead of 2 / 4.
template <int EPI, int BIG>
__global__ __launch_bounds__(Geo<BIG>::NT, BIG ? 1 : 2) void k_gemm16(GArgs a) {
  using G = Geo<BIG>;
  constexpr int TMx = G::TMx, TNx = G::TNx, FI = G::FI, HC = G::HC, TILE = G::TILE, RS = G::RSTEP;
  extern __shared__ __attribute__((aligned(16))) bf16 lds16[];
  auto As = [&](int i) -> bf16* { return lds16 + i * (2 * TILE); };
  auto Bs = [&](int i) -> bf16* { return lds16 + i * (2 * TILE) + TILE; };
  __shared__ int rowmap[TNx];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / G::WN, wn = wave % G::WN, arow = lane & 15, ag = lane >> 4;
  const int64_t id = blockIdx.x;
  const int xcd = (int)(id & 7);
  const int64_t j = id >> 3;
  int nt_idx; int64_t mt_idx, split_idx = 0;
  if (a.nsplit > 1) {   // all tiles of one K range on one XCD (gemm_tiled.hip)
    const int64_t tiles = a.mtiles * a.ntiles;
    split_idx = (j / tiles) * 8 + xcd;
    const int64_t tl = j % tiles;
    mt_idx = tl / a.ntiles; nt_idx = (int)(tl % a.ntiles);
    if (split_idx >= a.nsplit) return;
  } else {
    nt_idx = (int)(j % a.ntiles);
    mt_idx = (j / a.ntiles) * 8 + xcd;
    if (mt_idx >= a.mtiles) return;
  }
  const int64_t m0 = mt_idx * TMx;
  const int n0 = nt_idx * TNx;
  constexpr bool CELL = (EPI == EPI_LSTM);
  if (CELL) {
    if (tid < TNx) {
      const int q = tid / HC, u = nt_idx * HC + (tid % HC);
      rowmap[tid] = (u < a.H) ? q * a.H + u : -1;
    }
    __syncthreads();
  }
  const int* rmap = CELL ? rowmap : nullptr;
  const int64_t k_beg = split_idx * a.kchunk;
  const int64_t k_end1 = (k_beg + a.kchunk < a.K) ? k_beg + a.kchunk : a.K;
  const int64_t nch1 = (k_end1 > k_beg) ? (k_end1 - k_beg + TK - 1) / TK : 0;
  const int64_t nch2 = (a.A2 != nullptr) ? (a.K2 + TK - 1) / TK : 0;
  const int64_t nch = nch1 + nch2;
  f32x4 acc[FI][4];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ra[4], rb[4];
  unsigned ma = 0, mb = 0;
  Loader<RS> la, lb;
  const int64_t brow0 = CELL ? 0 : n0, bmax = CELL ? (int64_t)4 * a.H : (int64_t)a.N;
  auto seg_init = [&](int seg) {
    if (seg == 0) { la.init(a.A, a.lda, m0, a.M, k_beg, nullptr); lb.init(a.B, a.ldb, brow0, bmax, k_beg, rmap); }
    else { la.init(a.A2, a.lda2, m0, a.M, 0, nullptr); lb.init(a.B2, a.ldb2, brow0, bmax, 0, rmap); }
  };
  auto load_chunk = [&](int64_t c) {   // (chunks are loaded in order)
    if (c == nch1) seg_init(1);
    const bool s0 = c < nch1;
    const int64_t k0 = s0 ? k_beg + c * TK : (c - nch1) * TK;
    const int64_t ke = s0 ? k_end1 : a.K2;
    ma = la.load(k0, ke, ra);
    mb = lb.load(k0, ke, rb);
  };
  if (nch > 0) {
    if (nch1 > 0) seg_init(0);
    load_chunk(0);
    tile_store<RS>(As(0), ra, ma);
    tile_store<RS>(Bs(0), rb, mb);
  }
  __syncthreads();
  const int b_base = CELL ? wn * 16 : wn * 64;
  const int b_step = CELL ? HC : 16;
  for (int64_t c = 0; c < nch; ++c) {
    const int cur = (int)(c & 1);
    const bool more = c + 1 < nch;
    if (more) load_chunk(c + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {   // two 32-k MFMA blocks per chunk; lane (row, ag) supplies k = 32 kk + 8 ag .. + 7
      bf16x8 fb[4];
#pragma unroll
      for (int jn = 0; jn < 4; ++jn) fb[jn] = *(const bf16x8*)(Bs(cur) + (b_base + jn * b_step + arow) * LDB + kk * 32 + ag * 8);
#pragma unroll
      for (int ih = 0; ih < FI; ih += 4) {
        bf16x8 fa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = *(const bf16x8*)(As(cur) + (wm * (FI * 16) + (ih + i) * 16 + arow) * LDB + kk * 32 + ag * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jn = 0; jn < 4; ++jn)
            acc[ih + i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[jn], fa[i], acc[ih + i][jn], 0, 0, 0);
      }
    }
    if (more) {
      tile_store<RS>(As(cur ^ 1), ra, ma);
      tile_store<RS>(Bs(cur ^ 1), rb, mb);
    }
    __syncthreads();
  }
  if constexpr (EPI == EPI_STORE || EPI == EPI_ACCUM) {
    const bool vec = (EPI == EPI_STORE) && !(a.N & 3) && !(a.ldc & 3);
#pragma unroll
    for (int i = 0; i < FI; ++i) {
      const int64_t row = m0 + wm * (FI * 16) + i * 16 + arow;
      if (row >= a.M) continue;
#pragma unroll
      for (int jn = 0; jn < 4; ++jn) {
        const int col = n0 + wn * 64 + jn * 16 + ag * 4;
        if (col >= a.N) continue;
        float* dst = a.C + row * a.ldc + col;
        if (vec) {   // (N % 4 == 0: the four columns are all inside)
          f32x4 v = acc[i][jn];
          if (a.bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += a.bias[col + r];
          }
          *(f32x4*)dst = v;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (col + r >= a.N) continue;
            if (EPI == EPI_STORE) dst[r] = acc[i][jn][r] + (a.bias ? a.bias[col + r] : 0.f);
            else if (a.use_atomic) unsafeAtomicAdd(dst + r, acc[i][jn][r]);
            else dst[r] += acc[i][jn][r];
          }
        }
      }
    }
  } else {
    const int u = nt_idx * HC + wn * 16 + ag * 4;   // H % 8 == 0: u < H puts u .. u + 3 inside
    if (u < a.H) {
      f32x4 bq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) bq[q][r] = a.bias[q * a.H + u + r];   // (the flat parameter vector's offsets are not 16-byte aligned)
#pragma unroll
      for (int i = 0; i < FI; ++i) {
        const int64_t row = m0 + wm * (FI * 16) + i * 16 + arow;
        if (row >= a.M) continue;
        f32x4 cp = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a.cprev) cp = *(const f32x4*)(a.cprev + row * a.ldh + u);
        f32x4 cc, hh;
        bf16x4 gi, gg4, gf, go, hb;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ig = sigm_e2(acc[i][0][r] + bq[0][r]);
          const float gg = tanh_e2(acc[i][1][r] + bq[1][r]);
          const float fg = sigm_e2(acc[i][2][r] + bq[2][r]);
          const float og = sigm_e2(acc[i][3][r] + bq[3][r]);
          cc[r] = fg * cp[r] + ig * gg;
          hh[r] = og * tanh_e2(cc[r]);
          gi[r] = tobf(ig); gg4[r] = tobf(gg); gf[r] = tobf(fg); go[r] = tobf(og); hb[r] = tobf(hh[r]);
        }
        *(f32x4*)(a.cout + row * a.ldh + u) = cc;
        *(bf16x4*)(a.hout + row * a.ldh + u) = hb;
        if (a.hout_f32) *(f32x4*)(a.hout_f32 + row * a.ldh + u) = hh;
        if (a.act) {
          bf16* g = a.act + row * (int64_t)4 * a.H + u;
          *(bf16x4*)(g) = gi; *(bf16x4*)(g + a.H) = gg4; *(bf16x4*)(g + 2 * a.H) = gf; *(bf16x4*)(g + 3 * a.H) = go;
        }
      }
    }
  }
}

template <int EPI, int BIG>
static void launch16(hipStream_t s, GArgs a, int split_k) {
  const size_t lds_bytes = (size_t)4 * Geo<BIG>::TILE * sizeof(bf16);
  static PerDeviceOnce attr_done;
  if (attr_done.need()) {
    HIP_TRY(hipFuncSetAttribute((const void*)k_gemm16<EPI, BIG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  }
  a.nsplit = split_k;
  dim3 grid((unsigned)(((a.mtiles + 7) / 8) * 8 * a.ntiles));
  if (split_k > 1) grid = dim3((unsigned)(((split_k + 7) / 8) * 8 * a.mtiles * a.ntiles));
  hipLaunchKernelGGL((k_gemm16<EPI, BIG>), grid, dim3(Geo<BIG>::NT), lds_bytes, s, a);
  HIP_TRY(hipGetLastError());
}

// the 256-wide tile needs enough of them to fill the 256 CUs a few times over (one block per CU)
static bool big_tiles(int64_t M, int64_t N) {
  if (const char* e = getenv("KPRN_BF16_TILE")) {   // "big" | "small": the parity tests run both geometries at sizes the oracle handles
    if (e[0] == 'b') return true;
    if (e[0] == 's') return false;
  }
  return ((M + 255) / 256) * ((N + 255) / 256) >= 512;
}

// one FastLSTM step (forward() of lstm_bf16.hip): the 256-wide geometry where big_tiles says so; a column tile is Geo::HC hidden units x 4 gates
void lstm_step16(hipStream_t s, GArgs a) {
  a.kchunk = ((a.K + TK - 1) / TK) * TK;
  if (big_tiles(a.M, 4 * (int64_t)a.H)) {
    a.mtiles = (a.M + 255) / 256; a.ntiles = (a.H + 63) / 64;
    launch16<EPI_LSTM, 1>(s, a, 1);
  } else {
    a.mtiles = (a.M + 127) / 128; a.ntiles = (a.H + 31) / 32;
    launch16<EPI_LSTM, 0>(s, a, 1);
  }
}

// C[M][N] (fp32) = or += A[M][K] B[N][K]^T; K, lda, ldb multiples of 8 elements, 16-byte aligned pointers
void gemm16(hipStream_t s, Bf16GemmOpts o, const bf16* zero, const bf16* A, int64_t lda, const bf16* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int64_t K,
            bool accumulate, const float* bias, int split_k, Ran* ran) {
  if (!bias && gemm16x(s, o, zero, A, lda, B, ldb, C, ldc, M, N, K, accumulate, split_k, 0, 0, 1, ran)) return;   // the LDS-DMA kernel (large products without a bias)
  gemm16_plain(s, A, lda, B, ldb, C, ldc, M, N, K, accumulate, bias, split_k, ran);
}
// k_gemm16 alone: what gemm16 runs after gemm16x declines
void gemm16_plain(hipStream_t s, const bf16* A, int64_t lda, const bf16* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int64_t K,
                  bool accumulate, const float* bias, int split_k, Ran* ran) {
  GArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.K = K; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.bias = bias;
  if (split_k < 1 || !accumulate) split_k = 1;
  const bool big = split_k == 1 && big_tiles(M, N);
  const int tm = big ? 256 : 128;
  a.mtiles = (M + tm - 1) / tm; a.ntiles = (N + tm - 1) / tm;
  if (split_k > 1) {
    const int64_t tiles = a.mtiles * a.ntiles;
    split_k = (int)std::max<int64_t>(1, std::min<int64_t>(split_k, (3 * 256 + tiles - 1) / tiles));
  }
  int64_t kchunk = (K + split_k - 1) / split_k;
  kchunk = ((kchunk + TK - 1) / TK) * TK;
  split_k = (int)((K + kchunk - 1) / kchunk);
  a.kchunk = kchunk; a.use_atomic = split_k > 1 ? 1 : 0;
  if (ran) *ran = Ran{big ? KPRN_GEMM16_BIG : KPRN_GEMM16_SMALL, split_k, kchunk};
  if (big) { if (accumulate) launch16<EPI_ACCUM, 1>(s, a, 1); else launch16<EPI_STORE, 1>(s, a, 1); }
  else if (accumulate) launch16<EPI_ACCUM, 0>(s, a, split_k); else launch16<EPI_STORE, 0>(s, a, split_k);
}

// ---- the same product on 256 x 128 x 64 tiles with LDS-DMA operand staging (round 3) ------------------------------------------------------
// k_gemm16 above moves its operands global -> registers -> LDS (8 ds_write_b128 per thread and chunk) on 128 x 128 tiles and reaches 0.22 of the
// bf16 peak on the backward's products (dx, dh, split-K dW: 3.3 ms of configs[3]'s 8.6 ms step).  Here: 8 waves (4 x 2, 64 x 64 each on
// v_mfma_f32_32x32x16_bf16), three LDS stages of 48 KB filled by global_load_lds_dwordx4 two chunks ahead (counted vmcnt, one barrier per chunk,
// no staging registers, no ds_write), and a third fewer operand bytes per flop through the 64 B/clk L1 path, which is what bounds a 128 x 128 tile.
// LDS image: rows of 128 bytes (64 k); the DMA writes lane l at +16 l, i.e. 8 rows x 8 pieces per instruction, so the XOR swizzle that keeps
// ds_read_b128 of a 32-row fragment conflict-free is applied to the SOURCE piece (piece = slot ^ ((row >> 1) & 7)) and again to the read address.
namespace gx {
constexpr int BM = 256, BN = 128, BK = 64, NSTAGE = 3, NTHR = 512;
constexpr int STAGE_BYTES = (BM + BN) * BK * 2;
struct XArgs {
  const bf16* A; int64_t lda; const bf16* B; int64_t ldb; float* C; int64_t ldc; int64_t M; int N; int64_t K;
  int64_t kchunk; int nsplit; int64_t mtiles; int ntiles; const bf16* zero;   // zero: 16 zero bytes in global memory (source of every out-of-range piece)
  int touch;                // > 0: every wave touches the cache lines of the chunk `touch` chunks ahead (one dword per tile row: an L2 prefetch; k_gemm16x)
  int n_lo; int64_t k_lo;   // rows n >= n_lo of B are known to be ZERO for k < k_lo (the merged dW product's h_{t-1}^T block has no step -1): column tiles from n_lo on start at k_lo
};
__device__ __forceinline__ unsigned lds_off(const void* p) { return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p; }
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
typedef float f32x16 __attribute__((ext_vector_type(16)));

// DBG (measurement build only, KPRN_GEMM16_DBG): 1 no MFMAs, 2 no fragment reads either, 4 no DMA (the stages hold whatever they hold), 8 no epilogue,
// 16 the DMA pieces come from where a K-blocked layout [K / 64][rows][64] would hold them (tile rows 128 bytes apart instead of a row pitch apart; the same bytes,
// instructions and reuse between tiles: what the row-major layout costs in address translation / DRAM page locality), 32 every chunk re-reads the first 1 KB of
// its rows (everything an L2 hit: the delivery rate L2 -> LDS of this access shape, no HBM latency in it)
template <bool ACCUM, int DBG = 0>
__global__ __launch_bounds__(NTHR, 2) void k_gemm16x(XArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, kg = lane >> 5;
  const int64_t id = blockIdx.x;
  const int xcd = (int)(id & 7);
  const int64_t j = id >> 3;
  int nt_idx; int64_t mt_idx, split_idx = 0;
  if (a.nsplit > 1) {   // all tiles of one K range on one XCD
    const int64_t tiles = a.mtiles * a.ntiles;
    split_idx = (j / tiles) * 8 + xcd;
    const int64_t tl = j % tiles;
    mt_idx = tl / a.ntiles; nt_idx = (int)(tl % a.ntiles);
    if (split_idx >= a.nsplit) return;
  } else {              // the n-tiles of one m-tile back to back on one XCD: its A rows are fetched into that L2 once
    nt_idx = (int)(j % a.ntiles);
    mt_idx = (j / a.ntiles) * 8 + xcd;
    if (mt_idx >= a.mtiles) return;
  }
  const int64_t m0 = mt_idx * BM;
  const int n0 = nt_idx * BN;
  int64_t k_beg = split_idx * a.kchunk;
  const int64_t k_end = (k_beg + a.kchunk < a.K) ? k_beg + a.kchunk : a.K;
  if (a.k_lo > 0 && n0 >= a.n_lo && k_beg < a.k_lo) k_beg = a.k_lo;   // (k_lo is a multiple of 8: pieces stay 16-byte aligned)
  const int nch = (k_end > k_beg) ? (int)((k_end - k_beg + BK - 1) / BK) : 0;
  if (nch == 0) return;
  // this lane's share of a chunk's 48 DMA instructions (8 rows x 128 bytes each): instruction q = wave + 8 i covers tile rows 8 q .. 8 q + 7
  // (A: q < 32, B: q >= 32); the lane fetches piece (slot ^ key(row)) of row 8 q + (lane >> 3)
  const bf16* rowp[6]; int piece[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int q = wave + 8 * i;
    const bool isA = q < BM / 8;
    const int row = 8 * (isA ? q : q - BM / 8) + (lane >> 3);
    const int64_t gr = (isA ? m0 : (int64_t)n0) + row;
    const bool ok = gr < (isA ? a.M : (int64_t)a.N);
    rowp[i] = ok ? (isA ? a.A + gr * a.lda : a.B + gr * a.ldb) : nullptr;
    piece[i] = (lane & 7) ^ ((row >> 1) & 7);
  }
  const unsigned lds0 = lds_off(smem);
  auto issue = [&](int c) {
    const int64_t k0 = k_beg + (int64_t)c * BK;
    const unsigned st = lds0 + (unsigned)(c % NSTAGE) * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int64_t k = k0 + 8 * piece[i];
      const bf16* src = (rowp[i] && k < k_end) ? rowp[i] + k : a.zero;
      if constexpr ((DBG & 32) != 0) {   // every chunk from the first 1 KB of its row: 2 176 rows x 1 KB stay in every L2 -- the L2-hit delivery rate of this access shape
        if (rowp[i] && k < k_end) src = rowp[i] + (k & 511);
      }
      if constexpr ((DBG & 16) != 0) {   // the K-blocked layout [K / 64][rows][64], emulated inside the same allocations: the same reuse between tiles, rows 128 bytes apart
        if (rowp[i] && k < k_end) {
          const bool isA = (wave + 8 * i) < BM / 8;
          const int64_t gr = isA ? (rowp[i] - a.A) / a.lda : (rowp[i] - a.B) / a.ldb;
          src = (isA ? a.A + (k0 >> 6) * (a.M * 64) : a.B + (k0 >> 6) * ((int64_t)a.N * 64)) + gr * 64 + 8 * piece[i];
        }
      }
      dma16(src, (unsigned)__builtin_amdgcn_readfirstlane((int)(st + (unsigned)(wave + 8 * i) * 1024u)));
    }
  };
  // L2 prefetch by touch (round 5).  The knock-outs (scripts/gpu_gemm16_knockouts.py) show this launch bound by its operand staging, not by its MFMAs: DMA + waits +
  // barriers alone take 0.82 of the 1.06 ms, MFMAs + fragment reads alone 0.39 -- two 48 KB chunks in flight per CU against ~2 us of HBM latency is 20 B/clk per CU.
  // LDS cannot hold more stages; the L2 can hold the lines: a chunk row is exactly one 128-byte line, so ONE 4-byte load per tile row, `touch` chunks ahead, brings
  // the chunk into this XCD's L2 long before its DMA asks for it.  Thread L < 384 owns tile row L (A rows, then B rows); the loaded dword is never looked at and
  // must not land in a register (an asynchronous load into a VGPR that hipcc believes dead overwrites whatever it put there next -- the first build of this
  // faulted): it is a 4-byte LDS-DMA into a scratch strip behind the stages.  Issued unconditionally (a clamped address): the counted waits below allow for
  // exactly one more load per chunk in flight for waves 0-5.
  const int trow = wave * 64 + lane;
  const bf16* tptr = a.zero;
  if (a.touch > 0 && trow < BM + BN) {
    const bool isA = trow < BM;
    const int64_t gr = isA ? m0 + trow : (int64_t)n0 + (trow - BM);
    if (gr < (isA ? a.M : (int64_t)a.N)) tptr = (isA ? a.A + gr * a.lda : a.B + gr * a.ldb) + k_beg;
  }
  const bool toucher = a.touch > 0 && wave < (BM + BN) / 64;   // (wave-uniform)
  auto touch = [&](int c) {
    if (!toucher) return;
    const int64_t k = k_beg + (int64_t)c * BK;
    const bf16* p = (tptr != a.zero && k < k_end) ? tptr + (int64_t)c * BK : a.zero;
    unsigned keep;
    const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + (unsigned)NSTAGE * STAGE_BYTES + (unsigned)wave * 256u));
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(p), "s"(dst) : "memory");
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][jn][q] = 0.f;
  if (toucher) {   // the lines of the first chunks beyond the two requested below
    for (int c = 2; c < 2 + a.touch && c < nch; ++c) touch(c);
  }
  if (!(DBG & 4)) {
    issue(0);
    if (nch > 1) issue(1);
  }
  const int key = (r >> 1) & 7;
  const int arow = (wm * 64 + r) * 128, brow = BM * 128 + (wn * 64 + r) * 128;
  for (int c = 0; c < nch; ++c) {
    // chunk c has landed for this wave (its own 6 pieces; the 6 most recent ones belong to chunk c + 1 -- plus, for a touching wave, the one touch issued behind
    // them), then for every wave; and every wave has finished reading the stage chunk c + 2 is about to overwrite (it held chunk c - 1)
    if (c + 1 < nch) { if (toucher && c > 0) asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); }
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    touch(c + 2 + a.touch);   // (unconditional for a touching wave: a chunk past the range touches the zero block; BEFORE the DMA, so that exactly this one
                              //  touch and the next chunk's six pieces are younger than the pieces the next iteration waits for)
    if (c + 2 < nch && !(DBG & 4)) issue(c + 2);
    const char* st = smem + (c % NSTAGE) * STAGE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int po = ((2 * kk + kg) ^ key) << 4;
      bf16x8 fa[2], fb[2];
      if constexpr ((DBG & 2) != 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) { fa[i] = bf16x8{}; fb[i] = bf16x8{}; asm volatile("" : "+v"(fa[i]), "+v"(fb[i])); }
      } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *(const bf16x8*)(st + arow + i * 32 * 128 + po);
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) fb[jn] = *(const bf16x8*)(st + brow + jn * 32 * 128 + po);
      }
      if constexpr ((DBG & 1) != 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) asm volatile("" :: "v"(fa[i]), "v"(fb[i]));
      } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jn = 0; jn < 2; ++jn) acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[jn], acc[i][jn], 0, 0, 0);
      }
    }
  }
  if constexpr ((DBG & 8) != 0) {
    if (acc[0][0][0] == 123.456f) a.C[0] = acc[1][1][3];
    return;
  }
  // D[m][n]: lane (n = lane & 31, kg), register q <-> row (q & 3) + 8 (q >> 2) + 4 kg: 32 consecutive columns per store instruction
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) {
      const int n = n0 + wn * 64 + jn * 32 + r;
      if (n >= a.N) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t m = m0 + wm * 64 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * kg;
        if (m >= a.M) continue;
        float* dst = a.C + m * a.ldc + n;
        if (ACCUM) unsafeAtomicAdd(dst, acc[i][jn][q]); else *dst = acc[i][jn][q];
      }
    }
}

// ---- the same tiles with the A operand handed over K-MAJOR: C[m][n] = sum_k AT[k][m] B[n][k]  (round 4) ----------------------------------------------
// dx = dA W_i2g with dA as the persistent BPTT launch leaves it for the dW products anyway: TRANSPOSED, [gate column][step][path] (lstm_bf16_bwd_persist.hip).
// Reading it here saves that launch its second, row-major copy of dA (1.2 GB per step of configs[3], written in 16-byte pieces scattered over 64 rows per
// wave instruction: 0.46 ms of its 1.35).  The A stage is the k-major image itself: 64 k-rows of 256 paths (512 bytes), filled by the same LDS-DMA
// (one instruction = two k-rows), and the fragment of v_mfma_f32_32x32x16_bf16 -- lane (m, kg) holds A[m][8 kg .. + 7] -- is formed by two
// ds_read_b64_tr_b16 per lane: inside a 16-lane group, lane p points at 4 consecutive paths of k-row (p >> 2) and gets back the 4 k-rows of ITS path
// (probed: scripts/ubench/tr16_probe.hip).  Bank conflicts: the 32 lanes of a phase touch 4 k-rows x 64 bytes, and 512-byte rows put those on the
// same banks; the 64-byte unit a piece lands in is therefore XORed with (k & 3) -- on the SOURCE side (the DMA writes LDS linearly) and again in the
// read address.  Column m' of AT is (step, path) with Np >= N paths per step (pad columns): the epilogue maps it to row step N + path of C.
struct XTArgs {
  const bf16* AT; int64_t ldat; const bf16* B; int64_t ldb; float* C; int64_t ldc; int64_t Mp; int N; int64_t K;
  int64_t mtiles; int ntiles; int64_t Np, Nv; const bf16* zero;
};
__global__ __launch_bounds__(NTHR, 2) void k_gemm16xt(XTArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, kg = lane >> 5;
  const int64_t id = blockIdx.x;
  const int xcd = (int)(id & 7);
  const int64_t j = id >> 3;
  const int nt_idx = (int)(j % a.ntiles);              // the n-tiles of one m-tile back to back on one XCD: its A columns are fetched into that L2 once
  const int64_t mt_idx = (j / a.ntiles) * 8 + xcd;
  if (mt_idx >= a.mtiles) return;
  const int64_t m0 = mt_idx * BM;
  const int n0 = nt_idx * BN;
  const int nch = (int)((a.K + BK - 1) / BK);
  // this lane's share of a chunk's 48 DMA instructions.  A (q < 32): instruction q = k-rows 2 q, 2 q + 1; the lane fills physical slot lane & 31 of
  // k-row 2 q + (lane >> 5) with the piece (8 paths) whose 64-byte unit is (slot >> 2) ^ (k & 3).  B (q >= 32): 8 rows x 128 bytes, as k_gemm16x.
  const bf16* src0[6]; int64_t step[6]; int kofs[6]; bool isa[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int q = wave + 8 * i;
    isa[i] = q < 32;
    if (isa[i]) {
      const int krow = 2 * q + (lane >> 5), ps = lane & 31;
      const int ls = ((((ps >> 2) ^ (krow & 3))) << 2) | (ps & 3);
      const int64_t m = m0 + 8 * ls;
      kofs[i] = krow;
      src0[i] = (m < a.Mp) ? a.AT + (int64_t)krow * a.ldat + m : nullptr;
      step[i] = (int64_t)BK * a.ldat;
    } else {
      const int row = 8 * (q - 32) + (lane >> 3);
      const int piece = (lane & 7) ^ ((row >> 1) & 7);
      kofs[i] = 8 * piece;
      src0[i] = (n0 + row < a.N) ? a.B + (int64_t)(n0 + row) * a.ldb + 8 * piece : nullptr;
      step[i] = BK;
    }
  }
  const unsigned lds0 = lds_off(smem);
  auto issue = [&](int c) {
    const unsigned st = lds0 + (unsigned)(c % NSTAGE) * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const bf16* src = (src0[i] && (int64_t)c * BK + kofs[i] < a.K) ? src0[i] + (int64_t)c * step[i] : a.zero;
      dma16(src, (unsigned)__builtin_amdgcn_readfirstlane((int)(st + (unsigned)(wave + 8 * i) * 1024u)));
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][jn][q] = 0.f;
  issue(0);
  if (nch > 1) issue(1);
  // A fragment addresses: lane p of a 16-lane group -> k-row (p >> 2) of the read's four, paths mb + 4 (p & 3) .. + 3 of the wave's 32-row fragment i
  const int p16 = lane & 15, mb = r & 16;
  int aoff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ml = wm * 64 + i * 32 + mb + 4 * (p16 & 3);
    const int ls = ml >> 3, ps = ((((ls >> 2) ^ (p16 >> 2))) << 2) | (ls & 3);
    aoff[i] = (8 * kg + (p16 >> 2)) * 512 + ps * 16 + (ml & 7) * 2;
  }
  const int key = (r >> 1) & 7;
  const int brow = BM * 128 + (wn * 64 + r) * 128;
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (c + 2 < nch) issue(c + 2);
    const char* st = smem + (c % NSTAGE) * STAGE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int po = ((2 * kk + kg) ^ key) << 4;
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(st + aoff[i] + (16 * kk) * 512));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(st + aoff[i] + (16 * kk + 4) * 512));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        fa[i] = __builtin_bit_cast(bf16x8, both);
      }
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) fb[jn] = *(const bf16x8*)(st + brow + jn * 32 * 128 + po);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[jn], acc[i][jn], 0, 0, 0);
    }
  }
  const bool same = a.Np == a.Nv;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) {
      const int n = n0 + wn * 64 + jn * 32 + r;
      if (n >= a.N) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t mp = m0 + wm * 64 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * kg;
        if (mp >= a.Mp) continue;
        int64_t row = mp;
        if (!same) {   // pad columns between the steps (N not a multiple of 8): 32-bit arithmetic (host: Mp < 2^32)
          const unsigned tq = (unsigned)mp / (unsigned)a.Np, path = (unsigned)mp - tq * (unsigned)a.Np;
          if ((int64_t)path >= a.Nv) continue;
          row = (int64_t)tq * a.Nv + path;
        }
        a.C[row * a.ldc + n] = acc[i][jn][q];
      }
    }
}

// ---- the x tile with its operands staged through REGISTERS, four chunks in flight (round 5) --------------------------------------------------------------------------
// Knock-outs of k_gemm16x on the merged dW product (scripts/gpu_gemm16_knockouts.py, profiles/r05/gemm16_knockouts.txt): DMA + waits + barriers alone 0.82 of the
// 1.06 ms, MFMAs + fragment reads alone 0.39 -- the launch is bound by its operand staging, and that staging by LATENCY: two 48 KB chunks in flight per CU against
// ~2 us from HBM is 20 bytes per clock and CU, a third of what the L1 path carries.  LDS cannot hold more stages (3 x 48 KB).  Registers can: here every thread fetches
// its six 16-byte pieces of a chunk into VGPRs THREE chunks before it writes them to LDS (ds_write_b128, the same XOR swizzle applied to the write address), so four
// chunks = 192 KB per CU are in flight; LDS is a plain double buffer, one barrier per chunk.  No inline-asm loads: hipcc counts its own vmcnt exactly (the chunk loop
// is unrolled by the ring's period so that the ring is statically indexed), fences keep the loads where they are written.
constexpr int RRING = 4;   // chunk buffers per thread (3 ahead + the one being written)
template <bool ACCUM>
__global__ __launch_bounds__(NTHR, 2) void k_gemm16r(XArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, kg = lane >> 5;
  const int64_t id = blockIdx.x;
  const int xcd = (int)(id & 7);
  const int64_t j = id >> 3;
  int nt_idx; int64_t mt_idx, split_idx = 0;
  if (a.nsplit > 1) {
    const int64_t tiles = a.mtiles * a.ntiles;
    split_idx = (j / tiles) * 8 + xcd;
    const int64_t tl = j % tiles;
    mt_idx = tl / a.ntiles; nt_idx = (int)(tl % a.ntiles);
    if (split_idx >= a.nsplit) return;
  } else {
    nt_idx = (int)(j % a.ntiles);
    mt_idx = (j / a.ntiles) * 8 + xcd;
    if (mt_idx >= a.mtiles) return;
  }
  const int64_t m0 = mt_idx * BM;
  const int n0 = nt_idx * BN;
  int64_t k_beg = split_idx * a.kchunk;
  const int64_t k_end = (k_beg + a.kchunk < a.K) ? k_beg + a.kchunk : a.K;
  if (a.k_lo > 0 && n0 >= a.n_lo && k_beg < a.k_lo) k_beg = a.k_lo;
  const int nch = (k_end > k_beg) ? (int)((k_end - k_beg + BK - 1) / BK) : 0;
  if (nch == 0) return;
  // piece i of this thread: tile row 8 q + (lane >> 3) of instruction slot q = wave + 8 i (A: q < 32, B: q >= 32), 16-byte slot lane & 7 of the row's 128 bytes
  const bf16* src[6]; unsigned wofs[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int q = wave + 8 * i;
    const bool isA = q < BM / 8;
    const int row = 8 * (isA ? q : q - BM / 8) + (lane >> 3);
    const int64_t gr = (isA ? m0 : (int64_t)n0) + row;
    const bool ok = gr < (isA ? a.M : (int64_t)a.N);
    src[i] = ok ? (isA ? a.A + gr * a.lda : a.B + gr * a.ldb) + k_beg + 8 * (lane & 7) : nullptr;
    wofs[i] = (unsigned)((isA ? 0 : BM * 128) + row * 128 + (((lane & 7) ^ ((row >> 1) & 7)) << 4));
  }
  bf16x8 ring[RRING][6];
  auto fetch = [&](int c, bf16x8 (&dst)[6]) {   // chunk c of this thread's rows (pieces past the K range / the problem: the zero block)
    const int64_t kk0 = (int64_t)c * BK;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const bf16* p = (src[i] && c < nch && k_beg + kk0 + 8 * (lane & 7) < k_end) ? src[i] + kk0 : a.zero;
      dst[i] = *(const bf16x8*)p;
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto stash = [&](int stage, const bf16x8 (&v)[6]) {
    char* st = smem + stage * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < 6; ++i) *(bf16x8*)(st + wofs[i]) = v[i];
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][jn][q] = 0.f;
  const int key = (r >> 1) & 7;
  const int arow = (wm * 64 + r) * 128, brow = BM * 128 + (wn * 64 + r) * 128;
  auto product = [&](int stage) {
    const char* st = smem + stage * STAGE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int po = ((2 * kk + kg) ^ key) << 4;
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *(const bf16x8*)(st + arow + i * 32 * 128 + po);
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) fb[jn] = *(const bf16x8*)(st + brow + jn * 32 * 128 + po);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[jn], acc[i][jn], 0, 0, 0);
    }
  };
  // prologue: chunks 0 .. 3 requested, chunk 0 written to stage 0
  fetch(0, ring[0]); fetch(1, ring[1]); fetch(2, ring[2]); fetch(3, ring[3]);
  stash(0, ring[0]);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  // iteration c: chunk c + 4 is requested into the ring slot chunk c just left, chunk c + 1 goes from its registers to the other stage, chunk c is multiplied
  for (int c0 = 0; c0 < nch; c0 += RRING) {
#pragma unroll
    for (int u = 0; u < RRING; ++u) {
      const int c = c0 + u;
      if (c < nch) {   // (workgroup-uniform)
        fetch(c + RRING, ring[u]);
        stash((c + 1) & 1, ring[(u + 1) % RRING]);
        __builtin_amdgcn_sched_barrier(0);
        product(c & 1);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) {
      const int n = n0 + wn * 64 + jn * 32 + r;
      if (n >= a.N) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t m = m0 + wm * 64 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * kg;
        if (m >= a.M) continue;
        float* dst = a.C + m * a.ldc + n;
        if (ACCUM) unsafeAtomicAdd(dst, acc[i][jn][q]); else *dst = acc[i][jn][q];
      }
    }
}

// ---- 256 x 256 x 32 tiles, two wave groups one barrier apart (round 5) --------------------------------------------------------------------------------
// What k_gemm16x / k_gemm16y share is their lockstep: every wave meets the same barrier, then every wave reads its fragments, then every wave issues its MFMAs --
// the two waves of a SIMD wait for LDS at the same moment and want the matrix pipe at the same moment (0.28-0.36 of the bf16 peak whatever the tile).  Here the
// workgroup's eight waves form two groups, G0 = waves 0-3 (rows 0-127 of the tile) and G1 = waves 4-7 (rows 128-255): wave w and w + 4 share a SIMD.  A K tile of
// 32 is one READ segment (this wave's DMA requests three K tiles ahead, 12 ds_read_b128: 8 A + 4 B fragments of v_mfma_f32_32x32x16_bf16, the counted wait for its
// own pieces of the next K tile) and one MFMA segment (16 MFMAs = 512 matrix cycles on a 128 x 64 wave tile), each closed by s_barrier -- and G1 runs ONE BARRIER
// BEHIND G0, so on every SIMD one wave reads while the other multiplies:
//     barrier index       B0        B1          B2          B3          B4
//     G0            | R(0) | M(0)     | R(1)     | M(1)      | R(2) ...
//     G1            |  --  | R(0)     | M(0)     | R(1)      | M(1) ...
// Four LDS buffers of 32 KB (A 256 x 32 | B 256 x 32 bf16; rows of 64 bytes, the 16-byte piece a lane fetches chosen on the SOURCE side so that a 32-row fragment
// read is conflict-free: as k_gemm16y).  Hazards: K tile kt + 1 is complete for everybody before G0's R(kt + 1) -- every wave waits for its own pieces of kt + 1 at
// the end of its R(kt) (G0: interval 2 kt, G1: 2 kt + 1) and a barrier follows both; the buffer DMA(kt + 3) overwrites held K tile kt - 1, last read by G1's R(kt - 1) in
// interval 2 kt - 1, which ends with lgkmcnt(0) + barrier before G0 requests it in interval 2 kt.
constexpr int PBM = 256, PBN = 256, PBK = 32, PNBUF = 4, PBUF_BYTES = (PBM + PBN) * PBK * 2;
template <bool ACCUM>
__global__ __launch_bounds__(NTHR, 2) void k_gemm16p(XArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wg = wave >> 2, wc = wave & 3, r = lane & 31, kg = lane >> 5;
  const int64_t id = blockIdx.x;
  const int xcd = (int)(id & 7);
  const int64_t j = id >> 3;
  int nt_idx; int64_t mt_idx, split_idx = 0;
  if (a.nsplit > 1) {   // all tiles of one K range on one XCD
    const int64_t tiles = a.mtiles * a.ntiles;
    split_idx = (j / tiles) * 8 + xcd;
    const int64_t tl = j % tiles;
    mt_idx = tl / a.ntiles; nt_idx = (int)(tl % a.ntiles);
    if (split_idx >= a.nsplit) return;
  } else {
    nt_idx = (int)(j % a.ntiles);
    mt_idx = (j / a.ntiles) * 8 + xcd;
    if (mt_idx >= a.mtiles) return;
  }
  const int64_t m0 = mt_idx * PBM;
  const int n0 = nt_idx * PBN;
  int64_t k_beg = split_idx * a.kchunk;
  const int64_t k_end = (k_beg + a.kchunk < a.K) ? k_beg + a.kchunk : a.K;
  if (a.k_lo > 0 && n0 >= a.n_lo && k_beg < a.k_lo) k_beg = a.k_lo;
  const int nkt = (k_end > k_beg) ? (int)((k_end - k_beg + PBK - 1) / PBK) : 0;
  if (nkt == 0) return;   // (workgroup-uniform: no barrier has been executed)
  // this lane's share of a K tile's 32 DMA instructions: instruction q = wave + 8 i covers tile rows 16 q .. 16 q + 15 (A: q < 16, B: q >= 16), lane -> row
  // 16 q' + (lane >> 2), slot lane & 3, piece slot ^ ((row >> 1) & 3)
  const bf16* rowp[4]; int piece[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = wave + 8 * i;
    const bool isA = q < PBM / 16;
    const int row = 16 * (isA ? q : q - PBM / 16) + (lane >> 2);
    const int64_t gr = (isA ? m0 : (int64_t)n0) + row;
    const bool ok = gr < (isA ? a.M : (int64_t)a.N);
    rowp[i] = ok ? (isA ? a.A + gr * a.lda : a.B + gr * a.ldb) : nullptr;
    piece[i] = (lane & 3) ^ ((row >> 1) & 3);
  }
  const unsigned lds0 = lds_off(smem);
  auto issue = [&](int kt) {
    const int64_t k0 = k_beg + (int64_t)kt * PBK;
    const unsigned st = lds0 + (unsigned)(kt & (PNBUF - 1)) * PBUF_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t k = k0 + 8 * piece[i];
      const bf16* src = (rowp[i] && k < k_end) ? rowp[i] + k : a.zero;
      dma16(src, (unsigned)__builtin_amdgcn_readfirstlane((int)(st + (unsigned)(wave + 8 * i) * 1024u)));
    }
  };
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][jn][q] = 0.f;
  const int key = (r >> 1) & 3;
  const int arow = (wg * 128 + r) * 64, brow = PBM * 64 + (wc * 64 + r) * 64;
  int po[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) po[s] = ((2 * s + kg) ^ key) << 4;
  // prologue: three K tiles requested, the first one complete for everybody
  issue(0);
  if (nkt > 1) issue(1);
  if (nkt > 2) issue(2);
  {
    const int behind = (nkt - 1) < 2 ? (nkt - 1) : 2;
    if (behind == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else if (behind == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B0
  if (wg == 1) asm volatile("s_barrier" ::: "memory");               // G1 falls one barrier behind
  for (int kt = 0; kt < nkt; ++kt) {
    // ---- READ segment
    if (kt + 3 < nkt) issue(kt + 3);
    const char* st = smem + (kt & (PNBUF - 1)) * PBUF_BYTES;
    bf16x8 fa[4][2], fb[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) fb[jn][s] = *(const bf16x8*)(st + brow + jn * 32 * 64 + po[s]);
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i][s] = *(const bf16x8*)(st + arow + i * 32 * 64 + po[s]);
    }
    {   // this wave's pieces of K tile kt + 1 have landed (the pieces of kt + 2, kt + 3 may still be in flight)
      const int last = nkt - 1;
      const int issued = (kt + 3 < last) ? kt + 3 : last;
      const int behind = issued - (kt + 1);
      if (behind >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else if (behind == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // ---- MFMA segment (the partner wave on this SIMD is in its READ segment)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][s], fb[jn][s], acc[i][jn], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_barrier" ::: "memory");
  }
  if (wg == 0) asm volatile("s_barrier" ::: "memory");   // G0 meets G1's last barrier
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) {
      const int n = n0 + wc * 64 + jn * 32 + r;
      if (n >= a.N) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t m = m0 + wg * 128 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * kg;
        if (m >= a.M) continue;
        float* dst = a.C + m * a.ldc + n;
        if (ACCUM) unsafeAtomicAdd(dst, acc[i][jn][q]); else *dst = acc[i][jn][q];
      }
    }
}
}  // namespace gx

// one kernel of the gx family: its tile and the dynamic LDS it is launched with
struct XKernel { void (*fn)(gx::XArgs); int bm, bn, bk; size_t lds_bytes; };

bool gemm16x(hipStream_t s, Bf16GemmOpts o, const bf16* zero, const bf16* A, int64_t lda, const bf16* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int64_t K,
             bool accumulate, int split_k, int n_lo, int64_t k_lo, int sx_min, Ran* ran) {
  if (ran) *ran = Ran{};
  static const bool off = KPRN_DEV_ENV("KPRN_BF16_GEMM") && KPRN_DEV_ENV("KPRN_BF16_GEMM")[0] == 'o';   // "old": k_gemm16 everywhere (A/B measurements, tests)
  if (off || M < gx::BM || N < gx::BN || (K & 7) || (lda & 7) || (ldb & 7)) return false;
  gx::XArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.zero = zero;
  a.n_lo = n_lo; a.k_lo = k_lo;
  a.touch = o.touch;
  if (split_k < 1 || !accumulate) split_k = 1;
  // THE choice of the kernel: x, the lockstep LDS-DMA kernel (three stages + the touch scratch), unless a split-K product (accumulate, more than one K range
  // asked for) has one of the two switches set.  "bf16_gemm_pingpong": p, the two-group kernel, where the output holds whole 256 x 256 tiles' worth of rows and
  // at least one tile of columns (configs[3]'s merged dW: 1 536 x 640 = 6 x 3 tiles, the last one half empty).  "bf16_gemm_regstage": r, the x tile staged through
  // registers on a plain LDS double buffer, where the planner below leaves more than one range -- it asks for s >= 8, and ceil(K / s) rounded up to BK is below
  // K exactly when K > BK.
  constexpr size_t x_lds = (size_t)gx::NSTAGE * gx::STAGE_BYTES + 2048 /* touch scratch */;
  const XKernel xs = {gx::k_gemm16x<false>, gx::BM, gx::BN, gx::BK, x_lds}, xa = {gx::k_gemm16x<true>, gx::BM, gx::BN, gx::BK, x_lds};
  const XKernel r = {gx::k_gemm16r<true>, gx::BM, gx::BN, gx::BK, (size_t)2 * gx::STAGE_BYTES}, p = {gx::k_gemm16p<true>, gx::PBM, gx::PBN, gx::PBK, (size_t)gx::PNBUF * gx::PBUF_BYTES};
  const bool split = accumulate && split_k > 1;
  XKernel k = !accumulate ? xs : (split && o.pingpong && M >= gx::PBM && N >= gx::PBN) ? p : (split && o.regstage && K > gx::BK) ? r : xa;
  const int bk = k.bk;
  a.mtiles = (M + k.bm - 1) / k.bm; a.ntiles = (N + k.bn - 1) / k.bn;
  if (split_k > 1) {
    // K ranges are dealt to the XCDs (range r on XCD r % 8, all its tiles there), one workgroup per CU (147 KB of LDS), 32 CUs per XCD:
    // with s ranges per XCD the launch takes ceil(tiles s / 32) rounds of 1 / (8 s) of K each.  Pick the s <= 8 with the least
    // rounds / s (configs[3]'s dW: 18 tiles -> s = 7: 126 workgroups = 3.94 rounds per XCD; the old "3 x 256 workgroups" rule gave 43
    // ranges = 6 on three XCDs, 4 rounds of 1 / 43: a quarter more time)
    const int64_t tiles = a.mtiles * a.ntiles;
    static const int s_env = KPRN_DEV_ENV("KPRN_GEMM16_SX") ? atoi(KPRN_DEV_ENV("KPRN_GEMM16_SX")) : 0;   // (measurement)
    int best = 1;
    double best_t = 1e30;
    for (int sx = std::max(1, std::min(sx_min, 8)); sx <= 8 && sx * 8 <= std::max(split_k, 8); ++sx) {
      const double t = (double)((tiles * sx + 31) / 32) / sx;
      if (t < best_t - 1e-9) { best_t = t; best = sx; }
    }
    if (s_env > 0) best = s_env;
    split_k = best * 8;
  }
  int64_t kchunk = (K + split_k - 1) / split_k;
  kchunk = ((kchunk + bk - 1) / bk) * bk;
  split_k = (int)((K + kchunk - 1) / kchunk);
  a.kchunk = kchunk; a.nsplit = split_k;
  if (ran) *ran = Ran{k.fn == p.fn ? KPRN_GEMM16_P : k.fn == r.fn ? KPRN_GEMM16_R : KPRN_GEMM16_X, split_k, kchunk};
  static PerDeviceOnce attr_done;
  if (attr_done.need()) {
    for (const XKernel& v : {xs, xa, r, p}) HIP_TRY(hipFuncSetAttribute((const void*)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds_bytes));
  }
#ifdef KPRN_PERSIST_VARIANTS
  // measurement build (scripts/gpu_gemm16_knockouts.py): KPRN_GEMM16_DBG = knock-out mask of the accumulating x launch
  if (const char* e = KPRN_DEV_ENV("KPRN_GEMM16_DBG"); e && k.fn == xa.fn) {
#define KV(D) case D: k.fn = gx::k_gemm16x<true, D>; break;
    switch (atoi(e)) { KV(0) KV(1) KV(3) KV(4) KV(5) KV(7) KV(8) KV(9) KV(12) KV(16) KV(19) KV(32) KV(35) default: KPRN_REQUIRE(false, KPRN_E_ARG, "this knock-out of k_gemm16x is not compiled in"); }
#undef KV
    HIP_TRY(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds_bytes));
  }
#endif
  dim3 grid((unsigned)(((a.mtiles + 7) / 8) * 8 * a.ntiles));
  if (split_k > 1) grid = dim3((unsigned)(((split_k + 7) / 8) * 8 * a.mtiles * a.ntiles));
  hipLaunchKernelGGL(k.fn, grid, dim3(gx::NTHR), k.lds_bytes, s, a);
  HIP_TRY(hipGetLastError());
  return true;
}

// C[(step, path)][N] (fp32) = sum_k AT[k][step Np + path] B[n][k]: the k-major A operand (gx::k_gemm16xt); false = shape not covered
static bool dx_t_off() {   // KPRN_BF16_DX_T=0: dx from a row-major dA (tests/test_gpu_persist.py A/B)
  static const bool off = [] { const char* e = getenv("KPRN_BF16_DX_T"); return e && e[0] == '0'; }();
  return off;
}
// the ONE predicate of the k-major-A product: what gemm16xt takes is what dx_from_transposed_ok promises the BPTT launch
static bool xt_shape_ok(int64_t Mp, int N, int64_t K, int64_t Np, int64_t ldat, int64_t ldb) {
  return !dx_t_off() && Mp >= gx::BM && Mp < ((int64_t)1 << 32) && N >= gx::BN && !(K & 7) && !(ldat & 7) && !(ldb & 7) && !(Np & 7);
}
bool gemm16xt(hipStream_t s, const bf16* zero, const bf16* AT, int64_t ldat, const bf16* B, int64_t ldb, float* C, int64_t ldc, int64_t Mp, int N, int64_t K, int64_t Np, int64_t Nv,
              Ran* ran) {
  if (ran) *ran = Ran{};
  if (!xt_shape_ok(Mp, N, K, Np, ldat, ldb)) return false;
  if (ran) *ran = Ran{KPRN_GEMM16_XT, 1, ((K + gx::BK - 1) / gx::BK) * gx::BK};
  gx::XTArgs a;
  memset(&a, 0, sizeof(a));
  a.AT = AT; a.ldat = ldat; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc; a.Mp = Mp; a.N = N; a.K = K; a.Np = Np; a.Nv = Nv; a.zero = zero;
  a.mtiles = (Mp + gx::BM - 1) / gx::BM; a.ntiles = (N + gx::BN - 1) / gx::BN;
  const size_t lds_bytes = (size_t)gx::NSTAGE * gx::STAGE_BYTES;
  static PerDeviceOnce attr_done;
  if (attr_done.need()) {
    HIP_TRY(hipFuncSetAttribute((const void*)gx::k_gemm16xt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  }
  hipLaunchKernelGGL(gx::k_gemm16xt, dim3((unsigned)(((a.mtiles + 7) / 8) * 8 * a.ntiles)), dim3(gx::NTHR), lds_bytes, s, a);
  HIP_TRY(hipGetLastError());
  return true;
}
bool dx_from_transposed_ok(int64_t Mp, int N, int64_t K, int64_t Np) {   // (the BPTT launch asks before it drops its row-major copy of dA)
  return xt_shape_ok(Mp, N, K, Np, /*ldat = the padded (step, path) extent*/ Mp, /*ldb = the gate columns*/ K);
}

// measurement hook (kprn_debug_gemm what = 5 / 6): C[M][N] = A[M][K] B[N][K]^T on random bf16 operands, under h's switches; split_k > 1: the split-K accumulate form
float debug_gemm16(kprn_handle* h, int64_t M, int N, int64_t K, int split_k, int iters) {
  hipStream_t strm = h->stream;
  float* f = dalloc<float>(std::max<int64_t>(M * K, (int64_t)N * K));
  bf16 *A = dalloc<bf16>(M * K), *B = dalloc<bf16>((int64_t)N * K), *Z = dalloc<bf16>(128);   // Z: the zero block of these launches
  float* C = dalloc<float>(M * N);
  kk::fill_uniform(strm, f, M * K, 0.1f, 1, 0);
  cvt16(strm, f, A, M * K);
  kk::fill_uniform(strm, f, (int64_t)N * K, 0.1f, 2, 0);
  cvt16(strm, f, B, (int64_t)N * K);
  hipMemsetAsync(Z, 0, 256, strm);
  hipMemsetAsync(C, 0, (size_t)(M * N) * sizeof(float), strm);
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int it = -2; it < iters; ++it) {
    if (it == 0) hipEventRecord(e0, strm);
    gemm16(strm, h->bf16_gemm, Z, A, K, B, K, C, N, M, N, K, split_k > 1, nullptr, split_k);
  }
  hipEventRecord(e1, strm);
  hipEventSynchronize(e1);
  float t = 0.f;
  hipEventElapsedTime(&t, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  hipFree(f); hipFree(A); hipFree(B); hipFree(C); hipFree(Z);
  return t / (float)iters;
}

// test hook (kprn_debug_gemm16_run, include/kprn.h): one launch of one route on the caller's data.  Everything the products' contracts exclude is refused
// here, before anything is allocated; which kernel ran and on what K ranges is what the launcher itself reports (Ran).
void debug_gemm16_run(kprn_handle* h, const kprn_gemm16_call& c, const float* A, const float* B, const float* bias, float* C, kprn_gemm16_ran* ran) {
  KPRN_REQUIRE(A && B && C && ran, KPRN_E_ARG, "gemm16_run: NULL argument");
  const bool xt = c.route == 2;
  const int64_t lim = (int64_t)1 << 31, big = (int64_t)1 << 40;
  KPRN_REQUIRE(c.route >= 0 && c.route <= 3, KPRN_E_ARG, "gemm16_run: route must be 0..3");
  KPRN_REQUIRE(c.M >= 1 && c.N >= 1 && c.K >= 1 && c.M < lim && c.K < lim, KPRN_E_ARG, "gemm16_run: M, N, K must be in 1 .. 2^31 - 1");
  KPRN_REQUIRE(c.lda >= 1 && c.ldb >= 1 && c.ldc >= 1 && c.lda < lim && c.ldb < lim && c.ldc < lim, KPRN_E_ARG, "gemm16_run: a pitch must be in 1 .. 2^31 - 1");
  KPRN_REQUIRE(c.a_off >= 0 && c.b_off >= 0 && c.c_off >= 0 && c.a_count >= 1 && c.b_count >= 1 && c.c_count >= 1 && c.a_count < big && c.b_count < big && c.c_count < big,
               KPRN_E_ARG, "gemm16_run: an array's element count or a window's origin is out of range");
  KPRN_REQUIRE(!(c.K & 7) && !(c.lda & 7) && !(c.ldb & 7), KPRN_E_ARG, "gemm16_run: K, lda and ldb must be multiples of 8");
  KPRN_REQUIRE(!(c.a_off & 7) && !(c.b_off & 7) && !(c.c_off & 3), KPRN_E_ARG, "gemm16_run: a_off, b_off must be multiples of 8 and c_off of 4 (16-byte aligned operands)");
  KPRN_REQUIRE(c.k_lo >= 0 && !(c.k_lo & 7) && c.n_lo >= 0 && c.split_k >= 0 && c.sx_min >= 0, KPRN_E_ARG, "gemm16_run: k_lo must be a multiple of 8; n_lo, split_k, sx_min >= 0");
  KPRN_REQUIRE(!(bias && (c.accumulate || c.route == 1 || xt)), KPRN_E_ARG, "gemm16_run: a bias goes with the storing form of routes 0 and 3 only");
  int64_t c_rows = c.M;
  if (xt) {
    KPRN_REQUIRE(!c.accumulate, KPRN_E_ARG, "gemm16_run: the k-major-A product has no accumulating form");
    KPRN_REQUIRE(c.Np >= 8 && !(c.Np & 7) && c.Nv >= 1 && c.Nv <= c.Np && c.M % c.Np == 0, KPRN_E_ARG, "gemm16_run: Np must be a multiple of 8, 1 <= Nv <= Np, M a multiple of Np");
    KPRN_REQUIRE(c.lda >= c.M && c.a_off + (c.K - 1) * c.lda + c.M <= c.a_count, KPRN_E_ARG, "gemm16_run: the AT window does not fit its array");
    c_rows = (c.M / c.Np) * c.Nv;
  } else {
    KPRN_REQUIRE(c.lda >= c.K && c.a_off + (c.M - 1) * c.lda + c.K <= c.a_count, KPRN_E_ARG, "gemm16_run: the A window does not fit its array");
  }
  KPRN_REQUIRE(c.ldb >= c.K && c.b_off + (int64_t)(c.N - 1) * c.ldb + c.K <= c.b_count, KPRN_E_ARG, "gemm16_run: the B window does not fit its array");
  KPRN_REQUIRE(c.ldc >= c.N && c.c_off + (c_rows - 1) * c.ldc + c.N <= c.c_count, KPRN_E_ARG, "gemm16_run: the C window does not fit its array");
  struct Dev {   // (freed on every way out)
    float *f = nullptr, *C = nullptr, *bias = nullptr; bf16 *A = nullptr, *B = nullptr, *Z = nullptr;
    ~Dev() { hipFree(f); hipFree(C); hipFree(bias); hipFree(A); hipFree(B); hipFree(Z); }
  } d;
  hipStream_t strm = h->stream;
  d.f = dalloc<float>(std::max(c.a_count, c.b_count));
  d.A = dalloc<bf16>(c.a_count); d.B = dalloc<bf16>(c.b_count); d.Z = dalloc<bf16>(128);   // Z: the zero block of this launch
  d.C = dalloc<float>(c.c_count);
  HIP_TRY(hipMemcpyAsync(d.f, A, (size_t)c.a_count * sizeof(float), hipMemcpyHostToDevice, strm));
  cvt16(strm, d.f, d.A, c.a_count);
  HIP_TRY(hipStreamSynchronize(strm));   // (pageable host memory: the staging block is free again)
  HIP_TRY(hipMemcpyAsync(d.f, B, (size_t)c.b_count * sizeof(float), hipMemcpyHostToDevice, strm));
  cvt16(strm, d.f, d.B, c.b_count);
  HIP_TRY(hipMemsetAsync(d.Z, 0, 256, strm));
  HIP_TRY(hipMemcpyAsync(d.C, C, (size_t)c.c_count * sizeof(float), hipMemcpyHostToDevice, strm));
  if (bias) {
    d.bias = dalloc<float>(c.N);
    HIP_TRY(hipMemcpyAsync(d.bias, bias, (size_t)c.N * sizeof(float), hipMemcpyHostToDevice, strm));
  }
  const bf16 *a = d.A + c.a_off, *b = d.B + c.b_off;
  float* cw = d.C + c.c_off;
  Ran r;
  memset(ran, 0, sizeof(*ran));
  if (c.route == 0) gemm16(strm, h->bf16_gemm, d.Z, a, c.lda, b, c.ldb, cw, c.ldc, c.M, c.N, c.K, c.accumulate != 0, d.bias, c.split_k, &r);
  else if (c.route == 1) gemm16x(strm, h->bf16_gemm, d.Z, a, c.lda, b, c.ldb, cw, c.ldc, c.M, c.N, c.K, c.accumulate != 0, c.split_k, c.n_lo, c.k_lo, c.sx_min, &r);
  else if (xt) {
    gemm16xt(strm, d.Z, a, c.lda, b, c.ldb, cw, c.ldc, c.M, c.N, c.K, c.Np, c.Nv, &r);
    ran->dx_t_ok = dx_from_transposed_ok(c.M, c.N, c.K, c.Np) ? 1 : 0;
  } else gemm16_plain(strm, a, c.lda, b, c.ldb, cw, c.ldc, c.M, c.N, c.K, c.accumulate != 0, d.bias, c.split_k, &r);
  ran->kernel = r.kernel; ran->nsplit = r.nsplit; ran->kchunk = r.kchunk;
  HIP_TRY(hipMemcpyAsync(C, d.C, (size_t)c.c_count * sizeof(float), hipMemcpyDeviceToHost, strm));
  HIP_TRY(hipStreamSynchronize(strm));
}

}  // namespace bf16p
