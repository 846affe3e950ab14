// bf16 pipeline of the FastLSTM path (BASELINE.json configs[3]: 20 M entities, d = 128 -> D = H = 384, "bf16 MFMA LSTM"): bf16 STORAGE
// of everything the matrix cores read -- a bf16 shadow of the embedding tables and of the weights, bf16 step inputs, hidden states,
// gate values and pre-activation gradients -- products on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, fp32 cell state, fp32 master
// parameters and fp32 lazy-exact Adam (kprn_api.hip), which refreshes the shadow rows it touches.  gfx950 only.
//
// Stands for the same reference graph as gemm_tiled.hip (nn.LookupTable x 3 -> nn.Sequencer(nn.FastLSTM) x L -> nn.Linear:
// release/songPathRnn/net/FeatureEmbedding.lua:112-121, model/OneModel.lua:236,268-275) at reduced precision; tolerance-gated against the
// float64 oracle (tests/test_gpu_parity.py, tests/test_gpu_wide.py).
//
// In this file: the element-wise and layout kernels (conversions, the embedding gather, the transposes that bring everything the backward needs
// transposed -- dW = dA^T [x | h]: the contraction runs over the path rows -- into the products' one k-contiguous layout), the gate backward, the
// small-table kernels, the head, the handle's State (shadows, planes, the products' zero block) and forward / backward, which queue the launches.
// The products themselves, the step kernel with the cell epilogue among them, are gemm_bf16.hip; the persistent layer and BPTT launches
// lstm_bf16_persist.hip and lstm_bf16_bwd_persist.hip.
#include <string.h>

#include <algorithm>

#include "gate_math.h"
#include "gemm_bf16.h"

namespace bf16p {

// ---- element-wise / layout kernels --------------------------------------------------------------------------------------
__global__ void k_cvt(const float* __restrict__ x, bf16* __restrict__ y, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < n) {
    const f32x4 v = *(const f32x4*)(x + i);
    bf16x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = tobf(v[q]);
    *(bf16x4*)(y + i) = o;
  } else {
    for (int64_t k = i; k < n; ++k) y[k] = tobf(x[k]);
  }
}
void cvt16(hipStream_t s, const float* x, bf16* y, int64_t n) {
  hipLaunchKernelGGL(k_cvt, dim3((unsigned)((n / 4 + 256) / 256)), dim3(256), 0, s, x, y, n);
}
// y[c][r] = bf16(x[r][c]), x fp32 [R][C] (weights: small)
__global__ void k_cvt_T(const float* __restrict__ x, bf16* __restrict__ y, int R, int Cc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)R * Cc) return;
  const int c = (int)(i / R), r = (int)(i - (int64_t)c * R);
  y[i] = tobf(x[(int64_t)r * Cc + c]);
}
// shadow rows of the entity table after a row update: rows[0 .. *count)
__global__ void k_rows_cvt(const float* __restrict__ W, bf16* __restrict__ W16, const int32_t* __restrict__ rows, const int32_t* __restrict__ count,
                           int d) {
  const int n = *count;
  const int per = d >> 2;  // float4 pieces per row
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)n * per; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = rows[i / per];
    const int c = (int)(i % per) * 4;
    const f32x4 v = *(const f32x4*)(W + r * d + c);
    bf16x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = tobf(v[q]);
    *(bf16x4*)(W16 + r * d + c) = o;
  }
}
// FeatureEmbedding (net/FeatureEmbedding.lua:112-121) on the bf16 shadows: X16[t][n][:] = [ sum_k Wt[type_k] | We[ent] | Wr[rel] ], 8 columns
// per thread; ids are int32 (never through a float: 20 M entities exceed 2^24).  Several type slots: summed in fp32, rounded once.
__global__ void k_gather16(const int32_t* __restrict__ idx, int64_t N, int T, int F, int nT, const bf16* __restrict__ Wt, const bf16* __restrict__ We,
                           const bf16* __restrict__ Wr, int dt, int de, int dr, bf16* __restrict__ X) {
  const int D = dt + de + dr, DV = D >> 3;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= N * T * DV) return;
  const int cv = (int)(gid % DV);
  const int64_t nt = gid / DV;
  const int64_t n = nt / T;
  const int t = (int)(nt - n * T);
  const int32_t* f = idx + nt * F;
  const int col = cv * 8;
  bf16x8 v;
  if (col < dt) {
    v = *(const bf16x8*)(Wt + (int64_t)(f[F - nT - 2] - 1) * dt + col);
    if (nT > 1) {
      float acc[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = (float)v[q];
      for (int k = 1; k < nT; ++k) {
        const bf16x8 w = *(const bf16x8*)(Wt + (int64_t)(f[F - nT - 2 + k] - 1) * dt + col);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += (float)w[q];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = tobf(acc[q]);
    }
  } else if (col < dt + de) {
    v = *(const bf16x8*)(We + (int64_t)(f[F - 2] - 1) * de + (col - dt));
  } else {
    v = *(const bf16x8*)(Wr + (int64_t)(f[F - 1] - 1) * dr + (col - dt - de));
  }
  *(bf16x8*)(X + ((int64_t)t * N + n) * D + col) = v;
}
// The same gather written TRANSPOSED: XT[d][t][n] (pitch ldy = T Np, pad columns n >= N zero) -- the k-contiguous operand of the dW product.
// When the persistent layer kernel ran the training forward (it gathers for itself) the row-major plane X16 has no other reader, so the
// backward builds the transposed image straight from the shadow tables: 64 positions x 64 columns per workgroup through LDS, 16-byte accesses
// on both sides (k_gather16 + k_transpose16 of X: 0.13 + 0.16 ms on configs[3]).
__global__ __launch_bounds__(256) void k_gather16_T(const int32_t* __restrict__ idx, int64_t N, int64_t Np, int T, int F, int nT, const bf16* __restrict__ Wt,
                                                    const bf16* __restrict__ We, const bf16* __restrict__ Wr, int dt, int de, int dr, bf16* __restrict__ XT,
                                                    int64_t ldy) {
  __shared__ __attribute__((aligned(16))) bf16 tl[64][72];
  const int D = dt + de + dr;
  const int64_t n0 = (int64_t)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64, t = blockIdx.z;
  // Both of a thread's pieces: ids first, then rows, every load unconditional from a clamped address and masked afterwards (written as
  // `if (in range) load`, hipcc keeps the wait inside the branch: four dependent round trips per thread instead of two).
  const bf16* src[2]; const int32_t* idp[2]; bool ok[2], summed[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int f = threadIdx.x + 256 * e;
    const int rr = f >> 3, col = c0 + (f & 7) * 8;
    const int64_t n = n0 + rr;
    ok[e] = n < N && col < D;
    const int cl = col < D ? col : 0;
    const int32_t* id = idx + ((n < N ? n : N - 1) * T + t) * F;
    const int which = cl < dt ? 0 : (cl < dt + de ? 1 : 2);
    idp[e] = id;
    summed[e] = which == 0 && nT > 1;
    const int row = id[which == 0 ? F - nT - 2 : (which == 1 ? F - 2 : F - 1)] - 1;
    src[e] = which == 0 ? Wt + (int64_t)row * dt + cl : (which == 1 ? We + (int64_t)row * de + (cl - dt) : Wr + (int64_t)row * dr + (cl - dt - de));
  }
  bf16x8 ld[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) ld[e] = *(const bf16x8*)src[e];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int f = threadIdx.x + 256 * e;
    const int rr = f >> 3, col = c0 + (f & 7) * 8;
    bf16x8 v = ld[e];
    if (summed[e] && ok[e]) {   // several type slots per step: their rows summed (FeatureEmbedding.lua:55)
      float acc[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = (float)v[q];
      for (int k = 1; k < nT; ++k) {
        const bf16x8 w = *(const bf16x8*)(Wt + (int64_t)(idp[e][F - nT - 2 + k] - 1) * dt + col);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += (float)w[q];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = tobf(acc[q]);
    }
    if (!ok[e]) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = (bf16)0.f;
    }
    *(bf16x8*)(&tl[rr][(f & 7) * 8]) = v;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int f = threadIdx.x + 256 * e;
    const int cc = f >> 3, rq = (f & 7) * 8;
    if (c0 + cc < D && n0 + rq < Np) {
      bf16x8 v;
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = tl[rq + q][cc];
      *(bf16x8*)(XT + (int64_t)(c0 + cc) * ldy + (int64_t)t * Np + n0 + rq) = v;
    }
  }
}
// cell backward of one step on the saved bf16 gate values (kernels_basic.hip k_gates_bwd, with dA written in bf16)
__global__ void k_gates_bwd16(const bf16* __restrict__ act, const float* __restrict__ c, const float* __restrict__ c_prev, const float* __restrict__ dH_up,
                              float* __restrict__ dH, float* __restrict__ dC, bf16* __restrict__ dA, int64_t N, int H) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= N * H) return;
  const int jx = (int)(gid % H);
  const int64_t n = gid / H;
  const bf16* a = act + n * 4 * H;
  const float ig = (float)a[jx], gg = (float)a[H + jx], fg = (float)a[2 * H + jx], og = (float)a[3 * H + jx];
  const float tc = tanhf(c[gid]);
  const float dh = dH[gid] + (dH_up ? dH_up[gid] : 0.f);
  const float dO = dh * tc;
  const float dc = dC[gid] + dh * og * (1.f - tc * tc);
  const float cp = c_prev ? c_prev[gid] : 0.f;
  bf16* d = dA + n * 4 * H;
  d[jx] = tobf(dc * gg * ig * (1.f - ig));
  d[H + jx] = tobf(dc * ig * (1.f - gg * gg));
  d[2 * H + jx] = tobf(dc * cp * fg * (1.f - fg));
  d[3 * H + jx] = tobf(dO * og * (1.f - og));
  dC[gid] = dc * fg;
  dH[gid] = 0.f;
}
// The same cell backward on the persistent layer kernel's FRAGMENT-order saves (lstm_bf16_persist.hip Cell::store): record ((unit NCH + chunk) NW + wave) 64 +
// lane holds, for path 32 unit + (lane & 31) and hidden units HC chunk + 8 wave + 4 (lane >> 5) .. + 3, c (4 bf16: a copy of the fp32 cell state the recurrence itself runs on) and the gates as [i4 g4] / [f4 o4].
// One workgroup = one (unit, chunk): 32 rows x HC hidden units.  The records are read coalesced; everything row-major (dH, dC in / out, dA out) goes
// through LDS tiles so that global accesses are whole 128 / 256-byte row segments.
template <int NW>
__global__ __launch_bounds__(256) void k_gates_bwd16_frag(const bf16x8* __restrict__ A0, const bf16x8* __restrict__ A1, const bf16x4* __restrict__ cF,
                                                          const bf16x4* __restrict__ cprevF, const float* __restrict__ dH_up, const float* __restrict__ dH,
                                                          float* __restrict__ dC, bf16* __restrict__ dA, int64_t N, int H, bf16* __restrict__ dAT /* nullable: this
                                                          step's column block of dA^T [4H][T Np] */, int64_t ldT, int64_t Np, int64_t NU, int units_per_wg,
                                                          float* __restrict__ gbias /* nullable: [4H] += column sums of dA (the bias gradient) */) {
  constexpr int HC = 8 * NW, Q = HC / 4;
  __shared__ __attribute__((aligned(16))) float sH[32][HC + 4];
  __shared__ __attribute__((aligned(16))) float sC[32][HC + 4];
  __shared__ __attribute__((aligned(16))) bf16 sA[32][4][HC + 8];
  const int tid = threadIdx.x;
  const int c = blockIdx.y, NCH = gridDim.y, ub = HC * c;
  // A workgroup walks units_per_wg 32-row units of its chunk: the bias gradient (column sums of dA, formerly a second sweep over dA^T: 1.2 GB
  // per step) is summed per thread -- thread (g, u) owns gate row g H + ub + u -- across the units and leaves as ONE atomic per thread.
  float bsum = 0.f;
  const int bg = tid / HC, bu = tid - bg * HC;   // (tid < 4 HC)
  for (int ui = 0; ui < units_per_wg; ++ui) {
    const int64_t unit = (int64_t)blockIdx.x * units_per_wg + ui;
    if (unit >= NU) break;   // (workgroup-uniform)
    const int64_t row0 = unit * 32;
    if (ui > 0) __syncthreads();   // (the previous unit's tiles have been read)
    for (int i = tid; i < 32 * Q; i += 256) {
      const int r = i / Q, q = i - r * Q;
      const int64_t n = row0 + r;
      f32x4 vh = f32x4{0.f, 0.f, 0.f, 0.f}, vc = vh;
      if (n < N) {
        vh = *(const f32x4*)(dH + n * H + ub + 4 * q);
        vc = *(const f32x4*)(dC + n * H + ub + 4 * q);
        if (dH_up) { const f32x4 u = *(const f32x4*)(dH_up + n * H + ub + 4 * q); vh += u; }
      }
      *(f32x4*)&sH[r][4 * q] = vh;
      *(f32x4*)&sC[r][4 * q] = vc;
    }
    __syncthreads();
    for (int rl = tid; rl < NW * 64; rl += 256) {
      const int w = rl >> 6, lane = rl & 63, ln = lane & 31, ul = 8 * w + 4 * (lane >> 5);
      const int64_t rec = ((unit * NCH + c) * NW + w) * 64 + lane;
      const bf16x8 a0 = A0[rec], a1 = A1[rec];
      const bf16x4 cc16 = cF[rec];
      bf16x4 cp16;
#pragma unroll
      for (int j = 0; j < 4; ++j) cp16[j] = (bf16)0.f;
      if (cprevF) cp16 = cprevF[rec];
      f32x4 cc, cp;
#pragma unroll
      for (int j = 0; j < 4; ++j) { cc[j] = (float)cc16[j]; cp[j] = (float)cp16[j]; }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float ig = (float)a0[j], gg = (float)a0[4 + j], fg = (float)a1[j], og = (float)a1[4 + j];
        const float tc = tanhf(cc[j]);
        const float dh = sH[ln][ul + j];
        const float dO = dh * tc;
        const float dc = sC[ln][ul + j] + dh * og * (1.f - tc * tc);
        sA[ln][0][ul + j] = tobf(dc * gg * ig * (1.f - ig));
        sA[ln][1][ul + j] = tobf(dc * ig * (1.f - gg * gg));
        sA[ln][2][ul + j] = tobf(dc * cp[j] * fg * (1.f - fg));
        sA[ln][3][ul + j] = tobf(dO * og * (1.f - og));
        sC[ln][ul + j] = dc * fg;
      }
    }
    __syncthreads();
    // (dH is not cleared: the recurrent product of this step -- dh_{t-1} = dA_t W_o2g, plain stores -- or the next head backward overwrites it)
    for (int i = tid; i < 32 * Q; i += 256) {
      const int r = i / Q, q = i - r * Q;
      const int64_t n = row0 + r;
      if (n < N) *(f32x4*)(dC + n * H + ub + 4 * q) = *(const f32x4*)&sC[r][4 * q];
    }
    constexpr int P8 = HC / 8;   // 16-byte pieces of a (row, gate) segment
    for (int i = tid; i < 32 * 4 * P8; i += 256) {
      const int p = i % P8, g = (i / P8) & 3, r = i / (4 * P8);
      const int64_t n = row0 + r;
      if (n < N) *(bf16x8*)(dA + n * (int64_t)4 * H + (int64_t)g * H + ub + 8 * p) = *(const bf16x8*)&sA[r][g][8 * p];
    }
    if (dAT) {   // the transposed image the dW products contract over (k-contiguous operands): this tile's 4 HC gate rows x 32 paths, pad columns zero
      for (int i = tid; i < 4 * HC * 4; i += 256) {
        const int r8 = i & 3, u = (i >> 2) % HC, g = i / (4 * HC);
        const int64_t n0 = row0 + 8 * r8;
        if (n0 >= Np) continue;
        bf16x8 v;
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (n0 + q < N) ? sA[8 * r8 + q][g][u] : (bf16)0.f;
        *(bf16x8*)(dAT + ((int64_t)g * H + ub + u) * ldT + n0) = v;
      }
    }
    if (gbias && tid < 4 * HC) {   // the bf16-rounded values, as the separate row sum over dA^T read them
      float sacc = 0.f;
#pragma unroll 8
      for (int r = 0; r < 32; ++r) sacc += (row0 + r < N) ? (float)sA[r][bg][bu] : 0.f;
      bsum += sacc;
    }
  }
  if (gbias && tid < 4 * HC && bsum != 0.f) unsafeAtomicAdd(gbias + (int64_t)bg * H + ub + bu, bsum);
}

// y[c][r] = x[r][c] for r < R, 0 for R <= r < Rp (the padded row count: 16-byte rows of y); x bf16 [R][C] (C a multiple of 8), y pitch
// ldy (a multiple of 8); 64 x 64 tiles through LDS, 16-byte global accesses on both sides
__global__ __launch_bounds__(256) void k_transpose16(const bf16* __restrict__ x, bf16* __restrict__ y, int64_t R, int64_t Rp, int64_t Cc, int64_t ldy) {
  __shared__ __attribute__((aligned(16))) bf16 t[64][72];
  const int64_t r0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int f = threadIdx.x + 256 * e;
    const int rr = f >> 3, cq = (f & 7) * 8;
    bf16x8 v;
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (bf16)0.f;
    if (r0 + rr < R && c0 + cq < Cc) v = *(const bf16x8*)(x + (r0 + rr) * Cc + c0 + cq);
    *(bf16x8*)(&t[rr][cq]) = v;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int f = threadIdx.x + 256 * e;
    const int cc = f >> 3, rq = (f & 7) * 8;
    if (c0 + cc < Cc && r0 + rq < Rp) {
      bf16x8 v;
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = t[rq + q][cc];
      *(bf16x8*)(y + (c0 + cc) * ldy + r0 + rq) = v;
    }
  }
}
// h^T [H][T Np] (the dW_o2g product's k-contiguous operand) from the persistent forward's FRAGMENT-order h records (lstm_bf16_persist.hip Cell::store:
// record (((t NU + unit) NCHF + chunk) 8 + wave) 64 + lane = hidden units 64 chunk + 8 wave + 4 (lane >> 5) .. + 3 of path 32 unit + (lane & 31)).
// One workgroup = (two units = 64 paths, one chunk of 64 hidden units, one step): 8 KB of records in, coalesced; transposed through LDS by two-byte
// writes; 128-byte rows out.  Paths past N are written as zeros (their records hold a repeated row).
__global__ __launch_bounds__(256) void k_hfrag_T(const bf16x4* __restrict__ HsF, bf16* __restrict__ HT, int64_t NU, int64_t step_recs, int64_t N, int64_t Np, int64_t ldT, int H) {
  constexpr int TP = 64 + 8;   // elements: 144-byte rows (the two lane halves of a record wave write rows 4 apart: other banks)
  __shared__ __attribute__((aligned(16))) bf16 tl[64][TP];
  const int tid = threadIdx.x, cf = blockIdx.y, t = blockIdx.z, NCHF = H / 64;
  const int64_t u0 = (int64_t)blockIdx.x * 2, n0 = u0 * 32;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = tid + 256 * e;              // record of the pair of units: unit r >> 9, wave (r >> 6) & 7, lane r & 63
    const int uu = r >> 9, wf = (r >> 6) & 7, lane = r & 63, ln = lane & 31, half = lane >> 5;
    bf16x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (bf16)0.f;
    if (u0 + uu < NU && n0 + 32 * uu + ln < N) v = HsF[(int64_t)t * step_recs + (((u0 + uu) * NCHF + cf) * 8 + wf) * 64 + lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) tl[8 * wf + 4 * half + j][32 * uu + ln] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int pc = tid + 256 * e, hl = pc >> 3, oct = pc & 7;
    if (n0 + 8 * oct < Np) *(bf16x8*)(HT + (int64_t)(64 * cf + hl) * ldT + (int64_t)t * Np + n0 + 8 * oct) = *(const bf16x8*)&tl[hl][8 * oct];
  }
}
// out[r] += sum of row r of x (bf16 [R][n], n a multiple of 8): the bias gradient from dA^T
__global__ __launch_bounds__(256) void k_rowsum16(const bf16* __restrict__ x, int64_t n, float* __restrict__ out) {
  __shared__ float red[256];
  const bf16* row = x + (int64_t)blockIdx.x * n;
  float acc = 0.f;
  for (int64_t i = (int64_t)threadIdx.x * 8; i < n; i += 256 * 8) {
    const bf16x8 v = *(const bf16x8*)(row + i);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc += (float)v[q];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int sft = 128; sft > 0; sft >>= 1) {
    if ((int)threadIdx.x < sft) red[threadIdx.x] += red[threadIdx.x + sft];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] += red[0];
}

// ---- small tables: their gradients through ONE extra column block of the dW product (round 5) -------------------------------------------------
// The step input is x = [Wt[type] | We[entity] | Wr[relation]] (FeatureEmbedding.lua:112-121), so with the one-hot selectors S_t, S_r of a batch
//   x_r = S_r Wr                          =>   dW_i2g[:, relation columns] = dA^T x_r = (dA^T S_r) Wr        = G_r Wr
//   dWr = S_r^T dx_r = S_r^T (dA W_i2g_r)  =>   dWr                         = (S_r^T dA) W_i2g_r              = G_r^T W_i2g[:, relation columns]
// and the same for the type table: the relation / type thirds of the dx product and of the dW_i2g product, and both table-gradient launches, collapse
// into G = dA^T [S_r | S_t] -- 128 more columns of the split-K dW product (Vr + Vt <= 128 one-hot rows, exact in bf16) -- plus two tiny fp32 products.
// configs[3] (100 relations, 6 types, d = 128): dx shrinks from N = 384 to the entity slice (N = 128: a third of the flops, one column tile, dA^T
// read once instead of three times), the two dW products become ONE over the operand Z^T = [x_e^T | S^T | h_{t-1}^T] (N = 640 instead of 768, dA^T read
// by one launch instead of two), the one-hot table-gradient launch (0.27 ms, 400 MB of dx) and two thirds of the X^T gather disappear.
// G is a sum of bf16 dA values in fp32 and the small products run in fp32 on the same bf16 shadows the big ones read: the same gradient, fewer roundings.
//
// S^T rows of the operand: row r < Vr is relation r + 1, row Vr + y is type y + 1 (num_types = 1); [128][T][Np], pad columns zero.
__global__ __launch_bounds__(256) void k_onehot_T(const int32_t* __restrict__ idx, int64_t N, int64_t Np, int T, int F, int Vr, int Vt, bf16* __restrict__ ST, int64_t ldT) {
  __shared__ int rid[64], tyid[64];
  const int64_t n0 = (int64_t)blockIdx.x * 64;
  const int t = blockIdx.y;
  if (threadIdx.x < 64) {
    const int64_t n = n0 + threadIdx.x;
    const int32_t* id = idx + ((n < N ? n : N - 1) * T + t) * F;
    const int r = id[F - 1] - 1, y = id[F - 3] - 1;
    rid[threadIdx.x] = n < N ? r : -1;
    tyid[threadIdx.x] = n < N ? Vr + y : -1;
  }
  __syncthreads();
  const int row = threadIdx.x >> 1, half = threadIdx.x & 1;
  typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p0 = 32 * half + 8 * q;
    if (n0 + p0 >= Np) continue;
    u16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (rid[p0 + e] == row || tyid[p0 + e] == row) ? (unsigned short)0x3f80 : (unsigned short)0;   // bf16 1.0
    *(u16x8*)(ST + (int64_t)row * ldT + (int64_t)t * Np + n0 + p0) = v;
  }
}
// What the merged product leaves in Ct [4H][NZ] (NZ = de + 128 + H: entity columns | G | recurrent columns) goes where the optimiser reads it (all +=):
// workgroups [0, 4H): one gate row each -- gW_i2g[k][:] = [G_t Wt | Ct entity block | G_r Wr], gW_o2g[k][:]; workgroups behind them: one table row
// each -- gWr[r][:] += sum_k G[k][r] W_i2g[k][relation columns] (no atomics: a fixed summation order), likewise gWt.
struct FinArgs {
  const float* Ct; int NZ, G4, Din, H, dt, de, dr, Vt, Vr;
  const bf16* Wt16; const bf16* Wr16; const bf16* Wi16;
  float* gWi; float* gWo; float* gWt; float* gWr;
};
__global__ __launch_bounds__(256) void k_small_tables_finish(FinArgs a) {
  __shared__ float g[128];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < a.G4) {
    const int k = blockIdx.x;
    const float* row = a.Ct + (int64_t)k * a.NZ;
    if (tid < 128) g[tid] = row[a.de + tid];
    __syncthreads();
    for (int j = tid; j < a.Din; j += 256) {
      float v = 0.f;
      if (j < a.dt) {
        for (int y = 0; y < a.Vt; ++y) v += g[a.Vr + y] * (float)a.Wt16[y * a.dt + j];
      } else if (j < a.dt + a.de) {
        v = row[j - a.dt];
      } else {
        const int jj = j - a.dt - a.de;
#pragma unroll 4
        for (int r = 0; r < a.Vr; ++r) v += g[r] * (float)a.Wr16[r * a.dr + jj];
      }
      a.gWi[(int64_t)k * a.Din + j] += v;
    }
    for (int j = tid; j < a.H; j += 256) a.gWo[(int64_t)k * a.H + j] += row[a.de + 128 + j];
    return;
  }
  // one workgroup per one-hot row r (relation r, or type r - Vr), no atomics: two interleaved K sub-sums per column added in a fixed order
  __shared__ float red[256];
  const int r = (int)blockIdx.x - a.G4;
  const bool rel = r < a.Vr;
  const int w = rel ? a.dr : a.dt, col0 = rel ? a.dt + a.de : 0;
  const int j = tid & 127, sb = tid >> 7;
  const int jc = j < w ? j : w - 1;   // (w <= 128; idle lanes re-read the last column: loads stay unconditional)
  float acc = 0.f;
#pragma unroll 8
  for (int k = sb; k < a.G4; k += 2) acc += a.Ct[(int64_t)k * a.NZ + a.de + r] * (float)a.Wi16[(int64_t)k * a.Din + col0 + jc];
  red[tid] = acc;
  __syncthreads();
  if (sb == 0 && j < w) (rel ? a.gWr + (int64_t)r * a.dr : a.gWt + (int64_t)(r - a.Vr) * a.dt)[j] += red[tid] + red[tid + 128];
}

// ---- state + orchestration --------------------------------------------------------------------------------------------------
// lstm_bf16_persist.hip: fragment-order saves of the persistent layer kernel's training launch
struct PersistSaves { const bf16* CsF; const bf16* ActF0; const bf16* ActF1; const bf16* HsF; int64_t NU, step_recs; int NW; };

struct State {
  bf16* We16 = nullptr; bool we_all_dirty = true;
  bf16* dense16 = nullptr;      // bf16 image of the dense arena (same offsets)
  bf16* WT16 = nullptr;         // per layer: W_i2g^T [Din][4H] | W_o2g^T [H][4H]
  bool dense_dirty = true;
  bf16* zero = nullptr;         // 256 zero bytes: the source of every out-of-range DMA piece of the gx products (gemm_bf16.hip)
  int64_t cap_N = 0; int cap_T = 0;
  bf16 *X16 = nullptr, *XT16 = nullptr, *H16 = nullptr, *HT16 = nullptr, *ACT16 = nullptr, *dA16 = nullptr, *dAT16 = nullptr;
  bf16* ZT16 = nullptr; int64_t z_cap = 0;   // small-table backward: the merged dW product's operand [x_e^T | S^T | h_{t-1}^T], [de + 128 + H][T][Np]
  float* Ctmp = nullptr; int64_t ct_cap = 0; //   ... and its result [4H][de + 128 + H]
  void* persist = nullptr;      // lstm_bf16_persist.hip: packed weights + scratch slabs of the persistent layer kernel
  bool pack_dirty = true;       // its packed weights are stale
  void* persist_bwd = nullptr;  // lstm_bf16_bwd_persist.hip: packed W_o2g^T fragments of the persistent BPTT kernel
  bool packb_dirty = true;
  bool bias_in_gates = false;   // k_gates_bwd16_frag also summed the bias gradient (measurement switch)
  bool act_frag = false;        // the last training forward wrote c and the gate planes in fragment order (persistent kernel; k_gates_bwd16_frag)
  PersistSaves sv{};
  // the backward's side stream (backward(): the memory-bound helpers run beside the matrix-core launches they do not depend on)
  int side_probes = 0;   // candidates make_concurrent_stream tried for it
  hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_operands = nullptr, ev_dx = nullptr, ev_join = nullptr;
};
// lstm_bf16_persist.hip: the whole layer (gather + T steps) as one persistent launch
bool persist_shape_ok(const kprn_handle* h, const kprn_batch* b);
void persist_forward(kprn_handle* h, const kprn_batch* b, bool save, void*& st, bool repack, const bf16* Wt16, const bf16* We16, const bf16* Wr16, bf16* H16,
                     PersistSaves* sv);
void persist_release(void*& st);
// lstm_bf16_bwd_persist.hip: BPTT through the layer (cell backward + recurrent product of all T steps) as one persistent launch
bool persist_bwd_shape_ok(const kprn_handle* h, const PersistSaves& sv, int64_t N, int T);
void persist_backward(kprn_handle* h, int64_t N, int T, int cid, const PersistSaves& sv, void*& st, bool repack, bf16* dA16 /* nullable: no row-major copy */, bf16* dAT16, int64_t Np,
                      float* dXe /* nullable: the launch also forms the entity slice of dx, [T][N][de] */, int64_t ldT /* row pitch of dA^T, T Np .. T Np + 512 */);
bool persist_bwd_dxe_ok(const kprn_handle* h);
void persist_bwd_release(void*& st);
template <typename Tp> static Tp* dal(int64_t n) {
  void* p = nullptr;
  hipError_t e = kprn_dev_malloc(&p, (size_t)std::max<int64_t>(n, 1) * sizeof(Tp));
  if (e != hipSuccess) throw KprnError{KPRN_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e)};
  return (Tp*)p;
}
static State* st(kprn_handle* h) {
  if (!h->bf16_state) h->bf16_state = new State();
  State* s = (State*)h->bf16_state;
  if (!s->zero) {   // (once per handle, on its device; the device-wide wait makes it zero for every stream a later pass runs on)
    bf16* z = dal<bf16>(128);
    if (hipMemset(z, 0, 256) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { hipFree(z); throw KprnError{KPRN_E_NOMEM, "hipMemset failed (zero block)"}; }
    s->zero = z;
  }
  return s;
}
static int64_t wt_off(const kprn_handle* h, int l) {   // offset of layer l's transposed pair inside WT16
  int64_t o = 0;
  for (int k = 0; k < l; ++k) o += (int64_t)4 * h->cfg.H * (h->layer[k].Din + h->cfg.H);
  return o;
}

bool supported(const kprn_handle* h, const kprn_batch* b) {
  const kprn_config& c = h->cfg;
  const int64_t N = b->N;
  return c.compute_dtype == 1 && c.rnn_type == 0 && h->impl == 0 && N >= 256 && c.dt > 0 && c.de > 0 && (c.dt % 8) == 0 && (c.de % 8) == 0 && (c.dr % 8) == 0 && (c.H % 8) == 0;
}

void params_changed(kprn_handle* h, bool entity_rows_only) {
  if (!h->bf16_state) return;
  State* s = (State*)h->bf16_state;
  s->dense_dirty = true;
  s->pack_dirty = true;
  s->packb_dirty = true;
  if (!entity_rows_only) s->we_all_dirty = true;
}

// the optimiser / the catch-up replay rewrote these rows of entity_emb: refresh their shadow
void rows_updated(kprn_handle* h, const int32_t* rows, const int32_t* count, int64_t max_rows) {
  if (!h->bf16_state) return;
  State* s = (State*)h->bf16_state;
  if (s->we_all_dirty || !s->We16 || max_rows <= 0) return;   // (a full conversion is pending anyway)
  const int de = h->cfg.de;
  const int64_t work = max_rows * (de >> 2);
  hipLaunchKernelGGL(k_rows_cvt, dim3((unsigned)std::min<int64_t>((work + 255) / 256, 4096)), dim3(256), 0, h->stream, h->We, s->We16, rows, count, de);
  HIP_TRY(hipGetLastError());
}

void release(kprn_handle* h) {
  State* s = (State*)h->bf16_state;
  if (!s) return;
  for (bf16* p : {s->We16, s->dense16, s->WT16, s->zero, s->X16, s->XT16, s->H16, s->HT16, s->ACT16, s->dA16, s->dAT16, s->ZT16}) if (p) hipFree(p);
  if (s->Ctmp) hipFree(s->Ctmp);
  persist_release(s->persist);
  persist_bwd_release(s->persist_bwd);
  if (s->side) {
    hipStreamSynchronize(s->side); hipStreamDestroy(s->side);
    for (hipEvent_t e : {s->ev_fork, s->ev_operands, s->ev_dx, s->ev_join}) if (e) hipEventDestroy(e);
  }
  delete s;
  h->bf16_state = nullptr;
}

static void refresh_shadows(kprn_handle* h) {
  State* s = st(h);
  const kprn_config& c = h->cfg;
  hipStream_t strm = h->stream;
  if (!s->We16) { s->We16 = dal<bf16>(h->n_ent); s->we_all_dirty = true; }
  if (!s->dense16) { s->dense16 = dal<bf16>(h->n_dense); s->WT16 = dal<bf16>(wt_off(h, c.L)); s->dense_dirty = true; }
  if (s->we_all_dirty) {
    ProfScope ps(h, "bf16_shadow_table");
    cvt16(strm, h->We, s->We16, h->n_ent);
    s->we_all_dirty = false;
  }
  if (s->dense_dirty) {
    ProfScope ps(h, "bf16_shadow_weights");
    cvt16(strm, h->dense, s->dense16, h->n_dense);
    for (int l = 0; l < c.L; ++l) {
      const int Din = h->layer[l].Din, G4 = 4 * c.H;
      bf16* wt = s->WT16 + wt_off(h, l);
      hipLaunchKernelGGL(k_cvt_T, dim3((unsigned)(((int64_t)G4 * Din + 255) / 256)), dim3(256), 0, strm, h->dense + h->layer[l].Wi, wt, G4, Din);
      hipLaunchKernelGGL(k_cvt_T, dim3((unsigned)(((int64_t)G4 * c.H + 255) / 256)), dim3(256), 0, strm, h->dense + h->layer[l].Wo, wt + (int64_t)G4 * Din, G4, c.H);
    }
    s->dense_dirty = false;
  }
  HIP_TRY(hipGetLastError());
}

static void ensure_buffers(kprn_handle* h, int64_t N, int T) {
  State* s = st(h);
  if (N <= s->cap_N && T <= s->cap_T) return;
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (bf16** p : {&s->X16, &s->XT16, &s->H16, &s->HT16, &s->ACT16, &s->dA16, &s->dAT16}) if (*p) { hipFree(*p); *p = nullptr; }
  const kprn_config& c = h->cfg;
  const int64_t cn = std::max(N, s->cap_N);
  const int ct = std::max(T, s->cap_T);
  const int64_t rows = cn * ct, rows_p = ((cn + 7) & ~(int64_t)7) * ct;
  const int Dm = std::max(h->D, c.H);
  s->X16 = dal<bf16>(rows * h->D); s->XT16 = dal<bf16>(rows_p * Dm);
  s->H16 = dal<bf16>((int64_t)c.L * rows * c.H); s->HT16 = dal<bf16>(rows_p * c.H);
  s->ACT16 = dal<bf16>((int64_t)c.L * rows * 4 * c.H);
  s->dA16 = dal<bf16>(rows * 4 * c.H); s->dAT16 = dal<bf16>((rows_p + 512) * 4 * c.H);   // (+ 512: room for a padded row pitch, t_pitch)
  s->cap_N = cn; s->cap_T = ct;
}

// nn.Linear(H, C) on the last step's h for the bf16 pipeline (OneModel.lua:275): S[n][c] = sum_k bf16(h_T[n][k]) bf16(W_out[c][k]) + b[c], fp32 accumulation --
// the arithmetic the generic product did for this call (fp32 operands rounded to bf16 as fragments are formed), as its own launch: that product
// spent 0.082 ms per call on configs[3] (twice per step: 100 MB of h_T through 64 x 64 tiles of 4-byte loads); this is one pass over h_T.
// A wave owns 16 paths x all classes (NT column tiles of v_mfma_f32_16x16x32_bf16); a lane reads 64 contiguous bytes of its path's row per 64-k block
// -- the MFMA's k index is permuted to make that so (k = 64 j + 16 kg + 8 i + q), and the weights sit in LDS in the same permuted fragment order.
// The launch is a handful of round trips (weight fragments, then per block of 16 paths the row and the stores), so the fragment fill and a block's
// row are each requested in one go (first build: 9 + 6 dependent round trips, 0.039 ms).
template <int NT, int NJ>   // NT: 16-class column tiles; NJ = H / 64
__global__ __launch_bounds__(256) void k_head_fwd16(const float* __restrict__ hT, const bf16* __restrict__ W16, const float* __restrict__ bias,
                                                       float* __restrict__ S, int64_t N, int C) {
  constexpr int H = 64 * NJ, E = NJ * 2 * NT * 64, PE = (E + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) bf16x8 wf[];   // [NJ][2][NT][64 lanes]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  {
    // the weight fragments: all of a thread's pieces requested together, from clamped addresses; rows past C are zeroed by a mask the optimiser
    // cannot see through (a select here would put each load and its wait inside a branch: PE dependent round trips before the first row is read)
    u32x4 v[PE];
#pragma unroll
    for (int i = 0; i < PE; ++i) {
      const int e0 = threadIdx.x + 256 * i, e = e0 < E ? e0 : E - 1;
      const int l = e & 63, nt = (e >> 6) % NT, ji = (e >> 6) / NT;
      const int cls = nt * 16 + (l & 15);
      v[i] = *(const u32x4*)(W16 + (int64_t)(cls < C ? cls : C - 1) * H + 64 * (ji >> 1) + 16 * (l >> 4) + 8 * (ji & 1));
    }
#pragma unroll
    for (int i = 0; i < PE; ++i) {
      const int e = threadIdx.x + 256 * i;
      unsigned m = ((e >> 6) % NT) * 16 + (e & 15) < C ? 0xffffffffu : 0u;
      asm("" : "+v"(m));
      if (E % 256 == 0 || e < E) *(u32x4*)(wf + e) = v[i] & m;
    }
  }
  float bj[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) { const int col = nt * 16 + (lane & 15); bj[nt] = bias[col < C ? col : C - 1]; }
  __syncthreads();
  for (int64_t blk = (int64_t)blockIdx.x * 4 + wave; blk * 16 < N; blk += (int64_t)gridDim.x * 4) {
    const int64_t row = blk * 16 + (lane & 15);
    const float* src = hT + (row < N ? row : N - 1) * H + 16 * (lane >> 4);
    asm volatile("" ::: "memory");   // (keeps the weight fragments in LDS: hoisted out of this loop they take 48 NT registers and the row loads get serialized)
    f32x4 x[NJ][4];   // this lane's share of its path's row, requested at once: one round trip per 16 paths
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) x[j][q] = *(const f32x4*)(src + 64 * j + 4 * q);
    __builtin_amdgcn_sched_barrier(0);   // all 4 NJ requests are issued before the first is used (left alone, hipcc sinks each load down to its MFMA)
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      bf16x8 a0, a1;
#pragma unroll
      for (int q = 0; q < 4; ++q) { a0[q] = tobf(x[j][0][q]); a0[4 + q] = tobf(x[j][1][q]); a1[q] = tobf(x[j][2][q]); a1[4 + q] = tobf(x[j][3][q]); }
      const bf16x8* w0 = wf + (size_t)(j * 2) * NT * 64 + lane;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, w0[nt * 64], acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, w0[(NT + nt) * 64], acc[nt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = nt * 16 + (lane & 15);
      if (col >= C) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t ro = blk * 16 + 4 * (lane >> 4) + r;   // D: lane (col, rg) register r <-> row 4 rg + r
        if (ro < N) S[ro * C + col] = acc[nt][r] + bj[nt];
      }
    }
  }
}
// false: a shape this launch does not take (the caller falls back to the generic product).  KPRN_BF16_HEAD=0: always false (A/B)
static bool head_fwd16(hipStream_t s, const float* hT, const bf16* W16, const float* bias, float* S, int64_t N, int H, int C) {
  static const bool off = KPRN_DEV_ENV("KPRN_BF16_HEAD") && KPRN_DEV_ENV("KPRN_BF16_HEAD")[0] == '0';
  const int NT = (C + 15) / 16, NJ = H >> 6;
  const size_t lds = (size_t)NJ * 2 * NT * 64 * sizeof(bf16x8);
  if (off || N <= 0 || (H & 63) || C < 1 || NT > 4 || !(NJ == 2 || NJ == 3 || NJ == 4 || NJ == 6) || ((uintptr_t)W16 & 15) || ((uintptr_t)hT & 15)) return false;
  const dim3 grid((unsigned)std::min<int64_t>((N + 63) / 64, 2 * 256));   // two workgroups per CU (<= 256 registers per lane), all resident: a wave walks its blocks
#define KPRN_HF(NTv, NJv) hipLaunchKernelGGL((k_head_fwd16<NTv, NJv>), grid, dim3(256), lds, s, hT, W16, bias, S, N, C)
#define KPRN_HF_NJ(NTv) do { if (NJ == 2) KPRN_HF(NTv, 2); else if (NJ == 3) KPRN_HF(NTv, 3); else if (NJ == 4) KPRN_HF(NTv, 4); else KPRN_HF(NTv, 6); } while (0)
  if (NT == 1) KPRN_HF_NJ(1); else if (NT == 2) KPRN_HF_NJ(2); else if (NT == 3) KPRN_HF_NJ(3); else KPRN_HF_NJ(4);
#undef KPRN_HF_NJ
#undef KPRN_HF
  HIP_TRY(hipGetLastError());
  return true;
}

// forward of the whole stack; the head runs on the fp32 h_T of the top layer (written by its last step) through the generic bf16-product GEMM
void forward(kprn_handle* h, const kprn_batch* b, bool save) {
  const kprn_config& c = h->cfg;
  State* s = st(h);
  Workspace& w = h->ws;
  hipStream_t strm = h->stream;
  const int H = c.H, L = c.L, T = b->T, D = h->D;
  const int64_t N = b->N;
  refresh_shadows(h);
  ensure_buffers(h, N, T);
  const bool persist = persist_shape_ok(h, b);
  if (!persist) {   // (the persistent kernel gathers for itself, and the backward then builds the dW product's operand X^T from the tables: k_gather16_T)
    ProfScope ps(h, "embed_gather_bf16");
    const int64_t work = N * T * (D >> 3);
    hipLaunchKernelGGL(k_gather16, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, strm, b->idx, N, T, b->F, c.num_types, s->dense16 + h->off_Wt, s->We16,
                       s->dense16 + h->off_Wr, c.dt, c.de, c.dr, s->X16);
    HIP_TRY(hipGetLastError());
  }
  if (persist) {
    persist_forward(h, b, save, s->persist, s->pack_dirty, s->dense16 + h->off_Wt, s->We16, s->dense16 + h->off_Wr, /*row-major h plane: not needed, h^T is built from the fragment-order records*/ nullptr, &s->sv);
    s->pack_dirty = false;
    if (save) s->act_frag = true;
  }
  if (!persist && save) s->act_frag = false;
  for (int l = 0; l < L && !persist; ++l) {
    const int Din = h->layer[l].Din;
    const bf16* in = (l == 0) ? s->X16 : s->H16 + (int64_t)(l - 1) * T * N * H;
    bf16* hs = s->H16 + (int64_t)l * T * N * H;
    float* cs = w.Cs + (int64_t)l * T * N * H;
    bf16* act = s->ACT16 + (int64_t)l * T * N * 4 * H;
    ProfScope ps(h, "lstm_step_bf16");
    ps.launches = T;
    for (int t = 0; t < T; ++t) {
      GArgs a;
      memset(&a, 0, sizeof(a));
      a.A = in + (int64_t)t * N * Din; a.lda = Din; a.B = s->dense16 + h->layer[l].Wi; a.ldb = Din; a.K = Din;
      if (t > 0) { a.A2 = hs + (int64_t)(t - 1) * N * H; a.lda2 = H; a.B2 = s->dense16 + h->layer[l].Wo; a.ldb2 = H; a.K2 = H; }
      a.M = N; a.N = 4 * H; a.H = H; a.bias = h->dense + h->layer[l].bi;
      a.cprev = t > 0 ? cs + (int64_t)(t - 1) * N * H : nullptr; a.cout = cs + (int64_t)t * N * H;
      a.hout = hs + (int64_t)t * N * H; a.ldh = H; a.act = save ? act + (int64_t)t * N * 4 * H : nullptr;
      a.hout_f32 = (l == L - 1 && t == T - 1) ? w.Hs + ((int64_t)(L - 1) * T + (T - 1)) * N * H : nullptr;
      lstm_step16(strm, a);
    }
  }
  {
    ProfScope ps(h, "gemm_head_fwd");
    const float* hT = w.Hs + ((int64_t)(L - 1) * T + (T - 1)) * N * H;
    if (!head_fwd16(strm, hT, s->dense16 + h->off_outW, h->dense + h->off_outb, w.S, N, H, c.C))
      gemm::run(strm, hT, H, 1, h->dense + h->off_outW, 1, H, w.S, c.C, N, c.C, H, false, h->dense + h->off_outb, 1, true);
  }
}

// time-major x [T][N][C] -> y [C][T][Np] (Np = N rounded up to 8: every step's block of a row starts on 16 bytes, pad columns zero)
static void transpose_steps(hipStream_t s, const bf16* x, bf16* y, int T, int64_t N, int64_t Np, int64_t Cc) {
  for (int t = 0; t < T; ++t)
    hipLaunchKernelGGL(k_transpose16, dim3((unsigned)((Np + 63) / 64), (unsigned)((Cc + 63) / 64)), dim3(256), 0, s, x + (int64_t)t * N * Cc, y + (int64_t)t * Np, N, Np,
                       Cc, (int64_t)T * Np);
  HIP_TRY(hipGetLastError());
}

// needs forward(save = true) of the same batch; ws.dS holds d loss / d S[:, cid]
void backward(kprn_handle* h, const kprn_batch* b, int cid) {
  const kprn_config& c = h->cfg;
  State* s = st(h);
  Workspace& w = h->ws;
  hipStream_t strm = h->stream;
  const int H = c.H, L = c.L, T = b->T, D = h->D, G4 = 4 * c.H;
  const int64_t N = b->N, TN = (int64_t)T * N;
  const Bf16GemmOpts go = h->bf16_gemm;   // the products' A/B switches (options "bf16_gemm_*")
  float* gd = h->g_dense;
  // the persistent BPTT launch forms dh_T = dS W_out[cid] itself and keeps dh / dc on the chip: no dH plane, no dC plane
  const bool bptt_persist = s->act_frag && L == 1 && persist_bwd_shape_ok(h, s->sv, N, T);
  // Side stream (with the persistent BPTT launch): what is left of this backward is a chain of matrix-core launches -- BPTT, the dx product,
  // the two dW products -- and memory-bound helpers that each depend on only part of it.  The helpers run on a second stream beside the
  // launches they do not depend on: the head's backward and the two transposed operands of the dW products (in^T gathered from the tables,
  // h^T from the forward's records) beside BPTT; the three table gradients (they need dx only) beside the dW products.  The main stream
  // waits for the side stream before this function returns: nothing outside sees two streams.  KPRN_BF16_BWD_OVERLAP=0: one stream.
  static const bool overlap_env = [] { const char* e = getenv("KPRN_BF16_BWD_OVERLAP"); return !(e && e[0] == '0'); }();
  const bool overlap = bptt_persist && overlap_env;
  if (overlap && !s->side) {
    s->side = make_concurrent_stream(h, &s->side_probes);
    for (hipEvent_t* e : {&s->ev_fork, &s->ev_operands, &s->ev_dx, &s->ev_join}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  hipStream_t side = overlap ? s->side : strm;
  // an error thrown between the fork and the join below must not leave helpers running behind the caller's back: drain the side stream on the way out
  struct SideGuard {
    hipStream_t st; bool joined;
    ~SideGuard() { if (st && !joined) (void)hipStreamSynchronize(st); }
  } side_guard{overlap ? side : nullptr, false};
  if (overlap) {
    HIP_TRY(hipEventRecord(s->ev_fork, strm));
    HIP_TRY(hipStreamWaitEvent(side, s->ev_fork, 0));
  }
  {
    ProfScope ps(h, "head_bwd", side);
    const float* hT = w.Hs + ((int64_t)(L - 1) * T + (T - 1)) * N * H;
    kk::head_bwd(side, w.dS, hT, h->dense + h->off_outW, N, H, cid, bptt_persist ? nullptr : w.dH, gd + h->off_outW, gd + h->off_outb);
  }
  if (!bptt_persist) HIP_TRY(hipMemsetAsync(w.dC, 0, (size_t)N * H * sizeof(float), strm));
  for (int l = L - 1; l >= 0; --l) {
    const int Din = h->layer[l].Din;
    const bf16* act = s->ACT16 + (int64_t)l * TN * G4;
    const bf16* hs = s->H16 + (int64_t)l * TN * H;
    const float* cs = w.Cs + (int64_t)l * TN * H;
    const bf16* wt = s->WT16 + wt_off(h, l);          // W_i2g^T [Din][4H] | W_o2g^T [H][4H]
    const bool has_up = (l < L - 1);
    if (has_up) {
      HIP_TRY(hipMemsetAsync(w.dH, 0, (size_t)N * H * sizeof(float), strm));
      HIP_TRY(hipMemsetAsync(w.dC, 0, (size_t)N * H * sizeof(float), strm));
    }
    // dx straight from the transposed dA the BPTT launch writes for the dW products (gx::k_gemm16xt): that launch then writes no row-major copy
    const int64_t Np_ = (N + 7) & ~(int64_t)7;
    const bool dx_t = bptt_persist && dx_from_transposed_ok((int64_t)T * Np_, Din, G4, Np_);
    // Small tables (see k_onehot_T): dx for the entity slice only, ONE dW product over [x_e^T | S^T | h_{t-1}^T], the type / relation gradients from G.
    const bool tabs = bptt_persist && dx_t && l == 0 && h->bf16_small_tables && c.num_types == 1 && c.Vt + c.Vr <= 128 && c.dt <= 128 && c.dr <= 128 &&
                      c.de >= 128 && T > 1 && b->key_sorted != nullptr && !b->tile_k && s->sv.HsF && (H % 64) == 0;
    // ... and that slice of dx formed inside the BPTT launch itself (a fourth result tile per wave): no dx product launch, dA^T read once less
    const bool dxe_in_bptt = tabs && h->bf16_bptt_dxe != 0 && persist_bwd_dxe_ok(h);
    // Row pitch of the transposed images of the small-table route: T Np elements is 3 x 2^18 bytes at the bench's size -- the 1 536 rows of dA^T (and the 640 of the
    // merged product's other operand) that a K range touches then start at addresses 786 432 bytes apart, i.e. on the same few HBM channels.  A pad of bf16_t_pad
    // elements (kprn_set_option "bf16_t_pad", default 64 = one 128-byte line) walks consecutive rows over consecutive channels.
    const int64_t ldz = (int64_t)T * Np_ + (tabs ? h->bf16_t_pad : 0);
    if (bptt_persist) {
      persist_backward(h, N, T, cid, s->sv, s->persist_bwd, s->packb_dirty, dx_t ? nullptr : s->dA16, s->dAT16, Np_, dxe_in_bptt ? w.dIn : nullptr, ldz);
      s->packb_dirty = false;
      s->bias_in_gates = true;   // (the launch sums the bias gradient from the dA^T pieces it writes)
    }
    for (int t = T - 1; t >= 0 && !bptt_persist; --t) {
      bf16* dA_t = s->dA16 + (int64_t)t * N * G4;
      {
        ProfScope ps(h, "lstm_gates_bwd_bf16");
        if (s->act_frag && l == 0) {   // the persistent layer kernel's fragment-order saves
          const PersistSaves& v = s->sv;
          const int NCH = H / (8 * v.NW);
          const bf16x8* a0 = (const bf16x8*)v.ActF0 + (int64_t)t * v.step_recs;
          const bf16x8* a1 = (const bf16x8*)v.ActF1 + (int64_t)t * v.step_recs;
          const bf16x4* cf = (const bf16x4*)v.CsF + (int64_t)t * v.step_recs;
          const bf16x4* cpf = t > 0 ? (const bf16x4*)v.CsF + (int64_t)(t - 1) * v.step_recs : nullptr;
          const float* up = has_up ? w.dIn + (int64_t)t * N * H : nullptr;
          const int64_t Np_ = (N + 7) & ~(int64_t)7;
          bf16* dat = s->dAT16 + (int64_t)t * Np_;   // (this kernel has the tile in LDS: it writes the transposed image too, no transpose pass for dA)
          // Measured (configs[3], ms per launch): one unit per workgroup, bias sums left to k_rowsum16 0.224; the bias gradient summed here
          // 0.26-0.29 (units per workgroup 4 / 2 / 1 / 8) -- 6 x 0.04-0.06 costs what the separate sweep over dA^T costs (0.20 ms), so it stays
          // a separate launch; KPRN_GATES_FUSED_BIAS=<units per workgroup> switches the fused form on.
          static const int fb_env = KPRN_DEV_ENV("KPRN_GATES_FUSED_BIAS") ? atoi(KPRN_DEV_ENV("KPRN_GATES_FUSED_BIAS")) : 0;
          s->bias_in_gates = fb_env > 0;
          const int upw = fb_env > 0 ? fb_env : 1;
          const dim3 grid((unsigned)((v.NU + upw - 1) / upw), (unsigned)NCH);
          float* gb = fb_env > 0 ? gd + h->layer[l].bi : nullptr;
          if (v.NW == 8) hipLaunchKernelGGL((k_gates_bwd16_frag<8>), grid, dim3(256), 0, strm, a0, a1, cf, cpf, up, w.dH, w.dC, dA_t, N, H, dat, (int64_t)T * Np_, Np_, (int64_t)v.NU, upw, gb);
          else hipLaunchKernelGGL((k_gates_bwd16_frag<4>), grid, dim3(256), 0, strm, a0, a1, cf, cpf, up, w.dH, w.dC, dA_t, N, H, dat, (int64_t)T * Np_, Np_, (int64_t)v.NU, upw, gb);
        } else {
          hipLaunchKernelGGL(k_gates_bwd16, dim3((unsigned)((N * H + 255) / 256)), dim3(256), 0, strm, act + (int64_t)t * N * G4, cs + (int64_t)t * N * H,
                             t > 0 ? cs + (int64_t)(t - 1) * N * H : nullptr, has_up ? w.dIn + (int64_t)t * N * H : nullptr, w.dH, w.dC, dA_t, N, H);
        }
        HIP_TRY(hipGetLastError());
      }
      if (t > 0) {
        ProfScope ps(h, "gemm_o2g_bwd_dh");   // dh_{t-1} = dA_t W_o2g
        gemm16(strm, go, s->zero, dA_t, G4, wt + (int64_t)G4 * Din, G4, w.dH, H, N, H, G4, false, nullptr, 1);
      }
    }
    const int64_t Np = (N + 7) & ~(int64_t)7, TNp = (int64_t)T * Np;   // padded step blocks of the transposed images (pads are zero)
    if (tabs) {
      const int NZ = c.de + 128 + H;
      if (ldz * NZ > s->z_cap) {
        HIP_TRY(hipStreamSynchronize(strm));
        if (overlap) HIP_TRY(hipStreamSynchronize(side));
        if (s->ZT16) hipFree(s->ZT16);
        s->ZT16 = nullptr; s->ZT16 = dal<bf16>(ldz * NZ); s->z_cap = ldz * NZ;
      }
      if ((int64_t)G4 * NZ > s->ct_cap) {
        HIP_TRY(hipStreamSynchronize(strm));
        if (s->Ctmp) hipFree(s->Ctmp);
        s->Ctmp = nullptr; s->Ctmp = dal<float>((int64_t)G4 * NZ); s->ct_cap = (int64_t)G4 * NZ;
      }
      bf16* zt_e = s->ZT16;                              // rows [0, de): x_e^T, the entity slice of the step input
      bf16* zt_s = s->ZT16 + (int64_t)c.de * ldz;        // rows [de, de + 128): the one-hot selectors
      bf16* zt_h = s->ZT16 + (int64_t)(c.de + 128) * ldz;   // rows behind them: h_{t-1}^T (step block 0 zero)
      {
        ProfScope ps(h, "bf16_transposes", side);   // (side stream: beside the BPTT launch queued above -- nothing here reads what it writes)
        hipLaunchKernelGGL(k_gather16_T, dim3((unsigned)((Np + 63) / 64), (unsigned)((c.de + 63) / 64), (unsigned)T), dim3(256), 0, side, b->idx, N, Np, T, b->F, 1,
                           s->We16, s->We16, s->We16, 0, c.de, 0, zt_e, ldz);
        hipLaunchKernelGGL(k_onehot_T, dim3((unsigned)((Np + 63) / 64), (unsigned)T), dim3(256), 0, side, b->idx, N, Np, T, b->F, c.Vr, c.Vt, zt_s, ldz);
        HIP_TRY(hipMemset2DAsync(zt_h, (size_t)ldz * sizeof(bf16), 0, (size_t)Np * sizeof(bf16), (size_t)H, side));
        hipLaunchKernelGGL(k_hfrag_T, dim3((unsigned)((s->sv.NU + 1) / 2), (unsigned)(H / 64), (unsigned)(T - 1)), dim3(256), 0, side, (const bf16x4*)s->sv.HsF, zt_h + Np,
                           (int64_t)s->sv.NU, (int64_t)s->sv.step_recs, N, Np, ldz, H);
        HIP_TRY(hipGetLastError());
      }
      if (overlap) HIP_TRY(hipEventRecord(s->ev_operands, side));
      if (!dxe_in_bptt) {
        ProfScope ps(h, "gemm_i2g_bwd_dx_e");   // dx_e [T N][de] = dA W_i2g[:, entity columns] (compact: what the entity gather-reduce reads)
        const bool ran = gemm16xt(strm, s->zero, s->dAT16, ldz, wt + (int64_t)c.dt * G4, G4, w.dIn, c.de, TNp, c.de, G4, Np, N);
        KPRN_REQUIRE(ran, KPRN_E_ARG, "bf16 backward: the transposed-dA dx product does not cover this shape (dx_from_transposed_ok said it would)");
      }
      if (overlap) {
        HIP_TRY(hipEventRecord(s->ev_dx, strm));
        HIP_TRY(hipStreamWaitEvent(side, s->ev_dx, 0));
        HIP_TRY(hipStreamWaitEvent(strm, s->ev_operands, 0));
      }
      {
        ProfScope ps(h, "entity_grad", side);   // (beside the merged dW product)
        bidx::entity_grad(side, w.dIn, /*frag_order=*/0, b->key_sorted, b->pos_sorted, b->n_index, N, T, c.de, 0, c.de, c.Ve, h->g_We);
      }
      {
        ProfScope ps(h, "gemm_bwd_dw_merged");   // Ct [4H][NZ] = dA^T [x_e^T | S^T | h_{t-1}^T]^T, split-K
        HIP_TRY(hipMemsetAsync(s->Ctmp, 0, (size_t)G4 * NZ * sizeof(float), strm));
        const int split = (int)std::min<int64_t>(1024, std::max<int64_t>(1, TN / 4096));
        // (h_{t-1}^T has no step -1: its column tiles skip the K ranges of step block 0 -- a tenth of the launch's workgroups; 8 K ranges per XCD so that
        //  whole workgroups fall into that block)
        if (!gemm16x(strm, go, s->zero, s->dAT16, ldz, s->ZT16, ldz, s->Ctmp, NZ, G4, NZ, TNp, true, split, c.de + 128, Np, 8))
          gemm16(strm, go, s->zero, s->dAT16, ldz, s->ZT16, ldz, s->Ctmp, NZ, G4, NZ, TNp, true, nullptr, split);
      }
      {
        ProfScope ps(h, "small_tables_finish");
        FinArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.Ct = s->Ctmp; fa.NZ = NZ; fa.G4 = G4; fa.Din = Din; fa.H = H; fa.dt = c.dt; fa.de = c.de; fa.dr = c.dr; fa.Vt = c.Vt; fa.Vr = c.Vr;
        fa.Wt16 = s->dense16 + h->off_Wt; fa.Wr16 = s->dense16 + h->off_Wr; fa.Wi16 = s->dense16 + h->layer[l].Wi;
        fa.gWi = gd + h->layer[l].Wi; fa.gWo = gd + h->layer[l].Wo; fa.gWt = gd + h->off_Wt; fa.gWr = gd + h->off_Wr;
        hipLaunchKernelGGL(k_small_tables_finish, dim3((unsigned)(G4 + c.Vr + c.Vt)), dim3(256), 0, strm, fa);
        HIP_TRY(hipGetLastError());
      }
      if (overlap) {
        HIP_TRY(hipEventRecord(s->ev_join, side));
        HIP_TRY(hipStreamWaitEvent(strm, s->ev_join, 0));
        side_guard.joined = true;
      }
      return;   // (L = 1: nothing below this layer)
    }
    {
      // (with the side stream: in^T and h^T are built there, beside the BPTT launch queued above -- neither reads anything it writes)
      ProfScope ps(h, "bf16_transposes", side);
      if (!(s->act_frag && l == 0)) transpose_steps(strm, s->dA16, s->dAT16, T, N, Np, G4);                       // dA^T [4H][T][Np] (the fragment-order gate backward wrote it)
      if (l == 0 && s->act_frag) {   // in^T gathered straight into the transposed layout (the forward was the persistent kernel: no X16 plane)
        hipLaunchKernelGGL(k_gather16_T, dim3((unsigned)((Np + 63) / 64), (unsigned)((Din + 63) / 64), (unsigned)T), dim3(256), 0, side, b->idx, N, Np, T, b->F,
                           c.num_types, s->dense16 + h->off_Wt, s->We16, s->dense16 + h->off_Wr, c.dt, c.de, c.dr, s->XT16, (int64_t)T * Np);
        HIP_TRY(hipGetLastError());
      } else transpose_steps(strm, (l == 0) ? s->X16 : s->H16 + (int64_t)(l - 1) * TN * H, s->XT16, T, N, Np, Din);      // in^T [Din][T][Np]
      if (T > 1 && s->act_frag && l == 0 && s->sv.HsF && s->sv.NW == 8 && (H % 64) == 0) {   // h^T straight from the persistent forward's fragment-order records (steps 0 .. T-2)
        hipLaunchKernelGGL(k_hfrag_T, dim3((unsigned)((s->sv.NU + 1) / 2), (unsigned)(H / 64), (unsigned)(T - 1)), dim3(256), 0, side, (const bf16x4*)s->sv.HsF, s->HT16,
                           (int64_t)s->sv.NU, (int64_t)s->sv.step_recs, N, Np, (int64_t)T * Np, H);
        HIP_TRY(hipGetLastError());
      } else if (T > 1) {
        // (the persistent forward writes no row-major h plane: its records are the only copy, and k_hfrag_T above is their only reader)
        KPRN_REQUIRE(!(s->act_frag && l == 0), KPRN_E_ARG, "bf16 backward: h^T of a persistent forward needs its fragment-order records (NW = 8, H a multiple of 64)");
        transpose_steps(strm, hs, s->HT16, T, N, Np, H);                                                        // h^T  [H][T][Np]
      }
    }
    if (overlap) {
      HIP_TRY(hipEventRecord(s->ev_operands, side));
      // dx first: the table gradients (side stream) then run beside the two dW products
      {
        ProfScope ps(h, "gemm_i2g_bwd_dx");   // dx [T N][Din] = dA W_i2g
        if (dx_t) {   // (the BPTT launch wrote no row-major dA: there is nothing to fall back to)
          const bool ran = gemm16xt(strm, s->zero, s->dAT16, TNp, wt, G4, w.dIn, Din, TNp, Din, G4, Np, N);
          KPRN_REQUIRE(ran, KPRN_E_ARG, "bf16 backward: the transposed-dA dx product does not cover this shape (dx_from_transposed_ok said it would)");
        } else gemm16(strm, go, s->zero, s->dA16, G4, wt, G4, w.dIn, Din, TN, Din, G4, false, nullptr, 1);
      }
      HIP_TRY(hipEventRecord(s->ev_dx, strm));
      HIP_TRY(hipStreamWaitEvent(side, s->ev_dx, 0));
      HIP_TRY(hipStreamWaitEvent(strm, s->ev_operands, 0));
    }
    const int split = (int)std::min<int64_t>(1024, std::max<int64_t>(1, TN / 4096));
    {
      ProfScope ps(h, "gemm_i2g_bwd_dw");   // gW_i2g [4H][Din] += dA^T in
      gemm16(strm, go, s->zero, s->dAT16, TNp, s->XT16, TNp, gd + h->layer[l].Wi, Din, G4, Din, TNp, true, nullptr, split);
    }
    if (T > 1) {
      ProfScope ps(h, "gemm_o2g_bwd_dw");   // gW_o2g [4H][H] += dA[1..T-1]^T h[0..T-2]
      gemm16(strm, go, s->zero, s->dAT16 + Np, TNp, s->HT16, TNp, gd + h->layer[l].Wo, H, G4, H, (int64_t)(T - 1) * Np, true, nullptr, split);
    }
    if (!(s->act_frag && l == 0 && s->bias_in_gates)) {   // (else the fragment-order gate backward summed the bias gradient as it produced dA)
      ProfScope ps(h, "bias_colsum");
      hipLaunchKernelGGL(k_rowsum16, dim3((unsigned)G4), dim3(256), 0, strm, s->dAT16, TNp, gd + h->layer[l].bi);
      HIP_TRY(hipGetLastError());
    }
    if (!overlap) {
      ProfScope ps(h, "gemm_i2g_bwd_dx");   // dx [T N][Din] = dA W_i2g
      if (dx_t) {
        const bool ran = gemm16xt(strm, s->zero, s->dAT16, TNp, wt, G4, w.dIn, Din, TNp, Din, G4, Np, N);
        KPRN_REQUIRE(ran, KPRN_E_ARG, "bf16 backward: the transposed-dA dx product does not cover this shape (dx_from_transposed_ok said it would)");
      } else gemm16(strm, go, s->zero, s->dA16, G4, wt, G4, w.dIn, Din, TN, Din, G4, false, nullptr, 1);
    }
  }
  // (with the side stream these were queued behind ev_dx, i.e. they run beside the dW products issued above)
  {
    ProfScope ps(h, "embed_scatter", side);
    const bool have_index = b->key_sorted != nullptr && !b->tile_k;
    kk::embed_scatter(side, b->idx, N, T, b->F, c.num_types, w.dIn, c.dt, c.de, c.dr, c.Vt, c.Vr, gd + h->off_Wt, h->g_We, gd + h->off_Wr, have_index);
  }
  if (b->key_sorted != nullptr && !b->tile_k) {
    ProfScope ps(h, "entity_grad", side);
    bidx::entity_grad(side, w.dIn, /*frag_order=*/0, b->key_sorted, b->pos_sorted, b->n_index, N, T, D, c.dt, c.de, c.Ve, h->g_We);
  }
  if (overlap) {
    HIP_TRY(hipEventRecord(s->ev_join, side));
    HIP_TRY(hipStreamWaitEvent(strm, s->ev_join, 0));
    side_guard.joined = true;
  }
}

}  // namespace bf16p
