// nn.Dropout(p) on the rnn cell's step input (OneModel.lua:246-265: MaskZero(Sequential(ParallelTable(Sequential(Dropout(p), i2h), h2h), CAddTable, act), 1)
// inside nn.Recurrence, one such module per layer): y = x (.) m / (1 - p), m ~ Bernoulli(1 - p), independent per (layer, step, path, element); the recurrent
// input is never dropped.  Nothing stores a mask: every kernel here regenerates it from (seed, draw, layer, step, path, element) with Philox4x32-10
// (philox_dev.h), one call per 4-element quad.  The host twin kprn_host_dropout_keep states the same rule without a GPU.
#include "kprn_internal.h"

namespace {

constexpr int TPB = 256;
#define CHECK_LAUNCH() HIP_TRY(hipGetLastError())

// keep / drop VEC consecutive elements whose words start at r[p]
template <int VEC, typename VF>
__device__ __forceinline__ VF drop_apply(VF v, const uint32_t (&r)[4], int p, const philox::DropArgs& a) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) v[e] = (r[p + e] >= a.thr) ? v[e] * a.scale : 0.f;
  return v;
}

// kk::embed_gather's k_embed_rows with the layer-0 dropout in the same pass: one wave per (n, t) row, time-major output, the DROPPED row goes to X and
// MaskZero's flag is taken from the UNDROPPED values (MaskZero wraps the whole module, dropout included).  A lane owns whole quads (elements 4q .. 4q+3 =
// one Philox call) and moves them in VEC-wide pieces: every slice width is a multiple of VEC, so a piece never straddles two tables, a quad may; the last
// quad of a row whose width is no multiple of 4 is partial.  grid = (ceil(N / 4), T): no division anywhere.
template <int VEC>
__global__ void k_embed_rows_drop(const int32_t* __restrict__ idx, int64_t N, int T, int F, int nT, const float* __restrict__ Wt,
                                  const float* __restrict__ We, const float* __restrict__ Wr, int dt, int de, int dr, float* __restrict__ X,
                                  float* __restrict__ mask, philox::DropArgs a) {
  typedef float vf __attribute__((ext_vector_type(VEC)));
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  const int t = blockIdx.y;
  if (n >= N) return;
  const int32_t* f = idx + (n * T + t) * F;
  const int64_t orow = (int64_t)t * N + n;
  const int D = dt + de + dr;
  float* dst = X + orow * D;
  const float* we = We + (int64_t)(f[F - 2] - 1) * de;
  const float* wr = Wr + (int64_t)(f[F - 1] - 1) * dr;
  const float* wt0 = Wt + (int64_t)(f[F - nT - 2] - 1) * dt;
  const int Q = (D + 3) >> 2;
  int nz = 0;
  for (int q = lane; q < Q; q += 64) {
    uint32_t r[4];
    philox::quad_words(a, (uint32_t)q, (uint32_t)n, (uint32_t)t, r);
#pragma unroll
    for (int p = 0; p < 4; p += VEC) {
      const int j = 4 * q + p;
      if (j < D) {   // (D % VEC == 0: the whole piece is inside the row)
        vf v;
        if (j < dt) {
          v = *(const vf*)(wt0 + j);
          for (int k = 1; k < nT; ++k) v = v + *(const vf*)(Wt + (int64_t)(f[F - nT - 2 + k] - 1) * dt + j);
        } else if (j < dt + de) {
          v = *(const vf*)(we + (j - dt));
        } else {
          v = *(const vf*)(wr + (j - dt - de));
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) nz |= (v[e] != 0.f) ? 1 : 0;
        *(vf*)(dst + j) = drop_apply<VEC>(v, r, p, a);
      }
    }
  }
  if (mask) {
    nz = __any(nz);
    if (lane == 0) mask[orow] = nz ? 1.f : 0.f;
  }
}

// out[t][n][:] = in[t][n][:] (.) m s over time-major rows of W floats; out may be in (the backward's in-place scaling of dIn: every element is read and
// written by the same lane).  2^lsh lanes per row, a lane owns whole quads; grid = (ceil(N / rows per block), T).
template <int VEC>
__global__ void k_drop_rows(const float* in, float* out, int64_t N, int W, int lsh, philox::DropArgs a) {
  typedef float vf __attribute__((ext_vector_type(VEC)));
  const int64_t n = (int64_t)blockIdx.x * (TPB >> lsh) + (threadIdx.x >> lsh);
  const int t = blockIdx.y;
  if (n >= N) return;
  const int64_t base = ((int64_t)t * N + n) * W;
  const int Q = (W + 3) >> 2;
  for (int q = threadIdx.x & ((1 << lsh) - 1); q < Q; q += (1 << lsh)) {
    uint32_t r[4];
    philox::quad_words(a, (uint32_t)q, (uint32_t)n, (uint32_t)t, r);
#pragma unroll
    for (int p = 0; p < 4; p += VEC) {
      const int j = 4 * q + p;
      if (j < W) *(vf*)(out + base + j) = drop_apply<VEC>(*(const vf*)(in + base + j), r, p, a);
    }
  }
}

}  // namespace

namespace kk {

void embed_gather_drop(hipStream_t s, const int32_t* idx, int64_t N, int T, int F, int nT, const float* Wt, const float* We, const float* Wr, int dt, int de,
                       int dr, float* X, float* mask, const philox::DropArgs& a) {
  if (N <= 0 || T <= 0) return;
  const dim3 grid((unsigned)((N + TPB / 64 - 1) / (TPB / 64)), (unsigned)T);
  const int all = dt | de | dr;
  const uintptr_t pall = (uintptr_t)Wt | (uintptr_t)We | (uintptr_t)Wr | (uintptr_t)X;
  // (the VEC rule of kk::embed_gather)
  if ((all % 4 == 0) && !(pall & 15))
    hipLaunchKernelGGL((k_embed_rows_drop<4>), grid, dim3(TPB), 0, s, idx, N, T, F, nT, Wt, We, Wr, dt, de, dr, X, mask, a);
  else if ((all % 2 == 0) && !(pall & 7))
    hipLaunchKernelGGL((k_embed_rows_drop<2>), grid, dim3(TPB), 0, s, idx, N, T, F, nT, Wt, We, Wr, dt, de, dr, X, mask, a);
  else
    hipLaunchKernelGGL((k_embed_rows_drop<1>), grid, dim3(TPB), 0, s, idx, N, T, F, nT, Wt, We, Wr, dt, de, dr, X, mask, a);
  CHECK_LAUNCH();
}

void drop_rows(hipStream_t s, const float* in, float* out, int64_t N, int T, int W, const philox::DropArgs& a) {
  if (N <= 0 || T <= 0 || W <= 0) return;
  const int Q = (W + 3) >> 2;
  int lsh = 0;
  while (lsh < 6 && (1 << lsh) < Q) ++lsh;   // lanes per row: the power of two that covers the row's quads, a wave at the most
  const int rpb = TPB >> lsh;
  const dim3 grid((unsigned)((N + rpb - 1) / rpb), (unsigned)T);
  const uintptr_t pall = (uintptr_t)in | (uintptr_t)out;
  if ((W % 4 == 0) && !(pall & 15)) hipLaunchKernelGGL((k_drop_rows<4>), grid, dim3(TPB), 0, s, in, out, N, W, lsh, a);
  else if ((W % 2 == 0) && !(pall & 7)) hipLaunchKernelGGL((k_drop_rows<2>), grid, dim3(TPB), 0, s, in, out, N, W, lsh, a);
  else hipLaunchKernelGGL((k_drop_rows<1>), grid, dim3(TPB), 0, s, in, out, N, W, lsh, a);
  CHECK_LAUNCH();
}

}  // namespace kk

// the rule on the host cores (no handle, no GPU): keep [T][N][Din], 1 = kept
extern "C" int kprn_host_dropout_keep(uint64_t seed, unsigned int draw, int32_t layer, int32_t T, int64_t N, int32_t Din, float p, unsigned char* keep) {
  if (!keep || layer < 0 || layer > 65535 || T < 1 || T > 65535 || N < 1 || N >= ((int64_t)1 << 32) || Din < 1 || !(p >= 0.f && p < 1.f)) return KPRN_E_ARG;
  philox::DropArgs a;
  a.k0 = (uint32_t)(seed & 0xffffffffu); a.k1 = (uint32_t)(seed >> 32);
  a.draw = draw; a.layer16 = 65536u * (uint32_t)layer; a.thr = philox::threshold((double)p); a.scale = philox::keep_scale(p);
  const int Q = (Din + 3) >> 2;
  for (int32_t t = 0; t < T; ++t)
    for (int64_t n = 0; n < N; ++n) {
      unsigned char* row = keep + ((int64_t)t * N + n) * Din;
      for (int q = 0; q < Q; ++q) {
        uint32_t r[4];
        philox::quad_words(a, (uint32_t)q, (uint32_t)n, (uint32_t)t, r);
        for (int e = 0; e < 4 && 4 * q + e < Din; ++e) row[4 * q + e] = r[e] >= a.thr ? 1 : 0;
      }
    }
  return KPRN_OK;
}
