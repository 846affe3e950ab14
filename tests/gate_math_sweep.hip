// Test helper of tests/test_gpu_gate_math.py: EVERY finite float32 bit pattern through one gate function of the kernels, against the
// double-precision function on the device.  It includes the headers the kernels compile (gate_math.h, lstm_fused_common.h), so what
// it measures is the code the cells run, not a restatement of it.  Built by the test into tests/_build/ (gfx950).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gate_math.h"
#include "lstm_fused_common.h"

namespace {

// exp_fast as it stood before its argument clamp -- kept for one comparison only: which results the clamp changed, and how many
// inputs the unclamped form turned into NaN
__device__ __forceinline__ float exp_fast_unclamped(float x) {
  const float t = x * 1.4426950408889634f;
  const float lo = __builtin_fmaf(x, 1.9259629911e-8f, __builtin_fmaf(x, 1.4426950408889634f, -t));
  const float e = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(e, lo * 0.6931471805599453f, e);
}
__device__ __forceinline__ float sigm_unclamped(float x) { return __builtin_amdgcn_rcpf(1.0f + exp_fast_unclamped(-x)); }
__device__ __forceinline__ float tanh_unclamped(float x) {
  const float t = exp_fast_unclamped(-2.0f * __builtin_fabsf(x));
  return __builtin_copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), x);
}

// function ids (tests/test_gpu_gate_math.py FUNCS): even = a sigmoid, odd = a tanh
enum { F_SIGM = 0, F_TANH = 1, F_SIGM_E2 = 2, F_TANH_E2 = 3, F_FUSED_SIGM = 4, F_FUSED_TANH = 5, F_SIGM_UNCLAMPED = 6, F_TANH_UNCLAMPED = 7, F_N = 8 };

template <int FN> __device__ __forceinline__ float eval(float x) {
  if constexpr (FN == F_SIGM) return sigm(x);
  else if constexpr (FN == F_TANH) return tanh_fast(x);
  else if constexpr (FN == F_SIGM_E2) return sigm_e2(x);
  else if constexpr (FN == F_TANH_E2) return tanh_e2(x);
  else if constexpr (FN == F_FUSED_SIGM) return fused::fast_sigmoid(x);
  else if constexpr (FN == F_FUSED_TANH) return fused::fast_tanh(x);
  else if constexpr (FN == F_SIGM_UNCLAMPED) return sigm_unclamped(x);
  else return tanh_unclamped(x);
}

constexpr int NT = 256, NB = 16384;   // 2^32 patterns / (NT * NB) = 1 024 per thread

struct Part {
  double err;               // largest |f(x) - ref(x)| over the finite results
  uint32_t worst;           // its x (bit pattern; the smallest one on ties)
  uint32_t nonfinite;       // results that are inf / NaN
  uint32_t outside;         // finite results outside [0, 1] (sigmoid) / [-1, 1] (tanh)
  uint32_t changed;         // F_SIGM / F_TANH: results that differ in any bit from the unclamped form where that one is finite
                            // (sigm: x >= -88.72 only -- below, the clamp changes the value by design)
  uint32_t old_nonfinite;   // F_SIGM / F_TANH: inputs for which the unclamped form is inf / NaN
  uint32_t pad;
};

template <int FN>
__global__ __launch_bounds__(NT) void k_sweep(Part* __restrict__ out) {
  constexpr bool SIG = (FN % 2) == 0;
  double err = 0.0;
  uint32_t worst = 0, nonfinite = 0, outside = 0, changed = 0, old_nonfinite = 0;
  const uint64_t n = 1ull << 32, stride = (uint64_t)NT * NB;
  for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) {
    const uint32_t bits = (uint32_t)i;
    if ((bits & 0x7f800000u) == 0x7f800000u) continue;   // inf / NaN arguments: out of scope
    const float x = __uint_as_float(bits);
    const float y = eval<FN>(x);
    if (!isfinite(y)) {
      ++nonfinite;
    } else {
      const double xd = (double)x;
      const double ref = SIG ? 1.0 / (1.0 + exp(-xd)) : tanh(xd);
      const double e = fabs((double)y - ref);
      if (e > err || (e == err && bits < worst)) { err = e; worst = bits; }
      if (SIG ? (y < 0.0f || y > 1.0f) : (y < -1.0f || y > 1.0f)) ++outside;
    }
    if constexpr (FN == F_SIGM || FN == F_TANH) {
      const float o = (FN == F_SIGM) ? sigm_unclamped(x) : tanh_unclamped(x);
      if (!isfinite(o)) ++old_nonfinite;
      else if ((FN == F_TANH || x >= -88.72f) && __float_as_uint(o) != __float_as_uint(y)) ++changed;
    }
  }
  __shared__ double s_err[NT];
  __shared__ uint32_t s_worst[NT], s_cnt[4][NT];
  const int t = threadIdx.x;
  s_err[t] = err; s_worst[t] = worst;
  s_cnt[0][t] = nonfinite; s_cnt[1][t] = outside; s_cnt[2][t] = changed; s_cnt[3][t] = old_nonfinite;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (t < h) {
      if (s_err[t + h] > s_err[t] || (s_err[t + h] == s_err[t] && s_worst[t + h] < s_worst[t])) { s_err[t] = s_err[t + h]; s_worst[t] = s_worst[t + h]; }
      for (int c = 0; c < 4; ++c) s_cnt[c][t] += s_cnt[c][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    Part p;
    p.err = s_err[0]; p.worst = s_worst[0];
    p.nonfinite = s_cnt[0][0]; p.outside = s_cnt[1][0]; p.changed = s_cnt[2][0]; p.old_nonfinite = s_cnt[3][0]; p.pad = 0;
    out[blockIdx.x] = p;
  }
}

template <int FN> void launch(Part* d) { k_sweep<FN><<<NB, NT>>>(d); }

}  // namespace

// fn: one of the ids above.  res[0] = max abs error, res[1] = its x (as a float), counts[0..3] = nonfinite, outside, changed, old_nonfinite.
// Returns 0, or the HIP error code.
extern "C" int gate_sweep(int fn, double* res, unsigned long long* counts) {
  if (fn < 0 || fn >= F_N) return -1;
  Part* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, sizeof(Part) * NB);
  if (e != hipSuccess) return (int)e;
  typedef void (*L)(Part*);
  static const L fns[F_N] = {launch<0>, launch<1>, launch<2>, launch<3>, launch<4>, launch<5>, launch<6>, launch<7>};
  fns[fn](d);
  e = hipGetLastError();
  Part* h = new Part[NB];
  if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(Part) * NB, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e == hipSuccess) {
    double err = 0.0;
    uint32_t worst = 0;
    unsigned long long c[4] = {0, 0, 0, 0};
    for (int b = 0; b < NB; ++b) {
      if (h[b].err > err || (h[b].err == err && h[b].worst < worst)) { err = h[b].err; worst = h[b].worst; }
      c[0] += h[b].nonfinite; c[1] += h[b].outside; c[2] += h[b].changed; c[3] += h[b].old_nonfinite;
    }
    float wx;
    memcpy(&wx, &worst, 4);
    res[0] = err;
    res[1] = (double)wx;
    for (int k = 0; k < 4; ++k) counts[k] = c[k];
  }
  delete[] h;
  return (int)e;
}
