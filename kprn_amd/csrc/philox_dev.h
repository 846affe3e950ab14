// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the dropout rule built on it, shared by the kernels of dropout.hip
// and their host twin kprn_host_dropout_keep.  Nothing stores a mask: every (layer, step, path, element) regenerates its word from
//   key = (seed low, seed high), counter = (element / 4, path, step + 65536 * layer, draw), word = element % 4.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KPRN_HD __host__ __device__ __forceinline__
#else
#define KPRN_HD inline
#endif

namespace philox {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;   // round multipliers
constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;   // key increments

KPRN_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// out[0..3] = Philox4x32-10(counter c0..c3, key k0, k1)
KPRN_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = mulhi32(M0, c0), l0 = M0 * c0;
    const uint32_t h1 = mulhi32(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += W0; k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// what a launch needs to regenerate a layer's masks
struct DropArgs {
  uint32_t k0, k1;     // seed & 0xffffffff, seed >> 32
  uint32_t draw;       // training forwards since the seed was set
  uint32_t layer16;    // 65536 * layer
  uint32_t thr;        // kept iff word >= thr; thr = min(2^32 - 1, floor(p 2^32))
  float scale;         // (float)(1 / (1 - p))
};

// the four words of quad q (elements 4q .. 4q+3) of path n at step t
KPRN_HD void quad_words(const DropArgs& a, uint32_t q, uint32_t n, uint32_t t, uint32_t (&r)[4]) {
  philox4x32_10(q, n, t + a.layer16, a.draw, a.k0, a.k1, r);
}

inline uint32_t threshold(double p) {
  const double v = p * 4294967296.0;
  return v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;   // (the cast truncates: floor for p >= 0)
}
inline float keep_scale(float p) { return (float)(1.0 / (1.0 - (double)p)); }

}  // namespace philox
