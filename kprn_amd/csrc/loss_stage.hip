// Pooling and the loss stage of the path-scoring engine (gfx950): what every scoring pass and every training step does with the score matrix
// S [paths][C] once the head has written it.  Citations are to the reference's modules (release/songPathRnn/ of the reference).
//
// The stages that run, in order:
//   1  the reducer over a pair's paths for the selected class + nn.Sigmoid + nn.Select(2, classId)   (OneModel.lua:284-294, MyOptimizer.lua:126);
//      reduce_dev.h is the one definition of the reducer (shared with explain_paths.hip)
//   2  nn.BCECriterion forward and backward on that probability                                      (MyOptimizer.lua:193-195)
//   3  back through the sigmoid and the reducer: dS[n] = d loss / d S[n][classId] for every path n of the pair; on the fused path through
//      slot_of (the pair's q-th gradient goes to dS[slot_of[n0 + q]], the tile slot of the path)
//   4  the per-workgroup partial of the loss: the workgroup's pairs in index order, one plain store; k_sum_partials adds the partials in
//      index order when the loss is asked for (reproducible: no atomics anywhere in this file)
//   5  two passenger jobs in extra workgroups of the same launch: the fused backward's weight transposes (kk::TransposeJob) and the pooling
//      stage of a scoring pass that rode in the training forward's launch (kk::PoolJob, "score_dual")
//   2' the pairwise (BPR) loss over groups of pairs instead of stage 2 (option "loss" = "bpr"; include/kprn.h "pairwise loss"): k_loss_stage_pairwise, a
//      workgroup per group, with the same stages 1, 3, 4 and 5 around it
//   ig the LogSumExp reducer's inverse pooling temperature (option "pool_gamma", include/kprn.h "pooling temperature"): a float argument of every kernel here,
//      handed down to reduce_dev.h's lse_term / lse_finish / pool_sigmoid_of and to stage 3, where dy is scaled by it once per pair.  One set of instantiations: at
//      ig == 1.0f every product is exact and the bits are those of the plain reducer.  Max and TopK + Mean never read it.  VGPRs now / before the option
//      (no scratch anywhere, occupancy as before): k_pool 14 / 17 / 24 / 28 (13 / 16 / 24 / 28), k_loss_stage 34 and 49 (32 and 44), k_loss_stage_pairwise
//      37 and 50 (37 and 48) -- the growth is exp_shared / log_shared, the temperature path's own exp and log (reduce_dev.h).
// (The head's weight gradient is NOT formed here: the fused top-layer backward or the generic pipeline's head_bwd does that.)
//
//   6  Two forms.  A batch is kk::Segs: B pairs of P paths each, or (off != null, a ragged batch -- an extension, the reference has one path
//      count per batch) pair b = paths off[b] .. off[b+1]-1.  Thread form: a thread per pair, reduce_col / bce_pair.  Wave form: a wave per
//      pair, lanes stride the segment, then a butterfly over the 64 lanes (every lane ends with the same bits: no broadcast, no LDS); a pair of
//      at most RAGGED_THREAD_MAX paths still takes reduce_col's order there, so equal short counts give the rectangular batch's bits either
//      way.  The batch chooses once, when it is made (kk::ragged_plan: wave = some pair is longer than RAGGED_THREAD_MAX); a rectangular
//      batch is always the thread form.  SEG = false instantiations know no offsets, no workgroup table and no wave form: they are what a
//      batch without a ragged participant launches.  The launchers choose SEG from off.
#include <string.h>
#include "kprn_internal.h"
#include "reduce_dev.h"

namespace {

constexpr int TPB = 256;
constexpr int PPW = kk::RAGGED_WG_PAIRS;   // pairs per workgroup of the loss stage: small on purpose (latency-bound: many workgroups in flight)
static_assert(kk::RAGGED_WG_PATHS == PPW * kk::RAGGED_THREAD_MAX, "the ragged cut restates the rectangular one");
inline unsigned nblocks(int64_t n, int per = TPB) { return (unsigned)((n + per - 1) / per); }

// ---------------------------------------------------------------------------------------
// Stage 1 for one (pair b, class c): reduce the pair's column, sigmoid, store.  pooled != null: every class is asked (pooled / probs [B][C], at = b C + c);
// sel / sel_host (page-locked mirror: kprn_forward_batch hands the probabilities out without a copy operation) take class cid.
// Wave form (SEG and wave): the whole wave calls, lane 0 stores.  (b is 64 bits wide and the rectangular form multiplies it out itself: the every-class
// instantiations took 16 and 28 registers that way and 17 and 30 through an int; with the temperature path's exp and log they take 17 and 28.)
template <bool SEG>
__device__ __forceinline__ void pool_pair(const float* __restrict__ S, const int32_t* __restrict__ off, int P, int wave, int lane, int64_t b, int c, int C,
                                          int reducer, int K, float ig, float* __restrict__ pooled, float* __restrict__ probs, int64_t at, int cid,
                                          float* __restrict__ sel, float* __restrict__ sel_host) {
  if constexpr (!SEG) off = nullptr;
  const float* s = S + (SEG ? seg_begin(off, P, (int)b) : b * P) * C + c;
  const int cnt = seg_count(off, P, (int)b);
  const float y = SEG ? reduce_seg(s, cnt, C, reducer, K, ig, wave, lane) : reduce_col(s, cnt, C, reducer, K, ig);
  const float pr = pool_sigmoid_of(y, ig);
  if (SEG && wave && lane != 0) return;
  if (pooled) { pooled[at] = y; probs[at] = pr; }
  if (c == cid) {
    if (sel) sel[b] = pr;
    if (sel_host) sel_host[b] = pr;
  }
}

// The pooling stage of a scoring pass.  EVERY_CLASS: an item is a (pair, class), else a pair (only the selected class is reduced: what
// model:forward hands the caller, test_from_checkpoint.lua:82).  Thread form: one thread per item; wave form: one wave per item, four to a workgroup.
template <bool SEG, bool EVERY_CLASS>
__global__ __launch_bounds__(TPB) void k_pool(const float* __restrict__ S, kk::Segs g, int C, int reducer, int K, float ig, float* __restrict__ pooled,
                                              float* __restrict__ probs, int cid, float* __restrict__ sel, float* __restrict__ sel_host) {
  const bool wave = SEG && g.wave;
  const int64_t item = wave ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= (EVERY_CLASS ? (int64_t)g.B * C : (int64_t)g.B)) return;   // (wave form: the whole wave leaves)
  const int64_t b = EVERY_CLASS ? item / C : item;
  pool_pair<SEG>(S, g.off, g.P, g.wave, threadIdx.x & 63, b, EVERY_CLASS ? (int)(item % C) : cid, C, reducer, K, ig, EVERY_CLASS ? pooled : nullptr, probs,
                 item, cid, sel, sel_host);
}

// ---------------------------------------------------------------------------------------
// Stage 2: nn.BCECriterion on one pair's probability p against its target t.  *lossterm = the pair's term of the loss; returns
// dy = d loss / d (pooled value), i.e. already back through the sigmoid.  literal: the criterion's own gradient formula and the sigmoid's, multiplied
// out as the reference does; else their closed form (p - t).
__device__ __forceinline__ float bce(float p, float t, int literal, float invB, float* lossterm) {
  const float eps = 1e-12f;
  *lossterm = -(t * logf(p + eps) + (1.f - t) * logf(1.f - p + eps)) * invB;
  if (!literal) return (p - t) * invB;
  const float dp = -(t - p) / ((1.f - p + eps) * (p + eps)) * invB;
  return dp * p * (1.f - p);
}

// where a pair's gradients go: d(q) = d loss / d s[q]; slot (nullable): to dS[slot[q]] instead (fused path: tile slot of the path)
struct PairGrad {
  float* __restrict__ dpair; float* __restrict__ dS; const int32_t* __restrict__ slot;
  __device__ __forceinline__ float& operator()(int q) const { return slot ? dS[slot[q]] : dpair[q]; }
};

// Stage 3 for one pair by one thread: back through the reducer given dy = d loss / d (pooled value).  LogSumExp under the pooling temperature:
// d pooled / d s_q = ig x the path's share, so dy is scaled once per pair and the per-path expression keeps its shape (dy * 1.0f == dy).
__device__ void reducer_bwd(const float* __restrict__ s, int P, int C, int reducer, int K, float ig, float dy, PairGrad d) {
  if (reducer == 2) {
    dy *= ig;
    float m = s[0];
    for (int q = 1; q < P; ++q) m = fmaxf(m, s[(int64_t)q * C]);
    float sum = 0.f;
    for (int q = 0; q < P; ++q) sum += lse_term(s[(int64_t)q * C], m, ig);
    for (int q = 0; q < P; ++q) d(q) = lse_term(s[(int64_t)q * C], m, ig) / sum * dy;
  } else if (reducer == 0) {
    int arg = 0;
    for (int q = 1; q < P; ++q) if (s[(int64_t)q * C] > s[(int64_t)arg * C]) arg = q;
    for (int q = 0; q < P; ++q) d(q) = (q == arg) ? dy : 0.f;
  } else {
    int kk = K < P ? K : P;
    for (int q = 0; q < P; ++q) d(q) = 0.f;
    float last_v = INFINITY; int last_i = -1;
    for (int r = 0; r < kk; ++r) {
      float best = -INFINITY; int bi = -1;
      for (int q = 0; q < P; ++q) {
        float v = s[(int64_t)q * C];
        bool after = (v < last_v) || (v == last_v && q > last_i);
        if (after && (bi < 0 || v > best)) { best = v; bi = q; }
      }
      d(bi) = dy / (float)kk; last_v = best; last_i = bi;
    }
  }
}

// Stages 1-3 for one pair by one thread; returns the probability
__device__ float bce_pair(const float* __restrict__ s, int P, int C, int reducer, int K, float ig, int literal, float invB, float t, PairGrad d,
                          float* lossterm) {
  const float p = pool_sigmoid_of(reduce_col(s, P, C, reducer, K, ig), ig);
  reducer_bwd(s, P, C, reducer, K, ig, bce(p, t, literal, invB, lossterm), d);
  return p;
}

// Stage 3 by one wave (cnt > RAGGED_THREAD_MAX; the whole wave calls, under wave-uniform control flow).  Path q's gradient is written by lane q % 64 only,
// so the TopK form's zero-then-set is one thread's program order.
__device__ void reducer_bwd_wave(const float* __restrict__ s, int cnt, int C, int reducer, int K, float ig, float dy, PairGrad d, int lane) {
  if (reducer == 2) {
    dy *= ig;
    float m = -INFINITY;
    for (int q = lane; q < cnt; q += 64) m = fmaxf(m, s[(int64_t)q * C]);
    m = wave_all_max(m);
    float sum = 0.f;
    for (int q = lane; q < cnt; q += 64) sum += lse_term(s[(int64_t)q * C], m, ig);
    sum = wave_all_sum(sum);
    for (int q = lane; q < cnt; q += 64) d(q) = lse_term(s[(int64_t)q * C], m, ig) / sum * dy;
  } else if (reducer == 0) {
    float best; int arg;
    lane_best(s, cnt, C, lane, INFINITY, -1, best, arg);
    wave_all_best(best, arg);
    for (int q = lane; q < cnt; q += 64) d(q) = (q == arg) ? dy : 0.f;
  } else {
    const int kk = K < cnt ? K : cnt;
    for (int q = lane; q < cnt; q += 64) d(q) = 0.f;
    float last_v = INFINITY; int last_i = -1;
    for (int r = 0; r < kk; ++r) {
      float best; int bi;
      lane_best(s, cnt, C, lane, last_v, last_i, best, bi);
      wave_all_best(best, bi);
      if ((bi & 63) == lane) d(bi) = dy / (float)kk;
      last_v = best; last_i = bi;
    }
  }
}

// Stages 1-3 for one pair by one wave
__device__ float bce_pair_wave(const float* __restrict__ s, int cnt, int C, int reducer, int K, float ig, int literal, float invB, float t, PairGrad d,
                               float* lossterm, int lane) {
  const float p = pool_sigmoid_of(reduce_col_wave(s, cnt, C, reducer, K, ig, lane), ig);
  reducer_bwd_wave(s, cnt, C, reducer, K, ig, bce(p, t, literal, invB, lossterm), d, lane);
  return p;
}

// ---------------------------------------------------------------------------------------
// Stage 5, the passengers: workgroup rb of the pooling job (k_pool<SEG, false>'s items of pj's batch, under the launch's ig: a pass that rides in a training
// launch pools under the same temperature) / of the transposes (64 workgroups per 256x64 matrix)
template <bool SEG>
__device__ __forceinline__ void pool_passenger(int rb, int tid, int C, int reducer, int K, float ig, const kk::PoolJob& pj) {
  const int b = (SEG && pj.wave) ? rb * 4 + (tid >> 6) : rb * 256 + tid;
  if (b >= pj.B) return;
  pool_pair<SEG>(pj.S, pj.off, pj.P, pj.wave, tid & 63, b, pj.cid, C, reducer, K, ig, nullptr, nullptr, 0, pj.cid, pj.sel, pj.sel_host);
}
__device__ __forceinline__ void transpose_passenger(int rb, int tid, const kk::TransposeJob& tj) {
  const int m = rb >> 6, i = (rb & 63) * 256 + tid;  // over the 64*256 outputs of matrix m
  tj.WT[m][i] = tj.W[m][(i & 255) * 64 + (i >> 8)];
}

// ---------------------------------------------------------------------------------------
// The loss stage of a training step in one launch (was four: pool, select, bce, sum).  Workgroups [0, n_loss_blocks) do stages 1-4 for at most
// PPW pairs each: the pairs PPW w .. of workgroup w, or (g.wg != null, a ragged batch) wg[w] .. wg[w+1]-1, which kk::ragged_plan cut.  The
// workgroups behind them are the passengers.  SEG = true also serves a rectangular batch that carries a ragged passenger, and the reverse.
template <bool SEG>
__global__ __launch_bounds__(256) void k_loss_stage(const float* __restrict__ S, const float* __restrict__ labels, kk::Segs g, int C, int cid, int reducer, int K,
                                                    float ig, int literal, float invB, float* __restrict__ sel, float* __restrict__ dS,
                                                    const int32_t* __restrict__ slot_of, float* __restrict__ partial, int n_loss_blocks, kk::TransposeJob tj,
                                                    float* __restrict__ partial_host, kk::PoolJob pj) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if ((int)blockIdx.x >= n_loss_blocks + 64 * tj.n) {  // (workgroup-uniform) passenger: the pooling stage of a scoring pass
    pool_passenger<SEG>((int)blockIdx.x - n_loss_blocks - 64 * tj.n, tid, C, reducer, K, ig, pj);
    return;
  }
  if ((int)blockIdx.x >= n_loss_blocks) {  // (workgroup-uniform) passenger: 256x64 weight transposes
    transpose_passenger((int)blockIdx.x - n_loss_blocks, tid, tj);
    return;
  }
  __shared__ float lossw[PPW];
  const int32_t* off = SEG ? g.off : nullptr;
  const int32_t* wg = SEG ? g.wg : nullptr;
  const bool wave = SEG && g.wave;
  const int b0 = wg ? wg[blockIdx.x] : (int)blockIdx.x * PPW;
  const int nb = wg ? wg[blockIdx.x + 1] - b0 : ((g.B - b0 < PPW) ? (g.B - b0) : PPW);
  // 1-3: pair b0 + i belongs to thread i (thread form) or to wave i % 4 (wave form, wave-uniform); every slot of lossw is written once
  for (int i = wave ? wv : tid; i < PPW; i += wave ? 4 : 256) {
    float lt = 0.f;
    if (i < nb) {
      const int b = b0 + i;
      const int64_t n0 = seg_begin(off, g.P, b);
      const int cnt = seg_count(off, g.P, b);
      const PairGrad d{dS + n0, dS, slot_of ? slot_of + n0 : nullptr};
      float pr = 0.f;
      if (wave && cnt > kk::RAGGED_THREAD_MAX) pr = bce_pair_wave(S + n0 * C + cid, cnt, C, reducer, K, ig, literal, invB, labels[b], d, &lt, lane);
      else if (!wave || lane == 0) pr = bce_pair(S + n0 * C + cid, cnt, C, reducer, K, ig, literal, invB, labels[b], d, &lt);
      if (!wave || lane == 0) sel[b] = pr;
    }
    if (!wave || lane == 0) lossw[i] = lt;
  }
  __syncthreads();
  // 4 (a last-workgroup reduction here needs a device-scope release per workgroup = an L2 write-back each: measured 30 us)
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < PPW; ++i) s += lossw[i];
    partial[blockIdx.x] = s;
    if (partial_host) partial_host[blockIdx.x] = s;   // page-locked mirror: the host adds the partials itself (kprn_train_step's early loss)
  }
}

// ---------------------------------------------------------------------------------------
// Stage 2': the pairwise loss (include/kprn.h "pairwise loss"), the one statement of its fp32 formula for the kernel and for kprn_host_pairwise_loss.
__host__ __device__ inline float softplusf_(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
// A running fp32 sum with Kahan's compensation: a member of a full group adds 1023 addends, and a plain running sum of that many loses a few 1e-7 of the
// result -- the size of the bar the rule is tested at.  (No product anywhere in add: nothing for the compiler to contract.)
struct KahanSum {
  float sum = 0.f, comp = 0.f;
  __host__ __device__ inline void add(float x) { const float v = x - comp; const float t = sum + v; comp = (t - sum) - v; sum = t; }
};
// Member i of a group of n pairs with pooled values y and label bits pos: *dy = d loss / d y[i] over its partners in ascending index, *term = the sum of its
// loss terms (a positive's; unscaled).  A member without a partner gets +0.0f twice.
__host__ __device__ inline void pairwise_member(const float* y, const unsigned char* pos, int n, int i, float s, float* dy, float* term) {
  const float yi = y[i];
  KahanSum sg, lt;
  int partners = 0;
  if (pos[i]) {
    for (int j = 0; j < n; ++j)
      if (!pos[j]) { sg.add(1.0f / (1.0f + expf(yi - y[j]))); lt.add(softplusf_(y[j] - yi)); ++partners; }
    *dy = partners ? -s * sg.sum : 0.f;
  } else {
    for (int j = 0; j < n; ++j)
      if (pos[j]) { sg.add(1.0f / (1.0f + expf(y[j] - yi))); ++partners; }
    *dy = partners ? s * sg.sum : 0.f;
  }
  *term = lt.sum;
}

constexpr int PW_MAX = kk::PAIRWISE_MAX_GROUP;
static_assert(PW_MAX == KPRN_PAIRWISE_MAX_GROUP, "the header states the limit");

// The loss stage under option "loss" = "bpr" in one launch: workgroup w < G does stages 1, 2', 3 and 4 for group w = the pairs go[w] .. go[w+1]-1 (at most
// PW_MAX: kprn_batch_set_groups has checked the table); the workgroups behind them are k_loss_stage's passengers.  A pair takes the reducer form the BCE stage
// gives it: a thread, or (a ragged batch in wave form, more than RAGGED_THREAD_MAX paths) a wave -- so sel and the pooled values have that stage's bits.
// Every pair's dS entries are written, zeros where the pair has no term.  s: the scale of the rule (0 when the batch has no term).
// LDS: y, dy and the members' term sums, 3 x 4 KiB, and the label bits, 1 KiB.
template <bool SEG>
__global__ __launch_bounds__(256) void k_loss_stage_pairwise(const float* __restrict__ S, const float* __restrict__ labels, kk::Segs g, const int32_t* __restrict__ go,
                                                             int G, int C, int cid, int reducer, int K, float ig, float s, float* __restrict__ sel, float* __restrict__ dS,
                                                             const int32_t* __restrict__ slot_of, float* __restrict__ partial, kk::TransposeJob tj,
                                                             float* __restrict__ partial_host, kk::PoolJob pj) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if ((int)blockIdx.x >= G + 64 * tj.n) {  // (workgroup-uniform)
    pool_passenger<SEG>((int)blockIdx.x - G - 64 * tj.n, tid, C, reducer, K, ig, pj);
    return;
  }
  if ((int)blockIdx.x >= G) {  // (workgroup-uniform)
    transpose_passenger((int)blockIdx.x - G, tid, tj);
    return;
  }
  __shared__ float y_s[PW_MAX], dy_s[PW_MAX], term_s[PW_MAX];
  __shared__ unsigned char pos_s[PW_MAX];
  const int32_t* off = SEG ? g.off : nullptr;
  const bool wave = SEG && g.wave;
  const int b0 = go[blockIdx.x], n = go[blockIdx.x + 1] - b0;
  // 1: member i belongs to thread i % 256, or (wave form, a long pair) to wave i % 4 (i and the pair's count are wave-uniform there)
  for (int i = tid; i < n; i += 256) {
    const int b = b0 + i;
    const int cnt = seg_count(off, g.P, b);
    pos_s[i] = labels[b] > 0.5f ? 1 : 0;
    if (wave && cnt > kk::RAGGED_THREAD_MAX) continue;
    const float y = reduce_col(S + seg_begin(off, g.P, b) * C + cid, cnt, C, reducer, K, ig);
    y_s[i] = y;
    sel[b] = pool_sigmoid_of(y, ig);
  }
  if (wave) {
    for (int i = wv; i < n; i += 4) {
      const int b = b0 + i;
      const int cnt = seg_count(off, g.P, b);
      if (cnt <= kk::RAGGED_THREAD_MAX) continue;
      const float y = reduce_col_wave(S + seg_begin(off, g.P, b) * C + cid, cnt, C, reducer, K, ig, lane);
      if (lane == 0) { y_s[i] = y; sel[b] = pool_sigmoid_of(y, ig); }
    }
  }
  __syncthreads();
  // 2'
  for (int i = tid; i < n; i += 256) {
    float dy, lt;
    pairwise_member(y_s, pos_s, n, i, s, &dy, &lt);
    dy_s[i] = dy; term_s[i] = lt;
  }
  __syncthreads();
  // 4: the group's terms in index order, scaled once
  if (tid == 0) {
    KahanSum acc;
    for (int i = 0; i < n; ++i) acc.add(term_s[i]);
    const float a = acc.sum * s;
    partial[blockIdx.x] = a;
    if (partial_host) partial_host[blockIdx.x] = a;
  }
  // 3: the split of 1
  for (int i = tid; i < n; i += 256) {
    const int b = b0 + i;
    const int cnt = seg_count(off, g.P, b);
    if (wave && cnt > kk::RAGGED_THREAD_MAX) continue;
    const int64_t n0 = seg_begin(off, g.P, b);
    reducer_bwd(S + n0 * C + cid, cnt, C, reducer, K, ig, dy_s[i], PairGrad{dS + n0, dS, slot_of ? slot_of + n0 : nullptr});
  }
  if (wave) {
    for (int i = wv; i < n; i += 4) {
      const int b = b0 + i;
      const int cnt = seg_count(off, g.P, b);
      if (cnt <= kk::RAGGED_THREAD_MAX) continue;
      const int64_t n0 = seg_begin(off, g.P, b);
      reducer_bwd_wave(S + n0 * C + cid, cnt, C, reducer, K, ig, dy_s[i], PairGrad{dS + n0, dS, slot_of ? slot_of + n0 : nullptr}, lane);
    }
  }
}

// n_terms of a group table: positives x negatives of every group, in integers (one workgroup; thread t takes the groups t, t + 256, ...)
__global__ __launch_bounds__(256) void k_count_pair_terms(const float* __restrict__ labels, const int32_t* __restrict__ go, int G, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long acc[256];
  unsigned long long a = 0;
  for (int w = threadIdx.x; w < G; w += 256) {
    unsigned long long np = 0, nn = 0;
    for (int b = go[w]; b < go[w + 1]; ++b) { if (labels[b] > 0.5f) ++np; else ++nn; }
    a += np * nn;
  }
  acc[threadIdx.x] = a;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) acc[threadIdx.x] += acc[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = acc[0];
}

// loss = fixed-order sum of the per-workgroup partials (reproducible)
__global__ void k_sum_partials(const float* __restrict__ partial, int n, float* __restrict__ out, int accumulate) {
  __shared__ float pl[256];
  float s = 0.f;
  for (int base = 0; base < n; base += 256) {
    const int i = base + (int)threadIdx.x;
    pl[threadIdx.x] = (i < n) ? partial[i] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = (n - base < 256) ? (n - base) : 256;
      for (int k = 0; k < m; ++k) s += pl[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = s;
    if (accumulate) { out[1] += s; out[2] += 1.0f; }   // running sum / count of the losses since the last kprn_read_loss_sum
  }
}

}  // namespace

#define CHECK_LAUNCH() HIP_TRY(hipGetLastError())

namespace kk {

void pool_sigmoid(hipStream_t s, const float* S, const Segs& g, int C, int reducer, int K, float ig, float* pooled, float* probs, int cid, float* sel,
                  float* sel_host) {
  if (g.B <= 0) return;
  const int64_t items = pooled ? (int64_t)g.B * C : (int64_t)g.B;
  auto* const k = g.off ? (pooled ? k_pool<true, true> : k_pool<true, false>) : (pooled ? k_pool<false, true> : k_pool<false, false>);
  hipLaunchKernelGGL(k, dim3(nblocks(items, g.off && g.wave ? 4 : TPB)), dim3(TPB), 0, s, S, g, C, reducer, K, ig, pooled, probs, cid, sel, sel_host);
  CHECK_LAUNCH();
}

int loss_partials(int B) { return (B + PPW - 1) / PPW; }

int loss_stage(hipStream_t s, const float* S, const float* labels, const Segs& g, int C, int cid, int reducer, int K, float ig, int literal, float invB,
               float* sel, float* dS, const int32_t* slot_of, float* partial, const TransposeJob* tj, float* partial_host, const PoolJob* pj) {
  if (g.B <= 0) return 0;
  TransposeJob t;
  memset(&t, 0, sizeof(t));
  if (tj) t = *tj;
  PoolJob pjob;
  memset(&pjob, 0, sizeof(pjob));
  if (pj) pjob = *pj;
  const bool seg = g.off || pjob.off;
  const int nlb = g.wg ? g.n_wg : loss_partials(g.B);
  const int npb = (int)nblocks(pjob.B, seg && pjob.wave ? 4 : 256);
  hipLaunchKernelGGL(seg ? k_loss_stage<true> : k_loss_stage<false>, dim3((unsigned)(nlb + 64 * t.n + npb)), dim3(256), 0, s, S, labels, g, C, cid, reducer, K,
                     ig, literal, invB, sel, dS, slot_of, partial, nlb, t, partial_host, pjob);
  CHECK_LAUNCH();
  return nlb;
}

int loss_stage_pairwise(hipStream_t s, const float* S, const float* labels, const Segs& g, const int32_t* go, int G, int C, int cid, int reducer, int K, float ig,
                        float scale, float* sel, float* dS, const int32_t* slot_of, float* partial, const TransposeJob* tj, float* partial_host, const PoolJob* pj) {
  if (g.B <= 0 || G <= 0) return 0;
  TransposeJob t;
  memset(&t, 0, sizeof(t));
  if (tj) t = *tj;
  PoolJob pjob;
  memset(&pjob, 0, sizeof(pjob));
  if (pj) pjob = *pj;
  const bool seg = g.off || pjob.off;
  const int npb = (int)nblocks(pjob.B, seg && pjob.wave ? 4 : 256);
  hipLaunchKernelGGL(seg ? k_loss_stage_pairwise<true> : k_loss_stage_pairwise<false>, dim3((unsigned)(G + 64 * t.n + npb)), dim3(256), 0, s, S, labels, g, go, G, C,
                     cid, reducer, K, ig, scale, sel, dS, slot_of, partial, t, partial_host, pjob);
  CHECK_LAUNCH();
  return G;
}

void count_pair_terms(hipStream_t s, const float* labels, const int32_t* go, int G, int64_t* out) {
  hipLaunchKernelGGL(k_count_pair_terms, dim3(1), dim3(256), 0, s, labels, go, G, (unsigned long long*)out);
  CHECK_LAUNCH();
}

// a group table over B consecutive pairs: go[0] = 0, go[G] = B, non-decreasing, no group above PAIRWISE_MAX_GROUP (no device, no handle)
const char* pairwise_groups_why(const int32_t* go, int32_t G, int32_t B) {
  if (!go || G < 1 || B < 1) return "group_offsets is NULL, or G or B is below 1";
  if (go[0] != 0) return "group_offsets[0] must be 0";
  for (int32_t w = 0; w < G; ++w) {
    if (go[w + 1] < go[w]) return "group_offsets must not decrease";
    if (go[w + 1] - go[w] > PAIRWISE_MAX_GROUP) return "a group holds more than 1024 pairs (KPRN_PAIRWISE_MAX_GROUP)";
  }
  if (go[G] != B) return "group_offsets[G] must be the batch's number of pairs";
  return nullptr;
}

// Offsets, loss-stage workgroup table and the reducer form of a ragged batch (no device, no handle: kprn_host_ragged_plan).  A workgroup takes
// consecutive pairs while it holds fewer than RAGGED_WG_PAIRS pairs and the next pair keeps it within RAGGED_WG_PATHS paths; a pair longer than that
// is a workgroup of its own.  Equal counts <= 28 therefore cut as the rectangular loss stage does (RAGGED_WG_PAIRS pairs each).
bool ragged_plan(const int32_t* counts, int32_t B, int64_t N, int32_t* off, int32_t* wg, int32_t* summary) {
  if (!counts || B <= 0 || N < B || N > 0x7fffffffLL || !off || !wg || !summary) return false;
  int64_t o = 0;
  int32_t mx = 0, nw = 0, wpairs = 0;
  int64_t wpaths = 0;
  for (int32_t b = 0; b < B; ++b) {
    const int32_t c = counts[b];
    if (c < 1 || c > RAGGED_MAX_SEG) return false;
    if (wpairs == 0 || wpairs == RAGGED_WG_PAIRS || wpaths + c > RAGGED_WG_PATHS) { wg[nw++] = b; wpairs = 0; wpaths = 0; }
    ++wpairs; wpaths += c;
    off[b] = (int32_t)o;
    o += c;
    if (o > N) return false;
    if (c > mx) mx = c;
  }
  if (o != N) return false;
  off[B] = (int32_t)o;
  wg[nw] = B;
  summary[0] = nw; summary[1] = mx; summary[2] = mx > RAGGED_THREAD_MAX ? 1 : 0;
  return true;
}

void sum_partials(hipStream_t s, const float* partial, int n, float* out, int accumulate) {
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, s, partial, n, out, accumulate);
  CHECK_LAUNCH();
}

}  // namespace kk

// The pairwise rule on the host cores (no handle, no GPU): pairwise_member per pair, a group's terms added in index order and scaled once, the groups'
// partials added in group order -- the kernel's and k_sum_partials' order.
extern "C" int kprn_host_pairwise_loss(const float* pooled, const float* labels, const int32_t* group_offsets, int32_t G, int32_t B, float inv_batch, float* dy,
                                       float* loss, int64_t* n_terms) {
  if (!pooled || !labels || !dy || !loss || !n_terms || kk::pairwise_groups_why(group_offsets, G, B)) return KPRN_E_ARG;
  try {
    std::vector<unsigned char> pos((size_t)B);
    for (int32_t b = 0; b < B; ++b) pos[b] = labels[b] > 0.5f ? 1 : 0;
    int64_t terms = 0;
    for (int32_t w = 0; w < G; ++w) {
      int64_t np = 0;
      for (int32_t b = group_offsets[w]; b < group_offsets[w + 1]; ++b) np += pos[b];
      terms += np * (group_offsets[w + 1] - group_offsets[w] - np);
    }
    const float s = inv_batch > 0.f ? inv_batch : (terms > 0 ? 1.0f / (float)terms : 0.f);
    float total = 0.f;
    for (int32_t w = 0; w < G; ++w) {
      const int32_t b0 = group_offsets[w], n = group_offsets[w + 1] - b0;
      KahanSum acc;
      for (int32_t i = 0; i < n; ++i) {
        float lt;
        pairwise_member(pooled + b0, pos.data() + b0, n, i, s, dy + b0 + i, &lt);
        acc.add(lt);
      }
      const float a = acc.sum * s;
      total += a;
    }
    *loss = total;
    *n_terms = terms;
  } catch (...) { return KPRN_E_NOMEM; }
  return KPRN_OK;
}
