// The optimiser step (optim.adam / optim.adagrad, OneModel.lua:347-361; MyOptimizer.lua:196-218), kernels and host side: the gradient norm, the dense sweep,
// the lazy-exact row update of the entity table (with its catch-up, its whole-table flush and the data-parallel union route) and zeroPadTokens.  Every row
// route replays a row's skipped steps with the arithmetic of the dense sweep (adam_rows_dev.h): bit-identical to updating every row at every step.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "kprn_internal.h"
#include "adam_rows_dev.h"

namespace {

using kk_dev::AdamRowsArgs;
using kk_dev::addr_or;
using kk_dev::row_lanes;
using kk_dev::with_lanes;

constexpr int TPB = 256;
constexpr int SUMSQ_DET_BLOCKS = 512;   // workgroups of the deterministic gradient norm: 256 for the dense arena, 256 for the rows
inline unsigned nblocks(int64_t n, int per = TPB) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ---- the gradient norm (compiled under the default contraction: outside the region below) ----
__global__ void k_sumsq(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc += x[i] * x[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(out, acc);
}

__global__ void k_sumsq_rows(const float* __restrict__ G, const int32_t* __restrict__ rows, const int32_t* __restrict__ count, int d,
                             float* __restrict__ out) {
  int nrows = *count;
  float acc = 0.f;
  int64_t total = (int64_t)nrows * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float v = G[(int64_t)rows[i / d] * d + (i % d)];
    acc += v * v;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(out, acc);
}

// deterministic mode: workgroups [0, nb) take x, [nb, 2 nb) the listed rows of G (rows == null: they write 0); a thread sums its strided
// elements in ascending order, the wave adds its lanes by the butterfly of wave_sum, the workgroup's four waves are added as (0 + 1) + (2 + 3); the partial
// leaves with a plain store and k_sum_partials adds the 2 nb partials in index order
__global__ __launch_bounds__(256) void k_sumsq_det(const float* __restrict__ x, int64_t n, const float* __restrict__ G, const int32_t* __restrict__ rows,
                                                   const int32_t* __restrict__ count, int d, int nb, float* __restrict__ partial) {
  __shared__ float red[4];
  float acc = 0.f;
  if ((int)blockIdx.x < nb) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)nb * 256) acc += x[i] * x[i];
  } else if (rows) {
    const int64_t total = (int64_t)(*count) * d;
    for (int64_t i = (int64_t)((int)blockIdx.x - nb) * 256 + threadIdx.x; i < total; i += (int64_t)nb * 256) {
      const float v = G[(int64_t)rows[i / d] * d + (i % d)];
      acc += v * v;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the updates: everything down to the closing pragma rounds as written ----
#pragma clang fp contract(off)
__device__ __forceinline__ float clip_factor(const float* norm2, float clip) {
  if (!norm2) return 1.f;
  float nrm = sqrtf(*norm2);
  return (nrm > clip) ? clip / nrm : 1.f;
}

using kk_dev::adam_elem;   // (adam_rows_dev.h: shared with lstm_fused_prefix.hip's catch-up + prefix launch)

// A dense sweep's share of an optimiser step (k_adam_dense, or extra workgroups of the row update's launch; k_adagrad_dense: m = the sums of squares,
// step = the decayed learning rate, the rest of Adam's constants unused).  reg: clip by the norm in *norm2 (null: no clip), then add l2 x;
// consume != 0: the gradient is zeroed as it is used (zeroGradParameters of the next trainBatch, MyOptimizer.lua:186, done here);
// [z0,z0+zn0) and [z1,z1+zn1): pad rows of the span, re-zeroed after the update (zeroPadTokens, MyOptimizer.lua:219);
// tab_slot: this step's entry of the device step-size table (read by the lazy row replay).
struct AdamDenseJob {
  float *x, *g, *m, *v; int64_t n;
  float step, b1, b2, eps; const float* norm2; float clip, l2; int reg, consume;
  int64_t z0; int zn0; int64_t z1; int zn1; float* tab_slot;
};
__device__ __forceinline__ void adam_dense_block(const AdamDenseJob& a, int64_t block) {
  const int64_t i = block * blockDim.x + threadIdx.x;
  if (i == 0 && a.tab_slot) *a.tab_slot = a.step;
  if (i >= a.n) return;
  float gi = a.g[i];
  float xi = a.x[i];
  if (a.reg) { gi = gi * clip_factor(a.norm2, a.clip); gi = gi + a.l2 * xi; }
  float mi = a.m[i], vi = a.v[i];
  adam_elem(xi, mi, vi, gi, a.step, a.b1, a.b2, a.eps);
  if ((i >= a.z0 && i < a.z0 + a.zn0) || (i >= a.z1 && i < a.z1 + a.zn1)) xi = 0.f;
  a.x[i] = xi; a.m[i] = mi; a.v[i] = vi;
  if (a.consume) a.g[i] = 0.f;
}
__global__ void k_adam_dense(AdamDenseJob a) { adam_dense_block(a, blockIdx.x); }

__global__ void k_adagrad_dense(AdamDenseJob a) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  float gi = a.g[i];
  float xi = a.x[i];
  if (a.reg) { gi = gi * clip_factor(a.norm2, a.clip); gi = gi + a.l2 * xi; }
  float Gi = a.m[i] + gi * gi;
  a.m[i] = Gi;
  xi = xi - a.step * gi / (sqrtf(Gi) + 1e-10f);
  if ((i >= a.z0 && i < a.z0 + a.zn0) || (i >= a.z1 && i < a.z1 + a.zn1)) xi = 0.f;
  a.x[i] = xi;
  if (a.consume) a.g[i] = 0.f;
}

// One wave's update of row r, a float per lane at a time: replays the steps (l, upto] the row missed (gradient 0) with the same arithmetic as k_adam_dense,
// then (apply) applies step t_now with the accumulated gradient and clears it.
__device__ __forceinline__ void adam_row_wave(const AdamRowsArgs& a, int64_t r, int32_t l, int32_t upto, bool apply, int d) {
  const int lane = threadIdx.x & 63;
  for (int e = lane; e < d; e += 64) {
    const int64_t o = r * d + e;
    float x[1] = {a.W[o]}, mm[1] = {a.m[o]}, vv[1] = {a.v[o]};
    float g[1] = {0.f};
    float st = 0.f;
    if (apply) { g[0] = a.g[o]; st = a.step_tab[a.t_now]; }
    kk_dev::adam_replay<1>(a, x, mm, vv, l, upto, apply, g, st);
    if (apply) a.g[o] = 0.f;
    if (r == a.pad_row) x[0] = 0.f;  // zeroPadTokens after every step the row lived through (MyOptimizer.lua:219)
    a.W[o] = x[0]; a.m[o] = mm[0]; a.v[o] = vv[0];
  }
  if (lane == 0) a.last[r] = a.t_now;
}

// lazy-exact Adam over a list of rows: one wave per row.  Result is bit-identical to updating every
// row at every step, which is what optim.adam does to the flat vector.
__global__ void k_adam_rows(AdamRowsArgs a, int d) {
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= *a.count) return;
  const int64_t r = a.rows[wave];
  adam_row_wave(a, r, a.last[r], a.apply_step ? a.t_now - 1 : a.t_now, a.apply_step != 0, d);
}

// every row of the table that lags is brought up to t_now; a row that is current, or that no step has touched, is not touched at all (`last` included)
__global__ void k_adam_flush_all(AdamRowsArgs a, int64_t V, int d) {
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= V) return;
  const int32_t l = a.last[r];
  if (l <= 0 || l >= a.t_now) return;
  adam_row_wave(a, r, l, a.t_now, false, d);
}

// the same for rows of d = 4 G floats handled by G = 8 / 16 / 32 lanes with 16-byte accesses (d = 32: eight rows per wave instead of one
// half-empty wave per row; the per-element arithmetic is adam_elem's, so the result stays bit-identical to the dense sweep)
// dense (nullable in effect: no workgroup past rows_blocks): the dense arena's update rides in the same launch as workgroups [rows_blocks, gridDim.x)
// -- two latency-bound launches of the step's serial tail become one.  The row update then takes THIS step's size from a.step_now (the dense job writes the
// table entry for later replays; inside one launch nothing orders that store before a row's read of it); step_now < 0: read it from the table.
template <int G>
__global__ void k_adam_rows_v(AdamRowsArgs a, int rows_blocks, AdamDenseJob dense) {
  if ((int)blockIdx.x >= rows_blocks) { adam_dense_block(dense, (int64_t)blockIdx.x - rows_blocks); return; }
  kk_dev::adam_rows_lane_block<G>(a, (int64_t)blockIdx.x);
}

// Data-parallel exchange, union + update in ONE launch (lazy-exact Adam, no clip / L2).  `all` = the all-gathered packed buffers
// [world][stride] of kprn_sparse_grad_pack: {count, -, -, -, ids[cap] ASCENDING (the batch index's run-length-encoded sorted keys, each
// row once), rows[cap][d]}.  One G-lane group per (rank, entry); lane j finds the row in rank j's list by binary search (world <= G), the
// positions are shared through the group; the entry of the LOWEST rank that touched the row owns it: it adds the other ranks'
// contributions in RANK ORDER (the same addition order on every replica, and the order k_add_rank's launches used), replays the row's
// skipped steps and applies this one.  No flag array over the table, no compaction, no gradient accumulator round trip.
template <int G>
__global__ void k_union_adam(const int32_t* __restrict__ all, int world, int cap, int64_t stride, AdamRowsArgs a) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int64_t slot = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int j = threadIdx.x % G;
  const int base = (threadIdx.x & 63) & ~(G - 1);
  const int r = (int)(slot / cap), k = (int)(slot - (int64_t)r * cap);
  const bool in_range = r < world;
  const int32_t* mine = all + (int64_t)(in_range ? r : 0) * stride;
  const bool live = in_range && k < mine[0];
  const int32_t row = live ? mine[4 + k] : 0;
  int pos = -1;
  if (live && j < world && j != r) {
    const int32_t* o = all + (int64_t)j * stride;
    const int n = o[0];
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (o[4 + mid] < row) lo = mid + 1; else hi = mid;
    }
    if (lo < n && o[4 + lo] == row) pos = lo;
  }
  f4 g4 = f4{0.f, 0.f, 0.f, 0.f};
  if (live) g4 = *(const f4*)((const float*)(mine + 4 + cap) + (int64_t)k * (4 * G) + 4 * j);
  bool owner = live;
  for (int q = 0; q < world; ++q) {   // every lane of the wave takes every shuffle (the groups of one wave may belong to two ranks)
    const int p = __shfl(pos, base + q, 64);
    if (p < 0 || !live || q == r) continue;
    if (q < r) owner = false;
    else if (owner) g4 = g4 + *(const f4*)((const float*)(all + (int64_t)q * stride + 4 + cap) + (int64_t)p * (4 * G) + 4 * j);
  }
  if (!owner) return;
  const int32_t l = a.last[row];
  const int64_t o = (int64_t)row * (4 * G) + 4 * j;
  const f4 x4 = *(const f4*)(a.W + o), m4 = *(const f4*)(a.m + o), v4 = *(const f4*)(a.v + o);
  float x[4] = {x4[0], x4[1], x4[2], x4[3]}, mm[4] = {m4[0], m4[1], m4[2], m4[3]}, vv[4] = {v4[0], v4[1], v4[2], v4[3]};
  const float g[4] = {g4[0], g4[1], g4[2], g4[3]};
  kk_dev::adam_replay<4>(a, x, mm, vv, l, a.t_now - 1, true, g, a.step_tab[a.t_now]);
  if (row == a.pad_row) { x[0] = x[1] = x[2] = x[3] = 0.f; }  // zeroPadTokens (MyOptimizer.lua:219)
  *(f4*)(a.W + o) = f4{x[0], x[1], x[2], x[3]}; *(f4*)(a.m + o) = f4{mm[0], mm[1], mm[2], mm[3]}; *(f4*)(a.v + o) = f4{vv[0], vv[1], vv[2], vv[3]};
  if (j == 0) a.last[row] = a.t_now;
}

__global__ void k_adagrad_rows(float* __restrict__ W, float* __restrict__ g, float* __restrict__ G, const int32_t* __restrict__ rows,
                               const int32_t* __restrict__ count, int d, float clr, int64_t pad_row) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= *count) return;
  const int64_t r = rows[wave];
  for (int e = lane; e < d; e += 64) {
    const int64_t o = r * d + e;
    float gi = g[o];
    float Gi = G[o] + gi * gi;
    G[o] = Gi;
    W[o] = (r == pad_row) ? 0.f : W[o] - clr * gi / (sqrtf(Gi) + 1e-10f);
    g[o] = 0.f;
  }
}
#pragma clang fp contract(fast)

// MyOptimizer:zeroPadTokens (MyOptimizer.lua:74-93): the three pad rows in one launch
__global__ void k_zero_pad3(float* __restrict__ a, int na, float* __restrict__ b, int nb, float* __restrict__ c, int nc) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < na) a[j] = 0.f;
  if (j < nb) b[j] = 0.f;
  if (j < nc) c[j] = 0.f;
}

__global__ void k_fill_i32(int32_t* __restrict__ x, int64_t n, int32_t v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = v;
}

__global__ void k_clear_rows(float* __restrict__ G, const int32_t* __restrict__ rows, const int32_t* __restrict__ count, int d) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= *count) return;
  const int64_t r = rows[wave];
  for (int e = lane; e < d; e += 64) G[r * d + e] = 0.f;
}

#define CHECK_LAUNCH() HIP_TRY(hipGetLastError())

// ---- launchers ----
void dense_sweep(hipStream_t s, void (*kernel)(AdamDenseJob), const AdamDenseJob& job) {   // k_adam_dense / k_adagrad_dense over job.n elements
  if (job.n <= 0) return;
  hipLaunchKernelGGL(kernel, dim3(nblocks(job.n)), dim3(TPB), 0, s, job);
  CHECK_LAUNCH();
}

// The lazy-exact row update of the entity table, with an optional dense job riding in the same grid (rows of 32 / 64 / 128 floats, 16-byte aligned tables: the
// optimiser step of the rows AND of the dense arena as ONE launch; the rows then take this step's size from the job).  false: nothing was launched -- no rows,
// or a dense job on a shape the lane kernels do not cover (the caller launches the two separately).  Same per-element arithmetic on every route (adam_elem).
bool adam_rows(hipStream_t s, AdamRowsArgs a, int64_t max_rows, int d, const AdamDenseJob* dense = nullptr) {
  const int G = row_lanes(d, addr_or(a.W, a.g, a.m, a.v));
  if (max_rows <= 0 || (dense && (dense->n <= 0 || !G))) return false;
  a.step_now = dense ? dense->step : -1.f;
  if (G) {
    const AdamDenseJob dj = dense ? *dense : AdamDenseJob{};
    const int nd = dense ? (int)nblocks(dense->n) : 0;
    with_lanes(G, [&](auto lanes) {
      constexpr int LG = decltype(lanes)::value;
      const int nb = (int)nblocks(max_rows * LG);
      hipLaunchKernelGGL(k_adam_rows_v<LG>, dim3(nb + nd), dim3(TPB), 0, s, a, nb, dj);
    });
  } else {
    hipLaunchKernelGGL(k_adam_rows, dim3(nblocks(max_rows * 64)), dim3(TPB), 0, s, a, d);
  }
  CHECK_LAUNCH();
  return true;
}

// union of all ranks' packed rows + the lazy-exact Adam step on it (k_union_adam); false = shape not covered (the caller materialises
// the union with bidx::merge_rows and takes the ordinary row update)
bool union_adam(hipStream_t s, const void* all, int world, int cap, int64_t stride, int d, const AdamRowsArgs& a) {
  const int G = row_lanes(d, addr_or(a.W, a.m, a.v, all));
  if (!G || (stride & 3) != 0 || (cap & 3) != 0 || world > G || world <= 0 || cap <= 0) return false;
  const int64_t n = (int64_t)world * cap;
  with_lanes(G, [&](auto lanes) {
    constexpr int LG = decltype(lanes)::value;
    hipLaunchKernelGGL(k_union_adam<LG>, dim3(nblocks(n * LG)), dim3(TPB), 0, s, (const int32_t*)all, world, cap, stride, a);
  });
  CHECK_LAUNCH();
  return true;
}

// the entity table's row update as the handle stands: its constants are those of the last Adam step, t_now the step the table is current to
AdamRowsArgs rows_args(const kprn_handle* h, const int32_t* rows, const int32_t* count, int apply_step) {
  return AdamRowsArgs{h->We, h->g_We, h->s1_We, h->s2_We, h->We_last, rows, count, (int32_t)h->opt_step, apply_step, h->step_tab,
                      h->last_b1, h->last_b2, h->last_eps, (int64_t)h->cfg.Ve - 1, -1.f};
}

// the dense arena's (entity: the whole entity table's) share of a step of size `step`; the arena's gradient is consumed, the table's rows are cleared by list
AdamDenseJob dense_job(const kprn_handle* h, const kprn_opt* o, bool entity, float step, const float* norm2, float l2) {
  const kprn_config& c = h->cfg;
  AdamDenseJob a{};
  a.step = step; a.b1 = o->beta1; a.b2 = o->beta2; a.eps = o->eps; a.norm2 = norm2; a.clip = o->grad_clip_norm; a.l2 = l2;
  a.reg = (norm2 != nullptr || l2 != 0.f) ? 1 : 0;
  if (entity) {
    a.x = h->We; a.g = h->g_We; a.m = h->s1_We; a.v = h->s2_We; a.n = h->n_ent;
    a.z0 = ((int64_t)c.Ve - 1) * c.de; a.zn0 = c.de;
  } else {
    a.x = h->dense; a.g = h->g_dense; a.m = h->s1_dense; a.v = h->s2_dense; a.n = h->n_dense; a.consume = 1;
    a.z0 = h->off_Wt + (int64_t)(c.Vt - 1) * c.dt; a.zn0 = c.dt; a.z1 = h->off_Wr + (int64_t)(c.Vr - 1) * c.dr; a.zn1 = c.dr;
  }
  return a;
}

}  // namespace

namespace kk {

void clear_rows(hipStream_t s, float* G, const int32_t* rows, const int32_t* count, int64_t max_rows, int d) {
  if (max_rows <= 0) return;
  hipLaunchKernelGGL(k_clear_rows, dim3(nblocks(max_rows * 64)), dim3(TPB), 0, s, G, rows, count, d);
  CHECK_LAUNCH();
}

}  // namespace kk

namespace optim {

void step_tab_reserve(kprn_handle* h, int64_t need) {
  if (need < h->step_tab_cap) return;
  int64_t cap = std::max<int64_t>(4096, h->step_tab_cap * 2);
  while (cap <= need) cap *= 2;
  float* nd = dalloc<float>(cap);
  float* nh = nullptr;
  HIP_TRY(hipHostMalloc((void**)&nh, (size_t)cap * sizeof(float)));
  memset(nh, 0, (size_t)cap * sizeof(float));
  if (h->step_tab) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    memcpy(nh, h->step_tab_host, (size_t)h->step_tab_cap * sizeof(float));
    HIP_TRY(hipMemcpy(nd, nh, (size_t)h->step_tab_cap * sizeof(float), hipMemcpyHostToDevice));
    hipFree(h->step_tab);
    hipHostFree(h->step_tab_host);
  }
  h->step_tab = nd; h->step_tab_host = nh; h->step_tab_cap = cap;
}

// bring every entity row up to opt_step (needed before anything reads the whole table)
void flush_lazy(kprn_handle* h) {
  join_score(h);
  if (!h->lazy_pending) return;
  ProfScope ps(h, "adam_flush_all");
  hipLaunchKernelGGL(k_adam_flush_all, dim3(nblocks((int64_t)h->cfg.Ve * 64)), dim3(TPB), 0, h->stream, rows_args(h, nullptr, nullptr, 0), (int64_t)h->cfg.Ve,
                     h->cfg.de);
  CHECK_LAUNCH();
  h->lazy_pending = false;
  bf16p::params_changed(h, false);   // the replay rewrote rows no row list names: the bf16 shadow of the whole table is stale
}

void zero_pad_tokens(kprn_handle* h) {
  const kprn_config& c = h->cfg;
  join_score(h);
  const int n = std::max(c.dt, std::max(c.dr, c.de));
  hipLaunchKernelGGL(k_zero_pad3, dim3(nblocks(n)), dim3(TPB), 0, h->stream, h->dense + h->off_Wt + (int64_t)(c.Vt - 1) * c.dt, c.dt,
                     h->dense + h->off_Wr + (int64_t)(c.Vr - 1) * c.dr, c.dr, h->We + (int64_t)(c.Ve - 1) * c.de, c.de);
  CHECK_LAUNCH();
  h->pad_clean = true;
}

// rows of this batch that are behind opt_step are replayed before the forward reads them
void catch_up(kprn_handle* h, const kprn_batch* b) {
  if (h->lazy_pending && !b->has_index) { flush_lazy(h); return; }   // (no row list: bring the whole table up to date instead)
  if (!h->lazy_pending || b->n_uniq == 0) return;
  if (h->caught_serial == b->serial && h->caught_step == h->opt_step) return;  // this batch's rows are already current
  join_score(h);
  ProfScope ps(h, "adam_rows_catchup");
  const AdamRowsArgs ra = rows_args(h, b->uniq, b->uniq + b->uniq_cap, 0);   // (the count lives at the tail of the list buffer)
  // (fused path, a batch with an identical-prefix plan: its prefix table is one more workgroup of this launch -- fused::catch_up_with_prefix)
  const bool with_prefix = h->cfg.compute_dtype == 0 && use_fused(h, b, false) && fused::catch_up_with_prefix(h, b, ra);
  if (!with_prefix) adam_rows(h->stream, ra, b->n_uniq, h->cfg.de);
  bf16p::rows_updated(h, b->uniq, b->uniq + b->uniq_cap, b->n_uniq);
  h->caught_serial = b->serial; h->caught_step = h->opt_step;
}

// What a kprn_opt may not ask of this handle, checked before a step launches or writes anything.  The method stays what the handle's first step used: optimiser
// slot 0 holds Adam's first moments or Adagrad's sums of squares, one or the other -- Adagrad's square root over Adam's negative moments is NaN, Adam would
// read the sums as momentum -- and an Adagrad step leaves no step size for a lagging row's replay.
void opt_check(const kprn_handle* h, const kprn_opt* o) {
  KPRN_REQUIRE(o != nullptr, KPRN_E_ARG, "opt is NULL");
  KPRN_REQUIRE(o->method == 0 || o->method == 1, KPRN_E_ARG, "opt.method must be 0 (adagrad) or 1 (adam)");
  KPRN_REQUIRE(h->opt_method < 0 || o->method == h->opt_method, KPRN_E_ARG,
               std::string("opt.method changed from ") + (h->opt_method == 1 ? "adam to adagrad" : "adagrad to adam") +
                   " on a handle that has taken steps: the two methods keep different state in optimiser slot 0 (first moments / sums of squares); use a new handle");
}

// |g|^2 over the dense arena and the step's entity rows into h->d_norm2
static const float* grad_norm(kprn_handle* h) {
  hipStream_t s = h->stream;
  const int de = h->cfg.de;
  ProfScope ps(h, "grad_norm");
  if (h->deterministic) {
    // *d_norm2 = |x|^2 + |listed rows of G|^2 (no rows: the first term only) from one plain-stored partial per workgroup (a grid that depends on nothing but
    // n), summed in index order by kk::sum_partials' kernel -- no atomics
    const int nb = SUMSQ_DET_BLOCKS / 2;
    if (!h->det_norm_part) h->det_norm_part = dalloc<float>(SUMSQ_DET_BLOCKS);
    hipLaunchKernelGGL(k_sumsq_det, dim3(2 * nb), dim3(256), 0, s, h->g_dense, h->n_dense, h->g_We, h->step_rows_ub > 0 ? h->rows_view : nullptr, h->count_view,
                       de, nb, h->det_norm_part);
    CHECK_LAUNCH();
    kk::sum_partials(s, h->det_norm_part, 2 * nb, h->d_norm2, 0);
  } else {
    HIP_TRY(hipMemsetAsync(h->d_norm2, 0, sizeof(float), s));
    if (h->n_dense > 0) {
      hipLaunchKernelGGL(k_sumsq, dim3(std::min(nblocks(h->n_dense), 2048u)), dim3(TPB), 0, s, h->g_dense, h->n_dense, h->d_norm2);
      CHECK_LAUNCH();
    }
    if (h->step_rows_ub > 0) {
      hipLaunchKernelGGL(k_sumsq_rows, dim3(1024), dim3(TPB), 0, s, h->g_We, h->rows_view, h->count_view, de, h->d_norm2);
      CHECK_LAUNCH();
    }
  }
  return h->d_norm2;
}

// one Adam step over the dense arena and the entity table (merged / dense entity sweep / the exchange's union in place / row list); returns whether the
// pad rows are zero afterwards
static bool adam_step(kprn_handle* h, const kprn_opt* o, bool dense_ent, bool fuse_union, const float* norm2, float l2) {
  const kprn_config& c = h->cfg;
  hipStream_t s = h->stream;
  // rows that lag replay their skipped steps with the constants those steps ran with: new ones are adopted only once the table is current
  if (h->lazy_pending && (o->beta1 != h->last_b1 || o->beta2 != h->last_b2 || o->eps != h->last_eps)) flush_lazy(h);
  h->last_b1 = o->beta1; h->last_b2 = o->beta2; h->last_eps = o->eps;
  if (dense_ent && !h->ent_dense_mode) { flush_lazy(h); h->ent_dense_mode = true; }
  if (!dense_ent && h->ent_dense_mode) {
    hipLaunchKernelGGL(k_fill_i32, dim3(nblocks(c.Ve)), dim3(TPB), 0, s, h->We_last, (int64_t)c.Ve, (int32_t)h->opt_step);
    CHECK_LAUNCH();
    h->ent_dense_mode = false;
  }
  h->opt_step += 1;
  const int64_t t = h->opt_step;
  step_tab_reserve(h, t + 1);
  const double bc1 = 1.0 - pow((double)o->beta1, (double)t), bc2 = 1.0 - pow((double)o->beta2, (double)t);
  const float step = (float)((double)o->lr * sqrt(bc2) / bc1);
  h->step_tab_host[t] = step;  // host mirror (table growth); the device entry is written by the dense kernel
  AdamDenseJob arena = dense_job(h, o, false, step, norm2, l2);
  arena.tab_slot = h->step_tab + t;
  // the row update and the dense arena's update as ONE launch where the shapes allow (two latency-bound launches of the serial tail less; option
  // "adam_merged" = "0": separately): the same arithmetic per element either way
  bool merged = false;
  if (h->adam_merged && !dense_ent && !fuse_union && h->step_rows_ub > 0) {
    ProfScope ps(h, "adam_step");
    merged = adam_rows(s, rows_args(h, h->rows_view, h->count_view, 1), h->step_rows_ub, c.de, &arena);
  }
  if (merged) { h->lazy_pending = true; return h->pad_clean; }
  {
    ProfScope ps(h, "adam_dense");
    dense_sweep(s, k_adam_dense, arena);
  }
  if (dense_ent) {
    ProfScope ps(h, "adam_entity_dense");
    dense_sweep(s, k_adam_dense, dense_job(h, o, true, step, norm2, l2));
    kk::clear_rows(s, h->g_We, h->rows_view, h->count_view, h->step_rows_ub, c.de);
    return true;
  }
  ProfScope ps(h, "adam_entity_rows");
  if (fuse_union) {
    const int64_t stride = 4 + (int64_t)h->dp_cap * (1 + c.de) + dp_tail_words(h);
    if (union_adam(s, h->dp_all, h->dp_world, h->dp_cap, stride, c.de, rows_args(h, nullptr, nullptr, 1))) {
      h->dp_union_pending = false; h->step_rows_ub = 0; h->rows_view = h->step_rows; h->count_view = h->step_count; h->view_batch = nullptr;
    } else {
      fuse_union = false;
      materialize_union(h);
    }
  }
  if (!fuse_union) adam_rows(s, rows_args(h, h->rows_view, h->count_view, 1), h->step_rows_ub, c.de);
  h->lazy_pending = true;
  return h->pad_clean;  // the pad row is re-zeroed whenever the row update touches it; untouched it stays what it was
}

static bool adagrad_step(kprn_handle* h, const kprn_opt* o, bool reg, const float* norm2, float l2) {
  const kprn_config& c = h->cfg;
  hipStream_t s = h->stream;
  const float clr = (float)((double)o->lr / (1.0 + (double)h->opt_step * (double)o->lr_decay));
  {
    ProfScope ps(h, "adagrad_dense");
    dense_sweep(s, k_adagrad_dense, dense_job(h, o, false, clr, norm2, l2));
  }
  if (reg) {
    ProfScope ps(h, "adagrad_entity_dense");
    dense_sweep(s, k_adagrad_dense, dense_job(h, o, true, clr, norm2, l2));
    kk::clear_rows(s, h->g_We, h->rows_view, h->count_view, h->step_rows_ub, c.de);
  } else {
    ProfScope ps(h, "adagrad_entity_rows");
    if (h->step_rows_ub > 0) {
      hipLaunchKernelGGL(k_adagrad_rows, dim3(nblocks(h->step_rows_ub * 64)), dim3(TPB), 0, s, h->We, h->g_We, h->s1_We, h->rows_view, h->count_view, c.de, clr,
                         (int64_t)c.Ve - 1);
      CHECK_LAUNCH();
    }
  }
  h->opt_step += 1;
  return reg || h->pad_clean;
}

void apply_update(kprn_handle* h, const kprn_opt* o) {
  opt_check(h, o);
  const kprn_config& c = h->cfg;
  join_score(h);
  const bool reg = (o->regularize == 1);
  const bool dense_ent = reg || o->entity_update == 1;
  // the exchange's union: walked in place by the row update (lazy-exact Adam, fp32 table only, the lane rule's rows) or materialised first
  const int union_lanes = row_lanes(c.de, 0);
  const bool fuse_union = h->dp_union_pending && o->method == 1 && !dense_ent && !h->bf16_state && union_lanes && h->dp_world <= union_lanes &&
                          (h->dp_cap & 3) == 0;
  if (h->dp_union_pending && !fuse_union) materialize_union(h);
  if (!h->view_batch) { h->rows_view = h->step_rows; h->count_view = h->step_count; }  // (the exchange may have re-allocated the list)
  const float* norm2 = (reg && o->use_grad_clip) ? grad_norm(h) : nullptr;
  const float l2 = reg ? o->l2 : 0.f;
  // (pad rows: re-zeroed by the dense kernels right after the update, by the row kernels whenever they touch one -- zeroPadTokens, MyOptimizer.lua:219)
  const bool pad_done = (o->method == 1) ? adam_step(h, o, dense_ent, fuse_union, norm2, l2) : adagrad_step(h, o, reg, norm2, l2);
  h->ent_grads_dirty = false;
  h->dense_grads_clean = true;
  h->opt_method = o->method;
  if (pad_done) h->pad_clean = true;
  else zero_pad_tokens(h);   // MyOptimizer.lua:219
  // the rows this step updated are current; if they were one batch's rows, a forward over that batch needs no catch-up
  h->caught_serial = h->grads_serial; h->caught_step = h->opt_step;
  fused::params_changed(h);
  // bf16 shadows: the dense arena always; the entity table row by row unless the whole table moved (dense sweep)
  const bool whole_table = (o->method == 1) ? dense_ent : reg;
  bf16p::params_changed(h, !whole_table);
  if (!whole_table && h->step_rows_ub > 0) bf16p::rows_updated(h, h->rows_view, h->count_view, h->step_rows_ub);
}

}  // namespace optim
