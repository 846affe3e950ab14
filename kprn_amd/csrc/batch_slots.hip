// Batches and feed slots: the lifecycle of a kprn_batch (layout, reserve, enqueue, finish, ready, detach, release) and the C ABI entry points around it.
//
// A batch is a slot of device buffers (ids, labels, occurrence index, identical-prefix plan).  kprn_batch_create fills a new slot
// on the handle's stream and returns when it is ready; kprn_batch_feed_async refills a slot on the FEED stream and returns at
// once -- the role BatcherFileList:populateGPUTensor plays for the reference (preallocated tensors, one :copy per minibatch,
// BatcherFileList.lua:53-96), plus the per-batch device work this engine adds (validation, index, plan).
// All device arrays of a slot live in ONE allocation, laid out afresh for every fill from the batch's own sizes:
//   idx | idx_s | perm | slot_of | tile_k | pmeta | key_sorted | pos_sorted | uniq ... count | labels | flag
// (each rounded to 16 bytes).  The host-built feed prepares a page-locked image of exactly this block and uploads it with a
// single copy.
// Lifetime rules, each stated once: slots::detach says what the handle may still reference in a slot and what becomes of each reference before the slot's
// contents or the slot itself go away; slots::reserve drains every stream (sync_all_streams) before it frees a block that passes may still read.
#include <string.h>

#include <algorithm>
#include <exception>
#include <thread>

#include "kprn_internal.h"

namespace slots {
struct BatchLayout { int64_t idx, idx_s, perm, slot_of, tile_k, pmeta, off, wg, key, pos, uniq, cnt, labels, flag, words; };
// ragged: + the offsets [B+1] and the loss-stage workgroup table [<= B+1], in front of the index so that every upload range of the host-built feed holds them
static BatchLayout layout(int64_t B, int64_t N, int T, int F, bool plan, bool labels, bool ragged = false) {
  auto r4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  const int64_t nsteps = N * T, n_index = nsteps + (plan ? fused::KCAP : 0);
  BatchLayout l;
  int64_t o = 0;
  l.idx = o; o += r4(nsteps * F);
  l.idx_s = o; o += plan ? r4(nsteps * F) : 0;
  l.perm = o; o += plan ? r4(N) : 0;
  l.slot_of = o; o += plan ? r4(N) : 0;
  l.tile_k = o; o += plan ? r4((N + 63) / 64 + 1) : 0;
  l.pmeta = o; o += plan ? 24 : 0;
  l.off = o; o += ragged ? r4(B + 1) : 0;
  l.wg = o; o += ragged ? r4(B + 1) : 0;
  l.key = o; o += r4(n_index);
  l.pos = o; o += r4(n_index);
  l.uniq = o; o += r4(n_index);
  l.cnt = o; o += 4;
  l.labels = o; o += labels ? r4(B) : 0;
  l.flag = o; o += 4;
  l.words = o;
  return l;
}

static void free_buffers(kprn_batch* b) {
  dfree(b->block);
  b->block_cap = 0;
  b->idx = b->idx_s = b->perm = b->slot_of = b->tile_k = b->pmeta = b->off = b->wg = b->key_sorted = b->pos_sorted = b->uniq = b->d_flag = nullptr;
  b->labels = nullptr;
}

void release(kprn_batch* b) {
  if (b->job.valid()) { try { b->job.get(); } catch (...) {} }
  if (b->hs) { hipHostFree(b->hs); b->hs = nullptr; }
  if (b->ev_fork) { hipEventDestroy(b->ev_fork); hipEventDestroy(b->ev_fork2); b->ev_fork = b->ev_fork2 = nullptr; }
  free_buffers(b);
  dfree(b->groups);
  if (b->h_meta) { hipHostFree(b->h_meta); b->h_meta = nullptr; }
  if (b->ev_ready) { hipEventDestroy(b->ev_ready); b->ev_ready = nullptr; }
  delete b;
}

static bool wants_plan(kprn_handle* h, const kprn_batch* b) {
  // (small batches run on tiles of one 16-row m-tile, which have no per-tile prefix classes: lstm_fused_fwd.hip small_tiles)
  if (fused::small_tiles(h, b->N, false)) return false;
  return h->prefix_plan && use_fused(h, b, true) && b->F <= 16 && !(kprn_dbg_mask() & 64);
}

// word offsets in a slot's pinned summary h_meta: validation flag | distinct rows | plan header pmeta [8 + F <= 24] (the reference step's ids from word 8) | tile_k
struct Meta { static constexpr int flag = 0, n_uniq = 1, plan = 2, plan_ref = plan + 8, tile_k = plan + 8 + 16; };

// buffers for a [B,P,T,F] batch; a refill that fits the slot's capacities allocates nothing.  Before a buffer of a slot in use is freed every stream is
// drained: passes on the main, scoring, rest, feed and upload streams may still read it (a new batch has no buffers, so kprn_batch_create never waits here)
static void reserve(kprn_handle* h, kprn_batch* b, int32_t B, int32_t P, int32_t T, int32_t F, bool labels, int64_t min_pairs = 0, int64_t min_paths = 0,
                    int64_t n_ragged = 0) {
  const bool ragged = n_ragged > 0;   // (P is 0 then)
  b->B = B; b->P = P; b->T = T; b->F = F;
  const int64_t N = ragged ? n_ragged : (int64_t)B * P, nsteps = N * T;
  b->N = N;
  const bool plan = wants_plan(h, b);
  b->kcap = plan ? fused::KCAP : 0;
  b->n_index = nsteps + b->kcap;
  // the allocation only grows (a slot that has held the largest minibatch never allocates again; kprn_batch_slot_reserve sizes
  // it up front, for the larger of the two layouts)
  const BatchLayout l = layout(B, N, T, F, plan, labels, ragged);
  int64_t want = l.words;
  if (min_pairs > 0 || min_paths > 0)   // (a reserved slot holds a rectangular or a ragged batch of that size)
    want = std::max(want, layout(std::max<int64_t>(B, min_pairs), std::max<int64_t>(N, min_paths), T, F, true, true, true).words);
  if (want > b->block_cap) {
    if (b->block) { sync_all_streams(h); free_buffers(b); }
    b->block = dalloc<int32_t>(want);
    b->block_cap = want;
  }
  int32_t* k = b->block;
  b->idx = k + l.idx;
  b->idx_s = plan ? k + l.idx_s : nullptr; b->perm = plan ? k + l.perm : nullptr; b->slot_of = plan ? k + l.slot_of : nullptr;
  b->tile_k = plan ? k + l.tile_k : nullptr; b->pmeta = plan ? k + l.pmeta : nullptr;
  b->off = ragged ? k + l.off : nullptr; b->wg = ragged ? k + l.wg : nullptr;
  if (!ragged) { b->n_wg = 0; b->max_cnt = 0; b->seg_wave = 0; }
  b->key_sorted = k + l.key; b->pos_sorted = k + l.pos; b->uniq = k + l.uniq;
  b->uniq_cap = l.cnt - l.uniq;  // the distinct-row count lives at uniq[uniq_cap]
  b->labels = labels ? (float*)(k + l.labels) : nullptr;
  b->d_flag = k + l.flag;
  const int64_t meta_need = Meta::tile_k + (std::max<int64_t>(N, min_paths) + 63) / 64 + 1;
  if (meta_need > b->h_meta_cap) {
    if (b->h_meta) { sync_all_streams(h); hipHostFree(b->h_meta); b->h_meta = nullptr; }
    HIP_TRY(hipHostMalloc((void**)&b->h_meta, (size_t)meta_need * 2 * sizeof(int32_t)));
    b->h_meta_cap = meta_need * 2;
  }
}

// upload + validation + identical-prefix plan + occurrence index on stream s; the host-side summary (validation flag, distinct
// rows, plan header, per-tile prefix lengths) lands in the slot's pinned block behind them.  Nothing here waits for the device.
// idx == null: the ids are produced on the device by fill, straight into the slot's idx block
static void enqueue(kprn_handle* h, kprn_batch* b, const int32_t* idx, const float* labels, hipStream_t s, void* scratch, size_t scratch_bytes,
                    const DeviceFill* fill = nullptr) {
  const int32_t B = b->B, T = b->T, F = b->F;
  const int64_t N = b->N, nsteps = N * T;
  const bool plan = b->kcap > 0;
  if (idx) HIP_TRY(hipMemcpyAsync(b->idx, idx, (size_t)nsteps * F * sizeof(int32_t), hipMemcpyHostToDevice, s));
  else (*fill)(b->idx, s);
  if (b->off) {   // ragged: offsets + workgroup table as the host derived them (kk::ragged_plan)
    HIP_TRY(hipMemcpyAsync(b->off, b->hrag.data(), (size_t)(B + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b->wg, b->hrag.data() + (B + 1), (size_t)(b->n_wg + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  if (labels) HIP_TRY(hipMemcpyAsync(b->labels, labels, (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(b->d_flag, 0, sizeof(int32_t), s));
  kk::validate_indices(s, b->idx, nsteps, F, h->cfg.num_types, h->cfg.Vt, h->cfg.Ve, h->cfg.Vr, b->d_flag);
  // identical-prefix plan (fused path only): paths reordered by the number of leading steps they share with the batch's
  // reference step; the fused kernels start each 64-path tile behind its shared steps (lstm_fused_prefix.hip)
  if (plan)
    bidx::prefix_plan(s, b->idx, N, T, F, h->cfg.num_types, b->kcap, b->idx_s, b->perm, b->slot_of, b->tile_k, b->pmeta, scratch, scratch_bytes);
  // occurrence index: positions sorted by entity row + the sorted distinct rows (count at the tail of the list)
  bidx::build(s, plan ? b->idx_s : b->idx, N, T, F, h->cfg.Ve, plan ? b->tile_k : nullptr, plan ? b->pmeta : nullptr, b->kcap, b->key_sorted,
              b->pos_sorted, b->uniq, b->uniq + b->uniq_cap, scratch, scratch_bytes);
  int32_t* m = b->h_meta;
  HIP_TRY(hipMemcpyAsync(m + Meta::flag, b->d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(m + Meta::n_uniq, b->uniq + b->uniq_cap, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (plan) {
    HIP_TRY(hipMemcpyAsync(m + Meta::plan, b->pmeta, (size_t)(8 + F) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m + Meta::tile_k, b->tile_k, (size_t)((N + 63) / 64) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  }
}

// the device work of enqueue is complete: take the host-side summary over
static void finish(kprn_handle* h, kprn_batch* b) {
  const int32_t* m = b->h_meta;
  const int64_t nsteps = b->N * b->T, N = b->N;
  b->pending = false;
  b->n_uniq = m[Meta::n_uniq];
  b->h_kmax = 0;
  b->exec_steps = nsteps;
  if (b->kcap > 0) {
    b->h_kmax = m[Meta::plan];
    for (int c = 0; c < b->F && c < 16; ++c) b->h_ref[c] = m[Meta::plan_ref + c];
    const int32_t* tk = m + Meta::tile_k;
    for (int64_t tl = 0; tl < (N + 63) / 64; ++tl) b->exec_steps -= (int64_t)tk[tl] * std::min<int64_t>(64, N - tl * 64);
  }
  b->serial = h->next_serial++;
  b->bad = (m[Meta::flag] != 0);
  KPRN_REQUIRE(!b->bad, KPRN_E_INDEX, "an index is outside 1..vocabSize (ids are 1-based, int2torch.lua:60-63)");
}

// first use of a slot filled by kprn_batch_feed_async: wait for its feed (issued a step earlier), read the summary
void ready(kprn_handle* h, const kprn_batch* cb) {
  kprn_batch* b = const_cast<kprn_batch*>(cb);
  if (!b) return;
  if (b->pending && b->host_built) {
    // the worker thread has derived plan + index and queued the uploads: take its summary, order this stream behind the uploads
    b->pending = false;
    b->job.get();  // (rethrows what the job threw)
    const kprn_batch::HostResult& r = b->hres;
    b->bad = r.bad; b->n_uniq = r.n_uniq; b->h_kmax = r.kmax; b->exec_steps = r.exec_steps;
    for (int c = 0; c < 16; ++c) b->h_ref[c] = r.ref[c];
    b->serial = h->next_serial++;
    if (!b->bad) HIP_TRY(hipStreamWaitEvent(h->stream, b->ev_ready, 0));
  } else if (b->pending) {
    HIP_TRY(hipEventSynchronize(b->ev_ready));
    finish(h, b);
  }
  KPRN_REQUIRE(!b->bad, KPRN_E_INDEX, "an index is outside 1..vocabSize (ids are 1-based, int2torch.lua:60-63)");
}

// a fill's arguments, checked before a slot is touched.  counts != null: a ragged batch of N paths (P is ignored and comes back 0); its plan is derived here
struct RaggedPlan { std::vector<int32_t> tab; int32_t sum[3] = {0, 0, 0}; };   // offsets [B+1] | workgroup table, and kk::ragged_plan's summary words
static void check_fill(kprn_handle* h, const int32_t* idx, const int32_t* counts, int32_t B, int32_t* P, int64_t N, int32_t T, int32_t F, RaggedPlan* rp,
                       bool on_device = false) {
  KPRN_REQUIRE(idx || on_device, KPRN_E_ARG, "idx is NULL");
  if (!counts) KPRN_REQUIRE(B > 0 && *P > 0 && T > 0, KPRN_E_ARG, "B, P, T must be positive");
  else KPRN_REQUIRE(B > 0 && N >= B && T > 0, KPRN_E_ARG, "B, T must be positive and N >= B");
  KPRN_REQUIRE(F == h->cfg.F, KPRN_E_ARG, "F does not match numFeatureTemplates");
  if (!counts) return;
  *P = 0;
  KPRN_REQUIRE(N * T + fused::KCAP <= 0x7fffffffLL, KPRN_E_ARG, "N*T does not fit the 32-bit positions of the occurrence index");
  rp->tab.resize((size_t)(2 * (int64_t)B + 2));
  KPRN_REQUIRE(kk::ragged_plan(counts, B, N, rp->tab.data(), rp->tab.data() + (B + 1), rp->sum), KPRN_E_ARG,
               "counts: every pair needs 1..4096 paths and the counts must add up to N");
}

static void set_ragged(kprn_batch* b, RaggedPlan* rp) {
  b->hrag.swap(rp->tab); b->n_wg = rp->sum[0]; b->max_cnt = rp->sum[1]; b->seg_wave = rp->sum[2];
}

// a new batch, ready on return: built by the device kernels on the handle's stream.  counts != null: ragged, N paths (P is ignored); else B * P paths
// fill != null (and idx null): the ids come from the device (kprn_internal.h DeviceFill)
void create(kprn_handle* h, const int32_t* idx, const int32_t* counts, const float* labels, int32_t B, int32_t P, int64_t N, int32_t T, int32_t F,
            kprn_batch** out, const DeviceFill* fill) {
  *out = nullptr;
  RaggedPlan rp;
  check_fill(h, idx, counts, B, &P, N, T, F, &rp, fill != nullptr);
  if (!counts) N = (int64_t)B * P;
  kprn_batch* b = new kprn_batch();
  try {
    reserve(h, b, B, P, T, F, labels != nullptr, 0, 0, counts ? N : 0);
    if (counts) set_ragged(b, &rp);
    b->has_index = true; b->idx_valid = true;
    const size_t need = std::max(bidx::scratch_bytes(b->n_index, h->cfg.Ve), bidx::prefix_scratch_bytes(N, fused::KCAP));
    grow_device(h->bidx_scratch, h->bidx_scratch_bytes, need, need * 2, need * 2, {});   // (no wait, as before: the users of this scratch drain the stream)
    enqueue(h, b, idx, labels, h->stream, h->bidx_scratch, h->bidx_scratch_bytes, fill);
    HIP_TRY(hipStreamSynchronize(h->stream));
    finish(h, b);
  } catch (...) {
    release(b);
    throw;
  }
  *out = b;
}

// host-built feed: a worker thread runs hostfeed::build into a page-locked image of the slot's device block; ONE upload thread
// then moves each image with ONE copy, behind the positions the main / scoring streams had when the refill was requested, and
// keeps a single copy in flight (several streams' worth of small concurrent copies fell back from the DMA engines to copy
// kernels, which take CUs from the persistent kernels: measured, profiles/r02)
// inline_now (the host-buffer entry points kprn_train_step / kprn_forward, which return results and therefore wait for the feed anyway): derive on the
// CALLING thread and copy on the engine's own stream -- no worker hand-over, no upload thread, no cross-stream events (a 128-pair minibatch is
// microseconds of host work; the thread hand-overs were most of its feed time)
// The upload stream, made once -- by whichever feed path needs it first (the inline side upload of kprn_train_step or the worker-built feed; a second
// creation would drop the first handle with copies still queued on it, outside sync_all_streams' and kprn_destroy's reach).  A queue of its own: HIP
// multiplexes the streams of one priority onto a few hardware queues, and this stream spends its life waiting on events of the compute streams --
// sharing a hardware queue with one of them stalls that stream's kernels behind the waits (measured: every kernel of the step 1.2-5x slower).  The
// high-priority class has its own queues.
static void ensure_upload_stream(kprn_handle* h) {
  if (!h->upload_stream) h->upload_stream = make_priority_stream(/*high=*/true);
}

static void feed_host(kprn_handle* h, kprn_batch* b, const int32_t* idx, const float* labels, const int64_t* rows, bool inline_now = false) {
  const int32_t B = b->B, P = b->P, T = b->T, F = b->F;
  const int64_t N = b->N, nsteps = N * T, n_index = b->n_index;
  const bool ragged = b->off != nullptr;
  if (!h->feed_pool && !inline_now) {
    if (h->feed_workers <= 0) {  // defaults from the machine: a GPU host has cores to spare, a small container does not
      const unsigned hc = std::thread::hardware_concurrency();
      h->feed_workers = hc >= 32 ? 4 : 2;
      if (h->feed_threads <= 0) h->feed_threads = hc >= 64 ? 8 : (hc >= 16 ? 4 : 2);
    }
    if (h->feed_threads <= 0) h->feed_threads = 4;
    h->feed_pool = hostfeed::make_pool(std::max(1, h->feed_workers));
    h->upload_pool = hostfeed::make_pool(1);
    ensure_upload_stream(h);
  }
  if (!b->ev_fork) {
    HIP_TRY(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&b->ev_fork2, hipEventDisableTiming));
  }
  const bool plan = b->kcap > 0;
  const BatchLayout l = layout(B, N, T, F, plan, labels != nullptr, ragged);
  // a label-less batch is scored only: with no lazy row update pending nothing walks its entity rows -> no occurrence index is
  // built, and with a plan the ids in their original order are not uploaded either (a third of the bytes, none of the sorting)
  const bool want_index = labels != nullptr || h->lazy_pending;
  const bool want_idx = want_index || !plan;
  b->has_index = want_index; b->idx_valid = want_idx;
  if (b->block_cap > b->hs_cap) {  // the image is as large as the block: a reserved slot allocates it once
    if (b->hs) hipHostFree(b->hs);
    b->hs = nullptr; b->hs_cap = 0;
    HIP_TRY(hipHostMalloc((void**)&b->hs, (size_t)b->block_cap * sizeof(int32_t)));
    b->hs_cap = b->block_cap;
  }
  if ((int64_t)b->hw.size() < 4 * n_index) b->hw.resize((size_t)(4 * std::max(n_index, (b->block_cap / 8))));
  // (validation, plan and index are flat over the paths: a ragged batch is N "pairs" of one path to them)
  const hostfeed::Shape g{ragged ? (int)N : B, ragged ? 1 : P, T, F, h->cfg.num_types, h->cfg.Vt, h->cfg.Ve, h->cfg.Vr};
  const int kcap = b->kcap, dev = h->cfg.device_id;
  int32_t* hs = b->hs;
  int32_t* hw = b->hw.data();
  if (labels && rows) { float* hl = (float*)(hs + l.labels); for (int32_t i = 0; i < B; ++i) hl[i] = labels[rows[i]]; }
  else if (labels) memcpy(hs + l.labels, labels, (size_t)B * sizeof(float));
  hs[l.flag] = 0;
  if (ragged) {
    memcpy(hs + l.off, b->hrag.data(), (size_t)(B + 1) * sizeof(int32_t));
    memcpy(hs + l.wg, b->hrag.data() + (B + 1), (size_t)(b->n_wg + 1) * sizeof(int32_t));
  }
  b->host_built = true;
  auto done = std::make_shared<std::promise<void>>();
  b->job = done->get_future();
  // the host work of a fill, on nth threads: gather the rows (pair i of the minibatch = row rows[i] of the file's array, straight into the image), derive
  // validation + plan + index, complete the image
  auto derive = [=](int nth) {
    kprn_batch::HostResult* r = &b->hres;
    const int32_t* src = idx;
    if (rows) { hostfeed::gather_rows(hs + l.idx, idx, (int64_t)P * T * F, rows, B, nth); src = hs + l.idx; }
    hostfeed::build(g, src, kcap, nth, want_index, r, hs + l.idx_s, hs + l.perm, hs + l.slot_of, hs + l.tile_k, hs + l.pmeta, hs + l.key, hs + l.pos,
                    hs + l.uniq, hw, hw + n_index, hw + 2 * n_index, hw + 3 * n_index);
    if (r->bad) return;
    if (want_idx && !rows) memcpy(hs + l.idx, idx, (size_t)(nsteps * F) * sizeof(int32_t));
    hs[l.cnt] = r->n_uniq;
  };
  // the image is contiguous: idx | idx_s .. pmeta | key | pos | uniq | count | labels | flag -- ONE copy; a scoring-only batch moves the plan part
  auto upload = [=](hipStream_t s) {
    const int64_t w0 = want_idx ? 0 : l.idx_s, w1 = want_index ? l.words : l.key;
    HIP_TRY(hipMemcpyAsync(b->block + w0, hs + w0, (size_t)(w1 - w0) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  };
  if (inline_now) {
    try {
      // where the upload runs: beside the step in flight when nothing can still read this slot (kprn_internal.h: dropin_prev_waited), else in stream order
      const bool side_copy = h->inline_upload_side && labels != nullptr && h->dropin_prev_waited_now && h->inline_side_ok;
      hipStream_t cs = h->stream;
      const int nth1 = nsteps < 65536 ? 1 : std::max(1, h->feed_threads > 0 ? h->feed_threads : 4);
      derive(nth1);
      if (!b->hres.bad) {
        if (side_copy) ensure_upload_stream(h);
        cs = side_copy ? h->upload_stream : h->stream;
        if (h->score_pending && h->score_stream) HIP_TRY(hipStreamWaitEvent(cs, h->ev_score_done, 0));   // (a pass on the side stream may still read the slot)
        upload(cs);
      }
      HIP_TRY(hipEventRecord(b->ev_ready, cs));   // (ready orders the engine's stream behind it)
      done->set_value();
    } catch (...) { done->set_exception(std::current_exception()); }
    return;
  }
  const int nth = std::max(1, h->feed_threads);
  HIP_TRY(hipEventRecord(b->ev_fork, h->stream));
  const bool wait_score = h->score_pending && h->score_stream;
  if (wait_score) HIP_TRY(hipEventRecord(b->ev_fork2, h->score_stream));
  hostfeed::Pool* up_pool = (hostfeed::Pool*)h->upload_pool;
  hipStream_t us = h->upload_stream;
  hostfeed::submit((hostfeed::Pool*)h->feed_pool, [=]() {
    try { derive(nth); } catch (...) { done->set_exception(std::current_exception()); return; }
    hostfeed::submit(up_pool, [=]() {
      bool issued = false;
      try {
        HIP_TRY(hipSetDevice(dev));
        if (!b->hres.bad) {
          HIP_TRY(hipStreamWaitEvent(us, b->ev_fork, 0));
          if (wait_score) HIP_TRY(hipStreamWaitEvent(us, b->ev_fork2, 0));
          upload(us);
        }
        HIP_TRY(hipEventRecord(b->ev_ready, us));
        issued = true;
        done->set_value();
        HIP_TRY(hipStreamSynchronize(us));  // one image in flight at a time
      } catch (...) { if (!issued) done->set_exception(std::current_exception()); }
    });
  });
}

// What the handle may still reference in slot b, and what becomes of each reference before b's contents are replaced (refill), given up (reserve: a larger
// block, no contents until the next feed) or b itself goes away (destroy).  Every reader of the old contents was enqueued before this call; the caller orders
// the new fill behind them (feed) or drains the streams before it frees anything (reserve, kprn_batch_destroy).  destroy never throws: a step that fails leaves
// its reference cleared.
enum class Why { refill, reserve, destroy };
static void detach(kprn_handle* h, kprn_batch* b, Why why) {
  auto step = [&](auto&& fn, auto&& failed) {
    if (why != Why::destroy) { fn(); return; }
    try { fn(); } catch (...) { failed(); }
  };
  // 1. the deferred part of a split (or "score_dual") scoring pass still reads the old contents: it goes out now
  if (h->score_rest_batch == b) step([&] { launch_score_rest(h); }, [&] { h->score_rest_batch = nullptr; });
  // 2. the optimiser's row list is a view of b's distinct rows: it moves to the handle's own storage
  if (h->view_batch == b) {
    // refill only: with no gradients waiting for an update nothing names these rows any more and the view is dropped -- a refill runs once per step, the
    // copy would be two launches of every step; reserve and destroy run outside the step loop and always copy
    if (why == Why::refill && !h->ent_grads_dirty) { h->view_batch = nullptr; h->rows_view = h->step_rows; h->count_view = h->step_count; h->step_rows_ub = 0; }
    else step([&] { materialize_step_rows(h); }, [&] { h->view_batch = nullptr; h->rows_view = nullptr; h->step_rows_ub = 0; });
  }
  // 3. "b's entity rows are current" stops being true of whatever b holds next
  if (h->caught_serial == b->serial) h->caught_serial = -1;
  // 4. destroy only: the pooling stage a failed step left behind (between its forward and its loss stage) would name a freed batch; a slot that stays stays named
  if (why == Why::destroy && h->pool_defer_batch == b) h->pool_defer_batch = nullptr;
  // 5. a host-built fill nobody used: its job is joined.  refill hands the job's error to its caller (its previous fill failed); reserve and destroy swallow it
  if (why == Why::refill) { if (b->pending && b->host_built) b->job.get(); }
  else if (b->job.valid()) { try { b->job.get(); } catch (...) {} }
  // refill only, also when the slot was used: its uploads read the page-locked staging the next fill overwrites (the feed's back-pressure on a host running ahead)
  if (why == Why::refill && b->ev_ready && (b->pending || b->host_built)) HIP_TRY(hipEventSynchronize(b->ev_ready));
  b->pending = false;
  // 6. the group table of the pairwise loss (kprn_batch_set_groups) names the old contents' pairs: dropped; its storage stays with the slot
  b->n_groups = 0; b->n_terms = 0;
}

// body(b, fresh) on the slot's batch, or on a new one that becomes the slot's -- unless body throws: then it is released again and *slot stays as it was
template <class Body>
static void with_slot(kprn_batch** slot, Body&& body) {
  kprn_batch* b = *slot;
  const bool fresh = (b == nullptr);
  if (fresh) b = new kprn_batch();
  try { body(b, fresh); } catch (...) { if (fresh) release(b); throw; }
  *slot = b;
}

void feed(kprn_handle* h, kprn_batch** slot, const int32_t* idx, const float* labels, const int64_t* rows, int32_t B, int32_t P, int32_t T, int32_t F,
          bool inline_now, const int32_t* counts, int64_t n_ragged) {
  KPRN_REQUIRE(slot, KPRN_E_ARG, "slot is NULL");
  RaggedPlan rp;
  check_fill(h, idx, counts, B, &P, n_ragged, T, F, &rp);
  if (!h->feed_build_host && !h->feed_stream) {
    // device-built feed: its kernels are small and latency-bound; they get the CUs the persistent kernels leave idle in their
    // tails.  (Created only when used: HIP multiplexes streams onto a few hardware queues, and a stream that waits on events --
    // as the feed's do -- blocks whatever shares its queue.)
    h->feed_stream = make_priority_stream(/*high=*/true);
    HIP_TRY(hipEventCreateWithFlags(&h->ev_feed_fork, hipEventDisableTiming));
  }
  with_slot(slot, [&](kprn_batch* b, bool fresh) {
    h->inline_side_ok = !fresh && h->score_rest_batch != b && h->view_batch != b;   // (a fresh slot allocates: in stream order)
    if (!fresh) detach(h, b, Why::refill);   // (the feed stream starts behind the old contents' last readers, below)
    reserve(h, b, B, P, T, F, labels != nullptr, 0, 0, counts ? n_ragged : 0);
    if (counts) set_ragged(b, &rp);
    if (!b->ev_ready) HIP_TRY(hipEventCreateWithFlags(&b->ev_ready, hipEventDisableTiming));
    if (h->feed_build_host) {
      feed_host(h, b, idx, labels, rows, inline_now);
    } else {
      b->host_built = false; b->has_index = true; b->idx_valid = true;
      const int64_t N = b->N;
      const size_t need = std::max(bidx::scratch_bytes(b->n_index, h->cfg.Ve), bidx::prefix_scratch_bytes(N, fused::KCAP));
      grow_device(h->feed_scratch, h->feed_scratch_bytes, need, need * 2, need * 2, {h->feed_stream}, /*wait_if_empty=*/true);
      // everything enqueued on the handle so far (the last readers of this slot among it) comes first
      HIP_TRY(hipEventRecord(h->ev_feed_fork, h->stream));
      HIP_TRY(hipStreamWaitEvent(h->feed_stream, h->ev_feed_fork, 0));
      if (h->score_pending) HIP_TRY(hipStreamWaitEvent(h->feed_stream, h->ev_score_done, 0));
      const int32_t* src = idx;
      const float* lsrc = labels;
      if (rows) {   // device build: the rows are gathered by the calling thread into the slot's host scratch first
        const int64_t rw = (int64_t)P * T * F;
        if ((int64_t)b->hw.size() < (int64_t)B * rw + B) b->hw.resize((size_t)((int64_t)B * rw + B));
        hostfeed::gather_rows(b->hw.data(), idx, rw, rows, B, std::max(1, h->feed_threads));
        src = b->hw.data();
        if (labels) { float* hl = (float*)(b->hw.data() + (int64_t)B * rw); for (int32_t i = 0; i < B; ++i) hl[i] = labels[rows[i]]; lsrc = hl; }
      }
      enqueue(h, b, src, lsrc, h->feed_stream, h->feed_scratch, h->feed_scratch_bytes);
      HIP_TRY(hipEventRecord(b->ev_ready, h->feed_stream));
    }
    b->pending = true;
  });
}

}  // namespace slots

extern "C" {
int kprn_batch_create(kprn_handle* h, const int32_t* idx, const float* labels, int32_t B, int32_t P, int32_t T, int32_t F, kprn_batch** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out, KPRN_E_ARG, "out is NULL");
  slots::create(h, idx, nullptr, labels, B, P, 0, T, F, out);
  API_END(h)
}

int kprn_batch_create_ragged(kprn_handle* h, const int32_t* idx, const int32_t* counts, const float* labels, int32_t B, int64_t N, int32_t T, int32_t F,
                             kprn_batch** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out, KPRN_E_ARG, "out is NULL");
  *out = nullptr;
  KPRN_REQUIRE(idx, KPRN_E_ARG, "idx is NULL");
  KPRN_REQUIRE(counts, KPRN_E_ARG, "counts is NULL");   // (null counts would select the rectangular route)
  slots::create(h, idx, counts, labels, B, 0, N, T, F, out);
  API_END(h)
}

int kprn_host_ragged_plan(const int32_t* counts, int32_t B, int64_t N, int32_t* offsets, int32_t* wg_first, int32_t* summary) {
  int32_t sm[3];
  if (!summary) return KPRN_E_ARG;
  if (!kk::ragged_plan(counts, B, N, offsets, wg_first, sm)) return KPRN_E_ARG;
  summary[0] = sm[0]; summary[1] = sm[1]; summary[2] = sm[2];
  summary[3] = kk::RAGGED_MAX_SEG; summary[4] = kk::RAGGED_THREAD_MAX; summary[5] = kk::RAGGED_WG_PATHS; summary[6] = kk::RAGGED_WG_PAIRS; summary[7] = 0;
  return KPRN_OK;
}

// The group table of the pairwise loss (include/kprn.h "pairwise loss"): checked on the host, uploaded into storage the batch owns, its terms counted on the
// device; one wait.  Nothing of the batch changes before the table has passed its checks.
int kprn_batch_set_groups(kprn_handle* h, kprn_batch* b, const int32_t* group_offsets, int32_t G, int64_t* n_terms) {
  API_BEGIN(h)
  KPRN_REQUIRE(b != nullptr, KPRN_E_ARG, "batch is NULL");
  slots::ready(h, b);
  KPRN_REQUIRE(b->labels != nullptr, KPRN_E_ARG, "kprn_batch_set_groups: the batch has no labels");
  if (const char* why = kk::pairwise_groups_why(group_offsets, G, b->B)) throw KprnError{KPRN_E_ARG, std::string("kprn_batch_set_groups: ") + why};
  const int64_t need = (int64_t)G + 3;
  if (need > b->groups_cap) {
    int32_t* grown = dalloc<int32_t>(need * 2);
    if (b->groups) { HIP_TRY(hipStreamSynchronize(h->stream)); dfree(b->groups); }   // (a loss stage still queued reads the old table)
    b->groups = grown; b->groups_cap = need * 2;
  }
  b->n_groups = 0;
  HIP_TRY(hipMemcpyAsync(b->groups + 2, group_offsets, (size_t)(G + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  kk::count_pair_terms(h->stream, b->labels, b->groups + 2, G, (int64_t*)b->groups);
  int64_t terms = 0;
  HIP_TRY(hipMemcpyAsync(&terms, b->groups, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  b->n_groups = G; b->n_terms = terms;
  if (n_terms) *n_terms = terms;
  API_END(h)
}

int kprn_batch_num_paths(kprn_handle* h, const kprn_batch* b, int64_t* n) {
  API_BEGIN(h)
  KPRN_REQUIRE(b && n, KPRN_E_ARG, "NULL argument");
  *n = b->N;
  API_END(h)
}

int kprn_batch_read_idx(kprn_handle* h, const kprn_batch* b, int32_t* idx_out) {
  API_BEGIN(h)
  KPRN_REQUIRE(b && idx_out, KPRN_E_ARG, "NULL argument");
  slots::ready(h, b);
  const int64_t N = b->N, row = (int64_t)b->T * b->F;
  if (b->idx_valid) {
    HIP_TRY(hipMemcpyAsync(idx_out, b->idx, (size_t)(N * row) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  } else {
    // (a label-less fed batch with a plan keeps the reordered ids only: path perm[s] is row s of idx_s)
    KPRN_REQUIRE(b->idx_s && b->perm, KPRN_E_ARG, "the batch holds no ids");
    std::vector<int32_t> rows((size_t)(N * row)), perm((size_t)N);
    HIP_TRY(hipMemcpyAsync(rows.data(), b->idx_s, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(perm.data(), b->perm, perm.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int64_t s = 0; s < N; ++s) memcpy(idx_out + (int64_t)perm[s] * row, rows.data() + s * row, (size_t)row * sizeof(int32_t));
  }
  API_END(h)
}

int kprn_batch_feed_async(kprn_handle* h, kprn_batch** slot, const int32_t* idx, const float* labels, int32_t B, int32_t P, int32_t T, int32_t F) {
  API_BEGIN(h)
  slots::feed(h, slot, idx, labels, nullptr, B, P, T, F);
  API_END(h)
}

int kprn_batch_feed_ragged_async(kprn_handle* h, kprn_batch** slot, const int32_t* idx, const int32_t* counts, const float* labels, int32_t B, int64_t N,
                                 int32_t T, int32_t F) {
  API_BEGIN(h)
  KPRN_REQUIRE(counts, KPRN_E_ARG, "counts is NULL");
  slots::feed(h, slot, idx, labels, nullptr, B, 0, T, F, false, counts, N);
  API_END(h)
}

int kprn_batch_feed_rows_async(kprn_handle* h, kprn_batch** slot, const int32_t* data, const float* labels, int64_t n_rows, const int64_t* rows, int32_t B,
                               int32_t P, int32_t T, int32_t F) {
  API_BEGIN(h)
  KPRN_REQUIRE(rows, KPRN_E_ARG, "rows is NULL");
  for (int32_t i = 0; i < B; ++i) KPRN_REQUIRE(rows[i] >= 0 && rows[i] < n_rows, KPRN_E_ARG, "a row index is outside 0..n_rows-1");
  slots::feed(h, slot, data, labels, rows, B, P, T, F);
  API_END(h)
}

int kprn_batch_slot_reserve(kprn_handle* h, kprn_batch** slot, int32_t max_pairs, int64_t max_paths, int32_t T, int32_t F, int32_t with_labels) {
  API_BEGIN(h)
  KPRN_REQUIRE(slot && max_pairs > 0 && max_paths >= max_pairs && T > 0, KPRN_E_ARG, "bad argument");
  KPRN_REQUIRE(F == h->cfg.F, KPRN_E_ARG, "F does not match numFeatureTemplates");
  slots::with_slot(slot, [&](kprn_batch* b, bool fresh) {
    if (!fresh) slots::detach(h, b, slots::Why::reserve);
    b->bad = true;   // (no contents until the next feed; set before anything below can throw)
    const int32_t P1 = (int32_t)std::max<int64_t>(1, max_paths / max_pairs);
    slots::reserve(h, b, max_pairs, P1, T, F, with_labels != 0, max_pairs, max_paths);
  });
  API_END(h)
}

int kprn_host_batch_index(const int32_t* idx, int32_t B, int32_t P, int32_t T, int32_t F, int32_t num_types, int32_t Vt, int32_t Ve, int32_t Vr,
                          int32_t plan, int32_t threads, int32_t* idx_s, int32_t* perm, int32_t* slot_of, int32_t* tile_k, int32_t* pmeta,
                          int32_t* key_sorted, int32_t* pos_sorted, int32_t* uniq, int64_t* summary) {
  if (!idx || B <= 0 || P <= 0 || T <= 0 || F < num_types + 2 || num_types < 1 || !key_sorted || !pos_sorted || !uniq || !summary) return KPRN_E_ARG;
  if (plan && (T < 2 || F > 16 || !idx_s || !perm || !slot_of || !tile_k || !pmeta)) return KPRN_E_ARG;
  try {
    const int kcap = plan ? fused::KCAP : 0;
    const int64_t n_index = (int64_t)B * P * T + kcap;
    std::vector<int32_t> w((size_t)(4 * n_index));
    kprn_batch::HostResult r;
    const hostfeed::Shape g{B, P, T, F, num_types, Vt, Ve, Vr};
    hostfeed::build(g, idx, kcap, std::max(1, (int)threads), true, &r, idx_s, perm, slot_of, tile_k, pmeta, key_sorted, pos_sorted, uniq, w.data(),
                    w.data() + n_index, w.data() + 2 * n_index, w.data() + 3 * n_index);
    summary[0] = r.bad ? 1 : 0; summary[1] = r.kmax; summary[2] = r.n_uniq; summary[3] = r.exec_steps;
  } catch (...) { return KPRN_E_NOMEM; }
  return KPRN_OK;
}

int kprn_host_alloc(kprn_handle* h, size_t bytes, void** out) {
  API_BEGIN(h)
  KPRN_REQUIRE(out && bytes > 0, KPRN_E_ARG, "bad argument");
  *out = nullptr;
  hipError_t e = hipHostMalloc(out, bytes);
  if (e != hipSuccess) throw KprnError{KPRN_E_NOMEM, std::string("hipHostMalloc failed: ") + hipGetErrorString(e)};
  API_END(h)
}

int kprn_host_free(kprn_handle* h, void* p) {
  API_BEGIN(h)
  if (p) HIP_TRY(hipHostFree(p));
  API_END(h)
}

void kprn_batch_destroy(kprn_handle* h, kprn_batch* b) {
  if (!b) return;
  if (h) {
    hipSetDevice(h->cfg.device_id);
    slots::detach(h, b, slots::Why::destroy);
    sync_all_streams(h, /*nothrow=*/true);   // (an upload, a feed or a scoring pass on any stream may still read the batch)
  }
  slots::release(b);
}

int kprn_batch_distinct_rows(kprn_handle* h, const kprn_batch* b, int32_t* n) {
  API_BEGIN(h)
  KPRN_REQUIRE(b && n, KPRN_E_ARG, "NULL argument");
  slots::ready(h, b);
  *n = b->n_uniq;
  API_END(h)
}

int kprn_batch_executed_steps(kprn_handle* h, const kprn_batch* b, int64_t* steps) {
  API_BEGIN(h)
  KPRN_REQUIRE(b && steps, KPRN_E_ARG, "NULL argument");
  slots::ready(h, b);
  *steps = b->exec_steps;
  API_END(h)
}

int kprn_batch_handover_stats(kprn_handle* h, const kprn_batch* b, int64_t* out) {
  API_BEGIN(h)
  KPRN_REQUIRE(b && out, KPRN_E_ARG, "NULL argument");
  slots::ready(h, b);
  out[0] = out[1] = out[2] = out[3] = 0;
  if (use_fused(h, b, true) && h->cfg.compute_dtype == 0) fused::handover_stats(h, b, out);
  API_END(h)
}

}  // extern "C"
