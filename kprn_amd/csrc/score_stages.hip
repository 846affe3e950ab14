// libkprn.so -- the scoring stage: everything that serves a scoring pass and what is done with its result.  Passes beside the main stream
// (kprn_forward_batch_async and its deferred rest), the synchronous passes (kprn_forward_batch, kprn_forward, kprn_forward_ragged), the score board, the ranking
// and explanation calls and the one-call routes.  Kernels: lstm_fused_fwd*.hip, rank_groups.hip, rank_targets.hip, explain_paths.hip.  The pass itself and what it shares with
// training (forward_impl, pool_stage, dropin_feed) live in kprn_api.hip, the catch-up of a batch's rows in optim_step.hip.
//
// Streams.  main = h->stream: training, the synchronous passes, every ranking and explanation launch.  score = h->score_stream (option "score_overlap"; probed
// to run beside main): an asynchronous pass, or the first part of a split one; the copies of kprn_read_probs and kprn_board_put out of sel2.  rest =
// h->rest_stream (option "score_rest_before_bptt"; lowest priority): the deferred part of a split pass; without the option that part runs on score.
// A pass off the main stream writes S2 / sel2 (score::SideBuffers), never ws.S / ws.sel.
//
// Events, each with who records it and who waits for it.
//   ev_fork        recorded on main: kprn_forward_batch_async before its pass, launch_score_rest before the rest, score::order_behind_pass for a "score_dual" pass.
//                  waited for by the stream the work goes to (score, or rest): it starts behind everything queued on main so far.
//   ev_score_done  recorded behind a pass's pooling stage: on score by kprn_forward_batch_async (whole pass), on score or rest by launch_score_rest.  A "score_dual"
//                  pass that rode in a training forward's launch records nothing (score_on_main; forward_impl).
//                  waited for by main in join_score (while score_pending); by score at the start of the next asynchronous pass, which writes the same S2 / sel2,
//                  and in score::order_behind_pass; by the feed and copy streams of batch_slots.hip before they refill a slot the pass reads.
//   ev_part1       recorded on score behind the first part of a split pass, when the rest will run on rest.
//                  waited for by rest in launch_score_rest: the rest's pooling stage reads the first part's scores.
//   ev_put         recorded on score behind kprn_board_put's copy out of sel2 (put_side).
//                  waited for by main in score::join_put: before the board is read or written from main, and before a "score_dual" pass writes sel2 from main.
//
// Known and open (finding 2; not fixed here): a "score_dual" pass writes S2 / sel2 from MAIN, and an earlier pass still running on score or rest is
// ordered before it only through score's wait for ev_score_done in kprn_forward_batch_async -- the wrong stream.  async(A) on the side, async(B) deferred,
// train_step(B): A's late writes race with B's.  The fix is a wait of main for ev_score_done in front of fused::forward_dual (kprn_api.hip forward_impl).
#include <string.h>

#include <algorithm>

#include "kprn_internal.h"
#include "rank_targets_host.h"

namespace score {
// while it lives, "the handle's stream and score buffers" are the given side stream and S2 / sel2: what fused::forward and pool_stage launch goes there
struct SideBuffers {
  kprn_handle* h; hipStream_t stream0; float* S0; float* sel0;
  SideBuffers(kprn_handle* h_, hipStream_t side) : h(h_), stream0(h_->stream), S0(h_->ws.S), sel0(h_->ws.sel) { h->stream = side; h->ws.S = h->S2; h->ws.sel = h->sel2; }
  ~SideBuffers() { h->stream = stream0; h->ws.S = S0; h->ws.sel = sel0; }
};

// The selected class's probabilities of a synchronous pass (what model:forward hands test_from_checkpoint.lua:109) come back through a page-locked mirror the
// pool kernel writes: no copy operation between the pass and the caller.  Armed from here until the call ends, however it ends.  With the profiler on
// the mirror is off and the probabilities are copied out of ws.sel, as the other outputs are
struct ProbsMirror {
  kprn_handle* h; float* probs; int64_t B; bool on;
  ProbsMirror(kprn_handle* h_, float* probs_, int64_t B_) : h(h_), probs(probs_), B(B_), on(probs_ != nullptr && !h_->prof_on) {
    if (!on) return;
    grow_pinned(h->probs_mirror, h->probs_mirror_cap, B, (size_t)(2 * B + 64) * sizeof(float), 2 * B + 64, {h->stream});
    h->sel_host_armed = h->probs_mirror;
  }
  ~ProbsMirror() { h->sel_host_armed = nullptr; }
  void queue_copy() { if (probs && !on) HIP_TRY(hipMemcpyAsync(probs, h->ws.sel, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream)); }   // behind the pass
  void hand_out() { if (on) memcpy(probs, h->probs_mirror, (size_t)B * sizeof(float)); }                                                                // after the wait
};

// the scoring stream is ordered behind the pass whose result sel2 holds: what a copy out of sel2 queued there next needs
static void order_behind_pass(kprn_handle* h) {
  if (h->score_rest_batch) launch_score_rest(h);
  // (the second part of a split pass may have run on the rest stream, and a join may already have cleared score_pending: the pass's event orders the copy)
  if (h->score_on_main) {   // ("score_dual": the pass ran in a training forward's launch on the main stream)
    HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->score_stream, h->ev_fork, 0));
  } else if (h->ev_score_done) HIP_TRY(hipStreamWaitEvent(h->score_stream, h->ev_score_done, 0));
}
}  // namespace score

// scoring overlap: the main stream waits for the pass running on the side stream (before anything that changes what that pass
// reads -- parameters, the prefix table -- and before the backward kernels, which want the chip to themselves)
void join_score(kprn_handle* h) {
  if (h->score_rest_batch) launch_score_rest(h);   // (a split pass whose second part nobody placed: it goes now)
  if (!h->score_pending) return;
  HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_score_done, 0));
  h->score_pending = false;
}

// ranking stage: the main stream waits for the board puts queued on the scoring stream (before it reads the board, and before a pass that runs on the
// main stream writes the side buffers those puts read: "score_dual")
void score::join_put(kprn_handle* h) {
  if (!h->put_side) return;
  HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_put, 0));
  h->put_side = false;
}
using score::join_put;

// ---- a side stream that really runs beside the main stream ---------------------------------------------------------------------
// HIP multiplexes its streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default; assigned round-robin as streams are made),
// and two streams that land on the same queue execute IN ORDER.  In a process that also holds torch's and RCCL's streams the scoring
// pass's stream shared the main stream's queue in about every other run: the pass then ran strictly before the training forward
// (profiles/r03: 0.41 + 0.41 ms instead of 0.74 ms for the overlapped pair).  So the stream is probed: a kernel on the main stream
// waits (bounded, 200 us) for a flag that a kernel on the candidate sets; if the flag never arrives the two share a queue and the
// next candidate is tried (every new stream advances the round-robin).
extern "C" {
__global__ void k_probe_wait(int* flag, int* seen, long long max_ticks) {
  const long long t0 = wall_clock64();   // (100 MHz)
  int f = 0;
  while (!(f = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) && wall_clock64() - t0 < max_ticks) __builtin_amdgcn_s_sleep(32);
  *seen = f;
}
__global__ void k_probe_set(int* flag) { __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

}  // extern "C"
hipStream_t make_concurrent_stream(kprn_handle* h, int* probes) {
  const int kTries = 8;
  hipStream_t cand[kTries] = {};
  int32_t* d = dalloc<int32_t>(2);   // {flag, seen}
  hipStream_t pick = nullptr;
  int made = 0;
  try {
    for (int i = 0; i < kTries && !pick; ++i) {
      HIP_TRY(hipStreamCreateWithFlags(&cand[i], hipStreamNonBlocking));
      made = i + 1;
      HIP_TRY(hipMemsetAsync(d, 0, 2 * sizeof(int32_t), h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, h->stream, d, d + 1, (long long)20000);
      hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, cand[i], d);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(h->stream));
      HIP_TRY(hipStreamSynchronize(cand[i]));
      int32_t seen = 0;
      HIP_TRY(hipMemcpy(&seen, d + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
      if (seen) pick = cand[i];
    }
  } catch (...) {
    for (int i = 0; i < made; ++i) if (cand[i]) hipStreamDestroy(cand[i]);
    dfree(d);
    throw;
  }
  if (probes) *probes = made; else h->side_stream_probes = made;   // (default: the scoring stream's count, what kprn_get_stat reports)
  if (!pick) pick = cand[0];   // (every candidate shares the main stream's queue: correct anyway, just not concurrent)
  for (int i = 0; i < made; ++i) if (cand[i] && cand[i] != pick) hipStreamDestroy(cand[i]);
  dfree(d);
  return pick;
}

extern "C" {

int kprn_forward_batch_async(kprn_handle* h, const kprn_batch* b, int32_t class_id) {
  API_BEGIN(h)
  if (h->score_rest_batch) launch_score_rest(h);   // (the second part of an earlier split pass that nobody placed: before its buffers are reused)
  h->pool_defer_batch = nullptr;
  h->last_forward_side = false;
  if (h->score_overlap && b && use_fused(h, b, false)) {
    // the pass goes to the side stream with its own output buffers; everything it reads is final on the main stream first
    check_batch(h, b, class_id);
    const int64_t N = b->N;
    optim::catch_up(h, b);
    ensure_ws_common(h, N, b->B);
    if (!h->score_stream) {
      h->score_stream = make_concurrent_stream(h);
      HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_score_done, hipEventDisableTiming));
    }
    if (N > h->cap_N2 || b->B > h->cap_B2) {
      sync_side_streams(h);
      dfree(h->S2); dfree(h->sel2);
      h->cap_N2 = std::max(N, h->cap_N2); h->cap_B2 = std::max<int64_t>(b->B, h->cap_B2);
      h->S2 = dalloc<float>(h->cap_N2 * h->cfg.C);
      h->sel2 = dalloc<float>(h->cap_B2);
    }
    fused::prefix_forward(h, b);  // (main stream; cached for the pass below and for the training forward of the same batch)
    fused::mc_prepare(h);         // (likewise: the split weights of the matrix-core forward)
    if ((h->score_dual == 1 || (h->score_dual == 2 && fused::small_tiles(h, N, b->tile_k != nullptr))) && h->cfg.compute_dtype == 0 && h->cfg.L == 2 &&
        !(h->score_split > 0.f)) {
      // "score_dual": the WHOLE pass waits for the training forward that usually comes next and rides in its launch (forward_impl, fused::forward_dual) --
      // deferred like the second part of a split pass (tile 0 on): whoever needs its result, its buffers or the parameters it reads first runs it the usual
      // way (join_score -> launch_score_rest)
      if (h->score_pending && h->ev_score_done) HIP_TRY(hipStreamWaitEvent(h->score_stream, h->ev_score_done, 0));   // (an earlier pass wrote the same S2 / sel2)
      h->score_rest_batch = b; h->score_rest_cid = class_id; h->score_rest_tile0 = 0;
      h->score_on_main = false;
      h->score_pending = true;
      h->last_forward_side = true;
      h->last_B = b->B;
      return KPRN_OK;
    }
    h->score_on_main = false;
    HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->score_stream, h->ev_fork, 0));
    // an earlier pass (or its deferred part, which may have run on the rest stream: "score_rest_before_bptt") writes the same S2 / sel2: this pass
    // starts behind it whichever stream it finished on
    if (h->score_pending && h->ev_score_done) HIP_TRY(hipStreamWaitEvent(h->score_stream, h->ev_score_done, 0));
    // "score_split" f: the last f of the batch's tiles wait for kprn_forward_batch_async_rest (a data-parallel step places them under its
    // collective); the first part runs now, beside whatever is queued next, on the whole chip
    const int64_t n_tiles = (N + 63) / 64;
    const int64_t t_split = (h->score_split > 0.f && h->cfg.compute_dtype == 0 && n_tiles >= 64 && !fused::small_tiles(h, N, b->tile_k != nullptr))
                                ? std::max<int64_t>(1, std::min<int64_t>(n_tiles - 1, (int64_t)((1.0 - h->score_split) * n_tiles + 0.5))) : n_tiles;
    {
      score::SideBuffers on_side(h, h->score_stream);
      fused::forward(h, b, false, 0, t_split < n_tiles ? t_split : -1, t_split < n_tiles, class_id - 1);   // (kprn_read_probs / kprn_board_put: the selected class)
      if (t_split == n_tiles) pool_stage(h, b, class_id - 1, false);
    }
    if (t_split < n_tiles) {
      h->score_rest_batch = b; h->score_rest_cid = class_id; h->score_rest_tile0 = t_split;
      if (h->score_rest_before_bptt) {   // (the rest runs on another stream: its pooling stage reads this part's scores)
        if (!h->ev_part1) HIP_TRY(hipEventCreateWithFlags(&h->ev_part1, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->ev_part1, h->score_stream));
      }
    } else HIP_TRY(hipEventRecord(h->ev_score_done, h->score_stream));
    h->score_pending = true;
    h->last_forward_side = true;
    h->last_B = b->B;
    return KPRN_OK;
  }
  forward_impl(h, b, class_id, false, true, /*every_class=*/false);  // kprn_read_probs hands out the selected class
  API_END(h)
}

// the second part of a split scoring pass (kprn_set_option "score_split"): the remaining tiles + the pooling stage, behind everything queued
// on the main stream so far
extern "C++" void launch_score_rest(kprn_handle* h) {   // (declared in kprn_internal.h: batch_slots.hip calls it)
  const kprn_batch* b = h->score_rest_batch;
  h->score_rest_batch = nullptr;
  if (!b) return;
  hipStream_t rs = h->score_stream;
  if (h->score_rest_before_bptt && h->ev_part1) {
    if (!h->rest_stream) h->rest_stream = make_priority_stream(/*high=*/false);
    rs = h->rest_stream;
    HIP_TRY(hipStreamWaitEvent(rs, h->ev_part1, 0));
  }
  HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
  HIP_TRY(hipStreamWaitEvent(rs, h->ev_fork, 0));
  try {
    score::SideBuffers on_side(h, rs);
    fused::forward(h, b, false, h->score_rest_tile0, -1, false, h->score_rest_cid - 1);
    pool_stage(h, b, h->score_rest_cid - 1, false);
  } catch (...) {
    // the pass cannot finish: nobody may wait for it on a stale event, or hand out its half-filled S2 / sel2 as a finished pass
    h->score_pending = false; h->last_forward_side = false; h->last_B = 0;
    (void)hipStreamSynchronize(rs);
    throw;
  }
  HIP_TRY(hipEventRecord(h->ev_score_done, rs));
}

extern "C++" void score::rest_hook(kprn_handle* h) { if (h->score_rest_in_backward && h->score_rest_batch) launch_score_rest(h); }

int kprn_forward_batch_async_rest(kprn_handle* h) {
  API_BEGIN(h)
  launch_score_rest(h);
  API_END(h)
}

int kprn_read_probs(kprn_handle* h, float* probs, int32_t B) {
  API_BEGIN(h)
  KPRN_REQUIRE(probs && B > 0 && B <= h->last_B, KPRN_E_ARG, "bad probs buffer / B");
  if (h->last_forward_side) {
    score::order_behind_pass(h);
    HIP_TRY(hipMemcpyAsync(probs, h->sel2, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->score_stream));
    HIP_TRY(hipStreamSynchronize(h->score_stream));
  } else {
    HIP_TRY(hipMemcpyAsync(probs, h->ws.sel, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  prof_drain(h);
  API_END(h)
}

int kprn_forward_batch(kprn_handle* h, const kprn_batch* b, int32_t class_id, float* probs, float* all_probs, float* pooled, float* path_scores) {
  API_BEGIN(h)
  KPRN_REQUIRE(b != nullptr, KPRN_E_ARG, "batch is NULL");
  score::ProbsMirror mirror(h, probs, b->B);   // (the other outputs are copied, and cost the all-class reduction only when asked for)
  forward_impl(h, b, class_id, false, /*do_pool=*/true, /*every_class=*/all_probs != nullptr || pooled != nullptr, /*all_scores=*/path_scores != nullptr);
  const int C = h->cfg.C;
  hipStream_t s = h->stream;
  mirror.queue_copy();
  if (all_probs) HIP_TRY(hipMemcpyAsync(all_probs, h->ws.probs, (size_t)b->B * C * sizeof(float), hipMemcpyDeviceToHost, s));
  if (pooled) HIP_TRY(hipMemcpyAsync(pooled, h->ws.pooled, (size_t)b->B * C * sizeof(float), hipMemcpyDeviceToHost, s));
  if (path_scores) HIP_TRY(hipMemcpyAsync(path_scores, h->score_buf, (size_t)b->N * C * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  mirror.hand_out();
  prof_drain(h);
  API_END(h)
}

int kprn_forward(kprn_handle* h, const int32_t* idx, int32_t B, int32_t P, int32_t T, int32_t F, int32_t class_id, float* probs, float* all_probs) {
  if (!h) return KPRN_E_ARG;
  int rc = dropin_feed(h, /*score=*/true, idx, nullptr, B, P, T, F);   // (engine-owned feed slots: see kprn_train_step)
  if (rc != KPRN_OK) return rc;
  return kprn_forward_batch(h, h->dropin_slot[h->dropin_last], class_id, probs, all_probs, nullptr, nullptr);
}

int kprn_forward_ragged(kprn_handle* h, const int32_t* idx, const int32_t* counts, int32_t B, int64_t N, int32_t T, int32_t F, int32_t class_id, float* probs,
                        float* all_probs) {
  if (!h) return KPRN_E_ARG;
  if (!counts) { h->err = "counts is NULL"; return KPRN_E_ARG; }
  int rc = dropin_feed(h, /*score=*/true, idx, nullptr, B, 0, T, F, counts, N);
  if (rc != KPRN_OK) return rc;
  return kprn_forward_batch(h, h->dropin_slot[h->dropin_last], class_id, probs, all_probs, nullptr, nullptr);
}

// ---- ranking stage: the score board, kprn_rank_groups, kprn_recommend_ragged (kernels: rank_groups.hip) ---------------------------------------
int kprn_board_reserve(kprn_handle* h, int64_t n) {
  API_BEGIN(h)
  KPRN_REQUIRE(n >= 1 && n < (1ll << 40), KPRN_E_ARG, "board size must be >= 1");
  sync_compute_streams(h);   // (queued puts and a ranking call's reads of the old board)
  h->put_side = false;
  dfree(h->board);
  h->board_n = 0;
  h->board = dalloc<float>(n);
  h->board_n = n;
  for (int64_t o = 0; o < n; o += (1ll << 30))   // every entry NaN: ranking counts an entry nothing wrote as invalid
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(h->board + o), 0x7fc00000, (size_t)std::min<int64_t>(n - o, 1ll << 30), h->stream));
  API_END(h)
}

int kprn_board_put(kprn_handle* h, int64_t offset, int32_t B) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->board, KPRN_E_ARG, "no board: call kprn_board_reserve first");
  KPRN_REQUIRE(B > 0 && h->last_B > 0 && B <= h->last_B, KPRN_E_ARG, "no scoring pass to read from, or B beyond its pairs");
  KPRN_REQUIRE(offset >= 0 && offset <= h->board_n - B, KPRN_E_INDEX, "the range leaves the board");
  if (h->last_forward_side) {
    // kprn_read_probs with the copy staying on the device and nobody waiting on the host
    score::order_behind_pass(h);
    HIP_TRY(hipMemcpyAsync(h->board + offset, h->sel2, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, h->score_stream));
    // later passes on the scoring stream follow the copy in stream order, one on the rest stream starts behind its first part there; a pass that writes
    // sel2 from the main stream, and every reader of the board, waits for this event (join_put)
    if (!h->ev_put) HIP_TRY(hipEventCreateWithFlags(&h->ev_put, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->ev_put, h->score_stream));
    h->put_side = true;
  } else {
    HIP_TRY(hipMemcpyAsync(h->board + offset, h->ws.sel, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  }
  API_END(h)
}

int kprn_board_write(kprn_handle* h, int64_t offset, const float* src, int64_t n) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->board, KPRN_E_ARG, "no board: call kprn_board_reserve first");
  KPRN_REQUIRE(src && n > 0, KPRN_E_ARG, "bad source / n");
  KPRN_REQUIRE(offset >= 0 && offset <= h->board_n - n, KPRN_E_INDEX, "the range leaves the board");
  join_put(h);
  HIP_TRY(hipMemcpyAsync(h->board + offset, src, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  API_END(h)
}

int kprn_board_read(kprn_handle* h, int64_t offset, float* dst, int64_t n) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->board, KPRN_E_ARG, "no board: call kprn_board_reserve first");
  KPRN_REQUIRE(dst && n > 0, KPRN_E_ARG, "bad destination / n");
  KPRN_REQUIRE(offset >= 0 && offset <= h->board_n - n, KPRN_E_INDEX, "the range leaves the board");
  join_put(h);
  HIP_TRY(hipMemcpyAsync(dst, h->board + offset, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  API_END(h)
}

// arguments up, one or two launches, results down, all on the main stream; the caller has validated everything (rk::validate) and synchronises
// The one-call route (kprn_recommend_ragged) moves nothing with copy operations: the group table is read, and the top-K rows are written, by the kernel itself in
// page-locked host memory (as kprn_forward_batch's probabilities are), so the call is the pass, the pooling stage, one ranking launch and one wait; the rows are
// handed out after that wait (rank_pinned_fetch).  Measured with copies: 95 us a user against 68 us for kprn_forward_ragged + the host rule (profiles/rank).
static void rank_run_pinned(kprn_handle* h, const float* dev_scores, const int64_t* goff, int32_t G, int32_t mode, int32_t K, int max_n) {
  const size_t o_ti = ((size_t)(G + 1) * 8 + 15) & ~(size_t)15, o_ts = o_ti + (((size_t)G * K * 4 + 15) & ~(size_t)15), total = o_ts + (size_t)G * K * 4;
  grow_pinned(h->rank_pin, h->rank_pin_bytes, total, 2 * total + 256, 2 * total + 256, {h->stream}, /*wait_if_empty=*/true);
  char* base = (char*)h->rank_pin;
  memcpy(base, goff, (size_t)(G + 1) * 8);
  h->rank_pin_off[0] = o_ti; h->rank_pin_off[1] = o_ts;
  rk::Args a;
  a.scores = dev_scores; a.members = nullptr; a.goff = (const int64_t*)base; a.pos = nullptr;
  a.G = G; a.mode = mode; a.K = K; a.hist_len = 1;
  a.ranks = nullptr; a.tk_idx = (int32_t*)(base + o_ti); a.tk_score = (float*)(base + o_ts); a.hist = nullptr;
  a.sort_min = h->rank_sort_min;
  ProfScope ps(h, "rank_groups");
  rk::launch(h->stream, a, max_n);
}
static void rank_pinned_fetch(kprn_handle* h, int32_t G, int32_t K, int32_t* topk_idx, float* topk_score) {
  memcpy(topk_idx, (char*)h->rank_pin + h->rank_pin_off[0], (size_t)G * K * 4);
  memcpy(topk_score, (char*)h->rank_pin + h->rank_pin_off[1], (size_t)G * K * 4);
}

static void rank_run(kprn_handle* h, const float* dev_scores, const int64_t* members, const int64_t* goff, const int32_t* pos, int32_t G, int32_t mode, int32_t K,
                     int max_n, int32_t* ranks, int32_t* topk_idx, float* topk_score, int64_t* hist, int32_t hist_len) {
  const int64_t m0 = goff[0], M = members ? goff[G] - m0 : 0;
  auto up8 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t o_goff = 0, o_mem = o_goff + up8((size_t)(G + 1) * 8), o_hist = o_mem + up8((size_t)M * 8), o_pos = o_hist + up8((size_t)(hist_len + 4) * 8),
               o_ranks = o_pos + up8((size_t)G * 4), o_ti = o_ranks + up8((size_t)G * 4), o_ts = o_ti + up8((size_t)G * K * 4), total = o_ts + up8((size_t)G * K * 4);
  char* base = (char*)grow_call_block(h->stream, h->rank_buf, h->rank_buf_bytes, total);
  hipStream_t s = h->stream;
  std::vector<int64_t> rebased;
  const int64_t* goff_up = goff;
  if (members && m0 != 0) {   // (the kernels index the uploaded slice of members from 0)
    rebased.assign(goff, goff + G + 1);
    for (auto& v : rebased) v -= m0;
    goff_up = rebased.data();
  }
  HIP_TRY(hipMemcpyAsync(base + o_goff, goff_up, (size_t)(G + 1) * 8, hipMemcpyHostToDevice, s));
  if (members) HIP_TRY(hipMemcpyAsync(base + o_mem, members + m0, (size_t)M * 8, hipMemcpyHostToDevice, s));
  if (pos) HIP_TRY(hipMemcpyAsync(base + o_pos, pos, (size_t)G * 4, hipMemcpyHostToDevice, s));
  if (rebased.size()) HIP_TRY(hipStreamSynchronize(s));   // (the copy's source is a local)
  if (hist) HIP_TRY(hipMemsetAsync(base + o_hist, 0, (size_t)(hist_len + 4) * 8, s));
  rk::Args a;
  a.scores = dev_scores; a.members = members ? (const int64_t*)(base + o_mem) : nullptr; a.goff = (const int64_t*)(base + o_goff);
  a.pos = pos ? (const int32_t*)(base + o_pos) : nullptr;
  a.G = G; a.mode = mode; a.K = K; a.hist_len = hist_len;
  a.ranks = ranks ? (int32_t*)(base + o_ranks) : nullptr;
  a.tk_idx = topk_idx ? (int32_t*)(base + o_ti) : nullptr; a.tk_score = topk_idx ? (float*)(base + o_ts) : nullptr;
  a.hist = hist ? (unsigned long long*)(base + o_hist) : nullptr;
  a.sort_min = h->rank_sort_min;
  {
    ProfScope ps(h, "rank_groups");
    rk::launch(s, a, max_n);
  }
  if (ranks) HIP_TRY(hipMemcpyAsync(ranks, base + o_ranks, (size_t)G * 4, hipMemcpyDeviceToHost, s));
  if (topk_idx) {
    HIP_TRY(hipMemcpyAsync(topk_idx, base + o_ti, (size_t)G * K * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(topk_score, base + o_ts, (size_t)G * K * 4, hipMemcpyDeviceToHost, s));
  }
  if (hist) HIP_TRY(hipMemcpyAsync(hist, base + o_hist, (size_t)(hist_len + 4) * 8, hipMemcpyDeviceToHost, s));
}

int kprn_rank_groups(kprn_handle* h, const int64_t* members, const int64_t* group_offsets, const int32_t* pos, int32_t G, int32_t mode, int32_t K,
                     int32_t* ranks, int32_t* topk_idx, float* topk_score, int64_t* hist, int32_t hist_len) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->board, KPRN_E_ARG, "no board: call kprn_board_reserve first");
  KPRN_REQUIRE((topk_idx == nullptr) == (topk_score == nullptr), KPRN_E_ARG, "topk_idx and topk_score go together");
  int max_n = 0;
  std::string why;
  const int rc = rk::validate(h->board_n, members, group_offsets, pos, G, mode, K, hist_len, &max_n, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  join_put(h);
  rank_run(h, h->board, members, group_offsets, pos, G, mode, K, max_n, ranks, topk_idx, topk_score, hist, hist_len);
  HIP_TRY(hipStreamSynchronize(h->stream));
  prof_drain(h);
  API_END(h)
}

// ranking targets in groups of any size (kernel: rank_targets.hip): arguments up, ONE launch, results down, one wait
int kprn_rank_targets(kprn_handle* h, const int64_t* members, const int64_t* group_offsets, const int64_t* target_offsets, const int32_t* targets, int32_t G,
                      int32_t mode, int32_t* places, int64_t* hist, int32_t hist_len) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->board, KPRN_E_ARG, "no board: call kprn_board_reserve first");
  KPRN_REQUIRE(places && hist, KPRN_E_ARG, "places and hist are required");
  const char* why = "";
  const int rc = rt::validate(h->board_n, members, group_offsets, target_offsets, targets, G, mode, hist_len, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  join_put(h);
  const int64_t m0 = group_offsets[0], M = members ? group_offsets[G] - m0 : 0, NT = target_offsets[G];
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t o_goff = 0, o_toff = o_goff + up((size_t)(G + 1) * 8), o_mem = o_toff + up((size_t)(G + 1) * 8), o_hist = o_mem + up((size_t)M * 8),
               o_tg = o_hist + up((size_t)(hist_len + 4) * 8), o_pl = o_tg + up((size_t)NT * 4), total = o_pl + up((size_t)NT * 4);
  hipStream_t s = h->stream;
  char* base = (char*)grow_call_block(s, h->rank_buf, h->rank_buf_bytes, total);
  std::vector<int64_t> rebased;
  const int64_t* goff_up = group_offsets;
  if (members && m0 != 0) {   // (the kernel indexes the uploaded slice of members from 0)
    rebased.assign(group_offsets, group_offsets + G + 1);
    for (auto& v : rebased) v -= m0;
    goff_up = rebased.data();
  }
  HIP_TRY(hipMemcpyAsync(base + o_goff, goff_up, (size_t)(G + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(base + o_toff, target_offsets, (size_t)(G + 1) * 8, hipMemcpyHostToDevice, s));
  if (members) HIP_TRY(hipMemcpyAsync(base + o_mem, members + m0, (size_t)M * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(base + o_tg, targets, (size_t)NT * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(base + o_hist, 0, (size_t)(hist_len + 4) * 8, s));
  rt::Args a;
  a.scores = h->board; a.members = members ? (const int64_t*)(base + o_mem) : nullptr;
  a.goff = (const int64_t*)(base + o_goff); a.toff = (const int64_t*)(base + o_toff); a.targets = (const int32_t*)(base + o_tg);
  a.G = G; a.mode = mode; a.hist_len = hist_len;
  a.places = (int32_t*)(base + o_pl); a.hist = (unsigned long long*)(base + o_hist);
  {
    ProfScope ps(h, "rank_targets");
    rt::launch(s, a);
  }
  HIP_TRY(hipMemcpyAsync(places, base + o_pl, (size_t)NT * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hist, base + o_hist, (size_t)(hist_len + 4) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));   // (also covers `rebased`, the source of a pageable copy)
  prof_drain(h);
  API_END(h)
}

// the refusals of the one-call routes that need no device work, before anything is fed
static int recommend_check(kprn_handle* h, const int32_t* counts, int32_t B, const int32_t* group_counts, int32_t G, int32_t mode, int32_t K,
                           const int32_t* topk_idx, const float* topk_score, std::vector<int64_t>& goff, int* max_n) {
  API_BEGIN(h)
  KPRN_REQUIRE(counts && group_counts && topk_idx && topk_score && G >= 1 && B >= 1, KPRN_E_ARG, "NULL argument, or G / B < 1");
  goff.assign((size_t)G + 1, 0);
  for (int32_t g = 0; g < G; ++g) goff[g + 1] = goff[g] + group_counts[g];
  KPRN_REQUIRE(goff[G] == B, KPRN_E_ARG, "group_counts do not add up to B");
  std::string why;
  const int rc = rk::validate(B, nullptr, goff.data(), nullptr, G, mode, K, 1, max_n, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  API_END(h)
}

// ---- explanation stage: kprn_explain_batch, kprn_recommend_explain_ragged (kernels: explain_paths.hip) ---------------------------------------
static ex::Args explain_args(kprn_handle* h, const kprn_batch* b, int class_id, int M) {
  const kprn_config& c = h->cfg;
  ex::Args a;
  a.S = h->score_buf; a.off = b->off; a.B = b->B; a.P = b->P; a.seg_wave = b->off ? b->seg_wave : 0;
  a.C = c.C; a.cid = class_id - 1; a.reducer = c.reducer; a.K = c.K; a.M = M; a.ig = h->pool_ig;
  a.pairs = nullptr; a.goff = nullptr; a.per_group = 1; a.n = 0;
  a.idx = nullptr; a.score = nullptr; a.weight = nullptr; a.pooled = nullptr; a.prob = nullptr;
  return a;
}

int kprn_explain_batch(kprn_handle* h, const kprn_batch* b, int32_t class_id, const int32_t* pairs, int32_t n_pairs, int32_t M, int32_t* path_idx,
                       float* path_score, float* path_weight, float* pooled, float* probs) {
  API_BEGIN(h)
  KPRN_REQUIRE(b != nullptr, KPRN_E_ARG, "batch is NULL");
  KPRN_REQUIRE(path_idx && path_score && path_weight, KPRN_E_ARG, "path_idx, path_score and path_weight are required");
  std::string why;
  const int rc = ex::validate(b->B, pairs, n_pairs, M, &why);
  if (rc != KPRN_OK) throw KprnError{rc, why};
  forward_impl(h, b, class_id, false, /*do_pool=*/true, /*every_class=*/false);   // (refuses a bad class_id / an id out of range before anything is queued)
  const int64_t n = n_pairs;
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t rows = up((size_t)n * M * 4), o_pairs = 0, o_idx = up((size_t)n * 4), o_score = o_idx + rows, o_weight = o_score + rows,
               o_pooled = o_weight + rows, o_prob = o_pooled + up((size_t)n * 4), total = o_prob + up((size_t)n * 4);
  char* base = (char*)grow_call_block(h->stream, h->explain_buf, h->explain_buf_bytes, total);
  hipStream_t s = h->stream;
  if (pairs) HIP_TRY(hipMemcpyAsync(base + o_pairs, pairs, (size_t)n * 4, hipMemcpyHostToDevice, s));
  ex::Args a = explain_args(h, b, class_id, M);
  a.pairs = pairs ? (const int32_t*)(base + o_pairs) : nullptr;
  a.n = n;
  a.idx = (int32_t*)(base + o_idx); a.score = (float*)(base + o_score); a.weight = (float*)(base + o_weight);
  a.pooled = pooled ? (float*)(base + o_pooled) : nullptr; a.prob = probs ? (float*)(base + o_prob) : nullptr;
  {
    ProfScope ps(h, "explain_paths");
    ex::launch(s, a, b->off ? b->max_cnt : b->P);
  }
  HIP_TRY(hipMemcpyAsync(path_idx, a.idx, (size_t)n * M * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(path_score, a.score, (size_t)n * M * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(path_weight, a.weight, (size_t)n * M * 4, hipMemcpyDeviceToHost, s));
  if (pooled) HIP_TRY(hipMemcpyAsync(pooled, a.pooled, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  if (probs) HIP_TRY(hipMemcpyAsync(probs, a.prob, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  prof_drain(h);
  API_END(h)
}

// ---- the one-call routes: kprn_recommend_ragged, kprn_recommend_explain_ragged -------------------------------------------------------------------
// The pass of kprn_forward_ragged, the ranking kernel behind it on the same stream over the pass's own output and -- with path outputs -- one more launch behind
// that, whose pair list is the top-K rows the ranking kernel wrote (page-locked memory the device reads in place) and whose own rows land in page-locked memory
// too: one wait for all of it, no copy operation; the probabilities come back through the pool kernel's mirror as in kprn_forward_batch
static int recommend(kprn_handle* h, const int32_t* idx, const int32_t* counts, int32_t B, int64_t N, int32_t T, int32_t F, int32_t class_id,
                     const int32_t* group_counts, int32_t G, int32_t mode, int32_t K, int32_t M, int32_t* topk_idx, float* topk_score, int32_t* path_idx,
                     float* path_score, float* path_weight, float* probs) {
  std::vector<int64_t> goff;
  int max_n = 0;
  int rc = recommend_check(h, counts, B, group_counts, G, mode, K, topk_idx, topk_score, goff, &max_n);
  if (rc != KPRN_OK) return rc;
  rc = dropin_feed(h, /*score=*/true, idx, nullptr, B, 0, T, F, counts, N);
  if (rc != KPRN_OK) return rc;
  API_BEGIN(h)
  score::ProbsMirror mirror(h, probs, B);
  const int64_t n = (int64_t)G * K;
  const size_t rows = path_idx ? ((size_t)n * M * 4 + 15) & ~(size_t)15 : 0;
  if (path_idx) grow_pinned(h->explain_pin, h->explain_pin_bytes, 3 * rows, 6 * rows + 256, 6 * rows + 256, {h->stream}, /*wait_if_empty=*/true);
  char* pin = (char*)h->explain_pin;
  const kprn_batch* b = h->dropin_slot[h->dropin_last];
  forward_impl(h, b, class_id, false, /*do_pool=*/true, /*every_class=*/false);
  rank_run_pinned(h, h->ws.sel, goff.data(), G, mode, K, max_n);
  if (path_idx) {
    ex::Args a = explain_args(h, b, class_id, M);
    a.pairs = (const int32_t*)((char*)h->rank_pin + h->rank_pin_off[0]); a.goff = (const int64_t*)h->rank_pin; a.per_group = K;
    a.n = n;
    a.idx = (int32_t*)pin; a.score = (float*)(pin + rows); a.weight = (float*)(pin + 2 * rows);
    ProfScope ps(h, "explain_paths");
    ex::launch(h->stream, a, b->max_cnt);
  }
  mirror.queue_copy();
  HIP_TRY(hipStreamSynchronize(h->stream));
  rank_pinned_fetch(h, G, K, topk_idx, topk_score);
  if (path_idx) {
    memcpy(path_idx, pin, (size_t)n * M * 4);
    memcpy(path_score, pin + rows, (size_t)n * M * 4);
    memcpy(path_weight, pin + 2 * rows, (size_t)n * M * 4);
  }
  mirror.hand_out();
  prof_drain(h);
  API_END(h)
}

int kprn_recommend_ragged(kprn_handle* h, const int32_t* idx, const int32_t* counts, int32_t B, int64_t N, int32_t T, int32_t F, int32_t class_id,
                          const int32_t* group_counts, int32_t G, int32_t mode, int32_t K, int32_t* topk_idx, float* topk_score, float* probs) {
  return recommend(h, idx, counts, B, N, T, F, class_id, group_counts, G, mode, K, 0, topk_idx, topk_score, nullptr, nullptr, nullptr, probs);
}

int kprn_recommend_explain_ragged(kprn_handle* h, const int32_t* idx, const int32_t* counts, int32_t B, int64_t N, int32_t T, int32_t F, int32_t class_id,
                                  const int32_t* group_counts, int32_t G, int32_t mode, int32_t K, int32_t M, int32_t* topk_idx, float* topk_score,
                                  int32_t* path_idx, float* path_score, float* path_weight, float* probs) {
  if (!h) return KPRN_E_ARG;
  if (!path_idx || !path_score || !path_weight) { h->err = "path_idx, path_score and path_weight are required"; return KPRN_E_ARG; }
  if (M < 1 || M > KPRN_EXPLAIN_MAX_M) { h->err = "M must be in 1..32"; return KPRN_E_ARG; }
  return recommend(h, idx, counts, B, N, T, F, class_id, group_counts, G, mode, K, M, topk_idx, topk_score, path_idx, path_score, path_weight, probs);
}

}  // extern "C"
