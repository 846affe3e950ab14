// Internal declarations of libkprn.so (gfx950 only).  Public boundary: include/kprn.h.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <exception>
#include <functional>
#include <initializer_list>
#include <future>
#include <string>
#include <vector>
#include <map>

#include "../../include/kprn.h"
#include "philox_dev.h"

#define KPRN_MAX_LAYERS 8

// ---- error plumbing ---------------------------------------------------------------
struct KprnError { int code; std::string msg; };
#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e__ = (expr);                                                              \
    if (e__ != hipSuccess)                                                                \
      throw KprnError{KPRN_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__)}; \
  } while (0)
#define KPRN_REQUIRE(cond, code, text) \
  do { if (!(cond)) throw KprnError{(code), std::string(text)}; } while (0)

// ---- parameter table ----------------------------------------------------------------
struct ParamInfo {
  std::string name;
  int64_t flat_off;   // offset in the reference getParameters() order
  int64_t rows, cols; // cols == 1 for biases
  int where;          // 0 = dense arena, 1 = entity table
  int64_t dev_off;    // offset inside that device buffer
};

struct LayerOff {     // offsets into the dense arena (rnn: Wi = i2h.weight, bi = i2h.bias, Wo = h2h.weight, bo = h2h.bias)
  int64_t Wi, bi, Wo, bo;
  int64_t Wc, bc, Uc;  // gru: candidate c_i2h.weight, c_i2h.bias, c_h2h.weight
  int Din;
};

// ---- workspace for the generic (unfused) pipeline -------------------------------------
struct Workspace {
  int64_t cap_N = 0;   // paths (generic-pipeline buffers)
  int cap_T = 0;
  int64_t cap_Nc = 0;  // paths (common buffers S, dS)
  float* X = nullptr;      // [T][N][D]      gathered step inputs (time-major)
  float* Hs = nullptr;     // [L][T][N][H]
  float* Cs = nullptr;     // [L][T][N][H]
  float* ACT = nullptr;    // [L][T][N][4H]  pre-activations overwritten by gate values i,g,f,o
  float* dA = nullptr;     // [T][N][4H]     pre-activation grads of the layer being processed
  float* dIn = nullptr;    // [T][N][max(D,H)]
  float* dH = nullptr;     // [N][H]
  float* dC = nullptr;     // [N][H]
  float* S = nullptr;      // [N][C]   mapper output
  float* dS = nullptr;     // [N]      grad wrt S[:, classId]
  int64_t cap_B = 0;
  float* pooled = nullptr; // [B][C]
  float* probs = nullptr;  // [B][C]
  float* sel = nullptr;    // [B] probs[:, classId]
  float* dy = nullptr;     // [B]
  float* mask = nullptr;   // [L][T][N]  rnn: MaskZero flags of the step inputs
  float* HsD = nullptr;    // [L-1][T][N][H] rnn with dropout: the dropped copies of Hs[0 .. L-2] the layers above read (allocated at the first such training forward)
  int64_t cap_HsD = 0;     // floats
};

struct ProfEntry { double total_ms = 0; int64_t launches = 0; };

// Option "deterministic" = "2" (DESIGN.md 3.11): grow-only scratch, owned by the handle, that a producer kernel of the generic backward fills with one slab of
// partial sums per workgroup or K split (plain stores) and kk::slab_join, the launch behind it, adds up in slab order.  A null DetScratch* argument anywhere
// below means the default kernels with their fp32 atomics.
struct DetScratch { float* p = nullptr; int64_t cap = 0; };

namespace fused { constexpr int KCAP = 8; }  // longest identical prefix the fused kernels skip (lstm_fused_common.h)

struct kprn_graph;   // path_find_dev.h
struct kprn_sampler; // neg_sample.hip

struct kprn_batch {
  int32_t B, P, T, F;
  int64_t N = 0;              // paths of the batch: B*P, or sum of the counts of a ragged batch
  // ragged batch (kprn_batch_create_ragged; an extension, the reference has none): pair b owns the paths off[b] .. off[b+1]-1 of the flat
  // [N,T,F] ids.  off == null: rectangular.  P of a ragged batch is 0 and nothing reads it.
  int32_t* off = nullptr;     // device [B+1]
  int32_t* wg = nullptr;      // device [n_wg+1]: first pair of each loss-stage workgroup (kprn_host_ragged_plan)
  int32_t n_wg = 0;           // loss-stage workgroups = loss partials of a ragged batch
  int32_t max_cnt = 0;        // longest segment
  int32_t seg_wave = 0;       // 1: a wave per pair (max_cnt > kk::RAGGED_THREAD_MAX), chosen when the batch is made
  std::vector<int32_t> hrag;  // host: off [B+1] | wg [n_wg+1], the source of their upload
  // group table of the pairwise loss (kprn_batch_set_groups): an allocation of its own that only grows and goes with the batch; n_groups == 0: no table
  // (slots::detach drops it with the contents it described)
  int32_t* groups = nullptr;  // device: n_terms as one int64 (words 0, 1) | group_offsets [n_groups+1] from word 2
  int64_t groups_cap = 0;     // words
  int32_t n_groups = 0;
  int64_t n_terms = 0;        // (positive, negative) pairs within the groups, counted on the device when the table was set
  int32_t* idx = nullptr;     // device [B,P,T,F]  ([N,T,F] when ragged)
  float* labels = nullptr;    // device [B] or null
  int32_t* uniq = nullptr;    // device: distinct entity rows of this batch (0-based); count at uniq[uniq_cap]
  int64_t uniq_cap = 0;
  int32_t n_uniq = 0;
  int64_t serial = 0;         // identity of this batch for the catch-up bookkeeping
  // occurrence index (batch_index.hip): all B*P*T positions sorted by entity row
  int32_t* key_sorted = nullptr;  // device [B*P*T] entity row (0-based)
  int32_t* pos_sorted = nullptr;  // device [B*P*T] position n*T + t
  int64_t n_index = 0;            // entries of the index (B*P*T, + the virtual prefix positions of a plan)
  // identical-prefix plan (fused path; batch_index.hip prefix_plan).  With a plan, the index above lives in the
  // REORDERED path space and skips the positions the fused kernels do not execute.
  int32_t* idx_s = nullptr;       // device [B*P][T][F] paths reordered by prefix length
  int32_t* perm = nullptr;        // device [B*P] reordered slot -> original path
  int32_t* slot_of = nullptr;     // device [B*P] original path -> reordered slot
  int32_t* tile_k = nullptr;      // device [ceil(B*P/64)] shared prefix length of each 64-path tile
  int32_t* pmeta = nullptr;       // device [8+F]: longest prefix, reference path, the reference step's ids
  int kcap = 0;
  int h_kmax = 0;                 // host copy: longest shared prefix in the batch (0: nothing is skipped)
  int32_t h_ref[16] = {0};        // host copy: the reference step's ids (1-based, all F <= 16 columns)
  int64_t exec_steps = 0;         // (path, step) positions the kernels execute (B*P*T without a plan)
  // ---- streaming feed (kprn_batch_feed_async): a batch is a SLOT whose buffers are refilled in place, the way
  // BatcherFileList:populateGPUTensor copies every minibatch into preallocated tensors (BatcherFileList.lua:53-96)
  int32_t* block = nullptr; int64_t block_cap = 0;  // the ONE device allocation all arrays above point into (32-bit words)
  int32_t* d_flag = nullptr;      // device [4]: id-validation flag of this batch
  int32_t* h_meta = nullptr;      // pinned host [h_meta_cap]: flag, n_uniq, plan header [8+F], tile_k copy
  int64_t h_meta_cap = 0;
  hipEvent_t ev_ready = nullptr;  // recorded behind the slot's upload + index build on the feed stream
  bool pending = false;           // filled asynchronously: the host-side fields above are read back at first use
  bool bad = false;               // an id of the current contents is outside its vocabulary: every use returns KPRN_E_INDEX
  // host-built feed (host_feed.hip): a worker thread derives plan + index on the host cores into page-locked staging and queues
  // the uploads on the slot's own copy stream; the consumer waits for the job (host) and for ev_ready (stream-side, no host wait)
  bool has_index = true;          // occurrence index + distinct rows present (a label-less batch fed while no lazy row update is
                                  // pending carries none: scoring never walks them)
  bool idx_valid = true;          // the ids in their original order are on the device (not uploaded for such a batch when it has a plan)
  bool host_built = false;
  std::future<void> job;          // valid while pending && host_built
  int32_t* hs = nullptr; int64_t hs_cap = 0;   // page-locked image of the device block
  std::vector<int32_t> hw;        // work arrays of the host build (4 x index entries)
  hipEvent_t ev_fork = nullptr, ev_fork2 = nullptr;  // main / scoring stream position when the refill was requested
  struct HostResult { bool bad = false; int kmax = 0; int32_t ref[16] = {0}; int32_t n_uniq = 0; int64_t exec_steps = 0; } hres;
};

// A/B switches of the bf16 products (gemm_bf16.hip), per handle; all off by default, each one the record of a measurement:
struct Bf16GemmOpts {
  // option "bf16_gemm_touch": chunks ahead of its DMA k_gemm16x touches a chunk's cache lines.  MEASURED SLOWER (merged dW 1.06 -> 1.64 ms at 3 / 6 / 12 chunks: loads
  // retire in issue order, so a touch that misses to HBM holds back the retirement of every DMA piece issued behind it -- the prefetch sits on the critical path it
  // was meant to shorten).  The test holds it equal to the untouched launch.
  int touch = 0;
  bool regstage = false;   // option "bf16_gemm_regstage": the split-K products on k_gemm16r (operands through registers, four chunks in flight); measured no faster
  // option "bf16_gemm_pingpong": the split-K products of the bf16 backward on k_gemm16p where the shape suits it.  MEASURED SLOWER than the lockstep kernel
  // (profiles/r05/bench_c4_m_*, bench_c4_n_*: merged dW 1.50 against 1.10 ms at 64 K ranges, 1.62 / 2.05 / 1.97 at 32 / 16 / 8; k_gemm16x 1.08-1.12 at every count):
  // neither the SIMD-level phase collision nor the number of atomic passes is what holds these products at 0.28 of the bf16 peak.  tests/test_gpu_persist.py holds
  // it equal to k_gemm16x to fp32 reordering.
  bool pingpong = false;
};

struct kprn_handle {
  kprn_config cfg;
  int D = 0;
  int G = 4;  // rows of the recurrent weights per hidden unit: 4 (FastLSTM gates), 2 (gru r, z) or 1 (rnn)
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool stream_known = false;   // the caller chose the stream or has fetched it (kprn_stream): precondition of the data-parallel hooks
  std::string err;

  // parameters
  std::vector<ParamInfo> params;
  int64_t n_params = 0, n_dense = 0, n_ent = 0;
  int64_t off_Wt = 0, off_Wr = 0, off_outW = 0, off_outb = 0;
  LayerOff layer[KPRN_MAX_LAYERS];
  float *dense = nullptr, *g_dense = nullptr, *s1_dense = nullptr, *s2_dense = nullptr;
  float *We = nullptr, *g_We = nullptr, *s1_We = nullptr, *s2_We = nullptr;

  // lazy-exact entity update bookkeeping
  int32_t* We_last = nullptr;   // [Ve] optimiser step each row is current to
  int64_t opt_step = 0;         // optState.t / evalCounter
  int opt_method = -1;
  float* step_tab = nullptr;    // device: adam step size of every step so far (index = step)
  float* step_tab_host = nullptr; // pinned mirror
  int64_t step_tab_cap = 0;
  bool lazy_pending = false;    // some entity rows are behind opt_step
  bool ent_dense_mode = false;  // entity table currently updated densely (We_last not maintained)
  bool ent_grads_dirty = false; // g_We holds this step's rows (cleared by the optimiser / zero_grads)
  float last_b1 = 0.9f, last_b2 = 0.999f, last_eps = 1e-8f;

  // per-step touched-row list (union over ranks in data-parallel runs)
  int32_t* step_rows = nullptr;
  int32_t* step_count = nullptr; // device scalar
  int64_t step_rows_cap = 0;
  int64_t step_rows_ub = 0;      // host-side upper bound of *step_count
  // the list the optimiser walks: the handle's own buffers, or a VIEW of a batch's distinct-row list (single-rank
  // training: no copy; materialised before the batch can go away or the data-parallel exchange rewrites it)
  const int32_t* rows_view = nullptr; const int32_t* count_view = nullptr; const kprn_batch* view_batch = nullptr;
  // steady-state shortcuts (each one is a launch the previous step already did the work of)
  bool pad_clean = false;          // the three pad rows are zero (zeroPadTokens done and nothing wrote parameters since)
  bool dense_grads_clean = false;  // g_dense is all zero (the optimiser consumed it)
  int64_t caught_serial = -1, caught_step = -1;  // batch whose entity rows are current to opt_step
  int64_t grads_serial = -1;       // batch the gradients in g_We / g_dense came from
  int64_t next_serial = 1;
  int loss_accumulate = 0;   // option: every backward adds its loss to d_loss[1] (count in d_loss[2]) -- an epoch's error without a host sync per step
  float* loss_partial = nullptr; int64_t loss_partial_cap = 0; int loss_pending = 0;  // >0: d_loss = sum of that many partials, not formed yet
  // kprn_train_step / kprn_train_step_batch hand the loss back as soon as the loss stage has run (option "train_step_return": "loss", default) instead of after the
  // whole step ("drain"): the loss stage mirrors its per-workgroup partials into page-locked host memory, an event behind it is what the call waits for, the host adds
  // the partials in k_sum_partials' order.  The backward and the update run on while the caller prepares its next minibatch (MyOptimizer.lua:184-221 returns the loss of
  // a step whose update has happened; here it is ordered on the engine's stream before anything a later call can observe).
  float* loss_mirror = nullptr; int64_t loss_mirror_cap = 0; hipEvent_t ev_loss = nullptr;
  bool loss_early_armed = false; int loss_early_n = 0; int train_step_drain = 0;
  float* probs_mirror = nullptr; int64_t probs_mirror_cap = 0; float* sel_host_armed = nullptr;   // kprn_forward_batch: the selected class's probabilities, mirrored by the pool kernel
  // packing buffers for the data-parallel exchange
  int32_t* dp_mark = nullptr;   // [Ve] flags of the exchange's union (all zero between steps)
  // union + update fused (option "dp_fused_update"): kprn_sparse_grad_merge only records the gathered buffer; the update walks it directly
  // (optim_step.hip k_union_adam) or, where that does not apply (clip / L2, Adagrad, dense entity sweeps, bf16 shadows), materialises the union first
  bool dp_fused_update = false, dp_union_pending = false;
  const void* dp_all = nullptr; int dp_world = 0, dp_cap = 0;
  // the exchange issued by the engine itself (kprn_dp_init / kprn_dp_exchange_begin / _finish): RCCL communicator (ncclComm_t), the
  // in-place all-gather buffer [world][words], and -- dp_comm_stream -- a stream of its own for the collective so that work queued on
  // the main stream after _begin (a scoring pass forks from there) does not wait for it
  void* dp_comm = nullptr; int dp_rank = 0, dp_nranks = 0;
  int32_t* dp_gather = nullptr; int64_t dp_gather_words = 0;
  bool dp_comm_stream_on = false, dp_begun = false;
  hipStream_t dp_comm_stream = nullptr; hipEvent_t ev_dp_packed = nullptr, ev_dp_gathered = nullptr;
  bool dp_dense_in_pack = false; // option: the dense gradient arena rides in the packed buffer (one collective per step)
  bool dp_saved_dense_in_pack = false, dp_saved_fused_update = false;  // the two options as the caller had set them before kprn_dp_init forced them on (restored by kprn_dp_shutdown)
  int32_t* pack_buf = nullptr; int64_t pack_cap = 0, pack_words = 0;  // {count,-,-,-, ids[cap], rows[cap*de]} 32-bit words; cap of the last pack, allocated words

  // scalars on device
  float* d_loss = nullptr;      // [1]
  float* d_norm2 = nullptr;     // [1] sum g^2
  int32_t* d_flag = nullptr;    // [1] index-validation flag
  float* h_pinned = nullptr;    // pinned host scratch [>= 16]

  Workspace ws;
  float* score_buf = nullptr;   // where the mapper output [N][C] of the last forward lives (ws.S)
  void* fused_state = nullptr;  // owned by lstm_fused_*.hip
  void* bf16_state = nullptr;   // owned by lstm_bf16.hip (compute_dtype 1: bf16 shadows of tables / weights, bf16 activations)
  void* bidx_scratch = nullptr; size_t bidx_scratch_bytes = 0;  // batch_index.hip temporaries
  // streaming batch feed: upload + validation + occurrence index + prefix plan of the NEXT batch on their own stream, under
  // the step that is running (kprn_batch_feed_async)
  hipStream_t feed_stream = nullptr; hipEvent_t ev_feed_fork = nullptr;
  void* feed_scratch = nullptr; size_t feed_scratch_bytes = 0;
  int feed_build_host = 1;        // kprn_set_option "feed_build": host (worker threads + DMA, default) | device (kernels on the feed stream)
  int feed_workers = 0, feed_threads = 0;  // batches in preparation at once / helper threads per batch (0: from the core count)
  void* feed_pool = nullptr;      // hostfeed::Pool: builds the images
  void* upload_pool = nullptr;    // hostfeed::Pool of ONE thread: issues the uploads, one in flight at a time
  hipStream_t upload_stream = nullptr;
  int impl = 0;                 // 0 auto, 1 generic
  // scoring overlap (kprn_set_option "score_overlap"): kprn_forward_batch_async runs the fused scoring pass on a second stream
  // with its own output buffers, so that it shares the chip with whatever the main stream does next (the training forward
  // of the same step: neither depends on the other); every operation that would change what the pass reads waits for it
  int prefix_plan = 1;            // kprn_set_option "prefix_plan": build identical-prefix plans for new batches (fused path)
  int score_overlap = 0;
  hipStream_t score_stream = nullptr;
  int side_stream_probes = 0;     // candidates tried before one ran beside the main stream (score_stages.hip make_concurrent_stream)
  hipEvent_t ev_fork = nullptr, ev_score_done = nullptr;
  kprn_batch* dropin_slot[4] = {nullptr, nullptr, nullptr, nullptr};   // feed slots of the host-buffer entry points (kprn_train_step: 0 / 1, kprn_forward: 2 / 3)
  int dropin_next_train = 0, dropin_next_score = 0, dropin_last = 0;
  // The inline feed of kprn_train_step uploads on the upload stream (beside the previous step's backward) when every reader of the slot it refills is known to be
  // done: the slot was last read two calls ago, and the previous call WAITED for its own step's loss, i.e. for a kernel ordered behind that reader (option
  // "inline_upload" = "side", default; "main": on the engine's stream as in round 4).  kprn_train_step always waits for its loss stage (whether or not the
  // caller asked for the loss); the flag is consumed by the NEXT kprn_train_step (dropin_prev_waited_now: valid during that call's feed only) and set again
  // only by a call that succeeded, so a failed call never lends its predecessor's guarantee to its successor.
  bool dropin_prev_waited = false, dropin_prev_waited_now = false; int inline_upload_side = 1;
  bool inline_side_ok = true;   // (slots::feed: false when the handle still referred to the slot being refilled -- its rows are copied out in stream order first)
  bool score_pending = false;     // a pass is (possibly) still running on score_stream
  int bf16_bptt_dxe = 8;          // option "bf16_bptt_dxe": the persistent BPTT launch also forms dx for the entity slice (weight ring depth 8 | 16; 0: a separate product)
  int persist_layers = 1;     // option "persist_layers": generic fp32 LSTM / rnn layers as one persistent launch per layer where the shape allows (layer_f32_persist.hip)
  int persist_layers_grid = 0;   // option "persist_layers_grid": > 0 caps the workgroup count of those launches (tests: several tiles per workgroup at small N); 0: min(tiles, CUs)
  bool small_tables_fwd = true;   // option "small_tables_fwd": the fused D = H = 64 forward multiplies [S | x_e] by [Q ; W_i2g[:, e cols]^T] in layer 0 (lstm_fused_fwd.hip fwd_body IDENT)
  bool head_select = true;        // option "head_select": the fused fp32 forward's head forms column classId alone when no reader of the pass needs another (lstm_fused_fwd.hip head_tile_sel)
  bool small_tables = true;       // option "small_tables": generic fp32 pipelines (LSTM / rnn cells) form the layer-0 type / relation gradients from G (generic_pipeline.hip small_tables_route)
  float* lp_wot = nullptr; int64_t lp_wot_cap = 0;     // layer_f32_persist.hip: W_o2g^T of the layer whose BPTT launch is queued
  float* st_ctmp = nullptr; int64_t st_ctmp_cap = 0;   //   ... its [GH][ns + de] product result
  bool bf16_small_tables = true;  // option "bf16_small_tables": configs[3] backward forms the type / relation gradients from G = dA^T [S_r | S_t] (lstm_bf16.hip)
  int bf16_t_pad = 64;            // option "bf16_t_pad": pad (elements, a multiple of 8, <= 512) of the row pitch of dA^T / Z^T on the small-table route
  Bf16GemmOpts bf16_gemm;         // options "bf16_gemm_touch" / "bf16_gemm_regstage" / "bf16_gemm_pingpong"
  bool small_tiles_on = true;     // option "small_tiles": batches of <= 8 192 paths run on tiles of one 16-row m-tile (no identical-prefix plan)
  // option "tile_handover": the fused D = H = 64 BACKWARD launches let a tile change workgroups once between two of its steps, so that the workgroups'
  // step sums differ by less than a step (lstm_fused_common.h ho_plan).  "2" (default): workgroup b is paired with b + G / 2; "1": with G - 1 - b; "0": whole
  // tiles only (the A/B reference).  ho_fault: page-locked word a kernel sets when its wait for the other workgroup's state timed out -- every later API
  // call then fails instead of returning numbers computed from a stale slot
  int tile_handover = 2; int* ho_fault = nullptr;
  bool adam_merged = true;        // option "adam_merged": the row update and the dense arena's update of an Adam step in one launch
  bool bwd_pipe = true;           // option "bwd_pipe": small batches, two layers: both layers' BPTT in one launch, the bottom layer a step behind the top layer
  int score_dual = 2;             // option "score_dual": a queued scoring pass rides in the next training forward's launch (fused::forward_dual): 0 never | 1 always | 2 small batches
  bool catchup_prefix = true;     // option "catchup_prefix": a batch's row catch-up and its identical-prefix table in one launch (fused path)
  bool fused_small_tables = true; // option "fused_small_tables": the fused path's type / relation table gradients formed inside the bottom BPTT launch (one-hot MFMAs on dx)
  float score_split = 0.f;        // option: fraction of a scoring pass's tiles deferred to kprn_forward_batch_async_rest
  // option "score_rest_in_backward": the deferred part of a split pass is placed by the fused backward itself, right behind its last BPTT launch -- it runs on the side
  // stream beside the step's serial tail (prefix backward, gradient gather-reduce, slab reduce), whose latency-bound launches leave most CUs idle; the update joins it
  int score_rest_in_backward = 0;
  // option "score_rest_before_bptt": the deferred part goes out right behind the loss stage, BEFORE the BPTT launches, on a stream of the LOWEST priority: its
  // single-tile workgroups only get the CUs the first BPTT launch leaves idle in its tail (235 of 256 workgroups draw 18 tile-steps, 21 draw 20: DESIGN.md 7-1) and
  // finish inside the second launch's start-up skew -- a quarter of the scoring pass in time the step's schedule wastes anyway (the first part then ends 4 tile-steps earlier)
  int score_rest_before_bptt = 0;
  hipStream_t rest_stream = nullptr; hipEvent_t ev_part1 = nullptr;
  void (*after_bptt_hook)(kprn_handle*) = nullptr;   // (kprn_set_option installs score::rest_hook: lstm_fused_bwd.hip cannot see launch_score_rest)
  const kprn_batch* score_rest_batch = nullptr; int score_rest_cid = 1; int64_t score_rest_tile0 = 0;   // the deferred part of a split pass
  bool last_forward_side = false; // kprn_read_probs reads the side buffers
  bool score_on_main = false;     // ... which the last pass filled from the MAIN stream ("score_dual")
  const kprn_batch* pool_defer_batch = nullptr; int pool_defer_cid = 0;   // ... and whose pooling stage rides in the loss stage's launch that follows
  float* S2 = nullptr; float* sel2 = nullptr; int64_t cap_N2 = 0, cap_B2 = 0;
  int reserve_cus = 0;          // CUs the SCORING forward leaves free (a collective's copy kernels run beside it; kprn_set_option)
  int32_t last_B = 0;
  // ranking stage (rank_groups.hip): the score board = device-resident scores addressed by global line number.  kprn_board_put copies a pass's output
  // on the stream that produced it; a put queued on the scoring stream leaves ev_put behind it (put_side: not yet waited for by the main stream)
  float* board = nullptr; int64_t board_n = 0;
  hipEvent_t ev_put = nullptr; bool put_side = false;
  void* rank_buf = nullptr; size_t rank_buf_bytes = 0;   // device arguments and results of one kprn_rank_groups / kprn_rank_targets call
  void* sub_buf = nullptr; size_t sub_buf_bytes = 0;     // device arguments of one kprn_batch_subset call (the kept pairs' offsets, first source rows, pair numbers)
  int rank_sort_min = 512;   // option "rank_sort_min": counting wins at 257 members, the sort at 512 and above (profiles/rank/README.md, comparison 3)
  void* rank_pin = nullptr; size_t rank_pin_bytes = 0, rank_pin_off[2] = {0, 0};   // page-locked group table and top-K rows of kprn_recommend_ragged
  void* explain_buf = nullptr; size_t explain_buf_bytes = 0;   // device pair list and results of one kprn_explain_batch call
  void* explain_pin = nullptr; size_t explain_pin_bytes = 0;   // page-locked explanation rows of kprn_recommend_explain_ragged
  std::vector<kprn_graph*> graphs;                     // path_find.hip: the knowledge graphs alive on this handle (kprn_destroy frees what is left)
  void* pf_buf = nullptr; size_t pf_buf_bytes = 0;     // device arguments of one kprn_find_paths call (pairs, totals, first rows, counts, flag; per-walk counts)
  void* pf_keep = nullptr; size_t pf_keep_bytes = 0;   // option "path_cap" = "spread": the kept ranks of one find call, [rows of the batch] int64 beside the pairs' rows
  int path_cap = 0;                                    // option "path_cap": 0 "first" | 1 "spread" (path_find_dev.h CAP_*), read by every find call that has a seed
  std::vector<kprn_sampler*> samplers;                 // neg_sample.hip: the negative samplers alive on this handle (kprn_destroy frees what is left)
  void* ns_buf = nullptr; size_t ns_buf_bytes = 0;     // device arguments and results of one sampling call (users or positives, negatives, n_found)
  // candidates.hip: the handle's candidate list = the (user, item) rows of the last successful kprn_find_candidates, [cand_total][2] (cand_total < 0: none yet)
  int32_t* cand_list = nullptr; int64_t cand_total = -1; int32_t cand_Ve = 0;
  int64_t* cand_paths = nullptr;                       // the list's path counts [cand_total], row for row: kprn_find_candidates_top leaves them, kprn_find_candidates none
  void* cand_buf = nullptr; size_t cand_buf_bytes = 0; // device arguments of one kprn_find_candidates(_top) call (first rows, users, counts, flag, the users' bitmaps or tallies)

  // option "deterministic": every float sum of a training step whose addends come from different waves or workgroups of one launch is formed in an order that
  // depends on the batch and the launch geometry only; pipelines that cannot do that refuse to train
  // "2" (generic fp32 pipelines too): 1 and 2 launch the same kernels wherever 1 trains; 2 adds the slab forms of the generic backward's joins
  int deterministic = 0;
  int loss_bpr = 0;            // option "loss": 0 "bce" (nn.BCECriterion per pair) | 1 "bpr" (the pairwise loss over the batch's groups, include/kprn.h "pairwise loss")
  // option "pool_gamma": the LogSumExp reducer's temperature (include/kprn.h "pooling temperature").  pool_ig = (float)(1.0 / (double)pool_gamma)
  // is what every pooling, loss and explanation launch takes; both are 1 unless cfg.reducer == 2
  float pool_gamma = 1.0f, pool_ig = 1.0f;
  DetScratch det_slab;         // "2": where the generic backward's producers plain-store their partials (one buffer: producer and join are stream-ordered)
  float* det_seg = nullptr; int64_t det_seg_cap = 0;   // "2": bidx::DetEntity::seg_part of the row-major entity gradient [segments][2][de]
  // option "dropout" (rnn cell, fp32): nn.Dropout on every layer's step input in TRAINING forwards.  Masks are regenerated, never stored:
  // drop_draw counts the training forwards since the seed was set; the backward of a step uses the draw of its forward (drop_draw_cur)
  float dropout_p = 0.f;
  uint64_t dropout_seed = 0;   // default cfg.seed + cfg.rank (kprn_create)
  uint32_t drop_draw = 0, drop_draw_cur = 0;
  bool drop_live = false;      // the state saved by the last generic training forward was dropped (what generic::backward must undo)
  float* det_norm_part = nullptr;   // [SUMSQ_DET_BLOCKS of optim_step.hip] per-workgroup partials of the gradient norm

  bool prof_on = false;

  std::string prof_filter;  // profile only the kernel families whose name starts with this ("": all)
  std::map<std::string, ProfEntry> prof;
  struct Pending { std::string name; hipEvent_t a, b;  int launches = 1; };
  std::vector<Pending> prof_pending;
  std::vector<hipEvent_t> event_pool;
};

// ---- profiling scope: HIP events on the handle's stream ------------------------------------
struct ProfScope {
  kprn_handle* h; const char* name; hipEvent_t a = nullptr, b = nullptr;
  int launches = 1;  // launches of the family this scope spans (one event pair around several back-to-back launches)
  hipStream_t strm;  // the stream the family is launched on (the handle's, unless given)
  ProfScope(kprn_handle* h_, const char* n, hipStream_t on = nullptr);
  ~ProfScope();
};
hipStream_t make_concurrent_stream(kprn_handle* h, int* probes = nullptr);   // a stream whose work runs BESIDE the main stream's (score_stages.hip: probed, not assumed)
void prof_drain(kprn_handle* h);
void join_score(kprn_handle* h);  // main stream waits for the scoring pass on the side stream, if any

// ---- the C ABI's frame: device selected, the hand-over fault checked, exceptions -> status + kprn_last_error ----------------
#define API_BEGIN(h)                                   \
  if (!(h)) return KPRN_E_ARG;                         \
  try {                                                \
    HIP_TRY(hipSetDevice((h)->cfg.device_id));         \
    if ((h)->ho_fault && *(volatile int*)(h)->ho_fault) throw KprnError{KPRN_E_DEVICE, "a fused kernel's tile hand-over wait timed out: results since then are invalid"};
#define API_END(h)                                                                        \
  }                                                                                       \
  catch (const KprnError& e) { (h)->err = e.msg; return e.code; }                         \
  catch (const std::exception& e) { (h)->err = e.what(); return KPRN_E_DEVICE; }          \
  catch (...) { (h)->err = "unknown error"; return KPRN_E_DEVICE; }                       \
  return KPRN_OK;

// ---- host waits for the handle's streams, each set named once.  nothrow: the destroy routes and the profiler ignore a failed wait ----
inline void sync_stream(hipStream_t s, bool nothrow) { const hipError_t e = hipStreamSynchronize(s); if (!nothrow) HIP_TRY(e); }
inline void sync_side_streams(kprn_handle* h, bool nothrow = false) {   // scoring, rest: where passes run beside the main stream
  for (hipStream_t s : {h->score_stream, h->rest_stream}) if (s) sync_stream(s, nothrow);
}
inline void sync_compute_streams(kprn_handle* h, bool nothrow = false) { sync_side_streams(h, nothrow); sync_stream(h->stream, nothrow); }   // ... and main
inline void sync_all_streams(kprn_handle* h, bool nothrow = false) {    // ... and the two that fill slots: nothing queued anywhere reads a slot afterwards
  sync_compute_streams(h, nothrow);
  for (hipStream_t s : {h->feed_stream, h->upload_stream}) if (s) sync_stream(s, nothrow);
}
// a non-blocking stream of the highest or the lowest priority (each priority class has hardware queues of its own)
inline hipStream_t make_priority_stream(bool high) {
  int lo = 0, hi = 0;   // (lo = the numerically largest value = the LOWEST priority)
  hipStream_t s = nullptr;
  HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
  HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, high ? hi : lo));
  return s;
}

// ---- kprn_api.hip, for the slot code and the scoring stage: what training and scoring share ---------------------
bool use_fused(kprn_handle* h, const kprn_batch* b, bool save_for_backward);   // this pass over b runs on the fused D = H = 64 path
void materialize_step_rows(kprn_handle* h);  // the optimiser's row list stops being a view of a batch: copied to the handle's own storage
void check_batch(kprn_handle* h, const kprn_batch* b, int class_id);   // a fed slot is ready, class_id in 1..C
void ensure_ws_common(kprn_handle* h, int64_t N, int64_t B, int64_t n_wg = 0);
void pool_stage(kprn_handle* h, const kprn_batch* b, int cid, bool every_class);   // reducer + sigmoid + select on h->stream over ws.S into ws.sel (and the mirror, if armed)
void forward_impl(kprn_handle* h, const kprn_batch* b, int class_id, bool save_for_backward, bool do_pool = true, bool every_class = true, bool all_scores = false);
int dropin_feed(kprn_handle* h, bool score, const int32_t* idx, const float* labels, int32_t B, int32_t P, int32_t T, int32_t F, const int32_t* counts = nullptr,
                int64_t n_ragged = 0);   // the host-buffer entry points' minibatch -> the feed slot h->dropin_slot[h->dropin_last]; a status, its text in h->err
void materialize_union(kprn_handle* h);      // a gathered gradient still pending -> the summed rows in g_We + the sorted union list (no-op when there is none)
int64_t dp_tail_words(const kprn_handle* h); // words of the dense gradient arena riding behind the packed rows of the data-parallel exchange
// ---- the optimiser step (optim_step.hip): gradient norm, dense sweep, lazy-exact row update of the entity table, zeroPadTokens ----------------
namespace kk_dev { struct AdamRowsArgs; }    // adam_rows_dev.h
namespace optim {
void opt_check(const kprn_handle* h, const kprn_opt* o);    // what a kprn_opt may not ask of this handle; throws before a step launches or writes anything
void apply_update(kprn_handle* h, const kprn_opt* o);       // one optimiser step on the gradients the handle holds
void catch_up(kprn_handle* h, const kprn_batch* b);         // the batch's entity rows that are behind opt_step are replayed
void flush_lazy(kprn_handle* h);                            // every entity row is brought up to opt_step (before anything reads the whole table)
void zero_pad_tokens(kprn_handle* h);                       // MyOptimizer:zeroPadTokens: the three pad rows = 0
void step_tab_reserve(kprn_handle* h, int64_t need);        // the step-size table holds entry `need`
}  // namespace optim
// ---- the scoring stage (score_stages.hip): passes beside the main stream, the score board, ranking and explanation calls ----------------
void launch_score_rest(kprn_handle* h);      // the deferred part of a split scoring pass goes out now (no-op when there is none)
namespace score {
void join_put(kprn_handle* h);    // main stream waits for the board puts queued on the scoring stream, if any
void rest_hook(kprn_handle* h);   // kprn_handle::after_bptt_hook under option "score_rest_in_backward"
}  // namespace score
// ---- batches and feed slots (batch_slots.hip): the lifecycle of a kprn_batch and the kprn_batch_* / kprn_host_* entry points ----------------
namespace slots {
// ids that are already on the device: fill(idx_dev, s) queues on s whatever writes the batch's [N,T,F] ids into the slot's idx block (kprn_find_paths)
typedef std::function<void(int32_t* idx_dev, hipStream_t s)> DeviceFill;
// a new batch, ready on return (kprn_batch_create / _create_ragged); counts != null: ragged, N paths (P ignored); else B * P paths.  idx == null with
// fill: nothing is uploaded, fill writes the ids, and validation, prefix plan and occurrence index run over them where they are
void create(kprn_handle* h, const int32_t* idx, const int32_t* counts, const float* labels, int32_t B, int32_t P, int64_t N, int32_t T, int32_t F, kprn_batch** out,
            const DeviceFill* fill = nullptr);
// (re)fills *slot asynchronously (kprn_batch_feed_*_async); inline_now: derived on the calling thread (the host-buffer entry points)
void feed(kprn_handle* h, kprn_batch** slot, const int32_t* idx, const float* labels, const int64_t* rows, int32_t B, int32_t P, int32_t T, int32_t F,
          bool inline_now = false, const int32_t* counts = nullptr, int64_t n_ragged = 0);
void ready(kprn_handle* h, const kprn_batch* b);   // first use of a fed slot: waits for its feed, takes the summary over; KPRN_E_INDEX for a bad id
void release(kprn_batch* b);                       // frees a slot the handle no longer refers to, behind drained streams
}  // namespace slots

// ---- kernels (kernels_basic.hip) -----------------------------------------------------------
namespace kk {
void validate_indices(hipStream_t s, const int32_t* idx, int64_t nsteps, int F, int nT, int Vt, int Ve, int Vr, int32_t* flag);
void embed_gather(hipStream_t s, const int32_t* idx, int64_t N, int T, int F, int nT, const float* Wt, const float* We,
                  const float* Wr, int dt, int de, int dr, float* X, bool time_major, float* mask = nullptr /* MaskZero's row mask of X, same pass */);
void lstm_gates_fwd(hipStream_t s, float* act /*[N][4H] in: pre-act, out: gates*/, const float* c_prev, float* c, float* h, int64_t N, int H);
void lstm_gates_bwd(hipStream_t s, const float* act, const float* c, const float* c_prev, const float* dH_up /*nullable*/,
                    float* dH, float* dC, float* dA, int64_t N, int H);
void row_nonzero(hipStream_t s, const float* in, int64_t N, int D, float* mask);
// dropout.hip: embed_gather (time-major) writing the DROPPED rows, mask from the undropped values; out = in (.) m s over [T][N][W] rows (out may be in)
void embed_gather_drop(hipStream_t s, const int32_t* idx, int64_t N, int T, int F, int nT, const float* Wt, const float* We, const float* Wr, int dt, int de,
                       int dr, float* X, float* mask, const philox::DropArgs& a);
void drop_rows(hipStream_t s, const float* in, float* out, int64_t N, int T, int W, const philox::DropArgs& a);
void rnn_cell_fwd(hipStream_t s, float* pre, const float* bh, const float* mask, float* h, int64_t N, int H, int relu);
void rnn_cell_bwd(hipStream_t s, const float* pre, const float* hcur, const float* mask, const float* dH_up, const float* dH, float* dA, int64_t N,
                  int H, int relu);
void add_bias_rows(hipStream_t s, float* Y, const float* b, int64_t rows, int cols);
void add_into(hipStream_t s, float* dst, const float* src, int64_t n);   // dst[i] += src[i]
// det (here and below): the workgroups' partials leave as slabs in det's scratch and slab_join adds them in workgroup order (no atomics)
void col_sum_add(hipStream_t s, const float* A, int64_t rows, int cols, float* out, int64_t ld = 0, float* out2 = nullptr,   // ld: row stride of A (0 = cols); out2: also += there
                 DetScratch* det = nullptr);
// n floats of det's scratch (grown if need be: the stream is drained first)
float* det_reserve(DetScratch* det, hipStream_t s, int64_t n);
// dst[r * ldc + c] += ((slab 0 + slab 1) + slab 2) + ... over nslab slabs of [rows][cols] floats, `stride` floats apart: one running fp32 sum per element in slab
// order, one owner thread per element (sixteen slabs requested at a time); dst2 (nullable): the same sum is added there too
void slab_join(hipStream_t s, const float* slabs, int nslab, int64_t stride, int64_t rows, int cols, float* dst, int64_t ldc, float* dst2 = nullptr);
void gru_gates_fwd(hipStream_t s, float* a, const float* hp, int64_t N, int H);
void gru_out_fwd(hipStream_t s, float* a, const float* hp, float* h, int64_t N, int H);
void gru_bwd1(hipStream_t s, const float* a, const float* hp, const float* dH, const float* dH_up, float* dA, float* dHdir, int64_t N, int H);
void gru_bwd2(hipStream_t s, const float* a, const float* hp, float* dA, const float* dHdir, float* dH, int64_t N, int H);
// A second, independent job the loss-stage launch can carry in extra workgroups: WT[m] = W[m]^T for up to four [256][64]
// matrices (the fused backward's transposed LSTM weights, stale after every update).
struct TransposeJob { const float* W[4]; float* WT[4]; int n; };
// ... and the pooling stage of a scoring pass that ran in the training forward's launch ("score_dual"): reducer + sigmoid + select of ITS batch, as more
// workgroups of the loss stage's launch (B = 0: none)
struct PoolJob { const float* S; int B, P, cid; float* sel; float* sel_host; const int32_t* off = nullptr; int wave = 0; };
// a batch as the reducer sees it: B pairs of P paths each (rectangular: Segs{B, P, nullptr, nullptr, 0, 0}), or (off != null) pair b = paths
// off[b] .. off[b+1]-1; wg / n_wg: the loss stage's workgroup table of a ragged batch; wave: a wave per pair instead of a thread per pair
struct Segs { int B, P; const int32_t* off; const int32_t* wg; int n_wg; int wave; };
// segment limits of a ragged batch (DESIGN.md 'ragged batches')
// the pooling temperature's accepted range: option "pool_gamma", kprn_host_explain_gamma and a checkpoint's header word 14 (false for a NaN)
inline bool pool_gamma_ok(double g) { return g >= 1e-3 && g <= 1e3; }
inline float pool_ig_of(float gamma) { return (float)(1.0 / (double)gamma); }
constexpr int RAGGED_MAX_SEG = 4096;    // longest pair kprn_host_ragged_plan accepts
constexpr int RAGGED_THREAD_MAX = 28;    // longest pair a single thread reduces (the reference's largest path count: reduce_col's range)
constexpr int RAGGED_WG_PAIRS = 16;      // pairs per loss-stage workgroup, rectangular or ragged
constexpr int RAGGED_WG_PATHS = 448;     // paths per loss-stage workgroup (16 pairs of 28); a longer pair has a workgroup to itself
// offsets [B+1], workgroup table wg [<= B+1], summary {n_wg, max_cnt, wave}; false: a count < 1 or > RAGGED_MAX_SEG, or sum != N
bool ragged_plan(const int32_t* counts, int32_t B, int64_t N, int32_t* off, int32_t* wg, int32_t* summary);
// loss_stage.hip.  Reducer + sigmoid + select of a scoring pass; pooled / probs null: the selected class only.  The ragged forms launch when g.off is set.
// ig (here and in the two loss stages): kprn_handle::pool_ig, the LogSumExp reducer's inverse temperature (option "pool_gamma"; 1.0f = the plain reducer's bits)
void pool_sigmoid(hipStream_t s, const float* S, const Segs& g, int C, int reducer, int K, float ig, float* pooled, float* probs, int cid, float* sel,
                  float* sel_host = nullptr);
// the loss stage of a training step; the ragged form launches when the batch or the passenger pooling job is ragged.  Returns the number of partials
// (slot_of nullable: dS[slot_of[n]]; partial_host: optional page-locked mirror of the per-workgroup loss partials)
int loss_stage(hipStream_t s, const float* S, const float* labels, const Segs& g, int C, int cid, int reducer, int K, float ig, int literal, float invB,
               float* sel, float* dS, const int32_t* slot_of, float* partial, const TransposeJob* tj = nullptr, float* partial_host = nullptr, const PoolJob* pj = nullptr);
// the loss stage under option "loss" = "bpr": a workgroup per group of the table go [G+1] (device), the same passengers; returns G, the number of partials
constexpr int PAIRWISE_MAX_GROUP = 1024;   // pairs per group (KPRN_PAIRWISE_MAX_GROUP)
int loss_stage_pairwise(hipStream_t s, const float* S, const float* labels, const Segs& g, const int32_t* go, int G, int C, int cid, int reducer, int K, float ig,
                        float scale, float* sel, float* dS, const int32_t* slot_of, float* partial, const TransposeJob* tj = nullptr, float* partial_host = nullptr,
                        const PoolJob* pj = nullptr);
void count_pair_terms(hipStream_t s, const float* labels, const int32_t* go, int G, int64_t* out);   // *out (device) = sum over the groups of positives x negatives
const char* pairwise_groups_why(const int32_t* go, int32_t G, int32_t B);   // what is wrong with a (host) group table over B pairs, or null
void sum_partials(hipStream_t s, const float* partial, int n, float* out, int accumulate);
int loss_partials(int B);  // number of per-workgroup loss partials the loss stage writes for B pairs of a rectangular batch (sizes the partial buffer)
void head_bwd(hipStream_t s, const float* dS, const float* hT, const float* Wout, int64_t N, int H, int cid, float* dH, float* gWout, float* gbout,
              DetScratch* det = nullptr);
// det: the one-hot product route only (embed_scatter_det_ok) with skip_entity; anything else throws KPRN_E_UNSUPPORTED
void embed_scatter(hipStream_t s, const int32_t* idx, int64_t N, int T, int F, int nT, const float* dX /*[T][N][D]*/, int dt, int de, int dr,
                   int Vt, int Vr, float* gWt, float* gWe, float* gWr, bool skip_entity = false, DetScratch* det = nullptr);
bool embed_scatter_det_ok(int dt, int dr, int Vt, int Vr);   // both small tables go to k_table_grad_mfma (at most 128 rows, slices of at most 128 columns)
// Small tables (generic fp32 pipelines; lstm_bf16.hip has the bf16 twin and the derivation): with x = [Wt[type] | We[entity] | Wr[relation]] the
// type / relation blocks of dW_i2g and both table gradients follow from G = dA^T [S_r | S_t] (one-hot selectors):
//   dW_i2g[:, relation cols] = G_r Wr,  dWr = G_r^T W_i2g[:, relation cols]   (likewise for the type table)
// onehot_cols: X[(t N + n) ldx + col0 + j] = 1 iff j is the position's relation (j < Vr) or Vr + its type; j < ns (the columns [col0, col0 + ns) of the
// saved step input are overwritten in place: the backward reads X only as the dW product's operand).
void onehot_cols(hipStream_t s, const int32_t* idx, int64_t N, int T, int F, int Vr, int Vt, float* X, int64_t ldx, int col0, int ns);
// Ct [GH][ns + de] = dA^T [S | x_e] -> gWi[:, entity cols] += Ct[:, ns:], gWi[:, type / relation cols] += G Wt / G Wr, gWt += G_t^T Wi_t, gWr += G_r^T Wi_r
// (ct_has_entity = false: Ct = G [GH][ns], the entity columns of gWi are formed elsewhere -- the fused path)
void small_tables_finish(hipStream_t s, const float* Ct, int ns, int GH, int Din, int dt, int de, int dr, int Vt, int Vr, const float* Wt, const float* Wr,
                         const float* Wi, float* gWi, float* gWt, float* gWr, bool ct_has_entity = true);
void pack_rows(hipStream_t s, float* G, const int32_t* rows, const int32_t* count, int64_t max_rows, int d, int32_t* ids_out, float* rows_out, int32_t* count_out,
               const float* tail_src = nullptr, int64_t n_tail = 0, float* tail_dst = nullptr);
void fill_uniform(hipStream_t s, float* x, int64_t n, float a, uint64_t seed, uint64_t offset);
void clear_rows(hipStream_t s, float* G, const int32_t* rows, const int32_t* count, int64_t max_rows, int d);   // (optim_step.hip) the listed rows of G = 0
}  // namespace kk

// ---- ranking stage (rank_groups.hip) -------------------------------------------------------------
namespace rk {
struct Args {   // device pointers; members / pos / ranks / tk_idx + tk_score / hist may be null
  const float* scores; const int64_t* members; const int64_t* goff; const int32_t* pos;
  int G, mode, K, hist_len;
  int32_t* ranks; int32_t* tk_idx; float* tk_score; unsigned long long* hist;
  int sort_min;   // groups of this many members and more are sorted in LDS, smaller ones counted
};
// the refusals of kprn_rank_groups / kprn_host_rank_groups on host arrays: KPRN_OK, or the status with its text in *why; *max_n = the longest group
int validate(int64_t n_scores, const int64_t* members, const int64_t* goff, const int32_t* pos, int32_t G, int32_t mode, int32_t K, int32_t hist_len,
             int* max_n, std::string* why);
void launch(hipStream_t s, const Args& a, int max_n);   // hist must be zero; every group is ranked by exactly one of the two kernels
}  // namespace rk

// ---- ranking targets in groups of any size (rank_targets.hip; the rule, the refusals and the host twin: rank_targets_host.h) ------------------
namespace rt {
struct Args {   // device pointers; members may be null; goff indexes members from 0 when it is not
  const float* scores; const int64_t* members; const int64_t* goff; const int64_t* toff; const int32_t* targets;
  int G, mode, hist_len;
  int32_t* places; unsigned long long* hist;
};
void launch(hipStream_t s, const Args& a);   // hist must be zero; one workgroup per group
}  // namespace rt

// ---- path finder (path_find.hip): kprn_graph_* / kprn_find_paths / kprn_host_find_paths ---------------
namespace pf {
void release_all(kprn_handle* h);   // kprn_destroy: the graphs still alive and the finder's argument buffer
}  // namespace pf
// ---- negative sampler (neg_sample.hip): kprn_sampler_* / kprn_sample_negatives / kprn_find_training_paths / kprn_host_sample_negatives ----
namespace ns {
void release_all(kprn_handle* h);   // kprn_destroy: the samplers still alive and the sampling calls' buffer
}  // namespace ns
// ---- candidates of a user (candidates.hip): kprn_find_candidates(_top) / kprn_read_candidates / kprn_read_candidate_paths / kprn_find_paths_of_candidates /
// kprn_host_find_candidates(_top) ----
namespace cd {
void release_all(kprn_handle* h);   // kprn_destroy: the handle's candidate list and the call's buffer
}  // namespace cd

// ---- explanation stage (explain_paths.hip) -------------------------------------------------------
namespace ex {
struct Args {   // device pointers
  const float* S;            // mapper output [N][C] in the caller's path order
  const int32_t* off; int B, P;   // the batch's pairs: off [B+1], or null = P paths each
  int seg_wave;              // the batch pools a pair of more than RAGGED_THREAD_MAX paths by a wave (kprn_batch::seg_wave): pooled's order
  int C, cid, reducer, K, M;
  float ig;                  // LogSumExp's inverse pooling temperature (kprn_handle::pool_ig); Max and TopK never read it
  const int32_t* pairs;     // [n] pair per item; null = item i is pair i
  const int64_t* goff; int per_group;   // non-null: pairs holds a ranking's top-K rows [G][per_group] (index within the group, -1 = empty place)
  int64_t n;
  int32_t* idx; float* score; float* weight;   // [n][M]
  float* pooled; float* prob;                  // [n] or null
};
// the refusals on a host pair list: KPRN_OK, or the status with its text in *why
int validate(int32_t B, const int32_t* pairs, int64_t n, int32_t M, std::string* why);
void launch(hipStream_t s, const Args& a, int max_cnt);   // max_cnt: the batch's longest pair: <= RAGGED_THREAD_MAX = a thread per item, else a wave
}  // namespace ex

// ---- batch occurrence index (batch_index.hip) -------------------------------------------------
namespace bidx {
size_t scratch_bytes(int64_t n_index, int Ve);
// uniq: sorted distinct entity rows; *n_uniq_dev: their count.  tile_k / meta / kcap: identical-prefix plan (null, null, 0: none)
void build(hipStream_t s, const int32_t* idx, int64_t N, int T, int F, int Ve, const int32_t* tile_k, const int32_t* meta, int kcap,
           int32_t* key_sorted, int32_t* pos_sorted, int32_t* uniq, int32_t* n_uniq_dev, void* scratch, size_t scratch_sz);
size_t prefix_scratch_bytes(int64_t N, int kcap);
void prefix_plan(hipStream_t s, const int32_t* idx, int64_t N, int T, int F, int nT, int kcap, int32_t* idx_s, int32_t* perm, int32_t* slot_of, int32_t* tile_k,
                 int32_t* meta, void* scratch, size_t scratch_sz);
// Sum of the fused backward's per-workgroup weight-gradient slabs (lstm_fused_bwd.hip) -- a second, independent job that the
// entity-gradient launch can carry in extra workgroups (both run right after the backward kernels and neither fills the chip).
struct SlabReduce {
  const float* part[2]; float* gWi[2]; float* gWo[2]; float* gbi[2];
  int nslab, n_elem;   // slabs per layer, floats reduced per slab (2 * G * H + G rows: W_i2g | W_o2g | b, then optionally G)
  int slab;            // floats between two slabs
  float* gG[2];        // nullable: where that layer's elements past W_i2g | W_o2g | b go (the fused path's small-table identity: G [G * H][16])
  int L, ny;           // layers, slab-range splits
  const float* r1; int kmax, kcap, r1_stride, G, H;  // rank-1 terms of the identical-prefix steps; kmax = 0: none
};
__device__ __forceinline__ void slab_reduce_block(const SlabReduce& a, int bx, int by, int l) {
  const int i = bx * 256 + threadIdx.x;
  if (i >= a.n_elem) return;
  const int GH = a.G * a.H, nW = GH * a.H, nB = 2 * nW + GH;
  if (i >= nB && !a.gG[l]) return;
  const float* __restrict__ part = a.part[l];
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // sixteen slabs in flight per lane (four left the job latency-bound: 19 us for 68 MB, profiles/r03)
  for (int s = by * 4; s < a.nslab; s += a.ny * 16) {
    float x[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int sl = s + (u >> 2) * a.ny * 4 + (u & 3);
      // (unconditional load from a clamped slab, then the select: a load under a condition is a branch with the wait inside it)
      const float v = part[(int64_t)(sl < a.nslab ? sl : a.nslab - 1) * a.slab + i];
      x[u] = (sl < a.nslab) ? v : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u & 3] += x[u];
  }
  float v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  if (by == 0 && i < nB) {
    for (int t = 0; t < a.kmax; ++t) {
      const float* r1 = a.r1 + ((int64_t)l * a.kcap + t) * a.r1_stride;  // dA_{t+1}[GH] | dA_t[GH] | h_t[H] | in_t[H]
      if (i < nW) v += r1[GH + i / a.H] * r1[2 * GH + a.H + i % a.H];               // dW_i2g += dA_t (x) in_t
      else if (i < 2 * nW) v += r1[(i - nW) / a.H] * r1[2 * GH + (i - nW) % a.H];   // dW_o2g += dA_{t+1} (x) h_t
      else v += r1[GH + (i - 2 * nW)];                                               // db += dA_t
    }
  }
  if (i < nW) unsafeAtomicAdd(a.gWi[l] + i, v);
  else if (i < 2 * nW) unsafeAtomicAdd(a.gWo[l] + (i - nW), v);
  else if (i < nB) unsafeAtomicAdd(a.gbi[l] + (i - 2 * nW), v);
  else unsafeAtomicAdd(a.gG[l] + (i - nB), v);
}
// Third job the entity-gradient launch can carry: the type / relation table gradients of the fused path (nn.LookupTable backward for the
// two tiny tables, FeatureEmbedding.lua:29,41-49) from the bottom layer's fragment-order dx blocks: grad_table[v][:] = sum over the
// executed (path, step) positions with id == v of dx[:, slice].  One wave = one 16-column block of a slice; it walks (16-row block, t)
// items with one 1 KiB load each and keeps one accumulator per table row (<= 16 rows) per lane; a few atomics per wave at the end.
struct SmallGrad {
  const float* DX; const int32_t* idx; const int32_t* tile_k;
  int64_t N, n_mtiles; int T, F, nT, dt, de, dr, Vt, Vr;
  float* gWt; float* gWr; int nblocks;   // workgroups of this job
};
// DET (deterministic mode): the workgroup's [16][16] block leaves with plain stores (det_part[bx][v][c]); bidx::entity_grad_tail adds the blocks in workgroup order
template <bool DET = false>
__device__ __forceinline__ void small_grad_block(const SmallGrad& a, int bx, float* det_part = nullptr) {
  typedef float f32x4_ __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int arow = lane & 15, ag = lane >> 4;
  const int ncb_t = a.dt >> 4, ncb = ncb_t + (a.dr >> 4);
  // the four waves of a workgroup share one column block (their accumulators are summed in LDS: a quarter of the atomics)
  const int cb = bx % ncb, part = (bx / ncb) * 4 + wv, nparts = ((a.nblocks + ncb - 1) / ncb) * 4;
  const bool is_type = cb < ncb_t;
  const int wave_of_block = is_type ? cb : ((a.dt + a.de) >> 4) + (cb - ncb_t);   // 16-column block inside the D = 64 row
  const int idcol = is_type ? (a.F - a.nT - 2) : (a.F - 1);
  const int V = is_type ? a.Vt : a.Vr;
  // One-hot product on the matrix cores: grad[v][col] = sum_rows [id(row) == v] dx[row][col] is D += A B with A = one-hot [16 v x 4 k],
  // B = dx [4 k x 16 col] (v_mfma_f32_16x16x4_f32; 1.0 x is exact, fp32 accumulate).  MFMA r contracts over the rows {4 ag + r}: lane
  // (ag, arow) then holds exactly its B element (register r of its own fragment) and its A element (the id of its own row 4 ag + r
  // against v = arow) -- no shuffles, one compare per MFMA where the select form spent 16 compare-select-adds per element (which made
  // this job VALU-bound: 39 us of the 84 us launch).  D: lane (g, col) holds rows v = 4 g + i.
  f32x4_ acc = f32x4_{0.f, 0.f, 0.f, 0.f};
  const int64_t items = a.n_mtiles * a.T;
  // latency-bound (one 1 KiB block + 4 ids per item): the next item's loads are in flight while this one is accumulated
  auto fetch = [&](int64_t it, f32x4_& x, int (&id)[4]) -> bool {
    const int64_t mtile = it / a.T;
    const int t = (int)(it - mtile * a.T);
    // (the ids are requested before tile_k is known -- both loads in one round trip -- and discarded afterwards if the position is skipped)
    const int tk = a.tile_k ? a.tile_k[mtile >> 2] : 0;
    x = *(const f32x4_*)(a.DX + ((mtile * a.T + t) * 4 + wave_of_block) * 256 + lane * 4);
    int raw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = mtile * 16 + ag * 4 + r;
      const int rv = a.idx[((n < a.N ? n : a.N - 1) * a.T + t) * a.F + idcol];   // (unconditional, clamped: see slab_reduce_block)
      raw[r] = (n < a.N) ? rv : 0;
    }
    const bool live = !(t < tk);   // (wave-uniform) the prefix backward owns the skipped positions
#pragma unroll
    for (int r = 0; r < 4; ++r) id[r] = live ? raw[r] - 1 : -1;
    return live;
  };
  constexpr int DEPTH = 4;   // items in flight per wave (6 cost the whole launch two waves per SIMD of occupancy: the kernel is one register allocation)
  for (int64_t it0 = part; it0 < items; it0 += (int64_t)nparts * DEPTH) {
    f32x4_ x[DEPTH];
    int id[DEPTH][4];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const int64_t it = it0 + (int64_t)d * nparts;
      fetch(it < items ? it : items - 1, x[d], id[d]);   // (every item's loads issued, then the tail masked: no branch around a load)
      if (!(it < items)) { id[d][0] = id[d][1] = id[d][2] = id[d][3] = -1; }
    }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float onehot = (id[d][r] == arow) ? 1.f : 0.f;
        const float xv = (id[d][r] >= 0) ? x[d][r] : 0.f;   // (rows nobody owns may hold anything, and 0 x NaN is NaN)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(onehot, xv, acc, 0, 0, 0);
      }
  }
  __shared__ float sg_red[4][16][16];
#pragma unroll
  for (int i = 0; i < 4; ++i) sg_red[wv][4 * ag + i][arow] = acc[i];
  __syncthreads();
  {
    const int v = threadIdx.x >> 4, c = threadIdx.x & 15;   // 256 threads = 16 table rows x 16 columns
    const float s = (sg_red[0][v][c] + sg_red[1][v][c]) + (sg_red[2][v][c] + sg_red[3][v][c]);
    if constexpr (DET) { det_part[(int64_t)bx * 256 + threadIdx.x] = s; return; }
    if (v < V && s != 0.f) {
      if (is_type) unsafeAtomicAdd(a.gWt + (int64_t)v * a.dt + cb * 16 + c, s);
      else unsafeAtomicAdd(a.gWr + (int64_t)v * a.dr + (cb - ncb_t) * 16 + c, s);
    }
  }
}
// entity-table gradient = gather-reduce of dx over the occurrence index.  frag_order 1: the fused backward's fragment-order dx;
// 2: its compact entity slice [(n T + t)][de]; 0: time-major row-major [T][N][D] (generic pipeline).
// red / sg (nullable): the slab reduce / the small-table gradients carried by the same launch
// det (deterministic mode, frag_order 2 and, without passenger jobs, 0): the partial sums of runs that straddle segments and the small-table job's blocks go to det's scratch with plain
// stores, and entity_grad_tail -- a launch behind this one -- adds them in a fixed order
struct DetEntity {
  float* seg_part;   // [segments][2][de]: the part of a run that came in from the segment before | the part of the run this segment opens and hands on
  float* sg_part;    // [sg.nblocks][16][16]
};
void entity_grad(hipStream_t s, const float* DX, int frag_order, const int32_t* key_sorted, const int32_t* pos_sorted, int64_t n_index, int64_t N,
                 int T, int D, int dt, int de, int Ve, float* gWe, const SlabReduce* red = nullptr, const SmallGrad* sg = nullptr, const DetEntity* det = nullptr);
void entity_grad_tail(hipStream_t s, const int32_t* key_sorted, int64_t n_index, int de, int Ve, float* gWe, const DetEntity& det, const SmallGrad* sg);
size_t merge_scratch_bytes(int64_t n, int Ve);
void merge_rows(hipStream_t s, const void* all, int world, int cap, int de, int Ve, float* G, int32_t* union_rows, int32_t* union_count,
                int32_t* mark /*persistent [Ve], zero on entry and exit*/, void* scratch, size_t scratch_sz, int64_t tail_words = 0);
}  // namespace bidx

// ---- bf16 pipeline (lstm_bf16.hip; its products: gemm_bf16.hip / gemm_bf16.h): compute_dtype 1 with bf16 storage, FastLSTM, 8-element rows, >= 256 paths ----------------
namespace bf16p {
bool supported(const kprn_handle* h, const kprn_batch* b);
void forward(kprn_handle* h, const kprn_batch* b, bool save);
void backward(kprn_handle* h, const kprn_batch* b, int cid);
void params_changed(kprn_handle* h, bool entity_rows_only);   // parameters rewritten: shadows are stale (rows only: the dense arena + listed rows)
void rows_updated(kprn_handle* h, const int32_t* rows, const int32_t* count, int64_t max_rows);
void release(kprn_handle* h);
float debug_gemm16(kprn_handle* h, int64_t M, int N, int64_t K, int split_k, int iters);   // gemm_bf16.hip: ms per launch (kprn_debug_gemm what 5 / 6)
void debug_gemm16_run(kprn_handle* h, const kprn_gemm16_call& c, const float* A, const float* B, const float* bias, float* C, kprn_gemm16_ran* ran);   // gemm_bf16.hip: kprn_debug_gemm16_run
}  // namespace bf16p

// ---- fused D = H = 64 path (lstm_fused_*.hip): the host entry points ------------------------------------------------------------------
namespace fused {
bool fwd_supported(const kprn_handle* h, int T);
void forward(kprn_handle* h, const kprn_batch* b, bool save, int64_t tile_begin = 0, int64_t tile_end = -1, bool ignore_reserve = false, int sel = -1);
// small batches: tiles of ONE 16-row m-tile (four times as many workgroups, a quarter of the latency per tile); no identical-prefix plan
bool small_tiles(const kprn_handle* h, int64_t N, bool has_plan);
bool bwd_supported(const kprn_handle* h, int T);
void backward(kprn_handle* h, const kprn_batch* b, int cid);
void params_changed(kprn_handle* h);
bool transpose_job(kprn_handle* h, kk::TransposeJob* tj);
void prefix_forward(kprn_handle* h, const kprn_batch* b);
bool forward_dual(kprn_handle* h, const kprn_batch* bt, const kprn_batch* bs, float* S_score, int sel_train, int sel_score);
bool catch_up_with_prefix(kprn_handle* h, const kprn_batch* b, const kk_dev::AdamRowsArgs& rows);   // (optim::catch_up: b's rows and b's prefix table in one launch)
void mc_prepare(kprn_handle* h);
void forward_mc(kprn_handle* h, const kprn_batch* b, bool save);                     // (between the fused files)
bool prefix_backward(kprn_handle* h, const kprn_batch* b, int64_t n_tiles);         // (between the fused files)
void release(kprn_handle* h);
void handover_stats(kprn_handle* h, const kprn_batch* b, int64_t* out /*[4]: pairs, steps moved, longest workgroup in half steps without / with*/);
}  // namespace fused

// ---- generic fp32 pipeline (generic_pipeline.hip): every shape the two above do not take -- rnn, wide FastLSTM, gru, impl = generic ----------------
namespace generic {
void forward(kprn_handle* h, const kprn_batch* b, bool save);
void backward(kprn_handle* h, const kprn_batch* b, int cid);
// > 0: layer 0's input gradients take the small-table identity (the number of one-hot selector columns); the ONE statement of the route's conditions
int small_tables_route(const kprn_handle* h, int F, bool dropped, bool have_index);
void drop_check(const kprn_handle* h, const kprn_batch* b);   // option "dropout": the mask generator's addressing limits; throws before anything is launched
}  // namespace generic
void ensure_ws_generic(kprn_handle* h, int64_t N, int T);   // kprn_api.hip: the workspace the generic and the bf16 pipeline share

// ---- once per DEVICE -----------------------------------------------------------------------------------------
// hipFuncSetAttribute (the raised dynamic-LDS limit of a kernel) applies to the CURRENT device: a `static bool done` guard is per process, and the second
// GPU of a process (the data-parallel loopback and multichip tests hold several) then launches the kernel without it.  One bit per device ordinal.
struct PerDeviceOnce {
  unsigned long long mask = 0;
  bool need() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return true;
    const unsigned long long bit = 1ull << (d & 63);
    const unsigned long long old = __atomic_fetch_or(&mask, bit, __ATOMIC_RELAXED);
    return !(old & bit);
  }
};

// ---- environment switches ---------------------------------------------------------------------------------
// The shipped library reads a dozen environment variables, each set by a test that names it (README.md has the list).  Every other
// A/B and knock-out switch of the measurement rounds exists only in the measurement build (scripts/build_variants.py compiles the
// sources it lists with -DKPRN_PERSIST_VARIANTS): KPRN_DEV_ENV is nullptr in the shipped library, so those paths fold away.
#ifdef KPRN_PERSIST_VARIANTS
#define KPRN_DEV_ENV(name) getenv(name)
#else
#define KPRN_DEV_ENV(name) ((const char*)nullptr)
#endif
// KPRN_DBG: bit mask of cross-check modes the parity tests switch on (tests/test_gpu_parity.py: 64 = no identical-prefix plan, ...)
inline int kprn_dbg_mask() {
  static const int m = [] { const char* e = getenv("KPRN_DBG"); return e ? atoi(e) : 0; }();
  return m;
}

// ---- host side of the streaming feed (host_feed.hip) -------------------------------------------------
// Every device allocation goes through here.  KPRN_POISON_ALLOC=1 fills new memory with 0xFF bytes (NaN as float, -1 as int): nothing
// may depend on what hipMalloc returns (fresh pages are zero, recycled blocks are not) -- tests/test_gpu_parity.py runs a step that way.
inline hipError_t kprn_dev_malloc(void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) {
    static const bool poison = getenv("KPRN_POISON_ALLOC") != nullptr;
    if (poison) { e = hipMemset(*p, 0xFF, bytes); if (e == hipSuccess) e = hipDeviceSynchronize(); }  // (hipMemset may return before it has run)
  }
  return e;
}

template <typename T>
inline T* dalloc(int64_t n) {
  void* p = nullptr;
  if (n <= 0) n = 1;
  // 64 bytes of slack: the tiled GEMMs fetch 16-byte vectors that may straddle the end of a matrix's last row (gemm_tiled.hip)
  hipError_t e = kprn_dev_malloc(&p, (size_t)n * sizeof(T) + 64);
  if (e != hipSuccess) throw KprnError{KPRN_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e)};
  return (T*)p;
}
template <typename T>
inline void dfree(T*& p) { if (p) { hipFree(p); p = nullptr; } }
// Grow-only device scratch of the host code: need > cap -> drain the stream whose launches may still read the old block, free it, allocate `need` elements
// (dev_grow) or twice that (dev_grow2: lists whose length creeps up batch by batch), set the capacity.  Returns the buffer.
template <typename T>
inline T* dev_grow(hipStream_t s, T*& p, int64_t& cap, int64_t need, int factor = 1) {
  if (need > cap) {
    HIP_TRY(hipStreamSynchronize(s));
    dfree(p);
    p = dalloc<T>(need * factor);
    cap = need * factor;
  }
  return p;
}
template <typename T>
inline T* dev_grow2(hipStream_t s, T*& p, int64_t& cap, int64_t need) { return dev_grow(s, p, cap, need, 2); }
// Grow-only raw blocks whose size is a rule of their own (argument blocks, page-locked mirrors): need > cap -> wait for the streams whose queued work may still
// use the old block (only when there is one, or -- wait_if_empty -- whenever the block grows), free it, allocate alloc_bytes, record `record` (in cap's unit).
template <bool PINNED, typename T, typename C>
inline void grow_only(T*& p, C& cap, C need, size_t alloc_bytes, C record, std::initializer_list<hipStream_t> wait, bool wait_if_empty) {
  if (need <= cap) return;
  if (p || wait_if_empty) for (hipStream_t s : wait) HIP_TRY(hipStreamSynchronize(s));
  if (p) { if (PINNED) HIP_TRY(hipHostFree(p)); else hipFree(p); }
  p = nullptr; cap = 0;
  void* q = nullptr;
  if (PINNED) HIP_TRY(hipHostMalloc(&q, alloc_bytes));
  else if (const hipError_t e = kprn_dev_malloc(&q, alloc_bytes); e != hipSuccess) throw KprnError{KPRN_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e)};
  p = (T*)q; cap = record;
}
template <typename T, typename C> inline void grow_device(T*& p, C& cap, C need, size_t alloc_bytes, C record, std::initializer_list<hipStream_t> wait, bool wait_if_empty = false) { grow_only<false>(p, cap, need, alloc_bytes, record, wait, wait_if_empty); }
template <typename T, typename C> inline void grow_pinned(T*& p, C& cap, C need, size_t alloc_bytes, C record, std::initializer_list<hipStream_t> wait, bool wait_if_empty = false) { grow_only<true>(p, cap, need, alloc_bytes, record, wait, wait_if_empty); }
// the device arguments and results of ONE call (ranking, explanation, path finder, sampler): a quarter of headroom; s is drained whenever the block grows
inline void* grow_call_block(hipStream_t s, void*& p, size_t& bytes, size_t total) {
  grow_device(p, bytes, total, total + total / 4 + 64, total + total / 4, {s}, /*wait_if_empty=*/true);
  return p;
}

namespace hostfeed {
struct Shape { int B, P, T, F, nT, Vt, Ve, Vr; };
typedef kprn_batch::HostResult Result;
class Pool;
Pool* make_pool(int workers);
void free_pool(Pool* p);
std::future<void> submit(Pool* p, std::function<void()> fn);
// dst[i] = src row rows[i] (row_words int32 each), i < n: a shuffled minibatch read straight out of the file's array
// n score lines (counter \t %.5f \t %.14g) into out; returns the bytes written, or -(bytes needed) when cap is too small
int64_t format_scores(int64_t counter0, const float* probs, const float* labels, int64_t n, char* out, int64_t cap, int nth);
void gather_rows(int32_t* dst, const int32_t* src, int64_t row_words, const int64_t* rows, int64_t n, int nth);
void build(const Shape& g, const int32_t* idx, int kcap, int nth, bool want_index, Result* r, int32_t* idx_s, int32_t* perm, int32_t* slot_of, int32_t* tile_k,
           int32_t* pmeta, int32_t* key_sorted, int32_t* pos_sorted, int32_t* uniq, int32_t* w0, int32_t* w1, int32_t* w2, int32_t* w3);
}  // namespace hostfeed

// ---- one recurrent layer, all T steps, as ONE persistent fp32 launch (layer_f32_persist.hip): the wide shapes of the generic pipeline -------------
namespace lp32 {
bool supported(int cell /*0 FastLSTM, 1 rnn, 2 gru*/, int64_t N, int Din, int H, bool force /*any N (tests)*/);
// in [T][N][Din]; hs [T][N][H] (every step when save or write_all_h, else the last one); save: cs + gate values [T][N][4H] (FastLSTM) / pre-activations
// [T][N][H] (rnn) in the generic backward's layouts; mask [T][N] (rnn: MaskZero)
void forward_layer(hipStream_t s, int cell, const float* in, int64_t N, int T, int Din, int H, const float* Wi, const float* Wo, const float* bi, const float* bo,
                   float* hs, float* cs, float* act, const float* mask, int relu, bool save, bool write_all_h, const float* Wc = nullptr /*gru: c_i2h.weight*/,
                   const float* Uc = nullptr /*gru: c_h2h.weight*/, const float* bc = nullptr /*gru: c_i2h.bias*/,
                   int grid_cap = 0 /*option "persist_layers_grid": > 0 caps the launch's workgroup count; 0: min(tiles, CUs)*/);
// (gru: Wi / bi / Wo are i2g.weight [2H][Din] / i2g.bias / o2g.weight [2H][H]; act [T][N][4H] = [r | z | n | r * h'] when save)
// BPTT through the layer (cell backward of all T steps + dh_{t-1} = dA_t W_o2g) as one persistent launch; dA [T][N][GH] out (GH = 4H FastLSTM, H rnn)
bool bptt_supported(int cell, int64_t N, int H, bool force);
size_t bptt_scratch_floats(int H, int GH);
void bptt_layer(hipStream_t s, int cell, const float* act, const float* cs, const float* hs, const float* mask, const float* dHup, bool up, const float* Wo,
                float* wot, float* dA, int64_t N, int T, int H, int relu, const float* Uc = nullptr /*gru: c_h2h.weight; Wo = o2g.weight [2H][H], wot of bptt_scratch_floats(H, 3H)*/,
                float* dbias = nullptr, float* dbias2 = nullptr /*bptt_sums_bias(): the layer's bias gradient(s) += the column sums of dA, formed inside the launch*/,
                int grid_cap = 0 /*as forward_layer's*/);
bool bptt_sums_bias(int cell, int H);
}  // namespace lp32

// ---- GEMM (gemm_f32.hip): C[M,N] (+)= A(M,K) * B(K,N), arbitrary strides, fp32 MFMA -----------
namespace gemm {
// element (m,k) of A at A[m*sAm + k*sAk]; (k,n) of B at B[k*sBk + n*sBn]; C row-major ldc.
// accumulate: C += (atomic when split_k > 1); else C = A*B (+ bias[n]).
void run(hipStream_t s, const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc,
         int64_t M, int N, int64_t K, bool accumulate, const float* bias, int split_k, bool bf16 = false, bool untiled = false, DetScratch* det = nullptr);
// det (fp32, accumulate): split s plain-stores its partial product into slab s of a scratch [nsplit][M][N] and kk::slab_join adds the slabs to C in split order.
// The split count is capped so that one product's slabs stay within DET_SLAB_FLOATS (a function of M and N only).
constexpr int64_t DET_SLAB_FLOATS = (int64_t)1 << 24;   // 64 MiB
void run_untiled_slab(hipStream_t s, const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc, int64_t M, int N,
                      int64_t K, int64_t kchunk, int split_k, DetScratch* det);   // gemm_f32_slab.hip
// (untiled: keep the product off gemm_tiled.hip -- the GRU's split-K dW products, M = 2H / 3H = 500 / 750 rows: 1.53 against 2.06 ms, profiles/r06/bench_r_gru_*)
// gemm_tiled.hip: 128 x 128 x 32 LDS-tiled kernel (16-byte loads, XCD-aware tile order); false: shape / layout not covered
bool run_tiled(hipStream_t s, const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc, int64_t M, int N,
               int64_t K, bool accumulate, const float* bias, int split_k, DetScratch* det = nullptr);
// one recurrent step of one layer with the cell in the GEMM's epilogue: gates = [x_t | h_{t-1}] [W_i | W_o]^T + b
bool step_supported(const float* X, int64_t ldx, int Din, const float* Hprev, int64_t ldh, int H, const float* Wi, const float* Wo, int64_t N);
void lstm_step(hipStream_t s, const float* X, int64_t ldx, int Din, const float* Wi, const float* bi, const float* Hprev, const float* Wo,
               const float* Cprev, float* Cout, float* Hout, int64_t ldh, float* act, int64_t N, int H);
void rnn_step(hipStream_t s, const float* X, int64_t ldx, int Din, const float* Wi, const float* bi, const float* Hprev, const float* Wh,
              const float* bh, const float* mask, float* pre, float* Hout, int64_t ldh, int64_t N, int H, int relu);
}
