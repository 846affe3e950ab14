// libkprn.so -- C ABI (include/kprn.h) and step orchestration.
//
// One handle = the reference's training_net (MapReduce(predictor_net, reducer) + Sigmoid,
// release/songPathRnn/model/OneModel.lua:204-294) plus MyOptimizer's state
// (model/optimizer/MyOptimizer.lua:13-72), resident in HBM.
#include <ctype.h>
#include <dlfcn.h>
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <thread>

#include "kprn_internal.h"

static thread_local std::string g_create_error;

// ---------------------------------------------------------------------------------------
// profiling scopes
ProfScope::ProfScope(kprn_handle* h_, const char* n, hipStream_t on) : h(h_), name(n), strm(on ? on : h_->stream) {
  if (!h->prof_on) return;
  // an event pair costs ~4 us of stream time: a filter keeps the measurement of ONE kernel family from taxing all the others
  if (!h->prof_filter.empty() && strncmp(n, h->prof_filter.c_str(), h->prof_filter.size()) != 0) return;
  auto get = [&]() {
    hipEvent_t e;
    if (!h->event_pool.empty()) { e = h->event_pool.back(); h->event_pool.pop_back(); }
    else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
    return e;
  };
  a = get(); b = get();
  if (a) hipEventRecord(a, strm);
}
ProfScope::~ProfScope() {
  if (!h->prof_on || !a || !b) return;
  hipEventRecord(b, strm);
  h->prof_pending.push_back({name, a, b, launches});
  if (h->prof_pending.size() > 4096) prof_drain(h);
}
void prof_drain(kprn_handle* h) {
  if (h->prof_pending.empty()) return;
  sync_compute_streams(h, /*nothrow=*/true);
  for (auto& p : h->prof_pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      auto& e = h->prof[p.name];
      e.total_ms += ms;
      e.launches += p.launches;
    }
    h->event_pool.push_back(p.a);
    h->event_pool.push_back(p.b);
  }
  h->prof_pending.clear();
}

// ---------------------------------------------------------------------------------------
static void build_layout(kprn_handle* h) {
  const kprn_config& c = h->cfg;
  h->D = c.dt + c.de + c.dr;
  int64_t flat = 0, dn = 0;
  auto add = [&](const std::string& nm, int64_t rows, int64_t cols, int where, int64_t dev_off) {
    h->params.push_back({nm, flat, rows, cols, where, dev_off});
    flat += rows * cols;
  };
  h->off_Wt = dn; add("type_emb", c.Vt, c.dt, 0, dn); dn += (int64_t)c.Vt * c.dt;
  add("entity_emb", c.Ve, c.de, 1, 0);
  h->off_Wr = dn; add("relation_emb", c.Vr, c.dr, 0, dn); dn += (int64_t)c.Vr * c.dr;
  h->G = (c.rnn_type == 1) ? 1 : ((c.rnn_type == 2) ? 2 : 4);
  for (int l = 0; l < c.L; ++l) {
    const int Din = (l == 0) ? h->D : c.H;
    h->layer[l].Din = Din;
    const std::string ln = std::to_string(l + 1);
    if (c.rnn_type == 1) {  // nn.Recurrence(nn.MaskZero(...)): input2hidden / hidden2hidden nn.Linear, both with bias (OneModel.lua:231-232)
      h->layer[l].Wi = dn; add("rnn" + ln + ".i2h.weight", c.H, Din, 0, dn); dn += (int64_t)c.H * Din;
      h->layer[l].bi = dn; add("rnn" + ln + ".i2h.bias", c.H, 1, 0, dn); dn += c.H;
      h->layer[l].Wo = dn; add("rnn" + ln + ".h2h.weight", c.H, c.H, 0, dn); dn += (int64_t)c.H * c.H;
      h->layer[l].bo = dn; add("rnn" + ln + ".h2h.bias", c.H, 1, 0, dn); dn += c.H;
    } else if (c.rnn_type == 2) {  // nn.GRU: gates r, z from i2g (nn.Linear) + o2g (nn.LinearNoBias); candidate from its own pair of maps
      h->layer[l].Wi = dn; add("gru" + ln + ".i2g.weight", 2 * c.H, Din, 0, dn); dn += (int64_t)2 * c.H * Din;
      h->layer[l].bi = dn; add("gru" + ln + ".i2g.bias", 2 * c.H, 1, 0, dn); dn += (int64_t)2 * c.H;
      h->layer[l].Wo = dn; add("gru" + ln + ".o2g.weight", 2 * c.H, c.H, 0, dn); dn += (int64_t)2 * c.H * c.H;
      h->layer[l].Wc = dn; add("gru" + ln + ".c_i2h.weight", c.H, Din, 0, dn); dn += (int64_t)c.H * Din;
      h->layer[l].bc = dn; add("gru" + ln + ".c_i2h.bias", c.H, 1, 0, dn); dn += c.H;
      h->layer[l].Uc = dn; add("gru" + ln + ".c_h2h.weight", c.H, c.H, 0, dn); dn += (int64_t)c.H * c.H;
      h->layer[l].bo = -1;
    } else {
      h->layer[l].Wi = dn; add("lstm" + ln + ".i2g.weight", 4 * c.H, Din, 0, dn); dn += (int64_t)4 * c.H * Din;
      h->layer[l].bi = dn; add("lstm" + ln + ".i2g.bias", 4 * c.H, 1, 0, dn); dn += (int64_t)4 * c.H;
      h->layer[l].Wo = dn; add("lstm" + ln + ".o2g.weight", 4 * c.H, c.H, 0, dn); dn += (int64_t)4 * c.H * c.H;
      h->layer[l].bo = -1;
    }
  }
  h->off_outW = dn; add("out.weight", c.C, c.H, 0, dn); dn += (int64_t)c.C * c.H;
  h->off_outb = dn; add("out.bias", c.C, 1, 0, dn); dn += c.C;
  h->n_dense = dn;
  h->n_ent = (int64_t)c.Ve * c.de;
  h->n_params = flat;
}

static const ParamInfo* find_param(kprn_handle* h, const char* name) {
  if (!name) return nullptr;
  for (auto& p : h->params) if (p.name == name) return &p;
  return nullptr;
}

// parameters were written from outside the optimiser: every steady-state shortcut is off
static void params_touched(kprn_handle* h) {
  join_score(h);
  h->pad_clean = false;
  h->caught_serial = -1;
  fused::params_changed(h);
  bf16p::params_changed(h, false);
}

// the optimiser's row list: a view of the batch's distinct-row list until something needs an owned copy
static void view_step_rows(kprn_handle* h, const kprn_batch* b) {
  h->rows_view = b->uniq; h->count_view = b->uniq + b->uniq_cap; h->view_batch = b;
  h->step_rows_ub = b->n_uniq;
}

void materialize_step_rows(kprn_handle* h) {
  if (!h->view_batch) { h->rows_view = h->step_rows; h->count_view = h->step_count; return; }
  const kprn_batch* b = h->view_batch;
  int64_t need = std::max<int64_t>(b->n_uniq, 1);
  dev_grow2(h->stream, h->step_rows, h->step_rows_cap, need);
  if (b->n_uniq > 0)
    HIP_TRY(hipMemcpyAsync(h->step_rows, b->uniq, (size_t)b->n_uniq * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->step_count, b->uniq + b->uniq_cap, sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  h->step_rows_ub = b->n_uniq;
  h->rows_view = h->step_rows; h->count_view = h->step_count; h->view_batch = nullptr;
}

// loss partials a training step over b may write: the BCE stage's workgroups (rectangular / ragged), or one per group of the pairwise stage
static int64_t batch_partials(const kprn_batch* b) { return std::max<int64_t>(b->n_wg, b->n_groups); }

void ensure_ws_common(kprn_handle* h, int64_t N, int64_t B, int64_t n_wg) {
  const int64_t np = std::max<int64_t>(kk::loss_partials((int)B), n_wg);   // (n_wg: the loss-stage workgroups of a ragged batch, the groups of a pairwise loss)
  dev_grow2(h->stream, h->loss_partial, h->loss_partial_cap, np);
  Workspace& w = h->ws;
  const kprn_config& c = h->cfg;
  if (N > w.cap_Nc) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    dfree(w.S); dfree(w.dS);
    w.S = dalloc<float>(N * c.C);
    w.dS = dalloc<float>(N * 2 + 16);  // [N] grads + [B<=N] per-pair loss terms
    w.cap_Nc = N;
  }
  if (B > w.cap_B) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    dfree(w.pooled); dfree(w.probs); dfree(w.sel); dfree(w.dy);
    w.pooled = dalloc<float>(B * c.C);
    w.probs = dalloc<float>(B * c.C);
    w.sel = dalloc<float>(B);
    w.dy = dalloc<float>(B);
    w.cap_B = B;
  }
  h->score_buf = w.S;
}

void ensure_ws_generic(kprn_handle* h, int64_t N, int T) {
  Workspace& w = h->ws;
  const kprn_config& c = h->cfg;
  const int H = c.H, L = c.L, D = h->D;
  if (N > w.cap_N || T > w.cap_T) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    int64_t cn = std::max<int64_t>(N, w.cap_N);
    int ct = std::max(T, w.cap_T);
    dfree(w.X); dfree(w.Hs); dfree(w.Cs); dfree(w.ACT); dfree(w.dA); dfree(w.dIn); dfree(w.dH); dfree(w.dC); dfree(w.mask);
    w.mask = dalloc<float>((int64_t)L * ct * cn);
    w.X = dalloc<float>(cn * ct * D);
    w.Hs = dalloc<float>((int64_t)L * ct * cn * H);
    w.Cs = dalloc<float>((int64_t)L * ct * cn * H);
    w.ACT = dalloc<float>((int64_t)L * ct * cn * 4 * H);
    w.dA = dalloc<float>((int64_t)ct * cn * 4 * H);
    w.dIn = dalloc<float>((int64_t)ct * cn * std::max(D, H));
    w.dH = dalloc<float>(cn * H);
    w.dC = dalloc<float>(cn * H);
    w.cap_N = cn; w.cap_T = ct;
  }
}

// every_class: also pooled / probs of all C classes (what kprn_forward_batch can hand out); else the selected class only
void pool_stage(kprn_handle* h, const kprn_batch* b, int cid, bool every_class) {
  const kprn_config& c = h->cfg;
  Workspace& w = h->ws;
  ProfScope ps(h, "pool_sigmoid");
  const kk::Segs g{b->B, b->P, b->off, b->wg, b->n_wg, b->seg_wave};
  kk::pool_sigmoid(h->stream, w.S, g, c.C, c.reducer, c.K, h->pool_ig, every_class ? w.pooled : nullptr, every_class ? w.probs : nullptr, cid, w.sel, h->sel_host_armed);
}

void check_batch(kprn_handle* h, const kprn_batch* b, int class_id) {
  KPRN_REQUIRE(b != nullptr, KPRN_E_ARG, "batch is NULL");
  slots::ready(h, b);  // (a slot filled by kprn_batch_feed_async: its feed was issued a step ago)
  KPRN_REQUIRE(class_id >= 1 && class_id <= h->cfg.C, KPRN_E_ARG, "classId must be in 1..C (nn.Select(2,classId), MyOptimizer.lua:126)");
}

// A TRAINING call runs on the fused path (forward + backward): the one statement of it, for use_fused and for det_check.
// compute_dtype 0 (f32 MFMA), 2 (f32x6: exact fp32 products from bf16 pieces on the matrix cores) and 3: fused forward + fp32 backward; 1 (bf16 products): the
// fused matrix-core forward for scoring only, the generic or bf16 pipeline for training.  Embedding ablations (dt = 0 / de = 0) run on the generic pipeline.
static bool trains_fused(const kprn_handle* h, int T) {
  const kprn_config& c = h->cfg;
  return h->impl == 0 && c.rnn_type == 0 && c.compute_dtype != 1 && c.dt != 0 && c.de != 0 && fused::fwd_supported(h, T) && fused::bwd_supported(h, T);
}
bool use_fused(kprn_handle* h, const kprn_batch* b, bool save_for_backward) {
  if (save_for_backward) return trains_fused(h, b->T);
  return h->impl == 0 && h->cfg.rnn_type == 0 && h->cfg.dt != 0 && h->cfg.de != 0 && fused::fwd_supported(h, b->T);
}

// all_scores: the caller reads S itself, every column of it (path_scores).  The fused fp32 forward's head forms column classId alone unless a reader of the pass
// needs other columns (option "head_select"): the training forward never does (the loss stage and the BPTT launches read S[:, cid] and W_out[cid]), a scoring
// pass does when its pooling stage runs for every class or the caller copies S.
void forward_impl(kprn_handle* h, const kprn_batch* b, int class_id, bool save_for_backward, bool do_pool, bool every_class, bool all_scores) {
  check_batch(h, b, class_id);
  const int64_t N = b->N;
  const int sel = (save_for_backward || !(every_class || all_scores)) ? class_id - 1 : -1;
  optim::catch_up(h, b);
  ensure_ws_common(h, N, b->B, batch_partials(b));
  if (use_fused(h, b, save_for_backward)) {
    bool dual = false;
    if (save_for_backward && h->score_dual && h->score_rest_batch && h->score_rest_tile0 == 0 && h->ev_score_done) {
      // a deferred scoring pass ("score_dual") rides in this training forward's launch; its pooling stage follows on this stream, and the event the
      // pass's readers wait for is recorded here
      const kprn_batch* sb = h->score_rest_batch;
      score::join_put(h);   // (a board put queued on the scoring stream still reads sel2, which this pass's pooling stage writes from THIS stream)
      dual = fused::forward_dual(h, b, sb, h->S2, sel, h->score_rest_cid - 1);   // (the pass's pooling stage reads its own class's column)
      if (dual) {
        h->score_rest_batch = nullptr;
        h->pool_defer_batch = sb; h->pool_defer_cid = h->score_rest_cid - 1;   // (its pooling stage: more workgroups of the loss stage's launch, backward_impl)
        // the pass is now part of THIS stream's order: nothing is pending on the side stream, and no event is recorded for it here (an event record is
        // 6 us of idle queue in front of the loss stage at 256 paths) -- kprn_read_probs orders its copy behind this stream when somebody reads
        h->score_pending = false;
        h->score_on_main = true;
      }
    }
    if (!dual) fused::forward(h, b, save_for_backward, 0, -1, false, sel);
  } else if (!b->idx_valid) {
    throw KprnError{KPRN_E_ARG, "this label-less batch was fed for the fused kernels (plan only); feed it again after changing impl"};
  } else if (bf16p::supported(h, b)) {
    ensure_ws_generic(h, N, b->T);   // (fp32 cell state, dx, h_T and the head's buffers are shared with the generic pipeline)
    bf16p::forward(h, b, save_for_backward);
  } else {
    ensure_ws_generic(h, N, b->T);
    generic::forward(h, b, save_for_backward);
  }
  if (do_pool) pool_stage(h, b, class_id - 1, every_class);
  // a training forward beside (or carrying) a queued scoring pass leaves that pass the one kprn_read_probs / kprn_board_put hand out: its pair count stays
  // (a pass of MORE pairs than the training batch could not be read otherwise)
  if (!(save_for_backward && h->last_forward_side)) h->last_B = b->B;
}

static void dp_release(kprn_handle* h);
// words of the dense gradient arena riding behind the packed rows (padded so that every rank's slice of the gathered buffer keeps
// 16-byte alignment)
int64_t dp_tail_words(const kprn_handle* h) { return h->dp_dense_in_pack ? ((h->n_dense + 3) & ~(int64_t)3) : 0; }

// a union recorded by kprn_sparse_grad_merge (dp_fused_update) -> the summed rows in g_We + the sorted union list, as the unfused merge
// leaves them
void materialize_union(kprn_handle* h) {
  if (!h->dp_union_pending) return;
  h->dp_union_pending = false;
  const int64_t n = (int64_t)h->dp_world * h->dp_cap;
  const size_t need = bidx::merge_scratch_bytes(n, h->cfg.Ve);
  grow_device(h->bidx_scratch, h->bidx_scratch_bytes, need, need * 2, need * 2, {h->stream}, /*wait_if_empty=*/true);
  if (!h->dp_mark) {
    h->dp_mark = dalloc<int32_t>(h->cfg.Ve);
    HIP_TRY(hipMemsetAsync(h->dp_mark, 0, (size_t)h->cfg.Ve * sizeof(int32_t), h->stream));
  }
  ProfScope ps(h, "dp_merge_rows");
  bidx::merge_rows(h->stream, h->dp_all, h->dp_world, h->dp_cap, h->cfg.de, h->cfg.Ve, h->g_We, h->step_rows, h->step_count, h->dp_mark, h->bidx_scratch,
                   h->bidx_scratch_bytes, dp_tail_words(h));
  h->view_batch = nullptr; h->rows_view = h->step_rows; h->count_view = h->step_count;
  h->step_rows_ub = std::min<int64_t>(n, h->cfg.Ve);
  h->ent_grads_dirty = true;
}

// zeroGradParameters (MyOptimizer.lua:186): dense arena memset; entity rows cleared by list
static void zero_grads(kprn_handle* h) {
  if (h->dp_union_pending) {   // a gathered gradient nobody applied: the pack moved the rows out of g_We, so there is nothing to clear
    h->dp_union_pending = false; h->ent_grads_dirty = false; h->step_rows_ub = 0;
  }
  if (!h->dense_grads_clean) HIP_TRY(hipMemsetAsync(h->g_dense, 0, (size_t)h->n_dense * sizeof(float), h->stream));
  if (!h->view_batch) { h->rows_view = h->step_rows; h->count_view = h->step_count; }
  if (h->ent_grads_dirty && h->step_rows_ub > 0 && h->rows_view)
    kk::clear_rows(h->stream, h->g_We, h->rows_view, h->count_view, h->step_rows_ub, h->cfg.de);
  h->ent_grads_dirty = false;
  h->dense_grads_clean = true;
}

// the loss of the last backward = fixed-order sum of the loss stage's per-workgroup partials, formed on demand
static void form_loss(kprn_handle* h) {
  if (h->loss_pending <= 0) return;
  kk::sum_partials(h->stream, h->loss_partial, h->loss_pending, h->d_loss, h->loss_accumulate);
  h->loss_pending = 0;
}

// Option "deterministic": a training call goes on only where every float sum of the step has a fixed order.  "1": the fused fp32 path (D = H = 64,
// FastLSTM, compute_dtype 0 / 2 / 3) on its index routes.  "2": that path exactly as under "1", and the generic fp32 pipeline (FastLSTM and rnn cells, compute_dtype
// 0) with the slab forms of its joins.  Everything else is refused HERE, before anything is launched or any state is written.  b == null (kprn_train_step, before its
// feed): the handle's part of the check; the batch's part follows in kprn_train_step_batch.
static const char* det_fused_why(const kprn_handle* h) {
  const kprn_config& c = h->cfg;
  if (!(c.num_types == 1 && (c.dt % 16) == 0 && (c.de % 16) == 0 && (c.dr % 16) == 0 && c.Vt <= 16 && c.Vr <= 16))
    return "the fused path's general embedding scatter (more than one type slot, slices not in 16-column blocks, or a type / relation table of more than 16 rows)";
  if (kprn_dbg_mask() & (1 | 8 | 16)) return "a KPRN_DBG route of the fused path (scatter kernels with atomics)";
  return nullptr;
}
static void det_check(const kprn_handle* h, int T, const kprn_batch* b = nullptr) {
  if (!h->deterministic) return;
  const kprn_config& c = h->cfg;
  const char* why = nullptr;
  // the fused path trains where use_fused(.., true) says so, under "2" exactly as under "1"
  if (trains_fused(h, T)) why = det_fused_why(h);
  else if (h->deterministic == 1) {
    if (h->impl != 0) why = "the generic pipeline (impl = generic: split-K atomics in its weight-gradient products)";
    else if (c.rnn_type != 0) why = "the rnn / gru pipeline";
    else if (c.compute_dtype == 1) why = "the bf16 pipeline (compute_dtype 1)";
    else why = "the generic pipeline (this shape is not the fused D = H = 64 path's: wide persistent layers / split-K products)";
  }
  else if (c.rnn_type == 2) why = "the gru pipeline";
  else if (c.compute_dtype == 1) why = "the bf16 pipeline or the generic pipeline's bf16 products (compute_dtype 1)";
  else if (c.compute_dtype != 0) why = "the generic pipeline with a compute_dtype other than 0";
  else {
    // the generic fp32 pipeline.  Layer 0's table gradients: the small-table identity (no sums across workgroups but the split-K product's), or the scatter route,
    // whose one-hot products take tables of at most 128 rows x 128 columns (kernels_basic.hip table_grad_mfma; the kernels behind it have no deterministic form).
    // The handle's facts: this call's forward drops iff the option is on; a batch without the index is refused below whichever route it would take
    const bool will_drop = h->dropout_p > 0.f && c.rnn_type == 1;
    if (!generic::small_tables_route(h, b ? b->F : 3, will_drop, /*have_index=*/true) && !kk::embed_scatter_det_ok(c.dt, c.dr, c.Vt, c.Vr))
      why = "the generic pipeline's general embedding scatter (a type / relation table of more than 128 rows or a slice of more than 128 columns)";
    else if (b && c.de > 0 && (b->key_sorted == nullptr || b->tile_k))
      why = "the generic pipeline's entity scatter (a batch without the occurrence index, or with an identical-prefix plan)";
  }
  if (why) throw KprnError{KPRN_E_UNSUPPORTED, std::string(h->deterministic == 1 ? "deterministic = 1" : "deterministic = 2") + ": training would run on " + why + ", which has no deterministic form; set deterministic = 0"};
}

// Option "loss" = "bpr": what the pairwise stage cannot serve, refused HERE, before anything is launched or any state is written.  b == null: kprn_train_step,
// whose host buffers carry no groups.  inv_batch: the caller's scale (kprn_train_step_batch passes none)
static void loss_check(const kprn_handle* h, const kprn_batch* b, float inv_batch) {
  if (!h->loss_bpr) return;
  KPRN_REQUIRE(b != nullptr, KPRN_E_UNSUPPORTED, "loss = bpr: kprn_train_step takes host buffers, which carry no group table; use a batch, kprn_batch_set_groups and kprn_train_step_batch");
  KPRN_REQUIRE(b->labels != nullptr && b->n_groups > 0, KPRN_E_ARG, "loss = bpr: the batch has no group table (kprn_batch_set_groups; a refill of the slot drops it)");
  KPRN_REQUIRE(h->cfg.world <= 1 || inv_batch > 0.f, KPRN_E_UNSUPPORTED,
               "loss = bpr with world > 1: the scale 1 / n_terms would be this rank's alone; pass inv_batch = 1 / (the ranks' terms together) to kprn_backward_batch");
}

static void backward_impl(kprn_handle* h, const kprn_batch* b, int class_id, int literal, float inv_batch) {
  check_batch(h, b, class_id);
  det_check(h, b->T, b);
  loss_check(h, b, inv_batch);
  generic::drop_check(h, b);
  KPRN_REQUIRE(b->labels != nullptr && b->has_index, KPRN_E_ARG, "batch has no labels (targets are required, MyOptimizer.lua:179)");
  const kprn_config& c = h->cfg;
  zero_grads(h);
  h->dense_grads_clean = false;
  forward_impl(h, b, class_id, true, /*do_pool=*/false);
  Workspace& w = h->ws;
  const int cid = class_id - 1;
  float invB = inv_batch > 0.f ? inv_batch : 1.0f / (float)b->B;
  if (inv_batch <= 0.f && c.world > 1) invB = 1.0f / ((float)b->B * (float)c.world);
  const bool fusedp = use_fused(h, b, true);
  {
    // pooling + sigmoid + select + BCE (or the pairwise loss over the batch's groups) + reducer backward in one launch (the nn.Linear head's weight gradient
    // is formed by the top layer's backward kernel, fused path, or by the generic pipeline's own head backward)
    ProfScope ps(h, h->loss_bpr ? "loss_stage_pairwise" : "loss_stage");
    kk::TransposeJob tj;  // fused path: the backward's W^T copies, stale after an update, are rebuilt by passenger workgroups
    const bool have_tj = fusedp && fused::transpose_job(h, &tj);
    kk::PoolJob pj{h->S2, 0, 0, 0, h->sel2, nullptr};
    if (h->pool_defer_batch) {
      const kprn_batch* sb = h->pool_defer_batch;
      pj.B = sb->B; pj.P = sb->P; pj.off = sb->off; pj.wave = sb->seg_wave; pj.cid = h->pool_defer_cid; h->pool_defer_batch = nullptr;
    }
    const kk::Segs g{b->B, b->P, b->off, b->wg, b->n_wg, b->seg_wave};   // (a ragged batch or a ragged passenger: the launcher takes the segmented form)
    if (h->loss_bpr) {
      const float scale = inv_batch > 0.f ? inv_batch : (b->n_terms > 0 ? 1.0f / (float)b->n_terms : 0.f);
      h->loss_pending = kk::loss_stage_pairwise(h->stream, h->score_buf, b->labels, g, b->groups + 2, b->n_groups, c.C, cid, c.reducer, c.K, h->pool_ig, scale, w.sel,
                                                w.dS, fusedp ? b->slot_of : nullptr, h->loss_partial, have_tj ? &tj : nullptr,
                                                h->loss_early_armed ? h->loss_mirror : nullptr, pj.B > 0 ? &pj : nullptr);
    } else
    h->loss_pending = kk::loss_stage(h->stream, h->score_buf, b->labels, g, c.C, cid, c.reducer, c.K, h->pool_ig, literal, invB, w.sel, w.dS,
                                     fusedp ? b->slot_of : nullptr, h->loss_partial, have_tj ? &tj : nullptr, h->loss_early_armed ? h->loss_mirror : nullptr, pj.B > 0 ? &pj : nullptr);
    if (h->loss_early_armed) {   // what kprn_train_step_batch waits for instead of the end of the step
      h->loss_early_n = h->loss_pending;
      HIP_TRY(hipEventRecord(h->ev_loss, h->stream));
    }
    if (h->loss_accumulate) form_loss(h);   // (one single-workgroup launch; otherwise the sum is formed when somebody asks)
  }
  view_step_rows(h, b);
  if (fusedp && h->score_rest_before_bptt && h->score_rest_batch) launch_score_rest(h);   // (kprn_internal.h: into the first BPTT launch's idle tail)
  // (no join with a scoring pass on the side stream here: the backward writes nothing that pass reads -- gradients, dx, prefix sums --
  //  and making the main stream wait for the pass's last workgroups cost 3 % of the step; apply_update joins before it writes parameters)
  if (fusedp) fused::backward(h, b, cid);
  else if (bf16p::supported(h, b)) bf16p::backward(h, b, cid);
  else generic::backward(h, b, cid);
  h->ent_grads_dirty = true;
  h->grads_serial = b->serial;
}

// ---------------------------------------------------------------------------------------
extern "C" {

const char* kprn_version(void) { return "kprn-amd 0.1 gfx950 f32-mfma"; }

const char* kprn_last_error(const kprn_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int kprn_create(const kprn_config* cfg, kprn_handle** out) {
  if (!cfg || !out) { g_create_error = "kprn_create: NULL argument"; return KPRN_E_ARG; }
  *out = nullptr;
  kprn_handle* h = nullptr;
  try {
    const kprn_config& c = *cfg;
    KPRN_REQUIRE(c.Vt > 0 && c.Ve > 0 && c.Vr > 0, KPRN_E_ARG, "vocab sizes must be positive");
    // dt == 0: no entity-type table (-includeEntityTypes 0), de == 0: no entity table (-includeEntity 0): the embedding variants of
    // OneModel.lua:210-219 / FeatureEmbedding.lua:26-34,83-110 -- x_t = [types | relations], [entities | relations] or [relations]
    KPRN_REQUIRE(c.dt >= 0 && c.de >= 0 && c.dr > 0, KPRN_E_ARG, "embedding dims: relation > 0, type / entity >= 0 (0 = that table is not part of the model)");
    KPRN_REQUIRE(c.num_types >= 1, KPRN_E_ARG, "numEntityTypes must be >= 1");
    KPRN_REQUIRE(c.num_types <= c.F, KPRN_E_ARG, "assert(numEntityTypes <= numFeatureTemplates) (OneModel.lua:107)");
    KPRN_REQUIRE(c.F >= c.num_types + 2, KPRN_E_ARG, "numFeatureTemplates must cover types + entity + relation (FeatureEmbedding.lua:51)");
    KPRN_REQUIRE(c.H > 0 && c.C > 0, KPRN_E_ARG, "rnnHidSize and labelDimension must be positive");
    KPRN_REQUIRE(c.L >= 1 && c.L <= KPRN_MAX_LAYERS, KPRN_E_ARG, "numLayers must be in 1..8");
    KPRN_REQUIRE(c.compute_dtype >= 0 && c.compute_dtype <= 3, KPRN_E_ARG,
                 "compute_dtype must be 0 (f32 MFMA), 1 (bf16 MFMA products, f32 accumulate), 2 (f32x6: fp32 products from 3 bf16 pieces) or "
                 "3 (f32x3: from 2 fp16 pieces)");
    KPRN_REQUIRE(c.rnn_type >= 0 && c.rnn_type <= 2, KPRN_E_ARG, "rnn_type must be 0 (lstm), 1 (rnn) or 2 (gru)");
    KPRN_REQUIRE(c.reducer >= 0 && c.reducer <= 2, KPRN_E_ARG, "topK must be 0 (max), 1 (topK) or 2 (LogSumExp)");
    KPRN_REQUIRE(c.reducer != 1 || c.K >= 1, KPRN_E_ARG, "K must be >= 1 for the topK reducer");
    KPRN_REQUIRE(c.L == 1 || (c.dt + c.de + c.dr) == c.H, KPRN_E_ARG,
                 "numLayers > 1 needs totalInputEmbeddingDim == rnnHidSize: every layer is FastLSTM(D,H) (OneModel.lua:236,270-273)");
    KPRN_REQUIRE(c.world >= 1 && c.rank >= 0 && c.rank < c.world, KPRN_E_ARG, "bad rank/world");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    KPRN_REQUIRE(ndev > 0, KPRN_E_DEVICE, "no HIP device visible: libkprn has no CPU path");
    KPRN_REQUIRE(c.device_id >= 0 && c.device_id < ndev, KPRN_E_ARG, "device_id out of range");
    HIP_TRY(hipSetDevice(c.device_id));
    h = new kprn_handle();
    h->cfg = c;
    if (c.stream == KPRN_STREAM_LEGACY_DEFAULT) { h->stream = nullptr; h->own_stream = false; h->stream_known = true; }   // the null stream, by request
    else if (c.stream) { h->stream = (hipStream_t)c.stream; h->own_stream = false; h->stream_known = true; }
    else { HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; h->stream_known = false; }
    build_layout(h);
    h->dropout_seed = c.seed + (uint64_t)c.rank;   // (data-parallel replicas do not share masks)
    h->dense = dalloc<float>(h->n_dense); h->g_dense = dalloc<float>(h->n_dense);
    h->s1_dense = dalloc<float>(h->n_dense); h->s2_dense = dalloc<float>(h->n_dense);
    h->We = dalloc<float>(h->n_ent); h->g_We = dalloc<float>(h->n_ent);
    h->s1_We = dalloc<float>(h->n_ent); h->s2_We = dalloc<float>(h->n_ent);
    h->We_last = dalloc<int32_t>(c.Ve);
    h->d_loss = dalloc<float>(4); h->d_norm2 = dalloc<float>(4); h->d_flag = dalloc<int32_t>(4);
    h->step_count = dalloc<int32_t>(4);
    HIP_TRY(hipHostMalloc((void**)&h->h_pinned, 64 * sizeof(float)));
    hipStream_t s = h->stream;
    for (float* p : {h->g_dense, h->s1_dense, h->s2_dense}) HIP_TRY(hipMemsetAsync(p, 0, (size_t)h->n_dense * sizeof(float), s));
    for (float* p : {h->g_We, h->s1_We, h->s2_We}) HIP_TRY(hipMemsetAsync(p, 0, (size_t)h->n_ent * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(h->We_last, 0, (size_t)c.Ve * sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(h->d_loss, 0, 4 * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(h->step_count, 0, 4 * sizeof(int32_t), s));
    // param:uniform(-paramInit, paramInit) over training_net:parameters() (OneModel.lua:306-309)
    for (auto& p : h->params) {
      float* dst = (p.where == 1 ? h->We : h->dense) + p.dev_off;
      kk::fill_uniform(s, dst, p.rows * p.cols, c.param_init, c.seed, (uint64_t)p.flat_off);
    }
    if (c.rnn_type == 1 && c.rnn_init == 1) {
      // -rnnInitialization 1 (OneModel.lua:310-322): i2h.weight <- torch.eye(D, H) copied in STORAGE order into the [H, D]
      // tensor, h2h.weight <- eye(H), both biases <- 0
      for (int l = 0; l < c.L; ++l) {
        const int Din = h->layer[l].Din;
        std::vector<float> wi((size_t)c.H * Din, 0.f), wh((size_t)c.H * c.H, 0.f), z((size_t)c.H, 0.f);
        for (int r = 0; r < Din; ++r) if (r < c.H) wi[(size_t)r * c.H + r] = 1.f;  // eye(Din, H)[r][r], flat index r*H + r
        for (int r = 0; r < c.H; ++r) wh[(size_t)r * c.H + r] = 1.f;
        HIP_TRY(hipMemcpyAsync(h->dense + h->layer[l].Wi, wi.data(), wi.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->dense + h->layer[l].Wo, wh.data(), wh.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->dense + h->layer[l].bi, z.data(), z.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->dense + h->layer[l].bo, z.data(), z.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
      }
    }
    optim::step_tab_reserve(h, 1);
    HIP_TRY(hipStreamSynchronize(s));
    *out = h;
    return KPRN_OK;
  } catch (const KprnError& e) {
    g_create_error = e.msg;
    if (h) kprn_destroy(h);
    return e.code;
  } catch (const std::exception& e) {
    g_create_error = e.what();
    if (h) kprn_destroy(h);
    return KPRN_E_DEVICE;
  }
}

void kprn_destroy(kprn_handle* h) {
  if (!h) return;
  hipSetDevice(h->cfg.device_id);
  sync_compute_streams(h, /*nothrow=*/true);
  prof_drain(h);
  for (kprn_batch*& d : h->dropin_slot) if (d) { kprn_batch* old = d; d = nullptr; kprn_batch_destroy(h, old); }
  if (h->score_stream) { hipStreamDestroy(h->score_stream); hipEventDestroy(h->ev_fork); hipEventDestroy(h->ev_score_done); }
  if (h->ev_put) hipEventDestroy(h->ev_put);
  dfree(h->board);
  if (h->rank_buf) { hipFree(h->rank_buf); h->rank_buf = nullptr; }
  if (h->sub_buf) { hipFree(h->sub_buf); h->sub_buf = nullptr; }
  if (h->rank_pin) { hipHostFree(h->rank_pin); h->rank_pin = nullptr; }
  if (h->explain_buf) { hipFree(h->explain_buf); h->explain_buf = nullptr; }
  if (h->explain_pin) { hipHostFree(h->explain_pin); h->explain_pin = nullptr; }
  pf::release_all(h);
  ns::release_all(h);
  cd::release_all(h);
  if (h->feed_pool) { hostfeed::free_pool((hostfeed::Pool*)h->feed_pool); h->feed_pool = nullptr; }  // (joins the workers)
  if (h->upload_pool) { hostfeed::free_pool((hostfeed::Pool*)h->upload_pool); h->upload_pool = nullptr; }
  if (h->upload_stream) { hipStreamSynchronize(h->upload_stream); hipStreamDestroy(h->upload_stream); h->upload_stream = nullptr; }
  if (h->feed_stream) { hipStreamSynchronize(h->feed_stream); hipStreamDestroy(h->feed_stream); hipEventDestroy(h->ev_feed_fork); }
  if (h->feed_scratch) { hipFree(h->feed_scratch); h->feed_scratch = nullptr; }
  dp_release(h);
  dfree(h->S2); dfree(h->sel2); dfree(h->st_ctmp); dfree(h->lp_wot); dfree(h->ws.HsD);
  fused::release(h);
  bf16p::release(h);
  if (h->bidx_scratch) { hipFree(h->bidx_scratch); h->bidx_scratch = nullptr; }
  dfree(h->loss_partial);
  if (h->rest_stream) { hipStreamSynchronize(h->rest_stream); hipStreamDestroy(h->rest_stream); h->rest_stream = nullptr; }
  if (h->ev_part1) { hipEventDestroy(h->ev_part1); h->ev_part1 = nullptr; }
  if (h->loss_mirror) { hipHostFree(h->loss_mirror); h->loss_mirror = nullptr; }
  if (h->probs_mirror) { hipHostFree(h->probs_mirror); h->probs_mirror = nullptr; }
  if (h->ho_fault) { hipHostFree(h->ho_fault); h->ho_fault = nullptr; }
  if (h->ev_loss) { hipEventDestroy(h->ev_loss); h->ev_loss = nullptr; }
  for (auto e : h->event_pool) hipEventDestroy(e);
  Workspace& w = h->ws;
  for (float** p : {&w.X, &w.Hs, &w.Cs, &w.ACT, &w.dA, &w.dIn, &w.dH, &w.dC, &w.S, &w.dS, &w.pooled, &w.probs, &w.sel, &w.dy, &w.mask}) dfree(*p);
  for (float** p : {&h->dense, &h->g_dense, &h->s1_dense, &h->s2_dense, &h->We, &h->g_We, &h->s1_We, &h->s2_We, &h->d_loss, &h->d_norm2,
                    &h->step_tab, &h->det_norm_part, &h->det_slab.p, &h->det_seg})
    dfree(*p);
  for (int32_t** p : {&h->We_last, &h->d_flag, &h->step_rows, &h->step_count, &h->pack_buf, &h->dp_mark}) dfree(*p);
  if (h->step_tab_host) hipHostFree(h->step_tab_host);
  if (h->h_pinned) hipHostFree(h->h_pinned);
  if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
  delete h;
}

int kprn_num_params(kprn_handle* h, int64_t* n) {
  API_BEGIN(h)
  KPRN_REQUIRE(n, KPRN_E_ARG, "n is NULL");
  *n = h->n_params;
  API_END(h)
}

static int copy_named(kprn_handle* h, const char* name, float* dst, const float* src, int64_t n, int which /*0 param,1 grad*/) {
  API_BEGIN(h)
  const ParamInfo* p = find_param(h, name);
  KPRN_REQUIRE(p, KPRN_E_ARG, std::string("unknown parameter name: ") + (name ? name : "(null)"));
  KPRN_REQUIRE(n == p->rows * p->cols, KPRN_E_ARG, "element count does not match the tensor");
  if (n == 0) return KPRN_OK;   // (a table that is not part of the model: -includeEntity 0 / -includeEntityTypes 0)
  KPRN_REQUIRE(dst || src, KPRN_E_ARG, "NULL buffer");
  if (p->where == 1 && which == 0) optim::flush_lazy(h);
  if (which == 1) materialize_union(h);
  float* base;
  if (which == 0) base = (p->where == 1 ? h->We : h->dense);
  else base = (p->where == 1 ? h->g_We : h->g_dense);
  base += p->dev_off;
  if (dst) {
    HIP_TRY(hipMemcpyAsync(dst, base, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(base, src, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (which == 0) params_touched(h);
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  API_END(h)
}

int kprn_get_param(kprn_handle* h, const char* name, float* dst, int64_t n) { return copy_named(h, name, dst, nullptr, n, 0); }
int kprn_set_param(kprn_handle* h, const char* name, const float* src, int64_t n) { return copy_named(h, name, nullptr, src, n, 0); }
int kprn_get_grad(kprn_handle* h, const char* name, float* dst, int64_t n) { return copy_named(h, name, dst, nullptr, n, 1); }

// data-parallel exchange with the dense gradient arena riding in the packed row buffer (kprn_set_option "dp_dense_in_pack"): one collective
// per step instead of two.  The arena is copied behind the rows; after the all-gather every rank sums the W copies IN RANK ORDER (the same
// sequence of additions everywhere: bit-identical dense gradients on every replica by construction).
__global__ void k_dense_to_pack(const float* __restrict__ g, int64_t n, float* __restrict__ tail) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) tail[i] = g[i];
}
__global__ void k_dense_from_all(const float* __restrict__ all, int world, int64_t stride_words, int64_t tail_off, int64_t n, float* __restrict__ g) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float acc = all[tail_off + i];
    for (int r = 1; r < world; ++r) acc += all[(int64_t)r * stride_words + tail_off + i];
    g[i] = acc;
  }
}

// rows of one parameter tensor by 0-based row index (a 20 M-row entity table is 10 GB: reading the rows a batch touched must not copy it)
__global__ void k_rows_copy(float* __restrict__ W, const int64_t* __restrict__ rows, int64_t n, int64_t cols, float* __restrict__ buf, int to_table) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * cols; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = rows[i / cols], c = i % cols;
    if (to_table) W[r * cols + c] = buf[i]; else buf[i] = W[r * cols + c];
  }
}
static int copy_rows(kprn_handle* h, const char* name, const int64_t* rows, int64_t n_rows, float* dst, const float* src) {
  API_BEGIN(h)
  const ParamInfo* p = find_param(h, name);
  KPRN_REQUIRE(p, KPRN_E_ARG, std::string("unknown parameter name: ") + (name ? name : "(null)"));
  KPRN_REQUIRE(n_rows >= 0 && (rows || n_rows == 0) && (dst || src || n_rows == 0), KPRN_E_ARG, "NULL buffer");
  if (n_rows == 0 || p->rows * p->cols == 0) return KPRN_OK;
  for (int64_t i = 0; i < n_rows; ++i) KPRN_REQUIRE(rows[i] >= 0 && rows[i] < p->rows, KPRN_E_INDEX, "row index outside the tensor");
  if (p->where == 1) optim::flush_lazy(h);
  if (src) params_touched(h);   // (BEFORE the write is queued: it makes the main stream wait for a scoring pass that may still read these rows)
  float* base = (p->where == 1 ? h->We : h->dense) + p->dev_off;
  int64_t* d_rows = nullptr;
  float* d_buf = nullptr;
  try {
    d_rows = dalloc<int64_t>(n_rows);
    d_buf = dalloc<float>(n_rows * p->cols);
    HIP_TRY(hipMemcpyAsync(d_rows, rows, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    if (src) HIP_TRY(hipMemcpyAsync(d_buf, src, (size_t)(n_rows * p->cols) * sizeof(float), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_rows_copy, dim3((unsigned)std::min<int64_t>((n_rows * p->cols + 255) / 256, 8192)), dim3(256), 0, h->stream, base, d_rows, n_rows, p->cols, d_buf,
                       src ? 1 : 0);
    if (dst) HIP_TRY(hipMemcpyAsync(dst, d_buf, (size_t)(n_rows * p->cols) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  } catch (...) {
    hipStreamSynchronize(h->stream);
    dfree(d_rows); dfree(d_buf);
    throw;
  }
  dfree(d_rows); dfree(d_buf);
  API_END(h)
}
int kprn_get_param_rows(kprn_handle* h, const char* name, const int64_t* rows, int64_t n_rows, float* dst) { return copy_rows(h, name, rows, n_rows, dst, nullptr); }
int kprn_set_param_rows(kprn_handle* h, const char* name, const int64_t* rows, int64_t n_rows, const float* src) { return copy_rows(h, name, rows, n_rows, nullptr, src); }

static int copy_flat(kprn_handle* h, float* dst, const float* src, int64_t n, int which /*0 param,1 grad,2 s1,3 s2*/) {
  API_BEGIN(h)
  KPRN_REQUIRE(n == h->n_params, KPRN_E_ARG, "n must equal kprn_num_params");
  KPRN_REQUIRE(dst || src, KPRN_E_ARG, "NULL buffer");
  if (which != 1) optim::flush_lazy(h);
  else materialize_union(h);
  for (auto& p : h->params) {
    float* base;
    switch (which) {
      case 0: base = (p.where == 1 ? h->We : h->dense); break;
      case 1: base = (p.where == 1 ? h->g_We : h->g_dense); break;
      case 2: base = (p.where == 1 ? h->s1_We : h->s1_dense); break;
      default: base = (p.where == 1 ? h->s2_We : h->s2_dense); break;
    }
    base += p.dev_off;
    const size_t bytes = (size_t)(p.rows * p.cols) * sizeof(float);
    if (dst) HIP_TRY(hipMemcpyAsync(dst + p.flat_off, base, bytes, hipMemcpyDeviceToHost, h->stream));
    else HIP_TRY(hipMemcpyAsync(base, src + p.flat_off, bytes, hipMemcpyHostToDevice, h->stream));
  }
  if (!dst) params_touched(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  API_END(h)
}
int kprn_get_flat_params(kprn_handle* h, float* dst, int64_t n) { return copy_flat(h, dst, nullptr, n, 0); }
int kprn_set_flat_params(kprn_handle* h, const float* src, int64_t n) { return copy_flat(h, nullptr, src, n, 0); }
int kprn_get_flat_grads(kprn_handle* h, float* dst, int64_t n) { return copy_flat(h, dst, nullptr, n, 1); }
int kprn_get_flat_opt_state(kprn_handle* h, int32_t slot, float* dst, int64_t n) {
  if (slot != 0 && slot != 1) { if (h) h->err = "slot must be 0 or 1"; return KPRN_E_ARG; }
  return copy_flat(h, dst, nullptr, n, 2 + slot);
}

int kprn_zero_pad_tokens(kprn_handle* h) {
  API_BEGIN(h)
  // a no-op while the pad rows are known to be zero (the optimiser re-zeroes them at the end of every step, MyOptimizer.lua:219): the
  // data-parallel step calls this before every backward, and zeroing again made the main stream wait for the scoring pass on the side
  // stream and invalidated the fused kernels' derived weight copies -- 0.3 ms of a 1.5 ms step
  if (h->pad_clean) return KPRN_OK;
  optim::zero_pad_tokens(h);
  fused::params_changed(h);
  bf16p::params_changed(h, false);
  API_END(h)
}

// ---- batches and feed slots: batch_slots.hip; scoring, ranking and explaining: score_stages.hip ----------------------------------------------
// the host-buffer entry points' minibatch -> an engine-owned slot (0 / 1: training, 2 / 3: scoring), derived on the calling thread
extern "C++" int dropin_feed(kprn_handle* h, bool score, const int32_t* idx, const float* labels, int32_t B, int32_t P, int32_t T, int32_t F,
                             const int32_t* counts, int64_t n_ragged) {
  API_BEGIN(h)
  int& nx = score ? h->dropin_next_score : h->dropin_next_train;
  const int si = (score ? 2 : 0) + nx;
  nx ^= 1;
  if (!h->feed_build_host) {   // device-built feed selected: the plain create path of that build
    if (h->dropin_slot[si]) { kprn_batch* old = h->dropin_slot[si]; h->dropin_slot[si] = nullptr; kprn_batch_destroy(h, old); }
    slots::create(h, idx, counts, labels, B, P, n_ragged, T, F, &h->dropin_slot[si]);
  } else {
    slots::feed(h, &h->dropin_slot[si], idx, labels, nullptr, B, P, T, F, /*inline_now=*/true, counts, n_ragged);
  }
  h->dropin_last = si;
  API_END(h)
}

int kprn_embed(kprn_handle* h, const int32_t* idx, int64_t N, int32_t T, int32_t F, float* x) {
  API_BEGIN(h)
  KPRN_REQUIRE(idx && x && N > 0 && T > 0 && F == h->cfg.F, KPRN_E_ARG, "bad arguments");
  KPRN_REQUIRE(N < (1ll << 31), KPRN_E_ARG, "N too large");
  kprn_batch* b = nullptr;
  {
    int rc = kprn_batch_create(h, idx, nullptr, (int32_t)N, 1, T, F, &b);
    if (rc != KPRN_OK) return rc;
  }
  float* dx = nullptr;
  try {
    optim::catch_up(h, b);
    const kprn_config& c = h->cfg;
    dx = dalloc<float>(N * T * h->D);
    kk::embed_gather(h->stream, b->idx, N, T, F, c.num_types, h->dense + h->off_Wt, h->We, h->dense + h->off_Wr, c.dt, c.de, c.dr, dx, false);
    HIP_TRY(hipMemcpyAsync(x, dx, (size_t)N * T * h->D * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  } catch (...) { dfree(dx); kprn_batch_destroy(h, b); throw; }
  dfree(dx);
  kprn_batch_destroy(h, b);
  API_END(h)
}

int kprn_backward_batch(kprn_handle* h, const kprn_batch* b, int32_t class_id, int32_t bce_literal, float inv_batch, float* loss) {
  API_BEGIN(h)
  backward_impl(h, b, class_id, bce_literal, inv_batch);
  if (loss) {
    form_loss(h);
    HIP_TRY(hipMemcpyAsync(loss, h->d_loss, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    prof_drain(h);
  }
  API_END(h)
}

int kprn_apply_update(kprn_handle* h, const kprn_opt* opt) {
  API_BEGIN(h)
  optim::apply_update(h, opt);
  API_END(h)
}

int kprn_train_step_batch(kprn_handle* h, const kprn_batch* b, int32_t class_id, const kprn_opt* opt, float* loss) {
  API_BEGIN(h)
  optim::opt_check(h, opt);
  check_batch(h, b, class_id);
  det_check(h, b->T, b);
  loss_check(h, b, 0.f);
  generic::drop_check(h, b);
  optim::catch_up(h, b);
  if (!h->pad_clean) { optim::zero_pad_tokens(h); fused::params_changed(h); bf16p::params_changed(h, false); }  // MyOptimizer.lua:181 (a no-op when the last step left them zero)
  // the loss goes back as soon as the loss stage has run (option "train_step_return" = "loss"); profiling and "drain" wait for the whole step as before
  struct Disarm { kprn_handle* h; ~Disarm() { h->loss_early_armed = false; } } disarm{h};
  if (loss && !h->train_step_drain && !h->prof_on) {
    const int64_t np = std::max<int64_t>(kk::loss_partials(b->B), batch_partials(b));   // (as ensure_ws_common sizes the device partials)
    grow_pinned(h->loss_mirror, h->loss_mirror_cap, np, (size_t)(2 * np + 64) * sizeof(float), 2 * np + 64, {h->stream});
    if (!h->ev_loss) HIP_TRY(hipEventCreateWithFlags(&h->ev_loss, hipEventDisableTiming));
    h->loss_early_armed = true;
  }
  backward_impl(h, b, class_id, opt->bce_literal, 0.f);
  optim::apply_update(h, opt);
  if (loss && h->loss_early_armed) {
    HIP_TRY(hipEventSynchronize(h->ev_loss));
    float s = 0.f;   // k_sum_partials' order: one running fp32 sum over the partials in index order
    for (int i = 0; i < h->loss_early_n; ++i) s += h->loss_mirror[i];
    *loss = s;
  } else if (loss) {
    form_loss(h);
    HIP_TRY(hipMemcpyAsync(loss, h->d_loss, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    prof_drain(h);
  }
  API_END(h)
}

int kprn_train_step(kprn_handle* h, const int32_t* idx, int32_t B, int32_t P, int32_t T, int32_t F, const float* labels, int32_t class_id,
                    const kprn_opt* opt, float* loss) {
  if (!h) return KPRN_E_ARG;
  if (!labels) { h->err = "assert(targets) (MyOptimizer.lua:179)"; return KPRN_E_ARG; }
  try { optim::opt_check(h, opt); det_check(h, T); loss_check(h, nullptr, 0.f); } catch (const KprnError& e) { h->err = e.msg; return e.code; }   // (before the feed: a refused call uploads nothing)
  // The minibatch goes through one of two engine-owned feed slots (grow-only capacity, page-locked staging: steady state allocates nothing and
  // frees nothing; alternating, so that the rows the lazy optimiser still names belong to the OTHER slot) instead of a batch created and
  // destroyed per call (two device allocations, a device-side index build with its synchronisations and three stream drains per step:
  // 1.06 ms per 128-pair step against 0.38 ms for the step itself).
  // dropin_prev_waited says "the previous call waited for its own step's loss": it holds for exactly one call.  Taken and cleared here, so that a call
  // that fails anywhere below (an id out of range, a bad argument) leaves it false and the call after it uploads in stream order again.
  const bool prev_waited = h->dropin_prev_waited;
  h->dropin_prev_waited = false;
  h->dropin_prev_waited_now = prev_waited;   // (what the inline feed of THIS call reads)
  int rc = dropin_feed(h, /*score=*/false, idx, labels, B, P, T, F);
  h->dropin_prev_waited_now = false;
  if (rc != KPRN_OK) return rc;
  // (the loss is always fetched -- the call waits for the loss stage whether or not the caller passed `loss`: that wait is what lets the NEXT call's
  // upload run beside this step's backward)
  float l = 0.f;
  rc = kprn_train_step_batch(h, h->dropin_slot[h->dropin_last], class_id, opt, &l);
  h->dropin_prev_waited = (rc == KPRN_OK);
  if (loss) *loss = l;
  return rc;
}

int kprn_read_loss(kprn_handle* h, float* loss) {
  API_BEGIN(h)
  KPRN_REQUIRE(loss, KPRN_E_ARG, "loss is NULL");
  form_loss(h);
  HIP_TRY(hipMemcpyAsync(loss, h->d_loss, sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  prof_drain(h);
  API_END(h)
}

int kprn_format_score_lines(int64_t counter0, const float* probs, const float* labels, int64_t n, char* out, int64_t cap, int64_t* written) {
  if (!probs || !labels || !written || n < 0 || (cap > 0 && !out)) return KPRN_E_ARG;
  try {
    const unsigned hc = std::thread::hardware_concurrency();
    *written = hostfeed::format_scores(counter0, probs, labels, n, out, cap, hc >= 64 ? 16 : (hc >= 8 ? 4 : 1));
  } catch (...) { return KPRN_E_NOMEM; }
  return *written < 0 ? KPRN_E_ARG : KPRN_OK;
}

int kprn_read_loss_sum(kprn_handle* h, float* sum, int32_t* steps, int32_t reset) {
  API_BEGIN(h)
  KPRN_REQUIRE(sum && steps, KPRN_E_ARG, "sum / steps is NULL");
  form_loss(h);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  HIP_TRY(hipMemcpyAsync(v, h->d_loss, 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (reset) HIP_TRY(hipMemsetAsync(h->d_loss + 1, 0, 2 * sizeof(float), h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *sum = v[1]; *steps = (int32_t)v[2];
  prof_drain(h);
  API_END(h)
}

int kprn_sync(kprn_handle* h) {
  API_BEGIN(h)
  sync_compute_streams(h);
  prof_drain(h);
  API_END(h)
}

// ---- data-parallel hooks ------------------------------------------------------------------
int kprn_dense_grad_buffer(kprn_handle* h, void** dev_ptr, int64_t* n_floats) {
  API_BEGIN(h)
  KPRN_REQUIRE(dev_ptr && n_floats, KPRN_E_ARG, "NULL argument");
  KPRN_REQUIRE(h->stream_known, KPRN_E_ARG,
               "data-parallel hooks: the caller's collectives must be ordered with the engine's stream, but kprn_config.stream was NULL (the engine "
               "made its own) and kprn_stream() was never called -- pass a stream (KPRN_STREAM_LEGACY_DEFAULT for the null stream) or fetch the engine's");
  *dev_ptr = h->g_dense;
  *n_floats = h->n_dense;
  API_END(h)
}

int kprn_sparse_grad_capacity(kprn_handle* h, int32_t* max_rows) {
  API_BEGIN(h)
  KPRN_REQUIRE(max_rows, KPRN_E_ARG, "NULL argument");
  *max_rows = (int32_t)std::min<int64_t>(h->step_rows_ub, h->cfg.Ve);
  API_END(h)
}

// this step's touched entity rows (+ the dense arena behind them, dp_dense_in_pack) -> dst[words], cleared from the accumulator
static void pack_into(kprn_handle* h, int32_t capacity, int32_t* dst) {
  const int de = h->cfg.de;
  h->pack_cap = capacity;  // the capacity THIS buffer is laid out with (ids at +4, rows at +4+capacity): merge checks against it
  if (!h->view_batch) { h->rows_view = h->step_rows; h->count_view = h->step_count; }
  ProfScope ps(h, "dp_pack_rows");   // rows moved out of g_We (zeroed behind) + the dense arena behind them, one launch
  float* tail = (float*)(dst + 4 + (int64_t)capacity * (1 + de));
  kk::pack_rows(h->stream, h->g_We, h->rows_view, h->count_view, h->step_rows_ub, de, dst + 4, (float*)(dst + 4 + capacity), dst, h->g_dense,
                h->dp_dense_in_pack ? h->n_dense : 0, tail);
}

int kprn_sparse_grad_pack(kprn_handle* h, int32_t capacity, void** dev_buf, int64_t* n_words) {
  API_BEGIN(h)
  KPRN_REQUIRE(dev_buf && n_words, KPRN_E_ARG, "NULL argument");
  KPRN_REQUIRE(h->stream_known, KPRN_E_ARG,
               "data-parallel hooks: the caller's collectives must be ordered with the engine's stream, but kprn_config.stream was NULL (the engine "
               "made its own) and kprn_stream() was never called -- pass a stream (KPRN_STREAM_LEGACY_DEFAULT for the null stream) or fetch the engine's");
  KPRN_REQUIRE(capacity >= h->step_rows_ub && capacity > 0, KPRN_E_ARG, "capacity smaller than this step's touched-row count");
  materialize_union(h);   // (a gathered gradient still pending: make it what the unfused merge would have left before packing again)
  const int64_t words = 4 + (int64_t)capacity * (1 + h->cfg.de) + dp_tail_words(h);
  if (words > h->pack_words) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    dfree(h->pack_buf);
    h->pack_buf = dalloc<int32_t>(words);
    h->pack_words = words;
  }
  pack_into(h, capacity, h->pack_buf);
  *dev_buf = h->pack_buf;
  *n_words = words;
  API_END(h)
}

static void merge_impl(kprn_handle* h, const void* dev_all, int32_t world, int32_t capacity) {
  KPRN_REQUIRE(capacity == h->pack_cap, KPRN_E_ARG, "capacity differs from the packed buffer's (every rank packs with the same capacity)");
  const int64_t n = (int64_t)world * capacity;
  if (n + 4 > h->step_rows_cap) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    dfree(h->step_rows);
    h->step_rows_cap = (n + 4) * 2;
    h->step_rows = dalloc<int32_t>(h->step_rows_cap);
  }
  // the dense arena: sum of the W copies in rank order, now (the dense update and the norm read g_dense)
  if (h->dp_dense_in_pack) {
    ProfScope ps(h, "dp_dense_sum");
    const int64_t row_words = 4 + (int64_t)capacity * (1 + h->cfg.de);
    hipLaunchKernelGGL(k_dense_from_all, dim3((unsigned)std::min<int64_t>((h->n_dense + 255) / 256, 512)), dim3(256), 0, h->stream, (const float*)dev_all, (int)world,
                       row_words + dp_tail_words(h), row_words, h->n_dense, h->g_dense);
    HIP_TRY(hipGetLastError());
  }
  // the rows: recorded; the optimiser walks the gathered buffer itself (dp_fused_update: the caller keeps dev_all alive and unchanged until
  // kprn_apply_update returns) or the union is built here -- the optimiser then walks the union of all ranks' rows (sorted); exact count on the
  // device, upper bound on the host
  h->dp_all = dev_all; h->dp_world = world; h->dp_cap = capacity; h->dp_union_pending = true;
  h->view_batch = nullptr; h->rows_view = h->step_rows; h->count_view = h->step_count;
  h->step_rows_ub = std::min<int64_t>(n, h->cfg.Ve);
  h->ent_grads_dirty = true;
  if (!h->dp_fused_update) materialize_union(h);
}

int kprn_sparse_grad_merge(kprn_handle* h, const void* dev_all, int32_t world, int32_t capacity) {
  API_BEGIN(h)
  KPRN_REQUIRE(dev_all && world > 0 && capacity > 0, KPRN_E_ARG, "bad argument");
  KPRN_REQUIRE(h->stream_known, KPRN_E_ARG,
               "data-parallel hooks: the caller's collectives must be ordered with the engine's stream, but kprn_config.stream was NULL (the engine "
               "made its own) and kprn_stream() was never called -- pass a stream (KPRN_STREAM_LEGACY_DEFAULT for the null stream) or fetch the engine's");
  merge_impl(h, dev_all, world, capacity);
  API_END(h)
}

// ---- the exchange issued by the engine itself: RCCL on the engine's stream(s) ------------------------------------------------------
// The hooks above leave the collective to the caller (torch.distributed: its own stream, two cross-stream hand-overs of ~20 us each and
// ~0.3 ms of Python per step between pack and update).  Here the engine holds a communicator of its own and queues
// pack -> ncclAllGather (IN PLACE: every rank packs straight into its slot of the gathered buffer) -> dense sum -> optimiser step (the
// union of the rows inside the row kernel) back to back from one C call.  librccl is dlopen'ed (the copy the host process already
// uses -- torch ships one -- so the library has no link-time dependency on it); the communicator is bootstrapped by the caller's own
// control plane: rank 0 draws the 128-byte id (kprn_dp_unique_id), the caller broadcasts it, every rank calls kprn_dp_init.
}  // extern "C"   (the helpers below are C++: they return std::string)
namespace {
struct Id128 { char b[128]; };   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES), passed BY VALUE to ncclCommInitRank
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id128, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
std::string g_rccl_err;
bool rccl_load(const char* path) {
  if (g_rccl.lib) return true;
  const char* names[] = {path && path[0] ? path : nullptr, "librccl.so", "librccl.so.1"};
  void* lib = nullptr;
  for (const char* n : names) {
    if (!n) continue;
    lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (lib) break;
    const char* e = dlerror();
    g_rccl_err = e ? e : "dlopen failed";
  }
  if (!lib) return false;
  Rccl r;
  r.lib = lib;
  *(void**)&r.GetUniqueId = dlsym(lib, "ncclGetUniqueId");
  *(void**)&r.CommInitRank = dlsym(lib, "ncclCommInitRank");
  *(void**)&r.AllGather = dlsym(lib, "ncclAllGather");
  *(void**)&r.CommDestroy = dlsym(lib, "ncclCommDestroy");
  *(void**)&r.CommCount = dlsym(lib, "ncclCommCount");
  *(void**)&r.GetErrorString = dlsym(lib, "ncclGetErrorString");
  if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy) { g_rccl_err = "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy"; return false; }
  g_rccl = r;
  return true;
}
std::string rccl_msg(const char* what, int rc) {
  return std::string(what) + " failed: " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?") + " (" + std::to_string(rc) + ")";
}
const int kNcclInt32 = 2;   // ncclDataType_t (rccl.h)
}  // namespace
extern "C" {

static void dp_release(kprn_handle* h) {
  if (h->dp_comm && g_rccl.CommDestroy) {
    g_rccl.CommDestroy(h->dp_comm);
    h->dp_dense_in_pack = h->dp_saved_dense_in_pack;   // (kprn_dp_init forced both on)
    h->dp_fused_update = h->dp_saved_fused_update;
  }
  h->dp_comm = nullptr;
  // an exchange in flight dies with the communicator: nothing may point into the gathered buffer freed below (a later materialize_union /
  // kprn_get_grad / kprn_sparse_grad_pack would read it).  The rows a begun exchange had moved out of g_We are lost with it -- the caller
  // shut the exchange down between begin and finish.
  h->dp_begun = false; h->dp_union_pending = false; h->dp_all = nullptr; h->dp_world = 0; h->dp_cap = 0;
  if (h->dp_comm_stream) { hipStreamSynchronize(h->dp_comm_stream); hipStreamDestroy(h->dp_comm_stream); h->dp_comm_stream = nullptr; }
  if (h->ev_dp_packed) { hipEventDestroy(h->ev_dp_packed); h->ev_dp_packed = nullptr; }
  if (h->ev_dp_gathered) { hipEventDestroy(h->ev_dp_gathered); h->ev_dp_gathered = nullptr; }
  dfree(h->dp_gather); h->dp_gather_words = 0;
}

int kprn_dp_available(const char* rccl_path) {
  if (!rccl_load(rccl_path)) { g_create_error = "cannot load librccl: " + g_rccl_err; return KPRN_E_DEVICE; }
  return KPRN_OK;
}

int kprn_dp_unique_id(const char* rccl_path, void* id128) {
  if (!id128) return KPRN_E_ARG;
  if (!rccl_load(rccl_path)) { g_create_error = "kprn_dp_unique_id: cannot load librccl: " + g_rccl_err; return KPRN_E_DEVICE; }
  const int rc = g_rccl.GetUniqueId(id128);
  if (rc != 0) { g_create_error = rccl_msg("ncclGetUniqueId", rc); return KPRN_E_DEVICE; }
  return KPRN_OK;
}

int kprn_dp_init(kprn_handle* h, const char* rccl_path, const void* id128, int32_t rank, int32_t world) {
  API_BEGIN(h)
  KPRN_REQUIRE(id128 && world >= 1 && rank >= 0 && rank < world, KPRN_E_ARG, "bad id / rank / world");
  KPRN_REQUIRE(!h->dp_comm, KPRN_E_ARG, "kprn_dp_init: this handle already holds a communicator");
  KPRN_REQUIRE(rccl_load(rccl_path), KPRN_E_DEVICE, "cannot load librccl: " + g_rccl_err);
  Id128 id;
  memcpy(id.b, id128, 128);
  void* comm = nullptr;
  const int rc = g_rccl.CommInitRank(&comm, world, id, rank);   // (collective: every rank of the job is in this call)
  KPRN_REQUIRE(rc == 0 && comm, KPRN_E_DEVICE, rccl_msg("ncclCommInitRank", rc));
  h->dp_comm = comm; h->dp_rank = rank; h->dp_nranks = world;
  h->dp_saved_dense_in_pack = h->dp_dense_in_pack; h->dp_saved_fused_update = h->dp_fused_update;
  h->dp_dense_in_pack = true;    // one collective per step
  h->dp_fused_update = true;     // union of the rows inside the row update
  h->stream_known = true;        // (the collective is queued by the engine: nobody else has to know the stream)
  API_END(h)
}

int kprn_dp_comm_size(kprn_handle* h, int32_t* nranks) {
  API_BEGIN(h)
  KPRN_REQUIRE(nranks, KPRN_E_ARG, "NULL argument");
  KPRN_REQUIRE(h->dp_comm, KPRN_E_ARG, "kprn_dp_comm_size before kprn_dp_init");
  int n = h->dp_nranks;
  if (g_rccl.CommCount) {   // RCCL's own count of the communicator's ranks (a self-check for scaling runs: must equal the launcher's world size)
    const int rc = g_rccl.CommCount(h->dp_comm, &n);
    KPRN_REQUIRE(rc == 0, KPRN_E_DEVICE, rccl_msg("ncclCommCount", rc));
  }
  *nranks = n;
  API_END(h)
}

int kprn_dp_shutdown(kprn_handle* h) {
  API_BEGIN(h)
  HIP_TRY(hipStreamSynchronize(h->stream));
  dp_release(h);
  API_END(h)
}

int kprn_dp_exchange_begin(kprn_handle* h, int32_t capacity) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->dp_comm, KPRN_E_ARG, "kprn_dp_exchange_begin before kprn_dp_init");
  KPRN_REQUIRE(capacity >= h->step_rows_ub && capacity > 0, KPRN_E_ARG, "capacity smaller than this step's touched-row count");
  KPRN_REQUIRE((capacity & 3) == 0, KPRN_E_ARG, "capacity must be a multiple of 4 rows (every rank's slot of the gathered buffer stays 16-byte aligned)");
  materialize_union(h);
  const int W = h->dp_nranks;
  const int64_t words = 4 + (int64_t)capacity * (1 + h->cfg.de) + dp_tail_words(h);
  if (words * W > h->dp_gather_words) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->dp_comm_stream) HIP_TRY(hipStreamSynchronize(h->dp_comm_stream));
    dfree(h->dp_gather);
    h->dp_gather = dalloc<int32_t>(words * W);
    h->dp_gather_words = words * W;
  }
  int32_t* mine = h->dp_gather + (int64_t)h->dp_rank * words;
  pack_into(h, capacity, mine);
  hipStream_t cs = h->stream;
  if (h->dp_comm_stream_on) {   // (also at world 1, where the collective is empty: the hand-over is the same code a world-8 run takes)
    if (!h->dp_comm_stream) {
      h->dp_comm_stream = make_concurrent_stream(h);
      HIP_TRY(hipEventCreateWithFlags(&h->ev_dp_packed, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_dp_gathered, hipEventDisableTiming));
    }
    cs = h->dp_comm_stream;
    HIP_TRY(hipEventRecord(h->ev_dp_packed, h->stream));
    HIP_TRY(hipStreamWaitEvent(cs, h->ev_dp_packed, 0));
  }
  {
    ProfScope ps(h, "dp_allgather");
    // in place: sendbuff = recvbuff + rank * count (no staging copy; with one rank RCCL returns at once)
    const int rc = g_rccl.AllGather(mine, h->dp_gather, (size_t)words, kNcclInt32, h->dp_comm, cs);
    KPRN_REQUIRE(rc == 0, KPRN_E_DEVICE, rccl_msg("ncclAllGather", rc));
  }
  if (cs != h->stream) HIP_TRY(hipEventRecord(h->ev_dp_gathered, cs));
  h->dp_begun = true;
  API_END(h)
}

int kprn_dp_exchange_finish(kprn_handle* h, const kprn_opt* opt) {
  API_BEGIN(h)
  KPRN_REQUIRE(h->dp_comm && h->dp_begun, KPRN_E_ARG, "kprn_dp_exchange_finish without kprn_dp_exchange_begin");
  h->dp_begun = false;
  if (h->dp_comm_stream_on && h->dp_comm_stream) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_dp_gathered, 0));
  merge_impl(h, h->dp_gather, h->dp_nranks, (int32_t)h->pack_cap);
  optim::apply_update(h, opt);
  API_END(h)
}

/* the stream everything is queued on */
int kprn_stream(kprn_handle* h, void** stream) {
  API_BEGIN(h)
  KPRN_REQUIRE(stream, KPRN_E_ARG, "NULL argument");
  *stream = (void*)h->stream;
  h->stream_known = true;
  API_END(h)
}

// ---- checkpoints ------------------------------------------------------------------------
static const char kMagic[8] = {'K', 'P', 'R', 'N', 'A', 'M', 'D', '1'};

int kprn_save(kprn_handle* h, const char* path) {
  API_BEGIN(h)
  KPRN_REQUIRE(path, KPRN_E_ARG, "path is NULL");
  std::vector<float> flat((size_t)h->n_params);
  {
    int rc = kprn_get_flat_params(h, flat.data(), h->n_params);
    if (rc != KPRN_OK) return rc;
  }
  FILE* f = fopen(path, "wb");
  KPRN_REQUIRE(f, KPRN_E_IO, std::string("cannot open for writing: ") + path);
  const kprn_config& c = h->cfg;
  int32_t hdr[16] = {c.Vt, c.Ve, c.Vr, c.dt, c.de, c.dr, c.F, c.num_types, c.H, c.L, c.C, c.rnn_type, c.reducer, c.K, 0, 0};
  // word 14: the pooling temperature's float bits, 0 at gamma = 1 (the files written before option "pool_gamma" existed, byte for byte)
  if (h->pool_gamma != 1.0f) memcpy(&hdr[14], &h->pool_gamma, sizeof(float));
  bool ok = fwrite(kMagic, 1, 8, f) == 8 && fwrite(hdr, sizeof(int32_t), 16, f) == 16 && fwrite(&h->n_params, sizeof(int64_t), 1, f) == 1 &&
            fwrite(flat.data(), sizeof(float), flat.size(), f) == flat.size();
  ok = (fclose(f) == 0) && ok;
  KPRN_REQUIRE(ok, KPRN_E_IO, "short write");
  API_END(h)
}

int kprn_load(kprn_handle* h, const char* path) {
  API_BEGIN(h)
  KPRN_REQUIRE(path, KPRN_E_ARG, "path is NULL");
  FILE* f = fopen(path, "rb");
  KPRN_REQUIRE(f, KPRN_E_IO, std::string("cannot open: ") + path);
  char magic[8];
  int32_t hdr[16];
  int64_t n = 0;
  bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, kMagic, 8) == 0 && fread(hdr, sizeof(int32_t), 16, f) == 16 &&
            fread(&n, sizeof(int64_t), 1, f) == 1;
  const kprn_config& c = h->cfg;
  const int32_t want[12] = {c.Vt, c.Ve, c.Vr, c.dt, c.de, c.dr, c.F, c.num_types, c.H, c.L, c.C, c.rnn_type};
  if (ok) ok = memcmp(hdr, want, sizeof(want)) == 0 && n == h->n_params;
  std::vector<float> flat;
  if (ok) { flat.resize((size_t)n); ok = fread(flat.data(), sizeof(float), flat.size(), f) == flat.size(); }
  fclose(f);
  KPRN_REQUIRE(ok, KPRN_E_IO, "not a kprn checkpoint for this configuration");
  // a non-zero word 14 is the pooling temperature the file was saved under: a LogSumExp handle adopts it (a zero word leaves the option alone)
  float gamma = 0.f;
  memcpy(&gamma, &hdr[14], sizeof(float));
  const bool adopt = hdr[14] != 0 && c.reducer == 2;
  KPRN_REQUIRE(!adopt || kk::pool_gamma_ok((double)gamma), KPRN_E_IO, "checkpoint header word 14 is not a pooling temperature in [1e-3, 1e3]");
  const int rc = kprn_set_flat_params(h, flat.data(), n);
  if (rc == KPRN_OK && adopt) { h->pool_gamma = gamma; h->pool_ig = kk::pool_ig_of(gamma); }
  return rc;
  API_END(h)
}

// ---- measurement ------------------------------------------------------------------------
int kprn_profile_enable(kprn_handle* h, int32_t on) {
  API_BEGIN(h)
  prof_drain(h);
  h->prof_on = on != 0;
  API_END(h)
}
int kprn_profile_reset(kprn_handle* h) {
  API_BEGIN(h)
  prof_drain(h);
  h->prof.clear();
  API_END(h)
}
int kprn_profile_get(kprn_handle* h, kprn_prof_entry* out, int32_t cap, int32_t* n) {
  API_BEGIN(h)
  KPRN_REQUIRE(n, KPRN_E_ARG, "n is NULL");
  prof_drain(h);
  int k = 0;
  for (auto& kv : h->prof) {
    if (out && k < cap) {
      memset(&out[k], 0, sizeof(kprn_prof_entry));
      strncpy(out[k].name, kv.first.c_str(), sizeof(out[k].name) - 1);
      out[k].total_ms = kv.second.total_ms;
      out[k].launches = kv.second.launches;
    }
    ++k;
  }
  *n = k;
  API_END(h)
}

/* measurement hook (scripts/gpu_gemm_bench.py): times one GEMM shape of the generic pipeline on random data.
 * what: 0 = C = A B^T (forward i2g), 1 = C = A B (dx / dh), 2 = C += A^T B with split-K (dW), 3 = FastLSTM step kernel (M paths, N = H, K = Din),
 *       4 = Recurrence step kernel.  Returns the mean milliseconds per launch in *ms. */
int kprn_debug_gemm(kprn_handle* h, int32_t what, int64_t M, int32_t N, int64_t K, int32_t iters, float* ms) {
  API_BEGIN(h)
  KPRN_REQUIRE(ms && M > 0 && N > 0 && K > 0 && iters > 0, KPRN_E_ARG, "bad argument");
  hipStream_t s = h->stream;
  if (what == 5 || what == 6) {   // the bf16 pipeline's product (gemm_bf16.hip) under h's "bf16_gemm_*" options: 5 = C = A B^T, 6 = split-K accumulate
    *ms = bf16p::debug_gemm16(h, M, N, K, what == 6 ? 1024 : 1, iters);
    return KPRN_OK;
  }
  float *A = nullptr, *B = nullptr, *C = nullptr, *X = nullptr, *Z = nullptr;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
  try {
    const int64_t H = N, Din = K;
    if (what <= 2) {
      const int64_t na = M * K, nb = (int64_t)N * K, nc = (what == 2) ? (int64_t)N * K : M * (int64_t)N;
      A = dalloc<float>(what == 2 ? M * (int64_t)N : na); B = dalloc<float>(what == 2 ? M * K : nb); C = dalloc<float>(nc);
      kk::fill_uniform(s, A, what == 2 ? M * (int64_t)N : na, 0.1f, 1, 0); kk::fill_uniform(s, B, what == 2 ? M * K : nb, 0.1f, 2, 0);
      HIP_TRY(hipMemsetAsync(C, 0, (size_t)nc * sizeof(float), s));
    } else {
      X = dalloc<float>(M * Din); A = dalloc<float>(2 * M * H); B = dalloc<float>(4 * H * (Din + H) + 8 * H); C = dalloc<float>(2 * M * H); Z = dalloc<float>(M * 4 * H);
      kk::fill_uniform(s, X, M * Din, 0.1f, 1, 0); kk::fill_uniform(s, A, 2 * M * H, 0.1f, 2, 0); kk::fill_uniform(s, B, 4 * H * (Din + H) + 8 * H, 0.1f, 3, 0);
    }
    for (int it = -2; it < iters; ++it) {
      if (it == 0) HIP_TRY(hipEventRecord(e0, s));
      if (what == 0) gemm::run(s, A, K, 1, B, 1, K, C, N, M, N, K, false, nullptr, 1);
      else if (what == 1) gemm::run(s, A, K, 1, B, N, 1, C, N, M, N, K, false, nullptr, 1);            // B [K][N] n-contiguous
      else if (what == 2) gemm::run(s, A, 1, N, B, K, 1, C, K, N, (int)K, M, true, nullptr, 1024);     // C[N][K] += A[M][N]^T B[M][K]
      else if (what == 3) gemm::lstm_step(s, X, Din, (int)Din, B, B + 4 * H * (Din + H), A, B + 4 * H * Din, A + M * H, C, C + M * H, H, Z, M, (int)H);
      else gemm::rnn_step(s, X, Din, (int)Din, B, B + 4 * H * (Din + H), A, B + H * Din, B + 4 * H * (Din + H) + H, A + M * H, Z, C, H, M, (int)H, 1);
    }
    HIP_TRY(hipEventRecord(e1, s));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    *ms = t / (float)iters;
  } catch (...) { dfree(A); dfree(B); dfree(C); dfree(X); dfree(Z); hipEventDestroy(e0); hipEventDestroy(e1); throw; }
  dfree(A); dfree(B); dfree(C); dfree(X); dfree(Z); hipEventDestroy(e0); hipEventDestroy(e1);
  API_END(h)
}

/* test hook (tests/test_gpu_gemm16_products.py): one launch of one bf16 product on the caller's data (gemm_bf16.hip debug_gemm16_run) */
int kprn_debug_gemm16_run(kprn_handle* h, const kprn_gemm16_call* call, const float* A, const float* B, const float* bias, float* C, kprn_gemm16_ran* ran) {
  API_BEGIN(h)
  KPRN_REQUIRE(call, KPRN_E_ARG, "gemm16_run: NULL argument");
  bf16p::debug_gemm16_run(h, *call, A, B, bias, C, ran);
  API_END(h)
}

int kprn_set_option(kprn_handle* h, const char* key, const char* value) {
  API_BEGIN(h)
  KPRN_REQUIRE(key && value, KPRN_E_ARG, "NULL argument");
  if (strcmp(key, "impl") == 0) {
    if (strcmp(value, "auto") == 0) h->impl = 0;
    else if (strcmp(value, "generic") == 0) h->impl = 1;
    else throw KprnError{KPRN_E_ARG, "impl must be auto or generic"};
  } else if (strcmp(key, "prefix_plan") == 0) {
    h->prefix_plan = atoi(value) ? 1 : 0;  // batches created from now on (an existing batch keeps what it was built with)
  } else if (strcmp(key, "small_tiles") == 0) {
    // batches created / fed from now on: <= 8 192 paths on tiles of one 16-row m-tile and no identical-prefix plan ("1", default), or the
    // 64-path tiles at every size ("0").  (A split scoring pass whose second part is still unplaced is finished first: the rest launch decides
    // its tiling from this option.)
    join_score(h);
    h->small_tiles_on = atoi(value) != 0;
  } else if (strcmp(key, "tile_handover") == 0) {
    // fused D = H = 64 backward launches: a tile may change workgroups once between two of its steps -- "2" (default): workgroup b paired with b + G / 2,
    // "1": with G - 1 - b -- or workgroups run whole tiles only ("0")
    const int v = atoi(value);
    KPRN_REQUIRE(v >= 0 && v <= 2, KPRN_E_ARG, "tile_handover must be 0, 1 or 2");
    h->tile_handover = v;
  } else if (strcmp(key, "rank_sort_min") == 0) {
    // ranking stage: groups of this many members and more are ranked by an LDS sort, smaller ones by counting (rank_groups.hip; same results).  257 = every
    // group the workgroup kernel takes is sorted, 4097 = none is: the two sides of the measurement in profiles/rank/README.md
    const int v = atoi(value);
    KPRN_REQUIRE(v >= 257 && v <= 4097, KPRN_E_ARG, "rank_sort_min must be in 257..4097");
    h->rank_sort_min = v;
  } else if (strcmp(key, "adam_merged") == 0) {
    // lazy-exact Adam: the entity rows' update and the dense arena's update in ONE launch ("1", default) or in two ("0": the A/B reference; bit-identical)
    h->adam_merged = atoi(value) != 0;
  } else if (strcmp(key, "bwd_pipe") == 0) {
    // fused path, small batches (16-row tiles), two layers: both layers' BPTT as ONE launch with the bottom layer one step behind the top layer ("1", default)
    // or as two launches ("0": the A/B reference)
    h->bwd_pipe = atoi(value) != 0;
  } else if (strcmp(key, "score_dual") == 0) {
    // with "score_overlap": a scoring pass queued by kprn_forward_batch_async is held back and runs in the launch of the training forward that follows
    // (one kernel, two branches: no second stream, no fork / join events) -- "1": always, "2" (default): for batches below the 16-row-tile threshold
    // (8 192 paths: measured break-even; above it the side stream's pass lets the loss stage and the backward start under its tail), "0": never
    const int v = atoi(value);
    KPRN_REQUIRE(v >= 0 && v <= 2, KPRN_E_ARG, "score_dual must be 0, 1 or 2");
    h->score_dual = v;
  } else if (strcmp(key, "catchup_prefix") == 0) {
    // fused D = H = 64 path: a batch's lazy-exact row catch-up and its identical-prefix table in one launch ("1", default) or in two ("0": the A/B reference;
    // bit-identical)
    h->catchup_prefix = atoi(value) != 0;
  } else if (strcmp(key, "fused_small_tables") == 0) {
    // fused D = H = 64 path: the type / relation table gradients are formed inside the bottom layer's BPTT launch (one-hot MFMAs on the dx registers) ("1", default) or by a
    // passenger job of the entity-gradient launch that re-reads dx ("0": the A/B reference)
    h->fused_small_tables = atoi(value) != 0;
  } else if (strcmp(key, "persist_layers") == 0) {
    // generic fp32 pipelines: a recurrent layer as ONE persistent launch ("1", default: where layer_f32_persist.hip takes the shape and the batch gives
    // every CU a tile; "2": at any batch size -- tests) or one launch per step ("0")
    const int v = atoi(value);
    KPRN_REQUIRE(v >= 0 && v <= 2, KPRN_E_ARG, "persist_layers must be 0, 1 or 2");
    h->persist_layers = v;
  } else if (strcmp(key, "persist_layers_grid") == 0) {
    // those launches' workgroup count: min(tiles, CUs) ("0", default) or at most this many ("n" > 0: a workgroup then runs several tiles at batch sizes a
    // float64 reference handles -- tests).  Per handle, read at every launch.
    char* end = nullptr;
    const long v = strtol(value, &end, 10);
    KPRN_REQUIRE(end != value && *end == 0 && v >= 0 && v <= 0x7fffffff, KPRN_E_ARG, "persist_layers_grid must be 0 (one workgroup per CU at most) or a positive workgroup count");
    h->persist_layers_grid = (int)v;
  } else if (strcmp(key, "small_tables") == 0) {
    // generic fp32 pipelines: layer 0's type / relation gradients from G = dA^T [S_r | S_t] ("1", default) or from the full dx product + the
    // table-gradient launch ("0": the A/B reference)
    h->small_tables = atoi(value) != 0;
  } else if (strcmp(key, "small_tables_fwd") == 0) {
    // fused D = H = 64 forward (fp32, two layers, one type slot, dt = dr = 16, de = 32, Vt + Vr <= 16): layer 0's input half through the small-table identity,
    // K = 48 instead of 64 ("1", default) or over the full x row ("0": the A/B reference).  A key of its own: "small_tables" must leave the forward bit-identical.
    join_score(h);   // (a pass already queued keeps the route it was queued under)
    h->small_tables_fwd = atoi(value) != 0;
  } else if (strcmp(key, "head_select") == 0) {
    // fused D = H = 64 fp32 forward: the head forms the selected class's column alone wherever no reader of the pass needs another ("1", default), or all C
    // columns always ("0": the A/B reference).  The selected column is bit-identical either way.
    join_score(h);   // (a pass already queued keeps the head it was queued under)
    h->head_select = atoi(value) != 0;
  } else if (strcmp(key, "bf16_t_pad") == 0) {
    // small-table route: pad (elements, a multiple of 8, 0 .. 512) of the row pitch of dA^T / Z^T ("0": rows 2^18-aligned at the bench's size)
    const int n = atoi(value);
    h->bf16_t_pad = n < 0 ? 0 : (n > 512 ? 512 : (n & ~7));
  } else if (strcmp(key, "bf16_gemm_regstage") == 0) {
    // bf16 split-K products on gx::k_gemm16r ("1": opt-in, operands global -> registers -> LDS, four chunks in flight per thread) or gx::k_gemm16x ("0", default: LDS-DMA, two)
    h->bf16_gemm.regstage = atoi(value) != 0;
  } else if (strcmp(key, "bf16_gemm_touch") == 0) {
    // bf16 products on gx::k_gemm16x: every wave touches (one dword per tile row = one cache line) the chunk this many chunks (0 .. 32) ahead of its DMA: an L2
    // prefetch for a launch that is bound by its operand staging ("0": off)
    const int n = atoi(value);
    h->bf16_gemm.touch = n < 0 ? 0 : (n > 32 ? 32 : n);
  } else if (strcmp(key, "bf16_gemm_pingpong") == 0) {
    // bf16 pipeline: split-K products with >= 256 x 256 outputs on the two-group kernel gx::k_gemm16p ("1": opt-in, measured slower) or on gx::k_gemm16x ("0", default)
    h->bf16_gemm.pingpong = atoi(value) != 0;
  } else if (strcmp(key, "bf16_bptt_dxe") == 0) {
    // bf16 pipeline with "bf16_small_tables": the entity slice of dx is formed INSIDE the persistent BPTT launch (a fourth result tile per wave; value =
    // depth of its weight ring, 8 (default) or 16) or by its own product launch reading dA^T once more ("0")
    const int v = atoi(value);
    KPRN_REQUIRE(v == 0 || v == 8 || v == 16, KPRN_E_ARG, "bf16_bptt_dxe must be 0, 8 or 16");
    h->bf16_bptt_dxe = v;
  } else if (strcmp(key, "bf16_small_tables") == 0) {
    // bf16 pipeline, persistent BPTT: gradients of the type / relation tables (<= 128 rows together) and of their column blocks of W_i2g from one
    // extra column block of the merged dW product ("1", default) or from the full dx product + the table-gradient launch ("0": the A/B reference)
    h->bf16_small_tables = atoi(value) != 0;
  } else if (strcmp(key, "score_rest_before_bptt") == 0) {
    join_score(h);
    h->score_rest_before_bptt = atoi(value) ? 1 : 0;
  } else if (strcmp(key, "score_rest_in_backward") == 0) {
    join_score(h);
    h->score_rest_in_backward = atoi(value) ? 1 : 0;
    h->after_bptt_hook = h->score_rest_in_backward ? score::rest_hook : nullptr;
  } else if (strcmp(key, "score_split") == 0) {
    // kprn_forward_batch_async queues only the first (1 - f) of the batch's tiles; kprn_forward_batch_async_rest the others + the pooling
    join_score(h);
    const double f = atof(value);
    KPRN_REQUIRE(f >= 0.0 && f < 1.0, KPRN_E_ARG, "score_split: a fraction in [0, 1)");
    h->score_split = (float)f;
  } else if (strcmp(key, "score_overlap") == 0) {
    // kprn_forward_batch_async on a second stream (fused path): the scoring pass shares the chip with the work enqueued after it
    join_score(h);
    h->score_overlap = atoi(value) ? 1 : 0;
  } else if (strcmp(key, "loss_accumulate") == 0) {
    h->loss_accumulate = atoi(value) ? 1 : 0;
  } else if (strcmp(key, "inline_upload") == 0) {
    if (strcmp(value, "side") == 0) h->inline_upload_side = 1;
    else if (strcmp(value, "main") == 0) h->inline_upload_side = 0;
    else throw KprnError{KPRN_E_ARG, "inline_upload must be side or main"};
  } else if (strcmp(key, "train_step_return") == 0) {
    if (strcmp(value, "loss") == 0) h->train_step_drain = 0;
    else if (strcmp(value, "drain") == 0) h->train_step_drain = 1;
    else throw KprnError{KPRN_E_ARG, "train_step_return must be loss or drain"};
  } else if (strcmp(key, "feed_build") == 0) {
    if (strcmp(value, "host") == 0) h->feed_build_host = 1;
    else if (strcmp(value, "device") == 0) h->feed_build_host = 0;
    else throw KprnError{KPRN_E_ARG, "feed_build must be host or device"};
  } else if (strcmp(key, "feed_threads") == 0) {
    const int v = atoi(value);
    KPRN_REQUIRE(v >= 1 && v <= 64, KPRN_E_ARG, "feed_threads must be in 1..64");
    h->feed_threads = v;
  } else if (strcmp(key, "feed_workers") == 0) {
    const int v = atoi(value);
    KPRN_REQUIRE(v >= 1 && v <= 64 && !h->feed_pool, KPRN_E_ARG, "feed_workers must be in 1..64 and set before the first feed");
    h->feed_workers = v;
  } else if (strcmp(key, "profile_filter") == 0) {
    h->prof_filter = value;  // "" = every kernel family; else only families whose name starts with this
  } else if (strcmp(key, "dp_comm_stream") == 0) {
    // kprn_dp_exchange_begin queues the all-gather on a stream of its own (1) or on the main stream (0, default): with 1, work queued on the
    // main stream between _begin and _finish (a scoring pass on the side stream forks from there) runs while the collective is in flight
    h->dp_comm_stream_on = atoi(value) != 0;
  } else if (strcmp(key, "dp_fused_update") == 0) {
    h->dp_fused_update = atoi(value) != 0;
  } else if (strcmp(key, "dp_dense_in_pack") == 0) {
    // data-parallel exchange: the dense gradient arena travels behind the packed entity rows (one all-gather, no all-reduce); the merge sums
    // the ranks' copies in rank order
    h->dp_dense_in_pack = atoi(value) != 0;
  } else if (strcmp(key, "deterministic") == 0) {
    // "1": every float a training step hands back (loss, gradients, parameters, optimiser state) is a function of the inputs only -- the fused fp32 path's
    // atomic joins are replaced by plain-stored partials summed in a fixed order; a training call that would take any other pipeline returns
    // KPRN_E_UNSUPPORTED.  "0" (default): the kernels launched before this option existed.  Read at every training call.
    // "2": the same, and the generic fp32 pipeline (FastLSTM and rnn cells, compute_dtype 0) trains too, its atomic joins -- split-K products, column sums, head,
    // entity and table gradients -- replaced by slabs joined in index order; wherever "1" trains, "2" launches exactly what "1" launches.
    KPRN_REQUIRE(strcmp(value, "0") == 0 || strcmp(value, "1") == 0 || strcmp(value, "2") == 0, KPRN_E_ARG, "deterministic must be 0, 1 or 2");
    h->deterministic = value[0] - '0';
  } else if (strcmp(key, "loss") == 0) {
    // what kprn_backward_batch / kprn_train_step_batch train on: nn.BCECriterion per pair ("bce", default) or the pairwise loss over the batch's group table
    // ("bpr"; include/kprn.h "pairwise loss").  Read at every training call; scoring, ranking, explaining and recommending never look at it.
    if (strcmp(value, "bce") == 0) h->loss_bpr = 0;
    else if (strcmp(value, "bpr") == 0) h->loss_bpr = 1;
    else throw KprnError{KPRN_E_ARG, "loss must be bce or bpr"};
  } else if (strcmp(key, "path_cap") == 0) {
    // which of a pair's paths a find call keeps when more exist than max_paths (include/kprn.h "finding a pair's paths", cap): the first ones in the pair's
    // order ("first", default: the kernels' results before this option existed, bit for bit) or one drawn in each of max_paths strata of that order ("spread").
    // Read by every find call that has a seed and a draw; kprn_find_paths has none and always keeps the first.
    if (strcmp(value, "first") == 0) h->path_cap = 0;
    else if (strcmp(value, "spread") == 0) h->path_cap = 1;
    else throw KprnError{KPRN_E_ARG, "path_cap must be first or spread"};
  } else if (strcmp(key, "dropout") == 0) {
    // rate p of nn.Dropout on every rnn layer's step input in training forwards (OneModel.lua:246-265); "0" (default): the kernels launched
    // before this option existed.  Refused HERE where the reference ignores the flag (lstm, gru) or the pipeline has no dropped form (bf16 products).
    char* end = nullptr;
    // (strtod alone would take leading white space and hex floats: digits, '.', an exponent and its sign only, a digit or '.' first)
    const bool decimal = (isdigit((unsigned char)value[0]) || value[0] == '.') && value[strspn(value, "0123456789.eE+-")] == 0;
    const double p = decimal ? strtod(value, &end) : 0.0;
    KPRN_REQUIRE(decimal && end != value && *end == 0 && p >= 0.0 && p < 1.0 && (double)(float)p < 1.0, KPRN_E_ARG, "dropout must be a decimal rate in [0, 1)");
    if (p > 0.0) {
      KPRN_REQUIRE(h->cfg.rnn_type == 1, KPRN_E_UNSUPPORTED,
                   "dropout > 0: built for rnn_type 1 (rnn) only -- the reference's lstm / gru modules ignore -useDropout (OneModel.lua:237-239), so there is nothing to reproduce");
      KPRN_REQUIRE(h->cfg.compute_dtype == 0, KPRN_E_UNSUPPORTED, "dropout > 0: built for compute_dtype 0 (fp32) only; the bf16-product pipeline has no dropped form");
    }
    h->dropout_p = (float)p;
  } else if (strcmp(key, "pool_gamma") == 0) {
    // temperature of the LogSumExp reducer, the paper's log sum exp(s / gamma) (include/kprn.h "pooling temperature"); "1" (default): the bits
    // the kernels produced before this option existed.  Read at every scoring, explaining and training call.  The decimal syntax of "dropout".
    char* end = nullptr;
    const bool decimal = (isdigit((unsigned char)value[0]) || value[0] == '.') && value[strspn(value, "0123456789.eE+-")] == 0;
    const double g = decimal ? strtod(value, &end) : 0.0;
    KPRN_REQUIRE(decimal && end != value && *end == 0 && kk::pool_gamma_ok(g) && kk::pool_gamma_ok((double)(float)g), KPRN_E_ARG,
                 "pool_gamma must be a decimal temperature in [1e-3, 1e3]");
    KPRN_REQUIRE((float)g == 1.0f || h->cfg.reducer == 2, KPRN_E_UNSUPPORTED,
                 "pool_gamma != 1: the handle's reducer is not 2 (LogSumExp) -- Max and TopK + Mean have no temperature");
    h->pool_gamma = (float)g;
    h->pool_ig = kk::pool_ig_of(h->pool_gamma);
  } else if (strcmp(key, "dropout_seed") == 0) {
    // seed of the mask generator (decimal or 0x hex uint64; default cfg.seed + cfg.rank); setting it restarts the draw count
    char* end = nullptr;
    errno = 0;
    // (a digit first: no white space, no sign; base 10 unless "0x" leads, so a leading 0 is not octal)
    const bool hex = value[0] == '0' && (value[1] == 'x' || value[1] == 'X');
    const unsigned long long v = isdigit((unsigned char)value[0]) ? strtoull(value, &end, hex ? 16 : 10) : 0;
    KPRN_REQUIRE(end != nullptr && end != value && !(hex && end == value + 2) && *end == 0 && errno == 0, KPRN_E_ARG, "dropout_seed must be a decimal or 0x hex unsigned 64-bit number");
    h->dropout_seed = (uint64_t)v;
    h->drop_draw = 0;
  } else if (strcmp(key, "reserve_cus") == 0) {
    // the fused SCORING forward is a persistent one-workgroup-per-CU kernel that fills the register file of every CU it runs
    // on; leaving a few CUs free lets the copy kernels of a concurrently running collective (RCCL) make progress beside it
    const int v = atoi(value);
    KPRN_REQUIRE(v >= 0 && v <= 1024, KPRN_E_ARG, "reserve_cus must be in 0..1024");   // (the pass keeps at least one workgroup: lstm_fused_fwd.hip fwd_args)
    h->reserve_cus = v;
  } else {
    throw KprnError{KPRN_E_ARG, std::string("unknown option: ") + key};
  }
  API_END(h)
}

}  // extern "C"
