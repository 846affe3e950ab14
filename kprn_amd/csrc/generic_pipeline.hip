// Host side of the generic fp32 pipeline: every shape the fused D = H = 64 path (lstm_fused_*.hip) and the bf16 pipeline (lstm_bf16.hip) do not take -- the rnn
// cell, wide FastLSTM, GRU, impl = generic.  gather -> per layer {input GEMM, per step recurrent GEMM + cell} -> head, and back.  One walk over the layers per
// direction: a Cell says what the three cells share in numbers, layer_ops forms a layer's operands, and each tier (one persistent launch per layer,
// layer_f32_persist.hip; one launch per step, gemm_tiled.hip; GEMM + element-wise kernels) is chosen in one place.  Where a cell truly differs the walk branches on
// the cell id at that point.
#include <algorithm>

#include "kprn_internal.h"

namespace generic {
namespace {

struct Cell {
  int id;          // lp32's cell id = cfg.rnn_type: 0 FastLSTM, 1 rnn, 2 gru
  int wi_rows;     // rows of W_i2g: 4H, H, 3H (gru: i2g.weight [2H][Din] and c_i2h.weight [H][Din] are ONE operand of the record's first 3H columns)
  int rec;         // floats of a step record in ACT and dA: 4H gate values i,g,f,o; H pre-activations; 4H = [r | z | n | r*h']
  int g_rows;      // rows of the i2g / o2g arrays (G H): 4H, H, 2H
  int relu;        // rnn: the activation
  const char *layer_fwd, *step_fwd, *cell_fwd, *layer_bwd, *cell_bwd;   // profile families of the tiers
};
Cell cell_of(const kprn_handle* h) {
  const int H = h->cfg.H;
  switch (h->cfg.rnn_type) {
    case 1: return {1, H, H, H, h->cfg.use_relu == 1 ? 1 : 0, "rnn_layer_fwd", "rnn_step_fwd", "rnn_cell_fwd", "rnn_layer_bwd", "rnn_cell_bwd"};
    case 2: return {2, 3 * H, 4 * H, 2 * H, 0, "gru_layer_fwd", nullptr, "gru_cell_fwd", "gru_layer_bwd", "gru_cell_bwd"};
    default: return {0, 4 * H, 4 * H, 4 * H, 0, "lstm_layer_fwd", "lstm_step_fwd", "lstm_gates_fwd", "lstm_layer_bwd", "lstm_gates_bwd"};
  }
}

// operands of layer l; what a cell does not have is null (cs: FastLSTM only; mask, bo: rnn only; Wc / bc / Uc: gru only)
struct Layer {
  int Din; bool has_up;
  const float* in;                       // [T][N][Din] the layer's step inputs: X, or the plane below (dropped: the copy the training forward read, HsD)
  float *act, *hs, *cs, *mask;
  const float *Wi, *bi, *Wo, *bo, *Wc, *bc, *Uc;
  float *gWi, *gbi, *gWo, *gb2, *gWc, *gUc;   // gb2: the second bias that sees dA's column sums (rnn h2h.bias, gru c_i2h.bias)
};
Layer layer_ops(kprn_handle* h, const Cell& c, int l, int T, int64_t N, bool dropped) {
  Workspace& w = h->ws;
  const LayerOff& o = h->layer[l];
  const int64_t TNH = (int64_t)T * N * h->cfg.H;
  float* const gd = h->g_dense;
  Layer y;
  y.Din = o.Din; y.has_up = l < h->cfg.L - 1;
  y.in = (l == 0) ? w.X : (dropped ? w.HsD : w.Hs) + (l - 1) * TNH;
  y.act = w.ACT + (int64_t)l * T * N * c.rec; y.hs = w.Hs + l * TNH;
  y.cs = c.id == 0 ? w.Cs + l * TNH : nullptr;
  y.mask = c.id == 1 ? w.mask + (int64_t)l * T * N : nullptr;
  y.Wi = h->dense + o.Wi; y.bi = h->dense + o.bi; y.Wo = h->dense + o.Wo; y.bo = c.id == 1 ? h->dense + o.bo : nullptr;
  y.gWi = gd + o.Wi; y.gbi = gd + o.bi; y.gWo = gd + o.Wo; y.gb2 = c.id == 1 ? gd + o.bo : (c.id == 2 ? gd + o.bc : nullptr);
  const bool gru = c.id == 2;
  y.Wc = gru ? h->dense + o.Wc : nullptr; y.bc = gru ? h->dense + o.bc : nullptr; y.Uc = gru ? h->dense + o.Uc : nullptr;
  y.gWc = gru ? gd + o.Wc : nullptr; y.gUc = gru ? gd + o.Uc : nullptr;
  return y;
}

// Option "dropout": what a launch needs to regenerate layer l's masks of the training forward in flight (philox_dev.h)
philox::DropArgs drop_args(const kprn_handle* h, int l) {
  philox::DropArgs a;
  a.k0 = (uint32_t)(h->dropout_seed & 0xffffffffu); a.k1 = (uint32_t)(h->dropout_seed >> 32);
  a.draw = h->drop_draw_cur; a.layer16 = 65536u * (uint32_t)l;
  a.thr = philox::threshold((double)h->dropout_p); a.scale = philox::keep_scale(h->dropout_p);
  return a;
}

// the entity gradient from row-major dx over the occurrence index; option "deterministic" = "2": the partial sums of runs that straddle 64-position segments
// leave with plain stores and the launch behind adds them in segment order, as "1" does for the fused path's compact slice
void entity_grad_rowmajor(kprn_handle* h, const kprn_batch* b, const float* dx, int D, int dt) {
  const kprn_config& c = h->cfg;
  if (h->deterministic != 2) {
    bidx::entity_grad(h->stream, dx, /*frag_order=*/0, b->key_sorted, b->pos_sorted, b->n_index, b->N, b->T, D, dt, c.de, c.Ve, h->g_We);
    return;
  }
  dev_grow(h->stream, h->det_seg, h->det_seg_cap, (b->n_index + 63) / 64 * 2 * c.de);
  const bidx::DetEntity de_{h->det_seg, nullptr};
  bidx::entity_grad(h->stream, dx, /*frag_order=*/0, b->key_sorted, b->pos_sorted, b->n_index, b->N, b->T, D, dt, c.de, c.Ve, h->g_We, nullptr, nullptr, &de_);
  bidx::entity_grad_tail(h->stream, b->key_sorted, b->n_index, c.de, c.Ve, h->g_We, de_, nullptr);
}

// Layer 0 of the FastLSTM / rnn backward through the small-table identity (kprn_internal.h kk::onehot_cols): dx for the entity slice only, ONE dW product over
// [S | x_e] (the one-hot selectors are written over the last ns type columns of the saved step input, next to the entity columns), the type / relation blocks
// of gW_i2g and both table gradients from G.  GH = rows of W_i2g.
void backward_layer0_small_tables(kprn_handle* h, const kprn_batch* b, int ns, int GH, int split, bool bf) {
  const kprn_config& c = h->cfg;
  Workspace& w = h->ws;
  const int D = h->D;
  const int64_t N = b->N, TN = (int64_t)b->T * N;
  hipStream_t s = h->stream;
  float* gd = h->g_dense;
  const float* Wi = h->dense + h->layer[0].Wi;
  const int NZ = ns + c.de;
  dev_grow(s, h->st_ctmp, h->st_ctmp_cap, (int64_t)GH * NZ);
  {
    ProfScope ps(h, "gemm_bwd_dw_merged");   // Ct [GH][ns + de] = dA^T [S | x_e]
    kk::onehot_cols(s, b->idx, N, b->T, b->F, c.Vr, c.Vt, w.X, D, c.dt - ns, ns);
    HIP_TRY(hipMemsetAsync(h->st_ctmp, 0, (size_t)GH * NZ * sizeof(float), s));
    gemm::run(s, w.dA, 1, GH, w.X + (c.dt - ns), D, 1, h->st_ctmp, NZ, GH, NZ, TN, true, nullptr, split, bf, false, h->deterministic == 2 ? &h->det_slab : nullptr);
  }
  {
    ProfScope ps(h, "gemm_i2g_bwd_dx_e");    // dx_e [T N][de] = dA W_i2g[:, entity columns], compact
    gemm::run(s, w.dA, GH, 1, Wi + c.dt, D, 1, w.dIn, c.de, TN, c.de, GH, false, nullptr, 1, bf);
  }
  {
    ProfScope ps(h, "small_tables_finish");
    kk::small_tables_finish(s, h->st_ctmp, ns, GH, D, c.dt, c.de, c.dr, c.Vt, c.Vr, h->dense + h->off_Wt, h->dense + h->off_Wr, Wi, gd + h->layer[0].Wi, gd + h->off_Wt,
                            gd + h->off_Wr);
  }
  ProfScope ps(h, "entity_grad");
  entity_grad_rowmajor(h, b, w.dIn, c.de, 0);
}

// ---- forward: the unfused tier's steps ---------------------------------------------------------------------------------------------------------
void forward_steps(kprn_handle* h, const Cell& c, const Layer& y, int T, int64_t N, bool bf) {
  const int H = h->cfg.H;
  hipStream_t s = h->stream;
  for (int t = 0; t < T; ++t) {
    float* a_t = y.act + (int64_t)t * N * c.rec;
    float* h_t = y.hs + (int64_t)t * N * H;
    const float* hp = t > 0 ? h_t - N * H : nullptr;
    if (t > 0) {
      ProfScope ps(h, "gemm_o2g_fwd");
      gemm::run(s, hp, H, 1, y.Wo, 1, H, a_t, c.rec, N, c.g_rows, H, true, nullptr, 1, bf);
    }
    if (c.id == 2) {
      // nn.GRU: the candidate's recurrent product needs r, so a step is gates -> product -> output (two dependent products)
      {
        ProfScope ps(h, c.cell_fwd);
        kk::gru_gates_fwd(s, a_t, hp, N, H);
      }
      if (t > 0) {
        ProfScope ps(h, "gemm_o2g_fwd");
        gemm::run(s, a_t + 3 * H, 4 * H, 1, y.Uc, 1, H, a_t + 2 * H, 4 * H, N, H, H, true, nullptr, 1, bf);
      }
      ProfScope ps(h, c.cell_fwd);
      kk::gru_out_fwd(s, a_t, hp, h_t, N, H);
      continue;
    }
    ProfScope ps(h, c.cell_fwd);
    if (c.id == 0) kk::lstm_gates_fwd(s, a_t, t > 0 ? y.cs + (int64_t)(t - 1) * N * H : nullptr, y.cs + (int64_t)t * N * H, h_t, N, H);
    else kk::rnn_cell_fwd(s, a_t, y.bo, y.mask + (int64_t)t * N, h_t, N, H, c.relu);
  }
}

// ---- backward: the recurrent part of a layer without the persistent launch -------------------------------------------------------------------------
void backward_steps(kprn_handle* h, const Cell& c, const Layer& y, int T, int64_t N, bool bf) {
  Workspace& w = h->ws;
  const int H = h->cfg.H;
  hipStream_t s = h->stream;
  if (y.has_up) {
    HIP_TRY(hipMemsetAsync(w.dH, 0, (size_t)N * H * sizeof(float), s));
    if (c.id == 0) HIP_TRY(hipMemsetAsync(w.dC, 0, (size_t)N * H * sizeof(float), s));
  }
  for (int t = T - 1; t >= 0; --t) {
    float* dA_t = w.dA + (int64_t)t * N * c.rec;
    const float* a_t = y.act + (int64_t)t * N * c.rec;
    const float* hp = t > 0 ? y.hs + (int64_t)(t - 1) * N * H : nullptr;
    const float* dup = y.has_up ? w.dIn + (int64_t)t * N * H : nullptr;
    if (c.id == 2) {
      {
        ProfScope ps(h, c.cell_bwd);
        kk::gru_bwd1(s, a_t, hp, w.dH, dup, dA_t, w.dC /* direct dh' path */, N, H);
      }
      if (t > 0) {
        ProfScope ps(h, "gemm_o2g_bwd_dh");  // d(r*h') = d pre_n * c_h2h
        gemm::run(s, dA_t + 2 * H, 4 * H, 1, y.Uc, H, 1, dA_t + 3 * H, 4 * H, N, H, H, false, nullptr, 1, bf);
      }
      {
        ProfScope ps(h, c.cell_bwd);
        kk::gru_bwd2(s, a_t, hp, dA_t, w.dC, w.dH, N, H);
      }
      if (t > 0) {
        ProfScope ps(h, "gemm_o2g_bwd_dh");  // dh' += [d pre_r | d pre_z] * o2g
        gemm::run(s, dA_t, 4 * H, 1, y.Wo, H, 1, w.dH, H, N, H, 2 * H, true, nullptr, 1, bf);
      }
      continue;
    }
    {
      ProfScope ps(h, c.cell_bwd);
      if (c.id == 0) kk::lstm_gates_bwd(s, a_t, y.cs + (int64_t)t * N * H, t > 0 ? y.cs + (int64_t)(t - 1) * N * H : nullptr, dup, w.dH, w.dC, dA_t, N, H);
      else kk::rnn_cell_bwd(s, a_t, y.hs + (int64_t)t * N * H, y.mask + (int64_t)t * N, dup, w.dH, dA_t, N, H, c.relu);
    }
    if (t > 0) {
      ProfScope ps(h, "gemm_o2g_bwd_dh");
      gemm::run(s, dA_t, c.rec, 1, y.Wo, H, 1, w.dH, H, N, H, c.rec, false, nullptr, 1, bf);
    }
  }
}

// ---- backward: the input maps of a FastLSTM / rnn layer; true: layer 0 went through the small-table identity and the walk is over -----------------------------
bool input_maps(kprn_handle* h, const kprn_batch* b, const Cell& c, const Layer& y, int l, int st_ns, bool bptt, int split, bool bf, DetScratch* det) {
  Workspace& w = h->ws;
  const int GH = c.wi_rows;
  const int64_t TN = (int64_t)b->T * b->N;
  hipStream_t s = h->stream;
  if (det || !(bptt && lp32::bptt_sums_bias(c.id, h->cfg.H))) {   // (the persistent BPTT launch forms the sums itself)
    ProfScope ps(h, "bias_colsum");  // rnn: i2h.bias and h2h.bias see the same gradient (both are added to every pre-activation): one pass over dA for both
    kk::col_sum_add(s, w.dA, TN, GH, y.gbi, 0, y.gb2, det);
  }
  if (l == 0 && st_ns > 0) {
    backward_layer0_small_tables(h, b, st_ns, GH, split, bf);
    return true;
  }
  {
    ProfScope ps(h, "gemm_i2g_bwd_dw");
    gemm::run(s, w.dA, 1, GH, y.in, y.Din, 1, y.gWi, y.Din, GH, y.Din, TN, true, nullptr, split, bf, false, det);
  }
  {
    ProfScope ps(h, "gemm_i2g_bwd_dx");
    gemm::run(s, w.dA, GH, 1, y.Wi, y.Din, 1, w.dIn, y.Din, TN, y.Din, GH, false, nullptr, 1, bf);
  }
  if (h->drop_live) {
    // the product is the gradient wrt the DROPPED input: times the regenerated m s it is the gradient from above of layer l - 1, or what the table
    // gradients of layer 0 are formed from
    ProfScope ps(h, "drop_rows_bwd");
    kk::drop_rows(s, w.dIn, w.dIn, b->N, b->T, y.Din, drop_args(h, l));
  }
  return false;
}

// The GRU's input maps of the gates and of the candidate are two arrays (i2g.weight [2H][Din], c_i2h.weight [H][Din]) but ONE operand of the record's first 3H
// columns: one dW product into a zeroed [3H][Din] image (added to the two gradients behind it) and one dx product on a packed copy -- the [H][Din] halves alone
// fall below the tiled kernel's 256 rows, and the second dx product was a read-modify-write pass over dIn.
void input_maps_gru(kprn_handle* h, const Layer& y, int T, int64_t N, bool bptt, int split, bool bf) {
  Workspace& w = h->ws;
  const int H = h->cfg.H, Din = y.Din;
  const int64_t TN = (int64_t)T * N, cat = (int64_t)3 * H * Din, gates = (int64_t)2 * H * Din;
  hipStream_t s = h->stream;
  dev_grow(s, h->st_ctmp, h->st_ctmp_cap, 2 * cat);
  float* wcat = h->st_ctmp;
  float* gcat = h->st_ctmp + cat;
  {
    ProfScope ps(h, "gemm_i2g_bwd_dw");
    HIP_TRY(hipMemsetAsync(gcat, 0, (size_t)cat * sizeof(float), s));
    gemm::run(s, w.dA, 1, 4 * H, y.in, Din, 1, gcat, Din, 3 * H, Din, TN, true, nullptr, split, bf, /*untiled=*/true);
    kk::add_into(s, y.gWi, gcat, gates);
    kk::add_into(s, y.gWc, gcat + gates, (int64_t)H * Din);
  }
  if (!bptt) {   // (the persistent BPTT launch forms the sums itself)
    ProfScope ps(h, "bias_colsum");
    kk::col_sum_add(s, w.dA, TN, 2 * H, y.gbi, 4 * H);
    kk::col_sum_add(s, w.dA + 2 * H, TN, H, y.gb2, 4 * H);
  }
  ProfScope ps(h, "gemm_i2g_bwd_dx");
  HIP_TRY(hipMemcpyAsync(wcat, y.Wi, (size_t)gates * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(wcat + gates, y.Wc, (size_t)H * Din * sizeof(float), hipMemcpyDeviceToDevice, s));
  gemm::run(s, w.dA, 4 * H, 1, wcat, Din, 1, w.dIn, Din, TN, Din, 3 * H, false, nullptr, 1, bf);
}

}  // namespace

// The only statement of when layer 0's input gradients take the small-table identity; returns ns (the selector columns), 0: the dx product + scatter route.
// The backward asks with the batch's facts, det_check (kprn_api.hip) with the handle's before anything is launched.  dropped: a dropped x_t is no sum of table
// rows, and the route overwrites type columns of the saved input, which the dropped dW product reads
int small_tables_route(const kprn_handle* h, int F, bool dropped, bool have_index) {
  const kprn_config& c = h->cfg;
  const int ns = (c.Vr + c.Vt + 3) & ~3;
  const bool ok = !dropped && h->small_tables && c.num_types == 1 && c.rnn_type != 2 && ns <= c.dt && ns <= 128 && c.de > 0 && c.dr > 0 && have_index && F >= 3;
  return ok ? ns : 0;
}

// the addressing limits of the dropout counter (step and layer share a 32-bit word, the path has one of its own), checked before a training call launches or
// writes anything
void drop_check(const kprn_handle* h, const kprn_batch* b) {
  if (!(h->dropout_p > 0.f) || h->cfg.rnn_type != 1) return;
  KPRN_REQUIRE(b->T <= 65535 && h->cfg.L <= 65535 && b->N < ((int64_t)1 << 32), KPRN_E_ARG,
               "dropout: the mask generator addresses at most 65535 steps, 65535 layers and 2^32 - 1 paths per batch");
}

void forward(kprn_handle* h, const kprn_batch* b, bool save) {
  const kprn_config& c = h->cfg;
  const bool bf = c.compute_dtype == 1;  // bf16 MFMA products, fp32 accumulation (gemm_f32.hip)
  static const bool no_step = getenv("KPRN_NO_STEP_KERNEL") != nullptr;  // (measurement: GEMM + element-wise kernels per step)
  const Cell cell = cell_of(h);
  Workspace& w = h->ws;
  const int H = c.H, L = c.L, T = b->T;
  const int64_t N = b->N;
  hipStream_t s = h->stream;
  // option "dropout" (rnn, fp32): a TRAINING forward drops every layer's step input; a scoring pass never does
  const bool drop = save && h->dropout_p > 0.f && cell.id == 1;
  if (drop) drop_check(h, b);   // (throws before the flag below says that a dropped forward is behind the backward)
  h->drop_live = drop;
  if (drop) {
    h->drop_draw_cur = h->drop_draw++;
    dev_grow(s, w.HsD, w.cap_HsD, (int64_t)(L - 1) * T * N * H);
    ProfScope ps(h, "embed_gather_drop");
    // the dropped rows go to X; MaskZero's flags come from the undropped values in the same pass
    kk::embed_gather_drop(s, b->idx, N, T, b->F, c.num_types, h->dense + h->off_Wt, h->We, h->dense + h->off_Wr, c.dt, c.de, c.dr, w.X, w.mask, drop_args(h, 0));
  } else {
    ProfScope ps(h, "embed_gather");
    // (rnn: MaskZero's mask of the bottom layer's input rows comes out of the same pass)
    kk::embed_gather(s, b->idx, N, T, b->F, c.num_types, h->dense + h->off_Wt, h->We, h->dense + h->off_Wr, c.dt, c.de, c.dr, w.X, true, cell.id == 1 ? w.mask : nullptr);
  }
  // nn.Sequencer(cell) x L (OneModel.lua:237-273): nn.FastLSTM; nn.Recurrence(nn.MaskZero(act(i2h x_t + h2h h_{t-1}), 1)); nn.GRU
  for (int l = 0; l < L; ++l) {
    const Layer y = layer_ops(h, cell, l, T, N, /*dropped=*/false);
    const int Din = y.Din;
    const float* in = y.in;   // (y.in stays the undropped rows: what MaskZero looks at)
    if (drop && l > 0) {
      // the layer reads a dropped COPY of the plane below: the undropped one stays for the layer below's BPTT and for the mask above
      ProfScope ps(h, "drop_rows_fwd");
      float* din = w.HsD + (int64_t)(l - 1) * T * N * H;
      kk::drop_rows(s, in, din, N, T, Din, drop_args(h, l));
      in = din;
    }
    // the tier.  The gru has no step kernel (two dependent products a step) and keeps its persistent launch under KPRN_NO_STEP_KERNEL; the rnn takes the
    // persistent launch only where the step kernel would apply too (N >= 256)
    const bool stepk = cell.id != 2 && !bf && !no_step && gemm::step_supported(in, Din, Din, y.hs, H, H, y.Wi, y.Wo, N);
    const bool persist = !bf && h->persist_layers && (cell.id == 2 || (cell.id == 1 ? stepk : !no_step)) && lp32::supported(cell.id, N, Din, H, h->persist_layers == 2);
    if (!persist && !stepk) {
      ProfScope ps(h, "gemm_i2g_fwd");
      gemm::run(s, in, Din, 1, y.Wi, 1, Din, y.act, cell.rec, (int64_t)T * N, cell.g_rows, Din, false, y.bi, 1, bf);
      if (cell.id == 2) gemm::run(s, in, Din, 1, y.Wc, 1, Din, y.act + 2 * H, 4 * H, (int64_t)T * N, H, Din, false, y.bc, 1, bf);
    }
    if (cell.id == 1 && l > 0) {
      ProfScope ps(h, "rnn_mask");
      kk::row_nonzero(s, y.in, (int64_t)T * N, Din, y.mask);  // layer l > 1: the mask follows the ACTUAL input rows (h^{l-1}_t), as MaskZero does
    }
    if (persist) {
      // all T steps of the layer in ONE persistent launch: h (and c) never leave the CU, weights stream L2 -> LDS by DMA (layer_f32_persist.hip).  A scoring
      // pass needs the top layer's last step only; the training forward writes every step
      ProfScope ps(h, cell.layer_fwd);
      lp32::forward_layer(s, cell.id, in, N, T, Din, H, y.Wi, y.Wo, y.bi, y.bo, y.hs, y.cs, y.act, y.mask, cell.relu, save, /*write_all_h=*/y.has_up, y.Wc, y.Uc, y.bc,
                          h->persist_layers_grid);
    } else if (stepk) {
      // one launch per step: [x_t | h_{t-1}] [W_i2g | W_o2g]^T + b with the cell in the epilogue (gemm_tiled.hip); FastLSTM: gate values are written only
      // when a backward follows; rnn: both biases, the activation and MaskZero
      ProfScope ps(h, cell.step_fwd);
      ps.launches = T;
      for (int t = 0; t < T; ++t) {
        const float* x_t = in + (int64_t)t * N * Din;
        const int64_t at = (int64_t)t * N * H;
        const float* hp = t > 0 ? y.hs + at - N * H : nullptr;
        if (cell.id == 0) gemm::lstm_step(s, x_t, Din, Din, y.Wi, y.bi, hp, y.Wo, t > 0 ? y.cs + at - N * H : nullptr, y.cs + at, y.hs + at, H, save ? y.act + 4 * at : nullptr, N, H);
        else gemm::rnn_step(s, x_t, Din, Din, y.Wi, y.bi, hp, y.Wo, y.bo, y.mask + (int64_t)t * N, y.act + at, y.hs + at, H, N, H, cell.relu);
      }
    } else forward_steps(h, cell, y, T, N, bf);
  }
  ProfScope ps(h, "gemm_head_fwd");
  const float* hT = w.Hs + ((int64_t)(L - 1) * T + (T - 1)) * N * H;
  gemm::run(s, hT, H, 1, h->dense + h->off_outW, 1, H, w.S, c.C, N, c.C, H, false, h->dense + h->off_outb, 1, bf);
}

void backward(kprn_handle* h, const kprn_batch* b, int cid) {
  const kprn_config& c = h->cfg;
  const bool bf = c.compute_dtype == 1;
  const Cell cell = cell_of(h);
  Workspace& w = h->ws;
  const int H = c.H, L = c.L, T = b->T;
  const int64_t N = b->N;
  hipStream_t s = h->stream;
  float* gd = h->g_dense;
  const bool have_index = b->key_sorted != nullptr && !b->tile_k;  // (an index built for a prefix plan lives in the reordered path space)
  const int st_ns = small_tables_route(h, b->F, h->drop_live, have_index);   // > 0: layer 0's input gradients through the small-table identity
  // option "deterministic" = "2" (FastLSTM and rnn cells; det_check has refused the rest): every join of partial sums below takes its slab form -- the producer
  // plain-stores one slab per workgroup or K split into det's scratch, kk::slab_join behind it adds the slabs in index order
  DetScratch* const det = (h->deterministic == 2 && cell.id != 2) ? &h->det_slab : nullptr;
  {
    ProfScope ps(h, "head_bwd");
    const float* hT = w.Hs + ((int64_t)(L - 1) * T + (T - 1)) * N * H;
    kk::head_bwd(s, w.dS, hT, h->dense + h->off_outW, N, H, cid, w.dH, gd + h->off_outW, gd + h->off_outb, det);
  }
  HIP_TRY(hipMemsetAsync(w.dC, 0, (size_t)N * H * sizeof(float), s));
  const int split = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (T * N) / 2048));
  for (int l = L - 1; l >= 0; --l) {
    // (dropout: the input the layer saw is the dropped one -- X holds it for layer 0, HsD for the layers above)
    const Layer y = layer_ops(h, cell, l, T, N, h->drop_live);
    const bool bptt = !bf && h->persist_layers && lp32::bptt_supported(cell.id, N, H, h->persist_layers == 2);
    if (bptt) {
      // the cell backward of all T steps + the recurrent gradient (gru: both recurrent products of a step) in ONE persistent launch (layer_f32_persist.hip
      // k_bptt): dh / dc never leave the CU.  det: no bias sums inside the launch -- its workgroups join them with atomics; the column sum over dA takes them
      ProfScope ps(h, cell.layer_bwd);
      float* wot = dev_grow(s, h->lp_wot, h->lp_wot_cap, (int64_t)lp32::bptt_scratch_floats(H, cell.wi_rows));   // W_o2g^T (gru: [c_h2h^T | o2g^T])
      lp32::bptt_layer(s, cell.id, cell.id == 1 ? nullptr : y.act, y.cs, cell.id == 0 ? nullptr : y.hs, y.mask, y.has_up ? w.dIn : w.dH, y.has_up, y.Wo, wot, w.dA, N, T, H,
                       cell.relu, y.Uc, det ? nullptr : y.gbi, det ? nullptr : y.gb2, h->persist_layers_grid);
    } else backward_steps(h, cell, y, T, N, bf);
    if (T > 1) {
      ProfScope ps(h, "gemm_o2g_bwd_dw");
      // gWo += dA[1..T-1]^T h[0..T-2]  (gru: off gemm_tiled.hip, kprn_internal.h gemm::run)
      gemm::run(s, w.dA + N * cell.rec, 1, cell.rec, y.hs, H, 1, y.gWo, H, cell.g_rows, H, (int64_t)(T - 1) * N, true, nullptr, split, bf, /*untiled=*/cell.id == 2, det);
      if (cell.id == 2)   // c_h2h += d pre_n[1..T-1]^T (r*h')[1..T-1]
        gemm::run(s, w.dA + N * 4 * H + 2 * H, 1, 4 * H, y.act + N * 4 * H + 3 * H, 4 * H, 1, y.gUc, H, H, H, (int64_t)(T - 1) * N, true, nullptr, split, bf);
    }
    if (cell.id == 2) input_maps_gru(h, y, T, N, bptt, split, bf);
    else if (input_maps(h, b, cell, y, l, st_ns, bptt, split, bf, det)) return;
  }
  {
    ProfScope ps(h, "embed_scatter");
    kk::embed_scatter(s, b->idx, N, T, b->F, c.num_types, w.dIn, c.dt, c.de, c.dr, c.Vt, c.Vr, gd + h->off_Wt, h->g_We, gd + h->off_Wr, have_index, det);
  }
  if (have_index) {
    ProfScope ps(h, "entity_grad");
    entity_grad_rowmajor(h, b, w.dIn, h->D, c.dt);
  }
}

}  // namespace generic
