/*
 * kprn.h -- C ABI of libkprn.so: the MI355X (gfx950) path-scoring engine behind the
 * songPathRnn training / scoring surface of eBay/KPRN.
 *
 * The reference has NO native boundary; the operator API this library replaces is the
 * Torch7 nn.Module protocol as consumed by exactly two callers:
 *   release/songPathRnn/model/optimizer/MyOptimizer.lua:177-221  (trainBatch: zeroGrad,
 *       forward, BCE, backward, clip/L2, optim step, zeroPadTokens)
 *   release/songPathRnn/eval/test_from_checkpoint.lua:98-118     (model:forward -> preds[i])
 * Each entry point below cites the reference lines it stands in for.  The binding a
 * maintainer adds on the reference side (LuaJIT ffi.cdef) is in INTEGRATION.md and
 * bindings/kprn.lua.
 *
 * Conventions
 *  - plain C, no torch types; every function returns 0 on success or a negative
 *    kprn_status; the message is available from kprn_last_error(h) (h may be NULL for
 *    a failed kprn_create).  Nothing throws or aborts across the ABI.
 *  - the caller owns every host buffer it passes; the library owns all device memory.
 *  - indices are int32, 1-BASED, row-major [B,P,T,F] exactly like the reference's
 *    data tensor (release/songPathRnn/model/batcher/Batcher.lua:51): F columns per step =
 *    numEntityTypes type ids, then entity id, then relation id
 *    (model/net/FeatureEmbedding.lua:51,88,31).  Out-of-range ids are an error
 *    (KPRN_E_INDEX), never undefined behaviour.
 *  - one handle <-> one GPU <-> one host thread at a time.  Work is queued on one HIP
 *    stream; functions that return results to host memory synchronise that stream,
 *    functions documented "async" do not.
 *  - parameters are named and ordered as nn.Module:getParameters() flattens them
 *    (MyOptimizer.lua:42):  type_emb[Vt,dt] | entity_emb[Ve,de] | relation_emb[Vr,dr] |
 *    lstm{l}.i2g.weight[4H,D_l] lstm{l}.i2g.bias[4H] lstm{l}.o2g.weight[4H,H] (l=1..L) |
 *    out.weight[C,H] | out.bias[C]          (host side: row-major fp32)
 *    FastLSTM gate order inside the 4H rows: input, candidate(tanh), forget, output.
 *    rnnType rnn: per layer rnn{l}.i2h.weight[H,D_l] | rnn{l}.i2h.bias[H] | rnn{l}.h2h.weight[H,H] | rnn{l}.h2h.bias[H]
 *    rnnType gru: per layer gru{l}.i2g.weight[2H,D_l] | gru{l}.i2g.bias[2H] | gru{l}.o2g.weight[2H,H] (rows: reset, update) |
 *                 gru{l}.c_i2h.weight[H,D_l] | gru{l}.c_i2h.bias[H] | gru{l}.c_h2h.weight[H,H]
 */
#ifndef KPRN_H
#define KPRN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kprn_handle kprn_handle;
typedef struct kprn_batch kprn_batch;
typedef struct kprn_graph kprn_graph;
typedef struct kprn_sampler kprn_sampler;

typedef enum {
  KPRN_OK = 0,
  KPRN_E_ARG = -1,          /* bad argument / shape / name                        */
  KPRN_E_INDEX = -2,        /* an id outside 1..V                                 */
  KPRN_E_DEVICE = -3,       /* HIP error (message has the HIP string)             */
  KPRN_E_UNSUPPORTED = -4,  /* valid reference option not built yet               */
  KPRN_E_IO = -5,
  KPRN_E_NOMEM = -6
} kprn_status;

/* mirrors the torch.CmdLine flags of model/OneModel.lua:27-87 that shape the graph */
typedef struct {
  int32_t Vt, Ve, Vr;        /* -entityTypeVocabSize -entityVocabSize -relationVocabSize        */
  int32_t dt, de, dr;        /* -entityTypeEmbeddingDim -entityEmbeddingDim -relationEmbeddingDim; dt = 0: -includeEntityTypes 0 (no type
                                table in x_t), de = 0: -includeEntity 0 (no entity table): OneModel.lua:207-219; generic pipeline */
  int32_t F;                 /* -numFeatureTemplates                                             */
  int32_t num_types;         /* -numEntityTypes                                                  */
  int32_t H;                 /* -rnnHidSize                                                      */
  int32_t L;                 /* -numLayers  (L>1 requires dt+de+dr == H, OneModel.lua:236,270)   */
  int32_t C;                 /* labelDimension, 46 in the reference (OneModel.lua:119)           */
  int32_t rnn_type;          /* -rnnType: 0 = lstm (nn.FastLSTM), 1 = rnn (nn.Recurrence + nn.MaskZero, OneModel.lua:240-266;
                                the shipped config.sh default), 2 = gru (nn.GRU, OneModel.lua:237-238); rnn and gru run on the
                                generic pipeline */
  int32_t use_relu;          /* -useReLU (rnn): 1 = nn.ReLU, else nn.Tanh (OneModel.lua:225-229)  */
  int32_t rnn_init;          /* -rnnInitialization (rnn): i2h / h2h weights <- eye, biases <- 0 (OneModel.lua:310-322) */
  int32_t compute_dtype;     /* 0 = f32 (exact fp32 MFMA; the reference's arithmetic type on GPU).
                                1 = bf16: the recurrent / head GEMMs multiply in bf16 (operands rounded to nearest even) and
                                    accumulate in f32; parameters, activations and the optimiser stay f32 (BASELINE configs[3]).
                                    Scoring at D = H = 64 takes the fused matrix-core forward, everything else the generic pipeline.
                                2 = f32x6: fp32 results from the bf16 matrix cores -- every fp32 operand is split exactly into
                                    three bf16 pieces and the six partial products of weight >= 2^-16 are accumulated in f32; the
                                    dropped products are below 2^-24, i.e. the error is that of an fp32 FMA chain or smaller.
                                    Fused path only (forward on the matrix cores, backward as for 0); held to the same parity
                                    tolerances as 0.
                                3 = f32x3: as 2 with two fp16 pieces (2 x 11 mantissa bits) of every power-of-two pre-scaled
                                    operand and three partial products: half the matrix instructions of 2; the operands keep 22
                                    of their 24 mantissa bits.  Same tolerances.  Operand range: the fp16 high piece overflows,
                                    and the result is silently NaN, once |W_o2g| or the top layer's |W_i2g| exceeds 88.7 on the g
                                    rows (177 on i, f, o), the bottom layer's |W_i2g| 1419 (2838), or a table value 4094
                                    (65504 / (2^8 * 2 log2 e), / (2^4 * ...), / 2^4).  New options, not in the reference.      */
  int32_t reducer;           /* -topK: 0 = Max, 1 = TopK+Mean, 2 = LogSumExp (OneModel.lua:284-293) */
  int32_t K;                 /* -K                                                               */
  int32_t device_id;         /* HIP device ordinal                                               */
  int32_t rank, world;       /* data-parallel position; loss is scaled by the GLOBAL batch       */
  float param_init;          /* -paramInit: uniform(-a, a) over every parameter (OneModel.lua:306-309) */
  uint64_t seed;             /* init RNG seed (the reference leaves it unseeded, OneModel.lua:123) */
  void* stream;              /* hipStream_t the engine queues on.  NULL = the engine creates its own non-blocking stream (fetch it
                                with kprn_stream).  NOTE: the legacy default stream's handle is ALSO 0 -- a caller that means "my
                                default stream" (torch.cuda.current_stream() before any stream is set) must say
                                KPRN_STREAM_LEGACY_DEFAULT, or its own work is not ordered with the engine's.                    */
} kprn_config;
/* kprn_config.stream value for the legacy default (null) stream: the engine then queues on stream 0 instead of creating one */
#define KPRN_STREAM_LEGACY_DEFAULT ((void*)(intptr_t)-1)

/* mirrors optInfo / optConfig (OneModel.lua:340-384) */
typedef struct {
  int32_t method;            /* -useAdam: 1 = optim.adam, 0 = optim.adagrad                      */
  float lr;                  /* -learningRate                                                    */
  float beta1, beta2, eps;   /* 0.9, 0.999, -epsilon                                             */
  float lr_decay;            /* -learningRateDecay (adagrad)                                     */
  int32_t regularize;        /* -regularize: gates BOTH clip and L2 (MyOptimizer.lua:196)        */
  int32_t use_grad_clip;     /* -useGradClip                                                     */
  float grad_clip_norm;      /* -gradClipNorm                                                    */
  float l2;                  /* -l2                                                              */
  int32_t bce_literal;       /* 1 = nn.BCECriterion backward then nn.Sigmoid backward, eps 1e-12;
                                0 = fused (p - t)/B (identical away from fp32 saturation)         */
  int32_t entity_update;     /* 0 = lazy-exact: rows of entity_emb are brought up to date when
                                    touched; bit-identical to the dense update of optim.adam
                                1 = dense: every row every step, as the reference does          */
} kprn_opt;
/* Every field but method may change from one step to the next and the result stays that of the dense update with the same per-step values: lr costs
 * nothing; a change of beta1 / beta2 / eps, of entity_update 0 -> 1 or of regularize 0 -> 1 while entity rows lag costs one whole-table flush.  method
 * stays what the handle's first step used (KPRN_E_ARG otherwise): both methods keep their state in optimiser slot 0.                              */

/* ---- lifetime -------------------------------------------------------------------- */
/* OneModel.lua:204-309: build predictor_net + reducer, init uniform(-paramInit,paramInit) */
int kprn_create(const kprn_config* cfg, kprn_handle** out);
void kprn_destroy(kprn_handle* h);
const char* kprn_last_error(const kprn_handle* h);
/* library / kernel build id, e.g. "kprn-amd 0.1 gfx950" */
const char* kprn_version(void);

/* ---- parameters (nn.Module:parameters()/getParameters(), MyOptimizer.lua:42) -------- */
int kprn_num_params(kprn_handle* h, int64_t* n);
/* n = element count of dst/src, must match the tensor */
int kprn_get_param(kprn_handle* h, const char* name, float* dst, int64_t n);
int kprn_set_param(kprn_handle* h, const char* name, const float* src, int64_t n);
int kprn_get_grad(kprn_handle* h, const char* name, float* dst, int64_t n);
/* n_rows rows of one tensor by 0-based row index (Lua: lookup.weight[id], id = row + 1; net/FeatureEmbedding.lua:29,41-49,86):
   what one reads / writes of a 20 M-row nn.LookupTable without moving the table.  dst / src: [n_rows][cols] */
int kprn_get_param_rows(kprn_handle* h, const char* name, const int64_t* rows, int64_t n_rows, float* dst);
int kprn_set_param_rows(kprn_handle* h, const char* name, const int64_t* rows, int64_t n_rows, const float* src);
/* whole flat vector in getParameters() order */
int kprn_get_flat_params(kprn_handle* h, float* dst, int64_t n);
int kprn_set_flat_params(kprn_handle* h, const float* src, int64_t n);
int kprn_get_flat_grads(kprn_handle* h, float* dst, int64_t n);
/* optimiser state (optState: adam m,v / adagrad paramVariance) -- slot 0 or 1 */
int kprn_get_flat_opt_state(kprn_handle* h, int32_t slot, float* dst, int64_t n);
/* MyOptimizer:zeroPadTokens (MyOptimizer.lua:74-93): zero row V (1-based) of each table */
int kprn_zero_pad_tokens(kprn_handle* h);

/* ---- batches resident in HBM (BatcherFileList:populateGPUTensor, BatcherFileList.lua:78-96) */
/* validates every id against its vocabulary; labels may be NULL for scoring            */
int kprn_batch_create(kprn_handle* h, const int32_t* idx, const float* labels,
                      int32_t B, int32_t P, int32_t T, int32_t F, kprn_batch** out);
void kprn_batch_destroy(kprn_handle* h, kprn_batch* b);
/* Streaming feed = BatcherFileList's GPU double buffer (BatcherFileList.lua:53-96: tensors preallocated once, every minibatch
 * :copy()'d into them): (re)fills *slot (NULL: a new slot is allocated; a refill that fits the slot's buffers allocates nothing)
 * with the upload, the id validation, the occurrence index and the identical-prefix plan queued on a dedicated FEED stream, and
 * returns at once.  The feed starts behind everything queued on the handle so far (the last readers of the slot's previous
 * contents among it) and runs under whatever is queued next -- call it for batch i+1 right before the step on batch i.  The first
 * call that uses the slot waits for its feed; an out-of-range id surfaces there as KPRN_E_INDEX.  idx / labels must stay
 * unchanged until then; only page-locked host memory (kprn_host_alloc) is copied without holding the calling thread.      */
int kprn_batch_feed_async(kprn_handle* h, kprn_batch** slot, const int32_t* idx, const float* labels,
                          int32_t B, int32_t P, int32_t T, int32_t F);
/* The same for a SHUFFLED epoch (Batcher:shuffle, Batcher.lua:35-41, permutes the file's tensors; OneModel.lua:326 turns it on):
 * pair i of the minibatch is row rows[i] (0-based, < n_rows) of the file's arrays data [n_rows,P,T,F] / labels [n_rows], gathered
 * by the feed's worker threads straight into the upload image -- the caller permutes nothing and copies nothing.  data and rows
 * must stay unchanged until the slot's first use; labels are read before the call returns.                              */
int kprn_batch_feed_rows_async(kprn_handle* h, kprn_batch** slot, const int32_t* data, const float* labels, int64_t n_rows,
                               const int64_t* rows, int32_t B, int32_t P, int32_t T, int32_t F);
/* BatcherFileList.lua:53-60: size a slot once for the largest minibatch it will hold (max_pairs pairs, max_paths paths of T steps), so that
 * no later feed allocates (an allocation waits for the device).  *slot NULL: a new, empty slot.  Capacities only ever grow.           */
int kprn_batch_slot_reserve(kprn_handle* h, kprn_batch** slot, int32_t max_pairs, int64_t max_paths, int32_t T, int32_t F, int32_t with_labels);
/* Where the feed derives a batch's plan and index: kprn_set_option(h, "feed_build", "host") (default) -- worker threads on the host
 * cores write them into page-locked staging and the GPU sees DMA traffic only ("feed_workers" batches at once, "feed_threads" helper
 * threads each) -- or "device": the kernels of kprn_batch_create on a side stream.  Same arrays either way.
 * kprn_host_batch_index is the host derivation on its own (no handle, no GPU): ids [B,P,T,F] -> validation, identical-prefix plan
 * (plan != 0: idx_s [B*P*T*F], perm / slot_of [B*P], tile_k [ceil(B*P/64)], pmeta [24]) and the entity-occurrence index
 * (key_sorted / pos_sorted / uniq: B*P*T + 8 entries each); summary[4] = {an id out of range, longest shared prefix, distinct
 * entity rows, (path, step) positions the kernels execute}.                                                             */
int kprn_host_batch_index(const int32_t* idx, int32_t B, int32_t P, int32_t T, int32_t F, int32_t num_types, int32_t Vt, int32_t Ve, int32_t Vr,
                          int32_t plan, int32_t threads, int32_t* idx_s, int32_t* perm, int32_t* slot_of, int32_t* tile_k, int32_t* pmeta,
                          int32_t* key_sorted, int32_t* pos_sorted, int32_t* uniq, int64_t* summary);
/* ---- ragged batches (an extension: the reference has one path count per batch, one file per count) ----
 * A ragged batch is B pairs over a flat id array idx [N,T,F]: pair b owns counts[b] >= 1 consecutive paths, N = sum(counts).  It is accepted
 * wherever a kprn_batch is (scoring sync / async, kprn_backward_batch, kprn_train_step_batch, the kprn_dp_* calls); the recurrent kernels
 * are the same (they are flat over the paths), the reducer over a pair's paths and the loss stage are segmented kernels.  The loss is scaled
 * by the number of PAIRS, path_scores of kprn_forward_batch is [N,C].  A pair of at most 28 paths is reduced in the rectangular kernels'
 * order (equal counts give the rectangular batch's bits in the forward pass); a batch with a longer pair reduces every pair with one
 * wave (64 lanes).  At most 4096 paths per pair, N*T within 32-bit positions; a count outside 1..4096 or counts that do not add up to N
 * are KPRN_E_ARG, and nothing of the slot is changed.                                                                               */
int kprn_batch_create_ragged(kprn_handle* h, const int32_t* idx, const int32_t* counts, const float* labels /* [B] or NULL */,
                             int32_t B, int64_t N, int32_t T, int32_t F, kprn_batch** out);
/* kprn_batch_feed_async for a ragged batch ("feed_build" host or device); counts are read before the call returns.  A slot may hold a
 * rectangular batch after a ragged one and the reverse (kprn_batch_slot_reserve sizes it for either).                               */
int kprn_batch_feed_ragged_async(kprn_handle* h, kprn_batch** slot, const int32_t* idx, const int32_t* counts, const float* labels,
                                 int32_t B, int64_t N, int32_t T, int32_t F);
/* what the engine derives from the counts, on its own (no handle, no GPU): offsets [B+1]; wg_first [n_wg+1] = the first pair of each
 * loss-stage workgroup (consecutive pairs, at most 16 pairs and at most 448 paths per workgroup; a longer pair is a workgroup of its own),
 * room for B+1 entries; summary[8] = {n_wg, longest pair, 1 when the batch is reduced by a wave per pair, the limits: paths per pair,
 * longest pair one thread reduces, paths per workgroup, pairs per workgroup, 0}.  KPRN_E_ARG as above.                              */
int kprn_host_ragged_plan(const int32_t* counts, int32_t B, int64_t N, int32_t* offsets, int32_t* wg_first, int32_t* summary);
/* paths of a batch: B*P, or N of a ragged batch */
int kprn_batch_num_paths(kprn_handle* h, const kprn_batch* b, int64_t* n);
/* page-locked host buffers for the feed (the reference preallocates its staging tensors likewise, BatcherFileList.lua:53-60) */
int kprn_host_alloc(kprn_handle* h, size_t bytes, void** out);
int kprn_host_free(kprn_handle* h, void* p);
/* number of distinct entity rows the batch references (= the rows one training step on it touches) */
int kprn_batch_distinct_rows(kprn_handle* h, const kprn_batch* b, int32_t* n);
/* (path, step) positions a pass over the batch executes: B*P*T, less the leading steps that whole 64-path tiles share with
 * the batch's reference step (left padding, movie_data_format.py:250-254) and that the fused kernels therefore run once
 * for the batch instead of once per path -- same results; for work / roofline accounting                                  */
int kprn_batch_executed_steps(kprn_handle* h, const kprn_batch* b, int64_t* steps);
/* what the fused BPTT launches' time-split tile hand-over (option "tile_handover") does with this batch: out[0] = pairs of workgroups
 * between which a tile changes hands, out[1] = steps moved in all, out[2] / out[3] = the longest workgroup's work in HALF steps with whole
 * tiles only / with the hand-over (a tile's first executed step counts one half: it has no recurrent product).  All zero / equal when the
 * batch does not run on the fused kernels or the option is off.  Diagnostics: waits for the engine's stream.                          */
int kprn_batch_handover_stats(kprn_handle* h, const kprn_batch* b, int64_t* out /* [4] */);

/* ---- scoring: model:forward(inputs) (test_from_checkpoint.lua:81-82,109) ------------
 * probs[B]      = Sigmoid(reduce_p(mapper))[:, classId]       (Select(2,classId))
 * all_probs     = optional [B,C] (before Select)
 * pooled        = optional [B,C] reducer output before Sigmoid
 * path_scores   = optional [B*P,C] mapper output (nn.Linear(H,46), OneModel.lua:275); [N,C] for a ragged batch */
int kprn_forward(kprn_handle* h, const int32_t* idx, int32_t B, int32_t P, int32_t T, int32_t F,
                 int32_t class_id, float* probs, float* all_probs);
/* the same for a ragged batch in host buffers, one call (one user's candidate items, whatever their path counts): probs [B], all_probs
 * optional [B,C]                                                                                                                 */
int kprn_forward_ragged(kprn_handle* h, const int32_t* idx, const int32_t* counts, int32_t B, int64_t N, int32_t T, int32_t F,
                        int32_t class_id, float* probs, float* all_probs);
int kprn_forward_batch(kprn_handle* h, const kprn_batch* b, int32_t class_id,
                       float* probs, float* all_probs, float* pooled, float* path_scores);
/* async variant for throughput loops: results stay on the device until kprn_read_probs  */
int kprn_forward_batch_async(kprn_handle* h, const kprn_batch* b, int32_t class_id);
/* kprn_set_option(h, "score_split", "f"): kprn_forward_batch_async queues the first (1 - f) of the batch's 64-path tiles only; this call queues
 * the rest + the pooling stage behind everything queued so far (a data-parallel step: between kprn_dp_exchange_begin and _finish, so that the
 * collective has compute to hide under while most of the pass shared the chip with the training forward).  Whatever waits for the pass
 * (the optimiser step, kprn_read_probs) places a forgotten second part itself. */
int kprn_forward_batch_async_rest(kprn_handle* h);
/* the selected class's probabilities of the most recent scoring pass, probs [B] with B at most that pass's pairs.  A pass queued by
 * kprn_forward_batch_async stays that pass across training steps made before it is read (beside it, or carrying it: "score_dual"), with its own
 * pair count, whatever the training batch's; the next kprn_forward_batch_async replaces it. */
int kprn_read_probs(kprn_handle* h, float* probs, int32_t B);
/* embedding sub-net output x[N,T,D] (FeatureEmbedding.lua:112-121), for bit-exact checks */
int kprn_embed(kprn_handle* h, const int32_t* idx, int64_t N, int32_t T, int32_t F, float* x);

/* ---- ranking (an extension: the reference ranks in Python, from the text file the scoring writer leaves) ----
 * The reference's evaluation chain (eval/combine_result.py -> resort.py -> eval_score.py) as an engine stage: scores stay on the device, a kernel
 * ranks GROUPS of candidates (one user's positive and negatives), and only ranks, top-K lists and a rank histogram come back.
 * A group is a list of member scores s[0..n-1], 1 <= n <= KPRN_RANK_MAX_GROUP, and optionally the position pos of its positive.
 *  - mode KPRN_RANK_PRINTED (the chain's rule), for scores in [0, 1]: key = the integer "%.5f" prints, times 1e5 = rint((double)s * 1e5) (the product
 *    is exact in double and rint rounds half to even, as printf does); mode KPRN_RANK_RAW: key = the fp32 value, any finite value or +-inf.
 *  - invalid members: NaN in either mode (a board entry nothing wrote), and in mode 0 anything outside [0, 1].  An invalid member sorts below every
 *    valid one and is counted.
 *  - order: key descending, then member index ascending (heapq.nlargest keeps the first seen on a tie, eval_score.py:38); a member's place is the
 *    number of members before it in that order.
 *  - rank of the group = place of member pos (0-based).  Mode 0: a group in which no member prints above zero has rank KPRN_RANK_ZERO_GROUP (a miss for
 *    every k, eval_score.py:35-36).  pos = -1: no positive, top-K only, rank KPRN_RANK_NO_POSITIVE.
 *  - top-K: the first K members in that order, 1 <= K <= KPRN_RANK_MAX_K: index within the group and the RAW fp32 score; -1 / 0.0f where n < K.
 *  - hist [hist_len + 4] (int64): hist[r] = groups of rank r < hist_len, then [hist_len] = ranked lower, [hist_len + 1] = zero groups,
 *    [hist_len + 2] = groups without positive, [hist_len + 3] = invalid members seen.  hit@k = sum(hist[:k]) / n_groups, ndcg@k =
 *    sum(hist[r] * ln 2 / ln(r + 2), r < k) / n_groups with n_groups = every group that has a positive (zero groups included), formed by the caller.
 * Scores are addressed by global line number on a device-resident BOARD, because a user's candidates are not consecutive in a scored test set (the
 * pairs are bucketed by path count; the chain reunites them by line number, combine_result.py:24-27).  In a data-parallel run every rank ranks what
 * it scored; nothing here crosses ranks.                                                                                                        */
#define KPRN_RANK_PRINTED 0
#define KPRN_RANK_RAW 1
#define KPRN_RANK_ZERO_GROUP (-1)
#define KPRN_RANK_NO_POSITIVE (-2)
#define KPRN_RANK_MAX_GROUP 4096
#define KPRN_RANK_MAX_K 64
/* (re)sizes the board to n entries; keeps nothing; every entry starts as NaN (= invalid until written) */
int kprn_board_reserve(kprn_handle* h, int64_t n);
/* the selected-class probabilities of the most recent scoring pass (the B values kprn_read_probs would return) -> board[offset .. offset + B), queued
 * behind that pass on whichever stream ran it, ordered with events the way kprn_read_probs orders its copy (a forgotten second part of a split pass is
 * placed first).  Async: no host synchronise.  A later pass does not overwrite the pass's output before the put has read it.  KPRN_E_ARG: no pass to
 * read from, or B beyond that pass's pairs; KPRN_E_INDEX: the range leaves the board.                                                           */
int kprn_board_put(kprn_handle* h, int64_t offset, int32_t B);
/* host scores -> board (scores computed elsewhere) and back; both wait for every put queued so far and return when the copy is done */
int kprn_board_write(kprn_handle* h, int64_t offset, const float* src, int64_t n);
int kprn_board_read(kprn_handle* h, int64_t offset, float* dst, int64_t n);
/* ranks G groups of board entries.  members [M] = board line numbers, group g = members[group_offsets[g] .. group_offsets[g + 1]) (a line may appear
 * more than once); members NULL: group g is the consecutive run of board entries group_offsets[g] .. group_offsets[g + 1].  pos [G] or NULL (= 0
 * everywhere).  Any of ranks [G], topk_idx + topk_score [G,K] (both or neither), hist [hist_len + 4] may be NULL.  Waits for every put queued so far;
 * synchronous: the results are on the host when it returns, hist holds this call's groups only.  A member outside the board is KPRN_E_INDEX; a group
 * outside 1..4096 members, pos outside -1..n-1, K outside 1..64, hist_len outside 1..4096 or an unknown mode is KPRN_E_ARG; on an error nothing is written. */
int kprn_rank_groups(kprn_handle* h, const int64_t* members, const int64_t* group_offsets, const int32_t* pos, int32_t G,
                     int32_t mode, int32_t K, int32_t* ranks, int32_t* topk_idx, float* topk_score, int64_t* hist, int32_t hist_len);
/* one user's (or G users') candidates in host buffers -> each group's K best in one call: the pass of kprn_forward_ragged, ranked on the device behind
 * it, one wait.  group_counts [G] = pairs per group, consecutive, summing to B.  topk_idx (index within the group) / topk_score [G,K]; probs [B] may be
 * NULL.  The board is not involved.                                                                                                             */
int kprn_recommend_ragged(kprn_handle* h, const int32_t* idx, const int32_t* counts, int32_t B, int64_t N, int32_t T, int32_t F, int32_t class_id,
                          const int32_t* group_counts, int32_t G, int32_t mode, int32_t K, int32_t* topk_idx, float* topk_score, float* probs);
/* the same rule on the host cores over a host score array (no handle, no GPU): the arguments of kprn_rank_groups with scores [n_scores] as the board */
int kprn_host_rank_groups(const float* scores, int64_t n_scores, const int64_t* members, const int64_t* group_offsets, const int32_t* pos, int32_t G,
                          int32_t mode, int32_t K, int32_t* ranks, int32_t* topk_idx, float* topk_score, int64_t* hist, int32_t hist_len);

/* ---- ranking targets in groups of any size (an extension: held-out evaluation against everything a user reaches; the reference's own protocol, each held
 * pair against 100 sampled negatives, is "sampled evaluation groups" below and ranks with kprn_rank_groups) ----
 * kprn_rank_groups stops at 4096 members and one positive; in three hops a user reaches most of a catalogue and has several held-out items.  Here a
 * group has any size and any number of TARGETS, and only the targets' places and their histogram come back.
 *  - groups: scores live on the board; group g = members[group_offsets[g] .. group_offsets[g + 1]) as in kprn_rank_groups, members NULL = the
 *    consecutive board run.  1 <= n < 2^31 members.
 *  - targets: group g's are targets[target_offsets[g] .. target_offsets[g + 1]), indices WITHIN the group, strictly ascending; a group may have none;
 *    target_offsets[0] = 0 and NT = target_offsets[G] >= 1.
 *  - order: key and validity exactly as in "ranking" (modes KPRN_RANK_PRINTED / KPRN_RANK_RAW; NaN invalid in both, anything outside [0, 1] invalid in
 *    the printed mode; an invalid member sorts below every valid one).  Every member is one integer ((uint64_t)key << 32) | (0xFFFFFFFF - index):
 *    key descending, first seen first -- the order of "ranking" with the index in 32 bits instead of 12.
 *  - place: every target is its own sample, ranked against the group's NON-targets (eval_score.py: one positive against that user's negatives):
 *    place(t) = the number of non-target members of the group whose integer is larger than t's
 *             = (members with a larger integer) - (targets of the group with a larger integer).
 *  - zero samples: mode 0, neither t nor any non-target member of its group prints above zero: place KPRN_RANK_ZERO_GROUP (eval_score.py:35, as for
 *    groups).  A group in which only ANOTHER target prints above zero is a zero sample for t and an ordinary one for that other target.
 *  - places [NT] (int32), in the order of targets.  hist [hist_len + 4] (int64), hist_len in 1..4096: hist[r] = targets at place r < hist_len,
 *    [hist_len] = ranked lower, [hist_len + 1] = zero samples, [hist_len + 2] = always 0, [hist_len + 3] = invalid members, each group's counted
 *    once (groups without targets included).  The layout of kprn_rank_groups' histogram with samples for groups: hit@k and ndcg@k are formed the same way.
 * Nothing depends on timing: places come from integer counts and a prefix sum, the histogram from integer adds.
 * kprn_rank_targets waits for every put queued so far; synchronous, one launch and one wait: places and hist are on the host when it returns and hold
 * this call only.  Everything is checked on the host first and a refused call writes nothing: KPRN_E_ARG for NULL offsets / targets / places / hist, G < 1,
 * a group outside 1..2^31-1 members, more targets than members, target_offsets[0] != 0, NT = 0, a target outside its group or not above the one before,
 * hist_len outside 1..4096, an unknown mode, or no board; KPRN_E_INDEX for a member or a run outside the board.                                  */
int kprn_rank_targets(kprn_handle* h, const int64_t* members, const int64_t* group_offsets, const int64_t* target_offsets, const int32_t* targets,
                      int32_t G, int32_t mode, int32_t* places, int64_t* hist, int32_t hist_len);
/* the same rule on the host cores over a host score array (no handle, no GPU): the arguments of kprn_rank_targets with scores [n_scores] as the board */
int kprn_host_rank_targets(const float* scores, int64_t n_scores, const int64_t* members, const int64_t* group_offsets, const int64_t* target_offsets,
                           const int32_t* targets, int32_t G, int32_t mode, int32_t* places, int64_t* hist, int32_t hist_len);

/* ---- explaining a recommendation (an extension: the paper's pooling layer read backwards) ----
 * Which paths put a pair where it is: the M strongest paths behind the pair's pooled score in the selected class, each with the share it takes of that
 * score (for LogSumExp at the default "pool_gamma" that is d pooled / d s_q, the factor the loss stage multiplies dy by; under a temperature see
 * "pooling temperature" below, rule 4).  For a pair whose cnt paths have the fp32 scores s_0 .. s_{cnt-1}:
 *  - order: score descending, then path index ascending among equal scores (plain fp32 > / ==, so -0 and +0 tie; the reducers' own tie rule); a NaN
 *    score sorts after every number, lower index first.
 *  - weight: LogSumExp: expf((s_q - m) ig) / sum_p expf((s_p - m) ig), m = the maximum, ig = 1 unless "pool_gamma" is set; Max: 1 for the first place, 0 elsewhere; TopK + Mean: 1 / kk for the
 *    first kk = min(K, cnt) places, 0 elsewhere.
 *  - per explained pair, 1 <= M <= KPRN_EXPLAIN_MAX_M: path_idx [M] (index within the pair, 0-based; -1 where cnt < M), path_score [M] (the raw fp32
 *    score; 0.0f in empty places), path_weight [M] (0.0f in empty places), pooled (the reducer's output) and prob = sigmoid(pooled): the bits a scoring
 *    pass over the batch returns for that pair.
 * The mapper output stays on the device; only the M rows per pair come back.                                                                */
#define KPRN_EXPLAIN_MAX_M 32
/* runs the scoring pass of kprn_forward_batch on the batch (rectangular or ragged), then explains n_pairs pairs (0-based, repeats allowed; pairs NULL =
 * every pair in order, n_pairs = the batch's pair count) behind it on the same stream; one wait.  path_idx / path_score / path_weight [n_pairs,M];
 * pooled, probs [n_pairs] or NULL.  M outside 1..32 is KPRN_E_ARG, a pair outside 0..B-1 KPRN_E_INDEX; a refused call writes nothing.     */
int kprn_explain_batch(kprn_handle* h, const kprn_batch* b, int32_t class_id, const int32_t* pairs /* [n_pairs] or NULL */, int32_t n_pairs, int32_t M,
                       int32_t* path_idx, float* path_score, float* path_weight, float* pooled /* or NULL */, float* probs /* or NULL */);
/* kprn_recommend_ragged, and each group's K winners explained: the explanation launch reads its pair list from the rows the ranking kernel wrote, so
 * nothing returns to the host between ranking and explanation; one wait in all.  path_idx / path_score / path_weight [G,K,M]; the places n <= s < K
 * of a group of n < K members are -1 / 0 rows.                                                                                              */
int kprn_recommend_explain_ragged(kprn_handle* h, const int32_t* idx, const int32_t* counts, int32_t B, int64_t N, int32_t T, int32_t F, int32_t class_id,
                                  const int32_t* group_counts, int32_t G, int32_t mode, int32_t K, int32_t M, int32_t* topk_idx, float* topk_score,
                                  int32_t* path_idx, float* path_score, float* path_weight, float* probs /* [B] or NULL */);
/* the same rule on the host cores over a host score matrix path_scores [N,C] (no handle, no GPU): pair b owns the rows offsets[b] .. offsets[b+1]-1
 * (1..4096 each), class_id is 1-based, reducer / K_reducer as kprn_config's reducer / K; the other arguments as kprn_explain_batch's.  A pair of more
 * than 28 paths sums its exponentials in the order the wave kernel does.                                                                     */
int kprn_host_explain(const float* path_scores, const int32_t* offsets /* [B+1] */, int32_t B, int32_t C, int32_t class_id, int32_t reducer,
                      int32_t K_reducer, const int32_t* pairs, int32_t n_pairs, int32_t M, int32_t* path_idx, float* path_score, float* path_weight,
                      float* pooled, float* probs);

/* ---- pooling temperature (an extension of module/LogSumExp.lua: the gamma of the paper's weighted pooling layer, g = log sum_k exp(s_k / gamma)) ----
 * kprn_set_option(h, "pool_gamma", "<decimal>") on a handle whose reducer is 2 (LogSumExp); default "1", the reference's layer.  A small gamma moves the
 * layer towards max pooling, a large one towards mean pooling (plus log cnt), and it decides how peaked the shares are that an explanation reports.
 * ig = (float)(1.0 / (double)gamma) is formed once on the host and handed to every kernel.  For a pair with the fp32 scores s_0 .. s_{cnt-1} in the
 * selected class, m their maximum:
 *  1. t_q = (s_q - m) * ig;  sum = sum_q expf(t_q), in the order the thread / wave form adds without the option;  pooled = logf(sum) + m * ig, with m * ig
 *     rounded on its own (no fused multiply-add);  prob = sigmoid(pooled).  No factor gamma stands outside the logarithm: the paper's form.
 *  2. At ig == 1.0f every product above is exact and expf / logf are the library's: the results are bit for bit those of a handle that never saw the
 *     option.  At any other ig the exponential and the logarithm above (and the sigmoid's) are the engine's own plain-fp32 functions (csrc/reduce_dev.h
 *     exp_shared / log_shared, about 1 and 2 units in the last place), the same code in the kernels and in kprn_host_explain_gamma -- which is why that
 *     call returns the kernels' bits, where two libraries' expf would differ in the last places.
 *  3. Backward: d loss / d s_q = expf(t_q) / sum * (dy * ig), dy = d loss / d pooled scaled once per pair -- under "loss" "bce" (both forms of the
 *     criterion's gradient) and "bpr" alike.
 *  4. Explanation: path_weight_q = expf(t_q) / sum, the path's NORMALISED SHARE; the shares of a pair add up to 1.  It is not d pooled / d s_q, which is
 *     the share times ig and adds up to 1 / gamma.  Order, tie rule, path_score (the raw s_q), pooled and prob are as above.
 *  5. Max and TopK + Mean are unchanged and never see ig.
 * A scoring pass that rides in a training launch ("score_dual") pools under the value of that training call.  kprn_save writes gamma's float bits into
 * header word 14 when gamma != 1 and 0 otherwise (the files of before, byte for byte); kprn_load on a reducer-2 handle adopts a non-zero word 14 as the
 * handle's "pool_gamma", a zero word leaves the option alone.  The Torch7 container carries no gamma.
 * kprn_host_explain_gamma: kprn_host_explain under a temperature -- the bit-exact host statement of 1 and 4 -- with that call's refusals and the option's:
 * gamma not finite or outside [1e-3, 1e3] is KPRN_E_ARG, gamma != 1 with reducer 0 or 1 KPRN_E_UNSUPPORTED; a refused call writes nothing.
 * kprn_host_explain is this call at gamma = 1.                                                                                               */
int kprn_host_explain_gamma(const float* path_scores, const int32_t* offsets /* [B+1] */, int32_t B, int32_t C, int32_t class_id, int32_t reducer,
                            int32_t K_reducer, const int32_t* pairs, int32_t n_pairs, int32_t M, int32_t* path_idx, float* path_score,
                            float* path_weight, float* pooled, float* probs, float gamma);

/* ---- finding a pair's paths (an extension: the reference mines paths offline, data_prepare/path_find_depth_3.py, by random walks) ----
 * From a knowledge graph to a ragged batch on the device: the graph lives in HBM as CSR, and kprn_find_paths enumerates -- exhaustively and
 * deterministically, no sampling -- every path between B (user, item) pairs and lays the kept ones out as the rows of a ragged kprn_batch, which is
 * accepted wherever a ragged batch is (scoring, kprn_explain_batch, board puts and ranking, training).
 *  - vocabulary: nodes are the entity ids 1 .. Ve-1 (Ve is the pad row), relations 1 .. Vr, type ids 1 .. Vt, all the handle's.
 *  - graph: directed edges (src[e], rel[e], dst[e]), e < E <= 2^31 - 1, in any order; the caller supplies inverse edges itself (rate / _rate, ...).  The build
 *    sorts them by (src, dst, rel) and drops exact duplicates and self-loops.  node_types [Ve][num_types]: row e - 1 = the type-slot ids of entity e exactly as
 *    the formatter prints them for a step (slots already padded with the type table's pad id); the pad entity's row (the last) is ignored.  end_relation: the
 *    id of #END_RELATION.  An id outside its vocabulary is KPRN_E_INDEX and leaves no graph behind.
 *  - path of h hops: u = n0 -> n1 -> ... -> nh = i, every (n_k, r_k, n_k+1) an edge, all nodes pairwise distinct (the miner's `mid_node not in path_set`);
 *    u == i has no paths; two relations between the same two nodes give two paths.  1 <= min_hops <= max_hops <= 3: three hops is the reference's "depth 3"
 *    (user-item-user-item).  Four and five hops need sampling to stay bounded: kprn_find_paths refuses max_hops > 3 with KPRN_E_ARG, and
 *    kprn_find_paths_sampled ("sampled paths of four and five hops" below) appends them.  min_hops = 2 keeps the direct u-i edge out of a positive pair's paths.
 *  - order within a pair (canonical): hops ascending, then the integer sequence (n1, r0, n2, r1, ..., r_{h-1}) ascending lexicographically.
 *  - cap: found[b] = the number of paths that exist; the kept ones are the first counts[b] = min(found[b], max_paths) in that order, 1 <= max_paths <= 4096.
 *    Nothing depends on timing: ranks come from a counting pass and prefix sums, never from an atomic counter.
 *  - cap mode (kprn_set_option "path_cap" = "first" (default) | "spread"; any other value is KPRN_E_ARG).  "first" is the rule above.  "spread" keeps a
 *    stratified random subset of the pair's whole sequence -- hops 1, 2, 3 in canonical order, then the sampled hops 4 and 5 in walk order -- instead of its
 *    beginning, which holds only the paths through the user's lowest-id first edges.  It is read by every device find call that carries (seed, draw):
 *    kprn_find_paths_sampled, kprn_find_training_paths, kprn_find_training_paths_sampled, kprn_find_paths_of_candidates.  kprn_find_paths has no seed: it always
 *    keeps the first paths.  For the pair in row b of the call's pair list, F = found[b], K = max_paths:
 *      F <= K: every path is kept, exactly as under "first".
 *      F > K:  the ranks [0, F) are cut into K strata, lo_j = floor(j F / K), j = 0 .. K: stratum j = [lo_j, lo_{j+1}) is never empty and the sizes differ by
 *              at most one; the stratum of rank r is floor(((r + 1) K - 1) / F).  One rank is kept in each: r_j = lo_j + mulhi64(x_j, lo_{j+1} - lo_j) (the high
 *              half of the 128-bit product), x_j = (w[2 (j % 2)] << 32) | w[2 (j % 2) + 1], w = Philox4x32-10(counter = (j / 2, 131072, b, draw), key =
 *              (seed & 0xffffffff, seed >> 32)).  131072 keeps these counters apart from the negative sampler's (a / 4, n <= 255, b, draw) and the walks'
 *              (w, 65536 + h, b, draw) under the same seed and draw.  The counter holds the ROW b, not the ids: the same pair in two rows draws two subsets.
 *      Kept row j of the pair is the path of rank r_j, so the kept rows stay in the sequence's order.  counts[b] = min(F, K) and found[b] are what they are
 *      under "first"; the ragged plan, the labels and the compaction do not change.  A path in a stratum of size s is kept with probability 1 / s, s in
 *      {floor(F / K), ceil(F / K)}: hop counts and first edges are represented in proportion to their share of the sequence.  Nothing depends on timing, and no
 *      atomic hands out a slot or a rank.  All products stay in 64 bits while F < 2^51; a pair beyond that under "spread" is refused on the host after the
 *      counting pass (KPRN_E_ARG).
 *  - row of a kept path, [T][F], T >= max_hops + 1, as pathformat.py lays it out: T - (h + 1) steps of left padding (Vt x num_types, Ve, Vr), then step k < h =
 *    (node_types[n_k], n_k, r_k) and the last step (node_types[i], i, end_relation).  Where F > num_types + 2 the leading columns, which no kernel reads and
 *    the id validation does not look at, are written as Vt.
 *  - result: counts [B] (zeros allowed) and found [B] on the host (either may be NULL); *out = a ragged batch of the B' pairs with counts > 0 in input order,
 *    labels [B] (or NULL) compacted the same way; B' == 0: *out = NULL with KPRN_OK.  Synchronous.  A pair's node outside 1 .. Ve-1 is KPRN_E_INDEX.  If the
 *    fill pass places another number of rows than the counting pass allotted a pair, the call returns KPRN_E_DEVICE and no batch; no write leaves the
 *    pair's rows in either case.                                                                                                                    */
int kprn_graph_create(kprn_handle* h, const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types /* [Ve][num_types] */,
                      int32_t end_relation, kprn_graph** out);
/* kprn_destroy frees the graphs still alive */
void kprn_graph_destroy(kprn_handle* h, kprn_graph* g);
/* edges the graph stores: E less the duplicates and self-loops */
int kprn_graph_num_edges(kprn_handle* h, const kprn_graph* g, int64_t* n);
int kprn_find_paths(kprn_handle* h, const kprn_graph* g, const int32_t* pairs /* [B][2] = (u, i) */, const float* labels /* [B] or NULL */, int32_t B,
                    int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, int32_t* counts /* [B] */, int64_t* found /* [B] */, kprn_batch** out);
/* a batch's ids [N][T][F] in the caller's path order, back on the host (to print the paths an explanation names); any batch, rectangular ([B*P][T][F]) or ragged */
int kprn_batch_read_idx(kprn_handle* h, const kprn_batch* b, int32_t* idx_out);
/* the same rule on the host cores over the graph's raw arrays (no handle, no GPU), on `threads` threads: counts [B], found [B] (or NULL), and idx = the
 * [sum(counts)][T][F] rows of the pairs with counts > 0 in input order -- the ids kprn_batch_read_idx returns for kprn_find_paths' batch.  idx == NULL: it only
 * counts (call it once for the sizes, once for the rows).  The refusals are kprn_graph_create's and kprn_find_paths'; F < num_types + 2 is KPRN_E_ARG.    */
int kprn_host_find_paths(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr, int32_t Vt,
                         int32_t num_types, int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths,
                         int32_t T, int32_t F, int32_t threads, int32_t* counts, int64_t* found, int32_t* idx);

/* ---- updating a graph in place (an extension: the reference rebuilds its pickled dictionaries from the rating file for every change) ----
 * A recommender's graph never stands still: an interaction is a new rate / _rate edge, a withdrawn item a set of removed ones.  kprn_graph_update edits a
 * stored graph by merging a sorted delta into the sorted CSR -- one streaming pass over the E stored edges instead of the build's sorts over them.
 *  - result: with S = the edges g stores, D = the stored edges the removals name and A = the additions less self-loops, duplicates collapsed, g stores
 *    afterwards exactly what kprn_graph_create stores for the edge set (S \ D) u A: rowptr, col, rel (kprn_graph_read) and kprn_graph_num_edges are the same
 *    bits as a fresh build's, and so is the answer of every find, candidates and sampler call on g.
 *  - order inside one call: removals first, then additions.  An edge named in both is stored afterwards.
 *  - removals (del_src[k], del_dst[k], del_rel[k]), k < n_del: del_rel in 1 .. Vr names that one edge; del_rel == 0 names every stored edge
 *    del_src -> del_dst, whatever its relation.  Removing an edge that is not stored is a no-op; a removal may be listed twice.
 *  - additions (add_src[k], add_dst[k], add_rel[k]), k < n_add, in any order: adding a stored edge is a no-op, self-loops are dropped as the build drops them.
 *  - counts (either may be NULL): *n_added = the edges of A that are not in S \ D, *n_removed = the edges of S in D.  E_new = E + n_added - n_removed always
 *    holds: an edge that is removed and added again counts in both.
 *  - limits: n_add = n_del = 0 is KPRN_OK and changes nothing; an empty graph may be added to; every edge may be removed (E = 0).
 *  - refusals, made on the host before anything is queued; a refused call leaves the graph untouched, bit for bit: g not a graph of h, n_add or n_del
 *    outside 0 .. 2^31 - 1, a NULL array with a positive count: KPRN_E_ARG; a node outside 1 .. Ve-1, an added relation outside 1 .. Vr, a removed relation
 *    outside 0 .. Vr: KPRN_E_INDEX.  E_new > 2^31 - 1 is KPRN_E_ARG: it is known after the counting pass, before any array of g is written or replaced.  If
 *    the merge places another number of edges than the counting pass found, or any of them outside [0, E_new), the call is KPRN_E_DEVICE and the old
 *    arrays stay in place.  Nothing depends on timing: every edge's place is a rank from two prefix sums, never an atomic counter.
 *  - what survives: the pattern set of kprn_graph_set_patterns (its table depends on Vr only), the node types, end_relation.  Batches and candidate lists
 *    found earlier are copies and stay valid.
 *  - synchronisation: synchronous.  The call waits for everything queued on the handle's streams before it swaps the arrays, and frees the old ones
 *    afterwards.  It needs device memory for the new col / rel beside the old ones, 5 E bytes of temporaries and the delta's sort.                          */
int kprn_graph_update(kprn_handle* h, kprn_graph* g, const int32_t* add_src, const int32_t* add_dst, const int32_t* add_rel, int64_t n_add,
                      const int32_t* del_src, const int32_t* del_dst, const int32_t* del_rel, int64_t n_del, int64_t* n_added, int64_t* n_removed);
/* the CSR as stored, back on the host: rowptr [Ve + 1] by 1-based node id (the edges of node n are rowptr[n] .. rowptr[n + 1] - 1; node 0 has none), col [E]
 * the destinations and rel [E] the relations, E = kprn_graph_num_edges (col and rel may be NULL when E == 0).  It is what makes the equality above testable,
 * and how a caller checkpoints an updated graph: (the source of each row, col, rel) given to kprn_graph_create builds the same graph.  Synchronous.       */
int kprn_graph_read(kprn_handle* h, const kprn_graph* g, int32_t* rowptr /* [Ve + 1] */, int32_t* col /* [E] */, int32_t* rel /* [E] */);
/* replaces the type rows of n entities -- a node that first appears in a delta still has the row the graph was created with: rows [k] = the num_types slot
 * ids of entities [k], as kprn_graph_create's node_types holds them.  A plain row copy on the handle's stream, behind the calls queued before it;
 * synchronous.  An entity outside 1 .. Ve-1 or a type id outside 1 .. Vt is KPRN_E_INDEX, an entity listed twice or n outside 0 .. Ve-1 KPRN_E_ARG; a
 * refused call writes nothing.                                                                                                                          */
int kprn_graph_set_node_types(kprn_handle* h, kprn_graph* g, const int32_t* entities /* [n] */, const int32_t* rows /* [n][num_types] */, int64_t n);
/* the same rule on the host over raw arrays (no handle, no GPU): (src, dst, rel) [E] is an edge list in any order, as kprn_graph_create takes it; the result
 * is the CSR of the updated graph: rowptr [Ve + 1], col and rel_out with room for E + n_add entries of which *E_out are written, and the two counts (either
 * may be NULL), which are taken against the stored set S -- the list less duplicates and self-loops.  The refusals are kprn_graph_update's, plus
 * kprn_graph_create's for E, Ve, Vr and the edges' ids and KPRN_E_ARG for a NULL rowptr, col, rel_out or E_out; a refused call writes no output.          */
int kprn_host_graph_update(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, int32_t Vr, const int32_t* add_src,
                           const int32_t* add_dst, const int32_t* add_rel, int64_t n_add, const int32_t* del_src, const int32_t* del_dst, const int32_t* del_rel,
                           int64_t n_del, int32_t* rowptr, int32_t* col, int32_t* rel_out, int64_t* E_out, int64_t* n_added, int64_t* n_removed);

/* ---- sampled paths of four and five hops (an extension: the reference extends a three-hop path twice, data_prepare/path_find_depth_5.py, by sampling a few
 * neighbours of the last item and one random item behind each; its draws, Python's random, cannot be reproduced and are not restated) ----
 * The *_sampled calls accept 1 <= min_hops <= max_hops <= 5.  Hops 1..3 stay exhaustive, exactly as above.  Hops h in {4, 5} are sampled: a random prefix of
 * h - 2 hops out of the user, then an exhaustive close of the last two hops into the item (a prefix that had to hit i in one hop would almost never close).
 * For the pair in row b of the call's pair list, (u, i) with u != i and i != 0, and each asked h in {4, 5}, walks w = 0 .. walks-1:
 *  - words: r[0..3] = Philox4x32-10(counter = (w, 65536 + h, b, draw), key = (seed & 0xffffffff, seed >> 32)).  65536 + h keeps the counters apart from the
 *    negative sampler's (a / 4, n, b, draw), n <= 255, under the same seed and draw.  The counter holds the ROW b, not the user id: the same pair in two rows
 *    draws different walks.
 *  - prefix: n_0 = u; for k = 0 .. h-3: deg = rowptr[n_k + 1] - rowptr[n_k] (the node's stored edges, in the graph's (dst, rel) order); deg == 0: the walk is dead;
 *    else e_k = rowptr[n_k] + mulhi32(r[k], deg) (the high word of the 64-bit product), n_{k+1} = the edge's destination, r_k its relation: uniform over stored
 *    edges, so a multi-edge counts once per relation.  If n_{k+1} equals i or any of n_0 .. n_k the walk is dead.  No retries.
 *  - duplicates: walk w is dropped if a walk w' < w of the same h has the same edge sequence (e_0 .. e_{h-3}).  Stored edges are distinct, so equal edge
 *    sequences are equal prefixes, and distinct prefixes give distinct paths: no path is found twice.
 *  - paths of a live walk: every (e, c), e an edge n_{h-2} -> m with m not in {u, n_1, .., n_{h-2}, i}, c an edge m -> i; order: e ascending, then c ascending
 *    (adjacency order, then the closing multi-edges by relation).
 *  - order within a pair: hops ascending -- 1, 2, 3 in the canonical order above, then 4, then 5; inside a sampled hop count the walk index ascending, then
 *    the order above.  Walk order, not lexicographic order: the cap keeps an unbiased prefix of the sample, not the lowest ids.
 *  - found[b] = (the paths of hops <= 3 that exist) + (the distinct sampled paths of hops 4 and 5): for h > 3 found counts what was SAMPLED, not what
 *    exists.  counts[b] = min(found[b], max_paths).
 *  - limits: walks in 1..256 when max_hops > 3 (else KPRN_E_ARG); when max_hops <= 3, walks is ignored (it may be 0), and under "path_cap" "first" so are seed
 *    and draw: the call returns exactly what the unsampled call returns.  Under "spread" seed and draw address the cap's draws at every hop count.  T >= max_hops + 1.  Everything else -- row layout, padding, leading columns, compaction of the pairs without
 *    paths, labels, refusals, the KPRN_E_DEVICE check of the fill pass -- is kprn_find_paths'.  Nothing depends on timing: no atomic hands out a slot or a rank. */
int kprn_find_paths_sampled(kprn_handle* h, const kprn_graph* g, const int32_t* pairs /* [B][2] = (u, i) */, const float* labels /* [B] or NULL */, int32_t B,
                            int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, int32_t walks, uint64_t seed, unsigned int draw /* uint32 */,
                            int32_t* counts /* [B] */, int64_t* found /* [B] */, kprn_batch** out);
/* the same rule on the host cores (no handle, no GPU); the other arguments and the refusals as kprn_host_find_paths' */
int kprn_host_find_paths_sampled(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr,
                                 int32_t Vt, int32_t num_types, int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops,
                                 int32_t max_paths, int32_t T, int32_t F, int32_t walks, uint64_t seed, unsigned int draw, int32_t threads, int32_t* counts,
                                 int64_t* found, int32_t* idx);
/* kprn_host_find_paths_sampled with the cap mode: cap_mode 0 = "first" (exactly kprn_host_find_paths_sampled), 1 = "spread"; anything else is KPRN_E_ARG */
int kprn_host_find_paths_cap(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr, int32_t Vt,
                             int32_t num_types, int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops, int32_t max_paths,
                             int32_t T, int32_t F, int32_t walks, uint64_t seed, unsigned int draw, int32_t cap_mode, int32_t threads, int32_t* counts,
                             int64_t* found, int32_t* idx);
/* the ranks "spread" keeps of a pair in row b with `found` paths, ascending: ranks [min(found, max_paths)] (found <= max_paths: 0, 1, ..).  Host-only; it exists
 * so that a selection can be rebuilt anywhere.  found outside 0 .. 2^51 - 1, max_paths outside 1..4096 or b < 0 is KPRN_E_ARG.                              */
int kprn_host_cap_select(int64_t found, int32_t max_paths, int32_t b, uint64_t seed, unsigned int draw, int64_t* ranks /* [min(found, max_paths)] */);

/* ---- meta-paths (the reference's miners extend a path only along named schemas -- item-person-item, item-type-item, item-user-item, each with a budget
 * where 0 switches it off, data_prepare/path_find_depth_3.py and path_find_depth_5.py; here: keep only the paths whose relation sequence matches a pattern) ----
 * A graph may carry a pattern set of n patterns, 0 <= n <= KPRN_PATTERN_MAX.
 *  - pattern p has hops[p] in 1..5 positions; position k is a set of relation ids S[p][k], a subset of 1 .. Vr; an empty set means "any relation".
 *  - a path with relations (r_0 .. r_{h-1}) MATCHES iff some p has hops[p] == h and r_k in S[p][k] (or S[p][k] empty) for every k.  A path that matches several
 *    patterns is still one path.
 *  - n == 0 is the default and means no filter: every call then behaves exactly as described elsewhere in this header, in its results and in the kernels it
 *    launches.
 *  - n >= 1: every device call that takes the graph works on the FILTERED SEQUENCE of a pair = the pair's sequence as defined above (hops 1, 2, 3 in
 *    canonical order, then the sampled hops 4 and 5 in walk order) with the non-matching paths removed and the order kept.  found[b] is its length, counts[b] =
 *    min(found[b], max_paths), "first" keeps its first rows, "spread" draws its strata over F = the filtered found with the same Philox counters.  Ranks, row
 *    layout, compaction of the pairs without paths, labels and the KPRN_E_DEVICE check of the fill passes stay as they are.  An asked hop count that no
 *    pattern has yields no paths; a pattern whose hop count the call does not ask for is inert.
 *  - sampled hops: the walks are drawn exactly as without patterns -- words, the dead rule, the duplicate rule, no retries; whether a walk is live does not
 *    depend on the patterns.  The paths of a live walk are those of its (e, c) closes that match; the per-walk counts count matching paths only.  (A walk
 *    whose prefix no pattern admits has no matching close; an implementation may skip it.)
 *  - candidates: membership and n_paths count matching paths only, so "the candidates are exactly the members for which the finder would report found > 0"
 *    and "n_paths equals found" hold with a pattern set.  exclude_adjacent, the user's own entry and the negative sampler's adjacency test keep looking at
 *    stored edges of any relation.
 *  - kprn_find_paths_of_candidates, kprn_find_training_paths and kprn_find_training_paths_sampled inherit all of this through the finder's two passes.
 *    Changing the patterns between making a candidate list and finding its paths is allowed; pairs that end up with 0 paths are dropped, as everywhere.
 * The set is given with its positions numbered consecutively over the patterns: S = sum(hops); position s allows set_rels[set_offsets[s] ..
 * set_offsets[s + 1]) (empty = any relation).  n == 0 (the arrays may be NULL) clears the set.  Repeated relations in a set and repeated patterns are fine.
 * Refusals are decided on the host before anything is written, and a refused call leaves the previous set in place: n outside 0..32, a hop count outside
 * 1..5, offsets not ascending from 0, NULL arrays with n > 0: KPRN_E_ARG; a relation outside 1 .. Vr: KPRN_E_INDEX.  The table the kernels read -- bit p of
 * word [k][r] = position k of pattern p admits r, 5 (Vr + 1) words in HBM, owned by the graph -- is uploaded on the handle's stream; the call is synchronous. */
#define KPRN_PATTERN_MAX 32
int kprn_graph_set_patterns(kprn_handle* h, kprn_graph* g, const int32_t* hops /* [n] */, const int64_t* set_offsets /* [S + 1] */, const int32_t* set_rels,
                            int32_t n);
int kprn_graph_num_patterns(kprn_handle* h, const kprn_graph* g, int32_t* n);
/* the host twins (no handle, no GPU).  kprn_host_find_paths_patterns: the arguments of kprn_host_find_paths_cap, then the four pattern arguments.
 * kprn_host_find_candidates_patterns: the arguments of kprn_host_find_candidates_top (below), then the same four; a cap of 2^31 - 1 gives the plain candidates.
 * With n == 0 each returns exactly what the older twin returns.  The refusals of a set are those above; the candidates twin, which takes no Vr, refuses a
 * relation below 1 (KPRN_E_INDEX) and lets the table reach the largest relation the edges or the sets name.                                           */
int kprn_host_find_paths_patterns(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, const int32_t* node_types, int32_t Ve, int32_t Vr,
                                  int32_t Vt, int32_t num_types, int32_t end_relation, const int32_t* pairs, int32_t B, int32_t min_hops, int32_t max_hops,
                                  int32_t max_paths, int32_t T, int32_t F, int32_t walks, uint64_t seed, unsigned int draw, int32_t cap_mode, int32_t threads,
                                  int32_t* counts, int64_t* found, int32_t* idx, const int32_t* hops, const int64_t* set_offsets, const int32_t* set_rels,
                                  int32_t n);
int kprn_host_find_candidates_patterns(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, int64_t M,
                                       const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t cap,
                                       int32_t threads, int32_t* group_counts, int32_t* cand, int64_t* n_paths, const int32_t* hops,
                                       const int64_t* set_offsets, const int32_t* set_rels, int32_t n);

/* ---- sampling negatives (an extension: the reference draws them offline, data_prepare/sample.py:18-26,101-117 -- distinct non-interacted items, uniform at
 * alpha = 0, else weighted by frequency^alpha; its draws, numpy.random.multinomial and Python's random, cannot be reproduced and are not restated) ----
 * For B user slots, n_neg items per slot from a weighted candidate list, on the device and fully specified, so that any id can be rebuilt anywhere:
 *  - candidate list: items [M], entity ids in 1 .. Ve-1, strictly ascending, 1 <= M < 2^31; weights [M] fp32, finite and >= 0, NULL = all 1; at least one
 *    weight > 0.  Anything else is KPRN_E_ARG (KPRN_E_INDEX for an id outside the table), decided on the host before anything is allocated.
 *  - thresholds, built on the host in double in index order: cum_j = cum_{j-1} + (double)w_j, thr[j] = (uint64) floor(cum_j / cum_{M-1} * 4294967296.0), hence
 *    thr[M-1] = 2^32.  pick(r) of a 32-bit word r = the number of j with thr[j] <= r (an upper bound by binary search); an item of weight 0 is never picked.
 *  - words: Philox4x32-10 (the generator of the dropout rule above), key = (seed & 0xffffffff, seed >> 32), counter = (a / 4, n, b, draw); word a % 4 of that
 *    call belongs to attempt a of negative n of user slot b.  The counter holds the SLOT b, not the user id: the same user in two slots draws different items.
 *  - acceptance: for slot b, u = users[b], the negatives are settled in the order n = 0 .. n_neg-1.  Negative n = items[pick(word)] of its first attempt
 *    a < max_attempts whose candidate c satisfies all of: c != u; the stored graph has no edge u -> c of any relation; c is not one of the negatives already
 *    accepted for this slot.  No attempt qualifies: slot n is 0, and the later n still try.
 *  - limits: n_neg in 1..256, max_attempts in 1..64 (else KPRN_E_ARG); n_found[b] = the slot's non-zero entries.
 * A positive item is adjacent to its user, so it is never drawn as that user's negative.  Nothing depends on timing: no atomic hands out a slot.
 * A sampler is independent of any graph (the graph is an argument of the sampling calls); kprn_destroy frees the samplers still alive.                   */
int kprn_sampler_create(kprn_handle* h, const int32_t* items, const float* weights /* [M] or NULL */, int64_t M, kprn_sampler** out);
void kprn_sampler_destroy(kprn_handle* h, kprn_sampler* s);
/* neg: host [B][n_neg]; n_found: host [B] or NULL.  Synchronous.  A user outside 1 .. Ve-1 is KPRN_E_INDEX, bad limits KPRN_E_ARG; a refused call writes nothing. */
int kprn_sample_negatives(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s, const int32_t* users /* [B] */, int32_t B, int32_t n_neg,
                          int32_t max_attempts, uint64_t seed, unsigned int draw /* uint32 */, int32_t* neg, int32_t* n_found);
/* the same rule on the host cores over the graph's raw edge arrays (no handle, no GPU), on `threads` threads; rel is not looked at (an edge of any relation
 * counts).  The same refusals, plus kprn_graph_create's for E and the edges' nodes.                                                                        */
int kprn_host_sample_negatives(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, const float* weights,
                               int64_t M, const int32_t* users, int32_t B, int32_t n_neg, int32_t max_attempts, uint64_t seed, unsigned int draw,
                               int32_t threads, int32_t* neg, int32_t* n_found);
/* A training minibatch from B positives in one call: every positive's n_neg negatives are sampled on the device with slot b = the positive's index, the
 * sampling kernel writes the pair list where the finder reads it -- row b * (1 + n_neg) = (u, i) with label 1, then (u, negative k) with label 0, k = 0 ..
 * n_neg-1 -- and the finder's count and fill passes run over that list; the list never visits the host on the way.  The call waits where kprn_find_paths
 * waits (for the counts, for the finished batch); sampling adds no wait.  An empty negative slot (item 0) is a pair of 0 paths, not an error; pairs without
 * paths are dropped and the labels compacted exactly as kprn_find_paths does.  pairs_out (host [B * (1 + n_neg)][2], or NULL), counts and found
 * [B * (1 + n_neg)] (or NULL) and the batch -- ids, counts, labels -- equal those of kprn_sample_negatives followed by kprn_find_paths on the same pair list
 * and labels, the rows of item 0 left out of that call and counted as 0 paths.  A node of pos outside 1 .. Ve-1 is KPRN_E_INDEX; the limits are the two
 * calls'; B * (1 + n_neg) must stay below 2^31.  No pair has a path: *out = NULL with KPRN_OK.  Under "path_cap" "spread" the seed and draw address the
 * cap's draws too, and the equality holds with kprn_find_paths_sampled (walks 0) in kprn_find_paths' place.                                             */
int kprn_find_training_paths(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s, const int32_t* pos /* [B][2] = (u, i) */, int32_t B, int32_t n_neg,
                             int32_t max_attempts, uint64_t seed, unsigned int draw /* uint32 */, int32_t min_hops, int32_t max_hops, int32_t max_paths,
                             int32_t T, int32_t* pairs_out, int32_t* counts, int64_t* found, kprn_batch** out);

/* kprn_find_training_paths with the sampled hops: one seed / draw serves the negatives and the walks, and a walk's row b is the pair-list row
 * b * (1 + n_neg) + k.  By definition the outputs equal kprn_sample_negatives followed by kprn_find_paths_sampled on the same pair list, the rows of item 0
 * counted as 0 paths.  max_hops <= 3: exactly kprn_find_training_paths.                                                                               */
int kprn_find_training_paths_sampled(kprn_handle* h, const kprn_graph* g, const kprn_sampler* s, const int32_t* pos /* [B][2] = (u, i) */, int32_t B,
                                     int32_t n_neg, int32_t max_attempts, uint64_t seed, unsigned int draw /* uint32 */, int32_t min_hops, int32_t max_hops,
                                     int32_t max_paths, int32_t T, int32_t walks, int32_t* pairs_out, int32_t* counts, int64_t* found, kprn_batch** out);

/* ---- candidates of a user (an extension: the reference takes its candidates from files of 100 sampled negatives per user, data_prepare/sample.py; here
 * the candidates are the catalogue items the graph reaches from the user, and "sampled evaluation groups" below draws such negatives from them) ----
 * "What should this user get" without a candidate list from the caller: the walk runs from the user outward on the device, deg(u) * deg(a) * deg(b) steps,
 * and leaves the (user, item) rows in HBM, where the finder reads them.
 *  - catalogue: the item list of a kprn_sampler, items [M], ascending entity ids.  Its weights are not looked at: an item of weight 0 is still a member.
 *    (The sampler already holds exactly this list in HBM; training from a graph and recommending can share one object.)
 *  - candidates of a user u (a node, 1 .. Ve-1), for 1 <= min_hops <= max_hops <= 3: a catalogue member c is a candidate iff c != u; at least one path of
 *    min_hops .. max_hops hops leads from u to c in the finder's sense (stored edges only, all nodes pairwise distinct); and, if exclude_adjacent != 0, the
 *    stored graph has no edge u -> c of any relation (the items the user already has, by the negative sampler's own test).  Stored edges hold no
 *    self-loops, so the path condition is: 1 hop u -> c; 2 hops u -> a -> c with c != u; 3 hops u -> a -> b -> c with b != u, c != u, c != a.
 *    By definition the candidates are exactly the members for which kprn_find_paths over the same hops would report found > 0, less the exclusions.
 *  - order within a user: entity id ascending.  Nothing depends on timing: membership is a bitmap (a set), ranks come from popcounts and prefix sums, and
 *    no atomic hands out a slot or a rank.
 *  - result: B users in one call give B groups; group_counts [B] (zeros allowed) and *total = sum(group_counts) on the host.  The pair list,
 *    [total][2] = (u, c), users in input order, stays in HBM as THE HANDLE'S CANDIDATE LIST: it is replaced by the next successful call, freed by
 *    kprn_destroy, and read by kprn_read_candidates and kprn_find_paths_of_candidates.
 *  - refusals: hops outside 1..3, B < 1, B * ceil(M / 32) >= 2^31 or total >= 2^31 are KPRN_E_ARG; a user outside 1 .. Ve-1 is KPRN_E_INDEX.  A refused
 *    call writes nothing and leaves the handle's previous list as it was.  If the fill pass places another number of rows than the counting pass allotted
 *    a user, the call returns KPRN_E_DEVICE (no write leaves the user's rows in either case) and the previous list stays.
 * Synchronous: the call waits once for the counts (the list's size) and once for the fill pass's verdict.                                             */
int kprn_find_candidates(kprn_handle* h, const kprn_graph* g, const kprn_sampler* catalogue, const int32_t* users /* [B] */, int32_t B,
                         int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t* group_counts /* [B] */, int64_t* total);
/* the handle's candidate list back on the host; total must equal the list's, else KPRN_E_ARG (as is a handle that has no list yet) */
int kprn_read_candidates(kprn_handle* h, int32_t* pairs_out /* [total][2] */, int64_t total);
/* The finder's two passes over the handle's candidate list, copied device to device: the list never visits the host on the way.  labels = NULL; counts and
 * found [total] (or NULL); row b of the sampled walks' Philox counter is the list's row b.  walks == 0: the limits are kprn_find_paths'; otherwise
 * kprn_find_paths_sampled's (max_hops up to 5).  By definition the outputs equal those of kprn_find_paths (kprn_find_paths_sampled) on the pair list
 * kprn_read_candidates returns.  No list yet: KPRN_E_ARG.  An empty list: *out = NULL with KPRN_OK.  A graph whose Ve differs from that of the graph the list
 * was made on: KPRN_E_INDEX.  When the call asks for the same exhaustive hops that produced the list, every pair has found > 0, no pair is dropped, and
 * the batch's pair p is the list's row p.  Under "path_cap" "spread" seed and draw are read at walks == 0 too, and the outputs equal
 * kprn_find_paths_sampled's on that list.                                                                                                           */
int kprn_find_paths_of_candidates(kprn_handle* h, const kprn_graph* g, int32_t min_hops, int32_t max_hops, int32_t max_paths, int32_t T, int32_t walks,
                                  uint64_t seed, unsigned int draw /* uint32 */, int32_t* counts /* [total] */, int64_t* found /* [total] */, kprn_batch** out);
/* the same rule on the host cores over the graph's raw edge arrays and the item list (no handle, no GPU), on `threads` threads; rel is not looked at.
 * group_counts [B]; cand = the [sum(group_counts)] candidate entity ids, users in input order, or NULL = counts only (call it once for the sizes, once
 * for the ids).  The same refusals, plus kprn_sampler_create's for the item list and kprn_graph_create's for E and the edges' nodes.                    */
int kprn_host_find_candidates(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, int64_t M,
                              const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t threads,
                              int32_t* group_counts, int32_t* cand /* [sum] entity ids, or NULL = counts only */);

/* ---- the N strongest candidates of a user (a retrieval stage in front of the ranker: in three hops a user reaches most of a catalogue) ----
 * Everything not said here is kprn_find_candidates'.
 *  - path count of a member: for a user u, 1 <= min_hops <= max_hops <= 3 and a catalogue member c, n_paths(u, c) is the number of paths of min_hops ..
 *    max_hops hops from u to c in the finder's sense: stored edges, all nodes pairwise distinct, two relations between the same two nodes counted as two
 *    paths.  An int64.  By definition it equals `found` of kprn_find_paths for the pair (u, c) over the same hops.
 *  - candidates: exactly kprn_find_candidates': the members with n_paths > 0, less u itself and, with exclude_adjacent, the members u has a stored edge to.
 *    An excluded member neither appears nor uses up any of the cap.
 *  - kept: the user's candidates ordered by (n_paths descending, entity id ascending); the first min(cap, number of candidates) are kept,
 *    1 <= cap <= 2^31 - 1.
 *  - order of the result: within a user the kept rows lie by entity id ascending, as the list always does, so kprn_find_paths_of_candidates and "the
 *    batch's pair p is the list's row p" hold unchanged.  With cap >= every user's number of candidates the call leaves exactly the list, group_counts and
 *    total that kprn_find_candidates leaves.
 *  - nothing depends on timing: the counts are integer sums (any order of the adds gives the same sum), the cut is found by counting (a radix select
 *    over histograms), ranks come from prefix sums, and no atomic hands out a slot, a rank or a tie-break.
 *  - result: the (u, c) rows become the handle's candidate list; beside it lies a device array n_paths [total], row for row, which
 *    kprn_read_candidate_paths copies back.  A list left by kprn_find_candidates has no counts: the read is KPRN_E_ARG, as is a wrong total.
 *  - refusals, all decided on the host before anything is allocated or written: kprn_find_candidates' own; cap < 1 and B * M >= 2^28 (the per-user
 *    counts are 8 bytes each: a block of at most 2 GiB) are KPRN_E_ARG.  A refused call leaves the previous list and its counts as they were.  The fill
 *    pass is checked as kprn_find_candidates' (KPRN_E_DEVICE, the previous list stays, no write leaves the user's own rows).
 * Synchronous, with the same two waits: the counts, then the fill pass's verdict.                                                                     */
int kprn_find_candidates_top(kprn_handle* h, const kprn_graph* g, const kprn_sampler* catalogue, const int32_t* users /* [B] */, int32_t B,
                             int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t cap,
                             int32_t* group_counts /* [B] */, int64_t* total);
int kprn_read_candidate_paths(kprn_handle* h, int64_t* n_paths_out /* [total] */, int64_t total);
/* the same rule on the host cores (no handle, no GPU): kprn_host_find_candidates' arguments and refusals plus the two above; n_paths [sum] or NULL */
int kprn_host_find_candidates_top(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t E, int32_t Ve, const int32_t* items, int64_t M,
                                  const int32_t* users, int32_t B, int32_t min_hops, int32_t max_hops, int32_t exclude_adjacent, int32_t cap, int32_t threads,
                                  int32_t* group_counts, int32_t* cand /* [sum] entity ids, or NULL = counts only */, int64_t* n_paths /* [sum] or NULL */);

/* ---- sampled evaluation groups (the reference's evaluation protocol: data_prepare/sample.py draws 100 negatives for every held positive from the user's
 * non-interacted items that have paths, eval/eval_score.py ranks each positive among its 101) ----
 * For every held pair of B users: its negatives drawn from the user's rows of the handle's candidate list, the list cut down to the rows some sample needs,
 * and the rows of every group in the new list -- on the device, the list never visits the host.
 *  - input: the handle's candidate list as kprn_find_candidates / _top left it: B users' groups of group_counts[b] consecutive rows (u, c), within a user by
 *    entity id ascending.  Targets: target_items[target_offsets[b] .. target_offsets[b + 1]) are user slot b's held items, entity ids, strictly ascending
 *    within a user; a user may have none; target_offsets[0] = 0 and NT = target_offsets[B] >= 1.
 *  - for user slot b with user id u: H = its target items; D = its rows whose item is not in H, d = |D|; a target i is REACHABLE iff i is the item of one
 *    of the user's rows.  An unreachable target draws nothing.
 *  - key(u, i, c) = ((uint64)w0 << 32) | (uint32)c, w0 = word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (c, i, u, draw).
 *    Keys of one sample are distinct because c is.  For a reachable target i: S(u, i) = D if d <= n_neg, else the n_neg rows of D with the smallest keys --
 *    an exactly uniform draw without replacement, with no attempt limit and no floating point.  The key is a function of ids only: a pair's sample does not
 *    depend on the user's slot, on how the users are cut into calls, or on the list's layout.  Targets of a user are never each other's negatives.
 *  - kept rows of a user: the rows of its reachable targets and the union of their S.  The new candidate list is the kept rows in the old order; it
 *    REPLACES the handle's list.  The companion n_paths array is dropped: kprn_read_candidate_paths is KPRN_E_ARG afterwards; kprn_read_candidates and
 *    kprn_find_paths_of_candidates work on the new list as on any other.
 *  - outputs, on the host: new_group_counts [B]; *new_total; target_rows [NT] = the target's row in the new list, -1 = unreachable; neg_rows [NT][n_neg] =
 *    the rows of S in the new list, ascending, padded with -1; n_drawn [NT] = |S|, 0 for an unreachable target.  [target_rows[k], neg_rows[k][0 .. n_drawn[k])]
 *    mapped to board lines is a group of kprn_rank_groups' `members` with pos 0.
 *  - nothing depends on timing: randomness enters only through the keys; membership is a bitmap (a set: set-only atomicOr), the cut is found by counting (a
 *    radix select over histograms), ranks come from prefix sums, and no atomic hands out a slot.
 *  - refusals, all decided on the host before anything is allocated or written: KPRN_E_ARG for no list, sum(group_counts) != the list's total, a negative
 *    count, B < 1, NT < 1, target_offsets[0] != 0 or decreasing, targets not strictly ascending within a user, n_neg outside 1 .. KPRN_RANK_MAX_GROUP - 1
 *    (4095), NT * (n_neg + 1) >= 2^31, a NULL argument; KPRN_E_INDEX for a target id outside 1..Ve-1 (the Ve of the graph the list was made on).  A refused
 *    call writes nothing and leaves the list and its path counts as they were.  The new list is written to a block of its own and swapped in only after the
 *    fill pass's row count agrees with the counting pass's: on a disagreement the call returns KPRN_E_DEVICE and the old list stays.
 *  - weighted draws (sample.py's alpha != 0, a multinomial whose stream cannot be reproduced) are not restated: the draw is uniform.
 * Synchronous: the call waits once for the counts (the new list's size) and once for the fill pass's verdict and the results.                          */
int kprn_sample_eval_groups(kprn_handle* h, const int32_t* group_counts /* [B] */, int32_t B, const int64_t* target_offsets /* [B+1] */,
                            const int32_t* target_items /* [NT] */, int32_t n_neg, uint64_t seed, unsigned int draw /* uint32 */,
                            int32_t* new_group_counts /* [B] */, int64_t* new_total, int32_t* target_rows /* [NT] */, int32_t* neg_rows /* [NT][n_neg] */,
                            int32_t* n_drawn /* [NT] */);
/* the same rule on the host cores (no handle, no GPU) over a host list [total][2] made on a graph of Ve entities: the same arguments and refusals (a NULL
 * list with total > 0 is KPRN_E_ARG), and the list's own shape is checked too -- an id outside 1..Ve-1 is KPRN_E_INDEX, a group of more than one user or
 * items not strictly ascending KPRN_E_ARG.  new_list [*new_total][2] (room for `total` rows always suffices), or NULL = everything but the rows.           */
int kprn_host_sample_eval_groups(const int32_t* list /* [total][2] */, int64_t total, int32_t Ve, const int32_t* group_counts, int32_t B,
                                 const int64_t* target_offsets, const int32_t* target_items, int32_t n_neg, uint64_t seed, unsigned int draw,
                                 int32_t* new_group_counts, int64_t* new_total, int32_t* target_rows, int32_t* neg_rows, int32_t* n_drawn,
                                 int32_t* new_list /* [new_total][2] or NULL */);

/* ---- training ---------------------------------------------------------------------- */
/* fEval of MyOptimizer.lua:184-195: zeroGradParameters; forward; BCE; backward.
 * inv_batch = 0 -> 1/B; data-parallel callers pass 1/B_global.  loss may be NULL (async). */
int kprn_backward_batch(kprn_handle* h, const kprn_batch* b, int32_t class_id, int32_t bce_literal,
                        float inv_batch, float* loss);
/* MyOptimizer.lua:196-219 on the gradients now in the handle: clip/L2 iff regularize==1,
 * optim step, zeroPadTokens.  Async.                                                     */
int kprn_apply_update(kprn_handle* h, const kprn_opt* opt);
/* MyOptimizer:trainBatch = zeroPadTokens + kprn_backward_batch + kprn_apply_update.
 * With loss != NULL the call returns as soon as the loss is on the host, i.e. after the forward and the loss stage of this step: the backward and
 * the optimiser step are queued and complete in stream order BEFORE anything a later call on this handle can observe (parameters, gradients,
 * scores, the next step) -- the caller's idx / labels have been consumed, and the caller prepares its next minibatch while the device finishes
 * this one (MyOptimizer.lua:184-221 returns the same number; it just cannot overlap).  A device error raised by the rest of the step surfaces at
 * the next call.  kprn_set_option(h, "train_step_return", "drain") restores the wait for the whole step; kprn_sync always waits for everything.
 * kprn_train_step (host buffers) waits for the loss stage whether or not `loss` is NULL -- that wait is what lets the next call upload its
 * minibatch beside this step's backward; kprn_train_step_batch with loss == NULL is fully asynchronous.                                      */
int kprn_train_step(kprn_handle* h, const int32_t* idx, int32_t B, int32_t P, int32_t T, int32_t F,
                    const float* labels, int32_t class_id, const kprn_opt* opt, float* loss);
int kprn_train_step_batch(kprn_handle* h, const kprn_batch* b, int32_t class_id, const kprn_opt* opt,
                          float* loss /* NULL = async */);
/* loss of the most recent backward, once the stream has drained */
int kprn_read_loss(kprn_handle* h, float* loss);
/* kprn_set_option(h, "loss_accumulate", "1"): every backward adds its loss to a running sum on the device; this reads the sum and
 * the number of steps in it (MyOptimizer.lua:148-156 prints totalError / steps every gradientStepCounter steps and per epoch), so
 * the training loop needs no host sync per step.  reset != 0 starts a new sum.                                          */
int kprn_read_loss_sum(kprn_handle* h, float* sum, int32_t* steps, int32_t reset);
int kprn_sync(kprn_handle* h);

/* ---- pairwise loss (an extension: Bayesian personalised ranking over groups of pairs, in place of nn.BCECriterion on each pair by itself) ----
 * kprn_set_option(h, "loss", "bpr") makes kprn_backward_batch and kprn_train_step_batch train on this rule; the batch needs a group table
 * (kprn_batch_set_groups).  For a batch of B pairs, rectangular or ragged:
 *   y_b = the reducer's fp32 output for the selected class (what the pooling stage calls pooled, before the sigmoid); t_b = the batch's labels;
 *   go[0 .. G] = a group table over consecutive pairs: go[0] = 0, go[G] = B, non-decreasing (an empty group is allowed).
 * Terms.  Group g contributes one term per ordered pair (i, j) of its members with t_i > 0.5 and t_j <= 0.5.  Positives need not come first and there may
 *   be several; a group without a positive, or without a negative, contributes nothing.  n_terms = the batch's term count.
 * Loss.  L = s * sum over the terms of softplus(-(y_i - y_j)), softplus(x) = max(x, 0) + log1p(exp(-|x|)): -log sigmoid(y_i - y_j) in its stable form.
 *   s = inv_batch where the caller passes inv_batch > 0, else 1 / n_terms.  (The reference's criterion/BPRLoss.lua adds 1e-4 inside its logarithm; that
 *   criterion belongs to the reference's entity-type task, which is out of scope here, and its gradient is not the derivative of its value: it is NOT
 *   restated.)
 * Gradient.  With sigma_ij = 1 / (1 + exp(y_i - y_j)): dy_i = -s * sum_j sigma_ij for a positive i, dy_j = +s * sum_i sigma_ij for a negative j, each sum
 *   over the member's partners in ascending pair index; a pair without a term gets dy = +0.0f.  dy_b goes back through the reducer (LogSumExp, Max,
 *   TopK + Mean) exactly as the BCE stage's does, and EVERY pair's entries of dS are written -- zeros for a pair without a term, never skipped.  The
 *   selected probabilities sigmoid(y_b) are stored as before (kprn_read_probs).
 * No terms.  n_terms == 0: the loss is 0, every gradient is 0, nothing is refused.
 * Order.  No float atomics: a pair's sums run over its partners in index order, a group's terms are added in index order and scaled once, one plain
 *   store per group, and the groups' partials are added in group order -- the loss has the same bits run to run.  "deterministic" needs nothing new.
 *   The sums within a group (up to 1023 addends) are running fp32 sums with Kahan's compensation; the sum over the groups is a plain running sum.
 * Limits.  KPRN_PAIRWISE_MAX_GROUP pairs per group; a pair's path count keeps the ragged limit of 4096.
 * Under "loss" "bpr": bce_literal is ignored; a batch without a group table is KPRN_E_ARG; kprn_train_step (host buffers, no groups) is
 *   KPRN_E_UNSUPPORTED; kprn_config.world > 1 with inv_batch = 0 is KPRN_E_UNSUPPORTED (kprn_train_step_batch passes no inv_batch) -- all decided
 *   before anything is launched or written.  Scoring, ranking, explaining and recommending calls do not look at the option.
 *
 * kprn_batch_set_groups uploads the table into storage the batch owns and counts the terms on the device, in integers; synchronous (one wait).  The table
 * goes with the batch's contents: any refill or feed of the slot, kprn_batch_slot_reserve and kprn_batch_destroy drop it.  KPRN_E_ARG, with the batch's
 * previous table left in place: offsets that decrease, go[0] != 0, go[G] != B, a group above the limit, G < 1, or a batch without labels.
 * kprn_host_pairwise_loss applies the rule on the host cores (no handle, no GPU; the same fp32 formula and partner order): dy [B], *loss, *n_terms from
 * pooled [B], labels [B] and the table; KPRN_E_ARG for a NULL argument or a bad table.                                                              */
#define KPRN_PAIRWISE_MAX_GROUP 1024
int kprn_batch_set_groups(kprn_handle* h, kprn_batch* b, const int32_t* group_offsets /* [G+1] */, int32_t G, int64_t* n_terms /* or NULL */);
int kprn_host_pairwise_loss(const float* pooled /* [B] */, const float* labels, const int32_t* group_offsets, int32_t G, int32_t B, float inv_batch,
                            float* dy /* [B] */, float* loss, int64_t* n_terms);

/* ---- hard negatives (an extension: dynamic negative sampling -- draw a pool of negatives per positive, score it, train on the ones that score highest;
 * the reference trains on the negatives its offline sampler drew) ----
 * Two calls.  kprn_select_hardest says which members of board groups to keep; kprn_batch_subset makes a batch of the kept pairs of a batch out of the rows that
 * were scored.  Each is useful on its own (a subset by any keep mask; a keep mask over any board groups).
 * Selection.  Groups over the score board, addressed exactly as in kprn_rank_groups: group g = members[group_offsets[g] .. group_offsets[g + 1]) (a line may
 *   appear more than once), members NULL = the consecutive board run; 1 <= n <= KPRN_RANK_MAX_GROUP members; pos[g] in -1 .. n-1 = the group's positive, -1 =
 *   none; pos NULL = -1 everywhere (NOT kprn_rank_groups' 0).
 *  - order: the RAW order of "ranking" and nothing else.  Member i's integer is c_i = (key << 12) | (4095 - i), key = 0 for NaN (invalid: a board entry nothing
 *    wrote), else the fp32 value mapped to 1 .. in fp32 order, -0 and +0 one value, -inf and +inf ordinary values.  An invalid member sorts below every valid
 *    one; equal scores go to the lower index.  There is no printed mode: the "%.5f" key ties most of a saturated pool.
 *  - rule: member i is kept iff i == pos[g], or fewer than n_keep members j != pos[g] have c_j > c_i.  1 <= n_keep <= KPRN_SELECT_MAX_KEEP.  A group with n_keep
 *    or fewer non-positive members keeps them all (invalid ones included).  The positive is excluded from the counting -- it is not counted and subtracted
 *    afterwards -- and is kept wherever its own score lies.
 *  - keep (uint8, host): keep[m] = 1 / 0 for the member at m, group_offsets[0] <= m < group_offsets[G] (member order; a line that appears twice has two
 *    entries); nothing below group_offsets[0] is touched.  n_invalid (int64, or NULL): the invalid non-positive members seen, each entry counted once.
 *  - kprn_select_hardest waits for every put queued so far; synchronous, ONE launch and one wait.  Places come from integer counts; the only atomic is the
 *    integer add of the invalid count: nothing depends on timing.  Everything is checked on the host first and a refused call writes nothing: the refusals
 *    are kprn_rank_groups' -- KPRN_E_ARG for NULL offsets, G < 1, a group outside 1..4096 members, pos outside -1..n-1, no board; KPRN_E_INDEX for a member or a
 *    run outside the board -- plus KPRN_E_ARG for n_keep outside 1..256 or a NULL keep.
 *  - kprn_host_select_hardest: the same rule on the host cores over a host score array scores [n_scores] in the board's place (no handle, no GPU); the same
 *    arguments otherwise, the same refusals.
 * Subset.  kprn_batch_subset(h, src, keep, out): keep [src's pair count] (uint8, host).  src: any batch, ragged or rectangular (P <= 4096, the ragged limit of
 *   a pair).  *out = a RAGGED batch of the pairs b with keep[b] != 0, in order; each keeps its paths' rows [cnt][T][F] unchanged and in order (copied on the
 *   device from src's ids in the caller's order) and its label; a src without labels gives an out without.  The result is a batch like any other: validation,
 *   occurrence index, identical-prefix plan and ragged plan are derived for it.  src's group table is not inherited; src itself is left as it was and stays
 *   usable.  Nothing kept: *out = NULL with KPRN_OK.  A fed src nobody used yet is waited for first; a src whose contents hold an id out of range is
 *   KPRN_E_INDEX; a src that does not hold its ids in the caller's order (a label-less fed batch with an identical-prefix plan) is KPRN_E_ARG.  Synchronous (the
 *   one wait of kprn_batch_create_ragged).
 * Why a subset and not a second find call: the sampled walks and the draws of "path_cap" "spread" are addressed by the pair-list ROW b; a kept pair that moves
 *   to another row of a second call's pair list gets other paths than the ones that were scored.                                                        */
#define KPRN_SELECT_MAX_KEEP 256
int kprn_select_hardest(kprn_handle* h, const int64_t* members, const int64_t* group_offsets, const int32_t* pos, int32_t G, int32_t n_keep,
                        unsigned char* keep /* uint8 [group_offsets[G]] */, int64_t* n_invalid /* or NULL */);
int kprn_host_select_hardest(const float* scores, int64_t n_scores, const int64_t* members, const int64_t* group_offsets, const int32_t* pos, int32_t G,
                             int32_t n_keep, unsigned char* keep, int64_t* n_invalid);
int kprn_batch_subset(kprn_handle* h, const kprn_batch* src, const unsigned char* keep /* uint8 [src's pairs] */, kprn_batch** out);

/* ---- dropout on the rnn cell's input (-useDropout / -dropout, OneModel.lua:246-265) ----
 * kprn_set_option(h, "dropout", "p") with 0 < p < 1 makes every TRAINING forward of an rnn_type 1, compute_dtype 0 handle (a forward that saves for the
 * backward: kprn_backward_batch, kprn_train_step, kprn_train_step_batch) apply nn.Dropout(p) to every layer's step input -- x_t for layer 1, h^{l-1}_t
 * above, never the recurrent input: y = x * m / (1 - p), m ~ Bernoulli(1 - p), independent per (layer, step, path, element).  Scoring passes never drop
 * (the module in evaluation mode).  MaskZero's flag of a step is taken from the UNDROPPED row.  The generator is the engine's own (torch's stream is not
 * the target) and is fully specified, so that a mask can be rebuilt anywhere:
 *   Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (e / 4, n, t + 65536 * l, draw); word e % 4 of the call is element e's word r
 *   (l = layer, 0-based; t = step; n = the path's index in the batch, rectangular or ragged; e = element of the layer's Din-wide input row);
 *   kept iff r >= thr, thr = min(2^32 - 1, floor(p * 2^32)) in double, p the rate rounded to fp32; kept: x * (float)(1.0 / (1.0 - (double)p)); dropped: +0.0f;
 *   draw = training forwards this handle has run since the seed was last set (32 bits); the backward of a step regenerates the masks of its forward.
 * Nothing stores a mask.  T <= 65535 and N < 2^32 per batch, or the training call returns KPRN_E_ARG.
 * kprn_host_dropout_keep is the rule on the host cores (no handle, no GPU): keep [T][N][Din], 1 = kept; KPRN_E_ARG for layer / T outside 0 / 1..65535,
 * N outside 1..2^32 - 1, Din < 1 or p outside [0, 1).                                                                                          */
int kprn_host_dropout_keep(uint64_t seed, unsigned int draw /* uint32 */, int32_t layer, int32_t T, int64_t N, int32_t Din, float p,
                           unsigned char* keep /* uint8 [T][N][Din] */);

/* The scoring writer's lines (eval/test_from_checkpoint.lua:110-118: counter \t string.format("%.5f", score) \t label, one per
 * pair, the label as Lua 5.1 prints a number = "%.14g"), n of them from counter0 on, formatted by the host cores into out.
 * Host-only (no handle, no GPU).  *written = bytes written; KPRN_E_ARG with *written = -(bytes needed) when cap is too small. */
int kprn_format_score_lines(int64_t counter0, const float* probs, const float* labels, int64_t n, char* out, int64_t cap,
                            int64_t* written);

/* ---- data-parallel hooks (new design; the reference is single-device) -----
 * The dense gradients (type_emb, relation_emb, LSTM, head) live in ONE contiguous device
 * buffer that the caller all-reduces (RCCL).  entity_emb gradients are row-sparse: pack
 * -> ONE all-gather -> merge on every rank.  All pointers are DEVICE pointers.           */
int kprn_dense_grad_buffer(kprn_handle* h, void** dev_ptr, int64_t* n_floats);
/* upper bound of the rows one step of this rank touches (agree on the MAX over ranks as the packing capacity) */
int kprn_sparse_grad_capacity(kprn_handle* h, int32_t* max_rows_per_step);
/* moves this step's touched entity rows into ONE packed device buffer of 32-bit words
 *   { int32 count, 3 x pad, int32 ids[capacity] (sorted, 0-based), float rows[capacity][d_entity] }
 * and clears them from the local accumulator; *n_words = 4 + capacity (1 + d_entity): the unit of the all-gather. */
int kprn_sparse_grad_pack(kprn_handle* h, int32_t capacity, void** dev_buf, int64_t* n_words);
/* dev_all = the `world` packed buffers back to back (all-gather output, THIS rank's included).  The union of the rows with
 * their sums in rank order (identical bits on every rank) is what the next kprn_apply_update walks: built here in the
 * accumulator (a marking pass per rank + one compaction), or -- kprn_set_option(h, "dp_fused_update", "1") -- only recorded
 * and formed inside the optimiser's row kernel (lazy-exact Adam without clip / L2; anything else builds it first): the
 * caller then keeps dev_all alive and unchanged until kprn_apply_update has been queued.  With "dp_dense_in_pack" = 1 the
 * dense gradient buffer rides behind the rows (n_words grows by its length rounded up to 4) and is summed here too.       */
int kprn_sparse_grad_merge(kprn_handle* h, const void* dev_all, int32_t world, int32_t capacity);
/* the stream everything is queued on (hipStream_t), so the caller can order collectives  */
int kprn_stream(kprn_handle* h, void** stream);

/* ---- the exchange issued by the engine (new design, SURVEY 8e: RCCL over xGMI) --------
 * Instead of handing buffers to the caller's collectives, the engine holds an RCCL communicator and queues
 *   pack (straight into its slot of the gathered buffer) -> ncclAllGather IN PLACE -> dense sum -> optimiser step on the union
 * on its own stream from two C calls; nothing of the host program sits between the kernels.  librccl is dlopen'ed
 * (rccl_path, or NULL = "librccl.so" as the process already has it); the caller's control plane carries the bootstrap:
 *   rank 0: kprn_dp_unique_id(path, id) -> broadcast the 128 bytes -> every rank: kprn_dp_init(h, path, id, rank, world)
 * (collective).  Per step, after kprn_backward_batch with inv_batch = 1 / (pairs of the GLOBAL minibatch):
 *   kprn_dp_exchange_begin(h, capacity)   capacity = the same multiple of 4 on every rank, >= every rank's touched rows
 *   ... work that does not depend on the update (a scoring pass) may be queued here ...
 *   kprn_dp_exchange_finish(h, opt)       = kprn_sparse_grad_merge + kprn_apply_update on the gathered buffer
 * kprn_set_option(h, "dp_comm_stream", "1") puts the collective on a stream of its own so that the work queued in between
 * overlaps it (world > 1).  Replicas stay bit-identical (rank-ordered sums).                                             */
int kprn_dp_available(const char* rccl_path);   /* KPRN_OK when librccl loads and has the entry points (no handle, no GPU work) */
int kprn_dp_unique_id(const char* rccl_path, void* id128 /* out: 128 bytes */);
int kprn_dp_init(kprn_handle* h, const char* rccl_path, const void* id128, int32_t rank, int32_t world);
int kprn_dp_exchange_begin(kprn_handle* h, int32_t capacity);
int kprn_dp_exchange_finish(kprn_handle* h, const kprn_opt* opt);
int kprn_dp_comm_size(kprn_handle* h, int32_t* nranks);   /* the communicator's rank count as RCCL reports it (ncclCommCount) */
int kprn_dp_shutdown(kprn_handle* h);   /* destroys the communicator (kprn_destroy does it too); restores the two options kprn_dp_init forced on */

/* ---- checkpoints (OneModel.lua:392-408 torch.save{embeddingLayer,predictor_net}) ------
 * native format: header + flat fp32 vector in getParameters() order (optimizer state is
 * NOT saved, like the reference).                                                        */
int kprn_save(kprn_handle* h, const char* path);
int kprn_load(kprn_handle* h, const char* path);

/* ---- measurement ------------------------------------------------------------------- */
/* when enabled, every kernel family is bracketed by HIP events on the handle's stream   */
int kprn_profile_enable(kprn_handle* h, int32_t on);
int kprn_profile_reset(kprn_handle* h);
/* fills up to cap entries; returns the number of kernel families seen in *n             */
typedef struct { char name[48]; double total_ms; int64_t launches; } kprn_prof_entry;
int kprn_profile_get(kprn_handle* h, kprn_prof_entry* out, int32_t cap, int32_t* n);
/* options (all strings):
 *   "impl"            "auto" (fused kernels where the shape allows) | "generic"
 *   "prefix_plan"     "1" (default): batches created from now on get an identical-prefix plan (leading steps shared by whole
 *                     64-path tiles are run once per batch, fused path); "0": every step of every path is executed
 *   "score_overlap"   "1": kprn_forward_batch_async runs the (fused) scoring pass on a second stream with its own output
 *                     buffers, so that it shares the chip with the work enqueued after it -- typically the training forward of the
 *                     same step, which does not depend on it.  Whatever would change what the pass reads (an optimiser step, a row
 *                     catch-up, kprn_set_*) waits for it; kprn_read_probs / kprn_sync wait for it on the host.  "0" (default): in
 *                     order on the handle's stream.
 *   "reserve_cus"     CUs the persistent scoring kernel leaves free (a collective's copy kernels run beside it), 0..1024; the pass always keeps
 *                     at least one workgroup
 *   "profile_filter"  kernel-family name prefix: only those families get HIP events while profiling is on ("" = all); an event
 *                     pair costs ~4 us of stream time
 *   round 5 (each is the A/B switch of one design choice; the defaults are the fast paths, the tests run both sides in one process):
 *   "bf16_small_tables" "1" (default): bf16 pipeline (compute_dtype 1, persistent launches): the gradients of the type / relation tables (<= 128
 *                     rows together) and of their column blocks of W_i2g come from 128 one-hot columns of ONE merged dW product, dx is formed
 *                     for the entity slice only; "0": full dx product + table-gradient launch
 *   "bf16_bptt_dxe"   "8" (default) | "16": that slice of dx is formed inside the persistent BPTT launch (value = depth of its weight ring);
 *                     "0": by its own product launch
 *   "small_tables"    "1" (default): the same identity on layer 0 of the generic fp32 LSTM / rnn backward; "0": dx product + table-gradient launch
 *   "persist_layers"  "1" (default): a recurrent layer of the generic fp32 pipeline (FastLSTM / rnn, Din % 4 == 0, Din, H <= 256) runs as ONE
 *                     persistent launch, forward and BPTT, once the batch gives every CU a 64-path tile; "2": at any batch size; "0": one launch
 *                     per step
 *   "persist_layers_grid" "0" (default): those launches run min(tiles, CUs) workgroups; "n" > 0: at most n, so that a workgroup walks several 64-path tiles at
 *                     batch sizes a float64 reference handles (tests; same results up to fp32 re-association of the bias and weight gradient sums; the forward
 *                     is bit-identical).  Per handle, read at every launch.  A value above the CU count (or above the batch's tile count) has no effect.  Negative or not a
 *                     number: KPRN_E_ARG
 *   "bf16_gemm_pingpong" "0" (default) | "1", "bf16_gemm_regstage" "0" | "1", "bf16_gemm_touch" "0" | chunks ahead, "bf16_t_pad" "64" | 0..512
 *                     (elements, a multiple of 8): measured alternatives of the bf16 split-K dW product (two wave groups one barrier apart; operands
 *                     staged through registers; L2 prefetch by touch; row pitch of its transposed operands) -- none faster than the default,
 *                     kept as the record of DESIGN.md section 7-3 and run against the default by tests/test_gpu_persist.py.  All four per handle,
 *                     read at every backward (and by kprn_debug_gemm what 5 / 6 on that handle)
 *   "score_rest_before_bptt" "0" (default) | "1": with "score_split" f > 0, the deferred part is queued right behind the loss stage on a stream of the lowest
 *                     priority: its single-tile workgroups take the CUs the first BPTT launch leaves idle in its tail
 *   "score_rest_in_backward" "0" (default) | "1": with "score_split" f > 0, the fused backward places the deferred part of the scoring pass itself, right behind its
 *                     last BPTT launch (beside the step's serial tail); measured slower than the whole pass first at world 1
 *   "tile_handover"   "2" (default) | "1" | "0": the fused D = H = 64 BPTT launches let a 64-path tile change workgroups once, between two of its steps, so
 *                     that the workgroups' step sums differ by less than a step on a left-padded path set (workgroup b paired with b + G / 2; "1": with
 *                     G - 1 - b; "0": whole tiles only).  Same gradients up to fp32 re-association of the weight-gradient partial sums; see
 *                     kprn_batch_handover_stats, DESIGN.md section 3.3b
 *   "adam_merged"     "1" (default) | "0": lazy-exact Adam updates the touched entity rows and the dense arena in one launch (bit-identical to two)
 *   "bwd_pipe"        "1" (default) | "0": fused path, batches of 16-row tiles, two layers: both layers' BPTT in one launch, the bottom layer a step behind
 *                     the top layer | one launch per layer
 *   "score_dual"      "2" (default) | "1" | "0": with "score_overlap": a pass queued by kprn_forward_batch_async is held back and runs in the launch of the
 *                     training forward that follows (one kernel, no second stream) -- for batches below 8 192 paths | always | never; anything that needs
 *                     the pass earlier runs it the usual way
 *   "catchup_prefix"  "1" (default) | "0": fused D = H = 64 path: a batch's lazy-exact row catch-up and its identical-prefix table in one launch | two
 *                     (bit-identical)
 *   "fused_small_tables" "1" (default) | "0": fused D = H = 64 path: type / relation table gradients formed inside the bottom BPTT launch | by a
 *                     passenger job of the entity-gradient launch (equal to fp32 re-association)
 *   "small_tables_fwd" "1" (default) | "0": fused D = H = 64 forward (fp32, two layers, one type slot, dt = dr = 16, de = 32, Vt + Vr <= 16): layer 0's input
 *                     half multiplies [one-hot(relation, type) | entity row] by [Q ; W_i2g[:, entity cols]^T] with Q = table W_i2g[:, its cols]^T formed in the
 *                     launch's prologue (K = 48 instead of 64) | the full x row (equal to fp32 re-association of 32 of the 64 terms).  Independent of
 *                     "small_tables", which leaves the forward bit-identical
 *   "head_select"     "1" (default) | "0": fused D = H = 64 fp32 forward: the nn.Linear(H, C) head forms column classId alone (what nn.Select(2, classId) keeps)
 *                     in the training forward and in every scoring pass whose caller reads the selected class only; a call that asks for all_probs,
 *                     pooled or path_scores takes the every-class head | the every-class head always.  The selected column is bit-identical either way;
 *                     the other columns of a pass that took the selected head are not written
 *   "rank_sort_min"   "512" (default) | 257..4097: kprn_rank_groups ranks groups of this many members and more by a sort in LDS, smaller ones by counting
 *                     against every member (same results; counting is faster at 257 members, the sort from 512 on: profiles/rank/README.md)
 *   "train_step_return" "loss" (default) | "drain": see kprn_train_step
 *   "inline_upload"   "side" (default): kprn_train_step uploads its minibatch on the upload stream, beside the previous step's backward, whenever the previous
 *                     call waited for its loss (every reader of the slot being refilled is then known to be done); "main": on the engine's stream
 *   "deterministic"   "0" (default) | "1" | "2": bit-reproducible training ("2": below).  With "1" every float the engine hands back -- losses, kprn_get_grad / kprn_get_flat_grads,
 *                     parameters, both optimiser state slots -- is a function of the inputs only, never of timing: the same sequence of calls with the same
 *                     inputs gives the same bits across repeats, handles, processes and whatever else runs on the device, for a fixed build, device model (CU
 *                     count) and fixed values of all other options (no promise across grid or tile sizes, option values or builds).  Covered: the fused fp32
 *                     path (FastLSTM, D = H = 64, one or two layers, compute_dtype 0, 2 and 3; one type slot, slices in 16-column blocks, type / relation
 *                     tables of at most 16 rows), every tile size, batch form, entry point, optimiser and value of the other options: its float atomics are
 *                     replaced by plain-stored partial sums added in a fixed order.  Not covered, and REFUSED: kprn_backward_batch,
 *                     kprn_train_step_batch and kprn_train_step return KPRN_E_UNSUPPORTED -- before anything is launched or written, the message names the
 *                     pipeline -- when the call would run on the generic pipeline ("impl" "generic", any other shape), on rnn / gru, on the bf16 pipeline
 *                     (compute_dtype 1) or on a KPRN_DBG scatter route.  Scoring, ranking, explanation and parameter access are never refused; data-parallel
 *                     handles are accepted (the exchange sums in rank order).  "0" again makes the same handle train as before; with "0" nothing changes.
 *                     "2": everything "1" covers runs exactly as under "1" (same kernels, same bits), and the generic fp32 pipeline trains under the same
 *                     contract: rnn_type 0 (FastLSTM) and 1 (rnn, "dropout" included), compute_dtype 0, any D, H, L, "impl" "generic", every "persist_layers" /
 *                     "small_tables" value, optimiser, batch form and entry point -- its split-K products, column sums, head, entity and table gradients store
 *                     one slab of partials per workgroup or split, and a launch behind adds the slabs in index order.  Still KPRN_E_UNSUPPORTED under "2":
 *                     rnn_type 2 (gru), compute_dtype 1 and any compute_dtype != 0 that would land on the generic pipeline, a generic-pipeline batch without
 *                     the occurrence index or with an identical-prefix plan, and, where layer 0 takes the scatter route, a type / relation table of more than
 *                     128 rows or a slice wider than 128 columns.  Any other value: KPRN_E_ARG.
 *   "dropout"         "0" (default) | a decimal rate in (0, 1): nn.Dropout on the step input of every rnn layer in training forwards (see kprn_host_dropout_keep).
 *                     Not a number or outside [0, 1): KPRN_E_ARG.  A rate > 0 on a handle with rnn_type != 1 (the reference's lstm / gru ignore the flag) or
 *                     compute_dtype != 0 is refused with KPRN_E_UNSUPPORTED when it is set.  With a rate > 0 layer 0's backward leaves the small-table identity
 *                     ("small_tables") for the dx product + table-gradient route.  "0" restores the launches of a handle that never had the option
 *   "loss"            "bce" (default) | "bpr": what kprn_backward_batch and kprn_train_step_batch train on -- nn.BCECriterion on each pair by itself | the pairwise
 *                     ranking loss over the batch's group table (see kprn_batch_set_groups, "pairwise loss").  Read at every training call; with "bce" nothing
 *                     changes.  Any other value: KPRN_E_ARG
 *   "path_cap"        "first" (default) | "spread": which of a pair's paths a find call keeps when more exist than max_paths -- the first ones in the pair's
 *                     order | one drawn in each of max_paths strata of that order ("finding a pair's paths", cap mode).  Read by every find call that has a
 *                     seed and a draw; kprn_find_paths has none and always keeps the first.  With "first" nothing changes.  Any other value: KPRN_E_ARG
 *   "pool_gamma"      "1" (default) | a decimal temperature in [1e-3, 1e3] (the syntax of "dropout"): the gamma of the paper's pooling layer
 *                     log sum_k exp(s_k / gamma) on a LogSumExp handle (see "pooling temperature").  Read at every scoring, explaining and training call.
 *                     Not such a number, not finite or outside the range: KPRN_E_ARG.  A value other than 1 on a handle whose reducer is not 2 (LogSumExp):
 *                     KPRN_E_UNSUPPORTED -- Max and TopK + Mean have no temperature.  A refused call leaves the previous value.  With "1" nothing changes
 *   "dropout_seed"    decimal or 0x hex uint64 (default: kprn_config.seed + rank, so data-parallel replicas draw different masks): the generator's seed;
 *                     setting it restarts the draw count at 0
 *   (also: "small_tiles", "score_split", "loss_accumulate", "feed_build" / "feed_threads" / "feed_workers", "dp_comm_stream",
 *    "dp_fused_update", "dp_dense_in_pack" -- described at the calls they modify)                                                 */
int kprn_set_option(kprn_handle* h, const char* key, const char* value);
/* measurement hook: mean milliseconds per launch of one GEMM shape of the generic pipeline on random data (scripts/gpu_gemm_bench.py).
 * what: 0 C = A B^T, 1 C = A B, 2 C += A^T B (split-K), 3 FastLSTM step kernel (M paths, N = H, K = Din), 4 Recurrence step kernel */
int kprn_debug_gemm(kprn_handle* h, int32_t what, int64_t M, int32_t N, int64_t K, int32_t iters, float* ms);
/* test hook (tests/test_gpu_gemm16_products.py): ONE launch of a bf16 product of the bf16 pipeline (gemm_bf16.hip) on the caller's data, on h's stream,
 * under h's "bf16_gemm_*" options and with a zero block of its own:  C[M][N] (fp32) = or += bf16(A)[M][K] bf16(B)[N][K]^T (+ bias[N]).
 * A, B, C are host fp32 arrays of a_count / b_count / c_count elements; the operands are windows inside them: origin a_off / b_off / c_off (elements),
 * row pitch lda / ldb / ldc.  A and B are converted on the device with the pipeline's own conversion (round to nearest even) -- whole arrays, so what
 * surrounds a window may hold anything, NaN included; the whole C array goes up and comes back, so the caller sees every element a launch wrote.
 * route: 0 = gemm16 as the pipeline calls it (the LDS-DMA kernels where they cover the shape, else k_gemm16), 1 = the LDS-DMA kernels alone,
 *        2 = the k-major-A product: A is AT[K][lda] (lda >= M = T Np columns (step, path), Np - Nv pad columns per step), C has T Nv rows,
 *        3 = k_gemm16 alone.
 * accumulate, split_k (routes 0, 1, 3), n_lo, k_lo, sx_min (route 1), Np, Nv (route 2), bias (routes 0, 3; NULL = none) are handed to the product as they are.
 * KPRN_E_ARG, before anything is allocated or launched, for what the products' contracts exclude: K, lda, ldb, k_lo or Np not a multiple of 8; a_off or b_off
 * not a multiple of 8 or c_off not a multiple of 4 (16-byte aligned operands); a pitch below the extent or a window that does not fit its array; Nv > Np or
 * Nv < 1; M not a multiple of Np; a bias with accumulate or on routes 1, 2; M, N, K < 1; a NULL pointer.
 * ran: what the launchers report -- kernel (KPRN_GEMM16_*; DECLINED: the route does not cover the shape, nothing was launched, C comes back as it went up),
 * the number of K ranges and their width; dx_t_ok = dx_from_transposed_ok(M, N, K, Np), what the BPTT launch is promised (route 2 only, else 0). */
enum { KPRN_GEMM16_DECLINED = 0, KPRN_GEMM16_SMALL = 1, KPRN_GEMM16_BIG = 2, KPRN_GEMM16_X = 3, KPRN_GEMM16_R = 4, KPRN_GEMM16_P = 5, KPRN_GEMM16_XT = 6 };
typedef struct kprn_gemm16_call {
  int32_t route, accumulate, split_k, n_lo, sx_min, N;
  int64_t M, K, k_lo, Np, Nv;
  int64_t a_count, a_off, lda;
  int64_t b_count, b_off, ldb;
  int64_t c_count, c_off, ldc;
} kprn_gemm16_call;
typedef struct kprn_gemm16_ran {
  int32_t kernel, nsplit;
  int64_t kchunk;
  int32_t dx_t_ok, reserved;
} kprn_gemm16_ran;
int kprn_debug_gemm16_run(kprn_handle* h, const kprn_gemm16_call* call, const float* A, const float* B, const float* bias, float* C, kprn_gemm16_ran* ran);

#ifdef __cplusplus
}
#endif
#endif /* KPRN_H */
