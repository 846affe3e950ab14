"""Model construction from the reference's command-line surface (release/songPathRnn/model/OneModel.lua).

`parse_flags` accepts the torch.CmdLine flags of OneModel.lua:27-87 with the same names and
defaults; `build_engine` turns them into a kprn Engine the way OneModel.lua:204-309 builds
predictor_net / reducer / training_net.  Options the engine does not implement fail loudly with
the library's KPRN_E_UNSUPPORTED (dropout on lstm / gru, where the reference ignores the flag) instead of silently doing something else.
"""
import argparse

from . import _ffi

LABEL_DIMENSION = 46  # OneModel.lua:119


def flag_parser():
    p = argparse.ArgumentParser(prefix_chars="-", add_help=True, description="songPathRnn flags (OneModel.lua:27-87)")
    a = p.add_argument
    a("-dataDir", default=""); a("-minibatch", type=int, default=32); a("-testTimeMinibatch", type=int, default=32)
    a("-numRowsToGPU", type=int, default=1); a("-gpuid", type=int, default=-1); a("-lazyCuda", type=int, default=0)
    a("-relationVocabSize", type=int, default=51503); a("-entityTypeVocabSize", type=int, default=2267)
    a("-entityVocabSize", type=int, default=1540261)
    a("-relationEmbeddingDim", type=int, default=50); a("-entityTypeEmbeddingDim", type=int, default=50)
    a("-entityEmbeddingDim", type=int, default=50)
    a("-numFeatureTemplates", type=int, default=-1); a("-numEntityTypes", type=int, default=-1)
    a("-learningRate", type=float, default=0.001); a("-learningRateDecay", type=float, default=0.0)
    a("-tokenFeatures", type=int, default=1); a("-evaluationFrequency", type=int, default=10)
    a("-model", default=""); a("-exptDir", default=""); a("-initModel", default="")
    a("-paramInit", type=float, default=0.1); a("-startIteration", type=int, default=1); a("-saveFrequency", type=int, default=50)
    a("-embeddingL2", type=float, default=0.0001); a("-l2", type=float, default=0.0001)
    a("-architecture", default="rnn"); a("-numEpochs", type=int, default=300); a("-batchesPerEpoch", type=int, default=500)
    a("-rnnType", default="rnn"); a("-rnnDepth", type=int, default=1); a("-rnnHidSize", type=int, default=50)
    a("-useAdam", type=int, default=0); a("-epsilon", type=float, default=1e-8)
    a("-useGradClip", type=int, default=1); a("-gradClipNorm", type=float, default=5.0)
    a("-gradientStepCounter", type=int, default=100)
    a("-includeEntityTypes", type=int, default=1); a("-includeEntity", type=int, default=-1)
    a("-topK", type=int, default=0); a("-K", type=int, default=5)
    a("-package_path", default=""); a("-createExptDir", type=int, default=1)
    a("-useReLU", type=int, default=1); a("-rnnInitialization", type=int, default=1); a("-regularize", type=int, default=1)
    a("-numLayers", type=int, default=1); a("-useDropout", type=int, default=0); a("-dropout", type=float, default=0.0)
    # engine-side additions (not in the reference)
    a("-seed", type=int, default=12345); a("-entityUpdate", type=int, default=0)
    a("-dropoutSeed", type=lambda v: int(v, 0), default=None,
      help="seed of the dropout mask generator (decimal or 0x hex, 64 bits; default: -seed); a data-parallel rank r seeds with this + r, so replicas do not share masks; the engine's option \"dropout_seed\"")
    a("-deterministic", type=int, default=0, choices=[0, 1, 2],
      help="1: bit-reproducible training (the engine's option \"deterministic\": fixed-order gradient sums on the fused fp32 path; a model that would train on any other pipeline is refused with KPRN_E_UNSUPPORTED); "
           "2: the same, and the generic fp32 pipeline (lstm and rnn cells of any width, -useDropout included) trains with fixed-order sums too")
    a("-checkpointFormat", default="native", choices=["native", "t7", "both"],
      help="the native checkpoint is always written at <model>-latest; t7 / both ALSO write <model>-latest.t7, the parameters in a Torch7 {embeddingLayer, predictor_net} container (the reference writes its container at <model>-latest itself)")
    # evaluation during training (the slot OneModel.lua:389 left commented out): every -evaluationFrequency epochs the pairs of -testList are scored
    # and the groups of -rank_samples ranked on the device (scoring.rank_test_set); without -rank_samples nothing is evaluated
    a("-rank_samples", default=""); a("-rank_entity", default=""); a("-rank_users", default=""); a("-testList", default="test.list")
    # training from a knowledge graph (python -m kprn_amd.train; not in the reference): negatives sampled and paths found on the device, step by step
    a("-kg", default="", help="triples.tsv (head, relation, tail names per line, directed): train from this graph instead of -dataDir; needs -vocab_dir and -interaction_rel")
    a("-vocab_dir", default=""); a("-interaction_rel", default="", help="the relation whose (user, item) edges are the positives")
    a("-negatives", type=int, default=4); a("-neg_alpha", type=float, default=0.0, help="negatives are drawn with weight (item's interactions)^neg_alpha; 0 = uniform")
    a("-neg_attempts", type=int, default=16); a("-min_hops", type=int, default=2); a("-max_hops", type=int, default=3); a("-max_paths", type=int, default=28)
    a("-sampleSeed", type=int, default=1)
    a("-loss", default="bce", choices=["bce", "bpr"],
      help="with -kg: bce = nn.BCECriterion on each pair by itself; bpr = the pairwise ranking loss of each positive against its own sampled negatives (the engine's option \"loss\")")
    a("-walks", type=int, default=0, help="walks per pair and hop count that sample the paths of 4 and 5 hops (1..256); needed when -max_hops is above 3")
    a("-path_cap", default="first", help="which of a pair's paths are kept when more than -max_paths exist: first = the first ones in the finder's order; "
      "spread = one drawn in each of -max_paths strata of that order under -sampleSeed (the engine's option \"path_cap\"): training draws anew every step")
    a("-neg_pool", type=int, default=0, help="with -kg: hard negatives -- every step draws this many negatives per positive, scores them with the current model and "
      "trains on the -negatives that score highest (graph.train_from_graph neg_pool); 0 or -negatives = the sampled negatives as they are; at most 256")
    # held-out evaluation from the graph (graph.KnowledgeGraph.holdout + graph.evaluate_from_graph; python -m kprn_amd.train / kprn_amd.evaluate)
    a("-holdout", type=float, default=0.0, help="with -kg: this share of the -interaction_rel pairs is held out (the reference's split_train_test.py with "
      "train fraction 1 - this), training sees the rest, and every -evaluationFrequency epochs the held pairs are ranked among everything their users reach; 0 = no split")
    a("-holdout_seed", type=int, default=1, help="seed of the split's shuffle")
    a("-eval_users", type=int, default=0, help="evaluate the first N held-out users only (0 = all)")
    a("-max_candidates", type=int, default=0, help="evaluation ranks among each user's N strongest candidates by path count only (0 = all of them)")
    a("-eval_negatives", type=int, default=0, help="with -holdout: every held pair is ranked against at most N negatives drawn on the device from its user's "
      "candidates (the reference's sample.py / eval_score.py protocol with N = 100; the engine's \"sampled evaluation groups\"), at most 4095; 0 = against "
      "everything the user reaches")
    a("-meta_paths", default="", help="with -kg: a file of relation-sequence patterns, one per line (graph.parse_meta_paths: positions separated by blanks, "
      "a position `*` or relation names joined by `|`); only the paths that match one are found, as candidates, for training and for evaluation")
    a("-gamma", type=float, default=None, help="temperature of the LogSumExp reducer, the paper's log sum exp(s / gamma), in 0.001 .. 1000 (the engine's option "
      "\"pool_gamma\"); unset = what the checkpoint carried (1 if nothing); given, it is applied after the checkpoint is loaded; needs the LogSumExp reducer")
    return p


def check_walks(max_hops, walks, error):
    """the finder's sampling limits, decided on the host before an engine exists: error(message) for a -max_hops above 3 without -walks"""
    if max_hops > _ffi.FIND_MAX_HOPS_SAMPLED:
        error("-max_hops must be at most %d" % _ffi.FIND_MAX_HOPS_SAMPLED)
    if max_hops > _ffi.FIND_MAX_HOPS and not 1 <= walks <= _ffi.FIND_MAX_WALKS:
        error("-max_hops %d needs -walks N (1..%d): paths of more than %d hops are sampled, N walks per pair and hop count"
              % (max_hops, _ffi.FIND_MAX_WALKS, _ffi.FIND_MAX_HOPS))
    if walks < 0 or walks > _ffi.FIND_MAX_WALKS:
        error("-walks must be in 0..%d" % _ffi.FIND_MAX_WALKS)


POOL_GAMMA_MIN, POOL_GAMMA_MAX = 1e-3, 1e3   # the range of the engine's option "pool_gamma"


def check_gamma(gamma, reducer, reducer_flag, error):
    """-gamma, decided on the host before an engine exists: error(message) for a value outside the option's range, or for one other than 1 beside a reducer
    flag (named reducer_flag: -topK when training, -top_k when scoring) that does not select LogSumExp -- Max and TopK + Mean have no temperature"""
    if gamma is None:
        return
    if not POOL_GAMMA_MIN <= gamma <= POOL_GAMMA_MAX:   # (false for a NaN)
        error("-gamma must be in %g .. %g, got %r" % (POOL_GAMMA_MIN, POOL_GAMMA_MAX, gamma))
    if gamma != 1 and reducer != 2:
        error("-gamma %r needs %s 2 (LogSumExp): %s has no temperature" % (gamma, reducer_flag, "TopK + Mean" if reducer == 1 else "max pooling"))


def parse_flags(argv=None, gamma_beside="-topK"):
    """gamma_beside: the reducer flag -gamma is checked against here (-topK, the training flag); None = the caller checks it against its own (check_gamma)"""
    p = flag_parser()
    params = p.parse_args(argv)
    if gamma_beside is not None:
        check_gamma(params.gamma, reducer_of_train_flag(params.topK), gamma_beside, p.error)
    if params.kg and not (params.vocab_dir and params.interaction_rel):
        p.error("-kg needs -vocab_dir DIR (the vocabulary files) and -interaction_rel NAME (the relation of the user-item edges to train on)")
    if params.loss == "bpr" and not params.kg:
        p.error("-loss bpr needs -kg: the groups it ranks within (a positive and its sampled negatives) exist only when training from a graph")
    check_walks(params.max_hops, params.walks, p.error)
    if params.path_cap not in _ffi.PATH_CAPS:
        p.error("-path_cap must be first or spread, got %s" % params.path_cap)
    if params.neg_pool != 0 and not params.kg:
        p.error("-neg_pool needs -kg: the pool it selects from (a positive's sampled negatives) exists only when training from a graph")
    if params.neg_pool != 0 and not params.negatives <= params.neg_pool <= _ffi.SELECT_MAX_KEEP:
        p.error("-neg_pool must be 0 or in -negatives .. %d (the pool holds at least the negatives kept), got %d" % (_ffi.SELECT_MAX_KEEP, params.neg_pool))
    if params.meta_paths and not params.kg:
        p.error("-meta_paths needs -kg: the patterns select among the paths found in a graph")
    if not 0.0 <= params.holdout < 1.0:
        p.error("-holdout must be in 0 .. 1 (the share of the interactions held out)")
    if params.holdout > 0 and not params.kg:
        p.error("-holdout needs -kg: it splits the graph's -interaction_rel edges")
    if not 0 <= params.max_candidates <= 2**31 - 1 or params.eval_users < 0:
        p.error("-max_candidates must be in 0 .. 2^31 - 1 and -eval_users >= 0")
    if not 0 <= params.eval_negatives <= _ffi.EVAL_MAX_NEG:
        p.error("-eval_negatives must be in 0 .. %d" % _ffi.EVAL_MAX_NEG)
    if params.eval_negatives > 0 and params.holdout <= 0:
        p.error("-eval_negatives needs -holdout: it draws the negatives of the held pairs")
    return params


RNN_TYPES = {"lstm": 0, "rnn": 1, "gru": 2}


def dropout_rate(params):
    """the engine's option "dropout" for these flags: -dropout where -useDropout is on (OneModel.lua:246 builds nn.Dropout(params.dropout) only then), else 0"""
    return float(params.dropout) if params.useDropout != 0 and params.dropout > 0 else 0.0


def reducer_of_train_flag(topK):
    """OneModel.lua:284-293: -topK 1 -> TopK+Mean, 2 -> LogSumExp, ANYTHING ELSE -> nn.Max"""
    return {1: 1, 2: 2}.get(int(topK), 0)


def reducer_of_score_flag(top_k):
    """test_from_checkpoint.lua:69-79: -top_k 0 -> nn.Max, 2 -> LogSumExp, ANYTHING ELSE -> TopK+Mean"""
    return {0: 0, 2: 2}.get(int(top_k), 1)


REDUCER_NAME = {0: "Reducer is max pool", 1: "Reducer is topK", 2: "Reducer is LogSumExp"}

NATIVE_MAGIC = b"KPRNAMD1"


def load_checkpoint(eng, path):
    """-initModel / -model_path: the native format (kprn_save) or a reference Torch7 checkpoint {embeddingLayer, predictor_net}
    (OneModel.lua:392-400), told apart by the file's first bytes"""
    with open(path, "rb") as f:
        head = f.read(8)
    if head == NATIVE_MAGIC:
        eng.load(path)
        return "native"
    from . import formats
    params = formats.checkpoint_params(path, num_layers=eng.cfg.L)
    lay = eng.layout()
    missing = [n for n in lay if n not in params]
    if missing:
        raise _ffi.KprnError(_ffi.E_IO, f"{path}: checkpoint lacks {missing}")
    for n in lay:
        eng.set_param(n, params[n])
    return "t7"


def save_checkpoint_t7(eng, path):
    """PARAMETER EXCHANGE in the reference's container: a Torch7 table {embeddingLayer, predictor_net} (OneModel.lua:392-400) whose nn.* objects
    carry the weight tensors under the reference's field names, in module order -- what formats.checkpoint_params (and a Lua script that walks
    the tables) reads back.  NOT a runnable checkpoint for eval/test_from_checkpoint.lua: the Element-Research rnn modules in it have no
    recurrentModule graph, sharedClones or step state, so model:forward would fail; rebuild the model with OneModel.lua's constructor and copy
    the tensors in."""
    from . import formats
    formats.write_checkpoint(path, {n: eng.get_param(n) for n in eng.layout()}, num_entity_types=eng.cfg.num_types, use_relu=eng.cfg.use_relu)


def build_engine(params, rank=0, world=1, device_id=None, stream=None):
    """OneModel.lua:204-309.  The embedding variants of OneModel.lua:207-219: a table that is left out (-includeEntityTypes 0 /
    -includeEntity 0) is a table of width 0 to the engine -- x_t = [types | relations], [entities | relations] or [relations],
    parameters in the same flat order with the absent table contributing nothing."""
    inc_types, inc_ent = params.includeEntityTypes == 1, params.includeEntity == 1
    if params.numEntityTypes > params.numFeatureTemplates:
        raise _ffi.KprnError(_ffi.E_ARG, "assert(numEntityTypes <= numFeatureTemplates) (OneModel.lua:107)")
    if params.rnnType not in RNN_TYPES:
        raise _ffi.KprnError(_ffi.E_ARG, f"rnnType must be lstm, rnn or gru, got {params.rnnType}")
    rate = dropout_rate(params)
    if rate == 0 and params.useDropout != 0 and params.rnnType != "rnn":
        # -useDropout 1 at rate 0 sets no option, and the refusal of the flag on lstm / gru stays what it was
        raise _ffi.KprnError(_ffi.E_UNSUPPORTED, "-useDropout is built for -rnnType rnn only (the reference's lstm / gru modules ignore it)")
    if device_id is None:
        device_id = max(0, params.gpuid)
    eng = _ffi.Engine(params.entityTypeVocabSize, params.entityVocabSize, params.relationVocabSize,
                      params.entityTypeEmbeddingDim if inc_types else 0, params.entityEmbeddingDim if inc_ent else 0, params.relationEmbeddingDim,
                      params.rnnHidSize, params.numLayers, F=params.numFeatureTemplates, num_types=params.numEntityTypes,
                      C_=LABEL_DIMENSION, reducer=getattr(params, "reducer", reducer_of_train_flag(params.topK)), K=params.K, rnn_type=RNN_TYPES[params.rnnType],
                      use_relu=params.useReLU, rnn_init=params.rnnInitialization,
                      device_id=device_id, rank=rank, world=world, param_init=params.paramInit, seed=params.seed, stream=stream)
    try:
        if rate > 0:
            eng.set_option("dropout", repr(rate))   # (lstm / gru, where the reference ignores the flag: KprnError(E_UNSUPPORTED) from the library)
        if getattr(params, "dropoutSeed", None) is not None:
            # like the default seed (-seed + rank), the given one is offset by the rank: data-parallel replicas do not share masks
            eng.set_option("dropout_seed", str((int(params.dropoutSeed) + rank) & 0xFFFFFFFFFFFFFFFF))
        if getattr(params, "path_cap", "first") != "first":
            eng.set_option("path_cap", params.path_cap)   # (read by every find call that has a seed: training, recommending, evaluating from a graph)
        if getattr(params, "deterministic", 0):
            eng.set_option("deterministic", str(int(params.deterministic)))   # (a training call on a pipeline without fixed-order sums then raises KprnError(E_UNSUPPORTED))
        if params.initModel:
            load_checkpoint(eng, params.initModel)  # OneModel.lua:277-282
        if getattr(params, "gamma", None) is not None:
            eng.set_option("pool_gamma", repr(float(params.gamma)))   # (after the checkpoint: a given -gamma overrides the one a native checkpoint carries)
    except Exception:
        eng.close()   # (a refused option or an unreadable checkpoint: the handle and its device memory go now, not when the object is collected)
        raise
    return eng


def opt_from_flags(params):
    """optConfig / optInfo of OneModel.lua:340-384 as a kprn_opt."""
    return _ffi.make_opt(method=1 if params.useAdam == 1 else 0, lr=params.learningRate, beta1=0.9, beta2=0.999,
                         eps=params.epsilon, lr_decay=params.learningRateDecay, regularize=params.regularize,
                         use_grad_clip=params.useGradClip, grad_clip_norm=params.gradClipNorm, l2=params.l2,
                         bce_literal=0, entity_update=params.entityUpdate)
