"""`python -m kprn_amd.train <flags>` == `th model/OneModel.lua <flags>` (release/songPathRnn/run_scripts/train.sh:86).

Same flags (OneModel.lua:27-87), same data layout (dataDir/train.list naming .torch / .int / .npz
files), same epoch log lines, checkpoint "<model>-latest" every saveFrequency epochs
(OneModel.lua:392-408; native format, kprn_save).

With `-kg triples.tsv -vocab_dir DIR -interaction_rel NAME` (an extension) there are no path files: the (user, item) edges of that relation are the
positives, and every step samples -negatives items per positive (an item's weight is its number of interactions to the power -neg_alpha's value, 0 =
uniform; at most -neg_attempts draws per negative), finds the pairs' paths of -min_hops .. -max_hops hops (at most -max_paths each; -max_hops 4 or 5 needs -walks N, the walks that sample the paths of more than 3 hops) and trains, all on the device (graph.train_from_graph); -sampleSeed seeds the shuffles
and the draws.  Same epoch lines, same -model / -saveFrequency.  -loss bpr trains on the pairwise ranking loss of each positive against its own sampled
negatives instead of BCE on each pair (include/kprn.h "pairwise loss"); it needs -kg.
-neg_pool P (with -kg; 0 or -negatives .. 256) trains on hard negatives: every step draws P negatives per positive, scores that pool with the current model
and keeps the -negatives that score highest, their rows taken from the scored batch (include/kprn.h "hard negatives").
-holdout 0.2 [-holdout_seed 1 -eval_users 0 -max_candidates N] (with -kg) holds that share of the interactions out (KnowledgeGraph.holdout), trains on the
rest -- positives, catalogue, weights and paths are the train graph's -- and every -evaluationFrequency epochs ranks the held pairs among everything
their users reach (graph.evaluate_from_graph): the evaluation line of -rank_samples, plus the held pairs that never reached the ranking stage.
-eval_negatives N (with -holdout) ranks every held pair against at most N negatives drawn on the device from its user's candidates instead (the reference's
sample.py / eval_score.py protocol; include/kprn.h "sampled evaluation groups"); the line then ends with the samples that got fewer than N.
-meta_paths FILE (with -kg) keeps only the paths whose relation sequence matches a pattern of FILE (graph.parse_meta_paths; include/kprn.h "meta-paths"), in
training and in the -holdout evaluation.
"""
import os
import sys

import numpy as np

from . import model
from .batcher import BatcherFileList
from .optimizer import MyOptimizer, OptimizerCallback


def make_evaluator(eng, params, log=None):
    """the epoch hook behind -evaluationFrequency: scores -testList, ranks the groups of -rank_samples on the device, prints hit@k / ndcg@k"""
    from . import evalrank, scoring
    assert params.rank_entity, "-rank_samples needs -rank_entity (the positional test.list.entity file)"
    with open(params.rank_entity) as f:
        entity_lines = f.readlines()
    with open(params.rank_samples) as f:
        samples = evalrank.read_samples(f)
    users = None
    if params.rank_users:
        with open(params.rank_users) as f:
            users = f.readlines()
    members, group_offsets, n_used = evalrank.group_index(entity_lines, samples, users)
    testBatcher = BatcherFileList(params.dataDir, params.testTimeMinibatch, False, 1000, params.gpuid != -1, params.testList, check_ids=False)

    def evaluator(i):
        if n_used == 0:
            print("evaluation: no test sample has all its pairs in " + params.rank_entity, file=log or sys.stdout)
            return None
        testBatcher.reset()
        res, _n = scoring.rank_test_set(eng, testBatcher, members, group_offsets)
        hits, ndcgs, n = evalrank.metrics_from_hist(res["hist"], 15)
        print("evaluation at epoch %d over %d samples: " % (i, n) +
              "  ".join("hit@%d %.5f ndcg@%d %.5f" % (k, hits[k], k, ndcgs[k]) for k in (1, 5, 10, 15)), file=log or sys.stdout)
        return hits, ndcgs, n
    return evaluator


def make_graph_evaluator(eng, params, train_kg, held, sampler, log=None):
    """the epoch hook behind -holdout: the held pairs ranked among everything their users reach in the train graph (graph.evaluate_from_graph); prints
    make_evaluator's line and the number of held pairs that never reached the ranking stage"""
    from . import graph

    def evaluator(i):
        res = graph.evaluate_from_graph(eng, train_kg, held, sampler, min_hops=params.min_hops, max_hops=params.max_hops, max_paths=params.max_paths,
                                        walks=params.walks, seed=params.sampleSeed, max_candidates=params.max_candidates, max_users=params.eval_users,
                                        eval_negatives=params.eval_negatives)
        hits, ndcgs = res["hits"], res["ndcgs"]
        print("evaluation at epoch %d over %d samples: " % (i, res["n"]) +
              "  ".join("hit@%d %.5f ndcg@%d %.5f" % (k, hits[k], k, ndcgs[k]) for k in (1, 5, 10, 15)) + "  unreachable %d" % res["n_unreachable"] +
              ("  short %d" % res["n_short"] if params.eval_negatives > 0 else ""), file=log or sys.stdout)
        return res
    return evaluator


def train_from_kg(params, eng, callbacks):
    from . import graph
    from .pathformat import Vocabs
    kg = graph.KnowledgeGraph.from_triples(graph.read_triples(params.kg), Vocabs(params.vocab_dir), params.numEntityTypes)
    if params.meta_paths:   # (the split below hands the set to the train graph)
        with open(params.meta_paths) as f:
            kg.patterns = graph.parse_meta_paths(f, kg)
    held = None
    if params.holdout > 0:   # everything below -- positives, catalogue, weights, paths -- is the train graph's
        kg, held = kg.holdout(params.interaction_rel, 1.0 - params.holdout, params.holdout_seed)
    positives = kg.interactions(params.interaction_rel)
    if len(positives) == 0:
        sys.exit("the graph has no edge of relation %s" % params.interaction_rel)
    items = np.unique(positives[:, 1])
    sampler = eng.sampler(items, kg.item_weights(items, params.neg_alpha, params.interaction_rel))
    pool = ", the highest-scoring of a pool of %d" % params.neg_pool if params.neg_pool > params.negatives else ""
    print("Training from the graph: %d positives, %d candidate items, %d negatives each%s" % (len(positives), len(items), params.negatives, pool))
    if held is not None:
        print("Held out: %d pairs of %d users" % (len(held), len(np.unique(held[:, 0]))))
        callbacks = callbacks + [OptimizerCallback(params.evaluationFrequency, make_graph_evaluator(eng, params, kg, held, sampler), "evaluation")]
    graph.train_from_graph(eng, kg, positives, model.opt_from_flags(params), params.minibatch, params.negatives, params.numEpochs, params.sampleSeed,
                           sampler=sampler, max_attempts=params.neg_attempts, min_hops=params.min_hops, max_hops=params.max_hops, max_paths=params.max_paths,
                           epoch_hooks=callbacks, start_iteration=params.startIteration, gradient_step_counter=params.gradientStepCounter, walks=params.walks,
                           loss=params.loss, neg_pool=params.neg_pool)
    return 0


def check_kg_vocabulary(params):
    """before the engine exists: the vocabulary files must be the ones the model flags describe (as python -m kprn_amd.recommend checks)"""
    from .pathformat import Vocabs
    voc = Vocabs(params.vocab_dir)
    sizes = tuple(max(int(v) for v in d.values()) + 1 for d in (voc.entity_type, voc.entity, voc.relation))
    if sizes != (params.entityTypeVocabSize, params.entityVocabSize, params.relationVocabSize):
        sys.exit("the vocabularies hold %d types, %d entities, %d relations; the model flags say %d, %d, %d"
                 % (sizes + (params.entityTypeVocabSize, params.entityVocabSize, params.relationVocabSize)))


def main(argv=None):
    params = model.parse_flags(argv)
    if params.kg:
        check_kg_vocabulary(params)
    if params.createExptDir == 1 and params.exptDir:
        os.makedirs(params.exptDir, exist_ok=True)
        with open(os.path.join(params.exptDir, "config.txt"), "w") as f:  # OneModel.lua:128-170
            for k, v in sorted(vars(params).items()):
                f.write(f"{k}\t{v}\n")
    eng = model.build_engine(params)
    print(model.REDUCER_NAME[model.reducer_of_train_flag(params.topK)])
    print("Using Adam!" if params.useAdam == 1 else "Using adagrad!")
    trainBatcher = None if params.kg else BatcherFileList(params.dataDir, params.minibatch, True, 100, params.gpuid != -1, "train.list", seed=params.seed, check_ids=False)   # (the engine validates every id)
    callbacks = []
    if params.model:
        def saver(i):
            path = params.model + "-latest"
            print("saving to " + path)
            eng.save(path)   # the native checkpoint is always written: it is the one this package (and its scoring CLI) is tested to load back
            if params.checkpointFormat in ("t7", "both"):
                model.save_checkpoint_t7(eng, path + ".t7")
        if params.createExptDir == 1:
            callbacks.append(OptimizerCallback(params.saveFrequency, saver, "saving"))
        else:
            print("WARNING! - createExptDir is NOT set!")
    if params.rank_samples:
        callbacks.append(OptimizerCallback(params.evaluationFrequency, make_evaluator(eng, params), "evaluation"))   # (OneModel.lua:389)
    if params.kg:
        return train_from_kg(params, eng, callbacks)
    opt = model.opt_from_flags(params)
    optimizer = MyOptimizer(eng, {"numEpochs": params.numEpochs, "epochHooks": callbacks, "minibatchsize": params.minibatch},
                            opt, startIteration=params.startIteration, gradientStepCounter=params.gradientStepCounter)
    optimizer.train(trainBatcher)
    return 0


if __name__ == "__main__":
    sys.exit(main())
