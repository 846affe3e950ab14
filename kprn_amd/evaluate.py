"""`python -m kprn_amd.evaluate <flags>`: how good is a checkpoint on interactions it never saw, from a knowledge graph alone (an extension; the
reference evaluates offline text files against 100 sampled negatives).  A thin command line over KnowledgeGraph.holdout and graph.evaluate_from_graph:
the split of `python -m kprn_amd.train -kg ... -holdout` is made again from the same flags, and every held pair is ranked among everything its user
reaches in the train graph.

Flags: those of `python -m kprn_amd.score` that shape and load the model (-model_path, -top_k, -gpu_id and the OneModel flags), plus
  -kg triples.tsv  -vocab_dir DIR  -interaction_rel R   the graph, its vocabularies, the relation of the user-item edges (as for train -kg)
  -holdout 0.2 [-holdout_seed 1]                        the share held out and the shuffle's seed: give what training was given
  -eval_users N  -max_candidates N                      the first N held-out users only; only each user's N strongest candidates by path count
  -eval_negatives N                                     the reference's protocol: every held pair against at most N negatives drawn on the device from its
                                                        user's candidates that it did not interact with (include/kprn.h "sampled evaluation groups"); 0 = all
  -min_hops / -max_hops / -max_paths / -walks / -sampleSeed   the finder's limits (1, 3, 28), as for python -m kprn_amd.recommend
  -meta_paths FILE                                      only the paths whose relation sequence matches a pattern of FILE (graph.parse_meta_paths)
  -kg_delta FILE                                        changes to the graph since -kg was written (`+|- \\t head \\t relation \\t tail` per line,
                                                        graph.read_delta): the graph goes to the device as -kg holds it and is updated there in place
                                                        before the split is made: the output is that of a -kg file with the delta folded in
Output: the two lines of eval_score.py (`hit scores`, `ndcg scores`, k = 1..15), then `samples \\t unreachable \\t zero`: the held pairs evaluated, those
that never reached the ranking stage (misses), and the zero samples (misses); with -eval_negatives N > 0 a fourth field `short`: the ranked samples with
fewer than N negatives."""
import argparse
import sys

import numpy as np

from . import evalrank, graph, model
from .pathformat import Vocabs


def main(argv=None, out=sys.stdout):
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False)   # (-h would swallow -holdout; the model flags' parser answers -h)
    p.add_argument("-model_path", default=""); p.add_argument("-gpu_id", type=int, default=-1); p.add_argument("-top_k", type=int, default=2)
    p.add_argument("-min_hops", type=int, default=1)
    argv = list(sys.argv[1:] if argv is None else argv)
    kg_delta = ""   # (taken out by hand: a -kg_delta in this parser would make argparse read the model flags' -kg as its prefix)
    if "-kg_delta" in argv:
        at = argv.index("-kg_delta")
        if at + 1 >= len(argv):
            p.error("-kg_delta needs a file")
        kg_delta = argv[at + 1]
        del argv[at:at + 2]
    args, rest = p.parse_known_args(argv)
    params = model.parse_flags(rest, gamma_beside=None)
    model.check_gamma(params.gamma, model.reducer_of_score_flag(args.top_k), "-top_k", p.error)
    if not params.kg or params.holdout <= 0:
        p.error("needs -kg triples.tsv -vocab_dir DIR -interaction_rel NAME and -holdout SHARE (above 0)")
    params.reducer, params.initModel, params.gpuid = model.reducer_of_score_flag(args.top_k), args.model_path, args.gpu_id
    kg = graph.KnowledgeGraph.from_triples(graph.read_triples(params.kg), Vocabs(params.vocab_dir), params.numEntityTypes)
    if (kg.Vt, kg.Ve, kg.Vr) != (params.entityTypeVocabSize, params.entityVocabSize, params.relationVocabSize):
        sys.exit("the vocabularies hold %d types, %d entities, %d relations; the model flags say %d, %d, %d"
                 % (kg.Vt, kg.Ve, kg.Vr, params.entityTypeVocabSize, params.entityVocabSize, params.relationVocabSize))
    if params.meta_paths:
        with open(params.meta_paths) as f:
            kg.patterns = graph.parse_meta_paths(f, kg)

    def split():
        train_kg, held = kg.holdout(params.interaction_rel, 1.0 - params.holdout, params.holdout_seed)
        if len(held) == 0:
            sys.exit("nothing was held out: relation %s has too few edges for -holdout %g" % (params.interaction_rel, params.holdout))
        return train_kg, held, np.unique(train_kg.interactions(params.interaction_rel)[:, 1])

    if not kg_delta:
        train_kg, held, catalogue = split()
    eng = model.build_engine(params)
    try:
        if kg_delta:   # the whole graph on the device as -kg holds it, edited in place; the split is the updated graph's
            full = kg.on(eng)
            kg.apply(*graph.read_delta(kg_delta, kg))
            full.free()
            train_kg, held, catalogue = split()
        res = graph.evaluate_from_graph(eng, train_kg, held, eng.sampler(catalogue), min_hops=args.min_hops, max_hops=params.max_hops, max_paths=params.max_paths,
                                        walks=params.walks, seed=params.sampleSeed, max_candidates=params.max_candidates, max_users=params.eval_users,
                                        eval_negatives=params.eval_negatives)
    finally:
        eng.close()
    for line in evalrank.format_metric_lines(res["hits"], res["ndcgs"]):
        out.write(line)
    out.write("%d\t%d\t%d" % (res["n"], res["n_unreachable"], res["n_zero"]) + ("\t%d" % res["n_short"] if params.eval_negatives > 0 else "") + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
