"""`python -m kprn_amd.recommend <flags>`: which of the items in -items -- or, without -items, which items of the whole catalogue -- for -user, from a
knowledge graph and a checkpoint, and why (an extension; the reference mines paths offline and scores files).  A thin command line over graph.recommend.

Flags: those of `python -m kprn_amd.score` that shape and load the model (-model_path, -top_k, -gpu_id and the OneModel flags; the TopK reducer's K is the
model flag -K here, because -k is the number of items to return), plus
  -kg triples.tsv      the graph: `head \\t relation \\t tail` names per line, directed (list inverse edges yourself)
  -vocab_dir DIR       entity_type_id.txt, all_relation_id.txt, all_entity_id.txt, entity_to_type.txt, domain-label
  -user U  -items FILE the user's entity name; candidate item names, one per line
  -interaction_rel R [-seen 0]   without -items: the catalogue is every item an edge of relation R leads to, and the candidates are those the graph
                       reaches from the user in -min_hops .. min(-max_hops, 3) hops, found on the device; -seen 1 keeps the items the user already has an edge to
  -max_candidates N    without -items: only the user's N strongest candidates by path count are scored and ranked (0 = all of them)
  -k K                 items to return;  -explain_paths M  strongest paths printed per item
  -min_hops / -max_hops / -max_paths   the finder's limits (1, 3, 28)
  -walks N [-sampleSeed 1]             -max_hops 4 or 5: the paths of more than 3 hops are sampled, N walks (1..256) per item and hop count
  -meta_paths FILE                     only the paths whose relation sequence matches a pattern of FILE count: one pattern per line, positions separated
                       by blanks, a position `*` or relation names joined by `|` (graph.parse_meta_paths; include/kprn.h "meta-paths")
  -kg_delta FILE                       changes to the graph since -kg was written, one per line: `+ \\t head \\t relation \\t tail` adds an edge,
                       `- \\t head \\t relation \\t tail` removes one (relation `*`: every relation between the two); graph.read_delta.  The graph goes to
                       the device as -kg holds it and is updated there in place (include/kprn.h "updating a graph in place") before anything is found:
                       the output is that of a -kg file with the delta folded in
Output, tab separated: one line `rank, item, %.5f score, paths kept, paths found` per item, then one line `rank, place, %.5f weight, %.6g score, path`
per explained path (the path as scoring.format_path prints it)."""
import argparse
import sys

import numpy as np

from . import graph, model, scoring
from .pathformat import Vocabs


def main(argv=None, out=sys.stdout):
    p = argparse.ArgumentParser()
    p.add_argument("-model_path", default=""); p.add_argument("-gpu_id", type=int, default=-1); p.add_argument("-top_k", type=int, default=2)
    p.add_argument("-kg", required=True); p.add_argument("-vocab_dir", required=True)
    p.add_argument("-user", required=True); p.add_argument("-items", default="")
    p.add_argument("-k", type=int, default=10); p.add_argument("-explain_paths", type=int, default=3)
    p.add_argument("-min_hops", type=int, default=1); p.add_argument("-max_hops", type=int, default=3); p.add_argument("-max_paths", type=int, default=28)
    p.add_argument("-walks", type=int, default=0)
    p.add_argument("-interaction_rel", default=""); p.add_argument("-seen", type=int, default=0, choices=(0, 1))
    p.add_argument("-max_candidates", type=int, default=0)
    p.add_argument("-meta_paths", default=""); p.add_argument("-kg_delta", default="")
    args, rest = p.parse_known_args(argv)
    model.check_walks(args.max_hops, args.walks, p.error)
    if args.max_candidates and args.items:
        p.error("-max_candidates caps the candidates found in the graph and cannot be combined with -items (a list of candidates)")
    if not 0 <= args.max_candidates <= 2**31 - 1:
        p.error("-max_candidates must be in 0 .. 2^31 - 1")
    if not args.items and not args.interaction_rel:
        p.error("-kg needs -vocab_dir DIR (the vocabulary files) and -interaction_rel NAME (the relation of the user-item edges to train on)")   # (train -kg's)
    if not 1 <= args.explain_paths <= 32:
        sys.exit("-explain_paths must be in 1..32")
    if not 1 <= args.k <= 64:
        sys.exit("-k must be in 1..64")
    params = model.parse_flags(rest, gamma_beside=None)
    model.check_gamma(params.gamma, model.reducer_of_score_flag(args.top_k), "-top_k", p.error)
    params.reducer, params.initModel, params.gpuid = model.reducer_of_score_flag(args.top_k), args.model_path, args.gpu_id
    kg = graph.KnowledgeGraph.from_triples(graph.read_triples(args.kg), Vocabs(args.vocab_dir), params.numEntityTypes)
    if (kg.Vt, kg.Ve, kg.Vr) != (params.entityTypeVocabSize, params.entityVocabSize, params.relationVocabSize):
        sys.exit("the vocabularies hold %d types, %d entities, %d relations; the model flags say %d, %d, %d"
                 % (kg.Vt, kg.Ve, kg.Vr, params.entityTypeVocabSize, params.entityVocabSize, params.relationVocabSize))
    if args.meta_paths:
        with open(args.meta_paths) as f:
            kg.patterns = graph.parse_meta_paths(f, kg)

    def candidates():
        """-> (the -items list or None, the catalogue or None) of the graph as it stands"""
        if args.items:
            with open(args.items) as f:
                return [kg.entity_id(l.strip()) for l in f if l.strip()], None
        positives = kg.interactions(args.interaction_rel)
        if len(positives) == 0:
            sys.exit("the graph has no edge of relation %s" % args.interaction_rel)
        return None, np.unique(positives[:, 1])

    if not args.kg_delta:
        items, catalogue = candidates()
    eng = model.build_engine(params)
    try:
        if args.kg_delta:   # the graph on the device as -kg holds it, then edited in place; the catalogue is the updated graph's
            kg.on(eng)
            kg.apply(*graph.read_delta(args.kg_delta, kg))
            items, catalogue = candidates()
        sampler = None if catalogue is None else eng.sampler(catalogue)
        res = graph.recommend(eng, kg, kg.entity_id(args.user), items, args.k, args.explain_paths, args.min_hops, args.max_hops,
                              args.max_paths, walks=args.walks, seed=params.sampleSeed, sampler=sampler, exclude_adjacent=not args.seen,
                              max_candidates=args.max_candidates)
    finally:
        eng.close()
    for r in res:
        out.write("%d\t%s\t%.5f\t%d\t%d\n" % (r["rank"], kg.entity_name(r["item"]), r["score"], r["n_paths"], r["found"]))
        for place, (ids, w, s) in enumerate(r["paths"]):
            out.write("%d\t%d\t%.5f\t%.6g\t%s\n" % (r["rank"], place, w, s, scoring.format_path(ids, kg.Ve)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
