"""gpu: held-out evaluation from a graph.  graph.evaluate_from_graph against the same chain ending in board_read and the numpy restatement of the rule
(tests/rank_targets_ref.py), on graph D of tests/candidates_top_ref.py with a small randomly initialised model, and the two command lines against
evaluate_from_graph.  Every comparison is exact."""
import io
import json

import numpy as np
import pytest

from kprn_amd import _ffi, evalrank, graph as kgraph
from kprn_amd.pathformat import Vocabs

from . import candidates_top_ref as tref
from . import rank_targets_ref as ref

pytestmark = pytest.mark.gpu

SHAPE = (16, 32, 16, 64, 2)   # dt, de, dr, H, L
HIST_LEN = 15


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """graph D as a triples file with vocabularies (entity e<k> has id k; relations 1..4 are rate, _rate, also, _also), its 80/20 split, a saved model"""
    tmp = tmp_path_factory.mktemp("evaluate")
    g = tref.graph_d()[0]
    vdir = tmp / "vocab"
    vdir.mkdir()
    ents = ["e%d" % k for k in range(1, g["Ve"])]
    rels = ["rate", "_rate", "also", "_also"]
    is_user = lambda k: k <= 24 or 325 <= k <= 345
    w = lambda name, rows: (vdir / name).write_text("".join("%s\t%s\n" % r for r in rows))
    w("all_entity_id.txt", [(n, k) for k, n in enumerate(ents + ["#UNK_ENTITY", "#PAD_TOKEN"])])
    w("entity_type_id.txt", [(n, k) for k, n in enumerate(["user", "item", "#UNK_ENTITY_TYPE", "#PAD_TOKEN"])])
    w("all_relation_id.txt", [(n, k) for k, n in enumerate(rels + ["#UNK_RELATION", "#END_RELATION", "#PAD_TOKEN"])])
    w("entity_to_type.txt", [("e%d" % k, "user" if is_user(k) else "item") for k in range(1, g["Ve"])])
    json.dump({"domain": {"1": 1, "-1": 0}, "name": "label"}, open(str(vdir / "domain-label"), "w"))
    triples = [("e%d" % s, rels[r - 1], "e%d" % d) for s, d, r in zip(g["src"], g["dst"], g["rel"])]
    (tmp / "kg.tsv").write_text("".join("%s\t%s\t%s\n" % t for t in triples))
    kg = kgraph.KnowledgeGraph.from_triples(triples, Vocabs(str(vdir)), 1)
    assert np.array_equal(kg.src, g["src"]) and np.array_equal(kg.dst, g["dst"]) and np.array_equal(kg.rel, g["rel"])
    train_kg, held = kg.holdout("rate", 0.8, 1)
    eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, *SHAPE, param_init=0.35, seed=5)
    eng.save(str(tmp / "model"))
    flags = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1, "-kg", tmp / "kg.tsv", "-vocab_dir", vdir, "-interaction_rel", "rate"]
    sampler = eng.sampler(np.unique(train_kg.interactions("rate")[:, 1]))
    yield dict(tmp=tmp, kg=kg, train_kg=train_kg, held=held, eng=eng, sampler=sampler, flags=[str(f) for f in flags])
    eng.close()


@pytest.fixture(scope="module")
def chain(world):
    """the reference chain, once per max_candidates: every held user in one call, the scores read back from the board -> per user, its surviving items
    in board order and their scores"""
    memo = {}

    def get(cap):
        if cap not in memo:
            eng, gr = world["eng"], world["train_kg"].on(world["eng"])
            users = np.unique(world["held"][:, 0])
            pairs, gc = eng.find_candidates(gr, world["sampler"], users, 1, 3, True, cap=cap)
            batch, counts, _ = eng.find_paths_of_candidates(gr, len(pairs), 1, 3, 28, 4)
            try:
                eng.forward_async(batch, 1)
                eng.board_reserve(batch.B)
                eng.board_put(0, batch.B)
                scores = eng.board_read(0, batch.B)
            finally:
                batch.free()
            alive = pairs[counts > 0]
            assert len(alive) == len(scores)
            memo[cap] = {int(u): (alive[alive[:, 0] == u, 1], scores[alive[:, 0] == u]) for u in users}
        return memo[cap]
    return get


def expected(world, per_user, mode, users=None):
    """places of the held rows (PLACE_UNREACHABLE where the pair did not survive), the histogram with the unreachable pairs in hist[hist_len]"""
    held = world["held"] if users is None else world["held"][np.isin(world["held"][:, 0], users)]
    places = np.full(len(held), kgraph.PLACE_UNREACHABLE, np.int32)
    hist = np.zeros(HIST_LEN + 4, np.int64)
    for u in np.unique(held[:, 0]):
        items, scores = per_user[int(u)]
        rows = np.nonzero(held[:, 0] == u)[0]
        there = np.isin(held[rows, 1], items)
        t = np.sort(np.nonzero(np.isin(items, held[rows, 1]))[0])
        if len(items) == 0:
            continue
        p, inv = ref.group_places(scores, t, mode)
        assert inv == 0
        for item, v in zip(items[t], p):
            places[rows[held[rows, 1] == item]] = v
            hist[HIST_LEN + 1 if v < 0 else min(int(v), HIST_LEN)] += 1
        assert there.sum() == len(t)
    hist[HIST_LEN] += (places == kgraph.PLACE_UNREACHABLE).sum()
    return held, places, hist


@pytest.mark.parametrize("mode", [ref.PRINTED, ref.RAW])
@pytest.mark.parametrize("cap", [0, 8])
def test_evaluate_from_graph_equals_the_reference_chain(world, chain, cap, mode):
    held, places, hist = expected(world, chain(cap), mode)
    hits, ndcgs, n = evalrank.metrics_from_hist(hist, HIST_LEN)
    n_users = len(np.unique(held[:, 0]))
    assert len(held) >= 300 and n_users >= 40 and n == len(held)
    for per in (1, 5, n_users):
        got = kgraph.evaluate_from_graph(world["eng"], world["train_kg"], world["held"], world["sampler"], users_per_call=per, max_candidates=cap, mode=mode)
        assert np.array_equal(got["held"], held) and np.array_equal(got["places"], places), per
        assert np.array_equal(got["hist"], hist) and got["n"] == n and got["hits"] == hits and got["ndcgs"] == ndcgs, per
        assert got["n_unreachable"] == int((places == kgraph.PLACE_UNREACHABLE).sum()) and got["n_zero"] == int((places == ref.ZERO).sum()), per
    print("cap", cap, "mode", mode, "n", n, "unreachable", got["n_unreachable"], "hit@10", hits[10])


def test_the_cap_cuts_targets_and_max_users_takes_the_first(world, chain):
    eng, sm = world["eng"], world["sampler"]
    full = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm)
    capped = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, max_candidates=8)
    assert capped["n_unreachable"] > full["n_unreachable"] and capped["n"] == full["n"] == len(world["held"])
    assert (full["places"] >= 0).sum() > 100                                          # the uncapped run ranks most held pairs
    users = np.unique(world["held"][:, 0])[:3]
    held, places, hist = expected(world, chain(0), ref.PRINTED, users)
    got = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, max_users=3, ks=[1, 15])
    assert np.array_equal(got["held"], held) and np.array_equal(got["places"], places) and np.array_equal(got["hist"], hist)
    assert sorted(got["hits"]) == [1, 15]


def test_the_evaluate_command_line(world):
    from kprn_amd import evaluate as cli
    flags = world["flags"] + ["-gpu_id", "0", "-top_k", "2", "-model_path", str(world["tmp"] / "model"), "-holdout", "0.2", "-holdout_seed", "1"]
    for extra, kw in (([], {}), (["-max_candidates", "8", "-eval_users", "7"], dict(max_candidates=8, max_users=7))):
        buf = io.StringIO()
        assert cli.main(flags + extra, out=buf) == 0
        want = kgraph.evaluate_from_graph(world["eng"], world["train_kg"], world["held"], world["sampler"], **kw)
        lines = evalrank.format_metric_lines(want["hits"], want["ndcgs"])
        assert buf.getvalue() == lines[0] + lines[1] + "%d\t%d\t%d\n" % (want["n"], want["n_unreachable"], want["n_zero"])
    with pytest.raises(SystemExit):
        cli.main(world["flags"] + ["-model_path", str(world["tmp"] / "model")], out=io.StringIO())      # no -holdout


def test_the_train_command_line_with_holdout(world, capsys):
    from kprn_amd import train
    tmp = world["tmp"]
    flags = world["flags"] + ["-gpuid", "0", "-numEpochs", "1", "-saveFrequency", "1", "-evaluationFrequency", "1", "-minibatch", "128", "-useAdam", "1",
                              "-topK", "2", "-negatives", "2", "-sampleSeed", "3", "-holdout", "0.2", "-max_candidates", "64", "-model", str(tmp / "trained")]
    assert train.main(flags) == 0
    out = capsys.readouterr().out
    assert "Training from the graph: %d positives" % len(world["train_kg"].interactions("rate")) in out
    assert "Held out: %d pairs" % len(world["held"]) in out
    lines = [l for l in out.splitlines() if l.startswith("evaluation at epoch")]
    assert [l.split(" over ")[0] for l in lines] == ["evaluation at epoch 0", "evaluation at epoch 1"]
    eng = _ffi.Engine(world["kg"].Vt, world["kg"].Ve, world["kg"].Vr, *SHAPE)
    try:
        eng.load(str(tmp / "trained-latest"))
        sm = eng.sampler(np.unique(world["train_kg"].interactions("rate")[:, 1]))
        want = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, min_hops=2, seed=3, max_candidates=64)
    finally:
        eng.close()
    h, d = want["hits"], want["ndcgs"]
    assert lines[1] == ("evaluation at epoch 1 over %d samples: " % want["n"] + "  ".join("hit@%d %.5f ndcg@%d %.5f" % (k, h[k], k, d[k]) for k in (1, 5, 10, 15))
                        + "  unreachable %d" % want["n_unreachable"])
    with pytest.raises(SystemExit):
        train.main([f for f in flags if f not in ("-kg", str(tmp / "kg.tsv"))])        # -holdout needs -kg
    capsys.readouterr()
