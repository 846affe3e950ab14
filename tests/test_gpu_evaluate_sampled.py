"""gpu: sampled held-out evaluation from a graph (graph.evaluate_from_graph eval_negatives > 0; the reference's sample.py / eval_score.py protocol) against
the same chain spelt out with the host twin of the sampling stage, board_read and kprn_host_rank_groups, on graph D of tests/candidates_top_ref.py with a
small randomly initialised model (the set-up of tests/test_gpu_evaluate_graph.py, built again here), and the two command lines against the function.
Every comparison is exact."""
import io
import json

import numpy as np
import pytest

from kprn_amd import _ffi, evalrank, graph as kgraph
from kprn_amd.pathformat import Vocabs

from . import candidates_top_ref as tref

pytestmark = pytest.mark.gpu

SHAPE = (16, 32, 16, 64, 2)   # dt, de, dr, H, L
HIST_LEN = 15
# The held users of this split have d (candidates that are no held items) in two clusters, 143 .. 144 and 169 .. 177, so at N = 100 every sample takes the
# d > N branch; N = 160 lies between the clusters and has both branches (d <= N: the whole of D) among the users of one call
SPLIT = 160
NEGATIVES = (8, 100, SPLIT, 4095)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """graph D as a triples file with vocabularies (entity e<k> has id k; relations 1..4 are rate, _rate, also, _also), its 80/20 split, a saved model"""
    tmp = tmp_path_factory.mktemp("evaluate_sampled")
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
    train_kg, held = kg.holdout("rate", 0.8, 1)
    held = held[np.lexsort((held[:, 1], held[:, 0]))]
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
    """the reference chain, once per (N, max_candidates, seed): every held user in one call; the candidates from the device, the samples and the cut list
    from the host twin, kprn_find_paths on that list, the scores read back from the board -> dict(scores, members, goff, rows (the held row of every
    group), n_short, d (per user: its rows that are no held items))"""
    memo = {}

    def get(n_neg, cap=0, seed=1):
        if (n_neg, cap, seed) not in memo:
            eng, gr, held = world["eng"], world["train_kg"].on(world["eng"]), world["held"]
            users = np.unique(held[:, 0])
            toff = np.searchsorted(held[:, 0], np.concatenate([users, [users[-1] + 1]])).astype(np.int64)
            pairs, gc = eng.find_candidates(gr, world["sampler"], users, 1, 3, True, cap=cap)
            first = np.concatenate([[0], np.cumsum(gc)])
            d = np.array([gc[b] - np.isin(pairs[first[b]:first[b + 1], 1], held[toff[b]:toff[b + 1], 1]).sum() for b in range(len(users))])
            tw = _ffi.host_sample_eval_groups(pairs, world["kg"].Ve, gc, toff, held[:, 1], n_neg, seed, 0)
            batch, counts, _ = eng.find_paths(gr, tw["pairs"], 1, 3, 28, 4)
            try:
                eng.forward_async(batch, 1)
                eng.board_reserve(batch.B)
                eng.board_put(0, batch.B)
                scores = eng.board_read(0, batch.B)
            finally:
                batch.free()
            line = np.full(len(tw["pairs"]), -1, np.int64)
            line[counts > 0] = np.arange(int((counts > 0).sum()))
            members, goff, rows, n_short = [], [0], [], 0
            for k in range(len(held)):
                if tw["target_rows"][k] < 0 or line[tw["target_rows"][k]] < 0:
                    continue
                neg = line[tw["neg_rows"][k, :tw["n_drawn"][k]]]
                neg = neg[neg >= 0]
                members += [line[tw["target_rows"][k]]] + list(neg)
                goff.append(len(members)); rows.append(k)
                n_short += len(neg) < n_neg
            memo[(n_neg, cap, seed)] = dict(scores=scores, members=np.array(members, np.int64), goff=np.array(goff, np.int64), rows=np.array(rows), n_short=n_short,
                                            d=d)
        return memo[(n_neg, cap, seed)]
    return get


def expected(world, c, mode, hist_len=HIST_LEN):
    res = _ffi.host_rank_groups(c["scores"], c["goff"], members=c["members"], pos=np.zeros(len(c["rows"]), np.int32), mode=mode, hist_len=hist_len)
    places = np.full(len(world["held"]), kgraph.PLACE_UNREACHABLE, np.int32)
    places[c["rows"]] = res["ranks"]
    hist = res["hist"].copy()
    hist[hist_len] += (places == kgraph.PLACE_UNREACHABLE).sum()
    return places, hist


def same_result(got, world, c, mode):
    places, hist = expected(world, c, mode)
    hits, ndcgs, n = evalrank.metrics_from_hist(hist, HIST_LEN)
    assert np.array_equal(got["held"], world["held"]) and np.array_equal(got["places"], places)
    assert np.array_equal(got["hist"], hist) and got["n"] == n == len(places) and got["hits"] == hits and got["ndcgs"] == ndcgs
    assert got["n_unreachable"] == int((places == kgraph.PLACE_UNREACHABLE).sum()) and got["n_short"] == c["n_short"]
    assert got["n_zero"] == int((places == _ffi.RANK_ZERO_GROUP).sum())


@pytest.mark.parametrize("mode", [_ffi.RANK_PRINTED, _ffi.RANK_RAW])
@pytest.mark.parametrize("n_neg", NEGATIVES)
def test_sampled_evaluation_equals_the_reference_chain(world, chain, n_neg, mode):
    c = chain(n_neg)
    got = kgraph.evaluate_from_graph(world["eng"], world["train_kg"], world["held"], world["sampler"], mode=mode, eval_negatives=n_neg)
    same_result(got, world, c, mode)
    sizes = np.diff(c["goff"]) - 1
    assert len(c["rows"]) > 100 and sizes.max() <= n_neg
    print("N", n_neg, "mode", mode, "ranked", len(c["rows"]), "unreachable", got["n_unreachable"], "short", got["n_short"], "d", c["d"].min(), c["d"].max(),
          "hit@10", got["hits"][10])
    if n_neg == SPLIT:                                  # both branches of the rule occur among the held users
        assert (c["d"] <= SPLIT).any() and (c["d"] > SPLIT).any(), (c["d"].min(), c["d"].max())
        assert 0 < got["n_short"] < len(c["rows"])
    if n_neg <= 100:
        assert got["n_short"] == 0
    if n_neg == 4095:
        assert got["n_short"] == len(c["rows"])


def test_the_chunking_of_users_does_not_show(world, chain):
    eng, sm = world["eng"], world["sampler"]
    one = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, users_per_call=1, eval_negatives=SPLIT)
    many = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, users_per_call=64, eval_negatives=SPLIT)
    assert np.array_equal(one["places"], many["places"]) and np.array_equal(one["hist"], many["hist"]) and one["n_short"] == many["n_short"]
    same_result(one, world, chain(SPLIT), _ffi.RANK_PRINTED)


def test_with_the_candidate_cap_and_another_seed(world, chain):
    eng, sm = world["eng"], world["sampler"]
    got = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, users_per_call=5, max_candidates=8, eval_negatives=8)
    same_result(got, world, chain(8, cap=8), _ffi.RANK_PRINTED)
    assert got["n_unreachable"] > kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, eval_negatives=8)["n_unreachable"]
    other = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, seed=2, eval_negatives=8)
    same_result(other, world, chain(8, seed=2), _ffi.RANK_PRINTED)
    assert not np.array_equal(chain(8, seed=2)["members"], chain(8)["members"])        # another seed, other samples


def test_zero_negatives_is_the_full_protocol(world):
    eng, sm = world["eng"], world["sampler"]
    a = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, max_candidates=64)
    b = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, max_candidates=64, eval_negatives=0)
    assert sorted(a) == sorted(b) and "n_short" not in b
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    with pytest.raises(ValueError):
        kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, eval_negatives=4096)


def test_the_evaluate_command_line(world):
    from kprn_amd import evaluate as cli
    flags = world["flags"] + ["-gpu_id", "0", "-top_k", "2", "-model_path", str(world["tmp"] / "model"), "-holdout", "0.2", "-holdout_seed", "1"]
    for extra, kw in ((["-eval_negatives", "100"], dict(eval_negatives=100)),
                      (["-eval_negatives", "8", "-max_candidates", "8", "-eval_users", "7"], dict(eval_negatives=8, max_candidates=8, max_users=7))):
        buf = io.StringIO()
        assert cli.main(flags + extra, out=buf) == 0
        want = kgraph.evaluate_from_graph(world["eng"], world["train_kg"], world["held"], world["sampler"], **kw)
        lines = evalrank.format_metric_lines(want["hits"], want["ndcgs"])
        assert buf.getvalue() == lines[0] + lines[1] + "%d\t%d\t%d\t%d\n" % (want["n"], want["n_unreachable"], want["n_zero"], want["n_short"])
    buf = io.StringIO()                                 # 0: byte for byte the output without the flag
    assert cli.main(flags + ["-eval_negatives", "0", "-eval_users", "7"], out=buf) == 0
    plain = io.StringIO()
    assert cli.main(flags + ["-eval_users", "7"], out=plain) == 0
    assert buf.getvalue() == plain.getvalue() and len(plain.getvalue().splitlines()[2].split("\t")) == 3
    for bad in (["-eval_negatives", "4096"], ["-eval_negatives", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(flags + bad, out=io.StringIO())


def test_the_train_command_line_with_sampled_evaluation(world, capsys):
    from kprn_amd import train
    tmp = world["tmp"]
    flags = world["flags"] + ["-gpuid", "0", "-numEpochs", "1", "-saveFrequency", "1", "-evaluationFrequency", "1", "-minibatch", "128", "-useAdam", "1",
                              "-topK", "2", "-negatives", "2", "-sampleSeed", "3", "-holdout", "0.2", "-eval_negatives", "100", "-model", str(tmp / "trained")]
    assert train.main(flags) == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("evaluation at epoch")]
    assert [l.split(" over ")[0] for l in lines] == ["evaluation at epoch 0", "evaluation at epoch 1"]
    eng = _ffi.Engine(world["kg"].Vt, world["kg"].Ve, world["kg"].Vr, *SHAPE)
    try:
        eng.load(str(tmp / "trained-latest"))
        sm = eng.sampler(np.unique(world["train_kg"].interactions("rate")[:, 1]))
        want = kgraph.evaluate_from_graph(eng, world["train_kg"], world["held"], sm, min_hops=2, seed=3, eval_negatives=100)
    finally:
        eng.close()
    h, d = want["hits"], want["ndcgs"]
    assert lines[1] == ("evaluation at epoch 1 over %d samples: " % want["n"] + "  ".join("hit@%d %.5f ndcg@%d %.5f" % (k, h[k], k, d[k]) for k in (1, 5, 10, 15))
                        + "  unreachable %d  short %d" % (want["n_unreachable"], want["n_short"]))
    with pytest.raises(SystemExit):
        train.main([f for f in flags if f not in ("-holdout", "0.2")])                 # -eval_negatives needs -holdout
    capsys.readouterr()
