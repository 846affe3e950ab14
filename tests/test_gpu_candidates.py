"""gpu: kprn_find_candidates / kprn_read_candidates / kprn_find_paths_of_candidates against the host twin kprn_host_find_candidates (itself held to a brute
force by tests/test_candidates_host.py) and against kprn_find_paths on the list read back; the chain from a user to a recommendation without a candidate
list, its groups of more than 4096 members and its command line.  Every comparison is exact."""
import ctypes as C
import io
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph

from . import candidates_ref as cref
from . import path_find_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(dt=16, de=32, dr=16, H=64, L=2, F=3)


@pytest.fixture(scope="module")
def graphs():
    ga, ia, ua = cref.graph_a()
    gb, ib, ub, names = cref.graph_b()
    gc, ic, uc = cref.graph_c()
    return dict(A=(ga, ia, ua), B=(gb, ib, ub), C=(gc, ic, uc)), names


@pytest.fixture(scope="module")
def on_device(graphs):
    """one small engine per graph (the engine's Ve is the graph's), its graph and its catalogue in HBM"""
    made = {}

    def get(name):
        if name not in made:
            g, items, _ = graphs[0][name]
            eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, **SHAPE)
            made[name] = (eng, eng.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL), eng.sampler(items))
        return made[name]
    yield get
    for eng, _, _ in made.values():
        eng.close()


@pytest.fixture(scope="module")
def twin(graphs):
    """the host twin's (pairs [total, 2], group_counts [B]), computed once per argument set and left unchanged"""
    memo = {}

    def get(name, users, lo, hi, exclude, items=None):
        g, its, _ = graphs[0][name]
        its = its if items is None else items
        key = (name, users.tobytes(), lo, hi, exclude, its.tobytes())
        if key not in memo:
            cand, gc = _ffi.host_find_candidates(g["src"], g["dst"], g["rel"], g["Ve"], its, users, lo, hi, exclude, threads=8)
            pairs = np.stack([np.repeat(users, gc), cand], axis=1).astype(np.int32).reshape(-1, 2)
            pairs.setflags(write=False); gc.setflags(write=False)
            memo[key] = (pairs, gc)
        return memo[key]
    return get


def hub_of(graphs):
    return np.array([graphs[0]["A"][0]["cases"]["hub"]], np.int32)


@pytest.mark.parametrize("exclude", [0, 1])
@pytest.mark.parametrize("hops", cref.HOPS)
def test_device_equals_twin(graphs, on_device, twin, hops, exclude):
    for name, user_sets in (("A", (hub_of(graphs), graphs[0]["A"][2])), ("B", (graphs[0]["B"][2][:1], graphs[0]["B"][2]))):
        eng, gr, sm = on_device(name)
        for users in user_sets:
            want, want_gc = twin(name, users, hops[0], hops[1], exclude)
            pairs, gc = eng.find_candidates(gr, sm, users, hops[0], hops[1], exclude)
            assert np.array_equal(gc, want_gc), (name, len(users))
            assert pairs.shape == want.shape and np.array_equal(pairs, want), (name, len(users))


def test_device_equals_twin_on_c_two_users_of_266_words(graphs, on_device, twin):
    eng, gr, sm = on_device("C")
    users = graphs[0]["C"][2]
    for us in (users, users[::-1].copy(), np.array([8500, 8500, 8497], np.int32)):     # one user's bits must not reach the other's rows
        for exclude in (0, 1):
            want, want_gc = twin("C", us, 2, 2, exclude)
            pairs, gc = eng.find_candidates(gr, sm, us, 2, 2, exclude)
            assert np.array_equal(gc, want_gc) and np.array_equal(pairs, want)
    pairs, gc = eng.find_candidates(gr, sm, users, 2, 2, 1)
    assert gc.tolist() == [4200, 2800] and pairs[:4200, 1].tolist() == cref.c_expected(8500) and (pairs[:4200, 0] == 8500).all()


def test_same_result_twice_and_after_a_larger_call(graphs, on_device, twin):
    eng, gr, sm = on_device("A")
    g, items, users = graphs[0]["A"]
    small_items = items[:70].copy()                    # 2 full words and 6 bits
    small = eng.sampler(small_items)
    hub = hub_of(graphs)
    want, want_gc = twin("A", hub, 1, 3, 0, items=small_items)
    assert len(want) > 32
    for _ in range(2):
        big = eng.find_candidates(gr, sm, users, 1, 3, 0)                              # B = 28, M = 268
        assert np.array_equal(big[0], twin("A", users, 1, 3, 0)[0])
        pairs, gc = eng.find_candidates(gr, small, hub, 1, 3, 0)                       # B = 1, M = 70 in the scratch the larger call left
        assert np.array_equal(gc, want_gc) and np.array_equal(pairs, want)
    small.free()


@pytest.mark.parametrize("lo,hi,cap", [(1, 3, 5), (2, 3, 4096)])
def test_find_paths_of_candidates_equals_find_paths(graphs, on_device, lo, hi, cap):
    eng, gr, sm = on_device("A")
    users = graphs[0]["A"][2]
    pairs, gc = eng.find_candidates(gr, sm, users, lo, hi, True)
    total = len(pairs)
    assert total > 300
    batch, counts, found = eng.find_paths_of_candidates(gr, total, lo, hi, cap, 4)
    want_batch, want_counts, want_found = eng.find_paths(gr, pairs, lo, hi, cap, 4)
    try:
        assert (counts > 0).all() and batch.B == total                                 # the candidates are the pairs with found > 0: none is dropped
        assert np.array_equal(counts, want_counts) and np.array_equal(found, want_found)
        assert np.array_equal(batch.counts, want_batch.counts) and np.array_equal(batch.read_idx(), want_batch.read_idx())
    finally:
        batch.free(); want_batch.free()


def test_find_paths_of_candidates_with_sampled_hops(graphs, on_device):
    eng, gr, sm = on_device("A")
    users = graphs[0]["A"][2]
    pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, True)
    short, _, found3 = eng.find_paths_of_candidates(gr, len(pairs), 1, 3, 28, 4)
    short.free()
    batch, counts, found = eng.find_paths_of_candidates(gr, len(pairs), 1, 5, 28, 6, walks=8, seed=77, draw=3)
    want_batch, want_counts, want_found = eng.find_paths(gr, pairs, 1, 5, 28, 6, walks=8, seed=77, draw=3)
    try:
        assert np.array_equal(counts, want_counts) and np.array_equal(found, want_found) and found.sum() > found3.sum()   # (the sampled hops added paths)
        assert np.array_equal(batch.read_idx(), want_batch.read_idx())
    finally:
        batch.free(); want_batch.free()


def test_edges_no_candidate_no_list_and_a_refused_call(graphs, on_device):
    eng, gr, sm = on_device("A")
    g, items, users = graphs[0]["A"]
    fresh = _ffi.Engine(ref.VT, g["Ve"], ref.VR, **SHAPE)
    try:
        fgr = fresh.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL)
        with pytest.raises(_ffi.KprnError) as ei:
            fresh.find_paths_of_candidates(fgr, 0, 1, 3, 5, 4)
        assert ei.value.code == _ffi.E_ARG
        assert fresh.L.kprn_read_candidates(fresh.h, None, C.c_int64(0)) == _ffi.E_ARG
    finally:
        fresh.close()
    lonely = np.array([g["cases"]["lonely"][0], g["cases"]["unreachable"][0]], np.int32)
    pairs, gc = eng.find_candidates(gr, sm, lonely, 1, 3, False)
    assert pairs.shape == (0, 2) and gc.tolist() == [0, 0]
    batch, counts, found = eng.find_paths_of_candidates(gr, 0, 1, 3, 5, 4)
    assert batch is None and len(counts) == 0
    # a refused call writes nothing and leaves the earlier list readable
    pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, True)
    for kw, code in ((dict(min_hops=0), _ffi.E_ARG), (dict(max_hops=4), _ffi.E_ARG), (dict(min_hops=3, max_hops=2), _ffi.E_ARG),
                     (dict(users=np.zeros(0, np.int32)), _ffi.E_ARG), (dict(users=np.array([1, 0], np.int32)), _ffi.E_INDEX),
                     (dict(users=np.array([g["Ve"]], np.int32)), _ffi.E_INDEX)):
        a = dict(users=users, min_hops=1, max_hops=3)
        a.update(kw)
        out_gc = np.full(max(len(a["users"]), 1), -7, np.int32)
        total = C.c_int64(-7)
        rc = eng.L.kprn_find_candidates(eng.h, gr.ptr, sm.ptr, _ffi._fp(a["users"]), len(a["users"]), a["min_hops"], a["max_hops"], 1, _ffi._fp(out_gc), C.byref(total))
        assert rc == code and (out_gc == -7).all() and total.value == -7, kw
        back = np.zeros_like(pairs)
        assert eng.L.kprn_read_candidates(eng.h, _ffi._fp(back), C.c_int64(len(pairs))) == 0 and np.array_equal(back, pairs), kw
    assert eng.L.kprn_read_candidates(eng.h, _ffi._fp(back), C.c_int64(len(pairs) - 1)) == _ffi.E_ARG


def test_candidates_do_not_depend_on_what_hipmalloc_returns(graphs, twin):
    """the device calls in a fresh process with KPRN_POISON_ALLOC=1 (every new device allocation filled with 0xFF bytes), twice"""
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r)
        import numpy as np
        from kprn_amd import _ffi
        from tests import path_find_ref as ref, candidates_ref as cref
        g, items, users = cref.graph_a()
        eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, 16, 32, 16, 64, 2)
        gr = eng.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL)
        sm = eng.sampler(items)
        out = []
        for _ in range(2):
            for ex in (0, 1):
                pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, ex)
                b, c, f = eng.find_paths_of_candidates(gr, len(pairs), 1, 3, 5, 4)
                out.append([pairs.ravel().tolist(), gc.tolist(), int(b.B), bool((c > 0).all())])
                b.free()
        eng.close()
        print(json.dumps(out))
    """) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    users = graphs[0]["A"][2]
    for k, (rows, gc, nb, positive) in enumerate(json.loads(r.stdout.strip().splitlines()[-1])):
        want, want_gc = twin("A", users, 1, 3, k % 2)
        assert np.array_equal(np.array(rows, np.int32), want.ravel()) and np.array_equal(gc, want_gc) and nb == len(want) and positive


def same_recommendation(a, b):
    """two results of graph.recommend, field by field and bit by bit"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert {k: v for k, v in x.items() if k != "paths"} == {k: v for k, v in y.items() if k != "paths"}
        assert len(x["paths"]) == len(y["paths"])
        for (ids, w, s), (ids2, w2, s2) in zip(x["paths"], y["paths"]):
            assert np.array_equal(ids, ids2) and w == w2 and s == s2


def test_chain_equals_the_chain_fed_the_twins_candidates(graphs, on_device, twin):
    eng, gr, sm = on_device("A")
    c = graphs[0]["A"][0]["cases"]
    K, M = 4, 3
    three = [c["hub"], c["hub_next"][0], c["inside"][0]]
    singles = []
    for u in three:
        pairs, _ = twin("A", np.array([u], np.int32), 1, 3, 1)
        got = kgraph.recommend(eng, gr, u, None, K, M, sampler=sm)
        want = kgraph.recommend(eng, gr, u, pairs[:, 1], K, M)
        assert len(want) == min(K, len(pairs)) and len(want) >= 2
        same_recommendation(got, want)
        singles.append(want)
    together = kgraph.recommend_users(eng, gr, sm, three + [c["lonely"][0]], K, M)
    assert together[3] == []
    for got, want in zip(together, singles):
        same_recommendation(got, want)
    # the items the user already has stay candidates on request
    pairs, _ = twin("A", np.array([c["exact"][0]], np.int32), 1, 3, 0)
    same_recommendation(kgraph.recommend(eng, gr, c["exact"][0], None, K, M, sampler=sm, exclude_adjacent=False),
                        kgraph.recommend(eng, gr, c["exact"][0], pairs[:, 1], K, M))


@pytest.mark.parametrize("mode", [_ffi.RANK_PRINTED, _ffi.RANK_RAW])
def test_more_than_4096_candidates_are_ranked_as_one_group(graphs, on_device, mode):
    eng, gr, sm = on_device("C")
    K = 64
    got = kgraph.recommend_users(eng, gr, sm, [8500], K, 0, min_hops=2, max_hops=2, T=3, mode=mode)[0]
    scores = eng.board_read(0, 4200)                   # the chain's board: one score per candidate, in the list's order
    items = np.array(cref.c_expected(8500))
    assert np.isfinite(scores).all() and ((scores >= 0) & (scores <= 1)).all()
    key = np.rint(scores.astype(np.float64) * 1e5) if mode == _ffi.RANK_PRINTED else scores
    order = np.lexsort((np.arange(4200), -key.astype(np.float64)))[:K]                 # key descending, then index ascending
    assert (order >= 4096).any() and (order < 4096).any()                              # (winners from both sub-groups: the merge is exercised)
    assert [r["item"] for r in got] == items[order].tolist()
    assert [np.float32(r["score"]) for r in got] == scores[order].tolist()
    assert [r["rank"] for r in got] == list(range(K)) and all(r["n_paths"] == 1 and r["found"] == 1 and r["paths"] == [] for r in got)


def _cli_inputs(tmp_path):
    from kprn_amd.pathformat import Vocabs
    from .test_path_find_host import _write_vocab
    vdir = tmp_path / "vocab"
    vdir.mkdir()
    _write_vocab(str(vdir))
    triples = []
    for u, m in [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 0), (3, 4), (1, 4)]:
        triples += [("u%d" % u, "rate", "m%d" % m), ("m%d" % m, "_rate", "u%d" % u)]
    for m in (1, 2, 4):
        triples += [("m%d" % m, "act", "a0"), ("a0", "_act", "m%d" % m)]
    (tmp_path / "kg.tsv").write_text("".join("%s\t%s\t%s\n" % t for t in triples))
    kg = kgraph.KnowledgeGraph.from_triples(triples, Vocabs(str(vdir)), 1)
    eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, 16, 32, 16, 64, 2)
    try:
        eng.save(str(tmp_path / "model"))
    finally:
        eng.close()
    flags = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1, "-gpu_id", 0, "-top_k", 2, "-model_path", tmp_path / "model", "-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-user", "u0",
             "-k", 3, "-explain_paths", 2]
    return kg, [str(f) for f in flags]


def test_command_line_without_items(tmp_path, capsys):
    from kprn_amd import recommend as cli
    kg, flags = _cli_inputs(tmp_path)

    def run(extra):
        buf = io.StringIO()
        assert cli.main(flags + [str(x) for x in extra], out=buf) == 0
        return buf.getvalue()

    catalogue = np.unique(kg.interactions("rate")[:, 1])
    u0 = kg.entity_id("u0")
    for seen in (0, 1):
        cand, _ = _ffi.host_find_candidates(kg.src, kg.dst, kg.rel, kg.Ve, catalogue, [u0], 1, 3, not seen)
        names = [kg.entity_name(e) for e in cand]
        assert names == (["m2", "m4"] if not seen else ["m0", "m1", "m2", "m4"])
        path = tmp_path / ("items%d.txt" % seen)
        path.write_text("\n".join(names) + "\n")
        with_items = run(["-items", path])
        assert len(with_items.splitlines()) >= len(names) and run(["-interaction_rel", "rate", "-seen", seen]) == with_items
        # -items: what the chain behind it returns, in the lines the command has always printed
        eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, 16, 32, 16, 64, 2)
        try:
            eng.load(str(tmp_path / "model"))
            res = kgraph.recommend(eng, kg, u0, cand, 3, 2)
        finally:
            eng.close()
        from kprn_amd import scoring
        want = ""
        for r in res:
            want += "%d\t%s\t%.5f\t%d\t%d\n" % (r["rank"], kg.entity_name(r["item"]), r["score"], r["n_paths"], r["found"])
            for place, (ids, w, s) in enumerate(r["paths"]):
                want += "%d\t%d\t%.5f\t%.6g\t%s\n" % (r["rank"], place, w, s, scoring.format_path(ids, kg.Ve))
        assert with_items == want
    assert run(["-interaction_rel", "rate"]) == run(["-interaction_rel", "rate", "-seen", 0])
    with pytest.raises(SystemExit):
        cli.main(flags, out=io.StringIO())
    assert "-interaction_rel NAME (the relation of the user-item edges to train on)" in capsys.readouterr().err
