"""gpu: kprn_find_candidates_top / kprn_read_candidate_paths against the host twin kprn_host_find_candidates_top (itself held to a reference made of the
finder's twin and np.lexsort by tests/test_candidates_top_host.py), against the finder's own count pass on the list, and the capped chain from a user to a
recommendation with its command line.  Every comparison is exact."""
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
from . import candidates_top_ref as tref
from . import path_find_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(dt=16, de=32, dr=16, H=64, L=2, F=3)
CAPS = (1, 7, 64, 201, tref.CAP_MAX)


@pytest.fixture(scope="module")
def graphs():
    return dict(D=tref.graph_d(), C=cref.graph_c())


@pytest.fixture(scope="module")
def on_device(graphs):
    """one small engine per graph (the engine's Ve is the graph's), its graph and its catalogue in HBM"""
    made = {}

    def get(name):
        if name not in made:
            g, items, _ = graphs[name]
            eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, **SHAPE)
            made[name] = (eng, eng.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL), eng.sampler(items))
        return made[name]
    yield get
    for eng, _, _ in made.values():
        eng.close()


@pytest.fixture(scope="module")
def twin(graphs):
    """the host twin's (pairs [total, 2], group_counts [B], n_paths [total]), computed once per argument set and left unchanged"""
    memo = {}

    def get(name, users, lo, hi, exclude, cap):
        g, items, _ = graphs[name]
        key = (name, users.tobytes(), lo, hi, exclude, cap)
        if key not in memo:
            cand, gc, n_paths = _ffi.host_find_candidates_top(g["src"], g["dst"], g["rel"], g["Ve"], items, users, lo, hi, cap, exclude, threads=8)
            pairs = np.stack([np.repeat(users, gc), cand], axis=1).astype(np.int32).reshape(-1, 2)
            for a in (pairs, gc, n_paths):
                a.setflags(write=False)
            memo[key] = (pairs, gc, n_paths)
        return memo[key]
    return get


def device_equals_twin(eng, gr, sm, want, users, lo, hi, exclude, cap):
    pairs, gc = eng.find_candidates(gr, sm, users, lo, hi, exclude, cap=cap)
    assert np.array_equal(gc, want[1]) and eng._cand_total == len(want[0]), (lo, hi, exclude, cap)
    assert pairs.shape == want[0].shape and np.array_equal(pairs, want[0]), (lo, hi, exclude, cap)
    n_paths = eng.candidate_path_counts()
    assert n_paths.dtype == np.int64 and np.array_equal(n_paths, want[2]), (lo, hi, exclude, cap)


@pytest.mark.parametrize("exclude", [0, 1])
@pytest.mark.parametrize("hops", [(1, 3), (3, 3)])
def test_device_equals_twin_on_d(graphs, on_device, twin, hops, exclude):
    eng, gr, sm = on_device("D")
    users = graphs["D"][2]
    for cap in CAPS:
        device_equals_twin(eng, gr, sm, twin("D", users, hops[0], hops[1], exclude, cap), users, hops[0], hops[1], exclude, cap)


def test_one_user_per_call_and_a_small_call_after_a_large_one(graphs, on_device, twin):
    eng, gr, sm = on_device("D")
    g, _, users = graphs["D"]
    singles = [np.array([g["cases"]["hub"]], np.int32), np.array([1], np.int32)]
    for one in singles:
        for cap in CAPS:
            device_equals_twin(eng, gr, sm, twin("D", one, 1, 3, 1, cap), one, 1, 3, 1, cap)
    for one in singles:                                # the grow-only block holds the 26-user call's sums when the 1-user call starts
        device_equals_twin(eng, gr, sm, twin("D", users, 1, 3, 0, 64), users, 1, 3, 0, 64)
        device_equals_twin(eng, gr, sm, twin("D", one, 3, 3, 1, 7), one, 3, 3, 1, 7)


def test_capped_candidates_do_not_depend_on_what_hipmalloc_returns(graphs, twin):
    """the device calls in a fresh process with KPRN_POISON_ALLOC=1 (every new device allocation filled with 0xFF bytes), twice"""
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r)
        import numpy as np
        from kprn_amd import _ffi
        from tests import path_find_ref as ref, candidates_top_ref as tref
        g, items, users = tref.graph_d()
        eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, 16, 32, 16, 64, 2)
        gr = eng.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL)
        sm = eng.sampler(items)
        out = []
        for _ in range(2):
            for ex in (0, 1):
                pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, ex, cap=64)
                n_paths = eng.candidate_path_counts()
                b, c, f = eng.find_paths_of_candidates(gr, len(pairs), 1, 3, 5, 4)
                out.append([pairs.ravel().tolist(), gc.tolist(), n_paths.tolist(), int(b.B), f.tolist()])
                b.free()
        eng.close()
        print(json.dumps(out))
    """) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    users = graphs["D"][2]
    for k, (rows, gc, n_paths, nb, found) in enumerate(json.loads(r.stdout.strip().splitlines()[-1])):
        want, want_gc, want_n = twin("D", users, 1, 3, k % 2, 64)
        assert np.array_equal(np.array(rows, np.int32), want.ravel()) and np.array_equal(gc, want_gc) and np.array_equal(n_paths, want_n)
        assert nb == len(want) and np.array_equal(found, want_n)


@pytest.mark.parametrize("cap", [7, 64, tref.CAP_MAX])
def test_path_counts_are_the_finders_found(graphs, on_device, cap):
    eng, gr, sm = on_device("D")
    users = graphs["D"][2]
    pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, True, cap=cap)
    n_paths = eng.candidate_path_counts()
    batch, counts, found = eng.find_paths_of_candidates(gr, len(pairs), min_hops=1, max_hops=3, max_paths=5, T=4, walks=0)
    try:
        assert found.dtype == np.int64 and np.array_equal(found, n_paths) and n_paths.max() > 255
        assert (counts > 0).all() and batch.B == len(pairs)                            # no pair is dropped
    finally:
        batch.free()


def test_graph_c_two_users_of_more_than_one_chunk(graphs, on_device, twin):
    eng, gr, sm = on_device("C")
    users = graphs["C"][2]
    for cap in (300, 4199):
        want = twin("C", users, 2, 2, 1, cap)
        device_equals_twin(eng, gr, sm, want, users, 2, 2, 1, cap)
    pairs, gc = eng.find_candidates(gr, sm, users, 2, 2, 1, cap=300)
    assert gc.tolist() == [300, 300] and pairs[:300, 1].tolist() == list(range(2, 601, 2)) and pairs[300:, 1].tolist() == list(range(3, 901, 3))
    pairs, gc = eng.find_candidates(gr, sm, users, 2, 2, 1, cap=4199)
    assert gc.tolist() == [4199, 2800] and pairs[:4199, 1].tolist() == list(range(2, 8399, 2)) and pairs[4199:, 1].tolist() == cref.c_expected(8497)
    assert (pairs[:4199, 0] == 8500).all() and (eng.candidate_path_counts() == 1).all()


def test_a_refused_call_keeps_the_list_and_its_counts(graphs, on_device):
    eng, gr, sm = on_device("D")
    g, _, users = graphs["D"]
    pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, True, cap=7)
    n_paths = eng.candidate_path_counts()
    for kw, code in ((dict(cap=0), _ffi.E_ARG), (dict(cap=-1), _ffi.E_ARG), (dict(min_hops=0), _ffi.E_ARG), (dict(max_hops=4), _ffi.E_ARG),
                     (dict(users=np.array([1, g["Ve"]], np.int32)), _ffi.E_INDEX)):
        a = dict(users=users, min_hops=1, max_hops=3, cap=7)
        a.update(kw)
        out_gc = np.full(len(a["users"]), -7, np.int32)
        total = C.c_int64(-7)
        rc = eng.L.kprn_find_candidates_top(eng.h, gr.ptr, sm.ptr, _ffi._fp(a["users"]), len(a["users"]), a["min_hops"], a["max_hops"], 1, a["cap"],
                                            _ffi._fp(out_gc), C.byref(total))
        assert rc == code and (out_gc == -7).all() and total.value == -7, kw
        back, back_n = np.zeros_like(pairs), np.zeros_like(n_paths)
        assert eng.L.kprn_read_candidates(eng.h, _ffi._fp(back), C.c_int64(len(pairs))) == 0 and np.array_equal(back, pairs), kw
        assert eng.L.kprn_read_candidate_paths(eng.h, _ffi._fp(back_n), C.c_int64(len(pairs))) == 0 and np.array_equal(back_n, n_paths), kw
    assert eng.L.kprn_read_candidate_paths(eng.h, _ffi._fp(back_n), C.c_int64(len(pairs) - 1)) == _ffi.E_ARG
    with pytest.raises(_ffi.KprnError) as ei:
        eng.find_candidates(gr, sm, users, 1, 3, True, cap=-1)
    assert ei.value.code == _ffi.E_ARG


def test_a_plain_list_has_no_path_counts(graphs, on_device):
    eng, gr, sm = on_device("D")
    users = graphs["D"][2]
    capped, capped_gc = eng.find_candidates(gr, sm, users, 1, 3, True, cap=tref.CAP_MAX)
    assert len(eng.candidate_path_counts()) == len(capped)
    pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, True)
    assert np.array_equal(pairs, capped) and np.array_equal(gc, capped_gc)              # no effect above the count
    with pytest.raises(_ffi.KprnError) as ei:
        eng.candidate_path_counts()
    assert ei.value.code == _ffi.E_ARG


def same_recommendation(a, b):
    """two results of graph.recommend, field by field and bit by bit"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert {k: v for k, v in x.items() if k != "paths"} == {k: v for k, v in y.items() if k != "paths"}
        assert len(x["paths"]) == len(y["paths"])
        for (ids, w, s), (ids2, w2, s2) in zip(x["paths"], y["paths"]):
            assert np.array_equal(ids, ids2) and w == w2 and s == s2


def test_capped_chain_equals_the_chain_fed_the_twins_kept(graphs, on_device, twin):
    eng, gr, sm = on_device("D")
    users = graphs["D"][2]
    K, M = 10, 3
    got = kgraph.recommend_users(eng, gr, sm, users, K, M, max_candidates=64)
    assert len(got) == len(users)
    for u, mine in zip(users, got):
        pairs, _, _ = twin("D", np.array([u], np.int32), 1, 3, 1, 64)
        assert len(pairs) == 64
        want = kgraph.recommend(eng, gr, int(u), pairs[:, 1], K, M)
        assert len(want) == K
        same_recommendation(mine, want)
    same_recommendation(kgraph.recommend(eng, gr, 1, None, K, M, sampler=sm, max_candidates=64), got[0])
    three = users[[0, 24, 25]]
    plain = kgraph.recommend_users(eng, gr, sm, three, K, M)
    for a, b in zip(kgraph.recommend_users(eng, gr, sm, three, K, M, max_candidates=0), plain):
        same_recommendation(a, b)
    with pytest.raises(ValueError):
        kgraph.recommend(eng, gr, 1, [25, 26], K, M, max_candidates=64)


def _cli_inputs_d(tmp_path, g):
    """graph D as a triples file with vocabularies whose entity e<k> has id k and whose relations 1..4 are rate, _rate, also, _also; a small saved model"""
    from kprn_amd.pathformat import Vocabs
    vdir = tmp_path / "vocab"
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
    (tmp_path / "kg.tsv").write_text("".join("%s\t%s\t%s\n" % t for t in triples))
    kg = kgraph.KnowledgeGraph.from_triples(triples, Vocabs(str(vdir)), 1)
    eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, 16, 32, 16, 64, 2)
    try:
        eng.save(str(tmp_path / "model"))
    finally:
        eng.close()
    flags = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1, "-gpu_id", 0, "-top_k", 2, "-model_path", tmp_path / "model", "-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-user", "e325",
             "-k", 10, "-explain_paths", 3]
    return kg, [str(f) for f in flags]


def test_command_line_max_candidates(graphs, tmp_path, capsys):
    from kprn_amd import recommend as cli, scoring
    g = graphs["D"][0]
    kg, flags = _cli_inputs_d(tmp_path, g)
    assert np.array_equal(kg.src, g["src"]) and np.array_equal(kg.dst, g["dst"]) and np.array_equal(kg.rel, g["rel"])

    def run(extra):
        buf = io.StringIO()
        assert cli.main(flags + [str(x) for x in extra], out=buf) == 0
        return buf.getvalue()

    hub = kg.entity_id("e325")
    assert hub == g["cases"]["hub"]
    catalogue = np.unique(kg.interactions("rate")[:, 1])
    cand, gc, _ = _ffi.host_find_candidates_top(kg.src, kg.dst, kg.rel, kg.Ve, catalogue, [hub], 1, 3, 64, True)
    everyone, _ = _ffi.host_find_candidates(kg.src, kg.dst, kg.rel, kg.Ve, catalogue, [hub], 1, 3, True)
    assert len(cand) == 64 < len(everyone) and g["cases"]["target"] in cand
    eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, 16, 32, 16, 64, 2)
    try:
        eng.load(str(tmp_path / "model"))
        res = kgraph.recommend(eng, kg, hub, cand, 10, 3)
    finally:
        eng.close()
    want = ""
    for r in res:
        want += "%d\t%s\t%.5f\t%d\t%d\n" % (r["rank"], kg.entity_name(r["item"]), r["score"], r["n_paths"], r["found"])
        for place, (ids, w, s) in enumerate(r["paths"]):
            want += "%d\t%d\t%.5f\t%.6g\t%s\n" % (r["rank"], place, w, s, scoring.format_path(ids, kg.Ve))
    assert len(res) == 10 and run(["-interaction_rel", "rate", "-max_candidates", 64]) == want
    assert run(["-interaction_rel", "rate", "-max_candidates", 0]) == run(["-interaction_rel", "rate"])
    items_file = tmp_path / "items.txt"
    items_file.write_text("e25\ne26\n")
    with pytest.raises(SystemExit) as ei:
        cli.main(flags + ["-items", str(items_file), "-max_candidates", "64"], out=io.StringIO())
    err = capsys.readouterr().err
    assert ei.value.code != 0 and "-max_candidates" in err and "-items" in err
