"""gpu: kprn_graph_update / kprn_graph_read / kprn_graph_set_node_types (include/kprn.h "updating a graph in place"; kprn_amd/csrc/graph_update.hip) -- the
updated graph's CSR against the host twin (itself held to set arithmetic by tests/test_graph_update_host.py) and against a graph created fresh from the
edited edge list, and every find, candidates and sampler call on the two.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from kprn_amd import _ffi

from . import graph_update_ref as ref
from . import path_find_ref as pref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return ref.base_graph()


@pytest.fixture(scope="module")
def nt(g):
    return pref.node_types(g, 1)


@pytest.fixture(scope="module")
def planted(g):
    return ref.planted_delta(g)


@pytest.fixture(scope="module")
def eng(g):
    e = _ffi.Engine(pref.VT, g["Ve"], pref.VR, dt=16, de=32, dr=16, H=64, L=2, F=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pairs(g):
    pr = pref.pairs_of(g, 60, seed=29)
    assert len(pr) == 70
    return pr


def same_csr(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def update_and_check(eng, nt, gr, S, Ve, adds, removes):
    """one update of the device graph gr, which stores the edge set S: afterwards its CSR is the twin's and that of a fresh graph of the edited edge list
    -> the updated edge set"""
    want, n_added, n_removed = ref.apply_rule(S, adds.tolist(), removes.tolist())
    twin = _ffi.host_graph_update(*ref.edge_arrays(S), Ve, ref.VR, adds, removes)
    assert gr.update(adds, removes) == (n_added, n_removed) == twin[3:]
    got = gr.read_csr()
    assert same_csr(got, twin[:3]) and gr.n_edges == len(want) == len(S) + n_added - n_removed
    fresh = eng.graph(*ref.edge_arrays(want), nt, pref.END_REL)
    try:
        assert fresh.n_edges == gr.n_edges and same_csr(got, fresh.read_csr())
    finally:
        fresh.free()
    return want


def test_read_csr_is_the_stored_graph(eng, g, nt):
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    S = ref.stored(g["src"], g["dst"], g["rel"])
    assert same_csr(gr.read_csr(), ref.csr_of(S, g["Ve"])) and gr.n_edges == len(S) > 5 * 256
    assert gr.update() == (0, 0) and same_csr(gr.read_csr(), ref.csr_of(S, g["Ve"]))          # the empty delta
    gr.free()


def test_the_planted_delta(eng, g, nt, planted):
    adds, removes, _ = planted
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    update_and_check(eng, nt, gr, ref.stored(g["src"], g["dst"], g["rel"]), g["Ve"], adds, removes)
    gr.free()


def test_a_chain_of_five_deltas(eng, g, nt):
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    S = ref.stored(g["src"], g["dst"], g["rel"])
    for step in range(5):
        adds, removes = ref.random_delta(S, g["Ve"], seed=100 + step)
        S = update_and_check(eng, nt, gr, S, g["Ve"], adds, removes)
    gr.free()


def test_the_limits(eng, g, nt, planted):
    adds, removes, _ = planted
    none = np.zeros((0, 3), np.int32)
    empty = np.zeros(0, np.int32)
    S = ref.stored(g["src"], g["dst"], g["rel"])
    gr = eng.graph(empty, empty, empty, nt, pref.END_REL)                                       # E = 0: removals find nothing, additions build a graph
    assert update_and_check(eng, nt, gr, set(), g["Ve"], none, removes) == set()
    S0 = update_and_check(eng, nt, gr, set(), g["Ve"], adds, none)
    assert len(S0) > 300
    assert update_and_check(eng, nt, gr, S0, g["Ve"], none, ref.rows(sorted({(s, d, 0) for s, d, _ in S0}))) == set()   # every edge removed, by rel = 0
    gr.free()
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    assert update_and_check(eng, nt, gr, S, g["Ve"], adds, ref.rows(sorted(S))) == ref.apply_rule(set(), adds.tolist(), [])[0]   # ... and replaced
    gr.free()
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)                              # a delta larger than the graph
    rng = np.random.RandomState(77)
    big = np.stack([rng.randint(1, g["Ve"], 4000), rng.randint(1, g["Ve"], 4000), rng.randint(1, 5, 4000)], axis=1).astype(np.int32)
    assert len(update_and_check(eng, nt, gr, S, g["Ve"], big, none)) > 2 * len(S)
    gr.free()


def found_by(eng, gr, pairs, lo, hi, cap, T):
    batch, counts, found = eng.find_paths(gr, pairs, lo, hi, cap, T)
    idx = batch.read_idx()
    batch.free()
    return idx, counts, found


def test_every_call_on_the_updated_graph_equals_the_fresh_graphs(eng, g, nt, planted, pairs):
    adds, removes, _ = planted
    S = ref.stored(g["src"], g["dst"], g["rel"])
    want, _, _ = ref.apply_rule(S, adds.tolist(), removes.tolist())
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    before = found_by(eng, gr, pairs, 1, 3, 5, 4)
    gr.update(adds, removes)
    fresh = eng.graph(*ref.edge_arrays(want), nt, pref.END_REL)
    for lo, hi, cap, T in ((1, 3, 5, 4), (2, 3, 4096, 6)):
        a, b = found_by(eng, gr, pairs, lo, hi, cap, T), found_by(eng, fresh, pairs, lo, hi, cap, T)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[1].sum() > 20
    assert not np.array_equal(before[2], found_by(eng, gr, pairs, 1, 3, 5, 4)[2])               # (the delta changed what is found)
    items = np.arange(1, 200, dtype=np.int32)
    users = np.array([g["cases"]["hub"], g["cases"]["exact"][0], 3, 17, 250, g["cases"]["lonely"][0]], np.int32)
    sm = eng.sampler(items)
    ca, cb = eng.find_candidates(gr, sm, users, 1, 3), eng.find_candidates(fresh, sm, users, 1, 3)
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]) and ca[1].sum() > 0
    na, nb = eng.sample_negatives(gr, sm, users, 8, 12345, 2), eng.sample_negatives(fresh, sm, users, 8, 12345, 2)
    assert np.array_equal(na[0], nb[0]) and np.array_equal(na[1], nb[1]) and na[1].sum() > 0
    sm.free(); gr.free(); fresh.free()


def test_the_pattern_set_survives(eng, g, nt, planted, pairs):
    adds, removes, _ = planted
    S = ref.stored(g["src"], g["dst"], g["rel"])
    want, _, _ = ref.apply_rule(S, adds.tolist(), removes.tolist())
    patterns = [[{1, 2}], [None, {1, 3}], [{1, 2, 4}, None, {2, 3}]]
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    gr.set_patterns(patterns)
    gr.update(adds, removes)
    assert gr.num_patterns() == 3
    fresh = eng.graph(*ref.edge_arrays(want), nt, pref.END_REL)
    plain = found_by(eng, fresh, pairs, 1, 3, 4096, 4)
    fresh.set_patterns(patterns)
    a, b = found_by(eng, gr, pairs, 1, 3, 4096, 4), found_by(eng, fresh, pairs, 1, 3, 4096, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and 0 < a[2].sum() < plain[2].sum()  # (and the set does filter)
    gr.free(); fresh.free()


def test_set_node_types(eng, g, nt, pairs):
    a = g["cases"]["exact"][0]
    ent = np.array([a + 2, g["cases"]["hub"], a], np.int32)                                     # a middle node, a user, and not in ascending order
    rows = (nt[ent - 1] % (pref.VT - 1) + 1).astype(np.int32)                                   # another id of 1 .. VT - 1 for each
    assert (rows != nt[ent - 1]).all()
    nt2 = nt.copy()
    nt2[ent - 1] = rows
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    before = found_by(eng, gr, pairs, 1, 3, 4096, 4)
    csr = gr.read_csr()
    gr.set_node_types(ent, rows)
    fresh = eng.graph(g["src"], g["dst"], g["rel"], nt2, pref.END_REL)
    got, want = found_by(eng, gr, pairs, 1, 3, 4096, 4), found_by(eng, fresh, pairs, 1, 3, 4096, 4)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)) and same_csr(csr, gr.read_csr())
    changed = got[0] != before[0]
    assert changed.any() and not changed[:, :, 1:].any()                                        # the type column of some steps, and nothing else
    assert np.isin(got[0][:, :, 1][changed[:, :, 0]], ent).all()                                # ... all of them steps at the three entities
    for bad_ent, bad_rows, code in (([a, a], [[1], [2]], _ffi.E_ARG), ([0], [[1]], _ffi.E_INDEX), ([g["Ve"]], [[1]], _ffi.E_INDEX),
                                    ([a], [[0]], _ffi.E_INDEX), ([a], [[pref.VT + 1]], _ffi.E_INDEX)):
        with pytest.raises(_ffi.KprnError) as err:
            gr.set_node_types(np.array(bad_ent, np.int32), np.array(bad_rows, np.int32))
        assert err.value.code == code
    assert all(np.array_equal(x, y) for x, y in zip(found_by(eng, gr, pairs, 1, 3, 4096, 4), want))   # a refused call wrote nothing
    gr.free(); fresh.free()


def test_refused_calls_leave_the_graph_untouched(eng, g, nt):
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL)
    csr, Ve = gr.read_csr(), g["Ve"]
    ok = [(3, 4, 1)]
    for adds, removes, code in (([(0, 3, 1)], ok, _ffi.E_INDEX), ([(3, Ve, 1)], ok, _ffi.E_INDEX), ([(3, 4, 0)], ok, _ffi.E_INDEX),
                                ([(3, 4, ref.VR + 1)], ok, _ffi.E_INDEX), (ok, [(Ve, 3, 1)], _ffi.E_INDEX), (ok, [(3, 0, 0)], _ffi.E_INDEX),
                                (ok, [(3, 4, -1)], _ffi.E_INDEX), (ok, [(3, 4, ref.VR + 1)], _ffi.E_INDEX)):
        with pytest.raises(_ffi.KprnError) as err:
            gr.update(ref.rows(adds), ref.rows(removes))
        assert err.value.code == code and same_csr(csr, gr.read_csr())
    col = np.array([3], np.int32)
    p, null, one, n = _ffi._fp(col), None, C.c_int64(1), C.c_int64(0)
    for args in ((null, p, p, one, null, null, null, n), (p, p, null, one, null, null, null, n), (null, null, null, n, p, null, p, one),
                 (p, p, p, C.c_int64(-1), null, null, null, n), (null, null, null, n, p, p, p, C.c_int64(2**31))):
        assert eng.L.kprn_graph_update(eng.h, gr.ptr, *args, None, None) == _ffi.E_ARG and same_csr(csr, gr.read_csr())
    assert eng.L.kprn_graph_update(eng.h, None, p, p, p, one, null, null, null, n, None, None) == _ffi.E_ARG
    assert eng.L.kprn_graph_read(eng.h, gr.ptr, None, p, p) == _ffi.E_ARG
    assert gr.update(ref.rows(ok), None) == (0 if (3, 4, 1) in ref.stored(g["src"], g["dst"], g["rel"]) else 1, 0)   # (and it still takes a good one)
    gr.free()


def test_the_same_update_on_two_graphs_gives_the_same_bits(eng, g, nt, planted):
    adds, removes, _ = planted
    one, two = (eng.graph(g["src"], g["dst"], g["rel"], nt, pref.END_REL) for _ in range(2))
    assert one.update(adds, removes) == two.update(adds, removes)
    assert same_csr(one.read_csr(), two.read_csr())
    one.free(); two.free()


def test_recommend_command_line_with_a_delta(tmp_path):
    """python -m kprn_amd.recommend -kg_delta (called in-process) prints what the same command prints on a graph file with the delta folded in, with a list of
    items and with the catalogue found on the device"""
    import io
    from kprn_amd import graph as kgraph, recommend as cli
    from kprn_amd.pathformat import Vocabs
    from .test_path_find_host import _write_vocab
    vdir = tmp_path / "vocab"
    vdir.mkdir()
    _write_vocab(str(vdir))
    both = lambda h, r, t: [(h, r, t), (t, "_" + r, h)]
    triples = [e for u, m in [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 0), (3, 4), (1, 4)] for e in both("u%d" % u, "rate", "m%d" % m)]
    triples += [e for m in (1, 2, 4) for e in both("m%d" % m, "act", "a0")] + [("u0", "act", "m1")]
    # u0 rates m2 and takes everything between itself and m1 back; u3 rates m3; g0, which the graph file never names, acts in m3
    added = both("u0", "rate", "m2") + both("u3", "rate", "m3") + both("m3", "act", "g0")
    delta = ["# what happened since"] + ["+\t%s\t%s\t%s" % e for e in added] + ["", "-\tu0\t*\tm1", "-\tm1\t_rate\tu0", "-\tu2\trate\tm0"]
    gone = {("u0", "rate", "m1"), ("u0", "act", "m1"), ("m1", "_rate", "u0")}
    folded = [e for e in triples if e not in gone] + added
    (tmp_path / "kg.tsv").write_text("".join("%s\t%s\t%s\n" % t for t in triples))
    (tmp_path / "folded.tsv").write_text("".join("%s\t%s\t%s\n" % t for t in folded))
    (tmp_path / "delta.tsv").write_text("\n".join(delta) + "\n")
    (tmp_path / "items.txt").write_text("\n".join(["m0", "m1", "m2", "m3", "m4", "g0"]) + "\n")
    kg = kgraph.KnowledgeGraph.from_triples(triples, Vocabs(str(vdir)), 1)
    eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, 16, 32, 16, 64, 2)
    try:
        eng.save(str(tmp_path / "model"))
    finally:
        eng.close()
    flags = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1, "-gpu_id", 0, "-top_k", 2, "-model_path", tmp_path / "model", "-vocab_dir", vdir, "-user", "u0", "-k", 4, "-explain_paths", 2]

    def run(extra):
        buf = io.StringIO()
        assert cli.main([str(f) for f in flags + extra], out=buf) == 0
        return buf.getvalue()
    for route in (["-items", tmp_path / "items.txt"], ["-interaction_rel", "rate"]):
        want = run(["-kg", tmp_path / "folded.tsv"] + route)
        assert run(["-kg", tmp_path / "kg.tsv", "-kg_delta", tmp_path / "delta.tsv"] + route) == want
        assert len(want.splitlines()) >= 4 and run(["-kg", tmp_path / "kg.tsv"] + route) != want          # (the delta changes the answer)


def test_evaluate_command_line_with_a_delta(tmp_path):
    """python -m kprn_amd.evaluate -kg_delta prints what the same command prints on a graph file with the delta folded in"""
    import io
    from kprn_amd import evaluate as cli, graph as kgraph
    from kprn_amd.pathformat import Vocabs
    from .test_path_find_host import _write_vocab
    vdir = tmp_path / "vocab"
    vdir.mkdir()
    _write_vocab(str(vdir))
    both = lambda h, r, t: [(h, r, t), (t, "_" + r, h)]
    rated = [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 0), (3, 4), (1, 4), (2, 0), (3, 1), (0, 3), (1, 0), (2, 4)]
    triples = [e for u, m in rated for e in both("u%d" % u, "rate", "m%d" % m)] + [e for m in (1, 2, 4) for e in both("m%d" % m, "act", "a0")]
    added = both("u0", "rate", "m2") + both("u3", "rate", "m3") + both("m3", "act", "a0")
    gone = set(both("u0", "rate", "m1") + both("u2", "rate", "m4"))
    delta = ["+\t%s\t%s\t%s" % e for e in added] + ["-\tu0\t*\tm1", "-\tm1\t*\tu0", "-\tu2\trate\tm4", "-\tm4\t_rate\tu2"]
    (tmp_path / "kg.tsv").write_text("".join("%s\t%s\t%s\n" % t for t in triples))
    (tmp_path / "folded.tsv").write_text("".join("%s\t%s\t%s\n" % t for t in [e for e in triples if e not in gone] + added))
    (tmp_path / "delta.tsv").write_text("\n".join(delta) + "\n")
    kg = kgraph.KnowledgeGraph.from_triples(triples, Vocabs(str(vdir)), 1)
    eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, 16, 32, 16, 64, 2)
    try:
        eng.save(str(tmp_path / "model"))
    finally:
        eng.close()
    flags = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1, "-gpu_id", 0, "-top_k", 2, "-model_path", tmp_path / "model", "-vocab_dir", vdir, "-interaction_rel", "rate", "-holdout", 0.4]

    def run(extra):
        buf = io.StringIO()
        assert cli.main([str(f) for f in flags + extra], out=buf) == 0
        return buf.getvalue()
    want = run(["-kg", tmp_path / "folded.tsv"])
    assert run(["-kg", tmp_path / "kg.tsv", "-kg_delta", tmp_path / "delta.tsv"]) == want and len(want.splitlines()) == 3
    assert int(want.splitlines()[2].split("\t")[0]) >= 2                                             # (held pairs were evaluated)
