"""not gpu: the update rule on the host (include/kprn.h "updating a graph in place") -- kprn_host_graph_update against the set arithmetic of
tests/graph_update_ref.py, its refusals, graph.read_delta and KnowledgeGraph.apply through the host arrays.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from kprn_amd import _ffi
from kprn_amd import graph as kgraph
from kprn_amd.graph import KnowledgeGraph
from kprn_amd.pathformat import Vocabs

from . import graph_update_ref as ref
from .test_path_find_host import _write_vocab


@pytest.fixture(scope="module")
def g():
    return ref.base_graph()


@pytest.fixture(scope="module")
def planted(g):
    return ref.planted_delta(g)


def check(src, dst, rel, Ve, adds, removes):
    """the twin on (edge list, delta) equals the reference -> the updated edge set"""
    S = ref.stored(src, dst, rel)
    want, n_added, n_removed = ref.apply_rule(S, adds.tolist(), removes.tolist())
    rowptr, col, rl, got_added, got_removed = _ffi.host_graph_update(src, dst, rel, Ve, ref.VR, adds, removes)
    w_rowptr, w_col, w_rel = ref.csr_of(want, Ve)
    assert np.array_equal(rowptr, w_rowptr) and np.array_equal(col, w_col) and np.array_equal(rl, w_rel)
    assert (got_added, got_removed) == (n_added, n_removed) and len(col) == len(S) + n_added - n_removed
    return want


def test_new_symbols_are_declared_and_exported():
    import subprocess
    from kprn_amd import build as kbuild
    declared = _ffi.declared_symbols()
    syms = subprocess.check_output(["nm", "-D", kbuild.build()]).decode()
    for s in ("kprn_graph_update", "kprn_graph_read", "kprn_graph_set_node_types", "kprn_host_graph_update"):
        assert s in declared, s
        assert " T %s" % s in syms, s


def test_the_planted_delta_holds_every_case(g, planted):
    adds, removes, c = planted
    S = ref.stored(g["src"], g["dst"], g["rel"])
    A, R = [tuple(r) for r in adds.tolist()], [tuple(r) for r in removes.tolist()]
    hub = g["cases"]["hub"]
    hub_row = sorted(e for e in S if e[0] == hub)
    assert len(S) > 5 * 256 and len({d for _, d, _ in hub_row}) == 300
    assert hub_row[0] < c["add_inside_hub"] < hub_row[-1] and c["add_inside_hub"] not in S
    assert c["add_before_hub_first"] < hub_row[0] and c["add_before_hub_first"][0] == hub
    assert c["add_behind_hub_last"] > hub_row[-1] and c["add_behind_hub_last"][0] == hub
    s, d, r = c["add_between_relations"]
    assert sorted(x[2] for x in S if x[:2] == (s, d)) == [1, 4] and r == 2
    assert A.count(c["add_twice"][0]) == 2 and c["add_twice"][0] not in S
    assert c["add_stored"] in S and c["add_stored"] not in R
    assert c["add_self_loop"][0] == c["add_self_loop"][1]
    assert not any(e[0] == c["add_from_lonely"][0] for e in S)
    assert c["add_from_node_1"][0] == 1 and c["add_from_last_node"][0] == g["Ve"] - 1
    assert len(c["add_random"]) == 300
    assert c["remove_hub_middle"] in hub_row[100:200]
    s, d, r = c["remove_every_relation"]
    assert r == 0 and len([x for x in S if x[:2] == (s, d)]) == 3 and (s, d) == (g["cases"]["exact"][0] + 2, g["cases"]["exact"][1])
    assert c["remove_not_stored"] not in S
    assert R.count(c["remove_twice"][0]) == 2 and c["remove_twice"][0] in S
    assert c["remove_and_add"] in S and c["remove_and_add"] in A and c["remove_and_add"] in R
    node = c["remove_every_edge_of_a_node"][0][0]
    assert set(c["remove_every_edge_of_a_node"]) == {e for e in S if e[0] == node} and len(c["remove_every_edge_of_a_node"]) >= 2
    assert len(c["remove_random"]) == 200 and set(c["remove_random"]) <= S


def test_twin_equals_the_rule_on_the_planted_delta(g, planted):
    adds, removes, c = planted
    S = ref.stored(g["src"], g["dst"], g["rel"])
    want = check(g["src"], g["dst"], g["rel"], g["Ve"], adds, removes)
    assert c["remove_and_add"] in want and c["add_stored"] in want and c["add_self_loop"] not in want
    A = {tuple(r) for r in adds.tolist()}
    assert not any(e in want for e in c["remove_every_edge_of_a_node"] if e not in A)
    _, n_added, n_removed = ref.apply_rule(S, adds.tolist(), removes.tolist())
    assert n_added > len(want - S) and n_removed > len(S - want)      # the edge removed and added again counts in both


def test_twin_on_the_limits(g, planted):
    adds, removes, _ = planted
    none = np.zeros((0, 3), np.int32)
    S = ref.stored(g["src"], g["dst"], g["rel"])
    assert check(g["src"], g["dst"], g["rel"], g["Ve"], none, none) == S                     # the empty delta
    empty = np.zeros(0, np.int32)
    assert len(check(empty, empty, empty, g["Ve"], adds, none)) > 300                        # only additions, onto E = 0
    assert check(empty, empty, empty, g["Ve"], none, removes) == set()                       # removals from E = 0
    everything = ref.rows(sorted(S))
    assert check(g["src"], g["dst"], g["rel"], g["Ve"], none, everything) == set()           # every edge removed
    by_pair = ref.rows(sorted({(s, d, 0) for s, d, _ in S}))
    assert check(g["src"], g["dst"], g["rel"], g["Ve"], none, by_pair) == set()              # ... and by rel = 0 alone


def test_twin_on_a_chain_of_five_deltas(g):
    S = ref.stored(g["src"], g["dst"], g["rel"])
    for step in range(5):
        adds, removes = ref.random_delta(S, g["Ve"], seed=100 + step)
        before = len(S)
        S = check(*ref.edge_arrays(S), g["Ve"], adds, removes)
        assert len(S) != before


REFUSALS = [   # (what, Ve, Vr, adds, removes, status)
    ("an added node 0", None, None, [(0, 3, 1)], [], _ffi.E_INDEX),
    ("an added node Ve", None, None, [(3, "Ve", 1)], [], _ffi.E_INDEX),
    ("an added relation 0", None, None, [(3, 4, 0)], [], _ffi.E_INDEX),
    ("an added relation Vr + 1", None, None, [(3, 4, ref.VR + 1)], [], _ffi.E_INDEX),
    ("a removed node Ve", None, None, [], [("Ve", 3, 1)], _ffi.E_INDEX),
    ("a removed node 0", None, None, [], [(3, 0, 0)], _ffi.E_INDEX),
    ("a removed relation -1", None, None, [], [(3, 4, -1)], _ffi.E_INDEX),
    ("a removed relation Vr + 1", None, None, [], [(3, 4, ref.VR + 1)], _ffi.E_INDEX),
    ("Ve < 2", 1, None, [], [], _ffi.E_ARG),
    ("Vr < 1", None, 0, [], [], _ffi.E_ARG),
]


def raw_call(g, Ve, Vr, a, r, n_add=None, n_del=None, null_add=False, null_del=False, E=None, null_out=None):
    """kprn_host_graph_update with every argument in the caller's hands -> (status, the outputs, poisoned with -77 beforehand)"""
    src, dst, rel = (np.ascontiguousarray(x, np.int32) for x in (g["src"], g["dst"], g["rel"]))
    a, r = ref.rows(a), ref.rows(r)
    ac, rc_ = [np.ascontiguousarray(a[:, k]) for k in range(3)], [np.ascontiguousarray(r[:, k]) for k in range(3)]
    room = len(src) + len(a) + 1
    out = dict(rowptr=np.full(g["Ve"] + 1, -77, np.int32), col=np.full(room, -77, np.int32), rel=np.full(room, -77, np.int32))
    cnt = [C.c_int64(-77), C.c_int64(-77), C.c_int64(-77)]
    ptr = lambda cols, null: [None if null or not len(c) else _ffi._fp(c) for c in cols]
    outs = [None if null_out == k else _ffi._fp(out[k]) for k in ("rowptr", "col", "rel")]
    rc = _ffi.lib().kprn_host_graph_update(_ffi._fp(src), _ffi._fp(dst), _ffi._fp(rel), C.c_int64(len(src) if E is None else E), int(Ve), int(Vr),
                                           *ptr(ac, null_add), C.c_int64(len(a) if n_add is None else n_add),
                                           *ptr(rc_, null_del), C.c_int64(len(r) if n_del is None else n_del),
                                           *outs, None if null_out == "E_out" else C.byref(cnt[0]), C.byref(cnt[1]), C.byref(cnt[2]))
    return rc, out, [int(c.value) for c in cnt]


def untouched(out, cnt):
    return all((v == -77).all() for v in out.values()) and cnt == [-77, -77, -77]


@pytest.mark.parametrize("what,Ve,Vr,adds,removes,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_outputs_unwritten(g, what, Ve, Vr, adds, removes, status):
    fill = lambda lst: [tuple(g["Ve"] if x == "Ve" else x for x in e) for e in lst]
    rc, out, cnt = raw_call(g, g["Ve"] if Ve is None else Ve, ref.VR if Vr is None else Vr, fill(adds), fill(removes))
    assert rc == status and untouched(out, cnt)


def test_refusals_of_sizes_and_null_arrays(g):
    Ve = g["Ve"]
    for kw in (dict(n_add=-1), dict(n_del=-1), dict(n_add=2**31), dict(n_del=2**31), dict(null_add=True), dict(null_del=True), dict(E=-1), dict(E=2**31),
               dict(null_out="rowptr"), dict(null_out="col"), dict(null_out="rel"), dict(null_out="E_out")):
        rc, out, cnt = raw_call(g, Ve, ref.VR, [(3, 4, 1)], [(4, 3, 1)], **kw)
        assert rc == _ffi.E_ARG and untouched(out, cnt), kw
    bad = dict(g, src=np.where(np.arange(len(g["src"])) == 5, Ve, g["src"]).astype(np.int32))                # a stored edge's node outside 1..Ve-1
    rc, out, cnt = raw_call(bad, Ve, ref.VR, [], [])
    assert rc == _ffi.E_INDEX and untouched(out, cnt)
    rc, out, cnt = raw_call(g, Ve, ref.VR, [(3, 4, 1)], [(4, 3, 0)])                                         # (and the same call with nothing wrong)
    assert rc == 0 and cnt[0] == len(ref.apply_rule(ref.stored(g["src"], g["dst"], g["rel"]), [(3, 4, 1)], [(4, 3, 0)])[0])
    with pytest.raises(_ffi.KprnError):
        _ffi.host_graph_update(g["src"], g["dst"], g["rel"], Ve, ref.VR, np.zeros((2, 2), np.int32), None)


# ---- graph.read_delta and KnowledgeGraph.apply -----------------------------------------------------------------------------------------------------
TRIPLES = [(h, r, t) for u, m in [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 0), (3, 4), (1, 4), (2, 0), (3, 1), (0, 3)]
           for h, r, t in (("u%d" % u, "rate", "m%d" % m), ("m%d" % m, "_rate", "u%d" % u))] + \
          [(h, r, t) for m in (1, 2, 4) for h, r, t in (("m%d" % m, "act", "a0"), ("a0", "_act", "m%d" % m))] + [("u0", "act", "m1")]


@pytest.fixture()
def kg(tmp_path):
    _write_vocab(str(tmp_path))
    return KnowledgeGraph.from_triples(TRIPLES, Vocabs(str(tmp_path)), 1)


def test_read_delta_round_trip(kg, tmp_path):
    e, r = kg.entity_id, kg.relation_id
    path = tmp_path / "delta.tsv"
    path.write_text("# since the graph file was written\n+\tu0\trate\tm2\n+\tm2\t_rate\tu0\n\n-\tu0\t*\tm1\n-\tm1\t_rate\tu0\n+\tg0\tmade_of\tnobody\n-\ta0\t_act\tm4\n")
    adds, removes, (ent, rows) = kgraph.read_delta(str(path), kg)
    unk_e, unk_r = kg.entity_id("#UNK_ENTITY"), kg.relation_id("#UNK_RELATION")
    assert adds.dtype == np.int32 and adds.tolist() == [[e("u0"), e("m2"), r("rate")], [e("m2"), e("u0"), r("_rate")], [e("g0"), unk_e, unk_r]]
    assert removes.tolist() == [[e("u0"), e("m1"), 0], [e("m1"), e("u0"), r("_rate")], [e("a0"), e("m4"), r("_act")]]
    # g0 (no type entry) and the unknown entity are new to the graph: their rows are the formatter's; u0 and m2 keep the rows they have
    unk_t = int(kg.vocabs.entity_type["#UNK_ENTITY_TYPE"]) + 1
    assert ent.tolist() == sorted([e("g0"), unk_e]) and rows.tolist() == [[unk_t], [unk_t]]
    before = ref.stored(kg.src, kg.dst, kg.rel)
    want, n_added, n_removed = ref.apply_rule(before, adds.tolist(), removes.tolist())
    assert kg.apply(adds, removes, (ent, rows)) == (n_added, n_removed) == (3, 4)              # u0 -> m1 held rate and act
    assert ref.stored(kg.src, kg.dst, kg.rel) == want and len(kg.src) == len(want)
    assert kg.node_types[e("g0") - 1].tolist() == [unk_t] and [e("u0"), e("m2")] in kg.interactions("rate").tolist()
    assert [e("u0"), e("m1")] not in kg.interactions("rate").tolist()


@pytest.mark.parametrize("line,no", [("+\tu0\t*\tm2", 2), ("+\tu0\trate", 2), ("u0\trate\tm2\tx", 2), ("*\tu0\trate\tm2", 2), ("-\tu0\t\tm2", 2)])
def test_read_delta_names_the_bad_line(kg, tmp_path, line, no):
    path = tmp_path / "delta.tsv"
    path.write_text("+\tu1\trate\tm0\n" + line + "\n")
    with pytest.raises(ValueError, match="line %d" % no):
        kgraph.read_delta(str(path), kg)


def test_apply_reproduces_the_holdout_train_graph(kg):
    train_kg, held = kg.holdout("rate", 0.6, 3)
    assert 2 <= len(held) < len(kg.interactions("rate"))
    before = ref.stored(kg.src, kg.dst, kg.rel)
    removes = np.array([(u, i, 0) for u, i in held.tolist()] + [(i, u, 0) for u, i in held.tolist()], np.int32)
    n_added, n_removed = kg.apply(removes=removes)
    want = ref.stored(train_kg.src, train_kg.dst, train_kg.rel)
    assert ref.stored(kg.src, kg.dst, kg.rel) == want and want < before
    assert (n_added, n_removed) == (0, len(before) - len(want))
    assert np.array_equal(kg.interactions("rate"), train_kg.interactions("rate")) and np.array_equal(kg.node_types, train_kg.node_types)
    with pytest.raises(_ffi.KprnError):
        kg.apply(adds=np.array([(1, kg.Ve, 1)], np.int32))                                      # refused: nothing changes
    assert ref.stored(kg.src, kg.dst, kg.rel) == want
