"""not gpu: kprn_host_find_paths, the host twin of the device path finder (include/kprn.h "finding a pair's paths"), against a brute-force depth-first
search written here (tests/path_find_ref.py), against the formatter's own rows, and its refusals.  Every comparison is exact."""
import json
import os

import numpy as np
import pytest

from kprn_amd import _ffi
from kprn_amd.graph import KnowledgeGraph
from kprn_amd.pathformat import PathFormatter, Vocabs

from . import path_find_ref as ref

HOPS = [(lo, hi) for hi in (1, 2, 3) for lo in range(1, hi + 1)]


@pytest.fixture(scope="module")
def g():
    return ref.make_graph(n_rand=40, n_rand_edges=130, seed=5)     # 40 random + 17 planted nodes: about 60


@pytest.fixture(scope="module")
def pairs(g):
    return ref.pairs_of(g, 24, seed=11)


def test_new_symbols_are_declared_and_exported():
    import subprocess
    from kprn_amd import build as kbuild
    declared = _ffi.declared_symbols()
    syms = subprocess.check_output(["nm", "-D", kbuild.build()]).decode()
    for s in ("kprn_graph_create", "kprn_graph_destroy", "kprn_graph_num_edges", "kprn_find_paths", "kprn_batch_read_idx", "kprn_host_find_paths"):
        assert s in declared, s
        assert " T %s" % s in syms, s


def test_inputs_hold_every_case(g, pairs):
    """what the comparisons below rely on, asserted about the inputs themselves (hops 1..3, cap ref.MAX_PATHS)"""
    c = g["cases"]
    trip = list(zip(g["src"].tolist(), g["dst"].tolist(), g["rel"].tolist()))
    have = set(trip)
    n = lambda pr, lo=1, hi=3: len(ref.brute_paths(g, pr[0], pr[1], lo, hi))
    assert n(c["lonely"]) == 0 and n(c["unreachable"]) == 0                     # found == 0
    assert c["same"][0] == c["same"][1] and n(c["same"]) == 0                    # u == i
    assert n(c["direct"]) == 1 and n(c["direct"], 1, 1) == 1 and n(c["direct"], 2, 3) == 0   # only the direct edge: nothing left with min_hops = 2
    assert len(have) < len(trip)                                                  # a duplicated input edge
    assert any(s == d for s, d, r in trip)                                        # a self-loop
    assert any((s, d, r2) in have for s, d, r in have for r2 in range(1, 5) if r2 != r)   # a multi-edge
    u, i = c["through"]
    assert any(s == u and (d, u) in {(a, b) for a, b, _ in have} for s, d, r in have)     # a 2-cycle back to u
    assert (u, i) in {(a, b) for a, b, _ in have} and any(s == i and (d, i) in {(a, b) for a, b, _ in have} for s, d, r in have)   # u -> i -> x -> i
    assert n(c["exact"]) == ref.MAX_PATHS                                         # found == max_paths exactly
    ps = ref.brute_paths(g, *c["inside"], 1, 3)
    assert len(ps) > ref.MAX_PATHS
    last, nxt = ps[ref.MAX_PATHS - 1], ps[ref.MAX_PATHS]                          # the cap falls inside one first edge's subtree
    assert len(last[1]) == len(nxt[1]) and (last[0][1], last[1][0]) == (nxt[0][1], nxt[1][0])
    for pr in c.values():
        assert tuple(pr) in {tuple(p) for p in pairs.tolist()}


@pytest.mark.parametrize("num_types", [1, 2])
@pytest.mark.parametrize("hops", HOPS)
def test_twin_equals_brute_force(g, pairs, num_types, hops):
    nt = ref.node_types(g, num_types)
    lo, hi = hops
    for T in sorted({hi + 1, 6}):
        for F in (num_types + 2, num_types + 3):
            want = ref.brute_find(g, nt, pairs, lo, hi, ref.MAX_PATHS, T, F)
            got = _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, ref.MAX_PATHS, T, F=F, threads=3)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (T, F)
            assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (T, F)
    # counting alone, one thread, and an uncapped run
    _, c1, f1 = _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, 4096, hi + 1, want_idx=False)
    want = ref.brute_find(g, nt, pairs, lo, hi, 4096, hi + 1, num_types + 2)
    assert np.array_equal(c1, want[1]) and np.array_equal(f1, want[2]) and np.array_equal(c1, f1)


def test_twin_equals_brute_force_on_the_hub_graph():
    """the graph and pairs of tests/test_gpu_path_find.py (a hub of out-degree 300, as a user and next to one): the twin is the GPU test's reference"""
    g = ref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)
    nt = ref.node_types(g, 1)
    pairs = ref.pairs_of(g, 60, seed=29)
    for lo, hi, cap in ((1, 3, 5), (1, 3, 4096), (2, 3, 28)):
        want = ref.brute_find(g, nt, pairs, lo, hi, cap, 4, 3)
        got = _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, 4, threads=4)
        assert want[2].max() > 256 and all(np.array_equal(a, b) for a, b in zip(got, want))


def _write_vocab(d):
    """#PAD_TOKEN is the last id of each table (the engine's pad rows); #END_RELATION is not"""
    ents = ["u%d" % k for k in range(4)] + ["m%d" % k for k in range(5)] + ["a0", "g0"]
    w = lambda name, rows: open(os.path.join(d, name), "w").write("".join("%s\t%s\n" % r for r in rows))
    w("all_entity_id.txt", [(n, k) for k, n in enumerate(ents + ["#UNK_ENTITY", "#PAD_TOKEN"])])
    w("entity_type_id.txt", [(n, k) for k, n in enumerate(["user", "movie", "actor", "#UNK_ENTITY_TYPE", "#PAD_TOKEN"])])
    w("all_relation_id.txt", [(n, k) for k, n in enumerate(["rate", "_rate", "act", "_act", "#UNK_RELATION", "#END_RELATION", "#PAD_TOKEN"])])
    w("entity_to_type.txt", [(n, {"u": "user", "m": "movie", "a": "actor"}[n[0]]) for n in ents if n[0] != "g"])   # g0 has no type entry
    json.dump({"domain": {"1": 1, "-1": 0}, "name": "label"}, open(os.path.join(d, "domain-label"), "w"))
    return ents


@pytest.mark.parametrize("num_types", [1, 2])
def test_rows_are_the_formatters_rows(tmp_path, num_types):
    _write_vocab(str(tmp_path))
    voc = Vocabs(str(tmp_path))
    triples = []
    for u, m in [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 0), (3, 4), (1, 4)]:
        triples += [("u%d" % u, "rate", "m%d" % m), ("m%d" % m, "_rate", "u%d" % u)]
    for m in (1, 2, 4):
        triples += [("m%d" % m, "act", "a0"), ("a0", "_act", "m%d" % m)]
    triples += [("m3", "made_of", "g0"), ("g0", "_act", "m0"), ("nobody", "rate", "m2"), ("u0", "act", "a0")]     # an unknown relation, an untyped entity, an unknown entity, a 2-hop route
    kg = KnowledgeGraph.from_triples(triples, voc, num_types)
    assert (kg.Ve, kg.Vr, kg.Vt) == (13, 7, 5) and kg.end_relation == 6
    T = 5
    fmt = PathFormatter(voc, T, num_types)
    fmt.max_length = T
    ename = {int(v) + 1: k for k, v in voc.entity.items()}
    rname = {int(v) + 1: k for k, v in voc.relation.items()}
    pairs = np.array([(kg.entity_id("u%d" % u), kg.entity_id("m%d" % m)) for u in range(4) for m in range(5)], np.int32)
    idx, counts, found = kg.host_find_paths(pairs, 1, 3, 4096, T)
    assert counts.sum() > 20 and (counts == found).all() and idx.shape == (counts.sum(), T, num_types + 2)
    off = np.concatenate([[0], np.cumsum(counts)])
    seen_hops = set()
    for b, (u, i) in enumerate(pairs):
        if counts[b] == 0:
            continue
        rows = idx[off[b]:off[b + 1]]
        spelled = []
        for row in rows:                                   # r-e-r-...-r as the formatter reads it: the steps' relations and the entities between them
            steps = [s for s in row if s[-2] != kg.Ve]
            seen_hops.add(len(steps) - 1)
            toks = []
            for k, s in enumerate(steps[:-1]):
                toks.append(rname[int(s[-1])])
                if k + 1 < len(steps) - 1:
                    toks.append(ename[int(steps[k + 1][-2])])
            spelled.append("-".join(toks))
        line = fmt.format_pair(ename[int(u)], ename[int(i)], "###".join(spelled))
        printed = np.array([[[int(v) + 1 for v in step.split(",")] for step in path.split(" ")] for path in line.split(";")], np.int32)
        assert np.array_equal(printed, rows), (b, spelled)
    assert seen_hops == {1, 2, 3}


def test_from_triples_refuses_a_vocabulary_whose_pad_is_not_the_last_row():
    voc = Vocabs(os.path.join(os.path.dirname(__file__), "golden", "pathformat", "vocab"))     # the reference's layout: #END_RELATION after #PAD_TOKEN
    with pytest.raises(ValueError):
        KnowledgeGraph.from_triples([("p101", "r1", "p10083")], voc, 1)
    kg = KnowledgeGraph.from_triples([("p101", "r1", "p10083")], voc, 1, strict=False)
    assert kg.src.tolist() == [3] and kg.dst.tolist() == [2] and kg.rel.tolist() == [1]


def test_refusals(g, pairs):
    nt = ref.node_types(g, 1)
    ok = dict(src=g["src"], dst=g["dst"], rel=g["rel"], node_types=nt, Vr=ref.VR, Vt=ref.VT, end_relation=ref.END_REL, pairs=pairs, min_hops=1, max_hops=3,
              max_paths=5, T=4)
    _ffi.host_find_paths(**ok)

    def code(**kw):
        with pytest.raises(_ffi.KprnError) as ei:
            _ffi.host_find_paths(**{**ok, **kw})
        return ei.value.code

    def edge(arr, v):
        a = g[arr].copy()
        a[3] = v
        return {arr: a}

    Ve = g["Ve"]
    for kw in (edge("src", 0), edge("src", Ve), edge("dst", 0), edge("dst", Ve), edge("rel", 0), edge("rel", ref.VR + 1), dict(end_relation=0),
               dict(end_relation=ref.VR + 1), dict(pairs=np.array([[1, Ve]], np.int32)), dict(pairs=np.array([[0, 1]], np.int32))):
        assert code(**kw) == _ffi.E_INDEX, kw
    for bad in (0, ref.VT + 1):
        t = nt.copy()
        t[2, 0] = bad
        assert code(node_types=t) == _ffi.E_INDEX
    for kw in (dict(max_hops=4, T=5), dict(min_hops=0), dict(min_hops=3, max_hops=2), dict(T=3), dict(max_paths=0), dict(max_paths=4097), dict(F=2)):
        assert code(**kw) == _ffi.E_ARG, kw
