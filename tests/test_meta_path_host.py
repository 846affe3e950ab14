"""not gpu: meta-paths on the host (include/kprn.h "meta-paths") -- kprn_host_find_paths_patterns and kprn_host_find_candidates_patterns against the pure-Python
filter of tests/meta_path_ref.py over the brute-force path lists; that no patterns is the older twins bit for bit; the refusals; the text form and the
-meta_paths flag; the table builder and the match under AddressSanitizer as a stand-alone program.  Every comparison is integer equality."""
import itertools
import os
import subprocess
import types

import numpy as np
import pytest

from kprn_amd import _ffi, graph, model

from . import candidates_ref as cref
from . import candidates_top_ref as tref
from . import meta_path_ref as mp
from . import path_find_ref as ref
from . import path_walk_ref as wr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOPS = [(1, 3), (2, 3), (1, 1), (2, 2), (3, 3), (1, 5), (4, 5)]
CAPS = [ref.MAX_PATHS, 4096]
MODES = ["first", "spread"]
LAYOUTS = [(1, 3), (3, 7)]          # num_types, F: the two layouts of tests/test_path_find_host.py


@pytest.fixture(scope="module")
def small():
    g = ref.make_graph(40, 130, seed=5)
    return g, ref.pairs_of(g, 24, 11)


@pytest.fixture(scope="module")
def walked():
    return wr.make_inputs()


@pytest.fixture(scope="module")
def memo():
    return {}


def twin(g, nt, pairs, lo, hi, cap, T, walks, seed, draw, patterns, mode="first", **kw):
    return _ffi.host_find_paths_patterns(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, T, walks, seed, draw, cap=mode,
                                         patterns=patterns, **kw)


def same(got, want):
    return all(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))


def test_new_symbols_are_declared_exported_and_bound():
    from kprn_amd import build as kbuild
    declared = _ffi.declared_symbols()
    syms = subprocess.check_output(["nm", "-D", kbuild.build()]).decode()
    lua = open(os.path.join(ROOT, "bindings", "kprn.lua")).read()
    for s in ("kprn_graph_set_patterns", "kprn_graph_num_patterns", "kprn_host_find_paths_patterns", "kprn_host_find_candidates_patterns"):
        assert s in declared and " T %s" % s in syms and "int %s(" % s in lua, s
    assert "#define KPRN_PATTERN_MAX 32" in open(os.path.join(ROOT, "include", "kprn.h")).read() and _ffi.PATTERN_MAX == 32


def test_matches_is_the_rule():
    P = mp.FIXTURE
    assert mp.matches((3,), P) and not mp.matches((1,), P)
    assert mp.matches((2, 3), P) and not mp.matches((3, 1), P) and not mp.matches((1, 2), P)
    assert mp.matches((4, 2, 4), P) and mp.matches((1, 4, 3), P) and not mp.matches((2, 3, 2), P)
    assert mp.n_matching((1, 1, 4), P) == 2                      # both 3-hop patterns: still one path
    assert mp.matches((4, 1, 4, 3), P) and not mp.matches((4, 3, 4, 3), P)
    assert mp.matches((4, 4, 4, 4, 1), P) and mp.matches((3, 1, 1, 2, 2), P) and not mp.matches((4, 1, 1, 2, 2), P)
    assert not mp.matches((), P) and not mp.matches((1, 1, 1, 1, 1, 1), P)
    assert mp.keep([((1, 2), (1,))], None) == [((1, 2), (1,))]


def test_inputs_are_not_vacuous(small, walked, memo):
    """the figures the cases rest on, re-derived from the brute force and the filter"""
    g, pairs = small
    P = mp.FIXTURE
    full = mp.pair_lists(g, pairs, 1, 3, 0, 0, 0, None, memo)
    kept = mp.pair_lists(g, pairs, 1, 3, 0, 0, 0, P, memo)
    some = sum(1 for a, b in zip(full, kept) if 0 < len(b) < len(a))
    lost = sum(1 for a, b in zip(full, kept) if len(a) > 0 and len(b) == 0)
    twice = sum(1 for ps in full for _, rels in ps if mp.n_matching(rels, P) == 2)
    assert (some, lost, twice) == (6, 9, 4)
    names = [k for k, v in g["cases"].items() if isinstance(v, tuple)]
    exact, inside = names.index("exact"), names.index("inside")
    assert [rels for _, rels in kept[exact]] == [(1, 1), (1, 3), (2, 1), (1, 1, 1), (1, 1, 4)]      # the closing multi-edge 1, 2, 3 loses its MIDDLE relation
    assert [rels for _, rels in full[exact]][:3] == [(1, 1), (1, 2), (1, 3)]
    assert (len(full[inside]), len(kept[inside])) == (10, 9) and len(kept[inside]) > ref.MAX_PATHS   # the cap still binds after filtering
    g5, pairs5 = walked
    full5 = mp.pair_lists(g5, pairs5, 4, 5, wr.WALKS, wr.SEED, wr.DRAW, None, memo)
    kept5 = mp.pair_lists(g5, pairs5, 4, 5, wr.WALKS, wr.SEED, wr.DRAW, P, memo)
    assert len(pairs5) == 71
    assert sum(1 for a, b in zip(full5, kept5) if 0 < len(b) < len(a)) == 35
    assert sum(1 for a, b in zip(full5, kept5) if len(a) > 0 and len(b) == 0) == 14
    assert sum(1 for b in kept5 if len(b) > 28) == 3
    assert (len(full5[70]), len(kept5[70])) == (187, 118)       # the feeder row: its close walks the hub's 300 edges


@pytest.mark.parametrize("hops", HOPS)
def test_twin_equals_filtered_brute_force_small(small, memo, hops):
    g, pairs = small
    lo, hi = hops
    walks = wr.WALKS if hi > 3 else 0
    for (num_types, F), cap, mode in itertools.product(LAYOUTS, CAPS, MODES):
        nt = ref.node_types(g, num_types)
        for T, threads in ((hi + 1, 1), (hi + 2, 4)):
            want = mp.brute_find(g, nt, pairs, lo, hi, cap, T, F, walks, wr.SEED, wr.DRAW, mp.FIXTURE, mode, memo)
            got = twin(g, nt, pairs, lo, hi, cap, T, walks, wr.SEED, wr.DRAW, mp.FIXTURE, mode, F=F, threads=threads)
            assert same(got[1:], want[1:]), (num_types, F, cap, mode, T)
            assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (num_types, F, cap, mode, T)


@pytest.mark.parametrize("hops", [(1, 3), (1, 5), (4, 5)])
def test_twin_equals_filtered_brute_force_hub(walked, memo, hops):
    """the hub graph of the sampled hops' tests: long adjacencies, the feeder row, pairs over a cap of 28 after filtering"""
    g, pairs = walked
    lo, hi = hops
    nt = ref.node_types(g, 1)
    walks = wr.WALKS if hi > 3 else 0
    over = 0
    for cap, mode in itertools.product((7, 28, 4096), MODES):
        want = mp.brute_find(g, nt, pairs, lo, hi, cap, wr.T, 3, walks, wr.SEED, wr.DRAW, mp.FIXTURE, mode, memo)
        got = twin(g, nt, pairs, lo, hi, cap, wr.T, walks, wr.SEED, wr.DRAW, mp.FIXTURE, mode, threads=4)
        assert same(got, want), (cap, mode)
        over += int((want[2] > cap).sum())
    assert over > 0


def test_no_patterns_is_the_older_twin_bit_for_bit(small, walked):
    for (g, pairs), (lo, hi, walks) in itertools.product((small, walked), ((1, 3, 0), (1, 5, 64), (4, 5, 64))):
        nt = ref.node_types(g, 1)
        for cap, mode in itertools.product((7, 4096), MODES):
            want = _ffi.host_find_paths_cap(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, 6, walks, 1, 0, cap=mode)
            for none in (None, []):
                assert same(twin(g, nt, pairs, lo, hi, cap, 6, walks, 1, 0, none, mode), want), (lo, hi, cap, mode)
    # a single pattern of any relation per hop count is no filter either
    g, pairs = small
    nt = ref.node_types(g, 1)
    anything = [[None] * h for h in range(1, 6)]
    assert same(twin(g, nt, pairs, 1, 5, 7, 6, 64, 1, 0, anything), twin(g, nt, pairs, 1, 5, 7, 6, 64, 1, 0, None))


def test_bit_31_an_empty_match_and_an_inert_pattern(small, memo):
    g, pairs = small
    nt = ref.node_types(g, 1)
    # the only matching pattern is index 31 of 32
    only = [None, {1, 2}, {2, 4}]
    want = mp.brute_find(g, nt, pairs, 1, 3, 7, 4, 3, 0, 0, 0, [only], "first", memo)
    assert want[2].sum() > 0
    for index in (31, 0, 30):
        assert same(twin(g, nt, pairs, 1, 3, 7, 4, 0, 0, 0, mp.only_at(index, only)), want), index
    # a set that matches nothing: every pair is dropped
    idx, counts, found = twin(g, nt, pairs, 1, 3, 7, 4, 0, 0, 0, [[{ref.END_REL}]])
    assert idx.shape == (0, 4, 3) and not counts.any() and not found.any()
    # a pattern of 5 hops in a call that asks for 1..3 is inert ...
    three = [p for p in mp.FIXTURE if len(p) <= 3]
    assert same(twin(g, nt, pairs, 1, 3, 7, 4, 0, 0, 0, mp.FIXTURE), twin(g, nt, pairs, 1, 3, 7, 4, 0, 0, 0, three))
    # ... and an asked hop count that no pattern has yields no paths
    two = [[{1, 2}, {1, 3}]]
    a, b = twin(g, nt, pairs, 1, 3, 7, 4, 0, 0, 0, two), twin(g, nt, pairs, 2, 2, 7, 4, 0, 0, 0, two)
    assert same(a, b) and same(a, mp.brute_find(g, nt, pairs, 1, 3, 7, 4, 3, 0, 0, 0, two, "first", memo)) and a[2].sum() > 0
    assert not twin(g, nt, pairs, 3, 3, 7, 4, 0, 0, 0, two)[2].any()


def raw_twin(g, nt, pairs, hops, offs, rels, n, counts):
    C, fp = _ffi.C, _ffi._fp
    src, dst, rel = (np.ascontiguousarray(g[k], np.int32) for k in ("src", "dst", "rel"))
    arr = lambda a, t: None if a is None else np.array(a, t)
    hops, offs, rels = arr(hops, np.int32), arr(offs, np.int64), arr(rels, np.int32)
    return _ffi.lib().kprn_host_find_paths_patterns(fp(src), fp(dst), fp(rel), C.c_int64(len(src)), fp(nt), g["Ve"], ref.VR, ref.VT, 1, ref.END_REL, fp(pairs),
                                                    len(pairs), 1, 3, 7, 4, 3, 0, C.c_uint64(1), C.c_uint32(0), 0, 1, fp(counts), None, None, fp(hops), fp(offs),
                                                    fp(rels), n)


def test_refusals_write_nothing(small):
    g, pairs = small
    nt = ref.node_types(g, 1)
    bad = [
        ([1], [0, 1], [1], 33, _ffi.E_ARG), ([1], [0, 1], [1], -1, _ffi.E_ARG),                 # n outside 0..32
        ([0], [0], [1], 1, _ffi.E_ARG), ([6], [0, 1, 2, 3, 4, 5, 6], [1] * 6, 1, _ffi.E_ARG),   # a hop count outside 1..5
        ([2], [1, 1, 2], [1, 1], 1, _ffi.E_ARG), ([2], [0, 2, 1], [1, 1], 1, _ffi.E_ARG),       # offsets not ascending from 0
        (None, [0, 1], [1], 1, _ffi.E_ARG), ([1], None, [1], 1, _ffi.E_ARG), ([1], [0, 1], None, 1, _ffi.E_ARG),   # NULL arrays with n > 0
        ([1], [0, 1], [0], 1, _ffi.E_INDEX), ([2], [0, 1, 2], [1, ref.VR + 1], 1, _ffi.E_INDEX),                   # a relation outside 1..Vr
    ]
    for hops, offs, rels, n, code in bad:
        counts = np.full(len(pairs), -7, np.int32)
        assert raw_twin(g, nt, pairs, hops, offs, rels, n, counts) == code and (counts == -7).all(), (hops, offs, rels, n)
    # fine: repeated relations in a set, repeated patterns, the largest relation, NULL arrays with n == 0
    counts = np.full(len(pairs), -7, np.int32)
    assert raw_twin(g, nt, pairs, [2, 2], [0, 3, 5, 8, 10], [1, 2, 1, 1, 3, 1, 2, 1, 1, 3], 2, counts) == 0
    assert counts.tolist() == twin(g, nt, pairs, 1, 3, 7, 4, 0, 0, 0, [[{1, 2}, {1, 3}]])[1].tolist()
    assert raw_twin(g, nt, pairs, [1], [0, 1], [ref.VR], 1, counts) == 0 and raw_twin(g, nt, pairs, None, None, None, 0, counts) == 0
    with pytest.raises(_ffi.KprnError):
        twin(g, nt, pairs, 1, 3, 7, 4, 0, 0, 0, [[{1}]] * 33)


# ---- candidates --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cand_graphs():
    a = cref.graph_a()
    b = cref.graph_b()[:3]
    d = tref.graph_d()
    return dict(a=a, b=b, d=d)


def cand_twin(g, items, users, lo, hi, cap, exclude, patterns, **kw):
    return _ffi.host_find_candidates_patterns(g["src"], g["dst"], g["rel"], g["Ve"], items, users, lo, hi, cap, exclude, patterns, **kw)


def test_end_counts_is_the_finders_found(small):
    """the reference's one walk per user against the path lists: n_paths equals found, pair by pair, with and without the set"""
    g, pairs = small
    for P in (None, mp.FIXTURE):
        for u in sorted({int(u) for u, _ in pairs})[:12]:
            cnt = mp.end_counts(g, u, 1, 3, P)
            for c in range(1, g["Ve"]):
                assert cnt.get(c, 0) == len(mp.keep(ref.brute_paths(g, u, c, 1, 3), P)), (u, c)


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_candidates_twin_equals_filtered_candidates(cand_graphs, name):
    g, items, users = cand_graphs[name]
    differs = 0
    for (lo, hi), exclude in itertools.product(cref.HOPS, (0, 1)):
        plain = mp.candidates(g, items, users, lo, hi, exclude, mp.CAP_ALL, None)
        for cap in (3, mp.CAP_ALL):
            want = mp.candidates(g, items, users, lo, hi, exclude, cap, mp.FIXTURE)
            got = cand_twin(g, items, users, lo, hi, cap, exclude, mp.FIXTURE, threads=4)
            assert same(got, want), (lo, hi, exclude, cap)
        differs += int(not np.array_equal(plain[0], want[0]) or not np.array_equal(plain[2], want[2]))
        # no patterns: the older twins, bit for bit
        assert same(cand_twin(g, items, users, lo, hi, 3, exclude, None), _ffi.host_find_candidates_top(g["src"], g["dst"], g["rel"], g["Ve"], items, users, lo, hi,
                                                                                                       3, bool(exclude)))
        older = _ffi.host_find_candidates(g["src"], g["dst"], g["rel"], g["Ve"], items, users, lo, hi, bool(exclude))
        assert same(cand_twin(g, items, users, lo, hi, mp.CAP_ALL, exclude, None)[:2], older)
        assert same(older, plain[:2])
    assert differs > 0


def test_candidates_graph_c_and_refusals():
    g, items, users = cref.graph_c()
    # graph C at (2, 2): 8500 -1-> hub -(1 + e % 2)-> even e; [{1}, {2}] keeps the e with e % 2 == 1 among the evens: none; [{1}, {1}] keeps them all
    cand, gc, n_paths = cand_twin(g, items, users, 2, 2, mp.CAP_ALL, 1, [[{1}, {1}], [{2}, {1}]], threads=4)
    assert gc.tolist() == [4200, 2800] and cand[:4200].tolist() == cref.c_expected(8500) and cand[4200:].tolist() == cref.c_expected(8497) and (n_paths == 1).all()
    cand, gc, _ = cand_twin(g, items, users, 2, 2, mp.CAP_ALL, 1, [[{1}, {2}]])
    assert gc.tolist() == [0, 0] and len(cand) == 0
    with pytest.raises(_ffi.KprnError) as ei:
        cand_twin(g, items, users, 2, 2, 3, 1, [[{0}]])
    assert ei.value.code == _ffi.E_INDEX
    with pytest.raises(_ffi.KprnError) as ei:
        cand_twin(g, items, users, 2, 2, 3, 1, [[{1}] * 6])
    assert ei.value.code == _ffi.E_ARG


# ---- the text form, the KnowledgeGraph attribute, the flag ---------------------------------------------------------------------------------------
def named_kg(g, nt, patterns=None):
    vocabs = types.SimpleNamespace(relation={"rate": 0, "_rate": 1, "acted_by": 2, "has_type": 3, "#END_RELATION": 4, "#PAD_TOKEN": 5})
    return graph.KnowledgeGraph(g["src"], g["dst"], g["rel"], nt, ref.END_REL, ref.VR, ref.VT, vocabs, patterns)


def test_parse_meta_paths(small):
    g, _ = small
    kg = named_kg(g, ref.node_types(g, 1))
    text = ["# the schemas of the miner\n", "\n", "acted_by\n", "rate|_rate   rate|acted_by  # two hops\n", "* rate|_rate _rate|has_type\n", "rate * *\n",
            "   \t\n", "* _rate|rate * acted_by|rate\n", "rate|_rate|acted_by * * _rate|has_type *\n", "* * has_type * rate"]
    got = graph.parse_meta_paths(text, kg)
    assert got == [[sorted(s) if s else None for s in p] for p in mp.FIXTURE]
    assert graph.parse_meta_paths(graph.format_meta_paths(got, kg), kg) == got                     # round trip
    assert graph.parse_meta_paths(["# nothing\n", "\n"], kg) == []
    for lines, what in ((["rate\n", "rate|likes\n"], "line 2"), (["* * * * * *\n"], "line 1"), (["rate\n"] * 33, "line 33")):
        with pytest.raises(ValueError) as ei:
            graph.parse_meta_paths(lines, kg)
        assert what in str(ei.value), what
    assert len(graph.parse_meta_paths(["rate\n"] * 32, kg)) == 32


def test_knowledge_graph_carries_the_set(small):
    g, pairs = small
    nt = ref.node_types(g, 1)
    kg = named_kg(g, nt, mp.FIXTURE)
    assert same(kg.host_find_paths(pairs, 1, 3, 7, 4), twin(g, nt, pairs, 1, 3, 7, 4, 0, 0, 0, mp.FIXTURE))
    assert same(kg.host_find_paths(pairs, 1, 5, 7, 6, walks=64, seed=1, draw=2, cap="spread"), twin(g, nt, pairs, 1, 5, 7, 6, 64, 1, 2, mp.FIXTURE, "spread"))
    train, held = kg.holdout("rate", 0.8, 1)
    assert train.patterns is kg.patterns and len(held) > 0
    plain = named_kg(g, nt)
    assert plain.patterns is None and plain.holdout("rate", 0.8, 1)[0].patterns is None
    assert same(plain.host_find_paths(pairs, 1, 3, 7, 4), _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, 1, 3, 7, 4))


def test_flag_needs_kg(capsys, tmp_path):
    assert model.parse_flags([]).meta_paths == ""
    with pytest.raises(SystemExit) as ei:
        model.parse_flags(["-meta_paths", "schemas.txt"])
    assert ei.value.code != 0 and "-meta_paths needs -kg" in capsys.readouterr().err
    ok = model.parse_flags(["-kg", "t.tsv", "-vocab_dir", "d", "-interaction_rel", "rate", "-meta_paths", "schemas.txt"])
    assert ok.meta_paths == "schemas.txt"
    from kprn_amd import evaluate, recommend, train
    for main in (train.main, evaluate.main):
        with pytest.raises(SystemExit) as ei:
            main(["-meta_paths", "schemas.txt"])
        assert ei.value.code != 0 and "-meta_paths needs -kg" in capsys.readouterr().err
    with pytest.raises(SystemExit) as ei:
        recommend.main(["-vocab_dir", "none", "-user", "u0", "-meta_paths", "schemas.txt"])
    assert ei.value.code != 0 and "-kg" in capsys.readouterr().err


# ---- the table builder and the match under the sanitizers ----------------------------------------------------------------------------------------
def pattern_bytes(patterns):
    hops, offs, rels, n = _ffi._pattern_arrays(patterns)
    if n == 0:
        return np.array([0, 0], np.int64).tobytes()
    rels = rels[:int(offs[-1])]
    return np.array([n, len(rels)], np.int64).tobytes() + hops.tobytes() + offs.tobytes() + rels.tobytes()


def test_table_and_match_under_sanitizers(tmp_path):
    """tests/path_pattern_san_main.cpp: path_pattern_dev.h's builder and match over exact-size heap blocks, at Vr = 1 and the fixture's Vr, with 0, 1 and 32
    patterns; every sequence of up to 5 relations is matched and compared with meta_path_ref.matches"""
    exe = str(tmp_path / "path_pattern_san")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "kprn_amd", "csrc"), os.path.join(HERE, "path_pattern_san_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    sets = [(1, None), (1, [[{1}]]), (1, [[None, {1}]] * 32), (ref.VR, None), (ref.VR, [mp.FIXTURE[2]]), (ref.VR, mp.FIXTURE),
            (ref.VR, mp.only_at(31, mp.FIXTURE[5])), (ref.VR, (mp.FIXTURE * 5)[:32])]
    for k, (Vr, patterns) in enumerate(sets):
        seqs = [s for h in range(1, 6) for s in itertools.product(range(1, min(Vr, 4) + 1), repeat=h)]
        flat = np.array([x for s in seqs for x in (len(s),) + s], np.int32)
        src, dst = tmp_path / ("in%d" % k), tmp_path / ("out%d" % k)
        src.write_bytes(np.array([Vr, len(seqs), len(flat)], np.int64).tobytes() + pattern_bytes(patterns) + flat.tobytes())
        res = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        out = np.frombuffer(dst.read_bytes(), np.uint8)
        assert out[0] == 0 and len(out) == 1 + len(seqs)
        want = [1 if (not patterns or mp.matches(s, patterns)) else 0 for s in seqs] if patterns else [0] * len(seqs)
        assert out[1:].tolist() == want, k
        assert patterns is None or sum(want) > 0, k
