"""not gpu: the cap mode "spread" on the host (include/kprn.h "finding a pair's paths", cap mode) -- kprn_host_find_paths_cap and kprn_host_cap_select against
the brute-force restatement in tests/path_cap_ref.py; the properties of a selection; its inclusion frequencies; the -path_cap flag.  Every comparison of ids and
ranks is exact."""
import itertools
import math

import numpy as np
import pytest

from kprn_amd import _ffi, graph, model

from . import path_cap_ref as cr
from . import path_find_ref as ref
from . import path_walk_ref as wr

HOPS = [(1, 3), (2, 3), (1, 5), (4, 5)]
CAPS = [1, 7, 28, 4096]
WALKS = [1, 64]
LAYOUTS = list(itertools.product([6, 7], [1, 4]))       # T, threads


@pytest.fixture(scope="module")
def inputs():
    return wr.make_inputs()


@pytest.fixture(scope="module")
def memo():
    return {}, {}


def twin(g, nt, pairs, lo, hi, cap, T, walks, seed, draw, mode="spread", **kw):
    return _ffi.host_find_paths_cap(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, T, walks, seed, draw, cap=mode, **kw)


def test_new_symbols_are_declared_and_exported():
    import subprocess
    from kprn_amd import build as kbuild
    declared = _ffi.declared_symbols()
    syms = subprocess.check_output(["nm", "-D", kbuild.build()]).decode()
    for s in ("kprn_host_find_paths_cap", "kprn_host_cap_select"):
        assert s in declared, s
        assert " T %s" % s in syms, s


def test_inputs_leave_pairs_over_every_cap(inputs, memo):
    """the figures the issue's cases rest on, re-derived from the brute force"""
    g, pairs = inputs
    nt = ref.node_types(g, 1)
    f3 = wr.brute_find(g, nt, pairs, 1, 3, cr.ALL, 6, 3, 0, 0, 0, memo[0])[2]
    f5 = wr.brute_find(g, nt, pairs, 1, 5, cr.ALL, 6, 3, wr.WALKS, wr.SEED, wr.DRAW, memo[0])[2]
    assert len(pairs) == 71 and (f3[7], f3[8]) == (689, 121) and (f5[7], f5[8], f5[70]) == (924, 262, 187)
    for cap in (1, 7, 28):
        assert (f3 > cap).sum() >= 2 and (f5 > cap).sum() >= 2, cap
    assert max(f3.max(), f5.max()) <= cr.ALL


@pytest.mark.parametrize("hops", HOPS)
def test_twin_equals_restatement(inputs, memo, hops):
    g, pairs = inputs
    lo, hi = hops
    nt = ref.node_types(g, 1)
    over = 0
    for walks, cap, (T, threads) in itertools.product(WALKS, CAPS, LAYOUTS):
        want = cr.brute_find(g, nt, pairs, lo, hi, cap, T, 3, walks, wr.SEED, wr.DRAW, memo[0], memo[1])
        got = twin(g, nt, pairs, lo, hi, cap, T, walks, wr.SEED, wr.DRAW, threads=threads)
        what = (walks, cap, T, threads)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
        assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), what
        over += int((want[2] > cap).sum())
    assert over > 0


def test_cap_select_equals_restatement():
    for F, K, b, seed, draw in ((689, 28, 7, 1, 0), (924, 7, 7, 1, 3), (10, 3, 0, 1, 0), (29, 28, 5, 0xDEADBEEF12345678, 9), (4097, 4096, 2, 1, 1),
                                (5, 28, 1, 1, 0), (28, 28, 1, 1, 0), (0, 28, 0, 1, 0), (1, 1, 0, 1, 0), ((1 << 51) - 1, 4096, 3, 2, 4), (12345678901, 1, 0, 1, 2 ** 32 - 1)):
        got = _ffi.host_cap_select(F, K, b, seed, draw)
        assert got.dtype == np.int64 and got.tolist() == cr.select(F, K, b, seed, draw), (F, K, b)
    for bad in ((-1, 28, 0), (1 << 51, 28, 0), (10, 0, 0), (10, 4097, 0), (10, 3, -1)):
        with pytest.raises(_ffi.KprnError) as ei:
            _ffi.host_cap_select(*bad, 1, 0)
        assert ei.value.code == _ffi.E_ARG, bad


def test_mode_first_and_pairs_under_the_cap_are_the_sampled_call(inputs):
    g, pairs = inputs
    nt = ref.node_types(g, 1)
    sampled = lambda lo, hi, cap, walks: _ffi.host_find_paths_sampled(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, wr.T,
                                                                      walks, wr.SEED, wr.DRAW)
    for lo, hi, cap, walks in ((1, 3, 7, 0), (1, 5, 28, 64), (4, 5, 7, 64), (2, 3, 1, 0)):
        want = sampled(lo, hi, cap, walks)
        got = twin(g, nt, pairs, lo, hi, cap, wr.T, walks, wr.SEED, wr.DRAW, mode="first")
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (lo, hi, cap)
    # F <= K for every pair: "spread" keeps everything, as "first" does
    want = sampled(1, 5, 4096, 64)
    got = twin(g, nt, pairs, 1, 5, 4096, wr.T, 64, wr.SEED, wr.DRAW)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # ... and pair by pair at a cap some pairs stay under
    first, spread = sampled(1, 3, 28, 0), twin(g, nt, pairs, 1, 3, 28, wr.T, 0, wr.SEED, wr.DRAW)
    off = np.concatenate([[0], np.cumsum(first[1])])
    under = [b for b in range(len(pairs)) if 0 < first[2][b] <= 28]
    assert under and (first[2] > 28).any() and not np.array_equal(first[0], spread[0])
    for b in under:
        assert np.array_equal(first[0][off[b]:off[b + 1]], spread[0][off[b]:off[b + 1]]), b
    # a cap mode that does not exist is refused and writes nothing
    C, fp = _ffi.C, _ffi._fp
    src, dst, rel = (np.ascontiguousarray(g[k], np.int32) for k in ("src", "dst", "rel"))
    for mode in (2, -1):
        counts = np.full(len(pairs), -7, np.int32)
        rc = _ffi.lib().kprn_host_find_paths_cap(fp(src), fp(dst), fp(rel), C.c_int64(len(src)), fp(nt), g["Ve"], ref.VR, ref.VT, 1, ref.END_REL, fp(pairs), len(pairs),
                                                 1, 3, 7, 4, 3, 0, C.c_uint64(1), C.c_uint32(0), mode, 1, fp(counts), None, None)
        assert rc == _ffi.E_ARG and (counts == -7).all(), mode


def test_kept_ranks_ascend_one_in_each_stratum():
    for F, K in ((689, 28), (924, 7), (29, 28), (57, 28), (10, 3), (4097, 4096), (100000, 4096), ((1 << 51) - 1, 4096), (2, 1)):
        lo = cr.bounds(F, K)
        sizes = {b - a for a, b in zip(lo[:-1], lo[1:])}
        assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1 and sizes <= {F // K, -(-F // K)}, (F, K)
        for b, draw in ((0, 0), (7, 1), (70, 12345)):
            r = _ffi.host_cap_select(F, K, b, 1, draw).tolist()
            assert len(r) == K and all(x < y for x, y in zip(r[:-1], r[1:])), (F, K)
            assert all(lo[j] <= r[j] < lo[j + 1] and cr.stratum_of(r[j], F, K) == j for j in range(K)), (F, K)
    for F, K in ((10, 3), (57, 28), (689, 28)):       # the stratum formula, rank by rank
        lo = cr.bounds(F, K)
        assert [cr.stratum_of(r, F, K) for r in range(F)] == [j for j in range(K) for _ in range(lo[j + 1] - lo[j])]


def test_draw_seed_and_row_address_the_subset(inputs):
    base = _ffi.host_cap_select(689, 28, 7, 1, 0).tolist()
    assert base == _ffi.host_cap_select(689, 28, 7, 1, 0).tolist()
    for b, seed, draw in ((7, 1, 1), (8, 1, 0), (7, 2, 0), (7, 1 + (1 << 32), 0)):
        assert _ffi.host_cap_select(689, 28, b, seed, draw).tolist() != base, (b, seed, draw)
    # the same through the finder: another draw gives other rows, and the same pair in two rows draws two subsets
    g, pairs = inputs
    nt = ref.node_types(g, 1)
    run = lambda pr, draw: twin(g, nt, pr, 1, 3, 28, wr.T, 0, wr.SEED, draw)
    one, again, other = run(pairs, 0), run(pairs, 0), run(pairs, 1)
    assert np.array_equal(one[0], again[0]) and one[0].shape == other[0].shape and not np.array_equal(one[0], other[0])
    idx, counts, found = run(np.stack([pairs[7]] * 3), 0)
    assert counts.tolist() == [28] * 3 and found.tolist() == [689] * 3
    assert len({idx[28 * k:28 * (k + 1)].tobytes() for k in range(3)}) == 3
    assert np.array_equal(idx[:28], twin(g, nt, pairs[7:8], 1, 3, 28, wr.T, 0, wr.SEED, 0)[0])     # (row 0 either way)


def test_a_stratum_of_one_is_always_kept():
    K = 28
    lo = cr.bounds(K + 1, K)
    ones = [lo[j] for j in range(K) if lo[j + 1] - lo[j] == 1]
    assert len(ones) == K - 1
    for draw in range(50):
        assert set(ones) <= set(_ffi.host_cap_select(K + 1, K, 3, 1, draw).tolist())


@pytest.mark.parametrize("F,K", [(10, 3), (57, 28), (29, 28)])
def test_inclusion_frequencies(F, K):
    """over draws 0..3999 (seed 1, row 0) rank r of a stratum of size s is kept n / s times within 5 standard deviations sqrt(n p (1 - p)), p = 1 / s, and
    exactly n times where s = 1.  (With the rule as written the worst deviations are 1.93, 2.43 and 1.11 standard deviations: the bound tests the rule.)"""
    n = 4000
    hits = np.zeros(F, np.int64)
    for draw in range(n):
        hits[_ffi.host_cap_select(F, K, 0, 1, draw)] += 1
    lo = cr.bounds(F, K)
    worst = 0.0
    for j in range(K):
        s = lo[j + 1] - lo[j]
        for r in range(lo[j], lo[j + 1]):
            if s == 1:
                assert hits[r] == n, r
            else:
                p = 1.0 / s
                dev = abs(hits[r] - n * p) / math.sqrt(n * p * (1 - p))
                worst = max(worst, dev)
                assert dev <= 5.0, (r, int(hits[r]), n * p)
    print("worst deviation (F, K) = (%d, %d): %.2f standard deviations" % (F, K, worst))
    assert hits.sum() == n * K


def test_knowledge_graph_twin_takes_the_cap(inputs):
    g, pairs = inputs
    nt = ref.node_types(g, 1)
    kg = graph.KnowledgeGraph(g["src"], g["dst"], g["rel"], nt, ref.END_REL, ref.VR, ref.VT)
    for walks, hi in ((0, 3), (64, 5)):
        want = twin(g, nt, pairs, 1, hi, 7, wr.T, walks, 1, 2)
        got = kg.host_find_paths(pairs, 1, hi, 7, wr.T, walks=walks, seed=1, draw=2, cap="spread")
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        first = kg.host_find_paths(pairs, 1, hi, 7, wr.T, walks=walks, seed=1, draw=2)
        assert all(np.array_equal(a, b) for a, b in zip(first, kg.host_find_paths(pairs, 1, hi, 7, wr.T, walks=walks, seed=1, draw=2, cap="first")))
        assert not np.array_equal(first[0], got[0])
    with pytest.raises(_ffi.KprnError):
        kg.host_find_paths(pairs, 1, 3, 7, wr.T, cap="bogus")


def test_flag_parsing(capsys):
    assert model.parse_flags([]).path_cap == "first"
    assert model.parse_flags(["-path_cap", "spread"]).path_cap == "spread"
    assert model.parse_flags(["-path_cap", "first"]).path_cap == "first"
    with pytest.raises(SystemExit) as ei:
        model.parse_flags(["-path_cap", "bogus"])
    assert ei.value.code != 0 and "-path_cap" in capsys.readouterr().err


def test_command_lines_name_the_flag_before_an_engine_exists(capsys):
    from kprn_amd import evaluate, recommend
    with pytest.raises(SystemExit) as ei:
        recommend.main(["-kg", "none.tsv", "-vocab_dir", "none", "-user", "u0", "-items", "none.txt", "-path_cap", "bogus"])
    assert ei.value.code != 0 and "-path_cap" in capsys.readouterr().err
    with pytest.raises(SystemExit) as ei:
        evaluate.main(["-kg", "none.tsv", "-vocab_dir", "none", "-interaction_rel", "rate", "-holdout", "0.2", "-path_cap", "bogus"])
    assert ei.value.code != 0 and "-path_cap" in capsys.readouterr().err
