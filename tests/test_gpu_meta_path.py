"""gpu: meta-paths on the device (include/kprn.h "meta-paths") -- with a pattern set on the graph, every find and candidates call against the host twins
kprn_host_find_paths_patterns / kprn_host_find_candidates_patterns (themselves held to the pure-Python filter by tests/test_meta_path_host.py); clearing and
replacing the set; the refusals; one run on poisoned allocations; and the set through recommend_users, evaluate_from_graph and train_from_graph.  Every
comparison is integer equality."""
import io
import json
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph

from . import candidates_ref as cref
from . import candidates_top_ref as tref
from . import meta_path_ref as mp
from . import path_find_ref as ref
from . import path_walk_ref as wr
from .test_gpu_path_find import SHAPES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (16, 32, 16, 64, 2)   # dt, de, dr, H, L


def make_engine(g, **kw):
    return _ffi.Engine(ref.VT, g["Ve"], ref.VR, *SHAPE, **kw)


@pytest.fixture(scope="module")
def inputs():
    g, pairs = wr.make_inputs()
    assert len(pairs) == 71
    return g, pairs


@pytest.fixture(scope="module")
def nt(inputs):
    return ref.node_types(inputs[0], 1)


@pytest.fixture(scope="module")
def engine(inputs, nt):
    """-> (engine, the graph that carries the sets, a graph of the same edges that never had one)"""
    g = inputs[0]
    eng = make_engine(g)
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
    plain = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
    yield eng, gr, plain
    eng.close()


@pytest.fixture(scope="module")
def twin(inputs, nt):
    """the host twin's (idx, counts, found), computed once per argument set and left unchanged"""
    g = inputs[0]
    memo, sets = {}, {}

    def get(pairs, lo, hi, cap, T, walks, patterns, mode="first", seed=wr.SEED, draw=wr.DRAW):
        sets[id(patterns)] = patterns
        key = (pairs.tobytes(), lo, hi, cap, T, walks, id(patterns), mode, seed, draw)
        if key not in memo:
            memo[key] = _ffi.host_find_paths_patterns(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, T, walks, seed, draw,
                                                      cap=mode, patterns=patterns, threads=8)
            for a in memo[key]:
                a.setflags(write=False)
        return memo[key]
    return get


def read(batch):
    if batch is None:
        return np.zeros((0,), np.int32), np.zeros(0, np.int32)
    out = batch.read_idx(), batch.counts.copy()
    batch.free()
    return out


def device_equals(eng, gr, want, pairs, lo, hi, cap, T, walks, seed=wr.SEED, draw=wr.DRAW):
    idx, counts, found = want
    batch, c, f = eng.find_paths(gr, pairs, lo, hi, cap, T, walks=walks, seed=seed, draw=draw)
    what = (lo, hi, cap, walks)
    assert np.array_equal(c, counts) and np.array_equal(f, found), what
    if idx.shape[0] == 0:
        assert batch is None, what
        return
    assert batch is not None and batch.B == int((counts > 0).sum()) and batch.n_paths == idx.shape[0], what
    got, bc = read(batch)
    assert np.array_equal(bc, counts[counts > 0]) and np.array_equal(got, idx), what


@pytest.mark.parametrize("mode", ["first", "spread"])
@pytest.mark.parametrize("hops,walks", [((1, 3), 0), ((1, 5), 64), ((1, 5), 256), ((2, 3), 0), ((4, 5), 64)])
def test_find_paths_equals_twin(inputs, engine, twin, hops, walks, mode):
    eng, gr, _ = engine
    pairs = inputs[1]
    gr.set_patterns(mp.FIXTURE)
    assert gr.num_patterns() == len(mp.FIXTURE)
    eng.set_option("path_cap", mode)
    try:
        for cap in (7, 28):
            want = twin(pairs, hops[0], hops[1], cap, wr.T, walks, mp.FIXTURE, mode)
            unfiltered = twin(pairs, hops[0], hops[1], cap, wr.T, walks, None, mode)
            assert (want[2] > cap).any() and (want[2] == 0).any() and not np.array_equal(want[2], unfiltered[2])
            device_equals(eng, gr, want, pairs, hops[0], hops[1], cap, wr.T, walks)
    finally:
        eng.set_option("path_cap", "first")


def test_small_graph_both_layouts():
    """the planted pairs of the host test (the closing multi-edge that loses its middle relation; the cap that still binds), in both row layouts of
    tests/test_gpu_path_find.py: F = 3, and F = 4 with its leading column"""
    g = ref.make_graph(40, 130, seed=5)
    pairs = ref.pairs_of(g, 24, 11)
    nt = ref.node_types(g, 1)
    for F in (3, 4):
        eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, **SHAPES[F])
        gr = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
        gr.set_patterns(mp.FIXTURE)
        for lo, hi, walks in ((1, 3, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0), (1, 5, 64)):
            for cap in (ref.MAX_PATHS, 4096):
                want = _ffi.host_find_paths_patterns(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, hi + 1, walks, 1, 0,
                                                     patterns=mp.FIXTURE, F=F)
                device_equals(eng, gr, want, pairs, lo, hi, cap, hi + 1, walks, seed=1, draw=0)
        eng.close()


def test_bit_31_nothing_matches_inert_and_missing_hop_counts(inputs, engine, twin):
    eng, gr, _ = engine
    pairs = inputs[1]
    only = [None, {1, 2}, {2, 4}]
    one = [only]
    want = twin(pairs, 1, 3, 28, wr.T, 0, one)
    assert want[2].sum() > 0
    for index in (31, 0):
        gr.set_patterns(mp.only_at(index, only))
        assert gr.num_patterns() == 32
        device_equals(eng, gr, want, pairs, 1, 3, 28, wr.T, 0)
    gr.set_patterns([[{ref.END_REL}]])                       # nothing matches: every pair is dropped
    batch, c, f = eng.find_paths(gr, pairs, 1, 5, 28, wr.T, walks=64, seed=1, draw=0)
    assert batch is None and not c.any() and not f.any()
    two = [[{1, 2}, {1, 3}]]
    gr.set_patterns(two + [mp.FIXTURE[5]])                    # the 5-hop pattern is inert in a call of 1..3; hop counts 1 and 3 have no pattern
    device_equals(eng, gr, twin(pairs, 2, 2, 7, wr.T, 0, two), pairs, 1, 3, 7, wr.T, 0)
    batch, c, f = eng.find_paths(gr, pairs, 3, 3, 7, wr.T)
    assert batch is None and not f.any()


def test_clearing_and_replacing_the_set(inputs, engine, twin):
    eng, gr, plain = engine
    pairs = inputs[1]
    assert plain.num_patterns() == 0
    calls = [dict(lo=1, hi=3, walks=0), dict(lo=1, hi=5, walks=64)]
    find = lambda graph, k: eng.find_paths(graph, pairs, k["lo"], k["hi"], 28, wr.T, walks=k["walks"], seed=wr.SEED, draw=wr.DRAW)
    gr.set_patterns(mp.FIXTURE)
    for k in calls:
        filtered = find(gr, k)
        gr.set_patterns(None)
        assert gr.num_patterns() == 0
        cleared, never = find(gr, k), find(plain, k)
        a, b, c = read(filtered[0]), read(cleared[0]), read(never[0])
        assert b[0].tobytes() == c[0].tobytes() and b[1].tobytes() == c[1].tobytes()
        assert cleared[1].tobytes() == never[1].tobytes() and cleared[2].tobytes() == never[2].tobytes()
        assert a[0].tobytes() != b[0].tobytes()
        assert all(np.array_equal(x, y) for x, y in zip((c[0], never[1], never[2]), twin(pairs, k["lo"], k["hi"], 28, wr.T, k["walks"], None)))
        gr.set_patterns([])                                    # (the other spelling of no set)
        assert gr.num_patterns() == 0
        gr.set_patterns(mp.FIXTURE)
    # replacing a set takes effect on the next call
    other = [[{1}, None, None]]
    gr.set_patterns(other)
    device_equals(eng, gr, twin(pairs, 1, 3, 28, wr.T, 0, other), pairs, 1, 3, 28, wr.T, 0)
    gr.set_patterns(mp.FIXTURE)
    device_equals(eng, gr, twin(pairs, 1, 3, 28, wr.T, 0, mp.FIXTURE), pairs, 1, 3, 28, wr.T, 0)


def test_refusals_leave_the_previous_set(inputs, engine, twin):
    eng, gr, _ = engine
    pairs = inputs[1]
    gr.set_patterns(mp.FIXTURE)
    C, fp = _ffi.C, _ffi._fp
    arr = lambda a, t: None if a is None else np.array(a, t)
    bad = [
        ([1], [0, 1], [1], 33, _ffi.E_ARG), ([1], [0, 1], [1], -1, _ffi.E_ARG),
        ([0], [0], [1], 1, _ffi.E_ARG), ([6], [0, 1, 2, 3, 4, 5, 6], [1] * 6, 1, _ffi.E_ARG),
        ([2], [1, 1, 2], [1, 1], 1, _ffi.E_ARG), ([2], [0, 2, 1], [1, 1], 1, _ffi.E_ARG),
        (None, [0, 1], [1], 1, _ffi.E_ARG), ([1], None, [1], 1, _ffi.E_ARG), ([1], [0, 1], None, 1, _ffi.E_ARG),
        ([1], [0, 1], [0], 1, _ffi.E_INDEX), ([2], [0, 1, 2], [1, ref.VR + 1], 1, _ffi.E_INDEX),
    ]
    for hops, offs, rels, n, code in bad:
        h_, o_, r_ = arr(hops, np.int32), arr(offs, np.int64), arr(rels, np.int32)      # (held until the call has returned)
        rc = eng.L.kprn_graph_set_patterns(eng.h, gr.ptr, fp(h_), fp(o_), fp(r_), n)
        assert rc == code and gr.num_patterns() == len(mp.FIXTURE), (hops, offs, rels, n)
    with pytest.raises(_ffi.KprnError):
        gr.set_patterns([[{1}]] * 33)
    device_equals(eng, gr, twin(pairs, 1, 3, 7, wr.T, 0, mp.FIXTURE), pairs, 1, 3, 7, wr.T, 0)      # the previous set, intact


def training_pairs(eng, gr, s, pos, n_neg, seed, draw, attempts):
    neg, _ = eng.sample_negatives(gr, s, pos[:, 0], n_neg, seed, draw, max_attempts=attempts)
    prs = np.zeros((len(pos), 1 + n_neg, 2), np.int32)
    prs[:, :, 0] = pos[:, :1]
    prs[:, 0, 1] = pos[:, 1]
    prs[:, 1:, 1] = neg
    return prs.reshape(-1, 2)


@pytest.mark.parametrize("max_hops,walks", [(3, 0), (5, 64)])
def test_training_call_equals_sample_then_find(inputs, engine, max_hops, walks):
    g, pairs = inputs
    eng, gr, plain = engine
    gr.set_patterns(mp.FIXTURE)
    c = g["cases"]
    s = eng.sampler(np.arange(1, 300, dtype=np.int32))
    pos = np.array([c["exact"], c["hub_user"], tuple(pairs[7]), c["feeder"], tuple(pairs[8]), c["hub_next"]], np.int32)
    n_neg, seed, draw, cap, attempts = 6, 7, 2, 7, 4
    prs = training_pairs(eng, gr, s, pos, n_neg, seed, draw, attempts)
    assert np.array_equal(prs, training_pairs(eng, plain, s, pos, n_neg, seed, draw, attempts))       # the sampler's adjacency test sees every relation
    labels = np.zeros(len(prs), np.float32)
    labels[::1 + n_neg] = 1
    stand_in = np.where(prs[:, 1:] == 0, prs[:, :1], prs[:, 1:])
    want_b, wc, wf = eng.find_paths(gr, np.concatenate([prs[:, :1], stand_in], axis=1), 1, max_hops, cap, wr.T, labels=labels, walks=walks, seed=seed, draw=draw)
    got_b, got_prs, gc, gf = eng.find_training_paths(gr, s, pos, n_neg, seed, draw, 1, max_hops, cap, wr.T, max_attempts=attempts, walks=walks)
    assert np.array_equal(got_prs, prs) and np.array_equal(gc, wc) and np.array_equal(gf, wf) and wf.sum() > 0
    assert got_b.has_labels and np.array_equal(got_b.counts, want_b.counts) and np.array_equal(got_b.read_idx(), want_b.read_idx())
    assert all(mp.matches(r, mp.FIXTURE) for r in mp.rels_of_rows(got_b.read_idx(), ref.VR))
    got_b.free(); want_b.free(); s.free()


# ---- candidates --------------------------------------------------------------------------------------------------------------------------------
def candidate_cases(name):
    if name == "a":
        return cref.graph_a()
    if name == "b":
        return cref.graph_b()[:3]
    if name == "c":
        return cref.graph_c()
    return tref.graph_d()


PATTERNS_C = [[{1}, {1}], [{2}, {1}], [{3}]]


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_candidates_equal_twin_and_their_paths_are_the_lists_rows(name):
    g, items, users = candidate_cases(name)
    patterns = PATTERNS_C if name == "c" else mp.FIXTURE
    nt = ref.node_types(g, 1)
    eng = make_engine(g)
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
    gr.set_patterns(patterns)
    sm = eng.sampler(items)
    hops = ((2, 2), (1, 2)) if name == "c" else cref.HOPS
    checked = 0
    for (lo, hi), exclude in ((h, e) for h in hops for e in (0, 1)):
        for cap in (0, 3):
            want, wgc, wn = _ffi.host_find_candidates_patterns(g["src"], g["dst"], g["rel"], g["Ve"], items, users, lo, hi, cap or mp.CAP_ALL, exclude, patterns,
                                                               threads=8)
            listed, gc = eng.find_candidates(gr, sm, users, lo, hi, exclude, cap=cap)
            assert np.array_equal(gc, wgc) and np.array_equal(listed[:, 1], want) and np.array_equal(listed[:, 0], np.repeat(users, wgc)), (lo, hi, exclude, cap)
            if cap:
                assert np.array_equal(eng.candidate_path_counts(), wn), (lo, hi, exclude, cap)
            if len(listed) == 0 or (name == "c" and cap == 0 and exclude == 0):
                continue
            # pair p is the list's row p: every candidate has a matching path, n_paths equals found
            batch, c, f = eng.find_paths_of_candidates(gr, len(listed), lo, hi, 5, 4)
            assert (f > 0).all() and batch.B == len(listed), (lo, hi, exclude, cap)
            if cap:
                assert np.array_equal(f, wn)
            idx, _ = read(batch)
            off = np.concatenate([[0], np.cumsum(c)])
            assert np.array_equal(idx[off[:-1], -1, -2], listed[:, 1]) and all(mp.matches(r, patterns) for r in mp.rels_of_rows(idx, ref.VR))
            checked += 1
    assert checked > 0
    # changing the patterns between making a list and finding its paths is allowed: the pairs that end up with no path are dropped
    listed, _ = eng.find_candidates(gr, sm, users, 1, 2, 1)
    gr.set_patterns([[{ref.END_REL}]])
    batch, c, f = eng.find_paths_of_candidates(gr, len(listed), 1, 2, 5, 4)
    assert batch is None and not f.any()
    eng.close()


# ---- nothing depends on what hipMalloc returns ---------------------------------------------------------------------------------------------------
def test_filtered_calls_do_not_depend_on_what_hipmalloc_returns(inputs, twin):
    """filtered find (both cap modes, sampled hops) and candidates in a fresh process with KPRN_POISON_ALLOC=1 (every new device allocation filled with 0xFF bytes)"""
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r)
        import numpy as np
        from kprn_amd import _ffi
        from tests import path_find_ref as ref, path_walk_ref as wr, meta_path_ref as mp
        g, pairs = wr.make_inputs()
        eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, 16, 32, 16, 64, 2)
        gr = eng.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL)
        gr.set_patterns(mp.FIXTURE)
        sm = eng.sampler(np.arange(1, 381, dtype=np.int32))
        out = []
        for mode in ("first", "spread"):
            eng.set_option("path_cap", mode)
            b, c, f = eng.find_paths(gr, pairs, 1, 5, 7, wr.T, walks=64, seed=wr.SEED, draw=wr.DRAW)
            out.append([b.read_idx().ravel().tolist(), c.tolist(), f.tolist()])
            b.free()
        eng.set_option("path_cap", "first")
        users = pairs[:12, 0].copy()
        for cap in (0, 3):
            listed, gc = eng.find_candidates(gr, sm, users, 1, 3, 1, cap=cap)
            out.append([listed.ravel().tolist(), gc.tolist(), eng.candidate_path_counts().tolist() if cap else []])
        eng.close()
        print(json.dumps(out))
    """) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    g, pairs = inputs
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for (idx, c, f), mode in zip(out[:2], ("first", "spread")):
        want = twin(pairs, 1, 5, 7, wr.T, 64, mp.FIXTURE, mode)
        assert np.array_equal(np.array(idx, np.int32), want[0].ravel()) and np.array_equal(c, want[1]) and np.array_equal(f, want[2]), mode
    users = pairs[:12, 0].copy()
    for (listed, gc, n_paths), cap in zip(out[2:], (0, 3)):
        want, wgc, wn = _ffi.host_find_candidates_patterns(g["src"], g["dst"], g["rel"], g["Ve"], np.arange(1, 381, dtype=np.int32), users, 1, 3, cap or mp.CAP_ALL,
                                                           1, mp.FIXTURE)
        assert np.array_equal(np.array(listed, np.int32).reshape(-1, 2)[:, 1], want) and np.array_equal(gc, wgc) and wgc.sum() > 0
        assert not cap or np.array_equal(n_paths, wn)


# ---- the set through the chains ------------------------------------------------------------------------------------------------------------------
D_PATTERNS = [[{1}], [{1, 3}, {2, 4}, {1}]]           # graph D: rate; (rate | also) (_rate | _also) rate


@pytest.fixture(scope="module")
def world():
    g = tref.graph_d()[0]
    vocabs = types.SimpleNamespace(relation={"rate": 0, "_rate": 1, "also": 2, "_also": 3, "#END_RELATION": 4, "#PAD_TOKEN": 5})
    kg = kgraph.KnowledgeGraph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL, ref.VR, ref.VT, vocabs, D_PATTERNS)
    eng = make_engine(g, param_init=0.35, seed=5)
    yield kg, eng
    eng.close()


class Spy:
    """every batch a find call of the engine hands out has its relation sequences checked against the set before the chain goes on"""

    def __init__(self, eng, name, patterns, which=0):
        self.eng, self.name, self.patterns, self.which, self.rows = eng, name, patterns, which, 0
        self.inner = getattr(eng, name)

    def __enter__(self):
        def spy(*a, **kw):
            out = self.inner(*a, **kw)
            if out[self.which] is not None:
                seqs = mp.rels_of_rows(out[self.which].read_idx(), ref.VR)
                assert all(mp.matches(r, self.patterns) for r in seqs)
                self.rows += len(seqs)
            return out
        setattr(self.eng, self.name, spy)
        return self

    def __exit__(self, *exc):
        delattr(self.eng, self.name)


def test_recommend_evaluate_and_train_carry_the_set(world):
    kg, eng = world
    users = np.array([1, 2, 325], np.int32)
    catalogue = np.unique(kg.interactions("rate")[:, 1])
    sm = eng.sampler(catalogue)
    with Spy(eng, "find_paths_of_candidates", D_PATTERNS) as spy:
        res = kgraph.recommend_users(eng, kg, sm, users, 5, 3, max_paths=7)
    assert kg.on(eng).num_patterns() == len(D_PATTERNS) and spy.rows > 0
    assert all(len(r) > 0 for r in res)
    for r in res:
        for item in r:
            assert item["paths"] and all(mp.matches(s, D_PATTERNS) for s in mp.rels_of_rows(np.stack([ids for ids, _, _ in item["paths"]]), ref.VR))
    # the candidates are the members the filtered finder reaches: the 2-hop walks that the unfiltered graph offers are gone
    want, wgc, _ = _ffi.host_find_candidates_patterns(kg.src, kg.dst, kg.rel, kg.Ve, catalogue, users, 1, 3, mp.CAP_ALL, True, D_PATTERNS)
    listed, gc = eng.find_candidates(kg.on(eng), sm, users, 1, 3, True)
    assert np.array_equal(gc, wgc) and np.array_equal(listed[:, 1], want)
    # -holdout's train graph carries the set, and the evaluation runs on it
    train_kg, held = kg.holdout("rate", 0.8, 1)
    assert train_kg.patterns is kg.patterns
    sm_t = eng.sampler(np.unique(train_kg.interactions("rate")[:, 1]))
    with Spy(eng, "find_paths_of_candidates", D_PATTERNS) as spy:
        out = kgraph.evaluate_from_graph(eng, train_kg, held, sm_t, users_per_call=8, max_paths=7, max_users=8)
    assert train_kg.on(eng).num_patterns() == len(D_PATTERNS) and spy.rows > 0 and out["n"] > 0
    theta = eng.get_flat_params()
    with Spy(eng, "find_training_paths", D_PATTERNS) as spy:
        hist = kgraph.train_from_graph(eng, train_kg, train_kg.interactions("rate")[:48], _ffi.make_opt(method=1, lr=1e-3), 16, 2, 1, 3, sampler=sm_t, min_hops=1,
                                       max_hops=3, max_paths=7, out=io.StringIO())
    eng.set_flat_params(theta)
    assert len(hist) == 1 and np.isfinite(hist).all() and spy.rows > 0
    # the attribute replaced: the device graph follows on the next .on(eng)
    kg.patterns = None
    assert kg.on(eng).num_patterns() == 0
    kg.patterns = D_PATTERNS
    assert kg.on(eng).num_patterns() == len(D_PATTERNS)
    sm.free(); sm_t.free()
