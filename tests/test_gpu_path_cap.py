"""gpu: option "path_cap" = "spread" (include/kprn.h "finding a pair's paths", cap mode) -- every find call that carries a seed against the host twin
kprn_host_find_paths_cap (itself held to a brute-force restatement by tests/test_path_cap_host.py), the option's way back to "first", and the found batch
through scoring, training, recommending and train_from_graph.  Every comparison is np.array_equal."""
import io

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph

from . import path_find_ref as ref
from . import path_walk_ref as wr
from .test_gpu_path_find import SHAPES

pytestmark = pytest.mark.gpu


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
    """an engine of this file's own (SHAPES[3]: D = H = 64, L = 2, F = 3, the fused path): the option never reaches another file's handle"""
    g = inputs[0]
    eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, **SHAPES[3])
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
    yield eng, gr
    eng.close()


@pytest.fixture(scope="module")
def before(inputs, engine):
    """what three calls return on the handle BEFORE the option is ever set (every test that sets it asks for this fixture first)"""
    eng, gr = engine
    assert "path_cap" not in eng.options
    out = {}
    for key, kw in (("seeded3", dict(walks=0, seed=1, draw=0)), ("sampled", dict(walks=wr.WALKS, seed=wr.SEED, draw=wr.DRAW))):
        b, c, f = eng.find_paths(gr, inputs[1], 1, 5 if kw["walks"] else 3, 28, wr.T, **kw)
        out[key] = (b.read_idx(), c, f)
        b.free()
    return out


@pytest.fixture(scope="module")
def twin(inputs, nt):
    """the host twin's (idx, counts, found) under "spread", computed once per argument set and left unchanged"""
    g = inputs[0]
    memo = {}

    def get(pairs, lo, hi, cap, T, walks, seed=wr.SEED, draw=wr.DRAW, mode="spread"):
        key = (pairs.tobytes(), lo, hi, cap, T, walks, seed, draw, mode)
        if key not in memo:
            memo[key] = _ffi.host_find_paths_cap(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, T, walks, seed, draw, cap=mode,
                                                 threads=8)
            for a in memo[key]:
                a.setflags(write=False)
        return memo[key]
    return get


@pytest.fixture()
def spread(engine, before):
    eng, _ = engine
    eng.set_option("path_cap", "spread")
    yield
    eng.set_option("path_cap", "first")


def same_as_twin(eng, gr, twin, pairs, lo, hi, cap, T, walks, seed=wr.SEED, draw=wr.DRAW):
    idx, counts, found = twin(pairs, lo, hi, cap, T, walks, seed, draw)
    batch, c, f = eng.find_paths(gr, pairs, lo, hi, cap, T, walks=walks, seed=seed, draw=draw)
    what = (lo, hi, cap, walks)
    assert np.array_equal(c, counts) and np.array_equal(f, found), what
    assert batch is not None and batch.B == int((counts > 0).sum()) and batch.n_paths == idx.shape[0], what
    assert np.array_equal(batch.counts, counts[counts > 0]) and np.array_equal(batch.read_idx(), idx), what
    batch.free()
    return counts, found


@pytest.mark.parametrize("hops,walks,max_paths", [((1, 3), 0, 1), ((1, 3), 0, 7), ((1, 3), 0, 28), ((1, 5), 64, 7), ((1, 5), 64, 28), ((4, 5), 64, 28)])
def test_device_equals_twin(inputs, engine, twin, spread, hops, walks, max_paths):
    eng, gr = engine
    pairs = inputs[1]
    _, found = same_as_twin(eng, gr, twin, pairs, hops[0], hops[1], max_paths, wr.T, walks)
    assert (found > max_paths).sum() >= 2 and (found == 0).any()
    first = twin(pairs, hops[0], hops[1], max_paths, wr.T, walks, mode="first")
    assert not np.array_equal(first[0], twin(pairs, hops[0], hops[1], max_paths, wr.T, walks)[0])      # (the case tells the two modes apart)


def test_other_seed_draw_layout_and_a_cap_nothing_reaches(inputs, engine, twin, spread):
    eng, gr = engine
    pairs = inputs[1]
    same_as_twin(eng, gr, twin, pairs, 1, 5, 28, wr.T, wr.WALKS, seed=0xDEADBEEF12345678, draw=9)
    same_as_twin(eng, gr, twin, pairs, 2, 3, 7, 4, 0, seed=3, draw=2 ** 32 - 1)
    same_as_twin(eng, gr, twin, pairs[7:9], 1, 3, 28, wr.T, 0)                # rows 0 and 1 of a two-pair list: the counter holds the row
    _, found = same_as_twin(eng, gr, twin, pairs, 1, 5, 4096, wr.T, wr.WALKS)      # F <= K everywhere: every path, as "first"
    assert found.max() <= 4096


def test_find_paths_without_a_seed_keeps_the_first(inputs, engine, spread):
    """kprn_find_paths has no seed: the library keeps the first paths whatever the option says (Engine.find_paths itself routes to the seeded call)"""
    eng, gr = engine
    pairs = np.ascontiguousarray(inputs[1], np.int32)
    C = _ffi.C
    counts, found, ptr = np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.int64), C.c_void_p()
    eng._ck(eng.L.kprn_find_paths(eng.h, gr.ptr, _ffi._fp(pairs), None, len(pairs), 1, 3, 28, wr.T, _ffi._fp(counts), _ffi._fp(found), C.byref(ptr)))
    batch = _ffi.Batch._adopt(eng, ptr, counts[counts > 0].copy(), wr.T, eng.cfg.F, False)
    want = _ffi.host_find_paths(inputs[0]["src"], inputs[0]["dst"], inputs[0]["rel"], ref.node_types(inputs[0], 1), ref.VR, ref.VT, ref.END_REL, pairs, 1, 3, 28, wr.T)
    assert np.array_equal(batch.read_idx(), want[0]) and np.array_equal(counts, want[1]) and np.array_equal(found, want[2])
    batch.free()


def training_pairs(eng, gr, s, pos, n_neg, seed, draw, attempts):
    neg, _ = eng.sample_negatives(gr, s, pos[:, 0], n_neg, seed, draw, max_attempts=attempts)
    prs = np.zeros((len(pos), 1 + n_neg, 2), np.int32)
    prs[:, :, 0] = pos[:, :1]
    prs[:, 0, 1] = pos[:, 1]
    prs[:, 1:, 1] = neg
    return prs.reshape(-1, 2)


@pytest.mark.parametrize("max_hops,walks", [(5, 64), (3, 0), (3, 64)])
def test_training_call_equals_sample_then_find(inputs, engine, spread, max_hops, walks):
    g, pairs = inputs
    eng, gr = engine
    c = g["cases"]
    s = eng.sampler(np.arange(1, 300, dtype=np.int32))
    pos = np.array([c["exact"], c["hub_user"], tuple(pairs[7]), c["feeder"], tuple(pairs[8]), c["hub_next"]], np.int32)
    n_neg, seed, draw, cap, attempts = 6, 7, 2, 7, 4
    prs = training_pairs(eng, gr, s, pos, n_neg, seed, draw, attempts)
    labels = np.zeros(len(prs), np.float32)
    labels[::1 + n_neg] = 1
    # a row of item 0 counts 0 paths and keeps its place in the list (the cap's draws are addressed by row): (u, u) is such a row that the two-call form accepts
    stand_in = np.where(prs[:, 1:] == 0, prs[:, :1], prs[:, 1:])
    want_b, wc, wf = eng.find_paths(gr, np.concatenate([prs[:, :1], stand_in], axis=1), 1, max_hops, cap, wr.T, labels=labels, walks=walks, seed=seed, draw=draw)
    got_b, got_prs, gc, gf = eng.find_training_paths(gr, s, pos, n_neg, seed, draw, 1, max_hops, cap, wr.T, max_attempts=attempts, walks=walks)
    assert np.array_equal(got_prs, prs) and np.array_equal(gc, wc) and np.array_equal(gf, wf)
    assert (wf > cap).sum() >= 2
    assert got_b.has_labels and np.array_equal(got_b.counts, want_b.counts) and np.array_equal(got_b.read_idx(), want_b.read_idx())
    got_b.free(); want_b.free(); s.free()


@pytest.mark.parametrize("max_hops,walks", [(3, 0), (5, 64)])
def test_candidates_call_equals_find_on_the_list(inputs, engine, spread, max_hops, walks):
    g, pairs = inputs
    eng, gr = engine
    s = eng.sampler(np.arange(1, 381, dtype=np.int32))
    users = np.array([pairs[7][0], pairs[8][0], pairs[0][0]], np.int32)
    listed, gc = eng.find_candidates(gr, s, users, 1, 3)
    assert len(listed) > 3
    got_b, c, f = eng.find_paths_of_candidates(gr, len(listed), 1, max_hops, 7, wr.T, walks=walks, seed=5, draw=3)
    want_b, wc, wf = eng.find_paths(gr, listed, 1, max_hops, 7, wr.T, walks=walks, seed=5, draw=3)
    assert np.array_equal(c, wc) and np.array_equal(f, wf) and (f > 7).sum() >= 2
    assert np.array_equal(got_b.counts, want_b.counts) and np.array_equal(got_b.read_idx(), want_b.read_idx())
    got_b.free(); want_b.free(); s.free()


def test_back_at_first_the_calls_return_what_they_returned_before(inputs, engine, before, twin):
    eng, gr = engine
    pairs = inputs[1]
    eng.set_option("path_cap", "spread")
    b, _, _ = eng.find_paths(gr, pairs, 1, 3, 28, wr.T, walks=0, seed=1, draw=0)
    assert not np.array_equal(b.read_idx(), before["seeded3"][0])
    b.free()
    eng.set_option("path_cap", "first")
    assert eng.options["path_cap"] == "first"
    for key, hi, walks in (("seeded3", 3, 0), ("sampled", 5, wr.WALKS)):
        b, c, f = eng.find_paths(gr, pairs, 1, hi, 28, wr.T, walks=walks, seed=wr.SEED, draw=wr.DRAW)
        for got, want in zip((b.read_idx(), c, f), before[key]):
            assert np.array_equal(got, want), key
        b.free()
        assert all(np.array_equal(a, w) for a, w in zip(before[key], twin(pairs, 1, hi, 28, wr.T, walks, mode="first"))), key
    with pytest.raises(_ffi.KprnError) as ei:
        eng.set_option("path_cap", "bogus")
    assert ei.value.code == _ffi.E_ARG and eng.options["path_cap"] == "first"


def test_found_batch_scores_and_trains_like_the_uploaded_ids(inputs, engine, twin, spread):
    eng, gr = engine
    pairs = inputs[1]
    idx, counts, _ = twin(pairs, 1, 5, 28, wr.T, wr.WALKS)
    kept = counts > 0
    labels = (np.arange(len(pairs)) % 2).astype(np.float32)
    found_batch, _, _ = eng.find_paths(gr, pairs, 1, 5, 28, wr.T, labels=labels, walks=wr.WALKS, seed=wr.SEED, draw=wr.DRAW)
    up_batch = eng.batch_ragged(idx, counts[kept], labels[kept])
    a = eng.forward(found_batch, 1)["probs"]
    b = eng.forward(up_batch, 1)["probs"]
    assert a.shape == (int(kept.sum()),) and np.isfinite(a).all() and np.array_equal(a, b)
    theta = eng.get_flat_params()
    opt = _ffi.make_opt(method=1, lr=1e-3)
    la = eng.train_step(found_batch, opt)
    eng.set_flat_params(theta)
    lb = eng.train_step(up_batch, opt)
    eng.set_flat_params(theta)
    assert np.isfinite(la) and la > 0 and la == lb
    found_batch.free(); up_batch.free()


def test_recommend_with_a_spread_of_paths(inputs, engine, before, twin):
    g, pairs = inputs
    eng, gr = engine
    u = int(pairs[7][0])
    items = np.array([pairs[7][1], g["cases"]["lonely"][0], u], np.int32)
    res = kgraph.recommend(eng, gr, u, items, 2, 3, max_paths=28, cap="spread")
    assert eng.options["path_cap"] == "first"                              # put back
    mine = [r for r in res if r["item"] == int(pairs[7][1])]
    assert len(mine) == 1 and mine[0]["found"] == 689 and mine[0]["n_paths"] == 28
    rows = twin(np.stack([np.full(3, u, np.int32), items], axis=1), 1, 3, 28, 4, 0, seed=1, draw=0)[0]
    assert mine[0]["paths"] and all(any(np.array_equal(ids, row) for row in rows) for ids, _, _ in mine[0]["paths"])
    again = kgraph.recommend(eng, gr, u, items, 2, 3, max_paths=28, cap="spread")
    assert [(r["item"], r["score"]) for r in again] == [(r["item"], r["score"]) for r in res]      # draw 0: the same answer every time


def test_train_from_graph_draws_another_subset_every_epoch(inputs, engine, before):
    """one positive -- row 7's pair, 689 paths of 1..3 hops -- in minibatches of one: step k of the run is draw k, row 0 of its pair list is the positive.
    Two epochs see two subsets of its paths; the same seed and step see the same one."""
    g, pairs = inputs
    eng, gr = engine
    pos = np.array([tuple(pairs[7])], np.int32)
    s = eng.sampler(np.arange(1, 381, dtype=np.int32))
    theta = eng.get_flat_params()
    inner = eng.find_training_paths

    def run(epochs):
        seen = []

        def spy(*a, **kw):
            out = inner(*a, **kw)
            assert out[2][0] == 28 and out[3][0] == 689
            seen.append(out[0].read_idx()[:28].copy())
            return out
        eng.find_training_paths = spy
        try:
            hist = kgraph.train_from_graph(eng, gr, pos, _ffi.make_opt(method=1, lr=1e-3), 1, 2, epochs, 5, sampler=s, min_hops=1, max_hops=3, max_paths=28,
                                           out=io.StringIO(), cap="spread")
        finally:
            del eng.find_training_paths
            eng.set_flat_params(theta)
        assert len(hist) == epochs and np.isfinite(hist).all() and eng.options["path_cap"] == "first"
        return seen
    two = run(2)
    assert len(two) == 2 and not np.array_equal(two[0], two[1])
    assert np.array_equal(run(1)[0], two[0])                               # seed and step repeated
    want = _ffi.host_find_paths_cap(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.VR, ref.VT, ref.END_REL, pos, 1, 3, 28, 4, 0, 5, 1, cap="spread")[0]
    assert np.array_equal(two[1], want)                                    # step 1 = draw 1, row 0
    s.free()
