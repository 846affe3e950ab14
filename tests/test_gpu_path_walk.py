"""gpu: kprn_find_paths_sampled / kprn_find_training_paths_sampled against the host twin kprn_host_find_paths_sampled (itself held to a brute-force
restatement by tests/test_path_walk_host.py), and the found batch through scoring, training and the recommend chain.  Every comparison is np.array_equal."""
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
def engines(inputs, nt):
    g = inputs[0]
    made = {}

    def get(F):
        if F not in made:
            eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, **SHAPES[F])
            made[F] = (eng, eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL))
        return made[F]
    yield get
    for eng, _ in made.values():
        eng.close()


@pytest.fixture(scope="module")
def twin(inputs, nt):
    """the host twin's (idx, counts, found), computed once per argument set and left unchanged"""
    g = inputs[0]
    memo = {}

    def get(pairs, lo, hi, cap, T, F, walks, seed=wr.SEED, draw=wr.DRAW):
        key = (pairs.tobytes(), lo, hi, cap, T, F, walks, seed, draw)
        if key not in memo:
            memo[key] = _ffi.host_find_paths_sampled(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, T, walks, seed, draw, F=F,
                                                     threads=8)
            for a in memo[key]:
                a.setflags(write=False)
        return memo[key]
    return get


def same_as_twin(eng, gr, twin, pairs, lo, hi, cap, T, F, walks, seed=wr.SEED, draw=wr.DRAW):
    idx, counts, found = twin(pairs, lo, hi, cap, T, F, walks, seed, draw)
    batch, c, f = eng.find_paths(gr, pairs, lo, hi, cap, T, walks=walks, seed=seed, draw=draw)
    what = (lo, hi, cap, walks)
    assert np.array_equal(c, counts) and np.array_equal(f, found), what
    assert batch is not None and batch.B == int((counts > 0).sum()) and batch.n_paths == idx.shape[0], what
    assert np.array_equal(batch.counts, counts[counts > 0]) and np.array_equal(batch.read_idx(), idx), what
    batch.free()
    return counts, found


@pytest.mark.parametrize("walks", [64, 256])
@pytest.mark.parametrize("max_paths", [7, 28])
@pytest.mark.parametrize("hops", [(1, 5), (4, 5)])
def test_device_equals_twin(inputs, engines, twin, hops, max_paths, walks):
    eng, gr = engines(3)
    _, found = same_as_twin(eng, gr, twin, inputs[1], hops[0], hops[1], max_paths, wr.T, 3, walks)
    assert (found > max_paths).sum() >= 3 and (found == 0).any()


def test_device_equals_twin_uncapped_single_hop_counts_and_the_other_layout(inputs, engines, twin):
    """every chunk of the hub's closing adjacency (row 70: 300 edges) is written; 4 and 5 hops alone; one pair; F = 4 with a leading column, T = 7"""
    pairs = inputs[1]
    eng, gr = engines(3)
    _, found = same_as_twin(eng, gr, twin, pairs, 4, 5, 4096, wr.T, 3, wr.WALKS)
    assert found[70] > 64
    same_as_twin(eng, gr, twin, pairs, 4, 4, 28, 5, 3, wr.WALKS)
    same_as_twin(eng, gr, twin, pairs, 5, 5, 28, wr.T, 3, 3)
    same_as_twin(eng, gr, twin, pairs[70:], 2, 5, 4096, wr.T, 3, 1)
    same_as_twin(eng, gr, twin, pairs, 1, 5, 28, wr.T, 3, wr.WALKS, seed=0xDEADBEEF12345678, draw=9)
    eng4, gr4 = engines(4)
    same_as_twin(eng4, gr4, twin, pairs, 1, 5, 28, 7, 4, wr.WALKS)


def test_three_hops_or_fewer_is_find_paths(inputs, engines):
    eng, gr = engines(3)
    pairs = inputs[1]
    for lo, hi, cap in ((1, 3, 7), (2, 3, 4096)):
        want_b, wc, wf = eng.find_paths(gr, pairs, lo, hi, cap, wr.T)
        got_b, gc, gf = eng.find_paths(gr, pairs, lo, hi, cap, wr.T, walks=64, seed=5, draw=3)
        assert np.array_equal(gc, wc) and np.array_equal(gf, wf) and np.array_equal(got_b.read_idx(), want_b.read_idx())
        want_b.free(); got_b.free()


def test_same_result_twice(inputs, engines):
    eng, gr = engines(3)
    runs = []
    for _ in range(2):
        batch, c, f = eng.find_paths(gr, inputs[1], 1, 5, 28, wr.T, walks=wr.WALKS, seed=wr.SEED, draw=wr.DRAW)
        runs.append((batch.read_idx(), c, f))
        batch.free()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_found_batch_scores_and_trains_like_the_uploaded_ids(inputs, engines, twin):
    """SHAPES[3] (D = H = 64, L = 2, F = 3) at T = 6: the fused path"""
    eng, gr = engines(3)
    pairs = inputs[1]
    idx, counts, _ = twin(pairs, 1, 5, 28, wr.T, 3, wr.WALKS)
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


@pytest.mark.parametrize("max_hops,walks", [(5, 64), (4, 256), (3, 64)])
def test_training_call_equals_sample_then_find(inputs, engines, max_hops, walks):
    g, pairs = inputs
    eng, gr = engines(3)
    c = g["cases"]
    s = eng.sampler(np.arange(1, 300, dtype=np.int32))                  # every candidate is the hub's neighbour: the hub's slots stay empty
    pos = np.array([c["exact"], c["hub_user"], tuple(pairs[17]), c["feeder"], tuple(pairs[20]), c["hub_next"]], np.int32)
    n_neg, seed, draw, cap, attempts = 6, 7, 2, 28, 4
    neg, _ = eng.sample_negatives(gr, s, pos[:, 0], n_neg, seed, draw, max_attempts=attempts)
    prs = np.zeros((len(pos), 1 + n_neg, 2), np.int32)
    prs[:, :, 0] = pos[:, :1]
    prs[:, 0, 1] = pos[:, 1]
    prs[:, 1:, 1] = neg
    prs = prs.reshape(-1, 2)
    assert (prs[:, 1] == 0).any() and (prs[:, 1] != 0).sum() > len(pos)
    labels = np.zeros(len(prs), np.float32)
    labels[::1 + n_neg] = 1
    # a row of item 0 counts 0 paths and keeps its place in the list (the walks are addressed by row): (u, u) is such a row that the two-call form accepts
    stand_in = np.where(prs[:, 1:] == 0, prs[:, :1], prs[:, 1:])
    want_b, wc, wf = eng.find_paths(gr, np.concatenate([prs[:, :1], stand_in], axis=1), 2, max_hops, cap, wr.T, labels=labels, walks=walks, seed=seed, draw=draw)
    got_b, got_prs, gc, gf = eng.find_training_paths(gr, s, pos, n_neg, seed, draw, 2, max_hops, cap, wr.T, max_attempts=attempts, walks=walks)
    assert np.array_equal(got_prs, prs) and np.array_equal(gc, wc) and np.array_equal(gf, wf)
    assert (wc[prs[:, 1] == 0] == 0).all() and wc[0] > 0 and (wc[labels == 0] > 0).any()
    assert got_b.has_labels and np.array_equal(got_b.counts, want_b.counts) and np.array_equal(got_b.read_idx(), want_b.read_idx())
    if max_hops > 3:
        hops = (got_b.read_idx()[:, :, 1] != g["Ve"]).sum(axis=1) - 1
        assert hops.max() == max_hops
    la, lb = eng.backward(got_b, 1), eng.backward(want_b, 1)            # the labels ride in the batch: the loss is a function of them
    assert np.isfinite(la) and la == lb
    got_b.free(); want_b.free(); s.free()


def test_recommend_explains_with_paths_of_more_than_four_steps(inputs, engines):
    g, pairs = inputs
    eng, gr = engines(3)
    # from the brute force: a pair without any path of 1..3 hops whose walks (row 0 of a recommend call's list) find some
    for u, i in pairs[:70].tolist():
        if not ref.brute_paths(g, u, i, 1, 3) and len(wr.pair_paths(g, u, i, 0, 4, 5, wr.WALKS, 1, 0)) > 0:
            break
    else:
        raise AssertionError("no pair of the inputs has only sampled paths")
    want = wr.pair_paths(g, u, i, 0, 1, 5, wr.WALKS, 1, 0)
    items = np.array([i, g["cases"]["lonely"][0], u], np.int32)
    res = kgraph.recommend(eng, gr, u, items, 2, 3, max_hops=5, walks=wr.WALKS, max_paths=28)
    mine = [r for r in res if r["item"] == i]
    assert len(mine) == 1 and mine[0]["found"] == len(want) and mine[0]["n_paths"] == min(len(want), 28)
    steps = [int((ids[:, 1] != g["Ve"]).sum()) for ids, _, _ in mine[0]["paths"]]
    assert steps and max(steps) > 4 and all(ids.shape == (6, 3) for ids, _, _ in mine[0]["paths"])
    rows = ref.rows_of(want[:28], ref.node_types(g, 1), g["Ve"], 6, 3)
    assert all(any(np.array_equal(ids, row) for row in rows) for ids, _, _ in mine[0]["paths"])
    # without walks the same call is refused, and three hops find nothing for this pair
    with pytest.raises(_ffi.KprnError) as ei:
        kgraph.recommend(eng, gr, u, items, 2, 3, max_hops=5, max_paths=28)
    assert ei.value.code == _ffi.E_ARG
    assert [r for r in kgraph.recommend(eng, gr, u, items, 2, 3, max_paths=28) if r["item"] == i] == []


def test_sampled_finder_does_not_depend_on_what_hipmalloc_returns(inputs, twin):
    """one sampled case in a fresh process with KPRN_POISON_ALLOC=1 (every new device allocation filled with 0xFF bytes), twice"""
    import json
    import os
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r)
        import numpy as np
        from kprn_amd import _ffi
        from tests import path_find_ref as ref, path_walk_ref as wr
        g, pairs = wr.make_inputs()
        eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, 16, 32, 16, 64, 2)
        gr = eng.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL)
        out = []
        for _ in range(2):
            b, c, f = eng.find_paths(gr, pairs, 1, 5, 28, wr.T, walks=wr.WALKS, seed=wr.SEED, draw=wr.DRAW)
            out.append([b.read_idx().ravel().tolist(), c.tolist(), f.tolist(), bool(np.isfinite(eng.forward(b, 1)["probs"]).all())])
            b.free()
        eng.close()
        print(json.dumps(out))
    """) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    idx, counts, found = twin(inputs[1], 1, 5, 28, wr.T, 3, wr.WALKS)
    for rows, c, f, finite in json.loads(r.stdout.strip().splitlines()[-1]):
        assert np.array_equal(np.array(rows, np.int32), idx.ravel()) and np.array_equal(c, counts) and np.array_equal(f, found) and finite


def test_train_from_graph_with_walks(inputs, engines):
    """graph.train_from_graph(max_hops=5, walks=64): every step's batch comes from the sampled training call, and some hold six-step paths"""
    import io
    g, pairs = inputs
    eng, gr = engines(3)
    c = g["cases"]
    pos = np.array([c["exact"], tuple(pairs[17]), c["feeder"], tuple(pairs[20]), c["hub_next"], c["inside"], tuple(pairs[30])], np.int32)
    s = eng.sampler(np.arange(1, 381, dtype=np.int32))
    theta = eng.get_flat_params()
    steps, calls = [], []
    inner = eng.find_training_paths

    def spy(*a, **kw):
        out = inner(*a, **kw)
        calls.append(kw.get("walks"))
        if out[0] is not None:
            steps.append(int((out[0].read_idx()[:, :, 1] != g["Ve"]).sum(axis=1).max()))
        return out
    eng.find_training_paths = spy
    st = {}
    try:
        hist = kgraph.train_from_graph(eng, gr, pos, _ffi.make_opt(method=1, lr=1e-3), 3, 2, 2, 5, sampler=s, min_hops=2, max_hops=5, max_paths=28, walks=wr.WALKS,
                                       out=io.StringIO(), stats=st)
    finally:
        del eng.find_training_paths
        eng.set_flat_params(theta)
        s.free()
    assert len(hist) == 2 and np.isfinite(hist).all() and st["steps"] == len(steps) >= 4
    assert calls == [wr.WALKS] * 6 and max(steps) == 6


def test_refusals_through_the_handle(inputs, engines):
    g, pairs = inputs
    eng, gr = engines(3)
    s = eng.sampler(np.arange(1, 381, dtype=np.int32))
    ok = dict(min_hops=1, max_hops=5, max_paths=7, T=6, walks=64, seed=1, draw=0)
    batch, _, _ = eng.find_paths(gr, pairs[:4], **ok)
    if batch is not None:
        batch.free()
    for kw in (dict(max_hops=6, T=7), dict(walks=257), dict(walks=-1), dict(max_hops=4, walks=0), dict(T=5), dict(max_hops=4, T=4), dict(min_hops=0),
               dict(max_paths=4097)):
        a = dict(ok, **kw)
        with pytest.raises(_ffi.KprnError) as ei:
            eng.find_paths(gr, pairs[:4], **a)
        assert ei.value.code == _ffi.E_ARG, kw
        with pytest.raises(_ffi.KprnError) as ei:
            eng.find_training_paths(gr, s, pairs[:2], 4, a["seed"], a["draw"], a["min_hops"], a["max_hops"], a["max_paths"], a["T"], walks=a["walks"])
        assert ei.value.code == _ffi.E_ARG, kw
    with pytest.raises(_ffi.KprnError) as ei:
        eng.find_paths(gr, np.array([[1, g["Ve"]]], np.int32), **ok)
    assert ei.value.code == _ffi.E_INDEX
    s.free()
