"""gpu: kprn_graph_create / kprn_find_paths / kprn_batch_read_idx against the host twin kprn_host_find_paths (itself held to a brute-force search by
tests/test_path_find_host.py), and the found batch through scoring, training and the recommend chain.  Every comparison is np.array_equal."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph

from . import path_find_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {3: dict(dt=16, de=32, dr=16, H=64, L=2, F=3),              # the fused D = H = 64 path
          4: dict(dt=8, de=16, dr=8, H=40, L=1, F=4, rnn_type=1)}    # a generic shape (rnn cell), one leading column nothing reads


@pytest.fixture(scope="module")
def g():
    return ref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)     # about 400 nodes


@pytest.fixture(scope="module")
def nt(g):
    return ref.node_types(g, 1)


@pytest.fixture(scope="module")
def pairs(g):
    pr = ref.pairs_of(g, 60, seed=29)
    assert len(pr) == 70
    return pr


@pytest.fixture(scope="module")
def engines(g, nt):
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
def twin(g, nt):
    """the host twin's (idx, counts, found), computed once per argument set and left unchanged"""
    memo = {}

    def get(pairs, lo, hi, cap, T, F):
        key = (pairs.tobytes(), lo, hi, cap, T, F)
        if key not in memo:
            memo[key] = _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, T, F=F, threads=8)
            for a in memo[key]:
                a.setflags(write=False)
        return memo[key]
    return get


def test_inputs_hold_the_hub_cases(g, pairs, twin):
    c = g["cases"]
    stored = {(int(s), int(d), int(r)) for s, d, r in zip(g["src"], g["dst"], g["rel"]) if s != d}
    assert len({d for s, d, r in stored if s == c["hub"]}) == 300                     # more than a workgroup's 256 threads
    assert c["hub_user"][0] == c["hub"] and (c["hub_next"][0], c["hub"]) in {(s, d) for s, d, r in stored}
    want = {tuple(v) for v in c.values() if isinstance(v, tuple)}
    assert want <= {tuple(p) for p in pairs.tolist()}
    _, counts, found = twin(pairs, 1, 3, 5, 4, 3)
    by = {tuple(p): (int(counts[k]), int(found[k])) for k, p in enumerate(pairs.tolist())}
    assert by[c["hub_user"]][1] > 5 and by[c["hub_next"]][1] > 5                     # the hub as u and as u's neighbour both lead somewhere
    assert by[c["lonely"]] == (0, 0) and by[c["same"]] == (0, 0) and by[c["direct"]] == (1, 1) and by[c["exact"]][1] == ref.MAX_PATHS


@pytest.mark.parametrize("F", [3, 4])
@pytest.mark.parametrize("max_paths", [5, 4096])
@pytest.mark.parametrize("B", [1, 70])
def test_device_equals_twin(g, pairs, engines, twin, B, max_paths, F):
    eng, gr = engines(F)
    assert gr.n_edges == len({(int(s), int(d), int(r)) for s, d, r in zip(g["src"], g["dst"], g["rel"]) if s != d})
    pr = pairs if B == 70 else np.array([g["cases"]["hub_user"]], np.int32)
    for lo, hi, T in ((1, 3, 4), (2, 3, 6), (1, 1, 2)) if B == 70 else ((1, 3, 4),):
        idx, counts, found = twin(pr, lo, hi, max_paths, T, F)
        batch, c, f = eng.find_paths(gr, pr, lo, hi, max_paths, T)
        assert np.array_equal(c, counts) and np.array_equal(f, found), (lo, hi)
        assert batch is not None and batch.B == int((counts > 0).sum()) and batch.n_paths == idx.shape[0]
        assert np.array_equal(batch.counts, counts[counts > 0])
        assert np.array_equal(batch.read_idx(), idx), (lo, hi)
        batch.free()


def test_same_result_twice(g, pairs, engines):
    eng, gr = engines(3)
    runs = []
    for _ in range(2):
        batch, c, f = eng.find_paths(gr, pairs, 1, 3, 7, 5)
        runs.append((batch.read_idx(), c, f))
        batch.free()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_no_pair_has_a_path(g, engines):
    eng, gr = engines(3)
    c = g["cases"]
    batch, counts, found = eng.find_paths(gr, np.array([c["lonely"], c["same"], c["direct"]], np.int32), 2, 3, 5, 4)
    assert batch is None and counts.tolist() == [0, 0, 0] and found.tolist() == [0, 0, 0]


@pytest.mark.parametrize("F", [3, 4])
def test_found_batch_scores_like_the_twins_batch(pairs, engines, twin, F):
    eng, gr = engines(F)
    idx, counts, _ = twin(pairs, 1, 3, 28, 4, F)
    found_batch, _, _ = eng.find_paths(gr, pairs, 1, 3, 28, 4)
    twin_batch = eng.batch_ragged(idx, counts[counts > 0])
    a = eng.forward(found_batch, 1)["probs"]
    b = eng.forward(twin_batch, 1)["probs"]
    assert a.shape == (int((counts > 0).sum()),) and np.isfinite(a).all() and np.array_equal(a, b)
    found_batch.free(); twin_batch.free()


def test_one_training_step_on_a_found_batch(pairs, engines):
    eng, gr = engines(3)
    labels = (np.arange(len(pairs)) % 2).astype(np.float32)
    theta = eng.get_flat_params()
    batch, counts, _ = eng.find_paths(gr, pairs, 1, 3, 28, 4, labels=labels)
    assert batch.has_labels
    loss = eng.train_step(batch, _ffi.make_opt(method=1, lr=1e-3))
    assert np.isfinite(loss) and loss > 0
    batch.free()
    eng.set_flat_params(theta)


def test_recommend_chain_equals_the_chain_fed_from_the_twin(g, engines, twin):
    eng, gr = engines(3)
    c = g["cases"]
    user = c["hub"]
    items = np.array([c["hub_user"][1], c["exact"][1], c["inside"][1], c["lonely"][0], 5, 9, 17, c["exact"][0]], np.int32)
    K, M, cap, T = 4, 3, 28, 4
    got = kgraph.recommend(eng, gr, user, items, K, M, max_paths=cap, T=T)
    pr = np.stack([np.full(items.shape, user, np.int32), items], axis=1)
    idx, counts, found = twin(pr, 1, 3, cap, T, 3)
    cand = np.nonzero(counts)[0]
    assert len(cand) >= K and len(cand) < len(items)
    cnz = counts[cand]
    res = eng.recommend_explain_ragged(idx, cnz, np.array([len(cand)], np.int32), K, M)
    off = np.concatenate([[0], np.cumsum(cnz)])
    assert len(got) == K
    for place, r in enumerate(got):
        b = int(res["topk_idx"][0, place])
        assert r["rank"] == place and r["item"] == int(items[cand[b]]) and r["n_paths"] == int(cnz[b]) and r["found"] == int(found[cand[b]])
        assert np.float32(r["score"]) == res["topk_score"][0, place]
        want = [q for q in res["path_idx"][0, place] if q >= 0]
        assert len(r["paths"]) == len(want) == min(M, int(cnz[b]))
        for (ids, w, s), q, ww in zip(r["paths"], want, res["path_weight"][0, place]):
            assert np.array_equal(ids, idx[off[b] + q]) and np.float32(w) == ww
    # a user with no path to any item: an empty result, no error
    assert kgraph.recommend(eng, gr, c["lonely"][0], items, K, M, max_paths=cap, T=T) == []


def test_graph_refusals_leave_nothing_behind(g, nt, engines):
    eng, gr = engines(3)
    bad = g["dst"].copy()
    bad[7] = g["Ve"]
    with pytest.raises(_ffi.KprnError) as ei:
        eng.graph(g["src"], bad, g["rel"], nt, ref.END_REL)
    assert ei.value.code == _ffi.E_INDEX
    for kw, code in ((dict(max_hops=4, T=5), _ffi.E_ARG), (dict(T=3), _ffi.E_ARG), (dict(max_paths=0), _ffi.E_ARG), (dict(max_paths=4097), _ffi.E_ARG),
                     (dict(pairs=np.array([[1, g["Ve"]]], np.int32)), _ffi.E_INDEX)):
        a = dict(pairs=np.array([[1, 2]], np.int32), min_hops=1, max_hops=3, max_paths=5, T=4)
        a.update(kw)
        with pytest.raises(_ffi.KprnError) as ei:
            eng.find_paths(gr, **a)
        assert ei.value.code == code, kw


def test_finder_does_not_depend_on_what_hipmalloc_returns(g, nt, pairs, twin):
    """one finder case in a fresh process with KPRN_POISON_ALLOC=1 (every new device allocation filled with 0xFF bytes), twice"""
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r)
        import numpy as np
        from kprn_amd import _ffi
        from tests import path_find_ref as ref
        g = ref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)
        nt = ref.node_types(g, 1)
        pairs = ref.pairs_of(g, 60, seed=29)
        eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, 16, 32, 16, 64, 2)
        gr = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
        out = []
        for _ in range(2):
            b, c, f = eng.find_paths(gr, pairs, 1, 3, 7, 5)
            out.append([b.read_idx().ravel().tolist(), c.tolist(), f.tolist(), bool(np.isfinite(eng.forward(b, 1)["probs"]).all())])
            b.free()
        eng.close()
        print(json.dumps(out))
    """) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    idx, counts, found = twin(pairs, 1, 3, 7, 5, 3)
    for rows, c, f, finite in json.loads(r.stdout.strip().splitlines()[-1]):
        assert np.array_equal(np.array(rows, np.int32), idx.ravel()) and np.array_equal(c, counts) and np.array_equal(f, found) and finite


def test_recommend_command_line(tmp_path):
    """python -m kprn_amd.recommend (called in-process) prints what graph.recommend returns for the same checkpoint, graph, user and items"""
    import io
    from kprn_amd import recommend as cli
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
    names = ["m0", "m1", "m2", "m3", "m4", "g0"]                                   # g0 has no edge here: no path, not a candidate
    (tmp_path / "items.txt").write_text("\n".join(names) + "\n")
    kg = kgraph.KnowledgeGraph.from_triples(triples, Vocabs(str(vdir)), 1)
    eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, 16, 32, 16, 64, 2)
    try:
        eng.save(str(tmp_path / "model"))
        want = kgraph.recommend(eng, kg, kg.entity_id("u0"), [kg.entity_id(n) for n in names], 3, 2)
    finally:
        eng.close()
    assert len(want) == 3 and all(len(r["paths"]) >= 1 for r in want)
    buf = io.StringIO()
    flags = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1, "-gpu_id", 0, "-top_k", 2, "-model_path", tmp_path / "model", "-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-user", "u0",
             "-items", tmp_path / "items.txt", "-k", 3, "-explain_paths", 2]
    assert cli.main([str(f) for f in flags], out=buf) == 0
    lines = [l.split("\t") for l in buf.getvalue().splitlines()]
    heads = [l for l in lines if l[1] in names]
    assert [(int(l[0]), l[1], l[2], int(l[3]), int(l[4])) for l in heads] == \
        [(r["rank"], kg.entity_name(r["item"]), "%.5f" % r["score"], r["n_paths"], r["found"]) for r in want]
    assert len(lines) - len(heads) == sum(len(r["paths"]) for r in want)
