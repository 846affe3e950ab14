"""gpu: kprn_sampler_create / kprn_sample_negatives / kprn_find_training_paths against the host twin kprn_host_sample_negatives (itself held to a brute-force
restatement by tests/test_neg_sample_host.py) and against the two-call composition sample -> find, then training from the graph alone: the loop of
graph.train_from_graph against the hand-written composition, and python -m kprn_amd.train -kg.  Every comparison of ids is np.array_equal."""
import io
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph

from . import neg_sample_ref as nref
from . import path_find_ref as ref
from .test_gpu_path_find import SHAPES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return ref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)


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


def twin(g, cfg, **kw):
    a = dict(cfg, **kw)
    return _ffi.host_sample_negatives(g["src"], g["dst"], g["rel"], g["Ve"], a["items"], a["weights"], a["users"], a["n_neg"], a["seed"], a["draw"],
                                      max_attempts=a["max_attempts"], threads=8)


def device(eng, gr, cfg, sampler=None, **kw):
    a = dict(cfg, **kw)
    s = sampler or eng.sampler(a["items"], a["weights"])
    try:
        return eng.sample_negatives(gr, s, a["users"], a["n_neg"], a["seed"], a["draw"], max_attempts=a["max_attempts"])
    finally:
        if sampler is None:
            s.free()


@pytest.mark.parametrize("config", [nref.config_one, nref.config_two])
def test_device_equals_twin_on_the_two_configurations(g, engines, config):
    eng, gr = engines(3)
    cfg = config(g)
    want, got = twin(g, cfg), device(eng, gr, cfg)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (want[1] < cfg["n_neg"]).any() and (want[1] > 0).all()                      # empty slots and filled ones


@pytest.mark.parametrize("B", [1, 5, 70])
def test_device_equals_twin_over_slots_attempts_and_negatives(g, pairs, engines, B):
    """one wave, a partial workgroup, several workgroups; one attempt per lane group of 64, 16 and 1 negatives; an accepted list of up to 256 entries"""
    eng, gr = engines(4)
    cfg = dict(nref.config_one(g), users=pairs[:B, 0].copy(), seed=(3 << 32) | 11, draw=5)
    s = eng.sampler(cfg["items"], cfg["weights"])
    for max_attempts in (1, 4, 64):
        for n_neg in (1, 8, 256):
            want = twin(g, cfg, n_neg=n_neg, max_attempts=max_attempts)
            got = device(eng, gr, cfg, sampler=s, n_neg=n_neg, max_attempts=max_attempts)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (max_attempts, n_neg)
            if n_neg == 256 and max_attempts == 1 and B == 70:
                assert (want[0][:, 200:] == 0).mean() > 0.5                               # late slots mostly fail against a long list
    # a candidate list with a remainder (64 % max_attempts != 0) and uniform weights
    want = twin(g, cfg, weights=None, n_neg=9, max_attempts=24)
    got = device(eng, gr, cfg, weights=None, n_neg=9, max_attempts=24)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    s.free()


def test_same_result_twice(g, engines):
    eng, gr = engines(3)
    cfg = nref.config_one(g)
    a, b = device(eng, gr, cfg), device(eng, gr, cfg)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_refusals_write_nothing(g, engines):
    eng, gr = engines(3)
    cfg = nref.config_one(g)
    s = eng.sampler(cfg["items"], cfg["weights"])
    for kw, code in ((dict(users=np.array([5, 0], np.int32)), _ffi.E_INDEX), (dict(users=np.array([g["Ve"]], np.int32)), _ffi.E_INDEX), (dict(n_neg=0), _ffi.E_ARG),
                     (dict(n_neg=257), _ffi.E_ARG), (dict(max_attempts=0), _ffi.E_ARG), (dict(max_attempts=65), _ffi.E_ARG)):
        a = dict(cfg, **kw)
        neg, nf = np.full((len(a["users"]), 8), -7, np.int32), np.full(len(a["users"]), -7, np.int32)
        with pytest.raises(_ffi.KprnError) as ei:
            eng.sample_negatives(gr, s, a["users"], a["n_neg"], 7, 0, max_attempts=a["max_attempts"], out=(neg, nf))
        assert ei.value.code == code and (neg == -7).all() and (nf == -7).all(), kw
    with pytest.raises(_ffi.KprnError) as ei:
        eng.find_training_paths(gr, s, np.array([[5, g["Ve"]]], np.int32), 4, 7, 0, 2, 3, 28, 4)
    assert ei.value.code == _ffi.E_INDEX
    with pytest.raises(_ffi.KprnError) as ei:
        eng.find_training_paths(gr, s, np.array([[5, 6]], np.int32), 4, 7, 0, 2, 4, 28, 5)
    assert ei.value.code == _ffi.E_ARG
    s.free()
    for items, weights, code in (([3, 2], None, _ffi.E_ARG), ([2, 3], [0, 0], _ffi.E_ARG), ([2, 3], [1, -1], _ffi.E_ARG), ([2, g["Ve"]], None, _ffi.E_INDEX)):
        with pytest.raises(_ffi.KprnError) as ei:
            eng.sampler(items, weights)
        assert ei.value.code == code, (items, weights)


def positives_of(g):
    c = g["cases"]
    return np.array([c["exact"], c["inside"], c["direct"], c["hub_user"], (5, 9), (17, 40), c["hub_next"]], np.int32)


def composition(eng, gr, s, pos, n_neg, max_attempts, seed, draw, min_hops, max_hops, max_paths, T):
    """kprn_sample_negatives, the pair list and labels formed here, kprn_find_paths over the rows that have an item ->
    (batch or None, pairs [B (1 + n_neg), 2], counts, found)"""
    neg, _ = eng.sample_negatives(gr, s, pos[:, 0], n_neg, seed, draw, max_attempts=max_attempts)
    B = len(pos)
    prs = np.zeros((B, 1 + n_neg, 2), np.int32)
    prs[:, :, 0] = pos[:, :1]
    prs[:, 0, 1] = pos[:, 1]
    prs[:, 1:, 1] = neg
    prs = prs.reshape(-1, 2)
    labels = np.zeros(len(prs), np.float32)
    labels[::1 + n_neg] = 1
    real = prs[:, 1] != 0
    batch, c, f = eng.find_paths(gr, prs[real], min_hops, max_hops, max_paths, T, labels=labels[real])
    counts, found = np.zeros(len(prs), np.int32), np.zeros(len(prs), np.int64)
    counts[real], found[real] = c, f
    return batch, prs, counts, found, labels


@pytest.mark.parametrize("F", [3, 4])
@pytest.mark.parametrize("max_paths", [7, 28])
@pytest.mark.parametrize("min_hops", [1, 2])
def test_fused_call_equals_sample_then_find(g, engines, F, max_paths, min_hops):
    eng, gr = engines(F)
    cfg = nref.config_one(g)
    s = eng.sampler(cfg["items"], cfg["weights"])
    pos = positives_of(g)
    n_neg, T = 8, 4
    want_b, prs, counts, found, labels = composition(eng, gr, s, pos, n_neg, 4, 7, 2, min_hops, 3, max_paths, T)
    assert (prs[:, 1] == 0).any()                                                        # the hub's empty slots: rows of 0 paths, not an error
    got_b, got_prs, got_counts, got_found = eng.find_training_paths(gr, s, pos, n_neg, 7, 2, min_hops, 3, max_paths, T, max_attempts=4)
    assert np.array_equal(got_prs, prs) and np.array_equal(got_counts, counts) and np.array_equal(got_found, found)
    direct = 2 * (1 + n_neg)
    assert tuple(prs[direct]) == g["cases"]["direct"] and counts[direct] == (1 if min_hops == 1 else 0)   # only the direct edge: gone with min_hops = 2
    assert counts[0] > 0 and (counts[labels == 0] > 0).any()
    assert got_b is not None and got_b.has_labels and got_b.B == want_b.B
    assert np.array_equal(got_b.counts, want_b.counts) and np.array_equal(got_b.read_idx(), want_b.read_idx())
    # the labels ride in the batch: the loss of one backward over it is a function of them
    la, lb = eng.backward(got_b, 1), eng.backward(want_b, 1)
    assert np.isfinite(la) and la == lb
    got_b.free(); want_b.free(); s.free()


def test_no_pair_has_a_path(g, engines):
    eng, gr = engines(3)
    s = eng.sampler(np.arange(1, 381, dtype=np.int32))
    batch, prs, counts, found = eng.find_training_paths(gr, s, np.array([g["cases"]["lonely"]], np.int32), 4, 1, 0, 2, 3, 28, 4)
    assert batch is None and (prs[1:, 1] > 0).all() and counts.tolist() == [0] * 5 and found.tolist() == [0] * 5
    s.free()


def test_sampler_does_not_depend_on_what_hipmalloc_returns(g, engines):
    """the sampler and the fused call in a fresh process with KPRN_POISON_ALLOC=1 (every new device allocation filled with 0xFF bytes), twice"""
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r)
        import numpy as np
        from kprn_amd import _ffi
        from tests import path_find_ref as ref, neg_sample_ref as nref
        from tests.test_gpu_neg_sample import positives_of
        g = ref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)
        cfg = nref.config_one(g)
        eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, 16, 32, 16, 64, 2)
        gr = eng.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL)
        s = eng.sampler(cfg["items"], cfg["weights"])
        out = []
        for _ in range(2):
            neg, nf = eng.sample_negatives(gr, s, cfg["users"], 8, 7, 0, max_attempts=4)
            b, prs, c, f = eng.find_training_paths(gr, s, positives_of(g), 8, 7, 2, 2, 3, 7, 4, max_attempts=4)
            out.append([neg.tolist(), nf.tolist(), prs.tolist(), c.tolist(), f.tolist(), b.read_idx().ravel().tolist()])
            b.free()
        eng.close()
        print(json.dumps(out))
    """) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    eng, gr = engines(3)
    cfg = nref.config_one(g)
    want = twin(g, cfg)
    s = eng.sampler(cfg["items"], cfg["weights"])
    b, prs, c, f = eng.find_training_paths(gr, s, positives_of(g), 8, 7, 2, 2, 3, 7, 4, max_attempts=4)
    idx = b.read_idx().ravel()
    b.free(); s.free()
    for neg, nf, p2, c2, f2, rows in json.loads(r.stdout.strip().splitlines()[-1]):
        assert np.array_equal(neg, want[0]) and np.array_equal(nf, want[1])
        assert np.array_equal(p2, prs) and np.array_equal(c2, c) and np.array_equal(f2, f) and np.array_equal(np.array(rows, np.int32), idx)


def _fresh(g, nt, F, deterministic):
    eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, seed=77, **SHAPES[F])
    if deterministic:
        eng.set_option("deterministic", "1")
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
    return eng, gr, eng.sampler(np.arange(1, 381, dtype=np.int32), ((np.arange(380) + 10.0) ** -0.8).astype(np.float32))


def test_training_loop_equals_the_hand_written_composition(g, nt, pairs):
    """three steps on the fused path with "deterministic" = 1: graph.train_from_graph on one engine, sample -> find -> train_step written out here on another"""
    pos = np.concatenate([positives_of(g), pairs[10:24]])                                # 21 positives: three minibatches of 7
    seed, n_neg, mb = 5, 3, 7
    opt = _ffi.make_opt(method=1, lr=2e-3)
    a, gra, sa = _fresh(g, nt, 3, True)
    stats = {}
    hist = kgraph.train_from_graph(a, gra, pos, opt, mb, n_neg, 1, seed, sampler=sa, max_attempts=8, max_paths=7, out=io.StringIO(), stats=stats)
    assert stats["steps"] == 3 and stats["skipped"] == 0 and len(hist) == 1 and np.isfinite(hist[0])
    b, grb, sb = _fresh(g, nt, 3, True)
    order = np.random.RandomState(seed + 1).permutation(len(pos))
    b.set_option("loss_accumulate", "1")
    b.loss_sum(reset=True)
    for step in range(3):
        batch = composition(b, grb, sb, pos[order[step * mb:(step + 1) * mb]], n_neg, 8, seed, step, 2, 3, 7, 4)[0]
        b.train_step(batch, opt, want_loss=False)
        batch.free()
    total, n = b.loss_sum(reset=True)
    assert n == 3 and hist[0] == total / 3
    for k in (0, 1):
        assert np.array_equal(a.get_flat_opt_state(k), b.get_flat_opt_state(k))
    ta, tb = a.get_flat_params(), b.get_flat_params()
    assert np.array_equal(ta, tb) and np.isfinite(ta).all()
    fresh = _fresh(g, nt, 3, True)
    assert not np.array_equal(fresh[0].get_flat_params(), ta)                             # (the steps moved the parameters)
    for e in (a, b, fresh[0]):
        e.close()


def test_one_step_on_the_rnn_shape(g, nt):
    eng, gr, s = _fresh(g, nt, 4, False)
    batch, prs, counts, _ = eng.find_training_paths(gr, s, positives_of(g), 4, 3, 0, 2, 3, 28, 4)
    assert batch.F == 4 and batch.B == int((counts > 0).sum())
    loss = eng.train_step(batch, _ffi.make_opt(method=1, lr=1e-3))
    assert np.isfinite(loss) and loss > 0
    for nm, V in (("type_emb", ref.VT), ("entity_emb", g["Ve"]), ("relation_emb", ref.VR)):
        assert np.all(eng.get_param(nm)[V - 1] == 0), nm                                  # zeroPadTokens
    batch.free()
    eng.close()


def test_train_command_line_from_a_graph(tmp_path, capsys):
    """python -m kprn_amd.train -kg (called in-process) twice with the same -sampleSeed: the same epoch lines, a checkpoint python -m kprn_amd.recommend loads"""
    from kprn_amd import recommend, train
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
    kg = kgraph.KnowledgeGraph.from_triples(triples, Vocabs(str(vdir)), 1)
    shape = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1]
    flags = shape + ["-gpuid", 0, "-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-interaction_rel", "rate", "-numEpochs", 2, "-saveFrequency", 1, "-minibatch", 4,
                     "-useAdam", 1, "-topK", 2, "-negatives", 2, "-sampleSeed", 3]
    runs = []
    for name in ("M", "N"):
        assert train.main([str(f) for f in flags + ["-model", tmp_path / name]]) == 0
        lines = capsys.readouterr().out.splitlines()
        runs.append([l for l in lines if not l.startswith(("total elapsed", "time per batch", "examples/sec", "saving to"))])
        assert (tmp_path / (name + "-latest")).exists()
    assert runs[0] == runs[1]
    losses = [float(l.split("=")[1]) for l in runs[0] if l.startswith("avg loss in epoch")]
    assert len(losses) == 2 and all(np.isfinite(l) and l > 0 for l in losses)
    assert [l for l in runs[0] if l.startswith("Iter: ")] == ["Iter: 1", "Iter: 2"]
    (tmp_path / "items.txt").write_text("\n".join("m%d" % m for m in range(5)) + "\n")
    buf = io.StringIO()
    rflags = shape + ["-gpu_id", 0, "-top_k", 2, "-model_path", tmp_path / "M-latest", "-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-user", "u0", "-items",
                      tmp_path / "items.txt", "-k", 3, "-explain_paths", 2]
    assert recommend.main([str(f) for f in rflags], out=buf) == 0
    heads = [l.split("\t") for l in buf.getvalue().splitlines() if l.split("\t")[1].startswith("m")]
    assert len(heads) >= 1
    # a vocabulary that is not the model flags': refused before any training
    bad = [str(f) for f in flags]
    bad[bad.index("-entityVocabSize") + 1] = str(kg.Ve + 1)
    with pytest.raises(SystemExit):
        train.main(bad)
