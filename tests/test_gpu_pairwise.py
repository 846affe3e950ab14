"""-m gpu: the pairwise (BPR) loss over groups (include/kprn.h "pairwise loss"; option "loss" = "bpr", kprn_batch_set_groups, k_loss_stage_pairwise of
kprn_amd/csrc/loss_stage.hip) against the float64 oracle, and the graph trainer on it.

The oracle knows BCE only.  Its closed-form BCE gradient is (p - t) inv_batch for any real t, so it is fed the pseudo-labels t' = p - dy / inv_batch
(tests/pairwise_ref.py), p from its own forward and dy from the float64 restatement of the rule: it then back-propagates exactly that dy.  The
reference loss is the restatement's.  Bars: tests/test_gpu_ragged.py check()'s -- loss 1e-5 max(1, |L|), every parameter tensor's gradient 2e-4 of
its largest entry.

The parameters must spread theta = y_i - y_j: at the suites' init = 0.1 every pooled score agrees to 1e-3, every sigma is 0.5 and a wrong formula
passes.  Hence init = 0.3 and out.weight x 30 (pooled scores then spread with a standard deviation near 1), and every parity test asserts on the
oracle's numbers that there are terms and that the standard deviation of theta over them is at least 0.5: conditions on the inputs, not tolerances.
Shapes: D = H = 64, Ve = 300, T = 6.
"""
import functools
import io

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph, synth
from oracle.oracle import make_opt
from tests import path_find_ref as pref
from tests.pairwise_ref import offsets, pairwise, pseudo_labels
from tests.test_gpu_path_find import SHAPES
from tests.test_gpu_ragged import MODES, data, mk, oracle_backward, oracle_forward, rel_inf, set_mode

pytestmark = pytest.mark.gpu

REDUCERS = [(0, 5), (1, 3), (2, 5)]   # nn.Max, TopK(3) + Mean, LogSumExp
# (impl, L, tile mode, rnn_type): the fused path on every tile geometry with the prefix plan on and off, the generic FastLSTM pipeline, the rnn cell
ROUTES = [("auto", L, m, 0) for L in (2, 1) for m in sorted(MODES)] + [("generic", 2, "small_tiles", 0), ("auto", 2, "small_tiles", 1)]
LOSS_BAR, GRAD_BAR = 1e-5, 2e-4

# group shapes of batch (a): 1 + 4 | a lone positive | a lone negative | two positives among five | 1 + 16 | 1 + 14 | a positive that is last of nine
SIZES_A = [5, 1, 1, 5, 17, 15, 9]
LABELS_A = np.concatenate([[1, 0, 0, 0, 0], [1], [0], [0, 1, 0, 1, 0], [1] + [0] * 16, [1] + [0] * 14, [0] * 8 + [1]]).astype(np.float32)
assert sum(SIZES_A) == len(LABELS_A) == 53


def bits(x):
    return int(np.float32(x).view(np.uint32))


def spread(eng, o64, theta):
    """out.weight x 30, re-rounded through fp32 as mk rounds: the oracle sees exactly the engine's values"""
    off, shp = o64.layout()["out.weight"]
    theta = theta.copy()
    theta[off:off + int(np.prod(shp))] *= 30.0
    theta = theta.astype(np.float32).astype(np.float64)
    eng.set_flat_params(theta.astype(np.float32))
    return theta


def mkp(monkeypatch, route, reducer, K):
    impl, L, mode, rnn_type = route
    set_mode(monkeypatch, mode)
    eng, o64, theta = mk(L=L, reducer=reducer, K=K, impl=impl, rnn_type=rnn_type, seed=41, init=0.3)
    eng.set_option("prefix_plan", MODES[mode][1])
    eng.set_option("loss", "bpr")
    return eng, o64, spread(eng, o64, theta)


@functools.lru_cache(maxsize=None)
def batch_of(kind):
    """-> idx [N, T, F] (flat), counts [B], labels [B], group_offsets; P of the rectangular ones is counts[0]"""
    if kind == "a":     # rectangular, B = 53, P = 3
        idx = synth.make_paths(53, 3, 6, Ve=300, seed=41)[0]
        return idx.reshape((-1,) + idx.shape[2:]), np.full(53, 3, np.int32), LABELS_A, offsets(SIZES_A)
    if kind == "b":     # ragged: drawn counts, a pair of 70 paths and one of 449 inside the 1 + 16 group (the wave form), and an empty group
        counts = synth.draw_num_paths(np.random.default_rng(3), 53)
        counts[15], counts[20] = 70, 449
        return data(counts, seed=47)[0], counts, LABELS_A, offsets(SIZES_A[:4] + [0] + SIZES_A[4:])
    if kind == "c":     # one group of 1 + 256 pairs of one path each
        idx = synth.make_paths(257, 1, 6, Ve=300, seed=48)[0]
        return idx.reshape((-1,) + idx.shape[2:]), np.ones(257, np.int32), np.array([1] + [0] * 256, np.float32), offsets([257])
    raise KeyError(kind)


def make_batch(eng, kind):
    idx, counts, labels, go = batch_of(kind)
    if kind == "b":
        return eng.batch_ragged(idx, counts, labels)
    return eng.batch(idx.reshape((len(counts), int(counts[0])) + idx.shape[1:]), labels)


def reference(o64, theta, idx, counts, labels, go, class_id=1, inv_batch=0.0):
    """the float64 loss and flat gradient of the pairwise rule over this batch at theta, through the oracle's BCE backward on pseudo-labels"""
    _, pooled, probs = oracle_forward(o64, theta, idx, counts)
    r = pairwise(pooled[:, class_id - 1], labels, go, inv_batch)
    r["y"] = pooled[:, class_id - 1]
    assert r["n_terms"] > 0
    sd = float(np.std(r["theta"]))
    assert sd >= 0.5, sd
    tl = pseudo_labels(probs[:, class_id - 1], r["dy"], 1.0 / len(counts))   # (oracle_backward's inv_batch is 1 / B)
    _, grad = oracle_backward(o64, theta, idx, counts, tl, class_id)
    assert np.all(np.isfinite(grad))
    return r, grad


_REFS = {}


def cached_reference(key, o64, theta, kind):
    """one oracle pass per (layers, cell, reducer, batch): the routes of one model share it (same parameters: mk's seed and spread)"""
    if key not in _REFS:
        _REFS[key] = (theta.copy(),) + reference(o64, theta, *batch_of(kind))
    th, r, grad = _REFS[key]
    assert np.array_equal(th, theta)
    return r, grad


def compare(eng, b, r, grad, what, inv_batch=0.0):
    loss = eng.backward(b, 1, inv_batch=inv_batch)
    print(f"{what}: loss {loss!r} oracle {r['loss']!r} n_terms {r['n_terms']} sd(theta) {float(np.std(r['theta'])):.3f}")
    assert abs(loss - r["loss"]) < LOSS_BAR * max(1.0, abs(r["loss"])), (what, loss, r["loss"])
    g = eng.get_flat_grads()
    for nm, (off, shp) in eng.layout().items():
        n = int(np.prod(shp))
        if nm == "out.bias":
            # The loss does not change when every score of a group moves by the same amount, so each group's dy adds up to zero and so does this tensor,
            # the sum of dS over all paths: the oracle's value is float64 rounding noise (1e-17) and an error relative to IT says nothing.  The same bar
            # on the scale of the sum's largest addend, max |dy_b|, instead.
            e = float(np.max(np.abs(g[off:off + n] - grad[off:off + n])) / np.max(np.abs(r["dy"])))
            assert float(np.max(np.abs(grad[off:off + n]))) < 1e-12
        else:
            e = rel_inf(g[off:off + n], grad[off:off + n])
        print(f"    {nm}: rel_inf {e:.3e}")
        assert e < GRAD_BAR, (what, nm, e)
    return loss


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reducer,K", REDUCERS)
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "-".join(str(x) for x in r))
def test_parity_with_the_float64_oracle(monkeypatch, route, reducer, K):
    eng, o64, theta = mkp(monkeypatch, route, reducer, K)
    for kind in ("a", "b", "c"):
        b = make_batch(eng, kind)
        r, grad = cached_reference((route[1], route[3], reducer, K, kind), o64, theta, kind)
        assert b.set_groups(batch_of(kind)[3]) == r["n_terms"]
        compare(eng, b, r, grad, f"batch {kind}")
        np.testing.assert_allclose(eng.read_probs(b.B), 1.0 / (1.0 + np.exp(-r["y"])), rtol=1e-4)   # sel[b] = sigmoid(y_b) is still stored
        b.free()
    eng.close()


def test_inv_batch_is_the_scale_when_given(monkeypatch):
    eng, o64, theta = mkp(monkeypatch, ROUTES[2], 2, 5)
    idx, counts, labels, go = batch_of("a")
    b = make_batch(eng, "a")
    b.set_groups(go)
    r, grad = reference(o64, theta, idx, counts, labels, go, inv_batch=1.0 / 64)
    assert r["s"] == 1.0 / 64
    compare(eng, b, r, grad, "inv_batch 1/64", inv_batch=1.0 / 64)
    eng.close()


# ---- 2. no terms: the loss is 0.0f and EVERY entry of dS was written ------------------------------------------------------------------------
@pytest.mark.parametrize("reducer,K", REDUCERS)
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "-".join(str(x) for x in r))
def test_groups_without_terms_give_zero_loss_and_zero_gradients(monkeypatch, route, reducer, K):
    """30 positives then 23 negatives.  One training step over the whole batch as one group first, so that dS holds that step's values; then the table
    positives | negatives | an empty group, which has no term: the loss is +0.0f and every gradient is zero -- a pair without a term has its dS
    entries written, not skipped.  Rectangular, and ragged with pairs the wave form reduces."""
    eng, _, _ = mkp(monkeypatch, route, reducer, K)
    labels = np.array([1] * 30 + [0] * 23, np.float32)
    idx = batch_of("a")[0]
    counts = batch_of("b")[1]
    for b in (eng.batch(idx.reshape(53, 3, 6, -1), labels), eng.batch_ragged(batch_of("b")[0], counts, labels)):
        assert b.set_groups([0, 53]) == 30 * 23
        assert np.isfinite(eng.train_step(b, _ffi.make_opt(method=1, lr=1e-3)))
        assert b.set_groups([0, 30, 53, 53]) == 0
        loss = eng.backward(b, 1)
        assert bits(loss) == 0, loss
        g = eng.get_flat_grads()
        assert not np.any(g), float(np.max(np.abs(g)))
        b.free()
    eng.close()


# ---- 3. the same bits twice ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("impl", ["auto", "generic"])
def test_the_loss_has_the_same_bits_twice(monkeypatch, impl, kind):
    eng, _, _ = mkp(monkeypatch, (impl, 2, "small_tiles", 0), 2, 5)
    b = make_batch(eng, kind)
    b.set_groups(batch_of(kind)[3])
    l0, l1 = eng.backward(b, 1), eng.backward(b, 1)
    assert np.isfinite(l0) and l0 > 0 and bits(l0) == bits(l1), (l0, l1)
    eng.close()


@pytest.mark.parametrize("kind", ["a", "b"])
def test_deterministic_gradients_have_the_same_bytes_twice(monkeypatch, kind):
    eng, _, _ = mkp(monkeypatch, ("auto", 2, "small_tiles", 0), 2, 5)
    eng.set_option("deterministic", "1")
    b = make_batch(eng, kind)
    b.set_groups(batch_of(kind)[3])
    l0 = eng.backward(b, 1)
    g0 = eng.get_flat_grads().tobytes()
    l1 = eng.backward(b, 1)
    assert bits(l0) == bits(l1) and eng.get_flat_grads().tobytes() == g0 and np.any(np.frombuffer(g0, np.float32))
    eng.close()


# ---- 4. the passengers of the loss stage's launch ride in the pairwise launch too ---------------------------------------------------------------
def test_the_weight_transposes_ride(monkeypatch):
    """Three Adam steps (dense entity update) on the fused two-layer path against Oracle.train_step fed each step's pseudo-labels, computed at that step's
    zero-padded parameters; parameters within the project's 2e-4 absolute (tests/test_gpu_parity.py).  The fused backward multiplies by transposed
    copies of the LSTM weights that passenger workgroups of the loss stage rebuild after an update: without them every backward after the first update
    runs on stale copies.  So, behind the steps, one more backward is held to the oracle's gradient AT THE ENGINE'S OWN parameters, at the gradient bar:
    copies that are three updates of 1e-2 old miss it by orders of magnitude.
    Adam's eps is 1e-4 here: out.bias has an exactly zero gradient under this loss (compare()), the engine's is fp32 rounding noise of 1e-10 .. 1e-9, and
    with the default eps = 1e-8 Adam's g / (|g| + eps) turns that noise into a good part of a full step of lr."""
    eng, o64, theta = mkp(monkeypatch, ("auto", 2, "small_tiles", 0), 2, 5)
    idx, counts, labels, go = batch_of("a")
    B = len(counts)
    rect = idx.reshape((B, 3) + idx.shape[1:])
    b = make_batch(eng, "a")
    b.set_groups(go)
    kw = dict(method=1, lr=1e-2, eps=1e-4)
    th, st = theta.copy(), o64.new_state()
    lay = eng.layout()
    for step in range(3):
        at = th.copy()
        o64.zero_pad(at)
        _, pooled, probs = o64.forward(at, rect)
        r = pairwise(pooled[:, 0], labels, go)
        assert r["n_terms"] > 0 and float(np.std(r["theta"])) >= 0.5
        o64.train_step(th, st, make_opt(**kw), rect, pseudo_labels(probs[:, 0], r["dy"], 1.0 / B))
        loss = eng.train_step(b, _ffi.make_opt(entity_update=1, **kw))
        diff = np.abs(eng.get_flat_params() - th)
        d = float(np.max(diff))
        worst = max(lay, key=lambda nm: float(np.max(diff[lay[nm][0]:lay[nm][0] + int(np.prod(lay[nm][1]))])))
        print(f"step {step}: loss {loss!r} oracle {r['loss']!r} max |dtheta| {d:.3e} in {worst}")
        assert abs(loss - r["loss"]) < 2e-4 * max(1.0, abs(r["loss"])), (step, loss, r["loss"])   # (the parameters' bar: the two sides have drifted that far apart)
        assert d < 2e-4, (step, d)
    own = eng.get_flat_params().astype(np.float64)
    r, grad = reference(o64, own, idx, counts, labels, go)
    compare(eng, b, r, grad, "after three updates")
    eng.close()


@pytest.mark.parametrize("train", ["rectangular", "ragged"])
@pytest.mark.parametrize("score", ["rectangular", "ragged"])
def test_a_scoring_pass_rides_in_a_pairwise_training_step(monkeypatch, score, train):
    """tests/test_gpu_loss_stage.py test_a_scoring_pass_rides_in_a_training_step under "loss" = "bpr": the riding pass's pooling stage is a passenger of the
    pairwise launch; its probabilities are the bytes of eng.forward, no pooling launch of its own shows in the profile, the pairwise stage does"""
    eng, o64, theta = mkp(monkeypatch, ("auto", 2, "small_tiles", 0), 2, 5)
    o64.zero_pad(theta)
    eng.set_flat_params(theta.astype(np.float32))
    for key, value in (("score_overlap", "1"), ("score_dual", "2"), ("prefix_plan", "0")):
        eng.set_option(key, value)
    if score == "ragged":
        cs = np.concatenate([synth.draw_num_paths(np.random.default_rng(5), 37), [70]]).astype(np.int32)
        sb = eng.batch_ragged(data(cs, seed=43)[0], cs)
    else:
        sb = eng.batch(synth.make_paths(40, 2, 6, Ve=300, seed=44)[0])
    kind = "b" if train == "ragged" else "a"
    tb = make_batch(eng, kind)
    assert tb.set_groups(batch_of(kind)[3]) > 0
    opt = _ffi.make_opt(method=1, lr=1e-3, entity_update=1)
    eng.train_step(tb, opt)
    for step in range(2):
        want = eng.forward(sb, 1)["probs"]
        eng.profile(True)
        eng.profile_reset()
        eng.forward_async(sb, 1)
        loss = eng.train_step(tb, opt)
        got = eng.read_probs(sb.B)
        prof = eng.profile_get()
        eng.profile(False)
        assert np.isfinite(loss) and loss > 0
        assert "lstm_fused_fwd_dual" in prof and "loss_stage_pairwise" in prof and "pool_sigmoid" not in prof and "loss_stage" not in prof, sorted(prof)
        assert got.tobytes() == want.tobytes(), float(np.max(np.abs(got - want)))
    eng.close()


# ---- 5. refusals write nothing ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_gradients_and_parameters_untouched(monkeypatch):
    eng, _, _ = mkp(monkeypatch, ("auto", 2, "small_tiles", 0), 2, 5)
    idx, counts, labels, go = batch_of("a")
    rect = idx.reshape((53, 3) + idx.shape[1:])
    opt = _ffi.make_opt(method=1, lr=1e-3)
    b = make_batch(eng, "a")
    n_terms = b.set_groups(go)
    loss = eng.backward(b, 1)
    state = lambda: (eng.get_flat_grads().tobytes(), eng.get_flat_params().tobytes())
    before = state()
    assert np.any(np.frombuffer(before[0], np.float32))

    def refused(code, fn):
        with pytest.raises(_ffi.KprnError) as e:
            fn()
        assert e.value.code == code, (e.value.code, e.value.msg)
        assert state() == before, e.value.msg

    # no table
    bare = make_batch(eng, "a")
    refused(_ffi.E_ARG, lambda: eng.train_step(bare, opt))
    refused(_ffi.E_ARG, lambda: eng.backward(bare, 1))
    # a batch without labels takes no table
    unl = eng.batch(rect)
    refused(_ffi.E_ARG, lambda: unl.set_groups(go))
    # a table dropped by a refill of its slot
    slot = eng.feed(rect, labels)
    assert slot.set_groups(go) == n_terms
    slot.refill(rect, labels)
    refused(_ffi.E_ARG, lambda: eng.train_step(slot, opt))
    assert slot.set_groups(go) == n_terms   # (and set again it trains: below)
    # bad tables, each leaving the batch's previous table in place
    for bad in ([0, 20, 10, 53], [1, 53], [0, 52], [0, 54], [0]):
        refused(_ffi.E_ARG, lambda: b.set_groups(bad))
    big_idx, big_lab = synth.make_paths(1026, 1, 6, Ve=300, seed=49)
    big = eng.batch(big_idx, big_lab)
    assert big.set_groups([0, 1024, 1026]) >= 0
    refused(_ffi.E_ARG, lambda: big.set_groups([0, 1025, 1026]))
    # host buffers carry no groups
    refused(_ffi.E_UNSUPPORTED, lambda: eng.train_step_host(rect, labels, opt))
    # an unknown value of the option; the option stays
    refused(_ffi.E_ARG, lambda: eng.set_option("loss", "hinge"))
    assert eng.options["loss"] == "bpr"
    # the first batch still has its table: the same loss, bit for bit
    assert bits(eng.backward(b, 1)) == bits(loss)
    assert np.isfinite(eng.train_step(slot, opt)) and state()[1] != before[1]
    # and with the option back at its default the same batches train on BCE, table or none
    eng.set_option("loss", "bce")
    assert np.isfinite(eng.train_step(bare, opt)) and np.isfinite(eng.train_step_host(rect, labels, opt))
    eng.close()


# ---- 6. the graph trainer ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    return pref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)   # (the graph of tests/test_gpu_neg_sample.py)


def fresh(g):
    eng = _ffi.Engine(pref.VT, g["Ve"], pref.VR, seed=77, **SHAPES[3])
    eng.set_option("deterministic", "1")
    eng.zero_pad_tokens()   # (a training step zeroes the pad rows first: the forward taken before the step then sees the step's parameters)
    gr = eng.graph(g["src"], g["dst"], g["rel"], pref.node_types(g, 1), pref.END_REL)
    return eng, gr, eng.sampler(np.arange(1, 381, dtype=np.int32), ((np.arange(380) + 10.0) ** -0.8).astype(np.float32))


def positives_of(g):
    c = g["cases"]
    return np.array([c["exact"], c["inside"], c["direct"], c["hub_user"], (5, 9), (17, 40), c["hub_next"]], np.int32)


def test_one_step_of_the_graph_trainer_equals_the_composition(g):
    pos = positives_of(g)
    seed, n_neg = 5, 3
    opt = _ffi.make_opt(method=1, lr=2e-3)
    a, gra, sa = fresh(g)
    start = a.get_flat_params()
    stats = {}
    hist = kgraph.train_from_graph(a, gra, pos, opt, len(pos), n_neg, 1, seed, sampler=sa, max_attempts=8, max_paths=7, out=io.StringIO(), stats=stats,
                                   loss="bpr")
    assert stats["steps"] == 1 and stats["skipped"] == 0 and len(hist) == 1
    assert a.options["loss"] == "bce"   # put back
    b, grb, sb = fresh(g)
    order = np.random.RandomState(seed + 1).permutation(len(pos))
    batch, prs, counts, _ = b.find_training_paths(grb, sb, pos[order], n_neg, seed, 0, 2, 3, 7, 4, max_attempts=8)
    go = kgraph.groups_from_counts(counts, n_neg)
    labels = (np.arange(len(counts)) % (1 + n_neg) == 0).astype(np.float32)[counts > 0]
    assert go[-1] == batch.B == len(labels) and len(go) == len(pos) + 1
    pooled = b.forward(batch, 1, want=("pooled",))["pooled"][:, 0]
    want_loss, _, want_terms = _ffi.host_pairwise_loss(pooled, labels, go)
    b.set_option("loss", "bpr")
    assert batch.set_groups(go) == want_terms and want_terms > 0
    loss = b.train_step(batch, opt)
    batch.free()
    print(f"graph step: loss {loss!r} host twin {want_loss!r} n_terms {want_terms} avg {hist[0]!r}")
    assert abs(loss - want_loss) < 1e-5 * abs(want_loss), (loss, want_loss)
    assert hist[0] == loss
    ta, tb = a.get_flat_params(), b.get_flat_params()
    assert ta.tobytes() == tb.tobytes() and np.isfinite(ta).all() and not np.array_equal(ta, start)
    for e in (a, b):
        e.close()


def test_a_minibatch_whose_positives_lack_paths_is_skipped(g):
    """the hub reaches most of the graph, the lonely node has no edge: the positive (hub, lonely) has no path, its sampled negatives have -- a batch of
    negatives only, which BCE would train on and the pairwise loss has no term for"""
    eng, gr, s = fresh(g)
    pos = np.array([(g["cases"]["hub"], g["cases"]["lonely"][0])], np.int32)
    seed, n_neg = 5, 3
    batch, _, counts, _ = eng.find_training_paths(gr, s, pos, n_neg, seed, 0, 2, 3, 7, 4, max_attempts=8)
    assert batch is not None and counts[0] == 0 and (counts[1:] > 0).any(), counts
    batch.free()
    before = eng.get_flat_params().tobytes()
    stats = {}
    kgraph.train_from_graph(eng, gr, pos, _ffi.make_opt(method=1, lr=2e-3), 1, n_neg, 1, seed, sampler=s, max_attempts=8, max_paths=7, out=io.StringIO(),
                            stats=stats, loss="bpr")
    assert stats == dict(steps=0, skipped=1, pairs=0), stats
    assert eng.get_flat_params().tobytes() == before
    eng.close()


def test_train_command_line_with_loss_bpr(tmp_path, capsys):
    """python -m kprn_amd.train -kg ... -loss bpr (called in-process, the small graph of tests/test_gpu_neg_sample.py's command-line test): two epochs, finite
    epoch losses that are not the BCE run's (same seeds, so the minibatches are the same: only the loss differs), a checkpoint"""
    from kprn_amd import train
    from kprn_amd.pathformat import Vocabs
    from tests.test_path_find_host import _write_vocab
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
    flags = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1, "-gpuid", 0, "-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-interaction_rel", "rate", "-numEpochs", 2, "-saveFrequency", 1,
             "-minibatch", 4, "-useAdam", 1, "-topK", 2, "-negatives", 2, "-sampleSeed", 3]
    losses = {}
    for name in ("bpr", "bce"):
        assert train.main([str(f) for f in flags + ["-model", tmp_path / name, "-loss", name]]) == 0
        lines = capsys.readouterr().out.splitlines()
        losses[name] = [float(l.split("=")[1]) for l in lines if l.startswith("avg loss in epoch")]
        assert (tmp_path / (name + "-latest")).exists()
        assert len(losses[name]) == 2 and all(np.isfinite(v) and v > 0 for v in losses[name]), losses
    print(losses)
    assert losses["bpr"] != losses["bce"]
