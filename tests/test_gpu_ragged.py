"""-m gpu: ragged batches (pairs with different path counts in one batch; an extension, the reference has none) against the float64 oracle.

The oracle is rectangular, so a ragged batch is checked per count group: the pairs of one count go through Oracle.forward /
Oracle.forward_backward(..., inv_batch = 1 / B_total) (kprn_oracle.c: inv_batch replaces 1/B), scores are scattered back, losses and
gradients are SUMMED.  Bars are the project's own (tests/test_gpu_parity.py): scores 1e-4 relative, path scores 2e-5 of scale, gradients 2e-4
of each tensor's largest entry, loss 1e-5; compute_dtype 1 at the bf16 bars of tests/test_gpu_wide.py / test_gpu_parity.py.
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from kprn_amd import _ffi, batcher, formats, scoring, synth
from oracle.oracle import Oracle, make_cfg, make_opt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_RTOL = 1e-4   # as tests/test_gpu_parity.py
GRAD_RTOL = 2e-4
MAX_SEG = _ffi.RAGGED_MAX_SEG   # 4096: the longest pair a ragged batch accepts (include/kprn.h)


def rel_inf(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(1e-30, np.max(np.abs(b))))


def mk(Vt=6, Ve=300, Vr=9, dt=16, de=32, dr=16, H=64, L=2, reducer=2, K=5, impl="auto", seed=1, init=0.1, compute_dtype=0, rnn_type=0, use_relu=1):
    eng = _ffi.Engine(Vt, Ve, Vr, dt, de, dr, H, L, reducer=reducer, K=K, compute_dtype=compute_dtype, rnn_type=rnn_type, use_relu=use_relu)
    eng.set_option("impl", impl)
    o64 = Oracle(make_cfg(Vt=Vt, Ve=Ve, Vr=Vr, dt=dt, de=de, dr=dr, H=H, L=L, reducer=reducer, K=K, rnn_type=rnn_type, use_relu=use_relu), np.float64)
    theta = o64.init_params(seed, init).astype(np.float32).astype(np.float64)   # the oracle sees exactly the fp32 values
    eng.set_flat_params(theta.astype(np.float32))
    return eng, o64, theta


def groups(counts):
    off = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    for P in np.unique(counts):
        pairs = np.nonzero(counts == P)[0]
        rows = (off[pairs][:, None] + np.arange(int(P))[None, :]).reshape(-1)
        yield int(P), pairs, rows


def oracle_forward(o64, theta, idx, counts):
    N, B = idx.shape[0], len(counts)
    ps = pooled = probs = None
    for P, pairs, rows in groups(counts):
        a, b, c = o64.forward(theta, idx[rows].reshape((len(pairs), P) + idx.shape[1:]))
        if ps is None:
            ps, pooled, probs = np.empty((N, a.shape[1])), np.empty((B, b.shape[1])), np.empty((B, c.shape[1]))
        ps[rows], pooled[pairs], probs[pairs] = a, b, c
    return ps, pooled, probs


def oracle_backward(o64, theta, idx, counts, labels, class_id=1, bce_literal=False):
    """loss and gradient of the whole ragged batch: per count group with inv_batch = 1 / (pairs of the WHOLE batch), summed"""
    B = len(counts)
    loss, grad = 0.0, np.zeros(o64.n)
    for P, pairs, rows in groups(counts):
        l, g, _ = o64.forward_backward(theta, idx[rows].reshape((len(pairs), P) + idx.shape[1:]), labels[pairs], class_id=class_id,
                                       bce_literal=bce_literal, inv_batch=1.0 / B)
        loss += l
        grad += g
    return loss, grad


def check(eng, o64, theta, idx, counts, labels, class_id=1, literal=False, batch=None, bars=None):
    score_bar, prob_kw, loss_bar, grad_bar = bars or (2e-5, dict(rtol=SCORE_RTOL), 1e-5, GRAD_RTOL)
    b = batch if batch is not None else eng.batch_ragged(idx, counts, labels)
    assert b.n_paths == idx.shape[0] and b.B == len(counts)
    out = eng.forward(b, class_id, want=("probs", "all_probs", "pooled", "path_scores"))
    ps, pooled, probs = oracle_forward(o64, theta, idx, counts)
    assert out["path_scores"].shape == ps.shape
    e = rel_inf(out["path_scores"], ps)
    assert e < score_bar, e
    if bars is None:
        np.testing.assert_allclose(out["pooled"], pooled, rtol=SCORE_RTOL, atol=2e-6)
    np.testing.assert_allclose(out["all_probs"], probs, **prob_kw)
    np.testing.assert_allclose(out["probs"], probs[:, class_id - 1], **prob_kw)
    loss = eng.backward(b, class_id, bce_literal=literal)
    ol, og = oracle_backward(o64, theta, idx, counts, labels, class_id, literal)
    assert abs(loss - ol) < loss_bar * max(1, abs(ol)), (loss, ol)
    g = eng.get_flat_grads()
    for nm, (off, shp) in eng.layout().items():
        n = int(np.prod(shp))
        r = rel_inf(g[off:off + n], og[off:off + n])
        assert r < grad_bar, (nm, r)
    return out


def count_vector(kind, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "ones":
        return np.ones(70, np.int32)
    if kind == "one_pair":
        return np.array([5], np.int32)
    if kind == "drawn":          # 150 pairs, ~260 paths: N is not a multiple of 16
        c = synth.draw_num_paths(rng, 150)
        if c.sum() % 16 == 0:
            c[0] += 1
        return c
    if kind == "tiles":          # above 64 tiles of 64 paths
        c = synth.draw_num_paths(rng, 2600)
        if c.sum() % 64 == 0:
            c[0] += 1
        assert c.sum() > 64 * 64
        return c
    if kind == "edges":          # both sides of every threshold and the longest segment
        return np.array([1, 28, 29, 63, 64, 65, 257, MAX_SEG, 3, 1], np.int32)
    if kind == "long":           # wave form, several long pairs in one loss-stage workgroup and across them
        return np.array([100, 30, 29, 500, 2, 28, 449, 64, 65, 1, 129], np.int32)
    raise KeyError(kind)


def data(counts, seed=5, Ve=300):
    return synth.make_ragged(len(counts), 6, Ve=Ve, seed=seed, counts=counts)[::2]   # idx, labels


MODES = {"tiles64_plan": ("0", "1"), "tiles64_noplan": ("0", "0"), "small_tiles": (None, "1")}


def set_mode(monkeypatch, mode):
    small, _plan = MODES[mode]
    if small is None:
        monkeypatch.delenv("KPRN_SMALL_TILES", raising=False)
    else:
        monkeypatch.setenv("KPRN_SMALL_TILES", small)


# (tile geometry and prefix plan belong to the fused kernels: the generic pipeline runs once per shape)
ROUTES = [("auto", L, m) for L in (2, 1) for m in sorted(MODES)] + [("generic", 2, "small_tiles"), ("generic", 1, "small_tiles")]


@pytest.mark.parametrize("impl,L,mode", ROUTES)
@pytest.mark.parametrize("kind", ["ones", "one_pair", "drawn", "edges"])
def test_fused_shape_matches_the_oracle(monkeypatch, mode, impl, L, kind):
    set_mode(monkeypatch, mode)
    eng, o64, theta = mk(L=L, impl=impl)
    eng.set_option("prefix_plan", MODES[mode][1])
    counts = count_vector(kind)
    idx, labels = data(counts)
    check(eng, o64, theta, idx, counts, labels)


@pytest.mark.parametrize("mode", ["tiles64_plan", "small_tiles"])
def test_more_than_64_tiles(monkeypatch, mode):
    set_mode(monkeypatch, mode)
    eng, o64, theta = mk(L=2)
    counts = count_vector("tiles")
    idx, labels = data(counts)
    check(eng, o64, theta, idx, counts, labels)


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("class_id", [1, 3])
@pytest.mark.parametrize("reducer,K", [(0, 5), (2, 5), (1, 1), (1, 2), (1, 28), (1, 29), (1, 500), (1, 600)])
def test_reducers_classes_and_bce_forms(reducer, K, class_id, literal):
    """counts 1 .. 500 in one batch: K below the smallest count is impossible (K >= 1), so K = 1 equals it, 2 .. 29 lie between, 500 equals
    the largest and 600 is above it: min(K, count) everywhere"""
    eng, o64, theta = mk(L=1, reducer=reducer, K=K, impl="generic")
    counts = count_vector("long")
    idx, labels = data(counts, seed=8)
    check(eng, o64, theta, idx, counts, labels, class_id=class_id, literal=literal)


@pytest.mark.parametrize("reducer,K", [(0, 5), (1, 3), (1, 40), (2, 5)])
@pytest.mark.parametrize("impl", ["auto", "generic"])
def test_score_ties_inside_long_segments(reducer, K, impl):
    """repeated paths score identically: Max takes ONE of them and TopK counts each position once, whichever lanes hold them"""
    eng, o64, theta = mk(L=1, reducer=reducer, K=K, impl=impl)
    counts = np.array([200, 3, 70, 28], np.int32)
    idx, labels = data(counts, seed=9)
    off = np.concatenate([[0], np.cumsum(counts)])
    idx[off[0] + 64:off[0] + 200] = idx[off[0]:off[0] + 1]          # 137 copies of the pair's first path, across all lanes
    idx[off[2] + 1:off[2] + 70:2] = idx[off[2] + 69:off[2] + 70]    # every other path of the third pair
    idx[off[3]:off[3] + 28] = idx[off[3]:off[3] + 1]                # a short pair of identical paths
    check(eng, o64, theta, idx, counts, labels)


@pytest.mark.parametrize("rnn_type,use_relu,H,L", [(0, 1, 96, 2), (1, 0, 96, 1), (1, 1, 96, 2), (2, 1, 96, 1), (2, 1, 64, 1)])
def test_wide_lstm_rnn_and_gru(rnn_type, use_relu, H, L):
    eng, o64, theta = mk(dt=32, de=32, dr=32, H=H, L=L, rnn_type=rnn_type, use_relu=use_relu, init=0.08)
    counts = np.concatenate([count_vector("drawn"), [70, 29]]).astype(np.int32)
    idx, labels = data(counts, seed=11)
    check(eng, o64, theta, idx, counts, labels)


@pytest.mark.parametrize("compute_dtype", [2, 3])
@pytest.mark.parametrize("kind", ["drawn", "long"])
def test_f32x6_holds_the_fp32_bars(monkeypatch, compute_dtype, kind):
    monkeypatch.setenv("KPRN_SMALL_TILES", "0")
    eng, o64, theta = mk(L=2, compute_dtype=compute_dtype)
    counts = count_vector(kind)
    idx, labels = data(counts, seed=12)
    check(eng, o64, theta, idx, counts, labels)


BF16_BARS = (3e-2, dict(atol=2e-2), 3e-2, 6e-2)   # tests/test_gpu_wide.py: scores, probabilities (absolute), loss, gradients


@pytest.mark.parametrize("dims,H,L", [((16, 32, 16), 64, 2), ((64, 64, 64), 192, 2)])
def test_bf16_pipeline_at_its_own_bars(dims, H, L):
    """compute_dtype 1 from 256 paths up (the bf16 storage pipeline trains; at D = H = 64 scoring runs on the fused matrix-core forward)"""
    dt, de, dr = dims
    eng, o64, theta = mk(Ve=700, Vr=100, dt=dt, de=de, dr=dr, H=H, L=L, compute_dtype=1, seed=4, init=0.05)
    counts = np.concatenate([synth.draw_num_paths(np.random.default_rng(2), 170), [65, 30]]).astype(np.int32)
    assert counts.sum() >= 256
    idx, labels = synth.make_ragged(len(counts), 6, Ve=700, Vr=100, seed=13, counts=counts)[::2]
    check(eng, o64, theta, idx, counts, labels, bars=BF16_BARS)


@pytest.mark.parametrize("impl", ["auto", "generic"])
@pytest.mark.parametrize("P", [1, 3, 28])
def test_equal_counts_give_the_rectangular_batch_bit_for_bit(impl, P):
    """the forward pass has no atomics: path scores, pooled values and probabilities of a ragged batch whose counts are all P are the bits of the
    rectangular batch; the loss within 1e-5 (fixed-order sums, possibly cut differently); gradients (atomic sums) each within the bar of the oracle"""
    eng, o64, theta = mk(L=2, impl=impl)
    idx, labels = synth.make_paths(53, P, 6, Ve=300, seed=14)
    counts = np.full(53, P, np.int32)
    flat = idx.reshape((-1,) + idx.shape[2:])
    want = ("probs", "all_probs", "pooled", "path_scores")
    rect = eng.forward(eng.batch(idx, labels), 1, want=want)
    rb = eng.batch_ragged(flat, counts, labels)
    rag = eng.forward(rb, 1, want=want)
    for k in want:
        assert np.array_equal(rect[k], rag[k]), k
    l_rect = eng.backward(eng.batch(idx, labels), 1)
    l_rag = eng.backward(rb, 1)
    assert abs(l_rect - l_rag) < 1e-5 * max(1, abs(l_rect))
    check(eng, o64, theta, flat, counts, labels, batch=rb)


def _train_compare(eng, o64, theta, batches, gpu_batches, opt_kw, steps, tol):
    """tests/test_gpu_parity.py _train_compare, with the engine's batches handed in (ragged here, rectangular for the oracle)"""
    oopt = make_opt(**{k: v for k, v in opt_kw.items() if k != "entity_update"})
    gopt = _ffi.make_opt(**opt_kw)
    th = theta.copy()
    st = o64.new_state()
    for s in range(steps):
        i, l = batches[s % len(batches)]
        ol, _ = o64.train_step(th, st, oopt, i, l)
        gl = eng.train_step(gpu_batches[s % len(batches)], gopt)
        assert abs(gl - ol) < 2e-4 * max(1.0, abs(ol)), (s, gl, ol)
    got = eng.get_flat_params()
    d = float(np.max(np.abs(got - th)))
    assert d < tol, d
    return got, th


def _pad_rows_are_zero(eng, Ve=300):
    for nm, V in (("type_emb", 6), ("entity_emb", Ve), ("relation_emb", 9)):
        assert np.all(eng.get_param(nm)[V - 1] == 0), nm   # zeroPadTokens (MyOptimizer.lua:74-93)


@pytest.mark.parametrize("impl", ["auto", "generic"])
@pytest.mark.parametrize("method,regularize,entity_update", [(1, 0, 0), (1, 0, 1), (0, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1)])
def test_training_on_equal_count_ragged_batches_matches_the_oracle(impl, method, regularize, entity_update):
    eng, o64, theta = mk(L=2, impl=impl)
    batches = [synth.make_paths(32, P, 6, Ve=300, seed=20 + P) for P in (1, 3, 2)]
    gb = [eng.batch_ragged(i.reshape((-1,) + i.shape[2:]), np.full(32, i.shape[1], np.int32), l) for i, l in batches]
    kw = dict(method=method, lr=1e-2, lr_decay=0.0167, regularize=regularize, use_grad_clip=1, grad_clip_norm=0.02, l2=1e-3, entity_update=entity_update)
    _train_compare(eng, o64, theta, batches, gb, kw, 10, 2e-4)
    _pad_rows_are_zero(eng)


@pytest.mark.parametrize("impl", ["auto", "generic"])
def test_adam_on_changing_ragged_batches_matches_a_float64_adam_on_the_oracles_gradients(impl):
    """10 Adam steps, regularize 0, a new truly ragged batch every step (long pairs among them), against okprn_train_step restated in numpy
    (kprn_oracle.c: zero pad rows, gradient, okprn_adam, zero pad rows) on the oracle's summed per-group gradients"""
    eng, o64, theta = mk(L=2, impl=impl)
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    gopt = _ffi.make_opt(method=1, lr=lr, regularize=0)
    th, m, v = theta.copy(), np.zeros_like(theta), np.zeros_like(theta)
    for s in range(10):
        counts = synth.draw_num_paths(np.random.default_rng(100 + s), 40 + 3 * s)
        if s % 3 == 0:
            counts[s] = 29 + 40 * s
        idx, labels = data(counts, seed=30 + s)
        gl = eng.train_step(eng.batch_ragged(idx, counts, labels), gopt)
        o64.zero_pad(th)
        ol, g = oracle_backward(o64, th, idx, counts, labels)
        t = s + 1
        step = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        m = m * b1 + (1.0 - b1) * g
        v = v * b2 + (1.0 - b2) * g * g
        th = th - step * (m / (np.sqrt(v) + eps))
        o64.zero_pad(th)
        assert abs(gl - ol) < 2e-4 * max(1.0, abs(ol)), (s, gl, ol)
    d = float(np.max(np.abs(eng.get_flat_params() - th)))
    assert d < 2e-4, d
    _pad_rows_are_zero(eng)


@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("kind", ["drawn", "long"])
def test_feed_ragged_equals_batch_ragged(monkeypatch, build, kind):
    monkeypatch.setenv("KPRN_SMALL_TILES", "0")
    eng, o64, theta = mk(L=2)
    eng.set_option("feed_build", build)
    counts = count_vector(kind)
    idx, labels = data(counts, seed=15)
    want = ("probs", "all_probs", "pooled", "path_scores")
    ref = eng.forward(eng.batch_ragged(idx, counts, labels), 1, want=want)
    slot = eng.feed_ragged(idx, counts, labels)
    got = eng.forward(slot, 1, want=want)
    for k in want:
        assert np.array_equal(ref[k], got[k]), k
    check(eng, o64, theta, idx, counts, labels, batch=slot)
    # a label-less slot (scoring only: no occurrence index is built on the host route)
    s2 = eng.feed_ragged(idx, counts)
    assert np.array_equal(eng.forward(s2, 1)["probs"], ref["probs"])


@pytest.mark.parametrize("build", ["host", "device"])
def test_a_slot_goes_ragged_rectangular_ragged(monkeypatch, build):
    monkeypatch.setenv("KPRN_SMALL_TILES", "0")
    eng, o64, theta = mk(L=2)
    eng.set_option("feed_build", build)
    c1, c2 = count_vector("long"), count_vector("drawn")
    i1, l1 = data(c1, seed=16)
    i2, l2 = data(c2, seed=17)
    ri, rl = synth.make_paths(45, 3, 6, Ve=300, seed=18)
    slot = eng.feed_ragged(i1, c1, l1)
    check(eng, o64, theta, i1, c1, l1, batch=slot)
    slot = eng.feed(ri, rl, slot=slot)
    assert slot.n_paths == 45 * 3
    ref = eng.forward(eng.batch(ri, rl), 1, want=("probs", "path_scores"))
    got = eng.forward(slot, 1, want=("probs", "path_scores"))
    assert np.array_equal(ref["probs"], got["probs"]) and np.array_equal(ref["path_scores"], got["path_scores"])
    l_slot, l_ref = eng.backward(slot, 1), eng.backward(eng.batch(ri, rl), 1)
    assert abs(l_slot - l_ref) < 1e-6 * max(1, abs(l_ref))
    slot = eng.feed_ragged(i2, c2, l2, slot=slot)
    check(eng, o64, theta, i2, c2, l2, batch=slot)
    # a reserved slot takes either without allocating
    res = _ffi.Batch.reserve(eng, 400, 5000, 6, 3)
    res.refill_ragged(i1, c1, l1)
    check(eng, o64, theta, i1, c1, l1, batch=res)
    res.refill(ri, rl)
    assert np.array_equal(eng.forward(res, 1)["probs"], ref["probs"])


@pytest.mark.parametrize("build", ["host", "device"])
def test_bad_ids_and_bad_counts_are_codes(build):
    eng, o64, theta = mk(L=1)
    eng.set_option("feed_build", build)
    counts = count_vector("drawn")
    idx, labels = data(counts, seed=19)
    bad = idx.copy()
    bad[7, 2, 1] = 301
    with pytest.raises(_ffi.KprnError) as e:
        eng.batch_ragged(bad, counts, labels)
    assert e.value.code == _ffi.E_INDEX
    slot = eng.feed_ragged(bad, counts, labels)        # the feed returns at once; the id surfaces at first use
    with pytest.raises(_ffi.KprnError) as e:
        eng.forward(slot, 1)
    assert e.value.code == _ffi.E_INDEX
    good = eng.feed_ragged(idx, counts, labels)
    for wrong in (np.where(np.arange(len(counts)) == 3, 0, counts), np.where(np.arange(len(counts)) == 3, -2, counts), counts[:-1],
                  np.concatenate([counts[:-1], [MAX_SEG + 1]])):
        wrong = wrong.astype(np.int32)
        with pytest.raises(_ffi.KprnError) as e:
            eng.batch_ragged(idx, wrong, labels[:len(wrong)])
        assert e.value.code == _ffi.E_ARG
        with pytest.raises(_ffi.KprnError) as e:
            eng.feed_ragged(idx, wrong, labels[:len(wrong)], slot=good)
        assert e.value.code == _ffi.E_ARG
    check(eng, o64, theta, idx, counts, labels, batch=good)   # a refused refill left the slot as it was


_POISON = textwrap.dedent("""
    import sys, json, numpy as np
    sys.path.insert(0, %r)
    from kprn_amd import _ffi, synth
    eng = _ffi.Engine(6, 300, 9, 16, 32, 16, 64, 2, seed=3)
    counts = np.array([100, 30, 29, 500, 2, 28, 449, 64, 65, 1, 129] + [1, 2, 3] * 20, np.int32)
    idx, _, labels = synth.make_ragged(len(counts), 6, Ve=300, seed=5, counts=counts)
    opt = _ffi.make_opt(method=1, lr=1e-3)
    losses = [eng.train_step(eng.feed_ragged(idx, counts, labels), opt) for _ in range(3)]
    probs = eng.forward(eng.batch_ragged(idx, counts), 1)["probs"]
    print(json.dumps({"losses": losses, "probs": probs.astype(float).tolist(), "theta": float(np.abs(eng.get_flat_params()).sum())}))
""")


def test_training_steps_with_poisoned_allocations():
    """KPRN_POISON_ALLOC=1 fills every new device allocation with 0xFF bytes: a ragged step that read something it never wrote (offsets,
    workgroup table, a gradient slot of a long pair) would turn NaN or differ from the unpoisoned run"""
    import json
    res = {}
    for tag, env in (("plain", {}), ("poison", {"KPRN_POISON_ALLOC": "1"})):
        r = subprocess.run([sys.executable, "-c", _POISON % ROOT], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        res[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = res["plain"], res["poison"]
    assert np.isfinite(b["losses"]).all() and np.isfinite(b["probs"]).all() and np.isfinite(b["theta"])
    np.testing.assert_allclose(b["losses"], a["losses"], rtol=1e-5)
    np.testing.assert_allclose(b["probs"], a["probs"], rtol=1e-4)


@pytest.mark.parametrize("dual", ["0", "1", "2"])
def test_async_scoring_of_a_small_ragged_batch_around_a_training_step(dual):
    """forward_async, then a training step (score_dual: the pass rides in the training forward's launch and its pooling stage in the loss
    stage's), then read_probs -- the probabilities are those of the parameters BEFORE the step"""
    eng, o64, theta = mk(L=2)
    o64.zero_pad(theta)   # a training step zeroes the pad rows first (MyOptimizer.lua:181): scoring pass and step then see the same parameters
    eng.set_flat_params(theta.astype(np.float32))
    eng.set_option("score_overlap", "1")
    eng.set_option("score_dual", dual)
    cs, ct = count_vector("long"), count_vector("drawn")
    si, _ = data(cs, seed=21)
    ti, tl = data(ct, seed=22)
    sb, tb = eng.batch_ragged(si, cs), eng.batch_ragged(ti, ct, tl)
    rect_i, rect_l = synth.make_paths(40, 2, 6, Ve=300, seed=23)
    rect = eng.batch(rect_i, rect_l)
    _, _, probs = oracle_forward(o64, theta, si, cs)
    opt = _ffi.make_opt(method=1, lr=1e-3)
    # ragged passenger in a ragged step
    eng.forward_async(sb, 1)
    l1 = eng.train_step(tb, opt)
    np.testing.assert_allclose(eng.read_probs(len(cs)), probs[:, 0], rtol=SCORE_RTOL)
    ol, _ = oracle_backward(o64, theta, ti, ct, tl)
    assert abs(l1 - ol) < 1e-5 * max(1, abs(ol))
    # ragged passenger in a rectangular step, rectangular passenger in a ragged step
    th = eng.get_flat_params().astype(np.float64)
    eng.forward_async(sb, 1)
    eng.train_step(rect, opt)
    np.testing.assert_allclose(eng.read_probs(len(cs)), oracle_forward(o64, th, si, cs)[2][:, 0], rtol=SCORE_RTOL)
    th = eng.get_flat_params().astype(np.float64)
    eng.forward_async(rect, 1)
    eng.train_step(tb, opt)
    np.testing.assert_allclose(eng.read_probs(40), o64.forward(th, rect_i)[2][:, 0], rtol=SCORE_RTOL)


def test_score_split_on_a_ragged_batch(monkeypatch):
    monkeypatch.setenv("KPRN_SMALL_TILES", "0")
    eng, o64, theta = mk(L=2)
    eng.set_option("score_overlap", "1")
    eng.set_option("score_split", "0.5")
    counts = count_vector("tiles")
    idx, _ = data(counts, seed=24)
    b = eng.batch_ragged(idx, counts)
    eng.forward_async(b, 1)
    eng.forward_async_rest()
    _, _, probs = oracle_forward(o64, theta, idx, counts)
    np.testing.assert_allclose(eng.read_probs(len(counts)), probs[:, 0], rtol=SCORE_RTOL)


def test_one_call_for_one_users_candidates():
    """ranking ~101 candidate items of one user: one kprn_forward_ragged against one kprn_forward per distinct path count, within 2e-6 relative
    (the bar tests/test_gpu_parity.py sets for sub-batches of one batch)"""
    eng, o64, theta = mk(L=2)
    counts = synth.draw_num_paths(np.random.default_rng(7), 101)
    idx, _ = data(counts, seed=25)
    probs, allp = eng.forward_ragged_host(idx, counts, 1, want_all=True)
    want = np.empty(101, np.float32)
    want_all = np.empty((101, 46), np.float32)
    for P, pairs, rows in groups(counts):
        p, a = eng.forward_host(idx[rows].reshape((len(pairs), P) + idx.shape[1:]), 1)
        want[pairs], want_all[pairs] = p, a
    np.testing.assert_allclose(probs, want, rtol=2e-6)
    np.testing.assert_allclose(allp, want_all, rtol=2e-6)
    np.testing.assert_allclose(probs, oracle_forward(o64, theta, idx, counts)[2][:, 0], rtol=SCORE_RTOL)
    p2, none = eng.forward_ragged_host(idx, counts, 1)
    assert none is None and np.array_equal(p2, probs)


def test_merged_scoring_writes_the_same_lines(tmp_path):
    root = str(tmp_path)
    buckets = synth.make_bucketed(20000, 6, Ve=300, seed=31)
    names = []
    for P in sorted(buckets):
        bi, bl = buckets[P]
        formats.save_path_file(os.path.join(root, "test_%d.npz" % P), bl, bi, 1)
        names.append("test_%d.npz" % P)
    with open(os.path.join(root, "test.list"), "w") as f:
        f.write("\n".join(names) + "\n")
    eng, o64, theta = mk(L=2)
    n1 = scoring.test_from_checkpoint(eng, root, "test.list", os.path.join(root, "plain.res"))
    n2 = scoring.test_from_checkpoint(eng, root, "test.list", os.path.join(root, "merged.res"), merge_path_counts=True)
    a = [l.split("\t") for l in open(os.path.join(root, "plain.res")).read().splitlines()]
    b = [l.split("\t") for l in open(os.path.join(root, "merged.res")).read().splitlines()]
    assert n1 == n2 == len(a) == len(b) == sum(len(v[1]) for v in buckets.values())
    assert [x[0] for x in a] == [x[0] for x in b] and [x[2] for x in a] == [x[2] for x in b]
    # the probabilities themselves, before they are printed with five decimals
    fl = lambda: batcher.BatcherFileList(root, 512, False, 1000, True, "test.list", check_ids=False)
    pa = np.concatenate([p for _, p in scoring.score_batches(eng, fl(), 1)])
    pb = np.concatenate([p for _, p in scoring.score_batches(eng, fl(), 1, merge=True)])
    assert len(pa) == len(pb) == n1
    np.testing.assert_allclose(pb, pa, rtol=SCORE_RTOL)
    for lines, p in ((a, pa), (b, pb)):   # the files hold these values, printed with five decimals
        assert np.max(np.abs(np.array([float(x[1]) for x in lines]) - p)) <= 0.51e-5
    # and through the command line
    from kprn_amd import model, score
    ck = os.path.join(root, "model")
    eng.save(ck)
    out = os.path.join(root, "cli.res")
    flags = ["-input_dir", root, "-test_list", "test.list", "-out_file", out, "-model_path", ck, "-mergePathCounts", "1", "-top_k", "2"]
    flags += ["-entityVocabSize", "300", "-relationVocabSize", "9", "-entityTypeVocabSize", "6", "-rnnHidSize", "64", "-numLayers", "2", "-rnnType", "lstm",
              "-entityTypeEmbeddingDim", "16", "-entityEmbeddingDim", "32", "-relationEmbeddingDim", "16", "-numFeatureTemplates", "3", "-numEntityTypes", "1",
              "-includeEntity", "1"]
    assert score.main(flags) == 0
    assert open(out).read() == open(os.path.join(root, "merged.res")).read() and model is not None


_DP = textwrap.dedent("""
    import sys, json, threading, numpy as np
    sys.path.insert(0, %(root)r)
    from kprn_amd import _ffi, synth
    W, LOOP, steps = %(W)d, %(lib)r, 4
    mk = lambda rank, world: _ffi.Engine(6, 3000, 9, 16, 32, 16, 64, 2, rank=rank, world=world, param_init=0.1, seed=777)
    ref = mk(0, 1)
    theta = ref.get_flat_params()
    reps = [mk(r, W) for r in range(W)]
    for e in reps:
        e.set_flat_params(theta)
    uid = _ffi.dp_unique_id(LOOP)
    for r, e in enumerate(reps):
        e.dp_init(uid, r, W, LOOP)
    per = 12                                     # pairs per rank per step; the caller cuts the flat path array at pair boundaries
    counts = synth.draw_num_paths(np.random.default_rng(3), per * W)
    counts[1], counts[per + 2] = 70, 33          # long pairs on two ranks: wave form there, thread form on the others
    idx, _, lab = synth.make_ragged(per * W, 6, Ve=3000, seed=44, counts=counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    bref = ref.batch_ragged(idx, counts, lab)
    shards = [reps[r].batch_ragged(idx[off[r * per]:off[(r + 1) * per]], counts[r * per:(r + 1) * per], lab[r * per:(r + 1) * per]) for r in range(W)]
    cap = (max(b.n_uniq for b in shards) + 3) // 4 * 4
    opt = _ffi.make_opt(method=1, lr=1e-2)
    errors = []
    def rank_step(r):
        try:
            e, b = reps[r], shards[r]
            e.zero_pad_tokens()
            e.backward(b, 1, False, 1.0 / (per * W), want_loss=False)   # the loss is scaled by the pairs of the GLOBAL minibatch
            e.dp_exchange_begin(cap)
            e.dp_exchange_finish(opt)
            e.sync()
        except Exception as ex:   # noqa: BLE001
            errors.append((r, repr(ex)))
    for step in range(steps):
        ref.train_step(bref, opt)
        th = [threading.Thread(target=rank_step, args=(r,)) for r in range(W)]
        for t in th: t.start()
        for t in th: t.join()
        assert not errors, errors
    flats = [e.get_flat_params() for e in reps]
    a = ref.get_flat_params()
    print(json.dumps({"identical": bool(all(np.array_equal(flats[0], f) for f in flats[1:])), "vs_one_handle": float(np.max(np.abs(a - flats[0]))),
                      "moved": float(np.max(np.abs(a - theta)))}))
    for e in reps:
        e.dp_shutdown()
""")


@pytest.mark.parametrize("W", [2, 3])
def test_data_parallel_exchange_with_ragged_shards(W):
    """kprn_dp_* at the C level with ragged batches (pairs are what is sharded), through the loopback communicator of
    tests/test_gpu_dp_loopback.py and at its bars: replicas bit-identical, equal to one handle fed the global ragged minibatch to 3e-5"""
    import json
    from tests.test_gpu_dp_loopback import build_loopback
    r = subprocess.run([sys.executable, "-c", _DP % dict(root=ROOT, W=W, lib=build_loopback())], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-2500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["moved"] > 1e-3 and out["identical"], out
    assert out["vs_one_handle"] < 3e-5, out


def test_my_optimizer_train_batch_takes_ragged_inputs():
    """MyOptimizer.trainBatch with (idx [N,T,F], counts [B]) and with a ragged Batch: the same step, the oracle's loss"""
    import io
    from kprn_amd import optimizer
    counts = count_vector("long")
    idx, labels = data(counts, seed=26)
    losses = []
    for form in ("tuple", "batch"):
        eng, o64, theta = mk(L=2)
        o64.zero_pad(theta)
        eng.set_flat_params(theta.astype(np.float32))
        opt = optimizer.MyOptimizer(eng, {"numEpochs": 1, "epochHooks": [], "minibatchsize": 16}, _ffi.make_opt(method=1, lr=1e-3), out=io.StringIO())
        inputs = (idx, counts) if form == "tuple" else eng.batch_ragged(idx, counts, labels)
        err = opt.trainBatch(inputs, labels if form == "tuple" else None)
        ol, _ = oracle_backward(o64, theta, idx, counts, labels)
        assert abs(err - ol) < 1e-5 * max(1, abs(ol)) and opt.totalError == err
        losses.append((err, eng.get_flat_params()))
    assert losses[0][0] == losses[1][0]
    assert np.max(np.abs(losses[0][1] - losses[1][1])) < 1e-6   # (gradients are atomic sums: equal to rounding, not to the bit)
