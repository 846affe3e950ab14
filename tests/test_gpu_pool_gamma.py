"""-m gpu: the pooling temperature (include/kprn.h "pooling temperature"; option "pool_gamma") on the device.

The independent reference is the UNMODIFIED float64 oracle on theta' = theta with out.weight and out.bias divided by gamma (tests/pool_gamma_ref.py states
the identity, tests/test_pool_gamma_host.py checks it on the CPU): probabilities and loss are equal, every gradient outside the head is equal, and the head's
gradients map by 1 / gamma.  Bars are the project's (tests/test_gpu_ragged.py): path scores 2e-5 of scale, probabilities 1e-4 relative, loss 1e-5,
gradients 2e-4 of each tensor's largest entry; compute_dtype 1 at BF16_BARS.  Shapes: D = H = 64, Ve = 300, T = 6.

Inputs.  At init 0.1 a pair's scores span 0.01 and gamma is invisible, so the cases are (init 0.5, gamma 0.5), (0.5, 2) and (0.3, 0.1); every parity case
first asserts on the oracle's own numbers that at least half of its pairs of two or more paths spread their shares 3 : 1 (pool_gamma_ref.spread_conditions;
1.5 : 1 at gamma = 2, where 3 : 1 is out of reach for any input: share_ratio_bar) and that no label-0 pair has |pooled| > 6 (above that 1 - p loses in
fp32 the digits the loss bar needs).  The data seeds are the ones at which the first holds for both depths and both classes; for the second, a label-0 pair
whose reference |pooled| exceeds 6 is made a positive (pool_gamma_ref.labels_within_the_loss_bar) -- both decided on the oracle's numbers alone.

Every test here fails on the parent commit at its first set_option("pool_gamma", ...): the option is unknown there.

Explanations are compared with kprn_host_explain_gamma to the bit: under a temperature the kernels and the twin take exp and log from the same plain-fp32
functions (csrc/reduce_dev.h exp_shared / log_shared), not from two different libraries.  test_explain_batch_against_the_twin also holds the shares to the
derived bound against the float64 rule's own statement in the twin, and pooled / prob to the bytes of Engine.forward."""
import io
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph, synth
from tests import pool_gamma_ref as ref
from tests.test_gpu_loss_stage import EDGES
from tests.test_gpu_ragged import BF16_BARS, GRAD_RTOL, SCORE_RTOL, data, mk, oracle_backward, oracle_forward, rel_inf
from tests.test_pool_gamma_host import gamma_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(0.5, 0.5), (0.5, 2.0), (0.3, 0.1)]          # (init, gamma): both conditions hold on the oracle alone
KEYS = ("path_idx", "path_score", "path_weight", "pooled", "probs")
FP32_BARS = (2e-5, dict(rtol=SCORE_RTOL), 1e-5, GRAD_RTOL)


def mkg(gamma, init, **kw):
    """engine at (theta, gamma), the oracle, theta and theta' (float64: the oracle sees exactly the engine's fp32 theta, divided by gamma)"""
    eng, o64, theta = mk(init=init, **kw)
    eng.set_option("pool_gamma", repr(gamma))
    return eng, o64, theta, ref.scaled_head(theta, o64.layout(), gamma)


_REFS = {}


def oracle_case(key, o64, theta, theta_p, gamma, idx, counts, labels, class_id, literal):
    """the oracle's numbers for one (model, batch, class, BCE form), computed once and shared by the routes: the labels to train on, path scores at theta,
    pooled / probs / loss / gradient through theta', the gradient mapped back; the two input conditions are asserted here, on these numbers alone"""
    k = key + (class_id, literal)
    if k not in _REFS:
        ps, _, _ = oracle_forward(o64, theta, idx, counts)
        _, pooled, probs = oracle_forward(o64, theta_p, idx, counts)
        off = np.concatenate([[0], np.cumsum(counts)])
        mine = ref.pool_pairs(ps[:, class_id - 1], off, gamma)
        assert np.max(np.abs(mine[0] - pooled[:, class_id - 1])) < 1e-9           # the identity, on this batch
        labels = ref.labels_within_the_loss_bar(labels, pooled[:, class_id - 1])
        spread, worst = ref.spread_conditions(ps[:, class_id - 1], off, labels, gamma)
        assert spread >= 0.5, (k, spread)
        assert worst <= 6.0, (k, worst)
        loss, grad_p = oracle_backward(o64, theta_p, idx, counts, labels, class_id, literal)
        out = (labels, ps, pooled, probs, loss, ref.map_head_grads(grad_p, o64.layout(), gamma))
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REFS[k] = (theta.copy(),) + out
    assert np.array_equal(_REFS[k][0], theta)
    return _REFS[k][1:]


def check(eng, want, batch, class_id, literal, bars=FP32_BARS):
    score_bar, prob_kw, loss_bar, grad_bar = bars
    _, ps, pooled, probs, ol, og = want
    out = eng.forward(batch, class_id, want=("probs", "all_probs", "pooled", "path_scores"))
    e = rel_inf(out["path_scores"], ps)
    assert e < score_bar, e
    if bars is FP32_BARS:
        np.testing.assert_allclose(out["pooled"][:, class_id - 1], pooled[:, class_id - 1], rtol=SCORE_RTOL, atol=2e-6)
    np.testing.assert_allclose(out["all_probs"], probs, **prob_kw)
    np.testing.assert_allclose(out["probs"], probs[:, class_id - 1], **prob_kw)
    loss = eng.backward(batch, class_id, bce_literal=literal)
    assert abs(loss - ol) < loss_bar * max(1, abs(ol)), (loss, ol)
    g = eng.get_flat_grads()
    for nm, (off, shp) in eng.layout().items():
        n = int(np.prod(shp))
        r = rel_inf(g[off:off + n], og[off:off + n])
        assert r < grad_bar, (nm, r)


RECT = [(1, 1, 41), (1, 28, 43), (17, 1, 41), (17, 28, 41)]          # B, P, data seed
RAGGED = {"waves": ([3, 29, 1, 70, 28, 5, 2, 11], 45)}               # a 29-path pair (the first the wave form takes) and a 70-path pair; data seed
RAGGED.update({k: (v[0], 42 if k == "single_pair_workgroups" else 45) for k, v in EDGES.items()})


# ---- 1. parity with the oracle through the scaled head -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["auto", "generic"])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("init,gamma", CASES)
def test_rectangular_parity_through_the_scaled_head(init, gamma, L, impl):
    eng, o64, theta, theta_p = mkg(gamma, init, L=L, impl=impl)
    for B, P, seed in RECT:
        idx, labels = synth.make_paths(B, P, 6, Ve=300, seed=seed)
        flat, counts = idx.reshape((-1,) + idx.shape[2:]), np.full(B, P, np.int32)
        for class_id in (1, 3):
            for literal in (False, True):
                want = oracle_case((L, init, gamma, "rect", B, P), o64, theta, theta_p, gamma, flat, counts, labels, class_id, literal)
                check(eng, want, eng.batch(idx, want[0]), class_id, literal)
    eng.close()


@pytest.mark.parametrize("impl", ["auto", "generic"])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("init,gamma", CASES)
@pytest.mark.parametrize("kind", sorted(RAGGED))
def test_ragged_parity_through_the_scaled_head(kind, init, gamma, L, impl):
    """thread form and wave form of the reducer, its backward through slot_of on the fused path (impl auto), and the ragged cut's workgroup edges"""
    eng, o64, theta, theta_p = mkg(gamma, init, L=L, impl=impl)
    counts = np.array(RAGGED[kind][0], np.int32)
    idx, labels = data(counts, seed=RAGGED[kind][1])
    for class_id, literal in ((1, False), (3, True), (1, True), (3, False)) if kind == "waves" else ((1, False), (3, True)):
        want = oracle_case((L, init, gamma, kind), o64, theta, theta_p, gamma, idx, counts, labels, class_id, literal)
        check(eng, want, eng.batch_ragged(idx, counts, want[0]), class_id, literal)
    eng.close()


# ---- 2. gamma = 1 is the engine without the option ---------------------------------------------------------------------------------------------------
def step_bits(eng, batches):
    out = []
    for b in batches:
        loss = eng.backward(b, 1)
        out.append((np.float32(loss).tobytes(), eng.forward(b, 1, want=("probs", "pooled"))["probs"].tobytes(), eng.get_flat_grads().tobytes()))
    return out


def test_gamma_one_has_the_bits_of_an_engine_that_never_saw_the_option():
    """deterministic "1", one engine: set 0.5, run, set "1", run -- loss, probabilities and flat gradients have the bits of a fresh engine, rectangular and ragged"""
    idx, labels = synth.make_paths(17, 28, 6, Ve=300, seed=41)
    counts = np.array(RAGGED["waves"][0], np.int32)
    ridx, rlabels = data(counts, seed=42)

    def batches(eng):
        return [eng.batch(idx, labels), eng.batch_ragged(ridx, counts, rlabels)]

    fresh, _, _ = mk(L=2, init=0.5)
    fresh.set_option("deterministic", "1")
    want = step_bits(fresh, batches(fresh))
    fresh.close()
    eng, _, _ = mk(L=2, init=0.5)
    eng.set_option("deterministic", "1")
    eng.set_option("pool_gamma", "0.5")
    other = step_bits(eng, batches(eng))
    assert all(o[1] != w[1] and o[2] != w[2] for o, w in zip(other, want))          # (the option does something)
    eng.set_option("pool_gamma", "1")
    got = step_bits(eng, batches(eng))
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2]
    eng.close()


# ---- 3. the engine against itself through the identity -------------------------------------------------------------------------------------------------
def twin_engines(gamma, init, **kw):
    """engine (theta, gamma) and engine (theta', gamma = 1); theta' is rounded to fp32 once (gamma = 0.5 and 2 scale the head exactly)"""
    a, o64, theta = mk(init=init, **kw)
    a.set_option("pool_gamma", repr(gamma))
    b, _, _ = mk(init=init, **kw)
    b.set_flat_params(ref.scaled_head(theta, o64.layout(), gamma).astype(np.float32))
    return a, b


def compare_engines(a, b, ba, bb, gamma, bars, inv_batch=0.0):
    score_bar, prob_kw, loss_bar, grad_bar = bars
    np.testing.assert_allclose(a.forward(ba, 1)["probs"], b.forward(bb, 1)["probs"], **prob_kw)
    la, lb = a.backward(ba, 1, inv_batch=inv_batch), b.backward(bb, 1, inv_batch=inv_batch)
    print("loss under gamma %r: %r, through the scaled head: %r" % (gamma, la, lb))
    assert abs(la - lb) < loss_bar * max(1, abs(lb)), (la, lb)
    ga, gb = a.get_flat_grads().astype(np.float64), ref.map_head_grads(b.get_flat_grads(), a.layout(), gamma)
    lay = a.layout()
    for nm, (off, shp) in lay.items():
        n = int(np.prod(shp))
        scale = np.max(np.abs(gb[off:off + n]))
        if nm == "out.bias":
            # (under the pairwise loss a group's dy adds up to zero and this tensor, the sum of dS over all paths, is rounding noise: the bar on the scale
            #  of out.weight, whose entries are sums of the same addends times |h| < 1)
            wo, ws = lay["out.weight"]
            scale = max(scale, np.max(np.abs(gb[wo:wo + int(np.prod(ws))])))
        e = float(np.max(np.abs(ga[off:off + n] - gb[off:off + n])) / max(scale, 1e-30))
        assert e < grad_bar, (nm, e)


def test_pairwise_loss_on_a_group_table():
    from tests.test_gpu_pairwise import LABELS_A, SIZES_A
    from tests.pairwise_ref import offsets
    a, b = twin_engines(0.5, 0.5, L=2)
    counts = synth.draw_num_paths(np.random.default_rng(3), 53)
    counts[15], counts[20] = 70, 449                                             # the wave form inside the 1 + 16 group
    idx = data(counts, seed=47)[0]
    go = offsets(SIZES_A)
    batches = []
    for e in (a, b):
        e.set_option("loss", "bpr")
        bt = e.batch_ragged(idx, counts, LABELS_A)
        assert bt.set_groups(go) > 0
        batches.append(bt)
    compare_engines(a, b, batches[0], batches[1], 0.5, FP32_BARS)
    a.close(); b.close()


def test_select_hardest_picks_the_same_rows():
    a, b = twin_engines(0.5, 0.5, L=2)
    counts = synth.draw_num_paths(np.random.default_rng(4), 90)
    counts[7] = 70
    idx = data(counts, seed=48)[0]
    goff = np.array([0, 9, 30, 31, 90], np.int64)
    pos = np.array([0, 3, 0, -1], np.int32)                                      # the positive's index within its group; -1: none
    keeps = []
    for e in (a, b):
        bt = e.batch_ragged(idx, counts)
        e.forward_async(bt, 1)
        e.board_reserve(90)
        e.board_put(0, 90)
        keeps.append(e.select_hardest(goff, 4, pos=pos))
    # gamma = 0.5 scales the head by 2, which commutes with every fp32 rounding, so the two engines pool the same exponents; engine a takes exp and log from
    # reduce_dev.h's shared functions and engine b from the library, a few units in the last place apart.  The selection is compared in every group whose
    # boundary -- the gap between the last kept and the first dropped negative -- is wider than twice the boards' largest difference; that is all of them
    # unless two probabilities collide to within some 1e-7, and three of the four groups have to qualify (one has a single member and no boundary).
    sa, sb = a.board_read(0, 90).astype(np.float64), b.board_read(0, 90).astype(np.float64)
    np.testing.assert_allclose(sa, sb, rtol=SCORE_RTOL)
    noise, compared = 2.0 * float(np.max(np.abs(sa - sb))), 0
    assert keeps[0][1] == keeps[1][1]
    for g in range(4):
        lo, hi = int(goff[g]), int(goff[g + 1])
        neg = np.sort(np.delete(sb[lo:hi], pos[g]) if pos[g] >= 0 else sb[lo:hi])[::-1]
        if len(neg) > 4 and neg[3] - neg[4] <= noise:
            continue
        assert np.array_equal(keeps[0][0][lo:hi], keeps[1][0][lo:hi]), g
        compared += 1
    assert compared >= 3
    a.close(); b.close()


@pytest.mark.parametrize("rnn_type", [1, 2])
def test_rnn_and_gru_at_h_250(rnn_type):
    a, b = twin_engines(0.5, 0.3, dt=32, de=32, dr=32, H=250, L=1, rnn_type=rnn_type)
    counts = np.array([3, 29, 1, 70, 28, 5, 2, 11], np.int32)
    idx, labels = data(counts, seed=49)
    compare_engines(a, b, a.batch_ragged(idx, counts, labels), b.batch_ragged(idx, counts, labels), 0.5, FP32_BARS)
    a.close(); b.close()


def test_bf16_pipeline_at_its_own_bars():
    a, b = twin_engines(0.5, 0.3, Ve=700, Vr=100, L=2, compute_dtype=1, seed=4)
    counts = np.concatenate([synth.draw_num_paths(np.random.default_rng(2), 170), [65, 30]]).astype(np.int32)
    assert counts.sum() >= 256
    idx, labels = synth.make_ragged(len(counts), 6, Ve=700, Vr=100, seed=13, counts=counts)[::2]
    compare_engines(a, b, a.batch_ragged(idx, counts, labels), b.batch_ragged(idx, counts, labels), 0.5, BF16_BARS)
    a.close(); b.close()


# ---- 4. explanation -----------------------------------------------------------------------------------------------------------------------------------
EXPLAIN_COUNTS = np.array([1, 28, 70, 2, 449, 29, 5], np.int32)


def explain_case(gamma, ragged, M, class_id):
    eng, _, _ = mk(L=2, init=0.5)
    eng.set_option("pool_gamma", repr(gamma))
    if ragged:
        counts = EXPLAIN_COUNTS
        idx = data(counts, seed=50)[0]
        batch = eng.batch_ragged(idx, counts)
    else:
        counts = np.full(17, 28, np.int32)
        batch = eng.batch(synth.make_paths(17, 28, 6, Ve=300, seed=41)[0])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    fwd = eng.forward(batch, class_id, want=("probs", "pooled", "path_scores"))
    dev = eng.explain_batch(batch, M, class_id)
    host = _ffi.host_explain(fwd["path_scores"], off, class_id, 2, 5, M, gamma=gamma)
    eng.close()
    return dev, host, fwd, counts


@pytest.mark.parametrize("M", [1, 3, 32])
@pytest.mark.parametrize("ragged", [False, True], ids=["thread", "wave"])
@pytest.mark.parametrize("gamma", [0.5, 0.25])
def test_explain_batch_against_the_twin(gamma, ragged, M):
    """index and raw score: the twin's bits.  pooled / prob: the bytes Engine.forward returns.  Shares: within gamma_bound of the twin
    (tests/test_pool_gamma_host.py derives the bound), and within the same bound they add up to 1."""
    for class_id in (1, 3):
        dev, host, fwd, counts = explain_case(gamma, ragged, M, class_id)
        assert dev["path_idx"].tobytes() == host["path_idx"].tobytes()
        assert dev["path_score"].tobytes() == host["path_score"].tobytes()
        assert dev["pooled"].tobytes() == np.ascontiguousarray(fwd["pooled"][:, class_id - 1]).tobytes()
        assert dev["probs"].tobytes() == fwd["probs"].tobytes()
        tol = np.array([gamma_bound(int(n), gamma) for n in counts])
        err = np.abs(dev["path_weight"].astype(np.float64) - host["path_weight"]).max(axis=1)
        print("gamma %r M %d class %d: worst share error / bound = %.3f" % (gamma, M, class_id, float((err / tol).max())))
        assert np.all(err <= tol)
        full = counts <= M
        assert np.all(np.abs(dev["path_weight"][full].astype(np.float64).sum(axis=1) - 1.0) <= tol[full] + counts[full] * 2.0 ** -24)
        ptol = tol + 2.0 ** -22 * np.maximum(1.0, np.abs(host["pooled"]))
        assert np.all(np.abs(dev["pooled"].astype(np.float64) - host["pooled"]) <= ptol)
        top = dev["path_weight"][:, 0].astype(np.float64)
        assert np.all(top[counts >= 2] < 1.0) and np.median(top[counts == 28] * 28) > 1.5      # (peaked, not uniform: gamma is visible in the shares)


@pytest.mark.parametrize("ragged", [False, True], ids=["thread", "wave"])
def test_explain_batch_equals_the_twin_bit_for_bit(ragged):
    """index, score, share, pooled and prob of explain_batch are the twin's bits on the batch's path scores (M = 1, 3, 32; gamma 0.5 and 0.25, class 1 and 3)"""
    worst = 0
    for M in (1, 3, 32):
        dev, host, _, _ = explain_case(0.25, ragged, M, 3)
        for k in KEYS:
            assert dev[k].tobytes() == host[k].tobytes(), (M, k)
        dev, host, _, _ = explain_case(0.5, ragged, M, 1)
        for k in ("path_weight", "pooled", "probs"):
            d = np.abs(dev[k].view(np.int32).astype(np.int64) - host[k].view(np.int32).astype(np.int64))
            print("M %d %s: %d of %d values differ from the twin, by at most %d units in the last place" % (M, k, int((d > 0).sum()), d.size, int(d.max())))
            worst = max(worst, int(d.max()))
        assert dev["path_idx"].tobytes() == host["path_idx"].tobytes() and dev["path_score"].tobytes() == host["path_score"].tobytes()
    for M in (1, 3, 32):
        dev, host, _, _ = explain_case(0.5, ragged, M, 1)
        for k in KEYS:
            assert dev[k].tobytes() == host[k].tobytes(), (M, k, worst)


def test_recommend_explain_ragged_gives_the_same_on_its_winners():
    eng, _, _ = mk(L=2, init=0.5)
    eng.set_option("pool_gamma", "0.5")
    group_counts = [30, 1, 6]
    counts = synth.draw_num_paths(np.random.default_rng(61), 37)
    counts[[5, 33]] = (100, 70)
    idx = data(counts, seed=51)[0]
    goff = np.concatenate([[0], np.cumsum(group_counts)]).astype(np.int64)
    for K, M in ((4, 3), (8, 32)):
        ti, ts, probs = eng.recommend_ragged(idx, counts, group_counts, K, want_probs=True)
        r = eng.recommend_explain_ragged(idx, counts, group_counts, K, M, want_probs=True)
        assert r["topk_idx"].tobytes() == ti.tobytes() and r["topk_score"].tobytes() == ts.tobytes() and r["probs"].tobytes() == probs.tobytes()
        valid = ti >= 0
        pairs = (goff[:-1, None] + ti)[valid].astype(np.int32)
        e = eng.explain_batch(eng.batch_ragged(idx, counts), M, 1, pairs=pairs)
        for k in ("path_idx", "path_score", "path_weight"):
            assert r[k][valid].tobytes() == e[k].tobytes(), k
        assert e["probs"].tobytes() == probs[pairs].tobytes()
        plain = _ffi.host_explain(eng.forward(eng.batch_ragged(idx, counts), 1, want=("path_scores",))["path_scores"],
                                  np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), 1, 2, 5, M, pairs=pairs, gamma=1.0)
        assert np.max(np.abs(plain["path_weight"] - e["path_weight"])) > 1e-3          # (not the shares of gamma = 1)
    eng.close()


# ---- 5. a scoring pass that rides in a training step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score", ["rectangular", "ragged"])
def test_a_riding_scoring_pass_pools_under_gamma(score):
    """tests/test_gpu_loss_stage.py test_a_scoring_pass_rides_in_a_training_step ("score_dual" 2) at gamma = 0.5: the riding pass's probabilities are the
    bytes of eng.forward before the step (and not those of gamma = 1)"""
    eng, o64, theta = mk(L=2, init=0.5)
    o64.zero_pad(theta)
    eng.set_flat_params(theta.astype(np.float32))
    for key, value in (("score_overlap", "1"), ("score_dual", "2"), ("prefix_plan", "0"), ("pool_gamma", "0.5")):
        eng.set_option(key, value)
    if score == "ragged":
        cs = np.concatenate([synth.draw_num_paths(np.random.default_rng(5), 37), [70]]).astype(np.int32)
        sb = eng.batch_ragged(data(cs, seed=43)[0], cs)
    else:
        sb = eng.batch(synth.make_paths(40, 2, 6, Ve=300, seed=44)[0])
    tb = eng.batch(*synth.make_paths(53, 3, 6, Ve=300, seed=46))
    opt = _ffi.make_opt(method=1, lr=1e-3, entity_update=1)
    eng.train_step(tb, opt)
    for step in range(2):
        want = eng.forward(sb, 1)["probs"]
        eng.set_option("pool_gamma", "1")
        plain = eng.forward(sb, 1)["probs"]
        eng.set_option("pool_gamma", "0.5")
        eng.profile(True)
        eng.profile_reset()
        eng.forward_async(sb, 1)
        loss = eng.train_step(tb, opt)
        got = eng.read_probs(sb.B)
        prof = eng.profile_get()
        eng.profile(False)
        assert np.isfinite(loss)
        assert "lstm_fused_fwd_dual" in prof and "loss_stage" in prof and "pool_sigmoid" not in prof, sorted(prof)
        assert got.tobytes() == want.tobytes() and got.tobytes() != plain.tobytes()
    eng.close()


# ---- 6. training -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["auto", "generic"])
def test_adam_on_changing_ragged_batches_against_a_float64_adam_on_the_mapped_gradients(impl):
    """tests/test_gpu_ragged.py test_adam_on_changing_ragged_batches... at gamma = 0.5: five steps, a new ragged batch each, at that test's tolerance"""
    gamma = 0.5
    eng, o64, theta, _ = mkg(gamma, 0.5, L=2, impl=impl)
    lay = o64.layout()
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    gopt = _ffi.make_opt(method=1, lr=lr, regularize=0)
    th, m, v = theta.copy(), np.zeros_like(theta), np.zeros_like(theta)
    for s in range(5):
        counts = synth.draw_num_paths(np.random.default_rng(100 + s), 40 + 3 * s)
        if s % 3 == 0:
            counts[s] = 29 + 40 * s
        idx, labels = data(counts, seed=30 + s)
        gl = eng.train_step(eng.batch_ragged(idx, counts, labels), gopt)
        o64.zero_pad(th)
        ol, gp = oracle_backward(o64, ref.scaled_head(th, lay, gamma), idx, counts, labels)
        g = ref.map_head_grads(gp, lay, gamma)
        t = s + 1
        step = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        m = m * b1 + (1.0 - b1) * g
        v = v * b2 + (1.0 - b2) * g * g
        th = th - step * (m / (np.sqrt(v) + eps))
        o64.zero_pad(th)
        assert abs(gl - ol) < 2e-4 * max(1.0, abs(ol)), (s, gl, ol)
    d = float(np.max(np.abs(eng.get_flat_params() - th)))
    assert d < 2e-4, d
    eng.close()


# ---- 7. the option and the checkpoint ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_value():
    eng, _, _ = mk(L=2, init=0.5)
    batch = eng.batch(synth.make_paths(17, 28, 6, Ve=300, seed=41)[0])
    at_one = eng.forward(batch, 1)["probs"].tobytes()
    eng.set_option("pool_gamma", "0.5")
    at_half = eng.forward(batch, 1)["probs"].tobytes()
    assert at_half != at_one
    for bad in ("0", "-0.5", "nan", "inf", "-inf", "1e-4", "0.00099", "1000.5", "1e4", " 0.5", "0.5 ", "0x1p-1", "+0.5", "", "half", "1e400", "0.5f"):
        with pytest.raises(_ffi.KprnError) as ei:
            eng.set_option("pool_gamma", bad)
        assert ei.value.code == _ffi.E_ARG, bad
        assert eng.forward(batch, 1)["probs"].tobytes() == at_half, bad
    for ok in ("1e-3", "1e3", ".5", "5e-1"):
        eng.set_option("pool_gamma", ok)
    assert eng.forward(batch, 1)["probs"].tobytes() == at_half
    eng.set_option("pool_gamma", "1")
    assert eng.forward(batch, 1)["probs"].tobytes() == at_one
    eng.close()


@pytest.mark.parametrize("reducer", [0, 1])
def test_max_and_topk_have_no_temperature(reducer):
    eng, _, _ = mk(L=1, init=0.5, reducer=reducer, K=3)
    batch = eng.batch(synth.make_paths(17, 28, 6, Ve=300, seed=41)[0])
    want = eng.forward(batch, 1)["probs"].tobytes()
    for g in ("0.5", "2"):
        with pytest.raises(_ffi.KprnError) as ei:
            eng.set_option("pool_gamma", g)
        assert ei.value.code == _ffi.E_UNSUPPORTED and "LogSumExp" in str(ei.value)
    eng.set_option("pool_gamma", "1")
    eng.set_option("pool_gamma", "1.0")
    assert eng.forward(batch, 1)["probs"].tobytes() == want
    eng.close()


def test_the_checkpoint_carries_gamma(tmp_path):
    eng, _, _ = mk(L=2, init=0.5)
    batch_idx = synth.make_paths(17, 28, 6, Ve=300, seed=41)[0]
    eng.save(str(tmp_path / "one"))
    raw = open(tmp_path / "one", "rb").read()
    assert raw[8 + 14 * 4:8 + 15 * 4] == b"\0\0\0\0"                                # saved under 1: header word 14 is 0
    eng.set_option("pool_gamma", "0.5")
    want = eng.forward(eng.batch(batch_idx), 1)["probs"]
    eng.save(str(tmp_path / "half"))
    half = open(tmp_path / "half", "rb").read()
    assert half[8 + 14 * 4:8 + 15 * 4] == np.float32(0.5).tobytes() and half[:64] == raw[:64] and half[68:] == raw[68:]
    eng.close()
    fresh, _, _ = mk(L=2, init=0.1, seed=9)
    fresh.load(str(tmp_path / "half"))                                              # scores under 0.5 without setting the option
    assert fresh.forward(fresh.batch(batch_idx), 1)["probs"].tobytes() == want.tobytes()
    fresh.load(str(tmp_path / "one"))                                               # a zero word leaves the option alone
    assert fresh.forward(fresh.batch(batch_idx), 1)["probs"].tobytes() == want.tobytes()
    fresh.close()
    mx, _, _ = mk(L=2, init=0.1, reducer=0)                                          # a Max handle reads the parameters and no temperature
    mx.load(str(tmp_path / "half"))
    mx.set_option("pool_gamma", "1")
    mx.close()


_POISON = textwrap.dedent("""
    import sys, json
    sys.path.insert(0, %r)
    import numpy as np
    from kprn_amd import _ffi, synth
    from tests.test_gpu_ragged import data, mk
    eng, _, _ = mk(L=2, init=0.5)
    eng.set_option("pool_gamma", "0.5")
    counts = np.array([3, 29, 1, 70, 28, 5, 2, 11], np.int32)
    idx, labels = data(counts, seed=42)
    b = eng.batch_ragged(idx, counts, labels)
    loss = eng.backward(b, 1)
    ex = eng.explain_batch(b, 3, 1)
    print(json.dumps({"loss": loss, "probs": eng.forward(b, 1)["probs"].astype(float).tolist(), "grads": float(np.abs(eng.get_flat_grads()).sum()),
                      "shares": ex["path_weight"].astype(float).tolist()}))
""")


def test_poisoned_allocations():
    """KPRN_POISON_ALLOC=1 fills every new device allocation with 0xFF bytes: a launch that read something it never wrote would turn NaN or differ"""
    import json
    res = {}
    for tag, env in (("plain", {}), ("poison", {"KPRN_POISON_ALLOC": "1"})):
        r = subprocess.run([sys.executable, "-c", _POISON % ROOT], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        res[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = res["plain"], res["poison"]
    assert np.isfinite(b["loss"]) and np.isfinite(b["probs"]).all() and np.isfinite(b["grads"]) and np.isfinite(b["shares"]).all()
    assert a["probs"] == b["probs"] and a["shares"] == b["shares"]
    np.testing.assert_allclose([b["loss"], b["grads"]], [a["loss"], a["grads"]], rtol=1e-5)


# ---- 8. command lines -----------------------------------------------------------------------------------------------------------------------------------
def test_train_and_recommend_command_lines(tmp_path, capsys):
    """train -kg ... -topK 2 -gamma 0.5 for two epochs; recommend without -gamma prints the scores and shares of an Engine at 0.5 over the same checkpoint
    (the checkpoint carried it), with -gamma 1 those of gamma = 1"""
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
             "-includeEntity", 1, "-paramInit", 0.5]
    flags = shape + ["-gpuid", 0, "-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-interaction_rel", "rate", "-numEpochs", 2, "-saveFrequency", 1, "-minibatch", 4,
                     "-useAdam", 1, "-topK", 2, "-negatives", 2, "-sampleSeed", 3, "-gamma", 0.5, "-model", tmp_path / "M"]
    assert train.main([str(f) for f in flags]) == 0
    lines = capsys.readouterr().out.splitlines()
    losses = [float(l.split("=")[1]) for l in lines if l.startswith("avg loss in epoch")]
    assert len(losses) == 2 and all(np.isfinite(l) and l > 0 for l in losses)
    ck = tmp_path / "M-latest"
    assert open(ck, "rb").read()[8 + 14 * 4:8 + 15 * 4] == np.float32(0.5).tobytes()
    names = ["m0", "m1", "m2", "m3", "m4"]
    (tmp_path / "items.txt").write_text("\n".join(names) + "\n")
    rflags = shape + ["-gpu_id", 0, "-top_k", 2, "-model_path", ck, "-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-user", "u0", "-items",
                      tmp_path / "items.txt", "-k", 3, "-explain_paths", 3]
    printed = {}
    for gamma in (None, 1, 0.5):
        buf = io.StringIO()
        assert recommend.main([str(f) for f in rflags + ([] if gamma is None else ["-gamma", gamma])], out=buf) == 0
        printed[gamma] = buf.getvalue()
    want = {}
    for gamma in ("0.5", "1"):
        eng = _ffi.Engine(kg.Vt, kg.Ve, kg.Vr, 16, 32, 16, 64, 2)
        eng.load(str(ck))
        eng.set_option("pool_gamma", gamma)
        res = kgraph.recommend(eng, kg, kg.entity_id("u0"), [kg.entity_id(n) for n in names], 3, 3)
        eng.close()
        out = []
        for r in res:
            out.append("%d\t%s\t%.5f\t%d\t%d" % (r["rank"], kg.entity_name(r["item"]), r["score"], r["n_paths"], r["found"]))
            out += ["%d\t%d\t%.5f\t%.6g" % (r["rank"], place, w, s) for place, (_, w, s) in enumerate(r["paths"])]
        want[gamma] = out
    strip = lambda text: [l if l.split("\t")[1].startswith("m") else "\t".join(l.split("\t")[:4]) for l in text.splitlines()]
    assert strip(printed[None]) == want["0.5"] and strip(printed[0.5]) == want["0.5"] and strip(printed[1]) == want["1"]
    assert want["0.5"] != want["1"]
