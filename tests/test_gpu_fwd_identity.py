"""-m gpu: the small-table identity on the fused D = H = 64 FORWARD (kprn_amd/csrc/lstm_fused_fwd.hip fwd_body IDENT).

With x = [Wt[type] | We[entity] | Wr[relation]] (net/FeatureEmbedding.lua:112-121), layer 0's input half W_i2g x (model/OneModel.lua:268-274, nn.FastLSTM i2g)
is computed as [S | x_e] [Q ; W_i2g[:, e cols]^T]: S the one-hot columns of (relation, type), Q = table W_i2g[:, its cols]^T formed in the launch's prologue.
Option "small_tables_fwd" = 0 keeps the full-row kernels in-process.  What must hold, on one seeded engine shape:
  * route on vs off: path scores, probabilities, loss and every gradient within 2e-5 of the tensor's largest element -- the same sums in another order
    (the bar between two implementations of the same sums: tests/test_gpu_fullsize.py, tests/test_gpu_fused_identity.py; expected from the fp32 restatement
    in tests/test_fwd_identity_algebra.py: ~4e-7);
  * every launch form takes the same route: two passes over one batch, the pass inside the training forward's launch against the side-stream pass, a ragged
    batch of equal counts against the rectangular one -- bit-identical with the route on;
  * de != 32 and compute_dtype 2 do not take the route: bit-identical with the option on and off;
  * saturated gates (the bias bands of tests/test_gpu_gate_extremes.py, R1) through the route: finite, within that test's bars of the float64 oracle;
  * 20 Adam steps with clipping and L2 agree in the parameters.
The route is asserted through the profiler: a launch on the route leaves the (empty) family "small_tables_fwd" behind.
Every case prints its measured maxima ("MARGINS {...}").

Measured maxima (MI355X, profiles/r08/README.md), route on against off: path scores 6.1e-7 of the largest, probabilities 1.5e-7, loss 6e-8, gradients 1.03e-6
of each tensor's largest (19 200 x 1 paths; the other shapes 4.4e-7 .. 6.2e-7); saturated gates 3.1e-7 (scores) / 2.8e-7 (gradients) against the oracle and
8.2e-8 / 1.4e-7 against the full-row kernels; after 20 Adam steps parameters 3.1e-7, losses 1.2e-7."""
import json

import numpy as np
import pytest

from kprn_amd import _ffi, synth

pytestmark = pytest.mark.gpu
T = 6
ROUTE_FAMILY = "small_tables_fwd"


def mk(fwd_ident, plan=True, handover=2, dims=(16, 32, 16), Ve=30000, small_tiles="0", compute_dtype=0):
    eng = _ffi.Engine(6, Ve, 9, dims[0], dims[1], dims[2], 64, 2, compute_dtype=compute_dtype)
    eng.set_option("small_tiles", small_tiles)
    eng.set_option("prefix_plan", "1" if plan else "0")
    eng.set_option("tile_handover", str(handover))
    eng.set_option("small_tables_fwd", str(fwd_ident))
    rng = np.random.default_rng(5)
    eng.set_flat_params((rng.random(eng.n_params) * 0.2 - 0.1).astype(np.float32))
    return eng


def rel_inf(a, c):
    a, c = np.asarray(a, np.float64), np.asarray(c, np.float64)
    return float(np.max(np.abs(a - c))) / max(1e-30, float(np.max(np.abs(c))))


# (pairs, P, plan, hand-over, small tiles, dims, route taken): the case table of tests/test_gpu_fused_identity.py; the forward's route does not depend
# on the tile size, so the 16-row tiles take it too
CASES = [(65536 // 4, 4, True, 2, "0", (16, 32, 16), True),
         (65536 // 4, 4, False, 0, "0", (16, 32, 16), True),
         (4000, 4, True, 1, "0", (16, 32, 16), True),
         (19200, 1, False, 2, "0", (16, 32, 16), True),
         (300, 4, False, 0, "0", (16, 32, 16), True),
         (60, 4, True, 2, "1", (16, 32, 16), True),
         (4000, 4, True, 2, "0", (16, 16, 32), False)]


@pytest.mark.parametrize("pairs,P,plan,handover,small,dims,route", CASES)
def test_identity_forward_equals_full_row_forward(pairs, P, plan, handover, small, dims, route):
    idx, labels = synth.make_paths(pairs, P, T, Ve=30000, seed=pairs % 997 + P)
    res = []
    for on in (1, 0):
        eng = mk(on, plan, handover, dims, small_tiles=small)
        b = eng.batch(idx, labels)
        eng.profile(True)
        out = eng.forward(b, 1, want=("path_scores", "probs"))
        loss = eng.backward(b, 1)
        fam = eng.profile_get()
        assert any(k.startswith("lstm_fused_fwd") for k in fam), sorted(fam)
        assert (ROUTE_FAMILY in fam) == (route and on == 1), sorted(fam)
        res.append((out["path_scores"].copy(), out["probs"].copy(), loss, eng.get_flat_grads().astype(np.float64), eng.layout()))
        eng.close()
    (s1, p1, l1, g1, lay), (s0, p0, l0, g0, _) = res
    margins = {"scores": rel_inf(s1, s0), "probs": rel_inf(p1, p0), "loss": abs(l1 - l0) / max(1.0, abs(l0))}
    grads = {}
    seen = 0
    for nm, (off, shp) in lay.items():
        n = int(np.prod(shp))
        grads[nm] = rel_inf(g1[off:off + n], g0[off:off + n])
        seen += float(np.max(np.abs(g0[off:off + n]))) > 0
    margins["grad"] = max(grads.values())
    print("MARGINS " + json.dumps({"case": [pairs, P, plan, handover, small, list(dims)], **margins}))
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(g1))
    if not route:   # the route is not taken: the same kernels
        assert np.array_equal(s1, s0) and np.array_equal(p1, p0)
    assert margins["scores"] < 2e-5 and margins["probs"] < 2e-5 and margins["loss"] < 2e-5, margins
    for nm, v in grads.items():
        assert v < 2e-5, (nm, v)
    assert seen >= 8


@pytest.mark.parametrize("pairs,P,small", [(3000, 4, "0"), (60, 4, "1"), (20000, 1, "0")])
def test_every_launch_form_takes_the_route_bit_for_bit(pairs, P, small):
    """route on: a second pass over the batch, the pass as a branch of the training forward's launch (k_lstm_fwd_dual) against the side-stream pass
    (k_lstm_fwd), a ragged batch of equal counts against the rectangular one"""
    idx, labels = synth.make_paths(pairs, P, T, Ve=30000, seed=21 + P)
    first = []
    for dual in ("1", "0"):
        eng = mk(1, small_tiles=small)
        eng.set_option("score_overlap", "1")
        eng.set_option("score_dual", dual)
        b = eng.batch(idx, labels)
        opt = _ffi.make_opt(method=1, lr=0.0)   # (steps that leave the parameters where they are: every pass below is comparable bit for bit)
        eng.train_step(b, opt)                  # (a new engine's first step zeroes the pad rows first: a queued pass would run ahead of it, the usual way)
        eng.profile(True)
        probs = []
        for _ in range(2):
            eng.forward_async(b, 1)
            eng.train_step(b, opt)
            probs.append(eng.read_probs(b.B).copy())
        assert np.array_equal(probs[0], probs[1])
        first.append(probs[0])
        fam = eng.profile_get()
        assert ("lstm_fused_fwd_dual" in fam) == (dual == "1"), sorted(fam)
        assert ROUTE_FAMILY in fam, sorted(fam)
        eng.close()
    assert np.array_equal(first[0], first[1])
    eng = mk(1, small_tiles=small)
    want = ("probs", "pooled", "path_scores")
    b = eng.batch(idx, labels)
    one = {k: v.copy() for k, v in eng.forward(b, 1, want=want).items()}
    two = eng.forward(b, 1, want=want)
    rb = eng.batch_ragged(idx.reshape((-1,) + idx.shape[2:]), np.full(pairs, P, np.int32), labels)
    eng.profile(True)
    rag = eng.forward(rb, 1, want=want)
    assert ROUTE_FAMILY in eng.profile_get()
    for k in want:
        assert np.array_equal(one[k], two[k]), k
        assert np.array_equal(one[k], rag[k]), k
    eng.close()


@pytest.mark.parametrize("dims,compute_dtype", [((16, 16, 32), 0), ((16, 32, 16), 2)])
def test_shapes_outside_the_route_ignore_the_option(dims, compute_dtype):
    idx, labels = synth.make_paths(2000, 4, T, Ve=30000, seed=9)
    res = []
    for on in (1, 0):
        eng = mk(on, dims=dims, compute_dtype=compute_dtype)
        b = eng.batch(idx, labels)
        eng.profile(True)
        out = eng.forward(b, 1, want=("path_scores", "probs"))
        assert ROUTE_FAMILY not in eng.profile_get()
        res.append((out["path_scores"].copy(), out["probs"].copy()))
        eng.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_saturated_gates_through_the_route():
    """R1 of tests/test_gpu_gate_extremes.py (bias ladders over [-130, -92] and [+92, +130] in every gate block) on the fused two-layer shape: with the route
    on, finite and within that test's fp32 bars of the float64 oracle (scores 2e-5 of the largest, probabilities rtol 1e-4, loss 1e-5, gradients 2e-4 of each
    tensor's largest); and within 2e-5 of the full-row kernels"""
    from tests.test_gpu_gate_extremes import _case
    eng, o64, theta, idx, labels, info, _, _ = _case("fused64_plan_L2", "R1")
    ps, _, probs = o64.forward(theta, idx)
    ol, og, _ = o64.forward_backward(theta, idx, labels)
    b = eng.batch(idx, labels)
    res = []
    for on in ("1", "0"):
        eng.set_option("small_tables_fwd", on)
        eng.profile_reset()
        eng.profile(True)
        out = eng.forward(b, 1, want=("path_scores", "all_probs"))
        loss = eng.backward(b, 1)
        assert (ROUTE_FAMILY in eng.profile_get()) == (on == "1")
        eng.profile(False)
        res.append((out["path_scores"].copy(), out["all_probs"].copy(), loss, eng.get_flat_grads().astype(np.float64)))
    lay = eng.layout()
    eng.close()
    (s1, p1, l1, g1), (s0, p0, l0, g0) = res
    grad_o = max(rel_inf(g1[off:off + int(np.prod(shp))], og[off:off + int(np.prod(shp))]) for off, shp in lay.values())
    grad_ab = max(rel_inf(g1[off:off + int(np.prod(shp))], g0[off:off + int(np.prod(shp))]) for off, shp in lay.values())
    info.update(score=rel_inf(s1, ps), loss=abs(l1 - ol) / max(1.0, abs(ol)), grad=grad_o, score_ab=rel_inf(s1, s0), grad_ab=grad_ab)
    print("MARGINS " + json.dumps(info))
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(p1)) and np.isfinite(l1) and np.all(np.isfinite(g1)), info
    assert info["score"] < 2e-5, info
    np.testing.assert_allclose(p1, probs, rtol=1e-4)
    assert info["loss"] < 1e-5, info
    assert info["grad"] < 2e-4, info
    assert info["score_ab"] < 2e-5 and info["grad_ab"] < 2e-5 and abs(l1 - l0) < 2e-5 * max(1.0, abs(l0)), info


def test_identity_forward_adam_steps_with_clip_and_l2():
    batches = [synth.make_paths(4000, 4, T, Ve=30000, seed=71 + i) for i in range(2)]
    res = []
    for on in (1, 0):
        eng = mk(on)
        opt = _ffi.make_opt(method=1, lr=1e-3, use_grad_clip=1, grad_clip_norm=0.5, l2=1e-3)
        bs = [eng.batch(i, l) for i, l in batches]
        losses = [eng.train_step(bs[k % 2], opt) for k in range(20)]
        res.append((eng.get_flat_params().astype(np.float64), losses))
        eng.close()
    (w1, l1), (w0, l0) = res
    margins = {"params": rel_inf(w1, w0), "loss": float(np.max(np.abs(np.asarray(l1) - np.asarray(l0)))) / max(1.0, float(np.max(np.abs(l0))))}
    print("MARGINS " + json.dumps(margins))
    assert margins["loss"] < 1e-4
    assert margins["params"] < 2e-5
