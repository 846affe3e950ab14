"""-m gpu: the pooling kernel and the loss stage (kprn_amd/csrc/loss_stage.hip), rectangular against ragged.

A rectangular batch and a ragged batch run two instantiations of one body; which one launches is the launcher's choice (a ragged batch, or a
ragged scoring pass riding as a passenger).  What the instantiations share must give the same bits, and the ragged cut's workgroup edges the
float64 oracle's numbers at the bars of tests/test_gpu_ragged.py.  Shapes: D = H = 64, Ve = 300, T = 6; one layer, except where a scoring pass has
to ride in a training step's launches, which the engine does for two layers only (option "score_dual").
"""
import functools

import numpy as np
import pytest

from kprn_amd import _ffi, synth
from tests.test_gpu_ragged import check, data, mk

pytestmark = pytest.mark.gpu

REDUCERS = [(0, 5), (1, 3), (2, 5)]   # nn.Max, TopK(3) + Mean, LogSumExp


@functools.lru_cache(maxsize=None)
def rect(B, P, seed=41):
    return synth.make_paths(B, P, 6, Ve=300, seed=seed)   # idx [B, P, T, F], labels [B]


def bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("impl", ["auto", "generic"])
@pytest.mark.parametrize("reducer,K", REDUCERS)
def test_same_cut_same_bits(reducer, K, impl):
    """The loss of a rectangular batch and of the ragged batch whose counts all equal P are the same float32: kk::ragged_plan cuts equal counts of at
    most 28 into the rectangular stage's 16-pair workgroups, both forms reduce a pair by one thread in the same order, a workgroup adds its pairs in
    index order and the partials are added in index order.  B = 1, a full workgroup, one pair more, several workgroups; P = 1 and the longest pair a
    thread takes; both BCE forms."""
    eng, _, _ = mk(L=1, reducer=reducer, K=K, impl=impl)
    for B in (1, 16, 17, 53):
        for P in (1, 28):
            idx, labels = rect(B, P)
            rb = eng.batch(idx, labels)
            gb = eng.batch_ragged(idx.reshape((-1,) + idx.shape[2:]), np.full(B, P, np.int32), labels)
            for literal in (False, True):
                l_rect = eng.backward(rb, 1, bce_literal=literal)
                l_rag = eng.backward(gb, 1, bce_literal=literal)
                print(f"B={B} P={P} literal={literal}: rectangular {l_rect!r} ragged {l_rag!r}")
                assert np.isfinite(l_rect) and bits(l_rect) == bits(l_rag), (B, P, literal, l_rect, l_rag)


EDGES = {"seventeenth_pair": ([28] * 16 + [1], 2),        # a full workgroup of 16 pairs x 28 paths, then one pair more
         "cut_by_paths": ([28] * 15 + [29], 2),           # the sixteenth pair would make 449 paths
         "single_pair_workgroups": ([449, 1, 448], 3)}    # a long pair alone, a one-path pair alone (1 + 448 > 448), a 448-path pair filling its own


@pytest.mark.parametrize("impl", ["auto", "generic"])
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_workgroup_edges_of_the_ragged_cut(edge, impl):
    counts, n_wg = EDGES[edge]
    counts = np.array(counts, np.int32)
    assert _ffi.host_ragged_plan(counts)["n_wg"] == n_wg
    eng, o64, theta = mk(L=1, impl=impl)
    idx, labels = data(counts, seed=42)
    check(eng, o64, theta, idx, counts, labels)


@pytest.mark.parametrize("train", ["rectangular", "ragged"])
@pytest.mark.parametrize("score", ["rectangular", "ragged"])
def test_a_scoring_pass_rides_in_a_training_step(score, train):
    """forward_async, a training step, read_probs with "score_overlap" 1 and "score_dual" 2: the pass rides in the training forward's launch and its
    pooling stage in the loss stage's (the profile shows no pooling launch of its own).  The probabilities are the bytes of eng.forward of the same
    batch before the step: the riding pass runs the scoring forward's own tile body on the same tiles (fused::forward_dual takes fwd_args of the
    scoring batch as fused::forward does) and the passenger is the pooling kernel's body.  The ragged pass has a pair of 70 paths, so its pooling rides
    in the wave form; a ragged participant on either side launches the segmented loss stage, none the rectangular one."""
    eng, o64, theta = mk(L=2)
    o64.zero_pad(theta)   # a training step zeroes the pad rows first (MyOptimizer.lua:181): scoring pass and step then see the same parameters
    eng.set_flat_params(theta.astype(np.float32))
    for key, value in (("score_overlap", "1"), ("score_dual", "2"), ("prefix_plan", "0")):
        eng.set_option(key, value)
    if score == "ragged":
        cs = np.concatenate([synth.draw_num_paths(np.random.default_rng(5), 37), [70]]).astype(np.int32)
        sb = eng.batch_ragged(data(cs, seed=43)[0], cs)
    else:
        sb = eng.batch(rect(40, 2, seed=44)[0])
    if train == "ragged":
        ct = np.concatenate([synth.draw_num_paths(np.random.default_rng(6), 50), [29]]).astype(np.int32)
        ti, tl = data(ct, seed=45)
        tb = eng.batch_ragged(ti, ct, tl)
    else:
        tb = eng.batch(*rect(53, 3, seed=46))
    # a parameter change between forward_async and the training forward places the queued pass ahead of it, the usual way: a new engine's first step zeroes
    # the pad rows (hence one step first), and the lazy entity update brings the training batch's rows up to date (hence the dense update)
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
        assert np.isfinite(loss)
        assert "lstm_fused_fwd_dual" in prof and "loss_stage" in prof and "pool_sigmoid" not in prof, sorted(prof)
        print(f"step {step}: max |riding - forward| = {float(np.max(np.abs(got - want))):.3e}")
        assert got.tobytes() == want.tobytes()
