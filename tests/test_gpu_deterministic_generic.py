"""-m gpu: option "deterministic" = "2" (DESIGN.md 3.11): the generic fp32 pipelines -- the rnn cell, wide FastLSTM shapes, impl = generic -- train with every
float handed back a function of the inputs only, and wherever "1" trains, "2" gives "1"'s bits.

The default generic backward joins partial sums with fp32 atomics: the K splits of its weight-gradient products, the workgroups of the bias column sums, of the
head's row and of the one-hot table products, the entity runs that straddle 64-position segments, the bias sums inside the persistent BPTT launch.  Under "2" each
producer plain-stores one slab per workgroup or split and a launch behind it adds the slabs in index order.  Every test sets "2" first: a library without the
value answers KPRN_E_ARG.

Conventions of tests/test_gpu_deterministic.py: parameters from default_rng(4); "equal" is np.array_equal on the flat parameters, both optimiser slots, the flat
gradients of one more backward and the list of losses; the route is asserted through the profile's kernel families.  Shapes: rnn S (H = 100: no multiple of 64,
M = H < 256 rows -> the untiled split-K kernels) and FastLSTM W (4H = 384: the tiled kernel, two row tiles and a boundary, a 96-column block).  kprn_create takes
numLayers > 1 only with D = H (every layer is Cell(D, H), as in the reference model), so the rnn shape comes in two forms that together cover what one shape
cannot: S, two layers with D = H = 100 (de = 60), used everywhere, and S1, one layer with D = 80 != H = 100 (de = 40), added to the three-engine and oracle tests.  The batch
of 1 040 paths gives three K splits (two partials commute: they would prove nothing), 17 head workgroups, 13 one-hot product workgroups and entity rows whose
occurrences span three and more index segments."""
import threading

import numpy as np
import pytest

from kprn_amd import _ffi, synth
from oracle.oracle import Oracle, make_cfg

pytestmark = pytest.mark.gpu
T = 6
VE = 50
S = (6, VE, 9, 20, 60, 20, 100, 2)    # rnn, two layers: D = H = 100
S1 = (6, VE, 9, 20, 40, 20, 100, 1)   # rnn, one layer: D = 80 != H
W = (6, VE, 9, 24, 48, 24, 96, 2)     # FastLSTM
G64 = (6, VE, 9, 16, 32, 16, 64, 2)   # the fused path's shape
GRAD_RTOL, LOSS_RTOL = 2e-4, 1e-5     # tests/test_gpu_wide.py: the bars the default mode is held to on these pipelines


def _engine(shape, rnn_type=0, options=(), mode="2", **kw):
    eng = _ffi.Engine(*shape, rnn_type=rnn_type, **kw)
    if mode is not None:
        eng.set_option("deterministic", mode)
    for k, v in options:
        eng.set_option(k, v)
    rng = np.random.default_rng(4)
    eng.set_flat_params((rng.random(eng.n_params) * 0.2 - 0.1).astype(np.float32))
    return eng


def _state(eng, last_batch, losses):
    losses = list(losses) + [eng.backward(last_batch, 1)]
    return [eng.get_flat_params(), eng.get_flat_opt_state(0), eng.get_flat_opt_state(1), eng.get_flat_grads(), np.array(losses, np.float32)]


def _assert_equal(a, b):
    for name, x, y in zip(("parameters", "optimiser slot 0", "optimiser slot 1", "gradients", "losses"), a, b):
        assert np.array_equal(x, y), (name, int(np.sum(x != y)), float(np.max(np.abs(x.astype(np.float64) - y))))
        assert np.all(np.isfinite(x)), name
    assert np.any(a[3] != 0) and np.any(a[1] != 0)   # (the comparison is not one of zeros)


def _clip_opt(method=1):
    return _ffi.make_opt(method=method, lr=2e-3, regularize=1, use_grad_clip=1, grad_clip_norm=0.05, l2=1e-4)


def _run(shape, idx, labels, steps, rnn_type=0, options=(), opt=None, check=None, mode="2"):
    eng = _engine(shape, rnn_type, options, mode)
    opt = opt or _clip_opt()
    b = eng.batch(idx, labels)
    losses = [eng.train_step(b, opt) for _ in range(steps - 1)]
    eng.profile(True)
    losses.append(eng.train_step(b, opt))
    fam = eng.profile_get()
    eng.profile(False)
    if check:
        check(fam)
    st = _state(eng, b, losses)
    eng.close()
    return st


@pytest.fixture(scope="module")
def paths():
    """520 pairs x 2 paths over 50 entity rows: T N = 6 240 positions -> three K splits, 17 head workgroups (64 rows each), 13 one-hot product workgroups (512
    positions each); the pad row and at least two real rows occur 129 times or more: runs over three and more 64-position segments of the index"""
    idx, labels = synth.make_paths(520, 2, T, Ve=VE, seed=5)
    n = idx.shape[0] * idx.shape[1]
    assert n == 1040 and (n * T) // 2048 == 3 and (n + 63) // 64 == 17 and (n * T + 511) // 512 == 13
    cnt = np.bincount(idx[..., 1].reshape(-1), minlength=VE + 1)
    assert cnt[VE] >= 129 and int(np.sum(cnt[1:VE] >= 129)) >= 2, (cnt[VE], np.sort(cnt[1:VE])[-3:])
    return idx, labels


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("persist", ["0", "2"])
@pytest.mark.parametrize("shape", [S, S1], ids=["S", "S1"])
def test_rnn_three_engines_agree_bit_for_bit(paths, shape, persist, small):
    """rnn S, Adam with clip + L2 (the norm reduction), 6 steps: the per-step cell kernels or the persistent BPTT launch (whose bias sums go to the column sum),
    layer 0 through the small-table identity (one merged split-K product) or the scatter route (one-hot table products + the row-major entity gradient)"""
    def check(fam):
        assert ("gemm_bwd_dw_merged" in fam) == (small == "1") and ("embed_scatter" in fam) == (small == "0"), sorted(fam)
        assert "gemm_o2g_bwd_dw" in fam and "entity_grad" in fam and "grad_norm" in fam, sorted(fam)
        if persist == "2":
            assert "rnn_layer_bwd" in fam and "rnn_cell_bwd" not in fam and "bias_colsum" in fam, sorted(fam)
        else:
            assert "rnn_cell_bwd" in fam and "bias_colsum" in fam and "rnn_layer_bwd" not in fam, sorted(fam)
    opts = (("persist_layers", persist), ("small_tables", small))
    runs = [_run(shape, *paths, 6, rnn_type=1, options=opts, check=check) for _ in range(3)]
    _assert_equal(runs[0], runs[1])
    _assert_equal(runs[0], runs[2])


@pytest.mark.parametrize("persist,method", [("0", 1), ("2", 1), ("2", 0)])
def test_wide_lstm_three_engines_agree_bit_for_bit(paths, persist, method):
    """FastLSTM W: the tiled kernel's slab epilogue (M = 384: two row tiles and a boundary; a 96- and a 64-column block), Adam and Adagrad"""
    def check(fam):
        assert "gemm_o2g_bwd_dw" in fam and "gemm_bwd_dw_merged" in fam, sorted(fam)
        assert ("lstm_layer_bwd" in fam) == (persist == "2"), sorted(fam)
    runs = [_run(W, *paths, 6, options=(("persist_layers", persist),), opt=_clip_opt(method), check=check) for _ in range(3)]
    _assert_equal(runs[0], runs[1])
    _assert_equal(runs[0], runs[2])


def test_rnn_dropout_three_engines_agree_and_the_seed_matters(paths):
    """dropout 0.3 (Philox masks, a function of seed and draw): layer 0 takes the scatter route (a dropped x_t is no sum of table rows)"""
    def check(fam):
        assert "embed_scatter" in fam and "drop_rows_bwd" in fam, sorted(fam)
    opts = (("dropout", "0.3"), ("dropout_seed", "7"))
    runs = [_run(S, *paths, 6, rnn_type=1, options=opts, check=check) for _ in range(3)]
    _assert_equal(runs[0], runs[1])
    _assert_equal(runs[0], runs[2])
    other = _run(S, *paths, 6, rnn_type=1, options=(("dropout", "0.3"), ("dropout_seed", "8")))
    assert not np.array_equal(runs[0][0], other[0]) and not np.array_equal(runs[0][4], other[4])   # the noise is live


def test_impl_generic_on_the_fused_shape_three_engines_agree(paths):
    def check(fam):
        assert "gemm_o2g_bwd_dw" in fam and "head_bwd" in fam and "lstm_fused_bwd" not in fam, sorted(fam)
    runs = [_run(G64, *paths, 6, options=(("impl", "generic"),), check=check) for _ in range(3)]
    _assert_equal(runs[0], runs[1])
    _assert_equal(runs[0], runs[2])


def test_rnn_4200_paths_two_engines_agree_bit_for_bit():
    """N >= 4 096: the wave-per-row head kernel; T N = 25 200 -> twelve K splits; 66 row tiles on the forced persistent launch"""
    idx, labels = synth.make_paths(2100, 2, T, Ve=VE, seed=5)
    assert idx.shape[0] * idx.shape[1] == 4200 and (4200 * T) // 2048 == 12

    def check(fam):
        assert "rnn_layer_bwd" in fam and "head_bwd" in fam, sorted(fam)
    runs = [_run(S, idx, labels, 3, rnn_type=1, options=(("persist_layers", "2"),), check=check) for _ in range(2)]
    _assert_equal(runs[0], runs[1])


def test_a_second_handle_training_on_the_device_does_not_change_the_bits(paths):
    """one process, two handles: the run of the first test while another host thread keeps the device busy with default-mode training steps -- workgroups start
    and finish in another order, the sums keep theirs"""
    opts = (("persist_layers", "2"), ("small_tables", "0"))
    quiet = _run(S, *paths, 6, rnn_type=1, options=opts)
    other = _engine(S, 1, mode=None)
    ob = other.batch(*synth.make_paths(2048, 2, T, Ve=VE, seed=8))
    oopt = _ffi.make_opt(method=1, lr=1e-3)
    stop, steps, err = threading.Event(), [0], []

    def train():
        try:
            while not stop.is_set():
                other.train_step(ob, oopt)
                steps[0] += 1
        except Exception as ex:   # noqa: BLE001
            err.append(ex)
    th = threading.Thread(target=train)
    th.start()
    try:
        busy = _run(S, *paths, 6, rnn_type=1, options=opts)
    finally:
        stop.set()
        th.join()
    other.close()
    assert not err and steps[0] >= 1, (err, steps)
    _assert_equal(quiet, busy)


def test_host_buffer_entry_point_equals_the_batch_entry_point_bit_for_bit():
    """rnn S over minibatches of different shapes: kprn_train_step (the engine's own feed slots, host-built index) against batch + kprn_train_step_batch"""
    a, b = _engine(S, 1), _engine(S, 1)
    opt = _ffi.make_opt(method=1, lr=1e-3)
    la, lb = [], []
    for k, (pairs, Pk) in enumerate([(37, 3), (128, 2), (1, 5), (300, 1), (520, 2), (37, 3)]):
        idx, labels = synth.make_paths(pairs, Pk, T, Ve=VE, seed=70 + k)
        bb = b.batch(idx, labels)
        la.append(a.train_step_host(idx, labels, opt))
        lb.append(b.train_step(bb, opt))
    assert la == lb
    last = synth.make_paths(37, 3, T, Ve=VE, seed=75)
    _assert_equal(_state(a, a.batch(*last), la), _state(b, b.batch(*last), lb))
    a.close(); b.close()


def test_ragged_batch_two_engines_agree_bit_for_bit():
    idx, counts, labels = synth.make_ragged(400, T, Ve=VE, seed=9)
    assert len(np.unique(counts)) > 2
    res = []
    for _ in range(2):
        eng = _engine(S, 1)
        opt = _clip_opt()
        b = eng.batch_ragged(idx, counts, labels)
        losses = [eng.train_step(b, opt) for _ in range(4)]
        res.append(_state(eng, b, losses))
        eng.close()
    _assert_equal(res[0], res[1])


def test_mode_2_gives_mode_1s_bits_on_the_fused_path():
    """everything "1" covers runs under "2" exactly as under "1": tests/test_gpu_deterministic.py's default shape and its hubs batch, 12 steps"""
    idx, labels = synth.make_paths(150, 2, T, Ve=VE, seed=5)

    def check(fam):
        assert "lstm_fused_bwd" in fam and "det_join" in fam and "head_bwd" not in fam, sorted(fam)
    one = _run(G64, idx, labels, 12, mode="1", check=check)
    two = _run(G64, idx, labels, 12, mode="2", check=check)
    _assert_equal(one, two)


@pytest.fixture(scope="module")
def oracle_grads(paths):
    """float64 loss and gradients of S, S1 and W on the module's batch, computed once"""
    idx, labels = paths
    res = {}
    for name, shape, rt in (("S", S, 1), ("S1", S1, 1), ("W", W, 0)):
        Vt, Ve, Vr, dt, de, dr, H, L = shape
        o64 = Oracle(make_cfg(Vt=Vt, Ve=Ve, Vr=Vr, dt=dt, de=de, dr=dr, H=H, L=L, rnn_type=rt, use_relu=1), np.float64)
        theta = o64.init_params(7, 0.08).astype(np.float32).astype(np.float64)
        if rt:
            o64.zero_pad(theta)   # zero pad embeddings -> MaskZero masks the pad steps
        loss, grads, _ = o64.forward_backward(theta, idx, labels)
        res[name] = (theta.astype(np.float32), loss, grads, o64.layout())
    return res


@pytest.mark.parametrize("name,small,persist", [("S", "1", "0"), ("S", "0", "2"), ("S1", "1", "0"), ("S1", "0", "2"), ("W", "1", "0"),
                                                ("W", "0", "2")])
def test_deterministic_gradients_meet_the_default_modes_bars_against_the_f64_oracle(paths, oracle_grads, name, small, persist):
    """a fixed order is no excuse for a looser sum: one backward under "2" against the float64 oracle, at tests/test_gpu_wide.py's bars and normalisation (loss to
    1e-5, every gradient tensor within 2e-4 of its largest entry)"""
    idx, labels = paths
    theta32, want_loss, want, layout = oracle_grads[name]
    eng = _engine({"S": S, "S1": S1, "W": W}[name], 0 if name == "W" else 1, (("small_tables", small), ("persist_layers", persist)))
    eng.set_flat_params(theta32)
    loss = eng.backward(eng.batch(idx, labels), 1)
    got = eng.get_flat_grads().astype(np.float64)
    assert abs(loss - want_loss) < LOSS_RTOL * max(1.0, abs(want_loss)), (loss, want_loss)
    for nm, (off, shp) in layout.items():
        n = int(np.prod(shp))
        r = float(np.max(np.abs(got[off:off + n] - want[off:off + n])) / max(1e-30, np.max(np.abs(want[off:off + n]))))
        print(f"{name} small_tables={small} persist_layers={persist} {nm}: {r:.3e}")
        assert r < GRAD_RTOL, (nm, r)
    eng.close()


@pytest.mark.parametrize("case", ["gru", "bf16"])
def test_pipelines_without_a_deterministic_form_still_refuse_to_train(case):
    eng = _engine((6, 300, 9, 16, 32, 16, 64, 2), rnn_type=2 if case == "gru" else 0, compute_dtype=1 if case == "bf16" else 0)
    idx, labels = synth.make_paths(300, 1, T, Ve=300, seed=3)   # (300 paths: the bf16 pipeline would take them)
    b = eng.batch(idx, labels)
    opt = _ffi.make_opt(method=1, lr=1e-3)
    before = (eng.get_flat_params(), eng.get_flat_opt_state(0), eng.get_flat_opt_state(1))
    for call in (lambda: eng.train_step(b, opt), lambda: eng.backward(b, 1), lambda: eng.train_step_host(idx, labels, opt)):
        with pytest.raises(_ffi.KprnError) as e:
            call()
        assert e.value.code == _ffi.E_UNSUPPORTED and "deterministic" in e.value.msg, e.value.msg
    assert np.array_equal(before[0], eng.get_flat_params())
    assert np.array_equal(before[1], eng.get_flat_opt_state(0)) and np.array_equal(before[2], eng.get_flat_opt_state(1))
    assert np.all(np.isfinite(eng.forward(b, 1)["probs"]))      # scoring is never refused
    for bad in ("3", "x"):
        with pytest.raises(_ffi.KprnError) as e:
            eng.set_option("deterministic", bad)
        assert e.value.code == _ffi.E_ARG, (bad, e.value.msg)
    with pytest.raises(_ffi.KprnError):
        eng.backward(b, 1)                                      # (a refused value changes nothing: still "2")
    eng.set_option("deterministic", "0")
    assert np.isfinite(eng.train_step(b, opt))                  # ... and the same handle trains again
    assert not np.array_equal(before[0], eng.get_flat_params())
    eng.close()
