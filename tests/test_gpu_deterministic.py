"""-m gpu: option "deterministic" (DESIGN.md 3.11): with it on, every float a training step hands back is a function of the inputs only.

The default fused backward joins partial sums with fp32 atomics (entity runs that straddle 64-position segments, the 16 ranges of the weight-gradient slab
reduce, the head's row, the prefix table, the small tables, the gradient norm), whose arrival order changes from launch to launch; the deterministic mode
stores those partials and adds them in a fixed order.  Every test sets the option first -- a library without it answers KPRN_E_ARG (unknown key).

"Equal" is np.array_equal on the flat parameters, both optimiser state slots, the flat gradients of a last backward, and the list of losses.  Two agreeing
runs are evidence, not proof: the lazy / dense, host-buffer / batch and disturbed / undisturbed cases compare runs whose launches or timing differ by
construction.  (That the DEFAULT mode disagrees on these inputs is measured by scripts/gpu_deterministic_probe.py, not asserted: it sometimes does not.)"""
import threading

import numpy as np
import pytest

from kprn_amd import _ffi, synth
from oracle.oracle import Oracle, make_cfg

pytestmark = pytest.mark.gpu
T = 6
VE = 50
GRAD_RTOL, LOSS_RTOL = 2e-4, 1e-5   # the bars the default mode is held to


def _engine(Ve=VE, L=2, options=(), compute_dtype=0, shape=None, **kw):
    eng = _ffi.Engine(*(shape or (6, Ve, 9, 16, 32, 16, 64, L)), compute_dtype=compute_dtype, **kw)
    eng.set_option("deterministic", "1")
    for k, v in options:
        eng.set_option(k, v)
    rng = np.random.default_rng(4)
    eng.set_flat_params((rng.random(eng.n_params) * 0.2 - 0.1).astype(np.float32))
    return eng


def _state(eng, last_batch, losses):
    """(parameters, optimiser slots, gradients of one more backward over last_batch, losses)"""
    losses = list(losses) + [eng.backward(last_batch, 1)]
    return [eng.get_flat_params(), eng.get_flat_opt_state(0), eng.get_flat_opt_state(1), eng.get_flat_grads(), np.array(losses, np.float32)]


def _assert_equal(a, b):
    for name, x, y in zip(("parameters", "optimiser slot 0", "optimiser slot 1", "gradients", "losses"), a, b):
        assert np.array_equal(x, y), (name, int(np.sum(x != y)), float(np.max(np.abs(x.astype(np.float64) - y))))
        assert np.all(np.isfinite(x)), name
    assert np.any(a[3] != 0) and np.any(a[1] != 0)   # (the comparison is not one of zeros)


@pytest.fixture(scope="module")
def hubs():
    """150 pairs x 2 paths over 50 entity rows: 300 paths, hub rows whose occurrences straddle several 64-position segments of the index"""
    idx, labels = synth.make_paths(150, 2, T, Ve=VE, seed=5)
    cnt = np.bincount(idx[..., 1].reshape(-1), minlength=VE + 1)
    assert cnt[VE] == 446                        # the pad row: a run over at least 7 segments (no plan on 16-row tiles)
    assert cnt[1:VE].max() == 289                # the most frequent real row: at least 5 segments -- three and more partials do not commute
    assert int(np.sum(cnt[1:VE] >= 129)) >= 2    # two real rows reach a third segment
    assert int(np.sum((idx[..., 1] == VE).sum(-1) == 2)) == 223   # paths with two pad steps: what the identical-prefix plan skips
    return idx, labels


def _run(idx, labels, steps, options=(), opt=None, L=2, compute_dtype=0, Ve=VE, check=None):
    eng = _engine(Ve, L, options, compute_dtype)
    opt = opt or _ffi.make_opt(method=1, lr=2e-3, regularize=1, use_grad_clip=1, grad_clip_norm=0.05, l2=1e-4)
    b = eng.batch(idx, labels)
    losses = [eng.train_step(b, opt) for _ in range(steps - 1)]
    eng.profile(True)
    losses.append(eng.train_step(b, opt))
    fam = eng.profile_get()
    eng.profile(False)
    if check:
        check(eng, b, fam)
    st = _state(eng, b, losses)
    eng.close()
    return st


def test_16_row_tiles_three_engines_agree_bit_for_bit(hubs):
    """small batch: 16-row tiles, both layers' BPTT in one launch (bwd_pipe), the small-table passenger job, clip + L2 (the norm reduction)"""
    def check(eng, b, fam):
        assert b.executed_steps == 300 * T                 # no plan on these tiles
        assert fam["lstm_fused_bwd"][1] == 1, fam         # one launch for the two layers
        assert "grad_norm" in fam and "det_join" in fam, sorted(fam)
    runs = [_run(*hubs, 12, check=check) for _ in range(3)]
    _assert_equal(runs[0], runs[1])
    _assert_equal(runs[0], runs[2])


@pytest.mark.parametrize("plan,compute_dtype", [("1", 0), ("0", 0), ("1", 2)])
def test_64_path_tiles_three_engines_agree_bit_for_bit(hubs, plan, compute_dtype):
    """5 tiles = 5 workgroups meet in the slab reduce, the head's terms and the prefix table; with the plan, without it, and on the f32x6 forward"""
    def check(eng, b, fam):
        assert (b.executed_steps < 300 * T) == (plan == "1")
        assert fam["lstm_fused_bwd"][1] == 2, fam
    opts = (("small_tiles", "0"), ("prefix_plan", plan))
    runs = [_run(*hubs, 12, opts, compute_dtype=compute_dtype, check=check) for _ in range(3)]
    _assert_equal(runs[0], runs[1])
    _assert_equal(runs[0], runs[2])


def test_tile_handover_two_engines_agree_bit_for_bit():
    """263 tiles on at most 256 workgroups: a tile changes workgroups between two of its steps, the pair's weight-gradient partials land in two slabs"""
    idx, labels = synth.make_paths(8400, 2, T, Ve=2000, seed=6)

    def check(eng, b, fam):
        assert b.handover_stats[1] >= 1, b.handover_stats
    opt = _ffi.make_opt(method=1, lr=1e-3)
    runs = [_run(idx, labels, 3, opt=opt, Ve=2000, check=check) for _ in range(2)]
    _assert_equal(runs[0], runs[1])


@pytest.mark.parametrize("method", [0, 1])
def test_one_layer_lazy_update_equals_the_dense_update_with_hubs(hubs, method):
    """L = 1 (one launch, bottom and top at once; the small tables flushed from the launch): 24 steps cycling three batches, entity rows updated lazily
    (rows coast and replay) against the dense sweep -- the bitwise statement test_gpu_parity.py can make on six distinct rows only, here with hub rows"""
    batches = [hubs] + [synth.make_paths(150, 2, T, Ve=VE, seed=50 + k) for k in range(2)]
    res = []
    for mode in (0, 1):
        eng = _engine(VE, 1)
        opt = _ffi.make_opt(method=method, lr=5e-3, entity_update=mode)
        bs = [eng.batch(i, l) for i, l in batches]
        losses = [eng.train_step(bs[k % 3], opt) for k in range(24)]
        res.append(_state(eng, bs[0], losses))
        eng.close()
    _assert_equal(res[0], res[1])


def test_host_buffer_entry_point_equals_the_batch_entry_point_bit_for_bit():
    """the sequence of test_gpu_fullsize.py (there: losses to 1e-6, parameters to 1e-7); tests/test_host_index.py pins that both feeds build the same index"""
    a, b = _engine(5000), _engine(5000)
    opt = _ffi.make_opt(method=1, lr=1e-3)
    la, lb = [], []
    for k, (pairs, Pk) in enumerate([(37, 3), (128, 2), (1, 5), (300, 1), (37, 3)]):
        idx, labels = synth.make_paths(pairs, Pk, T, Ve=5000, seed=70 + k)
        bb = b.batch(idx, labels)
        la.append(a.train_step_host(idx, labels, opt))
        lb.append(b.train_step(bb, opt))
    assert la == lb
    last = synth.make_paths(37, 3, T, Ve=5000, seed=74)
    _assert_equal(_state(a, a.batch(*last), la), _state(b, b.batch(*last), lb))
    a.close(); b.close()


def test_ragged_batch_of_equal_counts_gives_the_rectangular_gradient_bits(hubs):
    idx, labels = hubs
    res = []
    for ragged in (False, True):
        eng = _engine()
        b = eng.batch_ragged(idx.reshape(-1, T, 3), np.full(150, 2, np.int32), labels) if ragged else eng.batch(idx, labels)
        loss = eng.backward(b, 1)
        res.append((loss, eng.get_flat_grads()))
        eng.close()
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1]) and np.any(res[0][1] != 0)


def test_ragged_mixed_counts_two_engines_agree_bit_for_bit():
    idx, counts, labels = synth.make_ragged(120, T, Ve=VE, seed=9)
    assert len(np.unique(counts)) > 2
    res = []
    for _ in range(2):
        eng = _engine()
        opt = _ffi.make_opt(method=1, lr=2e-3, regularize=1, grad_clip_norm=0.05)
        b = eng.batch_ragged(idx, counts, labels)
        losses = [eng.train_step(b, opt) for _ in range(6)]
        res.append(_state(eng, b, losses))
        eng.close()
    _assert_equal(res[0], res[1])


def test_a_second_handle_scoring_on_the_device_does_not_change_the_bits(hubs):
    """one process, two handles: the 64-path-tile run while another host thread keeps the device busy with scoring passes -- workgroups start and finish in
    another order, the sums keep theirs"""
    opts = (("small_tiles", "0"),)
    quiet = _run(*hubs, 12, opts)
    other = _ffi.Engine(6, 2000, 9, 16, 32, 16, 64, 2)
    ob = other.batch(*synth.make_paths(4096, 4, T, Ve=2000, seed=8))
    stop, passes, err = threading.Event(), [0], []

    def score():
        try:
            while not stop.is_set():
                other.forward(ob, 1)
                passes[0] += 1
        except Exception as ex:   # noqa: BLE001
            err.append(ex)
    th = threading.Thread(target=score)
    th.start()
    try:
        busy = _run(*hubs, 12, opts)
    finally:
        stop.set()
        th.join()
    other.close()
    assert not err and passes[0] >= 1, (err, passes)
    _assert_equal(quiet, busy)


@pytest.mark.parametrize("case", ["generic", "rnn", "gru", "wide", "bf16"])
def test_pipelines_without_a_deterministic_form_refuse_to_train(case):
    shape = (6, 300, 9, 24, 48, 24, 96, 2) if case == "wide" else (6, 300, 9, 16, 32, 16, 64, 2)
    eng = _engine(shape=shape, rnn_type={"rnn": 1, "gru": 2}.get(case, 0), compute_dtype=1 if case == "bf16" else 0)
    if case == "generic":
        eng.set_option("impl", "generic")
    idx, labels = synth.make_paths(300, 1, T, Ve=300, seed=3)   # (300 paths: the bf16 pipeline would take them)
    b = eng.batch(idx, labels)
    opt = _ffi.make_opt(method=1, lr=1e-3)
    before = (eng.get_flat_params(), eng.get_flat_opt_state(0))
    for call in (lambda: eng.train_step(b, opt), lambda: eng.backward(b, 1), lambda: eng.train_step_host(idx, labels, opt)):
        with pytest.raises(_ffi.KprnError) as e:
            call()
        assert e.value.code == _ffi.E_UNSUPPORTED and "deterministic" in e.value.msg, e.value.msg
    assert np.array_equal(before[0], eng.get_flat_params()) and np.array_equal(before[1], eng.get_flat_opt_state(0))
    assert np.all(np.isfinite(eng.forward(b, 1)["probs"]))      # scoring is never refused
    eng.set_option("deterministic", "0")
    assert np.isfinite(eng.train_step(b, opt))                  # ... and the same handle trains again
    assert not np.array_equal(before[0], eng.get_flat_params())
    eng.close()


@pytest.mark.parametrize("small", ["1", "0"])
def test_deterministic_gradients_meet_the_default_modes_bars_against_the_f64_oracle(hubs, small):
    """a fixed order is no excuse for a looser sum: first backward of the 16-row-tile and the 64-path-tile runs against the float64 oracle"""
    idx, labels = hubs
    o64 = Oracle(make_cfg(Vt=6, Ve=VE, Vr=9, dt=16, de=32, dr=16, H=64, L=2), np.float64)
    theta32 = o64.init_params(7, 0.1).astype(np.float32)
    want_loss, want, _ = o64.forward_backward(theta32.astype(np.float64), idx, labels)
    eng = _engine(options=(("small_tiles", small),))
    eng.set_flat_params(theta32)
    loss = eng.backward(eng.batch(idx, labels), 1)
    got = eng.get_flat_grads().astype(np.float64)
    assert abs(loss - want_loss) < LOSS_RTOL * max(1.0, abs(want_loss)), (loss, want_loss)
    for nm, (off, shp) in o64.layout().items():
        n = int(np.prod(shp))
        r = float(np.max(np.abs(got[off:off + n] - want[off:off + n])) / max(1e-30, np.max(np.abs(want[off:off + n]))))
        print(f"small_tiles={small} {nm}: {r:.3e}")
        assert r < GRAD_RTOL, (nm, r)
    eng.close()
