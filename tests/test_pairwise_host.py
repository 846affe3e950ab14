"""not gpu: kprn_host_pairwise_loss, the pairwise loss (include/kprn.h "pairwise loss") on the host cores, against its float64 restatement
(tests/pairwise_ref.py).  fp32 formula against float64 with no model in between, so the bars are the formula's own: the loss within
1e-6 max(1, |L|), dy within 1e-6 of its largest magnitude."""
import numpy as np
import pytest

from kprn_amd import _ffi
from tests.pairwise_ref import offsets, pairwise

# (sizes, labels) of the group shapes: 1 + 4, a lone positive, a lone negative, 2 positives + 3 negatives, a positive that is last, an empty group, 1024
SHAPES = [(5, [1, 0, 0, 0, 0]), (1, [1]), (1, [0]), (5, [0, 1, 0, 1, 0]), (4, [0, 0, 0, 1]), (0, []), (1024, [1] + [0] * 1020 + [1, 0, 1])]
N_TERMS = 4 + 0 + 0 + 6 + 3 + 0 + 3 * 1021


def batch(seed=7, spread=2.0):
    rng = np.random.default_rng(seed)
    go = offsets([n for n, _ in SHAPES])
    t = np.concatenate([np.asarray(l, np.float32) for _, l in SHAPES])
    y = (rng.standard_normal(len(t)) * spread + 3.0).astype(np.float32)
    return y, t, go


def compare(y, t, go, inv_batch=0.0):
    loss, dy, n = _ffi.host_pairwise_loss(y, t, go, inv_batch)
    ref = pairwise(y, t, go, inv_batch)
    le = abs(loss - ref["loss"]) / max(1.0, abs(ref["loss"]))
    de = float(np.max(np.abs(dy - ref["dy"])) / np.max(np.abs(ref["dy"])))
    print(f"loss {loss!r} ref {ref['loss']!r} err {le:.3e}; dy err {de:.3e} of max; n_terms {n}")
    assert n == ref["n_terms"]
    assert le < 1e-6, (loss, ref["loss"])
    assert de < 1e-6, de
    return loss, dy, n, ref


@pytest.mark.parametrize("seed", [7, 8, 9])
def test_every_group_shape_against_float64(seed):
    y, t, go = batch(seed)
    loss, dy, n, ref = compare(y, t, go)
    assert n == N_TERMS
    assert float(np.std(ref["theta"])) >= 0.5   # (the inputs spread theta: a wrong sigma would show)
    # pairs without a term: the lone positive, the lone negative
    assert dy[5] == 0.0 and dy[6] == 0.0 and not np.signbit(dy[5]) and not np.signbit(dy[6])
    # positives are pushed up, negatives down; a group's gradients cancel
    assert np.all(dy[t > 0.5] <= 0) and np.all(dy[t <= 0.5] >= 0)


def test_each_shape_alone():
    rng = np.random.default_rng(3)
    for size, lab in SHAPES:
        if size == 0:
            continue
        y = (rng.standard_normal(size) * 2).astype(np.float32)
        t = np.asarray(lab, np.float32)
        ref = pairwise(y, t, [0, size])
        if ref["n_terms"] == 0:
            loss, dy, n = _ffi.host_pairwise_loss(y, t, [0, size])
            assert n == 0 and loss == 0.0 and not np.any(dy)
        else:
            compare(y, t, np.array([0, size], np.int32))


def test_positions_decide_nothing():
    """positives need not come first: a permutation within the group permutes dy and keeps the loss within the bar"""
    y, t, _ = batch(11)
    y, t = y[:5].copy(), t[:5].copy()
    l0, d0, _ = _ffi.host_pairwise_loss(y, t, [0, 5])
    perm = np.array([3, 1, 4, 0, 2])
    l1, d1, _ = _ffi.host_pairwise_loss(y[perm], t[perm], [0, 5])
    assert abs(l0 - l1) < 1e-6 * max(1, abs(l0))
    np.testing.assert_allclose(d1, d0[perm], rtol=0, atol=1e-6 * float(np.max(np.abs(d0))))


@pytest.mark.parametrize("theta", [100.0, -100.0, 1e4, -1e4])
def test_extremes_stay_finite(theta):
    """theta = y_i - y_j far out: softplus(-theta) = max(-theta, 0) to one fp32 ulp (exactly 3.7e-44 more than 0 at theta = 100: anything from 0 to the
    smallest normal number is that value rounded or flushed), the gradients 0 (to the same allowance) or -s / +s exactly; no NaN anywhere"""
    tiny = float(np.finfo(np.float32).tiny)
    for s_in in (0.0, 0.25):
        y = np.array([theta, 0.0], np.float32)
        loss, dy, n = _ffi.host_pairwise_loss(y, [1, 0], [0, 2], s_in)
        s = s_in if s_in > 0 else 1.0
        assert n == 1 and np.isfinite(loss) and np.all(np.isfinite(dy))
        if theta > 0:
            assert 0.0 <= loss <= tiny and np.all(np.abs(dy) <= tiny), (loss, dy)
        else:
            want = np.float32(-theta) * np.float32(s)
            assert abs(np.float32(loss) - want) <= np.spacing(want), (loss, want)
            assert dy[0] == np.float32(-s) and dy[1] == np.float32(s), dy


def test_inv_batch_is_honoured():
    y, t, go = batch(5)
    l0, d0, n = _ffi.host_pairwise_loss(y, t, go)
    l1, d1, n1 = compare(y, t, go, inv_batch=1.0 / 64)[:3]
    assert n1 == n
    k = n / 64.0
    assert abs(l1 - l0 * k) < 2e-6 * max(1, abs(l1))
    np.testing.assert_allclose(d1, d0 * k, rtol=2e-6, atol=0)


def test_no_terms_is_no_error():
    loss, dy, n = _ffi.host_pairwise_loss([1.0, 2.0, 3.0], [1, 1, 0], [0, 2, 3, 3])
    assert n == 0 and loss == 0.0 and dy.tobytes() == np.zeros(3, np.float32).tobytes()


@pytest.mark.parametrize("go", [[0, 3, 2, 5],          # decreasing
                                [1, 3, 5],             # go[0] != 0
                                [0, 3, 4],             # go[G] != B
                                [0, 3, 6],             # go[G] != B (above)
                                [0]])                  # G = 0
def test_a_bad_table_is_refused(go):
    with pytest.raises(_ffi.KprnError) as e:
        _ffi.host_pairwise_loss(np.zeros(5, np.float32), np.zeros(5, np.float32), go)
    assert e.value.code == _ffi.E_ARG


def test_the_group_limit():
    n = _ffi.PAIRWISE_MAX_GROUP
    assert n == 1024
    y, t = np.zeros(n + 1, np.float32), np.zeros(n + 1, np.float32)
    with pytest.raises(_ffi.KprnError) as e:
        _ffi.host_pairwise_loss(y, t, [0, n + 1])
    assert e.value.code == _ffi.E_ARG
    _ffi.host_pairwise_loss(y, t, [0, n, n + 1])   # 1024 + 1: accepted


def test_null_arguments():
    L = _ffi.lib()
    import ctypes as C
    z = np.zeros(2, np.float32)
    go = np.array([0, 2], np.int32)
    loss, n = C.c_float(), C.c_int64()
    assert L.kprn_host_pairwise_loss(None, _ffi._fp(z), _ffi._fp(go), 1, 2, C.c_float(0), _ffi._fp(z.copy()), C.byref(loss), C.byref(n)) == _ffi.E_ARG
    assert L.kprn_host_pairwise_loss(_ffi._fp(z), _ffi._fp(z), _ffi._fp(go), 1, 2, C.c_float(0), None, C.byref(loss), C.byref(n)) == _ffi.E_ARG
