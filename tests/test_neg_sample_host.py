"""not gpu: kprn_host_sample_negatives, the host twin of the device negative sampler (include/kprn.h "sampling negatives"), against the brute-force
restatement of tests/neg_sample_ref.py, the distribution of its picks, and its refusals.  Every comparison of ids is np.array_equal."""
import math
import subprocess

import numpy as np
import pytest

from kprn_amd import _ffi

from . import neg_sample_ref as nref
from . import path_find_ref as ref


@pytest.fixture(scope="module")
def g():
    return ref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)


def twin(g, cfg, threads=1, **kw):
    a = dict(cfg, **kw)
    return _ffi.host_sample_negatives(g["src"], g["dst"], g["rel"], g["Ve"], a["items"], a["weights"], a["users"], a["n_neg"], a["seed"], a["draw"],
                                      max_attempts=a["max_attempts"], threads=threads)


def brute(g, cfg, stats=None, **kw):
    a = dict(cfg, **kw)
    return nref.sample(g, a["items"], a["weights"], a["users"], a["n_neg"], a["max_attempts"], a["seed"], a["draw"], stats=stats)


def test_new_symbols_are_declared_and_exported():
    from kprn_amd import build as kbuild
    declared = _ffi.declared_symbols()
    syms = subprocess.check_output(["nm", "-D", kbuild.build()]).decode()
    for s in ("kprn_sampler_create", "kprn_sampler_destroy", "kprn_sample_negatives", "kprn_host_sample_negatives", "kprn_find_training_paths"):
        assert s in declared, s
        assert " T %s" % s in syms, s


def test_inputs_hold_the_cases(g):
    """from the reference alone: what the first configuration is relied on to contain"""
    cfg = nref.config_one(g)
    neg, n_found = brute(g, cfg)
    adjacent = {(int(s), int(d)) for s, d in zip(g["src"], g["dst"])}
    assert cfg["users"][0] == g["cases"]["hub"] and 0 < n_found[0] < cfg["n_neg"]          # the hub: an empty slot and a filled one
    assert cfg["users"][3] == cfg["users"][4] and not np.array_equal(neg[3], neg[4])       # the same user in two slots
    for u, row in zip(cfg["users"], neg):
        got = [int(x) for x in row if x != 0]
        assert all(x != u and (int(u), x) not in adjacent for x in got)
        assert len(set(got)) == len(got)
    assert np.array_equal(n_found, (neg != 0).sum(axis=1))


def test_twin_equals_brute_force_first_configuration(g):
    cfg = nref.config_one(g)
    want = brute(g, cfg)
    got = twin(g, cfg)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for kw in (dict(max_attempts=1), dict(max_attempts=64, n_neg=40), dict(weights=None), dict(seed=(5 << 32) | 9, draw=3)):
        want, got = brute(g, cfg, **kw), twin(g, cfg, threads=3, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kw


def test_second_configuration_runs_out_of_items(g):
    cfg = nref.config_two(g)
    assert nref.thresholds(cfg["weights"], 4) == [2 ** 30, 2 ** 30, 3 * 2 ** 30, 2 ** 32]
    stats = {}
    want = brute(g, cfg, stats=stats)
    assert stats["duplicate"] >= 1                                                         # an attempt was turned down for being on the list already
    got = twin(g, cfg)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for row in got[0]:
        assert sorted(row[:3].tolist()) == [3, 20, 41] and row[3:].tolist() == [0, 0, 0]   # item 9 (weight 0) never
    assert got[1].tolist() == [3, 3, 3]


def test_picks_follow_the_weights(g):
    """4096 single draws of the lonely user: every item's count within 6 sigma of the binomial its threshold interval gives (8 bins: a correct sampler
    fails about once in 10^8 seeds; this seed is fixed, and the brute force agrees on it -- its worst bin is the figure printed below)"""
    N = 4096
    w = np.array([1, 2, 3, 4, 0, 6, 7, 8], np.float32)
    cfg = dict(items=np.arange(1, 9, dtype=np.int32), weights=w, users=np.full(N, g["cases"]["lonely"][0], np.int32), n_neg=1, max_attempts=1, seed=11, draw=0)
    neg, n_found = twin(g, cfg, threads=4)
    want = brute(g, cfg)
    assert np.array_equal(neg, want[0]) and np.array_equal(n_found, want[1]) and (n_found == 1).all()
    thr = [0] + nref.thresholds(w, 8)
    worst = 0.0
    for j in range(8):
        p = (thr[j + 1] - thr[j]) / 2.0 ** 32
        count = int((neg == j + 1).sum())
        if w[j] == 0:
            assert p == 0 and count == 0
            continue
        sigma = math.sqrt(N * p * (1 - p))
        worst = max(worst, abs(count - N * p) / sigma)
        assert abs(count - N * p) <= 6 * sigma, (j, count, N * p, sigma)
    print("worst bin: %.2f sigma" % worst)


def test_draw_and_seed_change_the_output_and_threads_do_not(g):
    cfg = nref.config_one(g)
    base = twin(g, cfg)
    assert not np.array_equal(twin(g, cfg, draw=1)[0], base[0])
    assert not np.array_equal(twin(g, cfg, seed=8)[0], base[0])
    assert not np.array_equal(twin(g, cfg, seed=7 + (1 << 32))[0], base[0])                # the seed's high half is part of the key
    for a, b in zip(twin(g, cfg, threads=8), base):
        assert np.array_equal(a, b)


def test_refusals_write_nothing(g):
    cfg = nref.config_one(g)
    Ve = g["Ve"]

    def code(**kw):
        a = dict(cfg, **kw)
        neg = np.full((len(a["users"]), 8), -7, np.int32)
        nf = np.full(len(a["users"]), -7, np.int32)
        with pytest.raises(_ffi.KprnError) as ei:
            _ffi.host_sample_negatives(g["src"], g["dst"], g["rel"], Ve, a["items"], a["weights"], a["users"], a["n_neg"], a["seed"], a["draw"],
                                       max_attempts=a["max_attempts"], out=(neg, nf))
        assert (neg == -7).all() and (nf == -7).all(), kw
        return ei.value.code

    def weights(j, v):
        w = cfg["weights"].copy()
        w[j] = v
        return w

    swapped = cfg["items"].copy()
    swapped[[4, 5]] = swapped[[5, 4]]
    repeated = cfg["items"].copy()
    repeated[9] = repeated[8]
    for kw in (dict(items=swapped), dict(items=repeated), dict(weights=weights(3, -1.0)), dict(weights=weights(3, np.nan)), dict(weights=weights(3, np.inf)),
               dict(weights=np.zeros(380, np.float32)), dict(n_neg=0), dict(n_neg=257), dict(max_attempts=0), dict(max_attempts=65)):
        assert code(**kw) == _ffi.E_ARG, kw
    outside = cfg["items"].copy()
    outside[-1] = Ve
    for kw in (dict(users=np.array([5, 0], np.int32)), dict(users=np.array([Ve, 5], np.int32)), dict(items=outside)):
        assert code(**kw) == _ffi.E_INDEX, kw
