"""Shared by tests/test_neg_sample_host.py and tests/test_gpu_neg_sample.py: a brute-force restatement of the sampling rule of include/kprn.h ("sampling
negatives") written independently of the library -- the numpy Philox of tests/dropout_ref.py, a set of (user, item) edges instead of a CSR, thresholds from
a plain Python float loop -- and the two configurations the tests are built around."""
import math

import numpy as np

from .dropout_ref import philox4x32_10


def thresholds(weights, M):
    """thr[j] = floor(cum_j / cum_{M-1} * 2^32) as Python ints, cum a Python float (an IEEE double) summed in index order"""
    w = [1.0] * M if weights is None else [float(np.float32(x)) for x in weights]
    total = 0.0
    for x in w:
        total = total + x
    thr, cum = [], 0.0
    for x in w:
        cum = cum + x
        thr.append(int(math.floor(cum / total * 4294967296.0)))
    return thr


def words(seed, draw, B, n_neg, max_attempts):
    """[B, n_neg, max_attempts] uint32: word a % 4 of Philox(counter (a / 4, n, b, draw), key = the seed's halves)"""
    a = np.arange(max_attempts, dtype=np.uint64)[None, None, :]
    n = np.arange(n_neg, dtype=np.uint64)[None, :, None]
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    out = philox4x32_10(a // np.uint64(4), n, b, np.uint64(int(draw) & 0xFFFFFFFF), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    sel = np.broadcast_to(a % np.uint64(4), out[0].shape)
    return np.choose(sel.astype(np.int64), out)


def sample(g, items, weights, users, n_neg, max_attempts, seed, draw, stats=None):
    """-> (neg [B, n_neg], n_found [B]); stats (a dict, optional) counts the attempts rejected as the user itself / adjacent / a duplicate"""
    items = [int(x) for x in items]
    thr = np.array(thresholds(weights, len(items)), np.uint64)
    adjacent = {(int(s), int(d)) for s, d in zip(g["src"], g["dst"]) if s != d}
    B = len(users)
    w = words(seed, draw, B, n_neg, max_attempts)
    picks = np.searchsorted(thr, w.astype(np.uint64), side="right")        # the number of j with thr[j] <= r
    neg = np.zeros((B, n_neg), np.int32)
    n_found = np.zeros(B, np.int32)
    st = dict(self=0, adjacent=0, duplicate=0)
    for b, u in enumerate(int(x) for x in users):
        have = []
        for n in range(n_neg):
            for a in range(max_attempts):
                c = items[int(picks[b, n, a])]
                if c == u:
                    st["self"] += 1
                elif (u, c) in adjacent:
                    st["adjacent"] += 1
                elif c in have:
                    st["duplicate"] += 1
                else:
                    have.append(c)
                    neg[b, n] = c
                    break
        n_found[b] = len(have)
    if stats is not None:
        stats.update(st)
    return neg, n_found


def config_one(g):
    """380 weighted items; the hub (adjacent to most of them), a planted user, the lonely node, node 5 in two slots, node 17"""
    c = g["cases"]
    items = np.arange(1, 381, dtype=np.int32)
    weights = ((np.arange(380) + 10.0) ** -0.8).astype(np.float32)
    users = np.array([c["hub"], c["exact"][0], c["lonely"][0], 5, 5, 17], np.int32)
    return dict(items=items, weights=weights, users=users, n_neg=8, max_attempts=4, seed=7, draw=0)


def config_two(g):
    """four items, one of weight 0, more negatives asked for than exist: three slots of the lonely user"""
    lonely = g["cases"]["lonely"][0]
    return dict(items=np.array([3, 9, 20, 41], np.int32), weights=np.array([1, 0, 2, 1], np.float32), users=np.array([lonely] * 3, np.int32), n_neg=6,
                max_attempts=64, seed=7, draw=0)
