"""Shared by tests/test_select_hardest_host.py and tests/test_gpu_hard_negatives.py: a numpy restatement of the selection rule (include/kprn.h "hard
negatives") that uses nothing of the code under test, and the group set both files run."""
import numpy as np


def select(scores, group_offsets, n_keep, members=None, pos=None):
    """-> (keep uint8 [group_offsets[G]], n_invalid): per group a stable argsort on the negated score (NaN after every number, -0 == +0, the lower index first
    among equals), the positive removed, the first n_keep kept, and the positive itself"""
    sc = np.asarray(scores, np.float32)
    goff = np.asarray(group_offsets, np.int64)
    keep = np.zeros(int(goff[-1]), np.uint8)
    n_invalid = 0
    for g in range(len(goff) - 1):
        o, e = int(goff[g]), int(goff[g + 1])
        lines = np.arange(o, e) if members is None else np.asarray(members, np.int64)[o:e]
        s = sc[lines].astype(np.float64)
        p = -1 if pos is None else int(pos[g])
        nan = np.isnan(s)
        order = np.lexsort((np.arange(e - o), np.where(nan, 0.0, -s), nan))   # (last key first: validity, then the negated score, then the index)
        order = order[order != p]
        keep[o + order[:n_keep]] = 1
        if p >= 0:
            keep[o + p] = 1
        n_invalid += int(nan.sum()) - (1 if p >= 0 and nan[p] else 0)
    return keep, n_invalid


SIZES = (1, 2, 64, 65, 256, 257, 4096)


def group_set(seed=5):
    """-> (scores [n] float32, group_offsets [G + 1] int64, pos [G] int32): every size of SIZES with pos -1, 0, last and middle on random scores with ties, then
    the special groups -- all scores equal, signed zeros, infinities, NaN among the negatives, NaN as the positive, an all-NaN group -- in both size classes"""
    rng = np.random.RandomState(seed)
    sc, goff, pos = [], [0], []

    def add(s, p):
        sc.append(np.asarray(s, np.float32)); goff.append(goff[-1] + len(s)); pos.append(p)

    for n in SIZES:
        for p in sorted({-1, 0, n - 1, n // 2}):
            add(np.round(rng.rand(n), 2 if n > 64 else 6), p)          # (two decimals: about a hundred distinct values, ties everywhere in a long group)
    for n in (5, 70, 300, 1000):
        add(np.full(n, 0.25), n // 2)                                   # all equal: the lowest indices win
        add(np.full(n, 0.25), -1)
        z = np.where(rng.rand(n) < 0.5, -0.0, 0.0); z[rng.randint(n)] = -1e-30
        add(z, 1)                                                       # -0 and +0 are one value
        s = rng.randn(n); s[rng.rand(n) < 0.3] = np.inf; s[rng.rand(n) < 0.3] = -np.inf
        add(s, n - 1)
        s = rng.rand(n); s[rng.rand(n) < 0.4] = np.nan
        add(s, 0 if not np.isnan(s[0]) else -1)                         # NaN among the negatives
        s = rng.rand(n); s[rng.rand(n) < 0.2] = -np.inf; s[2] = np.nan
        add(s, 2)                                                       # NaN as the positive; -inf stays above NaN
        add(np.full(n, np.nan), 3)
    return np.concatenate(sc), np.array(goff, np.int64), np.array(pos, np.int32)
