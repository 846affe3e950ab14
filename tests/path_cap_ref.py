"""Shared by tests/test_path_cap_host.py and tests/test_gpu_path_cap.py: a brute-force restatement of the cap mode "spread" (include/kprn.h "finding a pair's
paths", cap mode) in Python's own integers, with the Philox of tests/path_walk_ref.py.  The kept rows are taken out of the UNCAPPED list that
path_walk_ref.brute_find returns at a cap of 4096 (every pair of the inputs has fewer paths than that), at the kept ranks."""
import numpy as np

from . import path_walk_ref as wr

CAP_COUNTER = 131072
ALL = 4096   # the cap under which brute_find keeps every path of the inputs


def bounds(F, K):
    """lo_0 .. lo_K of the K strata of [0, F)"""
    return [j * F // K for j in range(K + 1)]


def stratum_of(r, F, K):
    return ((r + 1) * K - 1) // F


def select(F, K, b, seed, draw):
    """the kept ranks of the pair in row b: min(F, K) of them, ascending"""
    if F <= K:
        return list(range(F))
    lo = bounds(F, K)
    key = (seed & wr.M32, (seed >> 32) & wr.M32)
    out = []
    for j in range(K):
        w = wr.philox4x32_10((j // 2, CAP_COUNTER, b, draw & wr.M32), key)
        x = (w[2 * (j % 2)] << 32) | w[2 * (j % 2) + 1]
        out.append(lo[j] + ((x * (lo[j + 1] - lo[j])) >> 64))
    return out


def brute_find(g, nt, pairs, min_hops, max_hops, max_paths, T, F, walks, seed, draw, memo=None, full=None):
    """-> (idx [N,T,F], counts [B], found [B]) under "spread".  full (a dict): the uncapped results, kept per (hops, layout, walks, seed, draw)"""
    key = (pairs.tobytes(), min_hops, max_hops, T, F, nt.shape[1], walks, seed, draw)
    if full is None or key not in full:
        res = wr.brute_find(g, nt, pairs, min_hops, max_hops, ALL, T, F, walks, seed, draw, memo)
        assert res[2].max() <= ALL
        if full is not None:
            full[key] = res
    else:
        res = full[key]
    idx, _, found = res
    off = np.concatenate([[0], np.cumsum(found)])
    take = [off[b] + r for b in range(len(pairs)) for r in select(int(found[b]), max_paths, b, seed, draw)]
    return idx[np.array(take, np.int64)] if take else np.zeros((0, T, F), np.int32), np.minimum(found, max_paths).astype(np.int32), found
