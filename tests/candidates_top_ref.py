"""Shared by tests/test_candidates_top_host.py and tests/test_gpu_candidates_top.py: graph D and a reference for include/kprn.h "the N strongest candidates
of a user" that holds nothing of the code under test: n_paths is `found` of the finder's host twin (_ffi.host_find_paths, itself held to
path_find_ref.brute_paths) over every (user, member) pair, the exclusions come from the raw edge list, the order from np.lexsort."""
import numpy as np

from kprn_amd import _ffi

from . import path_find_ref as ref

CAP_MAX = 2**31 - 1


def graph_d():
    """users 1..24 rate 30 of the items 25..324 each, drawn without replacement with weight (rank + 5)^-0.8, every rating with its inverse and one in eight
    under a second relation as well; hub user 325 rates items 25..84; twenty fan users 326..345 rate each of those 60 items and the target item 346.
    Ve = 348, 4158 input edges.  catalogue = items 25..324 and 346 (M = 301: one entry more than a 256-entry chunk); users = 1..24, the hub, one fan.
    hub -> target has 60 * 20 = 1200 paths of 3 hops: more than one 8-bit digit -> (g, items, users)"""
    rng = np.random.RandomState(53)
    w = (np.arange(300) + 5.0) ** -0.8
    w /= w.sum()
    E = []
    for u in range(1, 25):
        for i in rng.choice(300, size=30, replace=False, p=w):
            i = 25 + int(i)
            E += [(u, i, 1), (i, u, 2)]
            if rng.randint(8) == 0:
                E += [(u, i, 3), (i, u, 4)]
    hub, target = 325, 346
    first60 = list(range(25, 85))
    for i in first60:
        E += [(hub, i, 1), (i, hub, 2)]
    for f in range(326, 346):
        for i in first60 + [target]:
            E += [(f, i, 1), (i, f, 2)]
    E = np.array(E, np.int32)
    g = dict(src=E[:, 0].copy(), dst=E[:, 1].copy(), rel=E[:, 2].copy(), Ve=348, n_rand=0, seed=53, cases=dict(hub=hub, target=target))
    items = np.array(list(range(25, 325)) + [target], np.int32)
    users = np.array(list(range(1, 25)) + [hub, 326], np.int32)
    return g, items, users


def path_counts(g, items, users, lo, hi):
    """n_paths [B, M] int64: `found` of the finder's host twin for every (user, member) pair, whatever the exclusions"""
    users, items = np.asarray(users, np.int32).reshape(-1), np.asarray(items, np.int32).reshape(-1)
    pairs = np.stack([np.repeat(users, len(items)), np.tile(items, len(users))], axis=1).astype(np.int32)
    _, _, found = _ffi.host_find_paths(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, 1, hi + 1, threads=8,
                                       want_idx=False)
    return found.astype(np.int64).reshape(len(users), len(items))


def counts_after_exclusions(g, items, users, n_paths, exclude):
    """n_paths with the entries of the user itself and -- exclude -- of the members it has an input edge to set to 0: what is left above 0 are the candidates"""
    out = n_paths.copy()
    for b, u in enumerate(users):
        gone = (items == u)
        if exclude:
            gone |= np.isin(items, g["dst"][(g["src"] == u) & (g["dst"] != u)])
        out[b, gone] = 0
    return out


def keep(items, counts, cap):
    """one user's counts [M] (0 = no candidate) -> (kept ids ascending, their n_paths): the first cap by (n_paths descending, id ascending), re-sorted by id"""
    at = np.nonzero(counts)[0]
    order = at[np.lexsort((items[at], -counts[at]))][:cap]
    order = order[np.argsort(items[order])]
    return items[order], counts[order]


def reference(g, items, users, n_paths, exclude, cap):
    """-> (cand [sum], group_counts [B], n_paths [sum]) as the twin returns them; n_paths [B, M] = path_counts(...) of the same hops"""
    counts = counts_after_exclusions(g, items, users, n_paths, exclude)
    per = [keep(items, counts[b], cap) for b in range(len(users))]
    cand = np.concatenate([p[0] for p in per]).astype(np.int32) if per else np.zeros(0, np.int32)
    return cand, np.array([len(p[0]) for p in per], np.int32), np.concatenate([p[1] for p in per]).astype(np.int64)
