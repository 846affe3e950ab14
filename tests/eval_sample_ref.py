"""The yardstick of the sampled-evaluation tests: the rule of include/kprn.h "sampled evaluation groups" restated in numpy and Python integers, without any
of the engine's code.  The Philox4x32-10 is tests/dropout_ref.py's; a sample is the n_neg smallest keys of D found by SORTING them."""
import numpy as np

from .dropout_ref import philox4x32_10


def keys(seed, draw, u, i, cs):
    """key(u, i, c) for every c of cs: Python ints (word 0 of Philox with key (seed low, seed high), counter (c, i, u, draw)) << 32 | c"""
    cs = np.asarray(cs, np.int64)
    if len(cs) == 0:
        return []
    w0 = philox4x32_10(cs, int(i), int(u), int(draw) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)[0]
    return [(int(w) << 32) | int(c) for w, c in zip(w0, cs)]


def reference(pairs, group_counts, target_offsets, target_items, n_neg, seed, draw=0):
    """-> dict(pairs [new_total, 2], group_counts [B], target_rows [NT], neg_rows [NT, n_neg], n_drawn [NT]) as the twin returns them"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    B, NT = len(group_counts), len(target_items)
    starts = np.concatenate([[0], np.cumsum(group_counts)]).astype(np.int64)
    kept = set()
    trow, negs = [-1] * NT, [[] for _ in range(NT)]
    for b in range(B):
        rows = list(range(int(starts[b]), int(starts[b + 1])))
        H = [int(x) for x in target_items[int(target_offsets[b]):int(target_offsets[b + 1])]]
        D = [r for r in rows if int(pairs[r, 1]) not in H]
        for k in range(int(target_offsets[b]), int(target_offsets[b + 1])):
            i = int(target_items[k])
            mine = [r for r in rows if int(pairs[r, 1]) == i]
            if not mine:
                continue
            u = int(pairs[mine[0], 0])
            trow[k] = mine[0]
            ky = keys(seed, draw, u, i, [int(pairs[r, 1]) for r in D])
            order = sorted(range(len(D)), key=lambda q: ky[q])
            negs[k] = sorted(D[q] for q in order[:n_neg])
            kept.update(negs[k] + mine[:1])
    new_of = {r: at for at, r in enumerate(sorted(kept))}
    out = dict(pairs=pairs[sorted(kept)].astype(np.int32).reshape(-1, 2),
               group_counts=np.array([sum(1 for r in kept if starts[b] <= r < starts[b + 1]) for b in range(B)], np.int32),
               target_rows=np.array([new_of[r] if r >= 0 else -1 for r in trow], np.int32),
               neg_rows=np.full((NT, n_neg), -1, np.int32), n_drawn=np.array([len(x) for x in negs], np.int32))
    for k, x in enumerate(negs):
        out["neg_rows"][k, :len(x)] = [new_of[r] for r in x]
    return out


NAMES = ("pairs", "group_counts", "target_rows", "neg_rows", "n_drawn")


def same(a, b):
    return all(np.array_equal(a[n], b[n]) and a[n].shape == b[n].shape for n in NAMES)
