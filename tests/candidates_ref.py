"""Shared by tests/test_candidates_host.py and tests/test_gpu_candidates.py: the three graphs of the candidate tests and a brute force written from the
definition (include/kprn.h "candidates of a user"): a catalogue member is a candidate when path_find_ref.brute_paths finds a path to it."""
import numpy as np

from . import path_find_ref as ref

HOPS = ((1, 3), (2, 3), (1, 1), (2, 2), (3, 3))


def _path_hops(g, u, c):
    """the hop counts of the paths brute_paths finds from u to c within 1..3 hops (one search per pair, shared by every hop range and both `exclude`)"""
    memo = g.setdefault("_memo", {})               # (kept in the graph's own dict: it lives and dies with the graph)
    if (u, c) not in memo:
        memo[u, c] = frozenset(len(rels) for _, rels in ref.brute_paths(_near(g, u), u, c, 1, 3))
    return memo[u, c]


def _near(g, u):
    """the edges a path of at most 3 hops out of u can use: those whose source is u or at most 2 edges away from it (brute_paths sorts the edge list it is
    given on every call; the whole graph per (user, item) pair would take a minute)"""
    memo = g.setdefault("_memo", {})
    if (u, None) not in memo:
        reach = np.array([u])
        for _ in range(2):
            reach = np.union1d(reach, g["dst"][np.isin(g["src"], reach)])
        m = np.isin(g["src"], reach)
        memo[u, None] = dict(src=g["src"][m], dst=g["dst"][m], rel=g["rel"][m])
    return memo[u, None]


def brute_candidates(g, items, u, lo, hi, exclude):
    """the members c of `items` (ascending) with a path u -> c of lo .. hi hops, c != u, and -- exclude -- no stored edge u -> c"""
    u = int(u)
    adjacent = {int(d) for s, d in zip(g["src"], g["dst"]) if int(s) == u and s != d}
    out = []
    for c in items:
        c = int(c)
        if c == u or (exclude and c in adjacent):
            continue
        if any(lo <= h <= hi for h in _path_hops(g, u, c)):
            out.append(c)
    return out


def brute_all(g, items, users, lo, hi, exclude):
    """-> (cand [sum], group_counts [B]) as the twin returns them"""
    per = [brute_candidates(g, items, int(u), lo, hi, exclude) for u in users]
    flat = [c for p in per for c in p]
    return np.array(flat, np.int32).reshape(-1), np.array([len(p) for p in per], np.int32)


def graph_a():
    """the finder's test graph (Ve = 402, 1381 stored edges); catalogue = the ids not divisible by 3 (268 items: 8 full words and 12 bits);
    users = every planted user and 20 random nodes -> (g, items, users)"""
    g = ref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)
    items = np.array([e for e in range(1, g["Ve"]) if e % 3], np.int32)
    planted = []
    for v in g["cases"].values():
        u = v[0] if isinstance(v, tuple) else v
        if u not in planted:
            planted.append(int(u))
    rng = np.random.RandomState(31)
    users = np.array(planted + [int(x) for x in rng.randint(1, g["n_rand"] + 1, size=20)], np.int32)
    return g, items, users


def graph_b():
    """a dozen planted nodes above a small random graph, catalogue = every node.  u -> a, a -> u, u -> c: c is reachable in 2 or 3 hops only through the
    walk that returns to u.  u -> a2, a2 -> b, b -> a2, b -> d: a2 is reachable in 3 hops only as c == a -> (g, items, users, names)"""
    rng = np.random.RandomState(41)
    n_rand = 40
    E = [(int(s), int(d), int(r)) for s, d, r in zip(rng.randint(1, n_rand + 1, 90), rng.randint(1, n_rand + 1, 90), rng.randint(1, 5, 90))]
    u, a, c, a2, b, d = (n_rand + k for k in range(1, 7))
    E += [(u, a, 1), (a, u, 2), (u, c, 1), (u, a2, 3), (a2, b, 1), (b, a2, 2), (b, d, 1)]
    Ve = n_rand + 13                                   # (the planted nodes above d have no edge)
    E = np.array(E, np.int32)
    g = dict(src=E[:, 0].copy(), dst=E[:, 1].copy(), rel=E[:, 2].copy(), Ve=Ve, n_rand=n_rand, seed=41, cases={})
    items = np.arange(1, Ve, dtype=np.int32)
    users = np.array([u, a, b, 3, 17], np.int32)
    return g, items, users, dict(u=u, a=a, c=c, a2=a2, b=b, d=d)


def graph_c():
    """Ve = 8502: user 8500 -> hub 8499 -> every even id 2..8400 (4200 items); user 8497 -> hub 8498 -> every multiple of 3 up to 8400; catalogue = 1..8496,
    266 words: more than one 256-word chunk of the compaction, with set bits in every chunk -> (g, items, users)"""
    E = [(8500, 8499, 1)] + [(8499, e, 1 + e % 2) for e in range(2, 8401, 2)] + [(8497, 8498, 2)] + [(8498, e, 1) for e in range(3, 8401, 3)]
    E = np.array(E, np.int32)
    g = dict(src=E[:, 0].copy(), dst=E[:, 1].copy(), rel=E[:, 2].copy(), Ve=8502, n_rand=0, seed=0, cases={})
    return g, np.arange(1, 8497, dtype=np.int32), np.array([8500, 8497], np.int32)


def c_expected(u):
    """graph C's candidates at (2, 2) by its construction (the brute force over 8496 items per user would take minutes)"""
    return list(range(2, 8401, 2)) if u == 8500 else list(range(3, 8401, 3))
