"""Shared by tests/test_path_walk_host.py and tests/test_gpu_path_walk.py: a pure-Python Philox4x32-10 and a brute-force restatement of the sampling rule
(include/kprn.h "sampled paths of four and five hops"), written independently of the library's CSR walk: adjacency lists in dictionaries, a walk's edges
named by (node, place in its list).  Graphs, pairs and rows come from tests/path_find_ref.py."""
import numpy as np

from . import path_find_ref as ref

M32 = 0xFFFFFFFF
GRAPH = dict(n_rand=380, n_rand_edges=1800, seed=23, hub=True)      # the graph of both test files
N_EXTRA, PAIR_SEED = 60, 29                                          # pairs_of(g, 60, seed=29): 70 pairs
WALKS, SEED, DRAW, T = 64, 1, 0, 6


def make_inputs():
    """-> (g, pairs).  Rows 0..69: make_graph(**GRAPH) and pairs_of(g, 60, seed=29), whose figures test_path_walk_host.py re-derives.  In that graph the hub's
    only in-edge comes from a node nothing leads to, so the hub can be a prefix's first node but never its last one, and no walk of those 70 pairs closes
    over more than 13 edges.  One planted node more, `feeder` -> hub_next's user, and the pair (feeder, the hub's item) in row 70 supply the walks
    feeder -> . -> hub whose closing adjacency is the hub's 300 edges: more than a wave's 64 lanes, five chunks of the fill pass.  Nothing leads to
    `feeder`, so rows 0..69 find what they find without it."""
    g = ref.make_graph(**GRAPH)
    c = g["cases"]
    feeder = g["Ve"]
    add = lambda a, v: np.concatenate([g[a], np.array([v], np.int32)])
    g = dict(g, src=add("src", feeder), dst=add("dst", c["hub_next"][0]), rel=add("rel", 3), Ve=feeder + 1, cases=dict(c, feeder=(feeder, c["hub_user"][1])))
    pairs = np.concatenate([ref.pairs_of(dict(g, cases=c), N_EXTRA, PAIR_SEED), np.array([g["cases"]["feeder"]], np.int32)])
    return g, pairs


def philox4x32_10(counter, key):
    """Salmon et al., SC'11: ten rounds, multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85 -> four 32-bit words"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


_adj = {}


def adjacency(g):
    """node -> [(dst, rel)] over the distinct non-loop edges, sorted: the order the stored graph keeps a node's edges in"""
    key = id(g["src"])
    if key not in _adj:
        out_of = {}
        for s, d, r in sorted({(int(s), int(d), int(r)) for s, d, r in zip(g["src"], g["dst"], g["rel"]) if s != d}):
            out_of.setdefault(s, []).append((d, r))
        _adj[key] = (g["src"], out_of)                                # (the array is kept alive, so its id stays its own)
    return _adj[key][1]


def walk(out_of, u, i, b, w, h, seed, draw):
    """-> ("deg",) / ("rep",) for a dead walk, else ("live", edges ((node, place), ..), nodes (u, n1, ..), rels)"""
    r = philox4x32_10((w, 65536 + h, b, draw), (seed & M32, (seed >> 32) & M32))
    nodes, rels, edges = [u], [], []
    for k in range(h - 2):
        adj = out_of.get(nodes[-1], [])
        if not adj:
            return ("deg",)
        place = (r[k] * len(adj)) >> 32
        d, rel = adj[place]
        if d == i or d in nodes:
            return ("rep",)
        edges.append((nodes[-1], place))
        nodes.append(d)
        rels.append(rel)
    return ("live", tuple(edges), tuple(nodes), tuple(rels))


def walk_paths(g, u, i, b, h, walks, seed, draw, stats=None):
    """the sampled paths of h hops of the pair in row b -> one list per walk (empty for a dead or dropped walk) of (nodes, rels), in the rule's order.
    stats (a dict) counts dead_deg / dead_rep / dup / live / multi (live walks with more than one path) / wide (the largest closing adjacency)"""
    out_of = adjacency(g)
    per_walk, seen = [], set()
    st = stats if stats is not None else {}
    for w in range(walks):
        paths = []
        per_walk.append(paths)
        if u == i or i == 0:
            continue
        res = walk(out_of, u, i, b, w, h, seed, draw)
        if res[0] != "live":
            st["dead_" + res[0]] = st.get("dead_" + res[0], 0) + 1
            continue
        _, edges, nodes, rels = res
        if edges in seen:
            st["dup"] = st.get("dup", 0) + 1
            continue
        seen.add(edges)
        st["live"] = st.get("live", 0) + 1
        closing = out_of.get(nodes[-1], [])
        st["wide"] = max(st.get("wide", 0), len(closing))
        for m, r1 in closing:
            if m == i or m in nodes:
                continue
            for d, r2 in out_of.get(m, []):
                if d == i:
                    paths.append((nodes + (m, i), rels + (r1, r2)))
        if len(paths) > 1:
            st["multi"] = st.get("multi", 0) + 1
    return per_walk


def pair_paths(g, u, i, b, min_hops, max_hops, walks, seed, draw):
    """a pair's paths in the order of its rows: the exhaustive hops, then 4 hops' walks, then 5 hops'"""
    ps = ref.brute_paths(g, u, i, min_hops, min(max_hops, 3)) if min_hops <= 3 else []
    for h in (4, 5):
        if min_hops <= h <= max_hops:
            for paths in walk_paths(g, u, i, b, h, walks, seed, draw):
                ps = ps + paths
    return ps


def brute_find(g, nt, pairs, min_hops, max_hops, max_paths, T, F, walks, seed, draw, memo=None):
    """-> (idx [N,T,F], counts [B], found [B]).  memo (a dict): the pairs' path lists, kept per (hops, walks, seed, draw) for the next layout or cap"""
    key = (pairs.tobytes(), min_hops, max_hops, walks if max_hops > 3 else 0, seed if max_hops > 3 else 0, draw if max_hops > 3 else 0)
    if memo is None or key not in memo:
        lists = [pair_paths(g, int(u), int(i), b, min_hops, max_hops, walks, seed, draw) for b, (u, i) in enumerate(pairs)]
        if memo is not None:
            memo[key] = lists
    else:
        lists = memo[key]
    found = np.array([len(ps) for ps in lists], np.int64)
    counts = np.minimum(found, max_paths).astype(np.int32)
    rows = [ref.rows_of(ps[:max_paths], nt, g["Ve"], T, F) for ps in lists]
    return (np.concatenate(rows) if rows else np.zeros((0, T, F), np.int32)), counts, found
