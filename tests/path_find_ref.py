"""Shared by tests/test_path_find_host.py and tests/test_gpu_path_find.py: seeded typed graphs with the finder's edge cases planted in them, and a
brute-force depth-first enumeration of a pair's paths written independently of the library's CSR walk (include/kprn.h "finding a pair's paths")."""
import numpy as np

VR, VT, END_REL = 6, 4, 5        # relations 1..4 are drawn, 5 = #END_RELATION, 6 = pad; types 1..3 are drawn, 4 = pad
MAX_PATHS = 7                    # the cap the planted pairs are built around


def make_graph(n_rand, n_rand_edges, seed, hub=False):
    """nodes 1 .. n_rand carry random edges; the planted structures sit on nodes of their own above them, so their path counts are known:
      exact (a, a+1)      exactly MAX_PATHS paths of 1..3 hops
      inside (b, b+1)     more than MAX_PATHS, the cap falls inside the subtree of one first edge
      direct (c, c+1)     only the direct edge
      through (d, d+1)    d -> d+1 -> d+2 -> d+1 would pass through the item; plus d -> d+3 -> d (a 2-cycle back to the user) -> ... and a self-loop
      lonely              a node with no edge at all
    hub: one node of out-degree 300 (once a user, once the first neighbour of a user).  -> dict"""
    rng = np.random.RandomState(seed)
    E = []
    for _ in range(n_rand_edges):
        s, d = rng.randint(1, n_rand + 1, size=2)
        E.append((int(s), int(d), int(rng.randint(1, 5))))            # (self-loops among them are part of the input)
    nxt = n_rand + 1
    a = nxt; nxt += 4       # exact: 2 hops 3 + 2, 3 hops 2
    E += [(a, a + 2, 1), (a + 2, a + 1, 1), (a + 2, a + 1, 2), (a + 2, a + 1, 3), (a, a + 3, 2), (a + 3, a + 1, 1), (a + 3, a + 1, 4), (a + 2, a + 3, 1)]
    b = nxt; nxt += 5       # inside: 2 hops 2 + 1, 3 hops 3 + 4
    E += [(b, b + 2, 1), (b, b + 3, 1), (b + 2, b + 1, 1), (b + 2, b + 1, 2), (b + 3, b + 1, 3), (b + 2, b + 3, 2), (b + 2, b + 4, 1), (b + 4, b + 1, 1),
          (b + 4, b + 1, 2), (b + 3, b + 2, 4), (b + 3, b + 4, 2)]
    c = nxt; nxt += 2       # direct edge only
    E += [(c, c + 1, 3)]
    d = nxt; nxt += 5       # through the item, a 2-cycle back to the user, a multi-edge, a self-loop, a duplicated edge
    E += [(d, d + 1, 1), (d + 1, d + 2, 1), (d + 2, d + 1, 2), (d, d + 3, 1), (d + 3, d, 2), (d + 3, d + 1, 1), (d + 3, d + 1, 4), (d + 3, d + 3, 1),
          (d + 3, d + 4, 1), (d + 4, d + 1, 2), (d, d + 3, 1)]
    lonely = nxt; nxt += 1
    cases = dict(exact=(a, a + 1), inside=(b, b + 1), direct=(c, c + 1), through=(d, d + 1), same=(d, d), lonely=(lonely, a + 1), unreachable=(a + 1, a))
    if hub:
        hub_n = nxt; nxt += 1
        tgt = list(range(1, 300)) + [a]                                 # 300 distinct neighbours
        E += [(hub_n, t, 1 + (t % 4)) for t in tgt]
        E += [(hub_n, 5, 4), (hub_n, 5, 4)]                             # (a duplicate among the hub's edges: out-degree stays 300 after the build ... + 0)
        before = nxt; nxt += 1
        E += [(before, hub_n, 2), (before, 7, 1)]
        item = nxt; nxt += 1
        E += [(int(t), item, int(1 + (t % 3))) for t in rng.choice(np.arange(1, n_rand + 1), size=150, replace=False)]
        cases.update(hub_user=(hub_n, item), hub_next=(before, item), hub_item_exact=(hub_n, a + 1))
        cases["hub"] = hub_n
    Ve = nxt + 1                                                        # nodes 1 .. Ve - 1, Ve = the pad row
    E = np.array(E, np.int32)
    E = E[rng.permutation(len(E))]                                      # any order
    return dict(src=E[:, 0].copy(), dst=E[:, 1].copy(), rel=E[:, 2].copy(), Ve=Ve, cases=cases, n_rand=n_rand, seed=seed)


def node_types(g, num_types):
    rng = np.random.RandomState(g["seed"] + 17 * num_types)
    nt = rng.randint(1, VT, size=(g["Ve"], num_types)).astype(np.int32)   # 1 .. VT - 1
    if num_types > 1:
        nt[rng.rand(g["Ve"]) < 0.5, 0] = VT                             # a slot left-padded with the type table's pad id
    nt[-1] = 0                                                          # the pad entity's row is ignored, whatever it holds
    return nt


def pairs_of(g, n_extra, seed):
    """the planted pairs first, then random pairs among the random nodes"""
    rng = np.random.RandomState(seed)
    pr = [v for k, v in g["cases"].items() if isinstance(v, tuple)]
    pr += [tuple(int(x) for x in rng.randint(1, g["n_rand"] + 1, size=2)) for _ in range(n_extra)]
    return np.array(pr, np.int32)


def brute_paths(g, u, i, min_hops, max_hops):
    """every path u -> i of min_hops .. max_hops hops over the distinct non-loop edges, all nodes distinct, in the canonical order ->
    [(nodes (u, n1, .., i), rels (r0, ..))]"""
    edges = sorted({(int(s), int(d), int(r)) for s, d, r in zip(g["src"], g["dst"], g["rel"]) if s != d})
    out_of = {}
    for s, d, r in edges:
        out_of.setdefault(s, []).append((d, r))
    found = []

    def dfs(nodes, rels):
        for d, r in out_of.get(nodes[-1], ()):
            if d in nodes:
                continue
            if d == i:
                if min_hops <= len(rels) + 1 <= max_hops:
                    found.append((nodes + (d,), rels + (r,)))
            elif len(rels) + 1 < max_hops:
                dfs(nodes + (d,), rels + (r,))

    if u != i:
        dfs((u,), ())
    key = lambda p: (len(p[1]), tuple(x for n, r in zip(p[0][1:], p[1]) for x in (n, r)))
    return sorted(found, key=key)


def rows_of(paths, nt, Ve, T, F):
    """the [len(paths), T, F] rows the finder writes for them"""
    num_types = nt.shape[1]
    lead = F - num_types - 2
    out = np.zeros((len(paths), T, F), np.int32)
    for p, (nodes, rels) in enumerate(paths):
        h = len(rels)
        out[p, :, :lead + num_types] = VT
        out[p, :, F - 2] = Ve
        out[p, :, F - 1] = VR
        for k, n in enumerate(nodes):
            t = T - (h + 1) + k
            out[p, t, lead:lead + num_types] = nt[n - 1]
            out[p, t, F - 2] = n
            out[p, t, F - 1] = rels[k] if k < h else END_REL
    return out


def brute_find(g, nt, pairs, min_hops, max_hops, max_paths, T, F):
    """-> (idx [N,T,F], counts [B], found [B]) by the brute force"""
    rows, counts, found = [], [], []
    for u, i in pairs:
        ps = brute_paths(g, int(u), int(i), min_hops, max_hops)
        found.append(len(ps))
        counts.append(min(len(ps), max_paths))
        rows.append(rows_of(ps[:max_paths], nt, g["Ve"], T, F))
    idx = np.concatenate(rows) if rows else np.zeros((0, T, F), np.int32)
    return idx, np.array(counts, np.int32), np.array(found, np.int64)
