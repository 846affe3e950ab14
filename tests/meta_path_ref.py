"""Shared by tests/test_meta_path_host.py and tests/test_gpu_meta_path.py: the meta-path rule (include/kprn.h "meta-paths") in pure Python -- `matches`, and
that function applied as a filter to the path lists the other references produce (path_find_ref.brute_paths, path_walk_ref.pair_paths, path_cap_ref.select,
the candidates).  Nothing here calls the library."""
import numpy as np

from . import path_cap_ref as cr
from . import path_find_ref as ref
from . import path_walk_ref as wr

# the fixture set: relations 1..4 are the ones path_find_ref draws.  A pattern = a list of positions; a position = a set of relation ids, None = any
FIXTURE = [
    [{3}],
    [{1, 2}, {1, 3}],
    [None, {1, 2}, {2, 4}],
    [{1}, None, None],
    [None, {1, 2}, None, {1, 3}],
    [{1, 2, 3}, None, None, {2, 4}, None],
    [None, None, {4}, None, {1}],
]
CAP_ALL = 2**31 - 1


def n_matching(rels, patterns):
    """how many patterns the relation sequence matches"""
    return sum(1 for p in patterns if len(p) == len(rels) and all(not s or int(r) in s for r, s in zip(rels, p)))


def matches(rels, patterns):
    return n_matching(rels, patterns) > 0


def keep(paths, patterns):
    """a list of (nodes, rels) with the non-matching paths removed, the order kept; patterns None or empty = no filter"""
    return list(paths) if not patterns else [p for p in paths if matches(p[1], patterns)]


def pair_lists(g, pairs, min_hops, max_hops, walks, seed, draw, patterns, memo=None):
    """every pair's filtered sequence; memo (a dict) keeps the unfiltered lists per (pairs, hops, walks, seed, draw)"""
    key = (pairs.tobytes(), min_hops, max_hops, walks, seed, draw)
    if memo is None or key not in memo:
        lists = [wr.pair_paths(g, int(u), int(i), b, min_hops, max_hops, walks, seed, draw) for b, (u, i) in enumerate(pairs)]
        if memo is not None:
            memo[key] = lists
    else:
        lists = memo[key]
    return [keep(ps, patterns) for ps in lists]


def brute_find(g, nt, pairs, min_hops, max_hops, max_paths, T, F, walks, seed, draw, patterns, cap="first", memo=None):
    """-> (idx [N,T,F], counts [B], found [B]): the cap ("first" | "spread", path_cap_ref.select over the FILTERED found) applied to the filtered sequences"""
    lists = pair_lists(g, pairs, min_hops, max_hops, walks, seed, draw, patterns, memo)
    found = np.array([len(ps) for ps in lists], np.int64)
    rows = []
    for b, ps in enumerate(lists):
        ranks = range(min(len(ps), max_paths)) if cap == "first" else cr.select(len(ps), max_paths, b, seed, draw)
        rows.append(ref.rows_of([ps[r] for r in ranks], nt, g["Ve"], T, F))
    idx = np.concatenate(rows) if rows else np.zeros((0, T, F), np.int32)
    return idx, np.minimum(found, max_paths).astype(np.int32), found


def end_counts(g, u, lo, hi, patterns):
    """node -> the number of (matching) paths of lo .. hi hops from u that end there, all nodes distinct: one depth-first walk out of u to 3 hops, kept in the
    graph's own dict per (user, pattern set) and summed over the asked hop counts"""
    memo = g.setdefault("_mp_memo", {})
    key = (int(u), id(patterns))
    if key not in memo:
        out_of = wr.adjacency(g)
        by_hop = {1: {}, 2: {}, 3: {}}

        def dfs(nodes, rels):
            for d, r in out_of.get(nodes[-1], ()):
                if d in nodes:
                    continue
                rr = rels + (r,)
                if not patterns or matches(rr, patterns):
                    by_hop[len(rr)][d] = by_hop[len(rr)].get(d, 0) + 1
                if len(rr) < 3:
                    dfs(nodes + (d,), rr)

        dfs((int(u),), ())
        memo[key] = (patterns, by_hop)                                # (the set is kept alive, so its id stays its own)
    counts = {}
    for h in range(lo, hi + 1):
        for d, n in memo[key][1][h].items():
            counts[d] = counts.get(d, 0) + n
    return counts


def candidates(g, items, users, lo, hi, exclude, cap, patterns):
    """-> (cand [sum], group_counts [B], n_paths [sum]) as the candidates twin returns them: per user the members with a matching path, less the user and --
    exclude -- the members it has a stored edge to (of any relation), the cap best by (n_paths descending, id ascending), laid out by id"""
    items = np.asarray(items, np.int32)
    member = set(int(c) for c in items)
    cand, gc, npaths = [], [], []
    for u in users:
        u = int(u)
        adjacent = {int(d) for s, d in zip(g["src"], g["dst"]) if int(s) == u and s != d}
        cnt = {c: n for c, n in end_counts(g, u, lo, hi, patterns).items() if c in member and c != u and not (exclude and c in adjacent)}
        best = sorted(cnt, key=lambda c: (-cnt[c], c))[:cap]
        best.sort()
        cand += best
        npaths += [cnt[c] for c in best]
        gc.append(len(best))
    return np.array(cand, np.int32), np.array(gc, np.int32), np.array(npaths, np.int64)


def rels_of_rows(idx, Vr):
    """the relation sequence of every row of idx [N,T,F]: the last column of the steps that are neither padding (Vr) nor the last one"""
    out = []
    for row in idx:
        col = [int(r) for r in row[:, -1] if int(r) != Vr]
        out.append(tuple(col[:-1]))
    return out


def only_at(index, pattern, n=32):
    """n patterns of which only `index` is `pattern`; the others ask for one hop over #END_RELATION, which no edge of the inputs carries"""
    never = [{ref.END_REL}]
    return [pattern if p == index else never for p in range(n)]
