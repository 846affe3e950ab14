"""Shared by tests/test_graph_update_host.py and tests/test_gpu_graph_update.py: the update rule of include/kprn.h "updating a graph in place" as Python set
arithmetic over (src, dst, rel) tuples, written independently of the library's CSR code, and the deltas the tests apply: one with every case planted in it,
and seeded random ones."""
import numpy as np

from . import path_find_ref as pref

VR = pref.VR


def base_graph():
    """about 1 500 stored edges -- six 256-thread workgroups -- with a hub row of out-degree 300, longer than a workgroup"""
    return pref.make_graph(n_rand=380, n_rand_edges=900, seed=23, hub=True)


def stored(src, dst, rel):
    """S: what the build stores for an edge list: the distinct edges less self-loops"""
    return {(int(s), int(d), int(r)) for s, d, r in zip(src, dst, rel) if s != d}


def apply_rule(S, adds, removes):
    """S a set of tuples, adds / removes lists of (s, d, r); removals first (r == 0: every relation), then additions -> (S', n_added, n_removed)"""
    exact = {(int(s), int(d), int(r)) for s, d, r in removes if r != 0}
    anyrel = {(int(s), int(d)) for s, d, r in removes if r == 0}
    D = {e for e in S if e in exact or (e[0], e[1]) in anyrel}
    A = {(int(s), int(d), int(r)) for s, d, r in adds if s != d}
    left = S - D
    return left | A, len(A - left), len(D)


def csr_of(S, Ve):
    """the CSR kprn_graph_create stores for the edge set S -> (rowptr [Ve + 1], col, rel) int32"""
    ed = sorted(S)
    rowptr = np.zeros(Ve + 1, np.int64)
    for s, _, _ in ed:
        rowptr[s + 1:] += 1
    return rowptr.astype(np.int32), np.array([d for _, d, _ in ed], np.int32), np.array([r for _, _, r in ed], np.int32)


def edge_arrays(S):
    """an edge list (three int32 arrays) that holds exactly S, in sorted order"""
    ed = np.array(sorted(S), np.int32).reshape(-1, 3)
    return ed[:, 0].copy(), ed[:, 1].copy(), ed[:, 2].copy()


def rows(lst):
    return np.array(lst, np.int32).reshape(-1, 3)


def planted_delta(g, seed=41):
    """every case of the update rule in one delta on base_graph() -> (adds [n, 3], removes [m, 3], cases: name -> the tuple(s) planted for it)"""
    rng = np.random.RandomState(seed)
    S = stored(g["src"], g["dst"], g["rel"])
    Ve, c = g["Ve"], g["cases"]
    hub = c["hub"]
    hub_row = sorted(e for e in S if e[0] == hub)
    hub_dsts = sorted({d for _, d, _ in hub_row})
    free_rel = lambda s, d: next(r for r in range(1, 5) if (s, d, r) not in S)
    cases, adds, removes = {}, [], []

    def add(name, *es):
        cases[name] = es if len(es) > 1 else es[0]
        adds.extend(es)

    def rem(name, *es):
        cases[name] = es if len(es) > 1 else es[0]
        removes.extend(es)

    mid = hub_dsts[len(hub_dsts) // 2]
    add("add_inside_hub", (hub, mid, free_rel(hub, mid)))                         # a second relation to a middle neighbour: inside the hub's row
    a = c["exact"][0]                                                               # the hub's last neighbour is `a`, above every random node; its first is 1
    assert hub_dsts[0] == 1 and hub_dsts[-1] == a and hub_row[0][2] > 1
    add("add_before_hub_first", (hub, 1, 1))                                        # sorts in front of the hub's first edge (1, relation 2)
    add("add_behind_hub_last", (hub, hub - 1, 1))                                   # a destination above the hub's last one
    a2 = a + 2                                                                      # a + 2 -> a + 1 holds relations 1, 2, 3; a + 3 -> a + 1 holds 1 and 4
    assert {(a + 3, a + 1, 1), (a + 3, a + 1, 4)} <= S and (a + 3, a + 1, 2) not in S
    add("add_between_relations", (a + 3, a + 1, 2))
    twice = (3, 5, free_rel(3, 5))
    add("add_twice", twice, twice)
    add("add_stored", hub_row[7])
    add("add_self_loop", (9, 9, 1))
    lonely = c["lonely"][0]
    assert not any(e[0] == lonely for e in S)
    add("add_from_lonely", (lonely, 2, 3))
    add("add_from_node_1", (1, Ve - 1, free_rel(1, Ve - 1)))
    add("add_from_last_node", (Ve - 1, 1, free_rel(Ve - 1, 1)))
    rand_adds = [(int(s), int(d), int(r)) for s, d, r in zip(rng.randint(1, Ve, 300), rng.randint(1, Ve, 300), rng.randint(1, 5, 300))]
    add("add_random", *rand_adds)

    rem("remove_hub_middle", hub_row[len(hub_row) // 2 + 3])
    assert {(a2, a + 1, 1), (a2, a + 1, 2), (a2, a + 1, 3)} <= S
    rem("remove_every_relation", (a2, a + 1, 0))                                    # the exact pair's triple edge
    rem("remove_not_stored", (lonely, 1, 2))
    gone_twice = hub_row[20]
    rem("remove_twice", gone_twice, gone_twice)
    both = hub_row[40]                                                              # removed and added again: stored afterwards, counted in both counts
    rem("remove_and_add", both)
    adds.append(both)
    victim = c["inside"][0] + 2                                                     # b + 2: four edges out
    rem("remove_every_edge_of_a_node", *sorted(e for e in S if e[0] == victim))
    pool = sorted(S - set(hub_row))
    rem("remove_random", *[pool[k] for k in rng.choice(len(pool), size=200, replace=False)])
    order_a, order_r = rng.permutation(len(adds)), rng.permutation(len(removes))    # any order
    return rows(adds)[order_a], rows(removes)[order_r], cases


def random_delta(S, Ve, seed, n_add=120, n_del=90):
    """a seeded delta against the edge set S: random additions (some stored, some loops), removals drawn from S with a few rel = 0 and a few not stored"""
    rng = np.random.RandomState(seed)
    ed = sorted(S)
    adds = [(int(s), int(d), int(r)) for s, d, r in zip(rng.randint(1, Ve, n_add), rng.randint(1, Ve, n_add), rng.randint(1, 5, n_add))]
    removes = []
    if ed:
        adds += [ed[k] for k in rng.randint(0, len(ed), 5)]
        removes += [ed[k] for k in rng.randint(0, len(ed), n_del)]
        removes += [(ed[k][0], ed[k][1], 0) for k in rng.randint(0, len(ed), 6)]
    removes += [(int(s), int(d), int(r)) for s, d, r in zip(rng.randint(1, Ve, 8), rng.randint(1, Ve, 8), rng.randint(0, 5, 8))]
    return rows(adds), rows(removes)
