"""gpu: kprn_sample_eval_groups against the host twin kprn_host_sample_eval_groups (itself held to a numpy restatement by tests/test_eval_sample_host.py):
every output and the list read back, the finder on the cut list, the ranking stage over the returned groups, and the refusals.  Every comparison is
exact."""
import numpy as np
import pytest

from kprn_amd import _ffi

from . import candidates_ref as cref
from . import eval_sample_ref as eref
from . import path_find_ref as ref

pytestmark = pytest.mark.gpu

SHAPE = dict(dt=16, de=32, dr=16, H=64, L=2, F=3)
N_NEGS = (1, 32, 33, 256, 257, 4095)
# graph C at hops (2, 2): user 8500 has the 4200 even ids 2..8400 (17 chunks of 256 rows, 132 bitmap words), user 8497 the 2800 multiples of 3
T_8500 = [2, 7, 512, 514, 8400]        # the first row, an id that is no row, the rows at positions 255 and 256, the last row
T_8497 = [3, 5, 4200, 8400]


@pytest.fixture(scope="module")
def graphs():
    gb, ib, ub, _names = cref.graph_b()
    gc, ic, uc = cref.graph_c()
    return dict(B=(gb, ib, ub), C=(gc, ic, uc))


@pytest.fixture(scope="module")
def on_device(graphs):
    """one small engine per graph (the engine's Ve is the graph's), its graph and its catalogue in HBM"""
    made = {}

    def get(name):
        if name not in made:
            g, items, _ = graphs[name]
            eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, **SHAPE)
            made[name] = (eng, eng.graph(g["src"], g["dst"], g["rel"], ref.node_types(g, 1), ref.END_REL), eng.sampler(items))
        return made[name]
    yield get
    for eng, _, _ in made.values():
        eng.close()


def offsets(targets):
    return np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int64), np.array([i for t in targets for i in t], np.int32)


def device_and_twin(eng, gr, sm, Ve, users, hops, targets, n_neg, seed=11, draw=0, cap=0):
    """find_candidates, then the device stage and the twin on the same list -> (device result, twin result, the uncut pairs, group_counts)"""
    pairs, gc = eng.find_candidates(gr, sm, np.asarray(users, np.int32), hops[0], hops[1], False, cap=cap)
    toff, ti = offsets(targets)
    got = eng.sample_eval_groups(gc, toff, ti, n_neg, seed, draw)
    want = _ffi.host_sample_eval_groups(pairs, Ve, gc, toff, ti, n_neg, seed, draw)
    return got, want, pairs, gc


@pytest.mark.parametrize("n_neg", N_NEGS)
def test_device_equals_twin_on_c(graphs, on_device, n_neg):
    eng, gr, sm = on_device("C")
    Ve = graphs["C"][0]["Ve"]
    for users, targets in (([8500], [T_8500]), ([8500, 8497], [T_8500, T_8497]), ([8497, 8500], [[], T_8500])):
        got, want, pairs, gc = device_and_twin(eng, gr, sm, Ve, users, (2, 2), targets, n_neg)
        assert gc[users.index(8500)] == 4200
        assert eref.same(got, want), (users, n_neg)
        assert eng._cand_total == len(want["pairs"])
        reach = want["target_rows"] >= 0
        assert list(reach[:5]) == [True, False, True, True, True] or users[0] != 8500
        d = np.repeat([4196 if u == 8500 else 2797 for u in users], [len(t) for t in targets])      # the rows that are no targets
        assert np.all(want["n_drawn"][reach] == np.minimum(n_neg, d[reach])) and np.all(want["n_drawn"][~reach] == 0)
    one = device_and_twin(eng, gr, sm, Ve, [8500], (2, 2), [T_8500], n_neg)[0]
    both = device_and_twin(eng, gr, sm, Ve, [8497, 8500], (2, 2), [T_8497, T_8500], n_neg)[0]
    for k in range(5):                                  # a pair's sample does not depend on the slot or on the other users of the call
        a, b = one["neg_rows"][k], both["neg_rows"][len(T_8497) + k]
        assert np.array_equal(one["pairs"][a[a >= 0], 1], both["pairs"][b[b >= 0], 1])


def test_seed_and_draw_on_the_device(graphs, on_device):
    eng, gr, sm = on_device("C")
    Ve = graphs["C"][0]["Ve"]
    seen = []
    for seed, draw in ((11, 0), (11, 1), (12, 0), (11 + 2**40, 0), (2**64 - 1, 2**32 - 1)):
        got, want, _, _ = device_and_twin(eng, gr, sm, Ve, [8500, 8497], (2, 2), [T_8500, T_8497], 33, seed, draw)
        assert eref.same(got, want), (seed, draw)
        seen.append(got["pairs"].tobytes())
    assert len(set(seen)) == len(seen)


@pytest.mark.parametrize("n_neg", [1, 3, 4095])
def test_device_equals_twin_on_b(graphs, on_device, n_neg):
    """graph B: a few dozen rows per user at most -- d <= n_neg takes the whole of D; users without rows and without targets"""
    eng, gr, sm = on_device("B")
    g, _, users = graphs["B"]
    pairs, gc = eng.find_candidates(gr, sm, users, 1, 3, False)
    first = np.concatenate([[0], np.cumsum(gc)])
    assert 3 <= gc.max() < 60
    targets = []
    for b in range(len(users)):
        mine = pairs[first[b]:first[b + 1], 1]
        absent = [c for c in range(1, g["Ve"]) if c not in mine][:2]
        targets.append(sorted(set([int(c) for c in mine[[0, -1, len(mine) // 2]]] + absent)) if b != 1 and len(mine) else [])
    lonely = np.array([g["Ve"] - 1], np.int32)            # a planted node without an edge: no rows
    got, want, pairs, gc = device_and_twin(eng, gr, sm, g["Ve"], list(users) + list(lonely), (1, 3), targets + [[3, 9]], n_neg)
    assert gc[-1] == 0 and eref.same(got, want)
    if n_neg == 4095:                                   # every row of a user with a reachable target is kept
        assert np.array_equal(got["group_counts"], [n if len(t) else 0 for n, t in zip(gc, targets + [[]])])
        first, toff = np.concatenate([[0], np.cumsum(gc)]), offsets(targets + [[3, 9]])[0]
        for b in range(len(users)):
            for k in range(int(toff[b]), int(toff[b + 1])):
                if got["target_rows"][k] >= 0:
                    assert got["n_drawn"][k] == gc[b] - np.isin(pairs[first[b]:first[b + 1], 1], targets[b]).sum()


def test_the_finder_reads_the_cut_list(graphs, on_device):
    eng, gr, sm = on_device("C")
    got, want, _, _ = device_and_twin(eng, gr, sm, graphs["C"][0]["Ve"], [8500, 8497], (2, 2), [T_8500, T_8497], 33)
    total = len(want["pairs"])
    assert 34 * 2 < total <= 7 * 34                    # seven reachable targets and their 33 negatives each, shared rows once
    batch, counts, found = eng.find_paths_of_candidates(gr, total, 2, 2, 5, 4)
    want_batch, want_counts, want_found = eng.find_paths(gr, want["pairs"], 2, 2, 5, 4)
    try:
        assert (counts > 0).all() and batch.B == total
        assert np.array_equal(counts, want_counts) and np.array_equal(found, want_found)
        assert np.array_equal(batch.counts, want_batch.counts) and np.array_equal(batch.read_idx(), want_batch.read_idx())
    finally:
        batch.free(); want_batch.free()


def groups_of(res):
    """the returned rows as kprn_rank_groups' members table: one group per reachable target, [target, its negatives ascending], pos 0"""
    members, goff = [], [0]
    for k in np.nonzero(res["target_rows"] >= 0)[0]:
        members += [res["target_rows"][k]] + list(res["neg_rows"][k, :res["n_drawn"][k]])
        goff.append(len(members))
    return np.array(members, np.int64), np.array(goff, np.int64)


def distinct_scores(n, seed):
    """n fp32 scores in (0, 1) that differ in what "%.5f" prints"""
    assert n < 9000
    return ((np.random.RandomState(seed).permutation(n) + 1) * 1e-4).astype(np.float32)


@pytest.mark.parametrize("mode", [_ffi.RANK_PRINTED, _ffi.RANK_RAW])
@pytest.mark.parametrize("n_neg", [33, 4095])
def test_rank_groups_over_the_returned_members(graphs, on_device, n_neg, mode):
    eng, gr, sm = on_device("C")
    got, _, _, _ = device_and_twin(eng, gr, sm, graphs["C"][0]["Ve"], [8500, 8497], (2, 2), [T_8500, T_8497], n_neg)
    members, goff = groups_of(got)
    scores = distinct_scores(len(got["pairs"]), 5)
    eng.board_reserve(len(scores))
    eng.board_write(0, scores)
    pos = np.zeros(len(goff) - 1, np.int32)
    dev = eng.rank_groups(goff, members=members, pos=pos, mode=mode)
    host = _ffi.host_rank_groups(scores, goff, members=members, pos=pos, mode=mode)
    assert np.array_equal(dev["ranks"], host["ranks"]) and np.array_equal(dev["hist"], host["hist"])
    assert np.all(np.diff(goff) == np.minimum(n_neg, [4196] * 4 + [2797] * 3) + 1)


@pytest.mark.parametrize("mode", [_ffi.RANK_PRINTED, _ffi.RANK_RAW])
def test_with_every_negative_drawn_the_places_are_rank_targets(graphs, on_device, mode):
    """n_neg >= every d: a held pair's group is the user's whole D, so its rank equals kprn_rank_targets' place on the uncut list (scores are distinct,
    so the two tie rules cannot differ).  User 8500's rows beyond the first 4000 are left out by the catalogue so that d < 4096"""
    eng, gr, _ = on_device("C")
    sm = eng.sampler(np.arange(1, 8001, dtype=np.int32))
    users = np.array([8500, 8497], np.int32)
    targets = [[2, 7, 512, 514, 8000], [3, 5, 4200]]
    pairs, gc = eng.find_candidates(gr, sm, users, 2, 2, False)
    assert list(gc) == [4000, 2666]
    scores = distinct_scores(len(pairs), 9)
    first = np.concatenate([[0], np.cumsum(gc)])
    tin = [np.nonzero(np.isin(pairs[first[b]:first[b + 1], 1], targets[b]))[0].astype(np.int32) for b in range(2)]
    eng.board_reserve(len(pairs))
    eng.board_write(0, scores)
    full = eng.rank_targets(first.astype(np.int64), offsets(tin)[0], np.concatenate(tin), mode=mode)
    toff, ti = offsets(targets)
    got = eng.sample_eval_groups(gc, toff, ti, 4095, 3)
    assert np.array_equal(got["pairs"], pairs)              # nothing is cut
    members, goff = groups_of(got)
    ranks = eng.rank_groups(goff, members=members, pos=np.zeros(len(goff) - 1, np.int32), mode=mode)["ranks"]
    assert len(ranks) == 6 and np.array_equal(ranks, full["places"])
    sm.free()


def test_a_refused_call_leaves_list_and_counts(graphs, on_device):
    eng, gr, sm = on_device("C")
    users = np.array([8500, 8497], np.int32)
    pairs, gc = eng.find_candidates(gr, sm, users, 2, 2, False, cap=300)
    n_paths = eng.candidate_path_counts()
    toff, ti = offsets([T_8500, T_8497])
    bad = [(_ffi.E_ARG, dict(n_neg=0)), (_ffi.E_ARG, dict(n_neg=4096)), (_ffi.E_ARG, dict(gc=gc + np.array([1, 0], np.int32))),
           (_ffi.E_ARG, dict(ti=np.array([2, 2, 512, 514, 8400, 3, 5, 4200, 8400], np.int32))), (_ffi.E_ARG, dict(toff=np.array([1, 5, 9], np.int64))),
           (_ffi.E_INDEX, dict(ti=np.array([2, 7, 512, 514, 8502, 3, 5, 4200, 8400], np.int32))),
           (_ffi.E_INDEX, dict(ti=np.array([0, 7, 512, 514, 8400, 3, 5, 4200, 8400], np.int32)))]
    for code, kw in bad:
        args = dict(gc=gc, toff=toff, ti=ti, n_neg=8)
        args.update(kw)
        with pytest.raises(_ffi.KprnError) as ei:
            eng.sample_eval_groups(args["gc"], args["toff"], args["ti"], args["n_neg"], 1)
        assert ei.value.code == code, kw
        back = np.zeros_like(pairs)
        eng._ck(eng.L.kprn_read_candidates(eng.h, _ffi._fp(back), _ffi.C.c_int64(len(pairs))))
        assert np.array_equal(back, pairs) and np.array_equal(eng.candidate_path_counts(), n_paths)
    # the accepted call: the capped list is cut, and its path counts are gone
    got = eng.sample_eval_groups(gc, toff, ti, 8, 1)
    want = _ffi.host_sample_eval_groups(pairs, graphs["C"][0]["Ve"], gc, toff, ti, 8, 1)
    assert eref.same(got, want)
    with pytest.raises(_ffi.KprnError) as ei:
        eng.candidate_path_counts()
    assert ei.value.code == _ffi.E_ARG


def test_no_list_is_refused(graphs):
    g = graphs["B"][0]
    eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, **SHAPE)
    try:
        with pytest.raises(_ffi.KprnError) as ei:
            eng.sample_eval_groups([0], [0, 1], [3], 4, 1)
        assert ei.value.code == _ffi.E_ARG
    finally:
        eng.close()
