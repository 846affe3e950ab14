"""kprn_host_find_candidates (no GPU) against a brute force written from the definition: a catalogue member is a candidate when path_find_ref.brute_paths
finds a path to it (include/kprn.h "candidates of a user").  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from kprn_amd import _ffi

from . import candidates_ref as cref


@pytest.fixture(scope="module")
def A():
    return cref.graph_a()


def twin(g, items, users, lo, hi, exclude, threads=8):
    return _ffi.host_find_candidates(g["src"], g["dst"], g["rel"], g["Ve"], items, users, lo, hi, exclude, threads=threads)


def of_user(cand, gc, users, u):
    k = [int(x) for x in users].index(int(u))
    off = int(gc[:k].sum())
    return cand[off:off + int(gc[k])].tolist()


def test_symbols_are_exported():
    L = _ffi.lib()
    for name in ("kprn_find_candidates", "kprn_read_candidates", "kprn_find_paths_of_candidates", "kprn_host_find_candidates"):
        assert name in _ffi.declared_symbols() and getattr(L, name)


def test_fixture_a_holds_the_figures(A):
    g, items, users = A
    stored = {(int(s), int(d), int(r)) for s, d, r in zip(g["src"], g["dst"], g["rel"]) if s != d}
    assert g["Ve"] == 402 and len(stored) == 1381 and len(items) == 268
    c = g["cases"]
    n = lambda u, lo, hi, ex: len(cref.brute_candidates(g, items, u, lo, hi, ex))
    hub, before = c["hub"], c["hub_next"][0]
    assert (n(hub, 1, 3, 0), n(hub, 1, 3, 1)) == (250, 50) and (n(hub, 2, 3, 0), n(hub, 2, 3, 1)) == (230, 50) and (n(hub, 1, 1, 0), n(hub, 1, 1, 1)) == (200, 0)
    assert (n(before, 1, 3, 0), n(before, 1, 3, 1)) == (245, 243)
    assert (n(c["direct"][0], 1, 3, 0), n(c["direct"][0], 1, 3, 1)) == (1, 0) and n(c["direct"][0], 2, 3, 0) == 0
    assert (n(c["exact"][0], 1, 3, 0), n(c["exact"][0], 1, 3, 1)) == (2, 1)
    assert (n(c["inside"][0], 1, 3, 0), n(c["inside"][0], 1, 3, 1)) == (3, 2) and (n(c["inside"][0], 3, 3, 0), n(c["inside"][0], 3, 3, 1)) == (2, 2)
    assert n(c["lonely"][0], 1, 3, 0) == 0 and n(c["unreachable"][0], 1, 3, 0) == 0
    assert {hub, before, c["lonely"][0], c["unreachable"][0]} <= set(users.tolist()) and len(users) == 28


@pytest.mark.parametrize("exclude", [0, 1])
@pytest.mark.parametrize("hops", cref.HOPS)
def test_twin_equals_brute_force_on_a(A, hops, exclude):
    g, items, users = A
    cand, gc = twin(g, items, users, hops[0], hops[1], exclude)
    want, want_gc = cref.brute_all(g, items, users, hops[0], hops[1], exclude)
    assert np.array_equal(gc, want_gc) and np.array_equal(cand, want)


def test_twin_on_b_the_walks_that_return():
    g, items, users, n = cref.graph_b()
    for hops in cref.HOPS:
        for exclude in (0, 1):
            cand, gc = twin(g, items, users, hops[0], hops[1], exclude)
            want, want_gc = cref.brute_all(g, items, users, hops[0], hops[1], exclude)
            assert np.array_equal(gc, want_gc) and np.array_equal(cand, want), (hops, exclude)
    cand, gc = twin(g, items, users, 2, 3, 0)
    mine = of_user(cand, gc, users, n["u"])
    assert n["c"] not in mine and n["a2"] not in mine and n["b"] in mine and n["d"] in mine
    cand, gc = twin(g, items, users, 3, 3, 0)
    mine = of_user(cand, gc, users, n["u"])
    assert n["d"] in mine and n["b"] not in mine and n["a2"] not in mine


def test_twin_on_c_more_than_one_chunk_of_words():
    g, items, users = cref.graph_c()
    assert (len(items) + 31) // 32 == 266
    for exclude in (0, 1):
        cand, gc = twin(g, items, users, 2, 2, exclude)
        assert gc.tolist() == [4200, 2800]
        assert of_user(cand, gc, users, 8500) == cref.c_expected(8500) and of_user(cand, gc, users, 8497) == cref.c_expected(8497)
    # the definition itself on a sample of the items (the whole catalogue would take minutes)
    some = np.array([1, 2, 3, 6, 4199, 4200, 8399, 8400, 8401, 8496], np.int32)
    cand, gc = twin(g, some, users, 2, 2, 1)
    want, want_gc = cref.brute_all(g, some, users, 2, 2, 1)
    assert np.array_equal(gc, want_gc) and np.array_equal(cand, want)
    cand, gc = twin(g, items, users, 1, 1, 0)
    assert cand.tolist() == [] and gc.tolist() == [0, 0]                 # the hubs are beyond the catalogue's last id


def test_threads_and_counts_only(A):
    g, items, users = A
    one = twin(g, items, users, 1, 3, 1, threads=1)
    eight = twin(g, items, users, 1, 3, 1, threads=8)
    assert np.array_equal(one[0], eight[0]) and np.array_equal(one[1], eight[1])
    gc = np.full(len(users), -7, np.int32)
    src, dst, rel = (np.ascontiguousarray(g[k], np.int32) for k in ("src", "dst", "rel"))
    rc = _ffi.lib().kprn_host_find_candidates(_ffi._fp(src), _ffi._fp(dst), _ffi._fp(rel), C.c_int64(len(src)), g["Ve"], _ffi._fp(items), C.c_int64(len(items)),
                                              _ffi._fp(users), len(users), 1, 3, 1, 2, _ffi._fp(gc), None)
    assert rc == 0 and np.array_equal(gc, one[1])


def test_refusals_write_nothing(A):
    g, items, users = A
    src, dst, rel = (np.ascontiguousarray(g[k], np.int32) for k in ("src", "dst", "rel"))

    def call(items=items, users=users, B=None, lo=1, hi=3):
        gc = np.full(max(len(users), 1), -7, np.int32)
        cand = np.full(4096 * 8, -7, np.int32)
        rc = _ffi.lib().kprn_host_find_candidates(_ffi._fp(src), _ffi._fp(dst), _ffi._fp(rel), C.c_int64(len(src)), g["Ve"], _ffi._fp(items), C.c_int64(len(items)),
                                                  _ffi._fp(users), len(users) if B is None else B, lo, hi, 1, 2, _ffi._fp(gc), _ffi._fp(cand))
        assert (gc == -7).all() and (cand == -7).all()
        return rc

    swapped = items.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert call(items=swapped) == _ffi.E_ARG                               # items not ascending
    for bad_user in (0, g["Ve"]):
        us = users.copy()
        us[5] = bad_user
        assert call(users=us) == _ffi.E_INDEX
    assert call(lo=0) == _ffi.E_ARG and call(hi=4) == _ffi.E_ARG and call(lo=3, hi=2) == _ffi.E_ARG
    assert call(B=0) == _ffi.E_ARG
    with pytest.raises(_ffi.KprnError) as ei:
        twin(g, items, np.zeros(0, np.int32), 1, 3, 1)
    assert ei.value.code == _ffi.E_ARG
