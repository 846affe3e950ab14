"""kprn_host_sample_eval_groups (include/kprn.h "sampled evaluation groups") against a numpy / Python-int restatement that uses nothing of it
(tests/eval_sample_ref.py) on hand-made candidate lists, its refusals, the uniformity of the draw, and the same twin as a stand-alone program under the
host sanitizers.  No GPU; every comparison is exact."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from kprn_amd import _ffi

from . import eval_sample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VE = 300
N_NEG = 4
EVEN = list(range(100, 140, 2))   # 20 rows with a gap between every two


def build(users):
    """users: (id, items ascending, targets ascending) per slot -> (pairs, group_counts, target_offsets, target_items)"""
    pairs = np.array([(u, c) for u, items, _ in users for c in items], np.int32).reshape(-1, 2)
    gc = np.array([len(items) for _, items, _ in users], np.int32)
    toff = np.concatenate([[0], np.cumsum([len(t) for _, _, t in users])]).astype(np.int64)
    ti = np.array([i for _, _, t in users for i in t], np.int32)
    return pairs, gc, toff, ti


USERS = [
    (10, [5, 6], [5, 6]),                              # d = 0
    (11, [5, 6, 7], [5, 7]),                           # d = 1
    (12, [2, 4, 6, 8], [4]),                           # d = n_neg - 1
    (16, [3, 4, 5], []),                               # no targets
    (13, [2, 4, 6, 8, 10], [6]),                       # d = n_neg
    (14, [1, 2, 3, 4, 5, 6], [3]),                     # d = n_neg + 1
    (17, [], [7, 9]),                                  # no rows
    (15, EVEN, [50, 100, 111, 120, 138, 200]),         # three reachable targets; unreachable ones first, between two rows, and last
    (18, [1, 299], [299]),                             # the id range's ends
    (15, EVEN, [50, 100, 111, 120, 138, 200]),         # the same user in another slot
]


@pytest.fixture(scope="module")
def case():
    arrays = build(USERS)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def twin(arrays, n_neg=N_NEG, seed=7, draw=0):
    return _ffi.host_sample_eval_groups(arrays[0], VE, arrays[1], arrays[2], arrays[3], n_neg, seed, draw)


@pytest.mark.parametrize("n_neg", [1, 3, N_NEG, 5, 17, 19, 4095])
@pytest.mark.parametrize("seed,draw", [(7, 0), (2**63 + 12345, 2**32 - 1)])
def test_twin_equals_the_reference(case, n_neg, seed, draw):
    got, want = twin(case, n_neg, seed, draw), ref.reference(*case, n_neg, seed, draw)
    assert ref.same(got, want)


def test_the_sentences_of_the_rule(case):
    pairs, gc, toff, ti = case
    got = twin(case)
    items = got["pairs"][:, 1]
    first = np.concatenate([[0], np.cumsum(got["group_counts"])])
    # d <= n_neg: the whole of D; d > n_neg: exactly n_neg
    want_drawn = {10: [0, 0], 11: [1, 1], 12: [3], 13: [4], 14: [4], 16: [], 17: [0, 0], 15: [0, 4, 0, 4, 4, 0], 18: [1]}
    for b, (u, _rows, t) in enumerate(USERS):
        assert list(got["n_drawn"][toff[b]:toff[b + 1]]) == want_drawn[u], u
        for k in range(int(toff[b]), int(toff[b + 1])):
            row, neg = got["target_rows"][k], got["neg_rows"][k]
            n = got["n_drawn"][k]
            assert np.all(neg[n:] == -1) and np.all(np.diff(neg[:n]) > 0)
            if ti[k] not in _rows:
                assert row == -1 and n == 0
                continue
            assert first[b] <= row < first[b + 1] and items[row] == ti[k] and got["pairs"][row, 0] == u
            assert np.all((neg[:n] >= first[b]) & (neg[:n] < first[b + 1]))
            assert not np.isin(items[neg[:n]], t).any()          # targets are never each other's negatives
    # the new list is the kept rows in the old order: every row is a target's or a drawn one, users stay consecutive
    used = set(got["target_rows"][got["target_rows"] >= 0]) | set(got["neg_rows"][got["neg_rows"] >= 0])
    assert used == set(range(len(got["pairs"])))
    assert got["group_counts"][3] == 0 and got["group_counts"][6] == 0
    # the same user id in two slots draws the same items
    a, b = (np.nonzero(np.array([u for u, _, _ in USERS]) == 15)[0])
    for ka, kb in zip(range(int(toff[a]), int(toff[a + 1])), range(int(toff[b]), int(toff[b + 1]))):
        na, nb = got["neg_rows"][ka], got["neg_rows"][kb]
        assert np.array_equal(items[na[na >= 0]], items[nb[nb >= 0]])
    # ... and alone in a call, at another place in the list
    alone = twin(build([USERS[7]]))
    for k, ka in enumerate(range(int(toff[a]), int(toff[a + 1]))):
        na, nb = got["neg_rows"][ka], alone["neg_rows"][k]
        assert np.array_equal(items[na[na >= 0]], alone["pairs"][nb[nb >= 0], 1])


def test_seed_and_draw_each_change_the_sample(case):
    base = twin(case, 4, 7, 0)
    for other in (twin(case, 4, 8, 0), twin(case, 4, 7 + 2**32, 0), twin(case, 4, 7, 1)):
        assert not ref.same(base, other)
        assert np.array_equal(base["n_drawn"], other["n_drawn"])
    assert ref.same(base, twin(case, 4, 7, 0))


def test_the_draw_is_uniform():
    """d = 12, n_neg = 4, seeds 0..5999: every row is chosen 2000 +- 220 times, six standard deviations of Binomial(6000, 1/3) (sd = 36.5)"""
    arrays = build([(21, list(range(40, 53)), [46])])
    hits_twin, hits_ref = np.zeros(13, np.int64), np.zeros(13, np.int64)
    for seed in range(6000):
        got = twin(arrays, 4, seed, 0)
        hits_twin[got["pairs"][got["neg_rows"][0], 1] - 40] += 1
        ks = ref.keys(seed, 0, 21, 46, [c for c in range(40, 53) if c != 46])
        for key in sorted(ks)[:4]:
            hits_ref[(key & 0xFFFFFFFF) - 40] += 1
    assert np.array_equal(hits_twin, hits_ref)
    assert hits_twin[6] == 0 and hits_twin.sum() == 24000
    rest = np.delete(hits_twin, 6)
    print("chosen", rest)
    assert np.all(np.abs(rest - 2000) <= 220)


# ---- refusals: straight through the C ABI, every output poisoned before the call ---------------------------------------------------------------------
def raw(pairs, gc, toff, ti, n_neg, Ve=VE, total=None, B=None, null=(), list_null=False):
    pairs, gc, ti = (np.ascontiguousarray(a, np.int32) for a in (pairs, gc, ti))
    toff = np.ascontiguousarray(toff, np.int64)
    NT, cols = max(len(ti), 1), min(max(n_neg, 1), 4096)
    out = dict(ngc=np.full(max(len(gc), 1), -77, np.int32), trow=np.full(NT, -77, np.int32), neg=np.full(NT * cols, -77, np.int32), nd=np.full(NT, -77, np.int32),
               new_list=np.full(max(2 * len(pairs), 2), -77, np.int32))
    new_total = C.c_int64(-77)
    ptr = lambda name: None if name in null else out[name].ctypes.data_as(C.c_void_p)
    rc = _ffi.lib().kprn_host_sample_eval_groups(None if list_null else pairs.ctypes.data_as(C.c_void_p), C.c_int64(len(pairs) if total is None else total), Ve,
                                                 gc.ctypes.data_as(C.c_void_p), len(gc) if B is None else B, toff.ctypes.data_as(C.c_void_p),
                                                 ti.ctypes.data_as(C.c_void_p), n_neg, C.c_uint64(1), C.c_uint32(0), ptr("ngc"),
                                                 None if "new_total" in null else C.byref(new_total), ptr("trow"), ptr("neg"), ptr("nd"), ptr("new_list"))
    untouched = new_total.value == -77 and all(np.all(a == -77) for a in out.values())
    return rc, untouched


GOOD = build([(10, [5, 6, 7, 8], [5, 7]), (11, [2, 9], [9])])


def test_every_refusal_leaves_the_outputs_untouched():
    p, gc, toff, ti = GOOD
    assert raw(p, gc, toff, ti, 2)[0] == 0
    refused = [
        (_ffi.E_ARG, dict(total=len(p) + 1)), (_ffi.E_ARG, dict(gc=[4, 1])), (_ffi.E_ARG, dict(gc=[-1, 7])), (_ffi.E_ARG, dict(B=0)),
        (_ffi.E_ARG, dict(toff=[0, 0, 0])), (_ffi.E_ARG, dict(toff=[1, 2, 3])), (_ffi.E_ARG, dict(toff=[0, 3, 2])),
        (_ffi.E_ARG, dict(ti=[5, 5, 9])), (_ffi.E_ARG, dict(ti=[7, 5, 9])),
        (_ffi.E_ARG, dict(n_neg=0)), (_ffi.E_ARG, dict(n_neg=-1)), (_ffi.E_ARG, dict(n_neg=4096)),
        (_ffi.E_ARG, dict(null=("ngc",))), (_ffi.E_ARG, dict(null=("new_total",))), (_ffi.E_ARG, dict(null=("trow",))), (_ffi.E_ARG, dict(null=("neg",))),
        (_ffi.E_ARG, dict(null=("nd",))), (_ffi.E_ARG, dict(list_null=True)),
        (_ffi.E_INDEX, dict(ti=[0, 7, 9])), (_ffi.E_INDEX, dict(ti=[5, 7, VE])), (_ffi.E_INDEX, dict(Ve=9)),
        (_ffi.E_ARG, dict(p=[(10, 5), (10, 5), (10, 7), (10, 8), (11, 2), (11, 9)])), (_ffi.E_ARG, dict(p=[(10, 5), (12, 6), (10, 7), (10, 8), (11, 2), (11, 9)])),
        (_ffi.E_INDEX, dict(p=[(10, 5), (10, 6), (10, 7), (10, VE), (11, 2), (11, 9)])),
    ]
    for code, kw in refused:
        kw = dict(kw)
        args = [kw.pop("p", p), kw.pop("gc", gc), kw.pop("toff", toff), kw.pop("ti", ti), kw.pop("n_neg", 2)]
        rc, untouched = raw(*args, **kw)
        assert rc == code and untouched, (code, kw, args)


def test_the_accepted_neighbours_of_the_refusals():
    p, gc, toff, ti = GOOD
    assert raw(p, gc, toff, ti, 4095)[0] == 0 and raw(p, gc, toff, ti, 1)[0] == 0
    assert raw(p, gc, toff, ti, 2, Ve=12)[0] == 0 and raw(p, gc, toff, ti, 2, Ve=11)[0] == _ffi.E_INDEX   # the largest id (user 11) is Ve - 1
    assert raw(p, gc, toff, ti, 2, null=("new_list",))[0] == 0                      # everything but the rows
    assert raw(p, gc, [0, 3, 3], [5, 7, 8], 2)[0] == 0                              # a user without targets
    assert raw(p, gc, toff, [5, 299, 9], 2)[0] == 0                                 # a target that is no row: unreachable, not refused
    empty = _ffi.host_sample_eval_groups(np.zeros((0, 2), np.int32), VE, [0, 0], [0, 1, 2], [4, 4], 3, 1)   # an empty list: everything unreachable
    assert len(empty["pairs"]) == 0 and list(empty["target_rows"]) == [-1, -1] and list(empty["n_drawn"]) == [0, 0] and np.all(empty["neg_rows"] == -1)


# ---- the twin as a stand-alone program under the host sanitizers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def san_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("san") / "eval_sample_san")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "kprn_amd", "csrc"),
           os.path.join(ROOT, "tests", "eval_sample_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_san(exe, tmp_path, pairs, gc, toff, ti, n_neg, seed, draw, Ve=VE):
    pairs, gc, ti = (np.ascontiguousarray(a, np.int32) for a in (pairs, gc, ti))
    toff = np.ascontiguousarray(toff, np.int64)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(pairs), Ve, len(gc), len(ti), n_neg, seed, draw], np.int64).tobytes())
        for a in (pairs, gc, toff, ti):
            f.write(a.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    raw_out = open(dst, "rb").read()
    rc, new_total = (int(x) for x in np.frombuffer(raw_out[:16], np.int64))
    body = np.frombuffer(raw_out[16:], np.int32)
    B, NT, nn = len(gc), len(ti), len(ti) * max(n_neg, 0)
    cuts = np.cumsum([B, NT, nn, NT])
    out = dict(group_counts=body[:cuts[0]], target_rows=body[cuts[0]:cuts[1]], neg_rows=body[cuts[1]:cuts[2]].reshape(NT, -1) if nn else body[:0],
               n_drawn=body[cuts[2]:cuts[3]], pairs=body[cuts[3]:].reshape(-1, 2))
    return rc, new_total, out


@pytest.mark.parametrize("n_neg", [1, N_NEG, 19, 4095])
def test_sanitized_twin_on_the_hand_made_lists(case, san_program, tmp_path, n_neg):
    rc, new_total, got = run_san(san_program, tmp_path, *case, n_neg, 7, 3)
    want = ref.reference(*case, n_neg, 7, 3)
    assert rc == 0 and new_total == len(want["pairs"]) and ref.same(got, want)


def test_sanitized_twin_refuses_cleanly(san_program, tmp_path):
    p, gc, toff, ti = GOOD
    for code, args in ((_ffi.E_ARG, (p, gc, toff, ti, 0)), (_ffi.E_ARG, (p, gc, toff, ti, 4096)), (_ffi.E_ARG, (p, gc, toff, [7, 5, 9], 2)),
                       (_ffi.E_INDEX, (p, gc, toff, [5, 7, VE], 2)), (_ffi.E_ARG, (p, [3, 2], toff, ti, 2)), (_ffi.E_ARG, (p, gc, [0, 0, 0], [], 2))):
        rc, new_total, got = run_san(san_program, tmp_path, *args, 1, 0)
        assert rc == code and new_total == -77 and all(np.all(got[n] == -77) for n in ref.NAMES if n != "pairs") and len(got["pairs"]) == 0, (code, args)
