"""not gpu: the selection rule of include/kprn.h "hard negatives" -- kprn_host_select_hardest, the host twin of kprn_amd/csrc/select_hardest.hip (built from the
same __host__ __device__ rule, select_hardest.h) -- against tests/select_hardest_ref.py, a few lines of numpy that use nothing of the code under test.  Every
comparison is np.array_equal."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from kprn_amd import _ffi

from . import select_hardest_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def groups():
    sc, goff, pos = sref.group_set()
    for a in (sc, goff, pos):
        a.setflags(write=False)
    return sc, goff, pos


def test_group_set_holds_what_it_promises(groups):
    sc, goff, pos = groups
    sizes = np.diff(goff)
    for n in sref.SIZES:
        assert set(pos[sizes == n].tolist()) >= {-1, 0, n - 1, n // 2}
    assert np.isnan(sc).any() and np.isposinf(sc).any() and np.isneginf(sc).any() and (np.signbit(sc) & (sc == 0)).any() and ((sc == 0) & ~np.signbit(sc)).any()
    nan_pos = [g for g in range(len(pos)) if pos[g] >= 0 and np.isnan(sc[goff[g] + pos[g]])]
    assert nan_pos                                                          # NaN as the positive


@pytest.mark.parametrize("n_keep", [1, 2, 4, 63, 64, 65, 255, 256])
def test_twin_equals_the_restatement(groups, n_keep):
    sc, goff, pos = groups
    want, want_inv = sref.select(sc, goff, n_keep, pos=pos)
    got, got_inv = _ffi.host_select_hardest(sc, goff, n_keep, pos=pos)
    assert np.array_equal(got, want) and got_inv == want_inv
    sizes, kept = np.diff(goff), np.add.reduceat(got.astype(np.int64), goff[:-1])
    assert np.array_equal(kept, np.minimum(sizes - (pos >= 0), n_keep) + (pos >= 0))   # a group with n_keep or fewer negatives keeps them all
    assert (sizes - (pos >= 0) <= n_keep).any() and (sizes - (pos >= 0) > n_keep).any()
    # NULL pos = no positive anywhere
    want, want_inv = sref.select(sc, goff, n_keep)
    got, got_inv = _ffi.host_select_hardest(sc, goff, n_keep)
    assert np.array_equal(got, want) and got_inv == want_inv == int(np.isnan(sc).sum())


def test_the_rules_sentences_by_hand():
    sc = np.array([0.5, 0.9, 0.9, 0.1, np.nan, 0.7], np.float32)
    one = lambda n_keep, p: _ffi.host_select_hardest(sc, [0, 6], n_keep, pos=[p])
    assert one(2, -1)[0].tolist() == [0, 1, 1, 0, 0, 0] and one(2, -1)[1] == 1          # ties: both 0.9
    assert one(1, -1)[0].tolist() == [0, 1, 0, 0, 0, 0]                                 # the lower index wins the tie
    assert one(1, 1)[0].tolist() == [0, 1, 1, 0, 0, 0]                                  # the positive does not use up a place
    assert one(2, 3)[0].tolist() == [0, 1, 1, 1, 0, 0]                                  # ... wherever it scores
    assert one(2, 4)[0].tolist() == [0, 1, 1, 0, 1, 0] and one(2, 4)[1] == 0                                          # a NaN positive is kept, not counted
    assert one(5, -1)[0].tolist() == [1, 1, 1, 1, 0, 1] and one(6, -1)[0].tolist() == [1] * 6                         # NaN sorts below every valid member
    zeros = np.array([-0.0, 0.0, -0.0, 1e-45], np.float32)
    assert _ffi.host_select_hardest(zeros, [0, 4], 2)[0].tolist() == [1, 0, 0, 1]                                     # -0 == +0: index 0 first
    inf = np.array([-np.inf, np.nan, np.inf, 3e38], np.float32)
    assert _ffi.host_select_hardest(inf, [0, 4], 3)[0].tolist() == [1, 0, 1, 1]                                       # -inf is valid: above NaN


def test_members_with_a_repeated_line_and_a_slice_of_the_table():
    rng = np.random.RandomState(2)
    sc = rng.rand(50).astype(np.float32)
    sc[7] = 2.0
    members = np.concatenate([[7, 7, 3, 7, 9], rng.randint(0, 50, 300), [49, 0]]).astype(np.int64)
    goff = np.array([0, 5, 305, 307], np.int64)
    pos = np.array([1, 17, -1], np.int32)
    for n_keep in (1, 2, 40):
        want, _ = sref.select(sc, goff, n_keep, members=members, pos=pos)
        got, inv = _ffi.host_select_hardest(sc, goff, n_keep, members=members, pos=pos)
        assert np.array_equal(got, want) and inv == 0
    assert _ffi.host_select_hardest(sc, goff, 2, members=members, pos=pos)[0][:5].tolist() == [1, 1, 0, 1, 0]   # line 7 three times: index order; pos kept
    # groups that start inside members / inside the scores: nothing below group_offsets[0] is touched
    keep = np.full(307, 9, np.uint8)
    got, _ = _ffi.host_select_hardest(sc, goff[1:], 3, members=members, pos=pos[1:], keep=keep)
    assert (got[:5] == 9).all() and np.array_equal(got[5:], sref.select(sc, goff, 3, members=members, pos=pos)[0][5:])
    keep = np.full(50, 9, np.uint8)
    got, _ = _ffi.host_select_hardest(sc, [10, 30, 50], 4, pos=[-1, 5], keep=keep)
    assert (got[:10] == 9).all() and np.array_equal(got[10:], sref.select(sc, [0, 10, 30, 50], 4, pos=[-1, -1, 5])[0][10:])


def _call(scores, n_scores, members, goff, pos, G, n_keep, keep, ninv):
    fp = _ffi._fp
    return _ffi.lib().kprn_host_select_hardest(fp(scores), C.c_int64(n_scores), fp(members), fp(goff), fp(pos), G, n_keep, fp(keep), fp(ninv))


def test_every_refusal_and_a_refused_call_writes_nothing():
    sc = np.linspace(0, 1, 5000).astype(np.float32)
    goff = np.array([0, 3, 10], np.int64)
    pos = np.array([0, 6], np.int32)
    mem = np.arange(10, dtype=np.int64)
    i64, i32 = (lambda *v: np.array(v, np.int64)), (lambda *v: np.array(v, np.int32))
    cases = [
        (dict(goff=None), _ffi.E_ARG), (dict(G=0), _ffi.E_ARG), (dict(n_keep=0), _ffi.E_ARG), (dict(n_keep=257), _ffi.E_ARG), (dict(n_keep=-1), _ffi.E_ARG),
        (dict(goff=i64(-1, 3, 10)), _ffi.E_ARG), (dict(goff=i64(0, 0, 10)), _ffi.E_ARG), (dict(goff=i64(0, 5, 3)), _ffi.E_ARG),
        (dict(goff=i64(0, 3, 4100), members=None), _ffi.E_ARG), (dict(pos=i32(0, 7)), _ffi.E_ARG), (dict(pos=i32(-2, 0)), _ffi.E_ARG), (dict(pos=i32(3, 0)), _ffi.E_ARG),
        (dict(members=i64(0, 1, 2, 3, 4, 5, 6, 7, 8, 5000)), _ffi.E_INDEX), (dict(members=i64(0, 1, 2, -1, 4, 5, 6, 7, 8, 9)), _ffi.E_INDEX),
        (dict(members=None, n_scores=9), _ffi.E_INDEX), (dict(scores=None), _ffi.E_ARG), (dict(n_scores=-1), _ffi.E_ARG), (dict(keep=None), _ffi.E_ARG),
    ]
    for kw, status in cases:
        a = dict(scores=sc, n_scores=len(sc), members=mem, goff=goff, pos=pos, G=2, n_keep=2)
        a.update(kw)
        keep, ninv = np.full(4200, 77, np.uint8), np.full(1, -77, np.int64)
        rc = _call(a["scores"], a["n_scores"], a["members"], a["goff"], a["pos"], a["G"], a["n_keep"], None if "keep" in kw else keep, ninv)
        assert rc == status and (keep == 77).all() and ninv[0] == -77, kw
    keep, ninv = np.full(10, 77, np.uint8), np.full(1, -77, np.int64)                      # the same arguments, unrefused; n_invalid may be NULL
    assert _call(sc, len(sc), mem, goff, pos, 2, 2, keep, ninv) == 0 and ninv[0] == 0 and keep.tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 1, 1]
    assert _call(sc, len(sc), mem, goff, pos, 2, 256, keep, None) == 0 and (keep == 1).all()
    # what the binding itself checks before the library is called
    for kw in (dict(group_offsets=[0]), dict(members=np.arange(4)), dict(pos=[0]), dict(keep=np.zeros(9, np.uint8)), dict(keep=np.zeros(10, np.int32))):
        a = dict(group_offsets=goff, n_keep=2, pos=pos)
        a.update(kw)
        with pytest.raises(_ffi.KprnError) as ei:
            _ffi.host_select_hardest(sc, **a)
        assert ei.value.code == _ffi.E_ARG, kw


# ---- the twin as a stand-alone program under the host sanitizers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def san_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("san") / "select_hardest_san")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "kprn_amd", "csrc"),
           os.path.join(ROOT, "tests", "select_hardest_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_san(exe, tmp_path, scores, members, goff, pos, n_keep):
    sc, goff = np.ascontiguousarray(scores, np.float32), np.ascontiguousarray(goff, np.int64)
    mem = None if members is None else np.ascontiguousarray(members, np.int64)
    p = None if pos is None else np.ascontiguousarray(pos, np.int32)
    keep_len = max(int(goff[-1]), 0)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(sc), len(goff) - 1, -1 if mem is None else len(mem), p is not None, n_keep, keep_len], np.int64).tobytes())
        for a in (sc, mem, goff, p):
            if a is not None:
                f.write(a.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]                                       # (a sanitizer report ends the program with a non-zero status)
    raw = open(dst, "rb").read()
    rc, ninv = np.frombuffer(raw[:16], np.int64)
    return int(rc), int(ninv), np.frombuffer(raw[16:], np.uint8)


def test_twin_under_the_host_sanitizers(san_program, tmp_path, groups):
    """the whole group set (every array a heap block of exactly its size), scattered members that end at the last score, and two refusals"""
    sc, goff, pos = groups
    for n_keep in (1, 4, 256):
        rc, ninv, keep = run_san(san_program, tmp_path, sc, None, goff, pos, n_keep)
        want, want_inv = sref.select(sc, goff, n_keep, pos=pos)
        assert rc == 0 and ninv == want_inv and np.array_equal(keep, want)
    members = np.concatenate([[len(sc) - 1, 0, len(sc) - 1], np.arange(len(sc) - 300, len(sc))]).astype(np.int64)
    mgoff, mpos = [0, 3, 303], [2, 299]
    rc, ninv, keep = run_san(san_program, tmp_path, sc, members, mgoff, mpos, 5)
    want, want_inv = sref.select(sc, mgoff, 5, members=members, pos=mpos)
    assert rc == 0 and ninv == want_inv and np.array_equal(keep, want)
    rc, ninv, keep = run_san(san_program, tmp_path, sc, members, mgoff, None, 1)     # pos NULL
    assert rc == 0 and np.array_equal(keep, sref.select(sc, mgoff, 1, members=members)[0])
    for bad_members, bad_keep, status in ((np.concatenate([members[:-1], [len(sc)]]), 5, _ffi.E_INDEX), (members, 0, _ffi.E_ARG)):
        rc, ninv, keep = run_san(san_program, tmp_path, sc, bad_members, mgoff, mpos, bad_keep)
        assert rc == status and ninv == -77 and (keep == 77).all()
