"""kprn_host_rank_targets (include/kprn.h "ranking targets in groups of any size") against a numpy restatement that uses nothing of it
(tests/rank_targets_ref.py), against the existing ranking stage where both apply, its refusals, the same twin as a stand-alone program under the host
sanitizers, and KnowledgeGraph.holdout.  No GPU; every comparison is exact."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph

from . import candidates_top_ref as tref
from . import path_find_ref as pref
from . import rank_targets_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIST_LEN = 15


@pytest.fixture(scope="module")
def shapes():
    """per mode: the shape list as one call, and the reference's (places, hist), computed once and left unchanged"""
    out = {}
    for mode in (ref.PRINTED, ref.RAW):
        c = ref.cases(mode)
        places, hist = ref.reference(c["scores"], c["group_offsets"], c["target_offsets"], c["targets"], c["members"], mode, HIST_LEN)
        for a in list(c.values()) + [places, hist]:
            a.setflags(write=False)
        out[mode] = (c, places, hist)
    return out


def twin(c, mode, hist_len=HIST_LEN):
    return _ffi.host_rank_targets(c["scores"], c["group_offsets"], c["target_offsets"], c["targets"], members=c["members"], mode=mode, hist_len=hist_len)


@pytest.mark.parametrize("mode", [ref.PRINTED, ref.RAW])
def test_twin_equals_the_reference_on_the_shape_list(shapes, mode):
    c, places, hist = shapes[mode]
    got = twin(c, mode)
    assert got["places"].dtype == np.int32 and got["hist"].dtype == np.int64
    bad = np.nonzero(got["places"] != places)[0]
    assert len(bad) == 0, (bad[:5], got["places"][bad[:5]], places[bad[:5]])
    assert np.array_equal(got["hist"], hist)
    assert hist[HIST_LEN + 2] == 0 and hist[:HIST_LEN + 2].sum() == len(places)
    sizes = set(np.diff(c["group_offsets"]).tolist())
    assert set(ref.SIZES) <= sizes                                                   # the list holds what it says it holds
    assert (places == ref.ZERO).any() == (mode == ref.PRINTED) and hist[HIST_LEN + 3] > 0 and (places >= HIST_LEN).any()


@pytest.mark.parametrize("mode", [ref.PRINTED, ref.RAW])
def test_consecutive_runs_without_members(mode):
    c = ref.consecutive_cases(mode)
    want = ref.reference(c["scores"], c["group_offsets"], c["target_offsets"], c["targets"], None, mode, 4096)
    got = twin(c, mode, hist_len=4096)
    assert np.array_equal(got["places"], want[0]) and np.array_equal(got["hist"], want[1])


def test_the_references_two_routes_agree():
    rng = np.random.RandomState(3)
    for mode in (ref.PRINTED, ref.RAW):
        for s, t in ref.special_groups(mode) + [(ref.draw_scores(rng, 900), ref.draw_targets(rng, 900, k)) for k in (1, 2, 65, 900)]:
            a, b = ref.group_places(s, t, mode, by_comparison=True), ref.group_places(s, t, mode, by_comparison=False)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_the_sentences_of_the_rule():
    """the special groups, by hand"""
    sp = ref.special_groups(ref.PRINTED)
    one = lambda k, mode: _ffi.host_rank_targets(sp[k][0], [0, len(sp[k][0])], [0, len(sp[k][1])], sp[k][1], mode=mode, hist_len=4)
    r = one(0, ref.PRINTED)
    assert r["places"].tolist() == [-1, -1, -1] and r["hist"].tolist() == [0, 0, 0, 0, 0, 3, 0, 0]
    assert one(0, ref.RAW)["places"].tolist() == [0, 7 - 1, 299 - 2]                  # mode 1 has no zero samples: first seen first among equals
    assert one(1, ref.PRINTED)["places"].tolist() == [0]
    assert one(2, ref.PRINTED)["places"].tolist() == [-1, 0]                          # a zero sample for the first target and not for the second
    r = one(3, ref.PRINTED)                                                          # 0.3 nan 0.3 nan 0.2 -0.0 0.0; targets 1 (NaN), 2, 5 (-0.0: valid, key 0)
    assert r["places"].tolist() == [3, 1, 2] and r["hist"][4 + 3] == 2                # (the other NaN has the larger index: it is not above target 1)
    r = one(4, ref.PRINTED)
    assert r["places"].tolist() == [-1, -1] and r["hist"][4 + 3] == 3
    assert one(4, ref.RAW)["places"].tolist() == [0, 1]                               # against the one non-target, which lies between them
    assert one(5, ref.PRINTED)["places"].tolist() == [2, 1] and one(5, ref.RAW)["places"].tolist() == [2, 2]
    sp = ref.special_groups(ref.RAW)
    r = one(6, ref.RAW)                                                              # inf -inf nan 0.0 -0.0 -inf inf 3e38 -3e38; targets 1, 4, 6
    assert r["places"].tolist() == [4, 3, 1] and r["hist"][4 + 3] == 1


@pytest.mark.parametrize("mode", [ref.PRINTED, ref.RAW])
def test_one_target_is_the_existing_ranking(shapes, mode):
    """nt = 1 and n <= 4096: places and hist are kprn_host_rank_groups' ranks and hist with pos = the target"""
    c = shapes[mode][0]
    sizes, nts = np.diff(c["group_offsets"]), np.diff(c["target_offsets"])
    gs = np.nonzero((nts == 1) & (sizes <= _ffi.RANK_MAX_GROUP))[0]
    assert len(gs) >= 6
    goff = np.concatenate([[0], np.cumsum(sizes[gs])]).astype(np.int64)
    mem = np.concatenate([c["members"][c["group_offsets"][g]:c["group_offsets"][g + 1]] for g in gs])
    pos = c["targets"][c["target_offsets"][gs]]
    new = _ffi.host_rank_targets(c["scores"], goff, np.arange(len(gs) + 1), pos, members=mem, mode=mode, hist_len=HIST_LEN)
    old = _ffi.host_rank_groups(c["scores"], goff, members=mem, pos=pos, mode=mode, hist_len=HIST_LEN)
    assert np.array_equal(new["places"], old["ranks"]) and np.array_equal(new["hist"], old["hist"])


@pytest.mark.parametrize("mode", [ref.PRINTED, ref.RAW])
def test_each_of_several_targets_is_the_existing_ranking_of_its_own_sample(shapes, mode):
    """a target's place = kprn_host_rank_groups over "the non-targets plus that target, in the original order" with pos = its position there"""
    c, places, _ = shapes[mode]
    sizes, nts = np.diff(c["group_offsets"]), np.diff(c["target_offsets"])
    checked = 0
    for g in np.nonzero((nts >= 2) & (sizes - nts + 1 <= _ffi.RANK_MAX_GROUP) & (sizes > nts))[0]:
        lines = c["members"][c["group_offsets"][g]:c["group_offsets"][g + 1]]
        t = c["targets"][c["target_offsets"][g]:c["target_offsets"][g + 1]]
        is_t = np.zeros(len(lines), bool)
        is_t[t] = True
        some = t[np.unique(np.linspace(0, len(t) - 1, 6).astype(int))]
        mem, pos = [], []
        for i in some:
            keep = ~is_t
            keep[i] = True
            mem.append(lines[keep])
            pos.append(int(keep[:i].sum()))
        goff = np.concatenate([[0], np.cumsum([len(m) for m in mem])]).astype(np.int64)
        old = _ffi.host_rank_groups(c["scores"], goff, members=np.concatenate(mem), pos=np.array(pos, np.int32), mode=mode)
        mine = places[c["target_offsets"][g]:c["target_offsets"][g + 1]][np.searchsorted(t, some)]
        assert np.array_equal(old["ranks"], mine), g
        checked += len(some)
    assert checked > 100


def raw_call(scores, members, goff, toff, targets, G, mode, hist_len, nt_alloc=4):
    """the C entry itself on poisoned outputs -> (status, places, hist)"""
    sc = np.ascontiguousarray(scores, np.float32)
    arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
    places, hist = np.full(nt_alloc, -77, np.int32), np.full(4096 + 4, -77, np.int64)
    mem, goff, toff, tg = arr(members, np.int64), arr(goff, np.int64), arr(toff, np.int64), arr(targets, np.int32)   # (alive through the call)
    rc = _ffi.lib().kprn_host_rank_targets(_ffi._fp(sc), C.c_int64(len(sc)), _ffi._fp(mem), _ffi._fp(goff), _ffi._fp(toff), _ffi._fp(tg), G, mode,
                                           _ffi._fp(places), _ffi._fp(hist), hist_len)
    return rc, places, hist


REFUSALS = [   # (what, members, goff, toff, targets, G, mode, hist_len, status): over scores [10]
    ("decreasing group offsets", None, [0, 5, 3], [0, 1, 2], [0, 0], 2, 0, 15, _ffi.E_ARG),
    ("an empty group", None, [0, 5, 5], [0, 1, 1], [0], 2, 0, 15, _ffi.E_ARG),
    ("a negative first offset", None, [-1, 5], [0, 1], [0], 1, 0, 15, _ffi.E_ARG),
    ("target offsets that do not start at 0", None, [0, 5], [1, 2], [0, 0], 1, 0, 15, _ffi.E_ARG),
    ("decreasing target offsets", None, [0, 5, 10], [0, 2, 1], [0, 1], 2, 0, 15, _ffi.E_ARG),
    ("more targets than members", None, [0, 2, 10], [0, 3, 3], [0, 1, 1], 2, 0, 15, _ffi.E_ARG),
    ("no target at all", None, [0, 5, 10], [0, 0, 0], [0], 2, 0, 15, _ffi.E_ARG),
    ("equal targets", None, [0, 5], [0, 2], [3, 3], 1, 0, 15, _ffi.E_ARG),
    ("descending targets", None, [0, 5], [0, 2], [3, 2], 1, 0, 15, _ffi.E_ARG),
    ("a target past its group", None, [0, 5, 10], [0, 1, 2], [5, 0], 2, 0, 15, _ffi.E_ARG),
    ("a negative target", None, [0, 5], [0, 1], [-1], 1, 0, 15, _ffi.E_ARG),
    ("hist_len 0", None, [0, 5], [0, 1], [0], 1, 0, 0, _ffi.E_ARG),
    ("hist_len 4097", None, [0, 5], [0, 1], [0], 1, 0, 4097, _ffi.E_ARG),
    ("an unknown mode", None, [0, 5], [0, 1], [0], 1, 2, 15, _ffi.E_ARG),
    ("G = 0", None, [0, 5], [0, 1], [0], 0, 0, 15, _ffi.E_ARG),
    ("NULL group offsets", None, None, [0, 1], [0], 1, 0, 15, _ffi.E_ARG),
    ("NULL target offsets", None, [0, 5], None, [0], 1, 0, 15, _ffi.E_ARG),
    ("a run past the scores", None, [0, 5, 11], [0, 1, 2], [0, 0], 2, 0, 15, _ffi.E_INDEX),
    ("a member past the scores", [0, 1, 10], [0, 3], [0, 1], [0], 1, 0, 15, _ffi.E_INDEX),
    ("a negative member", [0, -1, 9], [0, 3], [0, 1], [0], 1, 0, 15, _ffi.E_INDEX),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_refused_call_writes_nothing(case):
    _, members, goff, toff, targets, G, mode, hist_len, status = case
    rc, places, hist = raw_call(np.linspace(0, 1, 10), members, goff, toff, targets, G, mode, hist_len)
    assert rc == status and (places == -77).all() and (hist == -77).all()


def test_the_accepted_neighbours_of_the_refusals():
    rc, places, hist = raw_call(np.linspace(0, 1, 10), [0, 1, 9], [0, 3], [0, 1], [0], 1, 0, 4096)
    assert rc == 0 and places[0] == 2 and (places[1:] == -77).all() and hist[2] == 1 and hist.sum() == 1
    rc, places, hist = raw_call(np.linspace(0, 1, 10), None, [0, 5, 10], [0, 0, 1], [4], 2, 1, 1)
    assert rc == 0 and places[0] == 0 and hist[:5].tolist() == [1, 0, 0, 0, 0] and (hist[5:] == -77).all()
    with pytest.raises(_ffi.KprnError) as ei:                                       # the wrapper refuses what the C call would read past an array for
        _ffi.host_rank_targets(np.zeros(4, np.float32), [0, 4], [0, 2], [1])
    assert ei.value.code == _ffi.E_ARG


# ---- the twin as a stand-alone program under the host sanitizers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def san_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("san") / "rank_targets_san")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "kprn_amd", "csrc"),
           os.path.join(ROOT, "tests", "rank_targets_san_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_san(exe, tmp_path, scores, members, goff, toff, targets, mode, hist_len):
    sc, tg = np.ascontiguousarray(scores, np.float32), np.ascontiguousarray(targets, np.int32)
    goff, toff = np.ascontiguousarray(goff, np.int64), np.ascontiguousarray(toff, np.int64)
    mem = None if members is None else np.ascontiguousarray(members, np.int64)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(sc), len(goff) - 1, -1 if mem is None else len(mem), len(tg), mode, hist_len], np.int64).tobytes())
        for a in (sc, mem, goff, toff, tg):
            if a is not None:
                f.write(a.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    nh = max(hist_len, 0) + 4
    return (int(np.frombuffer(raw[:8], np.int64)[0]), np.frombuffer(raw[8:8 + 4 * len(tg)], np.int32),
            np.frombuffer(raw[8 + 4 * len(tg):8 + 4 * len(tg) + 8 * nh], np.int64))


@pytest.mark.parametrize("mode", [ref.PRINTED, ref.RAW])
def test_sanitized_twin_on_the_shape_list(shapes, san_program, tmp_path, mode):
    c, places, hist = shapes[mode]
    rc, got_places, got_hist = run_san(san_program, tmp_path, c["scores"], c["members"], c["group_offsets"], c["target_offsets"], c["targets"], mode, HIST_LEN)
    assert rc == 0 and np.array_equal(got_places, places) and np.array_equal(got_hist, hist)
    c = ref.consecutive_cases(mode)
    want = ref.reference(c["scores"], c["group_offsets"], c["target_offsets"], c["targets"], None, mode, 1)
    rc, got_places, got_hist = run_san(san_program, tmp_path, c["scores"], None, c["group_offsets"], c["target_offsets"], c["targets"], mode, 1)
    assert rc == 0 and np.array_equal(got_places, want[0]) and np.array_equal(got_hist, want[1])


def test_sanitized_twin_refuses_cleanly(san_program, tmp_path):
    for _, members, goff, toff, targets, G, mode, hist_len, status in REFUSALS:
        if goff is None or toff is None or G != len(goff) - 1:
            continue                                                                  # (the program takes G from the offsets' length)
        rc, places, hist = run_san(san_program, tmp_path, np.linspace(0, 1, 10), members, goff, toff, targets, mode, hist_len)
        assert rc == status and (places == -77).all() and (hist == -77).all()


# ---- KnowledgeGraph.holdout ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph_d():
    g, items, users = tref.graph_d()
    kg = kgraph.KnowledgeGraph(g["src"], g["dst"], g["rel"], pref.node_types(g, 1), pref.END_REL, pref.VR, pref.VT)
    kg.relation_id = lambda name: {"rate": 1, "_rate": 2, "also": 3, "_also": 4}[name]   # graph D has no vocabulary files: relation 1 is the rating
    return g, kg


def edge_multiset(kg):
    rows, counts = np.unique(np.stack([kg.src, kg.dst, kg.rel], axis=1), axis=0, return_counts=True)
    return {tuple(int(x) for x in r): int(c) for r, c in zip(rows, counts)}


@pytest.mark.parametrize("fraction,seed", [(0.8, 1), (0.5, 2), (0.05, 3)])
def test_holdout(graph_d, fraction, seed):
    g, kg = graph_d
    pos = kg.interactions("rate")
    train, held = kg.holdout("rate", fraction, seed)
    train.relation_id = kg.relation_id
    # the split restated: the reference's shuffle, and the users it would leave without a train pair
    perm = np.random.RandomState(seed).permutation(len(pos))
    first = set(map(tuple, pos[perm[:int(len(pos) * fraction)]].tolist()))
    users_kept = {u for u, _ in first}
    back = [tuple(p) for p in pos.tolist() if tuple(p) not in first and p[0] not in users_kept]
    assert (fraction > 0.05) or len(back) > 0                                          # at 5 % some user loses everything, and gets it back
    train_pairs = train.interactions("rate")
    assert len(train_pairs) == int(len(pos) * fraction) + len(back) and len(held) == len(pos) - len(train_pairs)
    assert set(map(tuple, train_pairs.tolist())) == first | set(back)
    assert np.array_equal(held, held[np.lexsort((held[:, 1], held[:, 0]))]) and held.dtype == np.int32
    assert set(held[:, 0].tolist()) <= set(train_pairs[:, 0].tolist())               # every held user keeps a train pair
    # no held pair is adjacent in the train graph, under any relation and in either direction
    adjacent = set(zip(train.src.tolist(), train.dst.tolist())) | set(zip(train.dst.tolist(), train.src.tolist()))
    held_set = set(map(tuple, held.tolist()))
    assert not (held_set & adjacent)
    doubled = [(s, d) for (s, d, r) in edge_multiset(kg) if r == 3 and (s, d) in held_set]
    assert fraction == 0.05 or len(doubled) > 0                                      # graph D's second relation: "the relation's edge and its inverse" would leave these
    # every other edge survives with its multiplicity
    want = {e: c for e, c in edge_multiset(kg).items() if (e[0], e[1]) not in held_set and (e[1], e[0]) not in held_set}
    assert edge_multiset(train) == want
    assert (train.Ve, train.Vr, train.Vt, train.end_relation) == (kg.Ve, kg.Vr, kg.Vt, kg.end_relation) and np.array_equal(train.node_types, kg.node_types)
    # the same seed gives the same split, another seed another
    again, held2 = kg.holdout("rate", fraction, seed)
    assert np.array_equal(held, held2) and np.array_equal(again.src, train.src) and np.array_equal(again.dst, train.dst) and np.array_equal(again.rel, train.rel)
    assert not np.array_equal(kg.holdout("rate", fraction, seed + 1)[1], held)


def test_holdout_of_nothing(graph_d):
    g, kg = graph_d
    train, held = kg.holdout("rate", 1.0, 1)
    assert held.shape == (0, 2) and np.array_equal(train.src, kg.src) and np.array_equal(train.dst, kg.dst) and np.array_equal(train.rel, kg.rel)
    with pytest.raises(ValueError):
        kg.holdout("rate", 1.5)
