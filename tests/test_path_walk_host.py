"""not gpu: kprn_host_find_paths_sampled, the host twin of the sampled hops (include/kprn.h "sampled paths of four and five hops"), against the brute-force
restatement in tests/path_walk_ref.py; the figures its inputs were chosen for; its refusals; the -walks flag.  Every comparison is exact."""
import itertools

import numpy as np
import pytest

from kprn_amd import _ffi, model

from . import path_find_ref as ref
from . import path_walk_ref as wr

HOPS = [(4, 4), (5, 5), (4, 5), (1, 5), (2, 4)]
CAPS = [1, 7, 28, 4096]
WALKS = [1, 3, 64, 256]
LAYOUTS = list(itertools.product([6, 7], [0, 1], [1, 2], [1, 4]))       # T, F - (num_types + 2), num_types, threads


@pytest.fixture(scope="module")
def inputs():
    return wr.make_inputs()


@pytest.fixture(scope="module")
def memo():
    return {}


def twin(g, nt, pairs, lo, hi, cap, T, walks, seed, draw, **kw):
    return _ffi.host_find_paths_sampled(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, T, walks, seed, draw, **kw)


def test_new_symbols_are_declared_and_exported():
    import subprocess
    from kprn_amd import build as kbuild
    declared = _ffi.declared_symbols()
    syms = subprocess.check_output(["nm", "-D", kbuild.build()]).decode()
    for s in ("kprn_find_paths_sampled", "kprn_host_find_paths_sampled", "kprn_find_training_paths_sampled"):
        assert s in declared, s
        assert " T %s" % s in syms, s


def test_philox_known_answer():
    assert wr.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)


def test_inputs_hold_every_case(inputs):
    """the figures the inputs were chosen for, re-derived from the brute force (walks 64, seed 1, draw 0), and the conditions the comparisons rely on"""
    g, pairs = inputs
    assert len(pairs) == 71
    st, n4, n5, per_pair, per_walk = {}, 0, 0, [], []
    for b, (u, i) in enumerate(pairs[:70]):
        walks = [wr.walk_paths(g, int(u), int(i), b, h, wr.WALKS, wr.SEED, wr.DRAW, st) for h in (4, 5)]
        c4, c5 = (sum(len(p) for p in w) for w in walks)
        n4 += c4 > 0
        n5 += c5 > 0
        per_pair.append(c4 + c5)
        per_walk.append([len(p) for p in walks[0] + walks[1]])
    assert (n4, n5, sum(per_pair), max(per_pair), sum(c > 7 for c in per_pair)) == (34, 48, 593, 235, 9)
    assert (st["dup"], st["dead_rep"], st["dead_deg"], st["multi"]) == (3155, 538, 1497, 124)
    assert n4 >= 20 and n5 >= 20 and st["dup"] >= 1 and st["dead_rep"] >= 1 and st["dead_deg"] >= 1
    per_walk.append([len(p) for h in (4, 5) for p in wr.walk_paths(g, int(pairs[70][0]), int(pairs[70][1]), 70, h, wr.WALKS, wr.SEED, wr.DRAW)])
    for lo, cap in ((1, 7), (1, 28), (4, 7), (4, 28)):                 # the cap falls inside a walk's paths, at every hop range and cap the GPU test runs
        inside = []
        for b, lens in enumerate(per_walk):
            run = np.cumsum([len(ref.brute_paths(g, int(pairs[b][0]), int(pairs[b][1]), 1, 3)) if lo == 1 else 0] + lens)
            inside += [b for r0, r1 in zip(run[:-1], run[1:]) if r0 < cap < r1]
        assert inside and ((lo, cap) != (4, 28) or min(inside) < 70), (lo, cap)
    assert st["wide"] <= 64                                            # rows 0..69 alone never close over more than a wave's lanes ...
    st70 = {}
    u, i = (int(x) for x in pairs[70])
    paths = wr.walk_paths(g, u, i, 70, 4, wr.WALKS, wr.SEED, wr.DRAW, st70)
    assert st70["wide"] > 256 and max(len(p) for p in paths) > 64      # ... row 70 closes over the hub's edges: several chunks of 64, paths in more than one


@pytest.mark.parametrize("hops", HOPS)
def test_twin_equals_brute_force(inputs, memo, hops):
    g, pairs = inputs
    lo, hi = hops
    nts = {n: ref.node_types(g, n) for n in (1, 2)}
    layouts = itertools.cycle(LAYOUTS)
    for walks in WALKS:
        for cap in CAPS:
            for T, lead, num_types, threads in itertools.islice(layouts, 3):      # the 16 layouts in turn: three times each per hop range
                F = num_types + 2 + lead
                want = wr.brute_find(g, nts[num_types], pairs, lo, hi, cap, T, F, walks, wr.SEED, wr.DRAW, memo)
                got = twin(g, nts[num_types], pairs, lo, hi, cap, T, walks, wr.SEED, wr.DRAW, F=F, threads=threads)
                what = (walks, cap, T, F, num_types, threads)
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
                assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), what
    assert want[2].sum() > 0


@pytest.mark.parametrize("T,lead,num_types,threads", LAYOUTS)
def test_twin_equals_brute_force_in_every_layout(inputs, memo, T, lead, num_types, threads):
    g, pairs = inputs
    nt = ref.node_types(g, num_types)
    F = num_types + 2 + lead
    for cap in (7, 4096):
        want = wr.brute_find(g, nt, pairs, 1, 5, cap, T, F, wr.WALKS, wr.SEED, wr.DRAW, memo)
        got = twin(g, nt, pairs, 1, 5, cap, T, wr.WALKS, wr.SEED, wr.DRAW, F=F, threads=threads)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), cap
    assert {len([s for s in row if s[-2] != g["Ve"]]) - 1 for row in want[0]} == {1, 2, 3, 4, 5}      # (cap 4096) rows of every hop count


def test_three_hops_or_fewer_is_the_unsampled_call(inputs):
    g, pairs = inputs
    nt = ref.node_types(g, 1)
    for lo, hi, cap in ((1, 3, 7), (2, 3, 4096), (1, 1, 5)):
        want = _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, lo, hi, cap, wr.T)
        for walks, seed, draw in ((0, 0, 0), (64, 1, 0), (256, 0xDEADBEEF12345678, 9), (257, 5, 5), (-1, 1, 1)):
            got = twin(g, nt, pairs, lo, hi, cap, wr.T, walks, seed, draw)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (lo, hi, walks)


def test_seed_draw_and_row_address_the_walks(inputs):
    g, pairs = inputs
    nt = ref.node_types(g, 1)
    run = lambda pr, seed, draw: twin(g, nt, pr, 4, 5, 28, wr.T, wr.WALKS, seed, draw)
    base, again = run(pairs, 1, 0), run(pairs, 1, 0)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    for seed, draw in ((2, 0), (1, 1), (1 + (1 << 32), 0)):           # (the seed's high half is part of the key)
        other = run(pairs, seed, draw)
        assert other[0].shape != base[0].shape or not np.array_equal(other[0], base[0]), (seed, draw)
    # the same pair in two rows draws different walks
    b = int(np.argmax(base[2]))
    idx, counts, found = run(np.stack([pairs[b]] * 4), 1, 0)
    off = np.concatenate([[0], np.cumsum(counts)])
    rows = [idx[off[k]:off[k + 1]].tobytes() for k in range(4)]
    assert counts.min() > 0 and len(set(rows)) > 1


def test_refusals_write_nothing(inputs):
    g, pairs = inputs
    nt = ref.node_types(g, 1)
    L = _ffi.lib()
    C = _ffi.C
    src, dst, rel = (np.ascontiguousarray(g[k], np.int32) for k in ("src", "dst", "rel"))
    B = len(pairs)

    def call(lo, hi, cap, T, walks):
        counts, found, idx = np.full(B, -7, np.int32), np.full(B, -7, np.int64), np.full((64, T, 3), -7, np.int32)
        rc = L.kprn_host_find_paths_sampled(_ffi._fp(src), _ffi._fp(dst), _ffi._fp(rel), C.c_int64(len(src)), _ffi._fp(nt), g["Ve"], ref.VR, ref.VT, 1, ref.END_REL,
                                            _ffi._fp(pairs), B, lo, hi, cap, T, 3, walks, C.c_uint64(1), C.c_uint32(0), 2, _ffi._fp(counts), _ffi._fp(found),
                                            _ffi._fp(idx))
        return rc, (counts == -7).all() and (found == -7).all() and (idx == -7).all()

    assert call(1, 5, 1, 6, 64)[0] == 0
    for lo, hi, cap, T, walks in ((1, 6, 7, 7, 64), (1, 5, 7, 6, 0), (1, 4, 7, 6, 0), (1, 5, 7, 6, 257), (4, 4, 7, 6, -1), (1, 5, 7, 5, 64), (1, 4, 7, 4, 64),
                                  (5, 4, 7, 6, 64), (0, 5, 7, 6, 64), (1, 5, 0, 6, 64), (1, 5, 4097, 6, 64)):
        rc, untouched = call(lo, hi, cap, T, walks)
        assert rc == _ffi.E_ARG and untouched, (lo, hi, cap, T, walks)
    # the unsampled twin keeps refusing more than three hops
    with pytest.raises(_ffi.KprnError) as ei:
        _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, 1, 4, 7, 6)
    assert ei.value.code == _ffi.E_ARG


def test_flag_parsing(capsys):
    p = model.parse_flags(["-max_hops", "5", "-walks", "64"])
    assert (p.max_hops, p.walks) == (5, 64)
    p = model.parse_flags([])
    assert (p.max_hops, p.walks) == (3, 0)
    assert model.parse_flags(["-max_hops", "2", "-walks", "0"]).walks == 0
    for flags in (["-max_hops", "5"], ["-max_hops", "4", "-walks", "0"], ["-max_hops", "5", "-walks", "257"], ["-max_hops", "6", "-walks", "64"]):
        with pytest.raises(SystemExit) as ei:
            model.parse_flags(flags)
        assert ei.value.code != 0
        err = capsys.readouterr().err
        assert ("-walks" in err) if flags[1] != "6" else ("-max_hops" in err), flags


def test_recommend_command_line_names_the_missing_flag(capsys):
    from kprn_amd import recommend
    with pytest.raises(SystemExit) as ei:
        recommend.main(["-kg", "none.tsv", "-vocab_dir", "none", "-user", "u0", "-items", "none.txt", "-max_hops", "5"])
    assert ei.value.code != 0 and "-walks" in capsys.readouterr().err
