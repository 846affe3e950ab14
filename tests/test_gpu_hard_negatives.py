"""gpu: hard negatives (include/kprn.h "hard negatives") -- kprn_select_hardest against its host twin (itself held to a numpy restatement by
tests/test_select_hardest_host.py), kprn_batch_subset against the source batch's rows and against the same batch built from the host, the kept rows against
the rows that were scored, and the loop of graph.train_from_graph(neg_pool=...) against the hand-written composition.  Every comparison of ids, masks, losses
and parameters is np.array_equal / ==."""
import io
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from kprn_amd import _ffi, graph as kgraph

from . import path_find_ref as ref
from . import select_hardest_ref as sref
from .test_gpu_path_find import SHAPES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VE = 500


# ---- 1. the selection on the device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board():
    """a small engine whose board holds the group set's scores"""
    sc, goff, pos = sref.group_set()
    eng = _ffi.Engine(ref.VT, VE, ref.VR, **SHAPES[4])
    with pytest.raises(_ffi.KprnError) as ei:                       # no board yet
        eng.select_hardest(goff, 2, pos=pos)
    assert ei.value.code == _ffi.E_ARG
    eng.board_reserve(len(sc) + 10)                                 # (the last 10 lines stay NaN: entries nothing wrote)
    eng.board_write(0, sc)
    yield eng, sc, goff, pos
    eng.close()


@pytest.mark.parametrize("n_keep", [1, 4, 64, 65, 256])
def test_device_equals_twin_bit_for_bit(board, n_keep):
    """both size classes in ONE call (a wave per group up to 256 members, a workgroup above), with and without positives, and the same result twice"""
    eng, sc, goff, pos = board
    assert (np.diff(goff) <= 256).any() and (np.diff(goff) > 256).any()
    for p in (pos, None):
        want, want_inv = _ffi.host_select_hardest(sc, goff, n_keep, pos=p)
        got, got_inv = eng.select_hardest(goff, n_keep, pos=p)
        assert np.array_equal(got, want) and got_inv == want_inv and want_inv > 0
        again, again_inv = eng.select_hardest(goff, n_keep, pos=p)
        assert np.array_equal(again, got) and again_inv == got_inv
    # a run of groups that starts inside the board: nothing below group_offsets[0] is written
    keep = np.full(int(goff[-1]), 9, np.uint8)
    got, _ = eng.select_hardest(goff[5:], n_keep, pos=pos[5:], keep=keep)
    want, _ = _ffi.host_select_hardest(sc, goff[5:], n_keep, pos=pos[5:], keep=np.full(int(goff[-1]), 9, np.uint8))
    assert np.array_equal(got, want) and (got[:goff[5]] == 9).all()


def test_members_repeated_lines_and_unwritten_entries(board):
    eng, sc, goff, pos = board
    rng = np.random.RandomState(4)
    n = len(sc)
    full = np.concatenate([sc, np.full(10, np.nan, np.float32)])
    members = np.concatenate([[7, 7, 3, 7, n + 2], rng.randint(0, n + 10, 300), rng.randint(0, n, 2000), [n + 9, 0]]).astype(np.int64)
    mgoff = np.array([0, 5, 305, 2305, 2307], np.int64)
    mpos = np.array([1, 17, 1999, -1], np.int32)
    for n_keep in (1, 3, 200):
        want, want_inv = _ffi.host_select_hardest(full, mgoff, n_keep, members=members, pos=mpos)
        got, got_inv = eng.select_hardest(mgoff, n_keep, members=members, pos=mpos)
        assert np.array_equal(got, want) and got_inv == want_inv and got_inv >= 2
    got, _ = eng.select_hardest(mgoff[1:], 3, members=members, pos=mpos[1:], keep=np.full(2307, 9, np.uint8))   # a slice of the member table
    assert (got[:5] == 9).all() and np.array_equal(got[5:], _ffi.host_select_hardest(full, mgoff, 3, members=members, pos=mpos)[0][5:])


def test_device_refusals_write_nothing(board):
    eng, sc, goff, pos = board
    n = len(sc) + 10
    C, fp = _ffi.C, _ffi._fp
    i64, i32 = (lambda *v: np.array(v, np.int64)), (lambda *v: np.array(v, np.int32))
    mem = np.arange(10, dtype=np.int64)
    cases = [(dict(goff=None), _ffi.E_ARG), (dict(G=0), _ffi.E_ARG), (dict(n_keep=0), _ffi.E_ARG), (dict(n_keep=257), _ffi.E_ARG), (dict(goff=i64(0, 0, 10)), _ffi.E_ARG),
             (dict(goff=i64(0, 3, 4100), members=None), _ffi.E_ARG), (dict(pos=i32(0, 7)), _ffi.E_ARG), (dict(pos=i32(-2, 0)), _ffi.E_ARG),
             (dict(members=i64(0, 1, 2, 3, 4, 5, 6, 7, 8, n)), _ffi.E_INDEX), (dict(members=None, goff=i64(n - 5, n - 2, n + 1), pos=i32(0, 1)), _ffi.E_INDEX), (dict(keep=None), _ffi.E_ARG)]
    for kw, status in cases:
        a = dict(members=mem, goff=i64(0, 3, 10), pos=i32(0, 6), G=2, n_keep=2)
        a.update(kw)
        keep, ninv = np.full(n + 8, 77, np.uint8), np.full(1, -77, np.int64)
        rc = eng.L.kprn_select_hardest(eng.h, fp(a["members"]), fp(a["goff"]), fp(a["pos"]), a["G"], a["n_keep"], None if "keep" in kw else fp(keep), fp(ninv))
        assert rc == status and (keep == 77).all() and ninv[0] == -77, kw
    keep = np.full(10, 77, np.uint8)                                                   # the same arguments, unrefused; n_invalid may be NULL
    assert eng.L.kprn_select_hardest(eng.h, fp(mem), fp(i64(0, 3, 10)), fp(i32(0, 6)), 2, 2, fp(keep), None) == 0
    assert np.array_equal(keep, _ffi.host_select_hardest(sc, [0, 3, 10], 2, members=mem, pos=[0, 6])[0])


# ---- 2. a batch from the kept pairs of a batch ----------------------------------------------------------------------------------------------
COUNTS = np.array([1, 2, 28, 29, 64, 4096, 29, 1, 2, 28, 64], np.int32)   # 1, 2, 28 | 29 (the wave reducer), 64, the most paths a pair may have


def make_source(F, T, seed):
    """random valid ids [N, T, F] for COUNTS (the leading column of F = 4 is one nothing reads), labels 1 / 0"""
    rng = np.random.RandomState(seed)
    N = int(COUNTS.sum())
    idx = np.empty((N, T, F), np.int32)
    idx[:, :, :F - 2] = rng.randint(1, ref.VT + 1, size=(N, T, F - 2))
    idx[:, :, F - 2] = rng.randint(1, VE + 1, size=(N, T))
    idx[:, :, F - 1] = rng.randint(1, ref.VR + 1, size=(N, T))
    return idx, (np.arange(len(COUNTS)) % 3 == 0).astype(np.float32)


def masks(B):
    one = np.zeros(B, np.uint8); one[5 % B] = 1
    first = np.ones(B, np.uint8); first[0] = 0
    last = np.ones(B, np.uint8); last[-1] = 0
    return dict(all=np.ones(B, np.uint8), one=one, first_dropped=first, last_dropped=last, alternating=(np.arange(B) % 2).astype(np.uint8))


def rows_of_kept(idx, counts, keep):
    off = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    return np.concatenate([idx[off[b]:off[b + 1]] for b in range(len(counts)) if keep[b]])


def run_subset_cases(F, T):
    """every mask on a ragged and on a rectangular source: ids, counts, path count; on the D = H = 64 shape (F = 3) under "deterministic" = 1 the subset
    batch against the same batch built from the host: loss and flat gradients of one backward bit for bit; the source scores to the same bits afterwards"""
    eng = _ffi.Engine(ref.VT, VE, ref.VR, seed=3, **SHAPES[F])
    if F == 3:
        eng.set_option("deterministic", "1")
    idx, labels = make_source(F, T, 11 + F)
    assert (T * F) % 4 != 0 or F == 4
    ragged = eng.batch_ragged(idx, COUNTS, labels)
    P = 3
    rect_idx = idx[:len(COUNTS) * P].reshape(len(COUNTS), P, T, F)
    rect = eng.batch(rect_idx, labels)
    bare = eng.batch_ragged(idx, COUNTS)                                              # no labels in, none out
    sources = dict(ragged=(ragged, idx, COUNTS), rect=(rect, rect_idx.reshape(-1, T, F), np.full(len(COUNTS), P, np.int32)))
    probs0 = {k: eng.forward(v[0], 1)["probs"].copy() for k, v in sources.items()}
    for name, (src, rows, counts) in sources.items():
        assert eng.batch_subset(src, np.zeros(src.B, np.uint8)) is None               # nothing kept
        for mname, keep in masks(src.B).items():
            sub = eng.batch_subset(src, keep)
            want = rows_of_kept(rows, counts, keep)
            assert sub.B == int(keep.sum()) and np.array_equal(sub.counts, counts[keep != 0]) and sub.n_paths == len(want) and sub.has_labels, (name, mname)
            assert np.array_equal(sub.read_idx(), want), (name, mname)
            if F == 3:
                host = eng.batch_ragged(want, counts[keep != 0], labels[keep != 0])
                la = eng.backward(sub, 1); ga = eng.get_flat_grads()
                lb = eng.backward(host, 1); gb = eng.get_flat_grads()
                assert np.isfinite(la) and la == lb and ga.tobytes() == gb.tobytes() and np.abs(ga).max() > 0, (name, mname)
                host.free()
            else:
                assert np.isfinite(eng.backward(sub, 1))
            sub.free()
        assert np.array_equal(src.read_idx(), rows)                                   # the source is as it was ...
        assert eng.forward(src, 1)["probs"].tobytes() == probs0[name].tobytes()       # ... and scores to the same bits
    sub = eng.batch_subset(bare, masks(bare.B)["alternating"])
    assert not sub.has_labels and np.array_equal(sub.read_idx(), rows_of_kept(idx, COUNTS, masks(bare.B)["alternating"]))
    assert np.isfinite(eng.forward(sub, 1)["probs"]).all()
    with pytest.raises(_ffi.KprnError) as ei:                                         # one keep entry per pair
        eng.batch_subset(bare, np.ones(3, np.uint8))
    assert ei.value.code == _ffi.E_ARG
    # a fed slot nobody used yet is waited for; a source with an id out of range is KPRN_E_INDEX
    fed = _ffi.Batch.ragged(eng, idx, COUNTS, labels, feed=True)
    sub2 = eng.batch_subset(fed, masks(fed.B)["first_dropped"])
    assert np.array_equal(sub2.read_idx(), rows_of_kept(idx, COUNTS, masks(fed.B)["first_dropped"]))
    bad_idx = idx.copy(); bad_idx[7, 0, F - 2] = VE + 1
    bad = _ffi.Batch.ragged(eng, bad_idx, COUNTS, labels, feed=True)
    with pytest.raises(_ffi.KprnError) as ei:
        eng.batch_subset(bad, np.ones(bad.B, np.uint8))
    assert ei.value.code == _ffi.E_INDEX
    eng.close()


@pytest.mark.parametrize("F,T", [(3, 5), (4, 4)])
def test_subset(F, T):
    run_subset_cases(F, T)


def test_subset_does_not_depend_on_what_hipmalloc_returns():
    """the same cases in a fresh process with KPRN_POISON_ALLOC=1 (every new device allocation filled with 0xFF bytes)"""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        from tests.test_gpu_hard_negatives import run_subset_cases
        run_subset_cases(3, 5)
        run_subset_cases(4, 4)
        print("subset cases passed")
    """) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=300)
    assert r.returncode == 0 and "subset cases passed" in r.stdout, r.stderr[-3000:]


# ---- 3. the kept rows are the scored rows ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    return ref.make_graph(n_rand=N_RAND, n_rand_edges=400, seed=31)   # dense: five edges a node, so most pairs have paths of 2 .. 4 hops


@pytest.fixture(scope="module")
def nt(g):
    return ref.node_types(g, 1)


N_RAND = 80
ITEMS = np.arange(1, N_RAND + 1, dtype=np.int32)
WEIGHTS = ((np.arange(N_RAND) + 10.0) ** -0.8).astype(np.float32)


def positives_of(g):
    """21 positives: two planted pairs, the node without an edge (a group in which no pair has a path), 18 random pairs (some without a path of their own)"""
    c = g["cases"]
    rng = np.random.RandomState(3)
    return np.array([c["exact"], c["inside"], c["lonely"]] + [tuple(int(x) for x in rng.randint(1, N_RAND + 1, size=2)) for _ in range(18)], np.int32)


def per_pair(idx, counts):
    off = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    return [idx[off[b]:off[b + 1]] for b in range(len(counts))]


@pytest.mark.parametrize("mode", ["walks", "spread"])
def test_the_kept_rows_are_the_scored_rows(g, nt, mode):
    """-walks 8 -max_hops 4, and path_cap spread: the draws are addressed by the pair-list row, so a second find call on the kept pair list returns other paths
    than the pool batch's for some pair -- the subset returns the pool batch's"""
    walks, max_hops, T, cap, max_paths = (8, 4, 5, "first", 28) if mode == "walks" else (0, 3, 4, "spread", 3)
    seed, draw, pool = 7, 2, 8
    pos = positives_of(g)[3:8]
    neg, _ = _ffi.host_sample_negatives(g["src"], g["dst"], g["rel"], g["Ve"], ITEMS, WEIGHTS, pos[:, 0], pool, seed, draw, max_attempts=16, threads=8)
    assert (neg > 0).all()                                                            # no empty slot: the pair list's rows are the finder's rows
    prs = np.zeros((len(pos), 1 + pool, 2), np.int32)
    prs[:, :, 0] = pos[:, :1]; prs[:, 0, 1] = pos[:, 1]; prs[:, 1:, 1] = neg
    prs = prs.reshape(-1, 2)
    find = lambda pairs: _ffi.host_find_paths_cap(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, pairs, 2, max_hops, max_paths, T, walks, seed, draw,
                                                  cap=cap, threads=8)
    # on the host twins first: the fixture has a kept pair whose paths differ between the pool's row and the kept list's row
    idx, counts, _ = find(prs)
    has = counts > 0
    keep_rows = has & ((np.arange(len(prs)) % (1 + pool) == 0) | (np.arange(len(prs)) % 3 == 1))   # every positive, a third of the negatives
    keep_rows[np.nonzero(has)[0][0]] = False                                          # (the first pair goes, so every kept pair moves to another row)
    idx2, counts2, _ = find(prs[keep_rows])
    pool_rows = dict(zip(np.nonzero(has)[0].tolist(), per_pair(idx, counts[has])))
    second = per_pair(idx2, counts2[counts2 > 0])
    kept_list = [r for r in np.nonzero(keep_rows)[0].tolist()]
    differ = [r for r, rows2 in zip([r for r, c in zip(kept_list, counts2) if c > 0], second)
              if rows2.shape != pool_rows[r].shape or not np.array_equal(rows2, pool_rows[r])]
    assert differ, "the fixture has no pair whose paths depend on its row"
    # the device
    eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, seed=77, **SHAPES[3])
    eng.set_option("path_cap", cap)
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
    s = eng.sampler(ITEMS, WEIGHTS)
    batch, got_prs, got_counts, _ = eng.find_training_paths(gr, s, pos, pool, seed, draw, 2, max_hops, max_paths, T, max_attempts=16, walks=walks)
    assert np.array_equal(got_prs, prs) and np.array_equal(got_counts, counts) and np.array_equal(batch.read_idx(), idx)
    sub = eng.batch_subset(batch, keep_rows[has])
    want = np.concatenate([pool_rows[r] for r in kept_list])
    assert np.array_equal(sub.read_idx(), want) and np.array_equal(sub.counts, counts[keep_rows])
    again, c2, _ = eng.find_paths(gr, prs[keep_rows], 2, max_hops, max_paths, T, walks=walks, seed=seed, draw=draw)
    assert np.array_equal(c2, counts2) and np.array_equal(again.read_idx(), idx2)
    assert again.read_idx().shape != want.shape or not np.array_equal(again.read_idx(), want)
    for b in (batch, sub, again):
        b.free()
    eng.close()


# ---- 4. the loop ----------------------------------------------------------------------------------------------------------------------------
def fresh(g, nt):
    eng = _ffi.Engine(ref.VT, g["Ve"], ref.VR, seed=77, **SHAPES[3])
    eng.set_option("deterministic", "1")
    gr = eng.graph(g["src"], g["dst"], g["rel"], nt, ref.END_REL)
    return eng, gr, eng.sampler(ITEMS, WEIGHTS)


@pytest.mark.parametrize("loss", ["bce", "bpr"])
def test_training_loop_with_a_pool_equals_the_hand_written_composition(g, nt, loss):
    """three steps with "deterministic" = 1: graph.train_from_graph(neg_pool=8, n_neg=2) on one engine; on another, written out here: host sampling twin ->
    host finder twin -> the pool batch scored on the device, its scores read back -> host selection twin -> batch_ragged of the kept rows -> train_step"""
    pos = positives_of(g)                                                             # three minibatches of 7
    seed, n_neg, pool, mb = 5, 2, 8, 7
    opt = _ffi.make_opt(method=1, lr=2e-3)
    a, gra, sa = fresh(g, nt)
    stats = {}
    hist = kgraph.train_from_graph(a, gra, pos, opt, mb, n_neg, 1, seed, sampler=sa, max_attempts=8, max_paths=7, out=io.StringIO(), stats=stats, loss=loss,
                                   neg_pool=pool)
    assert stats["steps"] == 3 and stats["skipped"] == 0 and len(hist) == 1 and np.isfinite(hist[0]) and a.options["loss"] == "bce"
    b, _, _ = fresh(g, nt)
    b.set_option("loss", loss)
    b.set_option("loss_accumulate", "1")
    b.loss_sum(reset=True)
    order = np.random.RandomState(seed + 1).permutation(len(pos))
    pool_pairs = kept_pairs = 0
    seen = dict(empty=0, no_positive=0, cut=0)
    for step in range(3):
        p = pos[order[step * mb:(step + 1) * mb]]
        neg, _ = _ffi.host_sample_negatives(g["src"], g["dst"], g["rel"], g["Ve"], ITEMS, WEIGHTS, p[:, 0], pool, seed, step, max_attempts=8, threads=8)
        prs = np.zeros((len(p), 1 + pool, 2), np.int32)
        prs[:, :, 0] = p[:, :1]; prs[:, 0, 1] = p[:, 1]; prs[:, 1:, 1] = neg
        prs = prs.reshape(-1, 2)
        labels = (np.arange(len(prs)) % (1 + pool) == 0).astype(np.float32)
        real = prs[:, 1] != 0
        idx, c, _ = _ffi.host_find_paths(g["src"], g["dst"], g["rel"], nt, ref.VR, ref.VT, ref.END_REL, prs[real], 2, 3, 7, 4, threads=8)
        counts = np.zeros(len(prs), np.int32)
        counts[real] = c
        has = counts > 0
        batch = b.batch_ragged(idx, counts[has], labels[has])
        b.forward_async(batch, 1)
        scores = b.read_probs(batch.B)
        batch.free()
        goff = kgraph.groups_from_counts(counts, pool).astype(np.int64)
        gpos = np.where(counts.reshape(-1, 1 + pool)[:, 0] > 0, 0, -1).astype(np.int32)
        full = np.diff(goff) > 0                                                      # (a group none of whose pairs has a path is no group of the call)
        seen["empty"] += int((~full).sum()); seen["no_positive"] += int((gpos[full] < 0).sum()); seen["cut"] += int((np.diff(goff) - (gpos >= 0) > n_neg).sum())
        keep, inv = _ffi.host_select_hardest(scores, goff[np.concatenate([[True], full])], n_neg, pos=gpos[full])
        assert inv == 0
        lab = labels[has]
        for k in range(len(goff) - 1):                                                # the kept negatives are the group's hardest
            sl = slice(int(goff[k]), int(goff[k + 1]))
            negs = lab[sl] == 0
            kn, dn = scores[sl][negs & (keep[sl] == 1)], scores[sl][negs & (keep[sl] == 0)]
            assert len(kn) == min(n_neg, int(negs.sum())) and (len(dn) == 0 or kn.min() >= dn.max()), (step, k)
        assert (keep[lab == 1] == 1).all() and keep.sum() < len(keep)
        kept = b.batch_ragged(rows_of_kept(idx, counts[has], keep), counts[has][keep == 1], lab[keep == 1])
        if loss == "bpr":
            upto = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
            assert kept.set_groups(upto[goff].astype(np.int32)) > 0
        b.train_step(kept, opt, want_loss=False)
        pool_pairs += int(has.sum()); kept_pairs += kept.B
        kept.free()
    total, n = b.loss_sum(reset=True)
    print(f"{loss}: trainer's epoch average {hist[0]!r}, composition {total / 3!r}; pairs scored {pool_pairs}, trained on {kept_pairs}")
    assert n == 3 and hist[0] == total / 3
    assert seen["empty"] > 0 and seen["no_positive"] > 0 and seen["cut"] >= 10, seen
    assert stats["pool_pairs"] == pool_pairs and stats["kept_pairs"] == kept_pairs == stats["pairs"]
    ta, tb = a.get_flat_params(), b.get_flat_params()
    assert ta.tobytes() == tb.tobytes() and np.isfinite(ta).all()
    for k in (0, 1):
        assert a.get_flat_opt_state(k).tobytes() == b.get_flat_opt_state(k).tobytes()
    for e in (a, b):
        e.close()


def test_no_pool_and_a_pool_of_n_neg_are_todays_step(g, nt):
    pos = positives_of(g)                                                             # three minibatches of 7
    opt = _ffi.make_opt(method=1, lr=2e-3)
    runs = []
    for kw in (dict(), dict(neg_pool=0), dict(neg_pool=2)):
        eng, gr, s = fresh(g, nt)
        stats = {}
        hist = kgraph.train_from_graph(eng, gr, pos, opt, 7, 2, 1, 5, sampler=s, max_attempts=8, max_paths=7, out=io.StringIO(), stats=stats, **kw)
        assert sorted(stats) == ["pairs", "skipped", "steps"] and stats["steps"] == 3
        runs.append((hist, eng.get_flat_params().tobytes()))
        eng.close()
    assert runs[0] == runs[1] == runs[2] and np.isfinite(runs[0][0][0])
    eng, gr, s = fresh(g, nt)
    for bad in (1, 257, -1):
        with pytest.raises(ValueError):
            kgraph.train_from_graph(eng, gr, pos, opt, 7, 2, 1, 5, sampler=s, out=io.StringIO(), neg_pool=bad)
    eng.close()


def test_train_command_line_with_neg_pool(tmp_path, capsys):
    """python -m kprn_amd.train -kg ... -neg_pool 4 (called in-process, the small graph of tests/test_gpu_neg_sample.py's command-line test), and every
    -neg_pool usage error"""
    from kprn_amd import train
    from kprn_amd.pathformat import Vocabs
    from .test_path_find_host import _write_vocab
    vdir = tmp_path / "vocab"
    vdir.mkdir()
    _write_vocab(str(vdir))
    triples = []
    for u, m in [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 0), (3, 4), (1, 4)]:
        triples += [("u%d" % u, "rate", "m%d" % m), ("m%d" % m, "_rate", "u%d" % u)]
    for m in (1, 2, 4):
        triples += [("m%d" % m, "act", "a0"), ("a0", "_act", "m%d" % m)]
    (tmp_path / "kg.tsv").write_text("".join("%s\t%s\t%s\n" % t for t in triples))
    kg = kgraph.KnowledgeGraph.from_triples(triples, Vocabs(str(vdir)), 1)
    shape = ["-entityTypeVocabSize", kg.Vt, "-entityVocabSize", kg.Ve, "-relationVocabSize", kg.Vr, "-entityTypeEmbeddingDim", 16, "-entityEmbeddingDim", 32,
             "-relationEmbeddingDim", 16, "-rnnHidSize", 64, "-numLayers", 2, "-numFeatureTemplates", 3, "-numEntityTypes", 1, "-rnnType", "lstm",
             "-includeEntity", 1, "-gpuid", 0, "-numEpochs", 2, "-minibatch", 4, "-useAdam", 1, "-topK", 2, "-negatives", 2, "-sampleSeed", 3]
    from_kg = ["-kg", tmp_path / "kg.tsv", "-vocab_dir", vdir, "-interaction_rel", "rate"]
    losses = {}
    for name, extra in (("pool", ["-neg_pool", 4]), ("plain", [])):
        assert train.main([str(f) for f in shape + from_kg + extra]) == 0
        lines = capsys.readouterr().out.splitlines()
        head = [l for l in lines if l.startswith("Training from the graph")]
        assert len(head) == 1 and ("pool of 4" in head[0]) == (name == "pool") and "2 negatives each" in head[0], head
        losses[name] = [float(l.split("=")[1]) for l in lines if l.startswith("avg loss in epoch")]
        assert len(losses[name]) == 2 and all(np.isfinite(v) and v > 0 for v in losses[name]), losses
    print(losses)
    assert losses["pool"] != losses["plain"]
    for flags in (shape + ["-neg_pool", 4],                                            # needs -kg
                  shape + from_kg + ["-neg_pool", 1], shape + from_kg + ["-neg_pool", 257], shape + from_kg + ["-neg_pool", -3]):
        with pytest.raises(SystemExit) as ei:
            train.main([str(f) for f in flags])
        assert ei.value.code == 2
        assert "-neg_pool" in capsys.readouterr().err
