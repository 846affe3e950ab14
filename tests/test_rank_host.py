"""not gpu: the ranking rule of include/kprn.h ("ranking") on the host cores -- kprn_host_rank_groups, evalrank.group_index / metrics_from_hist -- against
the evaluation chain itself (scores -> "%.5f" lines -> evalrank.combine_result -> (user, item) dict -> evalrank.hit_ndcg / eval_samples, the restatement of
the reference's eval/combine_result.py, eval_score.py), and the order against a sort written here.

Bounds: ranks and hit@k are integers / ratios of the same integers: equal exactly.  ndcg@k: both sides are double sums of at most 1e6 terms <= 1 in a
different order: <= 1e6 * 2^-53 ~ 1.1e-10, bound 1e-9."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from kprn_amd import _ffi, evalrank, build as kbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "eval_chain")
NEW = ["kprn_board_reserve", "kprn_board_put", "kprn_board_write", "kprn_board_read", "kprn_rank_groups", "kprn_recommend_ragged", "kprn_host_rank_groups"]
SIZES = (1, 2, 63, 64, 65, 101)


# ---- input families (shared with tests/test_gpu_rank.py) ------------------------------------------------------------------------------------
def straddling_floats():
    """for every printed half-way point (j + 0.5) / 1e5, j = 0..99999: the fp32 neighbours below and above it (and the point itself where fp32 holds it)"""
    h = (np.arange(100000, dtype=np.float64) + 0.5) / 1e5
    f = h.astype(np.float32)
    lo = np.where(f.astype(np.float64) > h, np.nextafter(f, np.float32(-1)), f)
    hi = np.where(f.astype(np.float64) < h, np.nextafter(f, np.float32(2)), f)
    out = np.stack([lo, hi], 1).reshape(-1).astype(np.float32)
    assert np.all(lo.astype(np.float64) <= h) and np.all(hi.astype(np.float64) >= h) and np.all(np.nextafter(lo, np.float32(2)) >= hi)
    return out


def saturated(rng, n):
    """scores the way the reference's fixture is saturated: a sixth print 1.00000, many 0.9999x, the rest anywhere"""
    u = rng.random(n)
    s = np.where(u < 1 / 6, 1.0 - rng.random(n) * 4e-6, np.where(u < 0.6, 1.0 - 10.0 ** (-rng.uniform(3.5, 5.5, n)), rng.random(n)))
    return s.astype(np.float32)


def cut(scores, sizes, rng=None):
    """a flat score array -> group_offsets of groups whose sizes cycle through `sizes` (the tail is the last, shorter group)"""
    off = [0]
    i = 0
    while off[-1] < len(scores):
        off.append(min(len(scores), off[-1] + sizes[i % len(sizes)]))
        i += 1
    return np.asarray(off, np.int64)


def families(seed=0, straddle=True):
    """name -> (scores float32 [n], group_offsets) of every input family of the issue, groups of at most 101 members"""
    rng = np.random.default_rng(seed)
    fam = {}
    s = rng.random(6000).astype(np.float32)
    fam["uniform"] = (s, cut(s, SIZES))
    s = saturated(rng, 6000)
    fam["saturated"] = (s, cut(s, SIZES))
    if straddle:
        s = straddling_floats()
        fam["straddle_sorted"] = (s, cut(s, SIZES))           # neighbours side by side: ties and near-ties inside every group
        s2 = s[rng.permutation(len(s))[:30000]]
        fam["straddle_shuffled"] = (s2, cut(s2, (101,)))
    s = np.zeros(500, np.float32)
    s[250:] = np.float32(4.9e-6)                              # prints 0.00000: a zero group only after rounding
    s[400:] = rng.choice(np.array([0.0, 4.9e-6, 5.1e-6, 1e-5], np.float32), 100)
    fam["zero"] = (s, cut(s, SIZES))
    # a positive that ties with members before and after it: six values, three of which print 0.50000 (with pos = 0 every tie comes after the positive)
    s = rng.choice(np.array([0.5, 0.500001, 0.500004, 0.25, 0.75, 1.0], np.float32), 3000)
    fam["ties"] = (s, cut(s, SIZES))
    return fam


# ---- the chain and the order, in Python -----------------------------------------------------------------------------------------------------
def chain(scores, off):
    """the reference chain on contiguous groups with the positive first -> (ranks per group, hits, ndcgs, n)"""
    entity, res = [], []
    for g in range(len(off) - 1):
        for i in range(off[g], off[g + 1]):
            entity.append("%d\tu%d\ti%d\n" % (i - off[g], g, i - off[g]))
            res.append("%d\t%.5f\t%d\n" % (i, scores[i], 1 if i == off[g] else 0))
    score_of = {}
    for line in evalrank.combine_result(entity, res):
        ll = line.strip().split("\t")
        score_of[(ll[0], ll[1])] = float(ll[3])
    samples = [("u%d" % g, "i0", ["i%d" % i for i in range(1, off[g + 1] - off[g])]) for g in range(len(off) - 1)]
    ranks = []
    for user, pos, negs in samples:
        sc = [score_of[(user, pos)]] + [score_of[(user, x)] for x in negs]
        rank = _ffi.RANK_ZERO_GROUP
        for k in range(1, len(sc) + 1):   # the smallest k with a hit, minus 1; none: a zero group
            if evalrank.hit_ndcg(sc, k)[0] == 1.0:
                rank = k - 1
                break
        ranks.append(rank)
    hits, ndcgs, n = evalrank.eval_samples(score_of, samples)
    return np.asarray(ranks, np.int32), hits, ndcgs, n


def py_key(p, mode):
    """(valid, key) of one score by the rule's text, independent of the library: mode 0 through the printed string itself"""
    p = float(p)
    if mode == 0:
        if not (0.0 <= p <= 1.0):
            return (0, 0)
        return (1, int(("%.5f" % p).replace(".", "")))
    return (0, 0) if math.isnan(p) else (1, p)


def py_order(scores, mode):
    keys = [py_key(p, mode) for p in scores]
    order = sorted(range(len(scores)), key=lambda i: (-keys[i][0], -keys[i][1], i))
    zero = mode == 0 and not any(v and k > 0 for v, k in keys)
    return order, zero, sum(1 for v, _ in keys if not v)


def check_order(res, scores, off, members, pos, mode, K, hist_len):
    """every output of a ranking call against py_order"""
    G = len(off) - 1
    hist = np.zeros(hist_len + 4, np.int64)
    for g in range(G):
        lines = np.arange(off[g], off[g + 1]) if members is None else members[off[g]:off[g + 1]]
        sc = scores[lines]
        order, zero, inv = py_order(sc, mode)
        p = 0 if pos is None else int(pos[g])
        hist[hist_len + 3] += inv
        if p < 0:
            want = _ffi.RANK_NO_POSITIVE
            hist[hist_len + 2] += 1
        elif zero:
            want = _ffi.RANK_ZERO_GROUP
            hist[hist_len + 1] += 1
        else:
            want = order.index(p)
            hist[min(want, hist_len)] += 1
        assert res["ranks"][g] == want, (g, res["ranks"][g], want)
        if K:
            top = order[:K]
            assert list(res["topk_idx"][g][:len(top)]) == top, (g, res["topk_idx"][g], top)
            assert res["topk_score"][g][:len(top)].tobytes() == sc[top].tobytes(), g   # the RAW scores, bit for bit (NaN included)
            assert np.all(res["topk_idx"][g][len(top):] == -1) and np.all(res["topk_score"][g][len(top):] == 0.0)
    assert np.array_equal(res["hist"], hist), (res["hist"], hist)


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    so = kbuild.build()
    assert b"amdgcn-amd-amdhsa--gfx950" in open(so, "rb").read()
    hdr = open(os.path.join(ROOT, "include", "kprn.h")).read()
    lua = open(os.path.join(ROOT, "bindings", "kprn.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]", lua.index("ffi.cdef[["))]
    syms = subprocess.check_output(["nm", "-D", so]).decode()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert " T %s" % name in syms, name
        assert re.search(r"\bint %s\s*\(" % name, cdef), name
    for const, val in (("KPRN_RANK_PRINTED", "0"), ("KPRN_RANK_RAW", "1"), ("KPRN_RANK_ZERO_GROUP", "(-1)"), ("KPRN_RANK_NO_POSITIVE", "(-2)")):
        assert re.search(r"#define %s %s\s*\n" % (const, re.escape(val)), hdr), const


def test_printed_key_is_the_integer_percent_5f_prints():
    """the rule's mode-0 key through the library (ranking a group of one pair against a probe) equals the printed string, on every straddling float"""
    s = np.concatenate([straddling_floats()[::7], np.array([0.0, 1.0, 1e-5, 5e-6, 0.5, 0.99999, 0.999995], np.float32)])
    # pairs (s[i], probe): s[i] is ranked first iff its key >= the probe's key (first seen wins the tie)
    for probe in (np.float32(0.5), np.float32(0.25003)):
        flat = np.stack([np.full_like(s, probe), s], 1).reshape(-1)
        res = _ffi.host_rank_groups(flat, np.arange(0, 2 * len(s) + 1, 2), pos=np.ones(len(s), np.int32))
        want = np.array([0 if py_key(x, 0)[1] > py_key(probe, 0)[1] else 1 for x in s], np.int32)
        assert np.array_equal(res["ranks"], want)


@pytest.mark.parametrize("name", ["uniform", "saturated", "straddle_sorted", "straddle_shuffled", "zero", "ties"])
def test_host_rank_groups_equals_the_reference_chain(name):
    scores, off = families()[name]
    ranks, hits, ndcgs, n = chain(scores, off)
    res = _ffi.host_rank_groups(scores, off, hist_len=15)
    assert np.array_equal(res["ranks"], ranks)
    h2, d2, n2 = evalrank.metrics_from_hist(res["hist"], 15)
    assert n2 == n == len(off) - 1
    for k in range(1, 16):
        assert h2[k] == hits[k], (k, h2[k], hits[k])
        assert abs(d2[k] - ndcgs[k]) <= 1e-9, (k, d2[k], ndcgs[k])
    if name == "zero":
        assert (ranks == _ffi.RANK_ZERO_GROUP).sum() >= 2 and res["hist"][16] == (ranks == -1).sum()
    if name in ("saturated", "ties", "straddle_sorted"):
        assert (ranks == 0).sum() > 0 and (ranks > 0).sum() > 0


def order_cases(seed=1):
    """(name, scores, offsets, members, pos, mode): the families with pos != 0 / -1, large groups, invalid members, scattered members with repeats, mode 1"""
    rng = np.random.default_rng(seed)
    out = []
    for name, (s, off) in families(seed, straddle=False).items():
        n = np.diff(off)
        out.append((name + "_pos", s, off, None, (rng.integers(0, 1 << 30, len(n)) % n).astype(np.int32), 0))
        pos = (rng.integers(0, 1 << 30, len(n)) % n).astype(np.int32)
        pos[::3] = -1
        out.append((name + "_nopos", s, off, None, pos, 0))
    s = straddling_floats()[:40000]
    out.append(("straddle_pos", s, cut(s, SIZES), None, None, 0))
    big = np.concatenate([saturated(rng, 6000), rng.random(6000).astype(np.float32)])
    off = cut(big, (1000, 4096, 257, 256, 512))
    out.append(("big", big, off, None, (rng.integers(0, 1 << 30, len(off) - 1) % np.diff(off)).astype(np.int32), 0))
    bad = rng.random(3000).astype(np.float32)
    bad[rng.integers(0, 3000, 300)] = np.nan
    bad[rng.integers(0, 3000, 100)] = 1.5
    bad[rng.integers(0, 3000, 100)] = -0.25
    bad[:65] = np.nan                                   # a group of invalid members only
    off = cut(bad, (65, 1, 2, 101, 700))
    out.append(("invalid", bad, off, None, (rng.integers(0, 1 << 30, len(off) - 1) % np.diff(off)).astype(np.int32), 0))
    out.append(("invalid_raw", bad, off, None, None, 1))
    board = saturated(rng, 5000)
    members = rng.integers(0, 5000, 12000).astype(np.int64)   # scattered, with repeats
    members[100:110] = members[100]
    off = cut(members, (101, 64, 300, 5))
    out.append(("scattered", board, off, members, (rng.integers(0, 1 << 30, len(off) - 1) % np.diff(off)).astype(np.int32), 0))
    raw = (rng.standard_normal(4000) * 10).astype(np.float32)
    raw[rng.integers(0, 4000, 40)] = np.inf
    raw[rng.integers(0, 4000, 40)] = -np.inf
    raw[rng.integers(0, 4000, 40)] = 0.0
    raw[rng.integers(0, 4000, 40)] = -0.0
    raw[rng.integers(0, 4000, 40)] = np.nan
    raw[rng.integers(0, 4000, 400)] = np.float32(2.5)
    off = cut(raw, SIZES + (600,))
    out.append(("raw", raw, off, None, (rng.integers(0, 1 << 30, len(off) - 1) % np.diff(off)).astype(np.int32), 1))
    return out


@pytest.mark.parametrize("K", [1, 10, 64])
def test_host_order_ranks_and_topk_against_a_python_sort(K):
    for name, s, off, members, pos, mode in order_cases():
        res = _ffi.host_rank_groups(s, off, members=members, pos=pos, mode=mode, K=K, hist_len=20)
        check_order(res, s, off, members, pos, mode, K, 20)


def test_golden_fixture_group_index_equals_the_dict_route():
    """the reference's own 300 lines: one sample per user that has a label-1 line (positive = its first label-1 item, negatives = its other items)"""
    entity = open(os.path.join(GOLD, "test_sample.list.entity")).readlines()
    res_lines = open(os.path.join(GOLD, "test_sample.res")).readlines()
    assert len(entity) == len(res_lines) == 300
    items, positive = {}, {}
    for e, r in zip(entity, res_lines):
        el, rl = e.strip().split("\t"), r.strip().split("\t")
        items.setdefault(el[1], [])
        if el[2] not in items[el[1]]:
            items[el[1]].append(el[2])
        if rl[-1] == "1" and el[1] not in positive:
            positive[el[1]] = el[2]
    samples = [(u, positive[u], [x for x in items[u] if x != positive[u]]) for u in items if u in positive]
    assert len(samples) > 100
    score_of = {}
    for line in evalrank.combine_result(entity, res_lines):
        ll = line.strip().split("\t")
        score_of[(ll[0], ll[1])] = float(ll[3])
    hits, ndcgs, n = evalrank.eval_samples(score_of, samples)
    members, off, n_used = evalrank.group_index(entity, samples)
    assert n_used == n == len(samples)
    scores = np.array([float(r.split("\t")[1]) for r in res_lines], np.float32)
    assert all("%.5f" % s == r.split("\t")[1] for s, r in zip(scores, res_lines))   # fp32 carries the printed value
    res = _ffi.host_rank_groups(scores, off, members=members)
    h2, d2, n2 = evalrank.metrics_from_hist(res["hist"], 15)
    assert n2 == n
    for k in range(1, 16):
        assert h2[k] == hits[k] and abs(d2[k] - ndcgs[k]) <= 1e-9, k
    # users outside user_ids are left out (resort.py:22-30)
    some = [s[0] for s in samples[:40]]
    _m, _o, n_some = evalrank.group_index(entity, samples, [u + "\n" for u in some])
    assert n_some == len(set(some))


def test_group_index_skips_unscored_and_honours_a_replaced_line():
    entity = ["0\tu\tp\n", "0\tu\ta\n", "0\tu\tb\n", "0\tu\ta\n", "0\tv\tp\n"]
    samples = [("u", "p", ["a", "b"]), ("u", "p", ["a", "zz"]), ("w", "p", ["a"]), ("v", "p", [])]
    members, off, n = evalrank.group_index(entity, samples)
    assert n == 2 and list(off) == [0, 3, 4]
    assert list(members) == [0, 3, 2, 4]   # (u, a): line 3 replaced line 1, as the dict does
    scores = np.array([0.8, 0.1, 0.1, 0.9, 0.3], np.float32)
    res = _ffi.host_rank_groups(scores, off, members=members)
    assert list(res["ranks"]) == [1, 0]
    score_of = {("u", "p"): 0.8, ("u", "a"): 0.9, ("u", "b"): 0.1, ("v", "p"): 0.3}
    hits, ndcgs, n2 = evalrank.eval_samples(score_of, samples, ks=[1, 2])
    h2, d2, n3 = evalrank.metrics_from_hist(res["hist"], 15, ks=[1, 2])
    assert n2 == n3 == 2 and h2 == hits and all(abs(d2[k] - ndcgs[k]) < 1e-12 for k in (1, 2))


def test_metrics_from_hist_refuses_invalid_members():
    res = _ffi.host_rank_groups(np.array([0.5, np.nan, 0.25], np.float32), [0, 3])
    assert res["hist"][15 + 3] == 1
    with pytest.raises(ValueError):
        evalrank.metrics_from_hist(res["hist"], 15)


def test_host_refusals_return_their_code_and_write_nothing():
    L = _ffi.lib()
    scores = np.linspace(0, 1, 50).astype(np.float32)
    big = np.zeros(5000, np.float32)

    def call(sc, goff, members=None, pos=None, mode=0, K=4, hist_len=15, G=None):
        goff = np.asarray(goff, np.int64)
        G = len(goff) - 1 if G is None else G
        mem = None if members is None else np.asarray(members, np.int64)
        p = None if pos is None else np.asarray(pos, np.int32)
        ranks = np.full(max(G, 1), -7, np.int32)
        ti = np.full((max(G, 1), 64), -7, np.int32)
        ts = np.full((max(G, 1), 64), -7, np.float32)
        hist = np.full(5000, -7, np.int64)
        rc = L.kprn_host_rank_groups(_ffi._fp(sc), C.c_int64(len(sc)), _ffi._fp(mem), _ffi._fp(goff), _ffi._fp(p), G, mode, K, _ffi._fp(ranks), _ffi._fp(ti),
                                     _ffi._fp(ts), _ffi._fp(hist), hist_len)
        untouched = np.all(ranks == -7) and np.all(ti == -7) and np.all(ts == -7) and np.all(hist == -7)
        return rc, untouched

    assert call(scores, [0, 10, 50]) == (0, False)
    assert call(scores, [0, 10, 10, 50]) == (_ffi.E_ARG, True)            # an empty group
    assert call(big, [0, 4097]) == (_ffi.E_ARG, True)                      # a group above 4096
    assert call(big, [0, 4096])[0] == 0
    assert call(scores, [0, 10, 50], pos=[10, 0]) == (_ffi.E_ARG, True)   # pos outside -1..n-1
    assert call(scores, [0, 10, 50], pos=[-2, 0]) == (_ffi.E_ARG, True)
    assert call(scores, [0, 10, 50], pos=[9, -1])[0] == 0
    for K in (0, 65, -1):
        assert call(scores, [0, 50], K=K) == (_ffi.E_ARG, True)
    for hl in (0, 4097):
        assert call(scores, [0, 50], hist_len=hl) == (_ffi.E_ARG, True)
    assert call(scores, [0, 50], mode=2) == (_ffi.E_ARG, True)
    assert call(scores, [0, 50], G=0) == (_ffi.E_ARG, True)
    assert call(scores, [0, 51]) == (_ffi.E_INDEX, True)                   # a run past the end of the scores
    assert call(scores, [0, 3], members=[0, 50, 1]) == (_ffi.E_INDEX, True)
    assert call(scores, [0, 3], members=[0, -1, 1]) == (_ffi.E_INDEX, True)
    assert call(scores, [0, 3], members=[0, 49, 49])[0] == 0
    with pytest.raises(_ffi.KprnError) as ei:
        _ffi.host_rank_groups(scores, [0, 51])
    assert ei.value.code == _ffi.E_INDEX


def test_score_cli_without_rank_flags_calls_test_from_checkpoint_as_before(monkeypatch, tmp_path):
    from kprn_amd import model, score, scoring
    calls = []
    engine = object()
    monkeypatch.setattr(model, "build_engine", lambda params: engine)
    monkeypatch.setattr(scoring, "test_from_checkpoint", lambda *a, **k: calls.append((a, k)))
    monkeypatch.setattr(scoring, "test_and_rank", lambda *a, **k: pytest.fail("ranking without -rank_samples"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    out = str(tmp_path / "test.res")
    rc = score.main(["-input_dir", str(tmp_path), "-out_file", out, "-model_path", "m", "-test_list", "test.list", "-gpu_id", "0", "-top_k", "2",
                     "-rnnHidSize", "16", "-numFeatureTemplates", "3", "-numEntityTypes", "1"])
    assert rc == 0 and len(calls) == 1
    a, k = calls[0]
    import sys
    assert a == (engine, str(tmp_path), "test.list", out)
    assert k == dict(log=sys.stdout, rank=0, world=1, barrier=None, merge_path_counts=False)
    # ... and with them, the ranking route gets the files
    calls.clear()
    ranked = []
    monkeypatch.setattr(scoring, "test_and_rank", lambda *a, **k: ranked.append((a, k)))
    rc = score.main(["-input_dir", str(tmp_path), "-out_file", out, "-model_path", "m", "-test_list", "test.list", "-rank_samples", "s.txt", "-rank_entity", "e.txt",
                     "-rank_out", "o.txt", "-rnnHidSize", "16"])
    assert rc == 0 and not calls and len(ranked) == 1
    assert ranked[0][0] == (engine, str(tmp_path), "test.list", out, "s.txt", "e.txt", None, "o.txt")
