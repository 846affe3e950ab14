"""gpu: the ranking stage on the device (include/kprn.h "ranking"; kprn_amd/csrc/rank_groups.hip) -- the kernels against their host twin bit for bit, the
board puts' ordering behind every way a scoring pass can run, rank_test_set / recommend_ragged / the score CLI end to end.  The rule itself is held against
the reference chain by tests/test_rank_host.py (host twin) and, on the engine's own scores, by the end-to-end test here.

Bounds: everything integer or copied (ranks, top-K indices, raw top-K scores, histogram, board contents) is compared for equality; ndcg@k against the chain
within 1e-9 (two double sums of at most 1e6 terms <= 1 in different orders: <= 1.1e-10)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from kprn_amd import _ffi, batcher, evalrank, formats, model, scoring, synth
from tests.test_rank_host import SIZES, cut, families, order_cases, saturated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mk(seed=3, Ve=300, **kw):
    return _ffi.Engine(6, Ve, 9, 16, 32, 16, 64, 2, seed=seed, **kw)


def same(dev, host, what=("ranks", "hist", "topk_idx", "topk_score")):
    for k in what:
        if k in host or k in dev:
            assert dev[k].shape == host[k].shape and dev[k].tobytes() == host[k].tobytes(), k


def both(eng, scores, off, members=None, pos=None, mode=0, K=10, hist_len=15):
    """one ranking call on the device and on the host over the same scores; the board holds `scores` from entry 0"""
    dev = eng.rank_groups(off, members=members, pos=pos, mode=mode, K=K, hist_len=hist_len)
    host = _ffi.host_rank_groups(scores, off, members=members, pos=pos, mode=mode, K=K, hist_len=hist_len)
    same(dev, host)
    return dev


def test_device_ranking_equals_the_host_twin_bit_for_bit():
    eng = mk()
    rng = np.random.default_rng(5)
    for name, (s, off) in families().items():
        eng.board_reserve(len(s))
        eng.board_write(0, s)
        assert eng.board_read(0, len(s)).tobytes() == s.tobytes()
        n = np.diff(off)
        for mode in (0, 1):
            for K in (0, 1, 10, 64):
                both(eng, s, off, mode=mode, K=K)
            pos = (rng.integers(0, 1 << 30, len(n)) % n).astype(np.int32)
            pos[::5] = -1
            both(eng, s, off, pos=pos, mode=mode, K=10, hist_len=3)
            # scattered members with repeats, groups cut anew
            members = rng.integers(0, len(s), 20000).astype(np.int64)
            moff = cut(members, SIZES + (300, 5))
            both(eng, s, moff, members=members, mode=mode, K=10)
            both(eng, s, moff[3:40], members=members, mode=mode, K=7)   # (group_offsets need not start at 0)
    for name, s, off, members, pos, mode in order_cases():
        eng.board_reserve(len(s))
        eng.board_write(0, s)
        for K in (1, 10, 64):
            both(eng, s, off, members=members, pos=pos, mode=mode, K=K, hist_len=20)
    # G from 1 to 100 000; group sizes 1000 and 4096 among small ones
    s = np.concatenate([saturated(rng, 150000), rng.random(150000).astype(np.float32)])
    eng.board_reserve(len(s))
    eng.board_write(0, s)
    both(eng, s, np.array([7, 108], np.int64))
    both(eng, s, np.arange(0, 200001, 2, dtype=np.int64), K=2)                       # 100 000 groups of 2
    both(eng, s, cut(s, (101,)), K=10)
    big = cut(s[:60000], (4096, 3, 1000, 64, 257, 2048, 101))
    d1 = both(eng, s, big, K=64, hist_len=4096)
    d2 = both(eng, s, big, K=64, hist_len=4096)                                     # a second call's histogram is its own
    assert np.array_equal(d1["hist"], d2["hist"]) and d1["hist"][:4098].sum() == len(big) - 1
    both(eng, s, big, mode=1, K=64, pos=np.full(len(big) - 1, -1, np.int32))
    # both bodies of the workgroup kernel on every large group: all sorted in LDS (257), all counted (4097); the default switches at 512
    for sort_min in ("257", "4097", "512"):
        eng.set_option("rank_sort_min", sort_min)
        for mode in (0, 1):
            both(eng, s, big, mode=mode, K=64, hist_len=4096, pos=(np.diff(big) // 2).astype(np.int32))
    for name, sc, off, members, pos, mode in order_cases():
        if name in ("big", "invalid", "invalid_raw", "scattered", "raw"):
            eng.board_reserve(len(sc))
            eng.board_write(0, sc)
            for sort_min in ("257", "4097", "512"):
                eng.set_option("rank_sort_min", sort_min)
                both(eng, sc, off, members=members, pos=pos, mode=mode, K=64, hist_len=20)
    for bad in ("256", "4098"):
        with pytest.raises(_ffi.KprnError) as e:
            eng.set_option("rank_sort_min", bad)
        assert e.value.code == _ffi.E_ARG
    # an entry nothing wrote is NaN: invalid, counted
    eng.board_reserve(300)
    eng.board_write(0, s[:200])
    d = eng.rank_groups(np.array([0, 101, 300], np.int64), K=3)
    assert d["hist"][15 + 3] == 100 and np.isnan(eng.board_read(200, 100)).all()
    with pytest.raises(ValueError):
        evalrank.metrics_from_hist(d["hist"], 15)
    eng.close()


def test_device_refusals():
    eng = mk()
    L = eng.L
    with pytest.raises(_ffi.KprnError) as e:
        eng.rank_groups([0, 5])                      # no board yet
    assert e.value.code == _ffi.E_ARG
    with pytest.raises(_ffi.KprnError) as e:
        eng.board_reserve(0)
    assert e.value.code == _ffi.E_ARG
    eng.board_reserve(5000)
    with pytest.raises(_ffi.KprnError) as e:
        eng.board_put(0, 4)                          # no pass to read from
    assert e.value.code == _ffi.E_ARG
    scores = np.linspace(0, 1, 5000).astype(np.float32)
    eng.board_write(0, scores)

    def call(goff, members=None, pos=None, mode=0, K=4, hist_len=15):
        goff = np.asarray(goff, np.int64)
        G = len(goff) - 1
        mem = None if members is None else np.asarray(members, np.int64)
        p = None if pos is None else np.asarray(pos, np.int32)
        ranks = np.full(G, -7, np.int32)
        ti, ts = np.full((G, 64), -7, np.int32), np.full((G, 64), -7, np.float32)
        hist = np.full(5000, -7, np.int64)
        rc = L.kprn_rank_groups(eng.h, _ffi._fp(mem), _ffi._fp(goff), _ffi._fp(p), G, mode, K, _ffi._fp(ranks), _ffi._fp(ti), _ffi._fp(ts), _ffi._fp(hist), hist_len)
        return rc, bool(np.all(ranks == -7) and np.all(ti == -7) and np.all(ts == -7) and np.all(hist == -7))

    assert call([0, 10, 50]) == (0, False)
    assert call([0, 10, 10, 50]) == (_ffi.E_ARG, True)
    assert call([0, 4097]) == (_ffi.E_ARG, True)
    assert call([0, 10, 50], pos=[10, 0]) == (_ffi.E_ARG, True)
    assert call([0, 10, 50], pos=[-2, 0]) == (_ffi.E_ARG, True)
    for K in (0, 65):
        assert call([0, 50], K=K) == (_ffi.E_ARG, True)
    for hl in (0, 4097):
        assert call([0, 50], hist_len=hl) == (_ffi.E_ARG, True)
    assert call([0, 50], mode=2) == (_ffi.E_ARG, True)
    assert call([4990, 5001]) == (_ffi.E_INDEX, True)
    assert call([0, 3], members=[0, 5000, 1]) == (_ffi.E_INDEX, True)
    assert call([0, 3], members=[0, -1, 1]) == (_ffi.E_INDEX, True)
    assert call([0, 3], members=[0, 4999, 4999])[0] == 0
    for off, n in ((-1, 4), (4998, 4)):
        with pytest.raises(_ffi.KprnError) as e:
            eng.board_write(off, scores[:n])
        assert e.value.code == _ffi.E_INDEX
        with pytest.raises(_ffi.KprnError) as e:
            eng.board_read(off, n)
        assert e.value.code == _ffi.E_INDEX
    idx, _ = synth.make_paths(8, 2, 6, Ve=300, seed=1)
    eng.forward(eng.batch(idx), 1)
    eng.board_put(10, 8)
    with pytest.raises(_ffi.KprnError) as e:
        eng.board_put(0, 9)                          # beyond the pass's pairs
    assert e.value.code == _ffi.E_ARG
    with pytest.raises(_ffi.KprnError) as e:
        eng.board_put(4995, 8)
    assert e.value.code == _ffi.E_INDEX
    # recommend_ragged: group_counts must add up to B; nothing is written
    ri, rc_, _ = synth.make_ragged(6, 6, Ve=300, seed=2)
    with pytest.raises(_ffi.KprnError) as e:
        eng.recommend_ragged(ri, rc_, [3, 2], 2)
    assert e.value.code == _ffi.E_ARG
    with pytest.raises(_ffi.KprnError) as e:
        eng.recommend_ragged(ri, rc_, [6], 65)
    assert e.value.code == _ffi.E_ARG
    eng.close()


# ---- the 1 500 x 101 evaluation, end to end ---------------------------------------------------------------------------------------------------
def test_rank_test_set_equals_the_reference_chain_on_the_engines_scores(tmp_path):
    """the evaluation of tests/test_gpu_host.py::test_hit_and_ndcg_at_k_... (same engine shape and seed, 1 500 users x 101 candidates), the pairs bucketed by
    path count into files and every user's candidates scattered over them; rank_test_set against the chain on the scores the board holds"""
    users, cand, T, Ve = 1500, 101, 6, 20000
    eng = _ffi.Engine(6, Ve, 9, 16, 32, 16, 64, 2, param_init=0.35, seed=7)
    pairs = users * cand
    root = str(tmp_path)
    names, left = [], pairs
    for i, (P, n) in enumerate(((1, 60000), (2, 50000), (3, 30000), (5, pairs - 140000))):
        idx, labels = synth.make_paths(n, P, T, Ve=Ve, seed=99 + i)
        formats.save_path_file(os.path.join(root, "test_%d.npz" % P), labels, idx, 1)
        names.append("test_%d.npz" % P)
        left -= n
    assert left == 0
    with open(os.path.join(root, "test.list"), "w") as f:
        f.write("\n".join(names) + "\n")
    line_of = np.random.default_rng(11).permutation(pairs)            # candidate c of user u is line line_of[u * cand + c]
    user_item = np.empty(pairs, np.int64)
    user_item[line_of] = np.arange(pairs)
    entity = ["0\t%d\t%d\n" % (user_item[i] // cand, user_item[i] % cand) for i in range(pairs)]
    samples = [(str(u), "0", [str(c) for c in range(1, cand)]) for u in range(users)]
    members, off, n_used = evalrank.group_index(entity, samples)
    assert n_used == users and np.array_equal(members, line_of)
    fl = batcher.BatcherFileList(root, 512, False, 1000, True, "test.list", check_ids=False)
    res, n = scoring.rank_test_set(eng, fl, members, off, K=10)
    assert n == pairs
    scores = eng.board_read(0, pairs)
    assert np.isfinite(scores).all() and scores.min() >= 0 and scores.max() <= 1
    # the board holds what the streaming scorer hands out
    fl2 = batcher.BatcherFileList(root, 512, False, 1000, True, "test.list", check_ids=False)
    ref_scores = np.concatenate([p for _l, p in scoring.score_batches(eng, fl2)])
    assert ref_scores.tobytes() == scores.tobytes()
    # the chain on those scores
    res_lines = ["%d\t%.5f\t%d\n" % (i, scores[i], 1 if user_item[i] % cand == 0 else 0) for i in range(pairs)]
    score_of = {}
    for line in evalrank.combine_result(entity, res_lines):
        ll = line.strip().split("\t")
        score_of[(ll[0], ll[1])] = float(ll[3])
    hits, ndcgs, n_chain = evalrank.eval_samples(score_of, samples)
    want = []
    for user, pos, negs in samples:
        sc = [score_of[(user, pos)]] + [score_of[(user, x)] for x in negs]
        rank = -1
        for k in range(1, cand + 1):
            if evalrank.hit_ndcg(sc, k)[0] == 1.0:
                rank = k - 1
                break
        want.append(rank)
    assert np.array_equal(res["ranks"], np.asarray(want, np.int32))
    h2, d2, n2 = evalrank.metrics_from_hist(res["hist"], 15)
    assert n2 == n_chain == users
    for k in range(1, 16):
        assert h2[k] == hits[k], (k, h2[k], hits[k])
        assert abs(d2[k] - ndcgs[k]) <= 1e-9, (k, d2[k], ndcgs[k])
    assert 0.0 < hits[10] < 1.0
    same(res, _ffi.host_rank_groups(scores, off, members=members, K=10))
    # merged (ragged) scoring of the same files: the same board up to the bar tests/test_gpu_ragged.py sets for merged against plain scoring (1e-4 relative),
    # the ranking call itself equal to its host twin
    fl3 = batcher.BatcherFileList(root, 512, False, 1000, True, "test.list", check_ids=False)
    res3, n3 = scoring.rank_test_set(eng, fl3, members, off, K=10, merge=True)
    s3 = eng.board_read(0, pairs)
    np.testing.assert_allclose(s3, scores, rtol=1e-4)
    same(res3, _ffi.host_rank_groups(s3, off, members=members, K=10))
    eng.close()


# ---- ordering of the puts ---------------------------------------------------------------------------------------------------------------------
def _drive(eng, how, use_put):
    """two scoring passes (a, b) each followed by a put / a read, driven the way `how` says; -> the two passes' probabilities"""
    # (learning rate 0: the step's kernels run and are ordered against the puts, the parameters the second pass reads stay the same bits in both
    # engines -- a training step's gradient sums are not reproducible to the last bit from run to run)
    opt = _ffi.make_opt(method=1, lr=0.0)
    big = how in ("overlap_side", "split")
    na, nb = (3000, 2500) if big else (90, 70)
    ia, _ = synth.make_paths(na, 2, 6, Ve=300, seed=41)
    ib, _ = synth.make_paths(nb, 3, 6, Ve=300, seed=42)
    ti, tl = synth.make_paths(128, 2, 6, Ve=300, seed=43)   # (not fewer pairs than a scoring pass: kprn_read_probs bounds B by the LAST forward's pairs)
    if how != "sync":
        ba, bb = eng.batch(ia), eng.batch(ib)
    tb = eng.batch(ti, tl)
    if how in ("overlap", "overlap_side", "dual_train", "split"):
        eng.set_option("score_overlap", "1")
    if how == "overlap_side":
        eng.set_option("score_dual", "0")
    if how == "split":
        eng.set_option("score_split", "0.5")
    if use_put:
        eng.board_reserve(na + nb + 10)
    out = []
    for k, (n, off) in enumerate(((na, 3), (nb, na + 5))):
        if how == "sync":
            eng.forward(eng.batch(ia if k == 0 else ib), 1)
        else:
            eng.forward_async(ba if k == 0 else bb, 1)
        if how == "dual_train":
            eng.train_step(tb, opt, want_loss=False)     # the pass rides in this step's forward; the optimiser step follows
        if use_put:
            eng.board_put(off, n)
            if how == "overlap" and k == 0:
                eng.train_step(tb, opt, want_loss=False)  # (work behind a queued put: the next pass and an update)
        else:
            out.append(eng.read_probs(n))
            if how == "overlap" and k == 0:
                eng.train_step(tb, opt, want_loss=False)
    if use_put:
        out = [eng.board_read(3, na), eng.board_read(na + 5, nb)]
        assert np.isnan(eng.board_read(0, 3)).all() and np.isnan(eng.board_read(na + 3, 2)).all()   # the puts wrote their ranges only
        r = eng.rank_groups(np.array([3, 3 + na], np.int64), K=5)       # ranking waits for the puts as well
        same(r, _ffi.host_rank_groups(np.concatenate([np.zeros(3, np.float32), out[0]]), np.array([3, 3 + na], np.int64), K=5))
    return out


HOWS = ["sync", "async_main", "overlap", "overlap_side", "split", "dual_train"]


@pytest.mark.parametrize("how", HOWS)
def test_board_put_reads_what_read_probs_returns(how, monkeypatch):
    if how == "split":
        monkeypatch.setenv("KPRN_SMALL_TILES", "0")   # (64-path tiles at this size too: a pass of >= 64 tiles is split)
    e1, e2 = mk(), mk()
    got = _drive(e1, how, True)
    want = _drive(e2, how, False)
    for g, w in zip(got, want):
        assert np.isfinite(w).all() and g.tobytes() == w.tobytes()
    e1.close()
    e2.close()


def test_board_put_orderings_with_poisoned_allocations():
    """once more with every new device allocation filled with 0xFF bytes (KPRN_POISON_ALLOC=1): a put that copied from a buffer its pass had not written
    yet would hand out NaN"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "test_board_put_reads_what_read_probs_returns"], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, KPRN_POISON_ALLOC="1"), timeout=900)
    assert r.returncode == 0 and "%d passed" % len(HOWS) in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]


# ---- one call for the K best ------------------------------------------------------------------------------------------------------------------
def test_recommend_ragged_equals_forward_ragged_plus_the_host_rule():
    eng = mk()
    rng = np.random.default_rng(9)
    rect, _ = synth.make_paths(20, 3, 6, Ve=300, seed=50)
    for trial, group_counts in enumerate(([101], rng.integers(1, 140, 37).tolist(), [1], [300, 1, 64, 65])):
        B = int(np.sum(group_counts))
        counts = synth.draw_num_paths(np.random.default_rng(60 + trial), B)
        idx, _, _ = synth.make_ragged(B, 6, Ve=300, seed=70 + trial, counts=counts)
        off = np.concatenate([[0], np.cumsum(group_counts)]).astype(np.int64)
        for mode, K in ((0, 10), (1, 64), (0, 1)):
            r0, _ = eng.forward_host(rect, 1, want_all=False)        # rectangular calls on the same handle in between
            probs, _ = eng.forward_ragged_host(idx, counts, 1)
            ti, ts, p2 = eng.recommend_ragged(idx, counts, group_counts, K, mode=mode, want_probs=True)
            assert p2.tobytes() == probs.tobytes()
            host = _ffi.host_rank_groups(probs, off, pos=np.full(len(group_counts), -1, np.int32), mode=mode, K=K)
            assert ti.tobytes() == host["topk_idx"].tobytes() and ts.tobytes() == host["topk_score"].tobytes()
            ti2, ts2, none = eng.recommend_ragged(idx, counts, group_counts, K, mode=mode)
            assert none is None and ti2.tobytes() == ti.tobytes() and ts2.tobytes() == ts.tobytes()
            assert eng.forward_host(rect, 1, want_all=False)[0].tobytes() == r0.tobytes()
    eng.close()


# ---- command line -----------------------------------------------------------------------------------------------------------------------------
FLAGS = ("-entityTypeVocabSize 6 -entityVocabSize 500 -relationVocabSize 9 -entityTypeEmbeddingDim 16 -entityEmbeddingDim 32 "
         "-relationEmbeddingDim 16 -numFeatureTemplates 3 -numEntityTypes 1 -rnnType lstm -rnnHidSize 64 -numLayers 2 -topK 2 "
         "-useAdam 1 -learningRate 0.01 -regularize 0 -includeEntity 1 -minibatch 16 -gradientStepCounter 100000")


def test_score_and_train_cli_rank_on_the_device(tmp_path):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "test"))
    os.makedirs(os.path.join(root, "train"))
    names, total = [], 0
    for i, (n, P) in enumerate([(300, 2), (210, 4), (96, 1)]):
        idx, labels = synth.make_paths(n, P, 6, Ve=500, seed=70 + i)
        formats.save_path_file(os.path.join(root, "test/test.txt.%d.npz" % P), labels, idx, 1)
        names.append("test/test.txt.%d.npz" % P)
        total += n
    open(os.path.join(root, "test.list"), "w").write("\n".join(names) + "\n")
    idx, labels = synth.make_paths(64, 2, 6, Ve=500, seed=80)
    formats.save_path_file(os.path.join(root, "train/train.txt.2.npz"), labels, idx, 1)
    open(os.path.join(root, "train.list"), "w").write("train/train.txt.2.npz\n")
    # 60 users x 10 candidates scattered over the 606 lines; 6 lines belong to a user outside the list; one sample names an unscored item
    rng = np.random.default_rng(3)
    perm = rng.permutation(total)
    entity = [None] * total
    for j, line in enumerate(perm):
        entity[line] = "0\t%d\t%d\n" % (j // 10, j % 10)
    ent_file, samp_file, users_file = (os.path.join(root, n) for n in ("test.list.entity", "samples.txt", "users.txt"))
    open(ent_file, "w").writelines(entity)
    samples = [(str(u), "0", [str(c) for c in range(1, 10)]) for u in range(60)] + [("60", "0", ["1", "2", "77"])]
    open(samp_file, "w").writelines("%s\t%s\t%s\n" % (u, p, "#".join(n)) for u, p, n in samples)
    open(users_file, "w").writelines("%d\n" % u for u in range(55))
    params = model.parse_flags(FLAGS.split() + ["-dataDir", root])
    ck = os.path.join(root, "m-latest")
    model.build_engine(params).save(ck)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "kprn_amd.score", "-input_dir", root, "-test_list", "test.list", "-model_path", ck, "-top_k", "2", "-gpu_id", "0"]
    plain, ranked, rank_out = (os.path.join(root, n) for n in ("plain.res", "ranked.res", "eval_res.txt"))
    r = subprocess.run(base + ["-out_file", plain] + FLAGS.split(), capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hit score" not in r.stdout
    r = subprocess.run(base + ["-out_file", ranked, "-rank_samples", samp_file, "-rank_entity", ent_file, "-rank_users", users_file, "-rank_out", rank_out] +
                       FLAGS.split(), capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(plain, "rb").read() == open(ranked, "rb").read() and len(open(plain).readlines()) == total
    # the Python chain on the written file
    comb = evalrank.combine_result(entity, open(plain).readlines())
    keep = evalrank.resort(comb, open(users_file).readlines())
    score_of = {}
    for line in keep:
        ll = line.strip().split("\t")
        score_of[(ll[0], ll[1])] = float(ll[3])
    hits, ndcgs, n = evalrank.eval_samples(score_of, samples)
    assert n == 55
    want = evalrank.format_metric_lines(hits, ndcgs)
    assert open(rank_out).readlines() == list(want)
    assert "hit score: " + str(["%.5f" % hits[k] for k in range(1, 16)]) in r.stdout
    assert "ndcg score: " + str(["%.5f" % ndcgs[k] for k in range(1, 16)]) in r.stdout
    # training with -evaluationFrequency: the callback prints the metrics every N epochs; without -rank_samples there is none
    tr = [sys.executable, "-m", "kprn_amd.train"] + FLAGS.split() + ["-dataDir", root, "-numEpochs", "2", "-evaluationFrequency", "1", "-gpuid", "0", "-createExptDir", "0"]
    r = subprocess.run(tr + ["-rank_samples", samp_file, "-rank_entity", ent_file, "-testList", "test.list"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    # (a hook of frequency 1 also runs once before the first epoch, MyOptimizer.lua:65-70)
    assert r.stdout.count("evaluation at epoch") == 3 and "evaluation at epoch 0 " in r.stdout and "evaluation at epoch 2 " in r.stdout and "over 60 samples" in r.stdout and "hit@10" in r.stdout
    r = subprocess.run(tr, capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "evaluation at epoch" not in r.stdout
