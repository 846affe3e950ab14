"""gpu: the explanation stage on the device (include/kprn.h "explaining a recommendation"; kprn_amd/csrc/explain_paths.hip) -- kprn_explain_batch against its
host twin fed the device's own path scores, against the float64 oracle, kprn_recommend_explain_ragged against recommend_ragged + explain_batch, the score
CLI's -explain_out end to end, and the refusals.

Bounds.  path_idx / path_score and the Max / TopK weights: equality with the twin.  pooled / probs: the bits of column class_id of Engine.forward's outputs
(the forward pass has no atomics and is bit-reproducible: tests/test_gpu_fwd_identity.py).  LogSumExp weights against float64 on the same fp32 scores, and
against the twin: (a + 8) * 2^-24 absolute (tests/test_explain_host.py derives it; a = cnt for a pair of at most 28 paths, ceil(cnt / 64) + 6 above).
Against the float64 oracle (its own scores, so near-tie orders may differ: weights are compared path by path): 2e-4 absolute, the project's gradient bar --
the weights are the reducer's gradient and at most 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kprn_amd import _ffi, formats, model, scoring, synth
from tests.test_explain_host import bound, check_against_rule64
from tests.test_gpu_ragged import mk as mk_with_oracle, oracle_forward

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("path_idx", "path_score", "path_weight", "pooled", "probs")
REDUCERS = [(2, 5), (0, 5), (1, 5)]


def mk(reducer=2, K=5, seed=3, Ve=300, **kw):
    return _ffi.Engine(6, Ve, 9, 16, 32, 16, 64, 2, seed=seed, reducer=reducer, K=K, param_init=0.35, **kw)


def against_twin(eng, batch, off, class_id, M, pairs=None, stats=None):
    """one explain_batch call against the host twin on the device's own path scores and against the float64 rule; -> the device's dict"""
    c = eng.cfg
    fwd = eng.forward(batch, class_id, want=("probs", "pooled", "path_scores"))
    dev = eng.explain_batch(batch, M, class_id, pairs=pairs)
    host = _ffi.host_explain(fwd["path_scores"], off, class_id, c.reducer, c.K, M, pairs=pairs)
    sel = np.arange(len(off) - 1) if pairs is None else np.asarray(pairs)
    assert dev["path_idx"].tobytes() == host["path_idx"].tobytes()
    assert dev["path_score"].tobytes() == host["path_score"].tobytes()
    assert dev["pooled"].tobytes() == np.ascontiguousarray(fwd["pooled"][sel, class_id - 1]).tobytes()
    assert dev["probs"].tobytes() == np.ascontiguousarray(fwd["probs"][sel]).tobytes()
    if c.reducer != 2:
        assert dev["path_weight"].tobytes() == host["path_weight"].tobytes()
    else:
        cnt = np.diff(off)[sel]
        tol = np.array([bound(int(n)) for n in cnt])[:, None]
        err = np.abs(dev["path_weight"].astype(np.float64) - host["path_weight"])
        print("LogSumExp weights, device against twin: worst error / bound = %.3f" % float((err / tol).max()))
        assert np.all(err <= tol), float((err / tol).max())
    check_against_rule64(dev, fwd["path_scores"], off, sel, class_id, c.reducer, c.K, M)
    if stats is not None and c.reducer == 2:
        from tests.test_explain_host import rule64
        for i, b in enumerate(sel):
            s32 = fwd["path_scores"][off[b]:off[b + 1], class_id - 1]
            o, w, _ = rule64(s32, 2, c.K)
            n = min(M, len(s32))
            stats.append(float(np.abs(dev["path_weight"][i, :n] - w[o[:n]]).max() / bound(len(s32))))
    return dev


def rect_off(B, P):
    return (np.arange(B + 1, dtype=np.int64) * P).astype(np.int32)


def ragged_off(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


WAVE_COUNTS = np.array([1, 4096, 1, 29, 64, 65, 28, 1, 200, 2], np.int32)


@pytest.mark.parametrize("reducer,K", REDUCERS)
def test_explain_batch_equals_the_host_twin(reducer, K):
    eng = mk(reducer, K)
    rng = np.random.default_rng(4)
    stats = []
    # rectangular: thread form up to 28 paths per pair, wave form above (pooled still in the pooling kernel's serial order)
    for P, B in ((1, 70), (3, 300), (28, 33), (40, 9)):
        idx, _ = synth.make_paths(B, P, 6, Ve=300, seed=20 + P)
        batch = eng.batch(idx)
        off = rect_off(B, P)
        for class_id in (1, 3):
            for M in (1, 3, 32):
                against_twin(eng, batch, off, class_id, M, stats=stats)
        pairs = np.concatenate([rng.integers(0, B, 40), [B - 1, 0, 0]]).astype(np.int32)
        against_twin(eng, batch, off, 3, 5, pairs=pairs, stats=stats)
    # ragged, thread form
    idx, counts, _ = synth.make_ragged(500, 6, Ve=300, seed=31)
    assert counts.max() <= 28
    batch = eng.batch_ragged(idx, counts)
    off = ragged_off(counts)
    for class_id, M in ((1, 3), (3, 32), (1, 1)):
        against_twin(eng, batch, off, class_id, M, stats=stats)
    against_twin(eng, batch, off, 1, 4, pairs=rng.integers(0, 500, 1000).astype(np.int32), stats=stats)
    # ragged, wave form: a 4096-path pair beside single-path pairs
    idx, counts, _ = synth.make_ragged(len(WAVE_COUNTS), 6, Ve=300, seed=32, counts=WAVE_COUNTS)
    batch = eng.batch_ragged(idx, counts)
    off = ragged_off(counts)
    for class_id, M in ((1, 3), (3, 32), (1, 1)):
        against_twin(eng, batch, off, class_id, M, stats=stats)
    against_twin(eng, batch, off, 3, 32, pairs=np.array([1, 1, 0, 9, 1, 4], np.int32), stats=stats)
    if stats:
        print("LogSumExp weights, device against float64 on the same scores: worst error / bound = %.3f" % max(stats))
    eng.close()


@pytest.mark.parametrize("plan", ["1", "0"])
def test_fused_path_with_the_prefix_plan_on_and_off(monkeypatch, plan):
    monkeypatch.setenv("KPRN_SMALL_TILES", "0")   # (64-path tiles at this size too: the plan belongs to them)
    eng = mk()
    eng.set_option("prefix_plan", plan)
    idx, _ = synth.make_paths(200, 3, 6, Ve=300, seed=41)
    against_twin(eng, eng.batch(idx), rect_off(200, 3), 1, 3)
    idx, counts, _ = synth.make_ragged(len(WAVE_COUNTS), 6, Ve=300, seed=42, counts=WAVE_COUNTS)
    against_twin(eng, eng.batch_ragged(idx, counts), ragged_off(counts), 3, 32)
    eng.close()


@pytest.mark.parametrize("reducer,K", REDUCERS)
def test_generic_shape_engine(reducer, K):
    eng = _ffi.Engine(6, 300, 9, 4, 8, 4, 16, 1, seed=5, reducer=reducer, K=K, param_init=0.35)
    idx, _ = synth.make_paths(50, 5, 6, Ve=300, seed=43)
    against_twin(eng, eng.batch(idx), rect_off(50, 5), 1, 3)
    counts = np.array([3, 1, 90, 28, 29, 1], np.int32)
    idx, counts, _ = synth.make_ragged(len(counts), 6, Ve=300, seed=44, counts=counts)
    against_twin(eng, eng.batch_ragged(idx, counts), ragged_off(counts), 3, 32, pairs=np.array([2, 5, 2, 0], np.int32))
    eng.close()


def oracle_weights(s, reducer, K):
    s = np.asarray(s, np.float64)
    w = np.zeros(len(s))
    order = np.lexsort((np.arange(len(s)), -s))
    if reducer == 2:
        e = np.exp(s - s.max())
        return e / e.sum()
    kk = 1 if reducer == 0 else min(K, len(s))
    w[order[:kk]] = 1.0 / kk
    return w


@pytest.mark.parametrize("reducer,K", REDUCERS)
def test_weights_against_the_float64_oracle(reducer, K):
    """the worst |weight - oracle's weight| over every returned path is printed before the assertion (bar 2e-4 absolute)"""
    eng, o64, theta = mk_with_oracle(reducer=reducer, K=K, init=0.35)
    counts = np.array([1, 300, 2, 28, 29, 64, 65, 5, 5, 1, 17], np.int32)
    idx, counts, _ = synth.make_ragged(len(counts), 6, Ve=300, seed=51, counts=counts)
    ps, _, _ = oracle_forward(o64, theta, idx, counts)
    off = ragged_off(counts)
    worst = 0.0
    for class_id in (1, 3):
        dev = eng.explain_batch(eng.batch_ragged(idx, counts), 32, class_id)
        for b in range(len(counts)):
            w = oracle_weights(ps[off[b]:off[b + 1], class_id - 1], reducer, K)
            n = min(32, int(counts[b]))
            q = dev["path_idx"][b, :n]
            assert np.all(q >= 0) and len(set(q.tolist())) == n
            worst = max(worst, float(np.abs(dev["path_weight"][b, :n] - w[q]).max()))
    print("reducer %d: worst |weight - oracle weight| = %.3g (bar 2e-4)" % (reducer, worst))
    assert worst <= 2e-4, worst
    eng.close()


def test_recommend_explain_ragged_equals_recommend_ragged_plus_explain_batch():
    eng = mk()
    rng = np.random.default_rng(9)
    for trial, group_counts in enumerate(([101], rng.integers(1, 40, 37).tolist(), [1], [300, 1, 64, 65, 3])):
        B = int(np.sum(group_counts))
        counts = synth.draw_num_paths(np.random.default_rng(60 + trial), B)
        if trial == 3:
            counts[[5, 300]] = (100, 4096)     # the wave form; pair 300 is the whole second group
        idx, _, _ = synth.make_ragged(B, 6, Ve=300, seed=70 + trial, counts=counts)
        goff = np.concatenate([[0], np.cumsum(group_counts)]).astype(np.int64)
        for mode, K, M in ((0, 10, 3), (1, 64, 32), (0, 1, 1)):
            ti, ts, probs = eng.recommend_ragged(idx, counts, group_counts, K, mode=mode, want_probs=True)
            r = eng.recommend_explain_ragged(idx, counts, group_counts, K, M, mode=mode, want_probs=True)
            assert r["topk_idx"].tobytes() == ti.tobytes() and r["topk_score"].tobytes() == ts.tobytes() and r["probs"].tobytes() == probs.tobytes()
            valid = ti >= 0
            assert np.array_equal(valid.sum(1), np.minimum(K, group_counts))            # groups of n < K members among them
            pairs = (goff[:-1, None] + ti)[valid].astype(np.int32)
            e = eng.explain_batch(eng.batch_ragged(idx, counts), M, 1, pairs=pairs)
            for k in ("path_idx", "path_score", "path_weight"):
                assert r[k].shape == (len(group_counts), K, M)
                assert r[k][valid].tobytes() == e[k].tobytes(), k
                assert np.all(r[k][~valid] == (-1 if k == "path_idx" else 0))
            assert e["probs"].tobytes() == ts[valid].tobytes()
            r2 = eng.recommend_explain_ragged(idx, counts, group_counts, K, M, mode=mode)
            assert r2["probs"] is None and all(r2[k].tobytes() == r[k].tobytes() for k in ("topk_idx", "path_idx", "path_weight"))
    eng.close()


def test_refusals_write_nothing():
    eng = mk()
    idx, _ = synth.make_paths(8, 2, 6, Ve=300, seed=1)
    batch = eng.batch(idx)

    def call(M=3, pairs=None, class_id=1):
        n = 8 if pairs is None else len(pairs)
        m = max(M, 1)
        out = dict(path_idx=np.full((n, m), -7, np.int32), path_score=np.full((n, m), -7, np.float32), path_weight=np.full((n, m), -7, np.float32),
                   pooled=np.full(n, -7, np.float32), probs=np.full(n, -7, np.float32))
        try:
            eng.explain_batch(batch, M, class_id, pairs=pairs, out=out)
            code = 0
        except _ffi.KprnError as e:
            code = e.code
        return code, all(bool(np.all(v == -7)) for v in out.values())

    assert call() == (0, False)
    assert call(M=32)[0] == 0
    for M in (0, 33, -1):
        assert call(M=M) == (_ffi.E_ARG, True)
    for pairs in ([0, 8], [-1], [7, 7, 100000]):
        assert call(pairs=pairs) == (_ffi.E_INDEX, True)
    for cid in (0, 47):
        assert call(class_id=cid) == (_ffi.E_ARG, True)
    bad = idx.copy()
    bad[3, 1, 2, 1] = 301                      # an id outside its vocabulary is refused where the batch is made
    with pytest.raises(_ffi.KprnError) as e:
        eng.explain_batch(eng.batch(bad), 3)
    assert e.value.code == _ffi.E_INDEX
    ri, rc_, _ = synth.make_ragged(6, 6, Ve=300, seed=2)

    def rcall(group_counts, K, M):
        G = len(group_counts)
        m = max(M, 1)
        out = dict(path_idx=np.full((G, K, m), -7, np.int32), path_score=np.full((G, K, m), -7, np.float32), path_weight=np.full((G, K, m), -7, np.float32))
        try:
            eng.recommend_explain_ragged(ri, rc_, group_counts, K, M, out=out)
            code = 0
        except _ffi.KprnError as e:
            code = e.code
        return code, all(bool(np.all(v == -7)) for v in out.values())

    assert rcall([4, 2], 2, 3) == (0, False)
    assert rcall([4, 2], 2, 33) == (_ffi.E_ARG, True)
    assert rcall([4, 2], 2, 0) == (_ffi.E_ARG, True)
    assert rcall([3, 2], 2, 3) == (_ffi.E_ARG, True)
    assert rcall([6], 65, 3) == (_ffi.E_ARG, True)
    assert call() == (0, False)                # the handle is usable after refusals
    eng.close()


# ---- command line -----------------------------------------------------------------------------------------------------------------------------
FLAGS = ("-entityTypeVocabSize 6 -entityVocabSize 500 -relationVocabSize 9 -entityTypeEmbeddingDim 16 -entityEmbeddingDim 32 "
         "-relationEmbeddingDim 16 -numFeatureTemplates 3 -numEntityTypes 1 -rnnType lstm -rnnHidSize 64 -numLayers 2 -topK 2 "
         "-useAdam 1 -learningRate 0.01 -regularize 0 -includeEntity 1 -minibatch 16 -gradientStepCounter 100000")


def test_score_cli_writes_the_explanation_file(tmp_path):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "test"))
    names, files = [], []
    for i, (n, P) in enumerate([(300, 2), (210, 4), (96, 1)]):
        idx, labels = synth.make_paths(n, P, 6, Ve=500, seed=70 + i)
        formats.save_path_file(os.path.join(root, "test/test.txt.%d.npz" % P), labels, idx, 1)
        names.append("test/test.txt.%d.npz" % P)
        files.append(idx)
    total = sum(len(f) for f in files)
    open(os.path.join(root, "test.list"), "w").write("\n".join(names) + "\n")
    params = model.parse_flags(FLAGS.split() + ["-dataDir", root])
    ck = os.path.join(root, "m-latest")
    e0 = model.build_engine(params)
    e0.save(ck)
    e0.close()
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "kprn_amd.score", "-input_dir", root, "-test_list", "test.list", "-model_path", ck, "-top_k", "2", "-gpu_id", "0"]
    M = 3
    out = {}
    for merge in ("0", "1"):
        plain, expl, ex_file = (os.path.join(root, n + merge) for n in ("plain.res", "explained.res", "explain.txt"))
        r = subprocess.run(base + ["-out_file", plain, "-mergePathCounts", merge] + FLAGS.split(), capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run(base + ["-out_file", expl, "-mergePathCounts", merge, "-explain_out", ex_file, "-explain_paths", str(M)] + FLAGS.split(),
                           capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(plain, "rb").read() == open(expl, "rb").read() and len(open(plain).readlines()) == total
        out[merge] = open(ex_file).read().splitlines()
    # the API on the same checkpoint, file by file in list order
    params.reducer, params.K, params.initModel = model.reducer_of_score_flag(2), 5, ck
    eng = model.build_engine(params)
    want, counter = [], 0
    for idx in files:
        res = eng.explain_batch(eng.batch(idx), M, 1)
        for b in range(len(idx)):
            for r_ in range(min(M, idx.shape[1])):
                q = int(res["path_idx"][b, r_])
                want.append((counter + b, r_, q, "%.5f" % res["path_weight"][b, r_], "%.6g" % res["path_score"][b, r_], idx[b, q]))
        counter += len(idx)
    for merge in ("0", "1"):
        assert len(out[merge]) == len(want) == 300 * 2 + 210 * 3 + 96
        for line, (c, place, q, w, s, path) in zip(out[merge], want):
            f = line.split("\t")
            assert len(f) == 6 and (int(f[0]), int(f[1])) == (c, place)
            steps = [tuple(int(v) for v in st.split(",")) for st in f[5].split(" ")]
            if merge == "0":
                assert (int(f[2]), f[3], f[4]) == (q, w, s), (line, q, w, s)
            else:                     # (merged scoring may differ from plain scoring in the last bits, tests/test_gpu_ragged.py: the line's own path_idx is taken)
                k = 0 if c < 300 else (1 if c < 510 else 2)
                path = files[k][c - (0, 300, 510)[k], int(f[2])]
            assert steps == [tuple(int(v) for v in st) for st in path if st[1] != 500], line      # the non-pad steps, in step order
            assert all(len(st) == 3 for st in steps) and 1 <= len(steps) <= 6
    eng.close()
    # with -rank_samples the flags are refused with a message, before anything is scored
    r = subprocess.run(base + ["-out_file", os.path.join(root, "x.res"), "-explain_out", os.path.join(root, "x.txt"), "-rank_samples", "s", "-rank_entity", "e"] +
                       FLAGS.split(), capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode != 0 and "-explain_out cannot be combined with -rank_samples" in r.stderr
    assert not os.path.exists(os.path.join(root, "x.txt"))
    # explain_test_set without a result file, on a file-list batcher
    from kprn_amd.batcher import BatcherFileList
    import io
    eng = model.build_engine(params)
    buf = io.StringIO()
    n = scoring.explain_test_set(eng, BatcherFileList(root, 512, False, 1000, True, "test.list", check_ids=False), buf, M)
    assert n == total and buf.getvalue().splitlines() == out["0"]
    eng.close()
