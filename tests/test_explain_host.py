"""not gpu: the explanation rule (include/kprn.h "explaining a recommendation") -- kprn_host_explain, the host twin of kprn_amd/csrc/explain_paths.hip and
compiled from the same rule source, against a plain numpy float64 restatement over generated score matrices.

Bounds.  Indices, scores, Max / TopK weights: equality (they are selected or copied fp32 values; 1 / kk is one fp32 division).  LogSumExp weights against
float64 on the same fp32 scores: (a + 8) * 2^-24 absolute, a = the longest chain of dependent additions of the form that ran -- cnt for a pair of at most 28
paths (serial sum), ceil(cnt / 64) + 6 for a longer one (64 strided partial sums, then a 6-level tree); the 8 covers expf, the subtraction and the division.
Every term of that error is relative to the weight, so a pair's weights sum to 1 within the same bound.  pooled (LogSumExp) = logf(sum) + m: the sum's
relative error (a + 8) * 2^-24 becomes absolute through the logarithm, plus logf's and the final addition's rounding, 2^-22 * max(1, |pooled|)."""
import numpy as np
import pytest

from kprn_amd import _ffi

COUNTS = (1, 2, 28, 29, 64, 65, 4096)
MS = (1, 3, 32)
C_ = 4
K_RED = 5


def adds(cnt):
    return cnt if cnt <= 28 else -(-cnt // 64) + 6


def bound(cnt):
    return (adds(cnt) + 8) * 2.0 ** -24


def rule64(s32, reducer, K):
    """the rule in float64 over one pair's fp32 scores -> (order, weights of every path, pooled)"""
    s = s32.astype(np.float64)
    cnt = len(s)
    order = np.lexsort((np.arange(cnt), -s))       # score descending, index ascending among equals (-0.0 == 0.0)
    w = np.zeros(cnt)
    if reducer == 2:
        m = s.max()
        e = np.exp(s - m)
        w = e / e.sum()
        pooled = np.log(e.sum()) + m
    elif reducer == 0:
        w[order[0]] = 1.0
        pooled = s[order[0]]
    else:
        kk = min(K, cnt)
        w[order[:kk]] = float(np.float32(1.0) / np.float32(kk))
        pooled = s[order[:kk]].sum() / kk
    return order, w, pooled


def families(rng):
    """name -> (path_scores [N, C_], offsets [B+1]): every count of COUNTS in each"""
    counts = np.array(COUNTS + (3, 1, 31, 32, 33, 100), np.int32)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    N = int(off[-1])
    fam = {}
    fam["normal"] = rng.normal(0, 2, (N, C_)).astype(np.float32)
    fam["wide"] = (rng.normal(0, 1, (N, C_)) * 30).astype(np.float32)                   # most weights underflow towards 0
    fam["halves"] = (np.round(rng.normal(0, 1, (N, C_)) * 2) / 2).astype(np.float32)    # heavy ties
    blocks = np.repeat(rng.normal(0, 1, (N // 7 + 1, C_)), 7, axis=0)[:N].astype(np.float32)   # blocks of 7 equal scores
    fam["blocks"] = blocks
    fam["equal"] = np.full((N, C_), 0.25, np.float32)
    z = np.where(rng.random((N, C_)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)   # +0 and -0 tie
    z[rng.random((N, C_)) < 0.1] = -1.5
    fam["zeros"] = z
    return {k: (v, off) for k, v in fam.items()}


def check_against_rule64(res, sc, off, pairs, class_id, reducer, K, M, weight_bound=bound):
    """the checks of this file on one result dict; also used by tests/test_gpu_explain.py on the device's results (weight_bound: per pair count)"""
    for i, b in enumerate(pairs):
        s32 = sc[off[b]:off[b + 1], class_id - 1]
        cnt = len(s32)
        order, w, pooled = rule64(s32, reducer, K)
        n = min(M, cnt)
        assert np.array_equal(res["path_idx"][i, :n], order[:n]), (i, b, cnt)
        assert np.all(res["path_idx"][i, n:] == -1) and np.all(res["path_score"][i, n:] == 0) and np.all(res["path_weight"][i, n:] == 0)
        assert res["path_score"][i, :n].tobytes() == s32[order[:n]].tobytes()
        got = res["path_weight"][i, :n].astype(np.float64)
        if reducer == 2:
            err = np.abs(got - w[order[:n]]).max()
            assert err <= weight_bound(cnt), (i, b, cnt, err, weight_bound(cnt))
        else:
            assert np.array_equal(got, w[order[:n]]), (i, b, cnt)
        if cnt <= M:
            assert abs(got.sum() - 1.0) <= weight_bound(cnt), (i, b, cnt, got.sum())


@pytest.mark.parametrize("reducer", [2, 0, 1])
def test_host_twin_equals_the_float64_rule(reducer):
    rng = np.random.default_rng(17)
    worst = 0.0
    for name, (sc, off) in families(rng).items():
        B = len(off) - 1
        for class_id in (1, 3):
            for M in MS:
                res = _ffi.host_explain(sc, off, class_id, reducer, K_RED, M)
                check_against_rule64(res, sc, off, range(B), class_id, reducer, K_RED, M)
                for b in range(B):
                    s32 = sc[off[b]:off[b + 1], class_id - 1]
                    _, _, pooled = rule64(s32, reducer, K_RED)
                    tol = 0.0 if reducer == 0 else (bound(len(s32)) if reducer == 2 else K_RED ** 2 * 2.0 ** -24 * np.abs(s32).max()) + 2.0 ** -22 * max(1.0, abs(pooled))
                    assert abs(float(res["pooled"][b]) - pooled) <= tol, (name, b, res["pooled"][b], pooled)
                    p = 1.0 / (1.0 + np.exp(-float(res["pooled"][b])))
                    assert abs(float(res["probs"][b]) - p) <= 2.0 ** -22
                    if reducer == 2:
                        o, w, _ = rule64(s32, reducer, K_RED)
                        n = min(M, len(s32))
                        worst = max(worst, np.abs(res["path_weight"][b, :n] - w[o[:n]]).max() / bound(len(s32)))
            # a pair subset with repeats, in any order
            pairs = np.array([B - 1, 0, 6, 6, 3, 0], np.int32)
            res = _ffi.host_explain(sc, off, 2, reducer, K_RED, 3, pairs=pairs)
            check_against_rule64(res, sc, off, pairs, 2, reducer, K_RED, 3)
            every = _ffi.host_explain(sc, off, 2, reducer, K_RED, 3)
            for k in ("path_idx", "path_score", "path_weight", "pooled", "probs"):
                assert res[k].tobytes() == every[k][pairs].tobytes(), k
    print("worst LogSumExp weight error / bound: %.3f" % worst)


def test_topk_reducer_with_k_above_and_below_the_count():
    rng = np.random.default_rng(3)
    sc = rng.normal(0, 1, (40, 2)).astype(np.float32)
    off = np.array([0, 3, 10, 40], np.int32)
    for K in (1, 5, 64):
        res = _ffi.host_explain(sc, off, 2, 1, K, 32)
        check_against_rule64(res, sc, off, range(3), 2, 1, K, 32)
        for b, cnt in enumerate((3, 7, 30)):
            assert np.count_nonzero(res["path_weight"][b]) == min(K, cnt)


def test_nan_scores_sort_last_lower_index_first():
    s = np.array([np.nan, 1.0, np.nan, 3.0, -np.inf, np.inf], np.float32)[:, None]
    res = _ffi.host_explain(s, np.array([0, 6], np.int32), 1, 0, 1, 6)
    assert res["path_idx"][0].tolist() == [5, 3, 1, 4, 0, 2]


def test_refusals_write_nothing():
    rng = np.random.default_rng(1)
    sc = rng.normal(0, 1, (20, C_)).astype(np.float32)
    off = np.array([0, 5, 6, 20], np.int32)

    def call(M=3, pairs=None, class_id=1, reducer=2, K=5, off_=off, sc_=sc):
        n = 3 if pairs is None else len(pairs)
        out = dict(path_idx=np.full((n, max(M, 1)), -7, np.int32), path_score=np.full((n, max(M, 1)), -7, np.float32),
                   path_weight=np.full((n, max(M, 1)), -7, np.float32), pooled=np.full(n, -7, np.float32), probs=np.full(n, -7, np.float32))
        try:
            _ffi.host_explain(sc_, off_, class_id, reducer, K, M, pairs=pairs, out=out)
            code = 0
        except _ffi.KprnError as e:
            code = e.code
        return code, all(bool(np.all(v == -7)) for v in out.values())

    assert call() == (0, False)
    assert call(M=32)[0] == 0
    for M in (0, 33, -1):
        assert call(M=M) == (_ffi.E_ARG, True)
    for pairs in ([0, 3], [-1], [2, 1, 0, 1000000]):
        assert call(pairs=pairs) == (_ffi.E_INDEX, True)
    assert call(pairs=[2, 2, 0])[0] == 0
    for cid in (0, C_ + 1):
        assert call(class_id=cid) == (_ffi.E_ARG, True)
    for red in (-1, 3):
        assert call(reducer=red) == (_ffi.E_ARG, True)
    assert call(reducer=1, K=0) == (_ffi.E_ARG, True)
    assert call(off_=np.array([0, 5, 5, 20], np.int32)) == (_ffi.E_ARG, True)          # an empty pair
    big = np.zeros((4100, C_), np.float32)
    assert call(off_=np.array([0, 1, 2, 4099], np.int32), sc_=big) == (_ffi.E_ARG, True)   # a pair of 4097 paths
    assert call(off_=np.array([0, 1, 2, 4098], np.int32), sc_=big)[0] == 0
    with pytest.raises(_ffi.KprnError):
        _ffi.host_explain(sc, np.array([0, 5, 21], np.int32), 1, 2, 5, 3)              # offsets past the matrix
