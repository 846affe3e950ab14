"""-m gpu: the scoring stage (kprn_amd/csrc/score_stages.hip) -- what the ranking and explanation tests leave open in the code that scores, ranks and explains
through ONE body each: the page-locked probability mirror against the copy route, the grow-only buffers when they are replaced and then reused, the one
recommend body with and without its explanation launch, refusals while the mirror is armed, and a split pass whose rest runs on the rest stream and is read
through a board put.  The order of puts, reads and ranking calls is tests/test_gpu_rank.py's.

Every comparison is array_equal / bytes-equal: a scoring pass has no atomics, and nothing here trains (or trains with lr = 0), so each call is a function of its
inputs and every result equals what a fresh engine returns for that one call."""
import ctypes as C

import numpy as np
import pytest

from kprn_amd import _ffi, synth

pytestmark = pytest.mark.gpu

T, F, VE = 6, 3, 300
TOPK = ("topk_idx", "topk_score")
PATHS = ("path_idx", "path_score", "path_weight")


def mk(**options):
    """the fused configuration of the ranking and explanation tests: D = H = 64, two layers, dt = dr = 16, de = 32.  The pad rows are zeroed at once, as a
    training step's first act would: a step with lr = 0 then leaves every parameter as it is, and finds nothing to do before its forward"""
    eng = _ffi.Engine(6, VE, 9, 16, 32, 16, 64, 2, seed=3, param_init=0.35)
    for k, v in options.items():
        eng.set_option(k, v)
    eng.zero_pad_tokens()
    return eng


def ragged(B, seed):
    """(idx [N,T,F], counts [B], labels [B]); counts from synth.draw_num_paths"""
    return synth.make_ragged(B, T, Ve=VE, seed=seed)


def groups(B, G, seed):
    """G group sizes >= 1 that add up to B"""
    cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, B), G - 1, replace=False))
    return np.diff(np.concatenate([[0], cuts, [B]])).astype(np.int32)


def same(got, want, what):
    assert (got is None) == (want is None), what
    if got is not None:
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def same_dict(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        same(got[k], want[k], f"{what}: {k}")


def fresh(call, **options):
    """call(engine) on an engine that has done nothing else"""
    eng = mk(**options)
    out = call(eng)
    eng.close()
    return out


# ---- the calls of the stage, each as engine -> dict of arrays ---------------------------------------------------------------------------------------
def c_forward(idx, counts):
    def call(eng):
        return eng.forward(eng.batch_ragged(idx, counts), 1, want=("probs", "all_probs", "pooled", "path_scores"))
    return call


def c_forward_ragged(idx, counts):
    def call(eng):
        probs, allp = eng.forward_ragged_host(idx, counts, 1, want_all=True)
        return dict(probs=probs, all_probs=allp)
    return call


def c_recommend(idx, counts, gc, K, want_probs=True):
    def call(eng):
        ti, ts, probs = eng.recommend_ragged(idx, counts, gc, K, want_probs=want_probs)
        return dict(topk_idx=ti, topk_score=ts, probs=probs)
    return call


def c_recommend_explain(idx, counts, gc, K, M, want_probs=True):
    def call(eng):
        return eng.recommend_explain_ragged(idx, counts, gc, K, M, want_probs=want_probs)
    return call


def c_explain(idx, counts, M, pairs):
    def call(eng):
        return eng.explain_batch(eng.batch_ragged(idx, counts), M, 1, pairs=pairs)
    return call


def c_rank_board(scores, gc, K):
    def call(eng):
        eng.board_reserve(len(scores))
        eng.board_write(0, scores)
        return eng.rank_groups(np.concatenate([[0], np.cumsum(gc)]).astype(np.int64), mode=0, K=K)
    return call


def c_train_lr0(idx, counts, labels):
    def call(eng):
        return dict(loss=np.float32(eng.train_step(eng.batch_ragged(idx, counts, labels), _ffi.make_opt(method=1, lr=0.0))))
    return call


# ---- 1. mirror route against copy route ----------------------------------------------------------------------------------------------------------
def test_profiling_takes_the_copy_route_and_returns_the_same_bits():
    idx, counts, _ = ragged(150, 11)
    gc = groups(150, 7, 12)
    calls = [("forward_batch", c_forward(idx, counts), ()),
             ("recommend_ragged", c_recommend(idx, counts, gc, 5), ("rank_groups",)),
             ("recommend_explain_ragged", c_recommend_explain(idx, counts, gc, 5, 3), ("rank_groups", "explain_paths"))]
    eng = mk()
    for name, call, families in calls:
        eng.profile(False)
        mirrored = call(eng)
        eng.profile(True)
        eng.profile_reset()
        copied = call(eng)
        prof = eng.profile_get()
        same_dict(copied, mirrored, name)
        for fam in families:
            assert fam in prof, (name, fam, sorted(prof))
        eng.profile(False)
        same_dict(call(eng), mirrored, name + ", the mirror again")
    eng.close()


# ---- 2. buffers that grow and are then reused ------------------------------------------------------------------------------------------------------
def test_buffers_grow_and_are_reused():
    """small -> large -> small on one engine.  Large: B = 400 > 2 * 40 + 64 (the probability mirror), G * K * M = 12 * 8 * 8 = 48 times 4 * 2 * 2 (the page-locked
    top-K and explanation rows hold twice the first need + 256 bytes; the device blocks a quarter more than the need)"""
    small = dict(B=40, G=4, K=2, M=2, seed=21)
    large = dict(B=400, G=12, K=8, M=8, seed=23)
    assert large["B"] > 2 * small["B"] + 64 and large["G"] * large["K"] * large["M"] >= 4 * small["G"] * small["K"] * small["M"]

    def calls_of(B, G, K, M, seed):
        idx, counts, _ = ragged(B, seed)
        gc = groups(B, G, seed + 1)
        rng = np.random.default_rng(seed + 2)
        pairs = rng.integers(0, B, B // 2).astype(np.int32)
        board = rng.standard_normal(B).astype(np.float32)
        return [("recommend_explain", c_recommend_explain(idx, counts, gc, K, M)),
                ("explain_batch", c_explain(idx, counts, 2 * M, pairs)),
                ("recommend", c_recommend(idx, counts, gc, K)),
                ("rank_groups", c_rank_board(board, gc, K)),
                ("forward_ragged", c_forward_ragged(idx, counts)),
                ("recommend, no probs", c_recommend(idx, counts, gc, K, want_probs=False))]

    eng = mk()
    for size, shape in (("small", small), ("large", large), ("small again", small)):
        for name, call in calls_of(**shape):
            same_dict(call(eng), fresh(call), f"{size}: {name}")
    eng.close()


# ---- 3. the merged recommend body ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 9])
def test_recommend_explain_is_recommend_plus_explain(K):
    idx, counts, _ = ragged(60, 31)
    gc = np.array([20, 3, 1, 30, 6], np.int32)        # K = 9: three groups have fewer members, their rows are padded
    goff = np.concatenate([[0], np.cumsum(gc)])
    M = 4
    eng = mk()
    r = eng.recommend_explain_ragged(idx, counts, gc, K, M, want_probs=True)
    ti, ts, probs = eng.recommend_ragged(idx, counts, gc, K, want_probs=True)
    same(r["topk_idx"], ti, "top-K rows")
    same(r["topk_score"], ts, "top-K scores")
    same(r["probs"], probs, "probabilities")
    valid = ti >= 0
    assert np.array_equal(valid.sum(1), np.minimum(K, gc))
    pairs = (goff[:-1, None] + ti)[valid].astype(np.int32)
    e = eng.explain_batch(eng.batch_ragged(idx, counts), M, 1, pairs=pairs)
    for k in PATHS:
        same(np.ascontiguousarray(r[k][valid]), e[k], k)
        assert np.all(r[k][~valid] == (-1 if k == "path_idx" else 0)), k
    eng.close()


# ---- 4. refusals leave nothing armed -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_armed():
    """every refusal is an argument check: nothing reaches the device with bad data"""
    idx, counts, labels = ragged(50, 41)
    idx, counts = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(counts, np.int32)
    B, N = len(counts), len(idx)
    gc = groups(B, 5, 42)
    K, M = 3, 2
    eng = mk()
    L, h = eng.L, eng.h
    batch = eng.batch_ragged(idx, counts)
    probs = np.empty(B, np.float32)
    gcp = np.ascontiguousarray(gc)
    ti, ts = np.empty((5, K), np.int32), np.empty((5, K), np.float32)
    pi, ps, pw = np.empty((5, K, M), np.int32), np.empty((5, K, M), np.float32), np.empty((5, K, M), np.float32)
    p = _ffi._fp

    def recommend(group_counts):
        g = np.ascontiguousarray(group_counts, np.int32)
        return L.kprn_recommend_ragged(h, p(idx), p(counts), B, C.c_int64(N), T, F, 1, p(g), len(g), 0, K, p(ti), p(ts), p(probs))

    def recommend_explain(group_counts=gcp, m=M, path_idx=pi):
        g = np.ascontiguousarray(group_counts, np.int32)
        return L.kprn_recommend_explain_ragged(h, p(idx), p(counts), B, C.c_int64(N), T, F, 1, p(g), len(g), 0, K, m, p(ti), p(ts), p(path_idx), p(ps), p(pw),
                                               p(probs))

    short = gc.copy()
    short[0] += 1
    class_text = "classId must be in 1..C (nn.Select(2,classId), MyOptimizer.lua:126)"
    sum_text = "group_counts do not add up to B"
    refusals = [(lambda: L.kprn_forward_batch(h, batch.ptr, 47, p(probs), None, None, None), class_text),
                (lambda: L.kprn_forward_batch(h, batch.ptr, 0, p(probs), None, None, None), class_text),
                (lambda: recommend(short), sum_text),
                (lambda: recommend_explain(short), sum_text),
                (lambda: recommend_explain(m=0), "M must be in 1..32"),
                (lambda: recommend_explain(m=33), "M must be in 1..32"),
                (lambda: recommend_explain(path_idx=None), "path_idx, path_score and path_weight are required")]
    follow_ups = [("forward_batch", c_forward(idx, counts)),
                  ("recommend_ragged", c_recommend(idx, counts, gc, K)),
                  ("recommend_explain_ragged", c_recommend_explain(idx, counts, gc, K, M)),
                  ("train_step, lr = 0", c_train_lr0(idx, counts, labels))]
    want = {name: fresh(call) for name, call in follow_ups}
    for refused, text in refusals:
        assert refused() == _ffi.E_ARG
        assert L.kprn_last_error(h).decode() == text
        for name, call in follow_ups:
            same_dict(call(eng), want[name], f"{name} after '{text}'")
    eng.close()


# ---- 5. a split pass whose rest runs on the rest stream ---------------------------------------------------------------------------------------------
def test_split_pass_with_its_rest_on_the_rest_stream_read_and_put():
    """score_split = 0.5 over 65 tiles of 64 paths, the rest placed by the training step's backward on the rest stream ("score_rest_before_bptt"); the step trains
    with lr = 0, so the pass reads the parameters the third engine scores with"""
    idx, counts, labels = ragged(2400, 81)
    B = len(counts)
    assert len(idx) > 4032 and (len(idx) + 63) // 64 >= 64
    split = dict(small_tiles="0", score_overlap="1", score_split="0.5", score_rest_before_bptt="1")
    opt = _ffi.make_opt(method=1, lr=0.0)
    want = fresh(lambda eng: eng.forward(eng.batch_ragged(idx, counts), 1)["probs"], small_tiles="0")

    eng = mk(**split)
    batch = eng.batch_ragged(idx, counts, labels)
    eng.forward_async(batch, 1)
    eng.train_step(batch, opt)
    same(eng.read_probs(B), want, "read_probs")
    eng.close()

    eng = mk(**split)
    batch = eng.batch_ragged(idx, counts, labels)
    eng.board_reserve(B + 7)
    eng.forward_async(batch, 1)
    eng.train_step(batch, opt)
    eng.board_put(7, B)
    same(eng.board_read(7, B), want, "board_put + board_read")
    assert np.all(np.isnan(eng.board_read(0, 7)))
    eng.close()
