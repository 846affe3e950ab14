"""-m gpu: option "head_select" (kprn_amd/csrc/lstm_fused_fwd.hip head_tile_sel): the fused fp32 forward's nn.Linear(H, C) head forms column
classId alone wherever no reader of the pass needs another column -- the training forward, and every scoring pass whose caller reads the selected class only.

The change is built so that NO BIT MOVES: an MFMA output element depends on its A row and its B column only, and the selected head keeps the every-class head's
accumulation chain per row.  So every comparison here is "head_select" = 1 against 0 on fresh engines from the same seed, and is exact (np.array_equal): a
tolerance would hide a wrong row or column.  The route is asserted through the profiler: a pass that took the selected-class head leaves the (empty) family
"head_select" behind, one entry per pass.

Shapes: both head sites (the head of the tile before inside a tile's first slot, and the drain's) need a workgroup that owns two tiles; both row edges need a
partly filled last tile.  Scoring gets there with "reserve_cus" (4 workgroups, 5 full tiles + 3 rows), training -- whose forward ignores that option -- with one
tile more than the chip has CUs, + 5 rows, at T = 2."""
import numpy as np
import pytest

from kprn_amd import _ffi, synth

pytestmark = pytest.mark.gpu
T = 6
VE = 2000
FAMILY = "head_select"


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def mk(hs, L=2, C=46, small_tiles="0", plan="1", stf="1", options=()):
    eng = _ffi.Engine(6, VE, 9, 16, 32, 16, 64, L, C_=C)
    eng.set_option("head_select", str(hs))
    eng.set_option("small_tiles", small_tiles)
    eng.set_option("prefix_plan", plan)
    eng.set_option("small_tables_fwd", stf)
    for k, v in options:
        eng.set_option(k, v)
    rng = np.random.default_rng(11)
    eng.set_flat_params((rng.random(eng.n_params) * 0.2 - 0.1).astype(np.float32))
    return eng


def paths(n, Tt=T, padded=True, seed=3):
    """n pairs of one path; padded: 73 % of the paths start with two pad steps (what the identical-prefix plan sorts into tiles of their own: perm)"""
    return synth.make_paths(n, 1, Tt, Ve=VE, seed=seed, real_len=None if padded else Tt)


def marks(eng):
    fam = eng.profile_get()
    return fam[FAMILY][1] if FAMILY in fam else 0


def both(fn, **kw):
    """fn(engine, head_select) on a fresh engine per side -> (result with the option on, result with it off)"""
    out = []
    for hs in (1, 0):
        eng = mk(hs, **kw)
        try:
            out.append(fn(eng, hs))
        finally:
            eng.close()
    return out


def same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and np.array_equal(x, y), (i, int(np.sum(x != y)), float(np.max(np.abs(x.astype(np.float64) - y))))
        assert np.all(np.isfinite(x)), i


# C = 46: both sides of each 16-column tile edge and the last live column; C = 1, 16, 17: first and last class
@pytest.mark.parametrize("C,cids", [(46, (1, 16, 17, 32, 33, 46)), (1, (1,)), (16, (1, 16)), (17, (1, 17))])
def test_probabilities_of_every_class_id(C, cids):
    idx, labels = paths(5 * 64 + 3)

    def run(eng, hs):
        b = eng.batch(idx, labels)
        eng.profile(True)
        res = [eng.forward(b, cid)["probs"].copy() for cid in cids]
        assert marks(eng) == (len(cids) if hs else 0), eng.profile_get()
        return res
    on, off = both(run, C=C)
    same(on, off)
    if len(cids) > 1:
        assert not np.array_equal(on[0], on[-1])   # (the class id reaches the head)


# (L, small_tables_fwd, 16-row tiles): L = 1 has no 16-row instantiation
ROUTES = [(2, "1", "0"), (2, "1", "1"), (2, "0", "0"), (2, "0", "1"), (1, "1", "0")]


@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("L,stf,small", ROUTES)
def test_scoring_both_head_sites_and_row_edges(cus, L, stf, small, padded):
    """4 workgroups walk 6 tiles: workgroups 0 and 1 form their first tile's head inside their second tile's first slot, all four the drain's; the last tile
    has 3 live rows"""
    rows = 16 if small == "1" else 64
    n = 5 * rows + 3
    idx, labels = paths(n, padded=padded, seed=7 + L)

    def run(eng, hs):
        b = eng.batch(idx, labels)
        if small == "0" and padded:
            assert b.executed_steps < n * T     # a plan: the tiles hold the paths in another order (perm)
        else:
            assert b.executed_steps == n * T
        eng.profile(True)
        res = [eng.forward(b, cid)["probs"].copy() for cid in (17, 46)]
        assert marks(eng) == (2 if hs else 0), eng.profile_get()
        return res
    same(*both(run, L=L, small_tiles=small, stf=stf, options=(("reserve_cus", str(cus - 4)),)))


def _train(idx, labels, steps, det, **kw):
    def run(eng, hs):
        if det:
            eng.set_option("deterministic", "1")
        b = eng.batch(idx, labels) if not isinstance(idx, tuple) else eng.batch_ragged(idx[0], idx[1], labels)
        opt = _ffi.make_opt(method=1, lr=2e-3)
        eng.profile(True)
        losses = [eng.train_step(b, opt, class_id=17) for _ in range(steps)]
        fam = eng.profile_get()
        assert any(k.startswith("lstm_fused_fwd") for k in fam), sorted(fam)
        assert marks(eng) == (steps if hs else 0), fam
        # every dense parameter and every entity row (the touched ones among them)
        return [np.array(losses, np.float32)] + ([eng.get_flat_params()] if det else [])
    return both(run, **kw)


@pytest.mark.parametrize("plan", ["1", "0"])
@pytest.mark.parametrize("L,stf,small", ROUTES)
def test_training_both_head_sites_and_row_edges(cus, L, stf, small, plan):
    """one tile more than the chip has CUs, + 5 rows, at T = 2: workgroup 0 owns two tiles, workgroup 1 the partly filled one.  With "deterministic" three Adam
    steps leave every parameter bit-equal; without it the gradients' atomics make runs drift, and only the first step's loss is compared"""
    rows = 16 if small == "1" else 64
    idx, labels = paths(rows * (cus + 1) + 5, Tt=2, seed=13)
    kw = dict(L=L, small_tiles=small, stf=stf, plan=plan)
    same(*_train(idx, labels, 3, True, **kw))
    same(*_train(idx, labels, 1, False, **kw))


def test_training_with_an_identical_prefix_plan(cus):
    """the same number of tiles at T = 6 with left-padded paths: T = 2 leaves the plan nothing to skip, here the training forward writes S through perm"""
    n = 64 * (cus + 1) + 5
    idx, labels = paths(n, seed=17)
    eng = mk(1)
    assert eng.batch(idx, labels).executed_steps < n * T
    eng.close()
    same(*_train(idx, labels, 3, True))
    same(*_train(idx, labels, 1, False))


def test_ragged_batch():
    idx, counts, labels = synth.make_ragged(150, T, Ve=VE, seed=19)

    def run(eng, hs):
        b = eng.batch_ragged(idx, counts, labels)
        eng.profile(True)
        res = [eng.forward(b, 33)["probs"].copy()]
        assert marks(eng) == (1 if hs else 0)
        return res
    for small in ("0", "1"):
        same(*both(run, small_tiles=small))
        same(*_train((idx, counts), labels, 3, True, small_tiles=small))


def test_split_pass(cus):
    """"score_split": the first tiles on the side stream, the others behind kprn_forward_batch_async_rest -- two launches, each with the pass's class id"""
    idx, labels = paths(70 * 64 + 3, seed=23)

    def run(eng, hs):
        b = eng.batch(idx, labels)
        eng.profile(True)
        eng.forward_async(b, 32)
        eng.forward_async_rest()
        res = [eng.read_probs(b.B).copy()]
        fam = eng.profile_get()
        assert fam["lstm_fused_fwd"][1] == 2, fam
        assert marks(eng) == (2 if hs else 0), fam
        return res
    same(*both(run, options=(("score_overlap", "1"), ("score_split", "0.5"))))


@pytest.mark.parametrize("small", ["1", "0"])
def test_pass_riding_in_the_training_forward_selects_its_own_class(small):
    """"score_dual": the two branches of k_lstm_fwd_dual carry different class ids.  (One batch for both passes: the row catch-up of another batch's training
    step would write parameters the queued pass reads, and the pass would run ahead of it the usual way.)"""
    idx, labels = paths(5 * 64 + 3, seed=29)

    def run(eng, hs):
        b = b2 = eng.batch(idx, labels)
        opt = _ffi.make_opt(method=1, lr=0.0)   # (the parameters stay where they are: the passes below are comparable bit for bit)
        eng.train_step(b, opt, class_id=2)      # (a new engine's first step zeroes the pad rows first: a queued pass would run ahead of it, the usual way)
        eng.profile(True)
        eng.forward_async(b2, 33)
        loss = eng.train_step(b, opt, class_id=2)
        dual = eng.read_probs(b2.B).copy()
        fam = eng.profile_get()
        assert "lstm_fused_fwd_dual" in fam, sorted(fam)
        assert marks(eng) == (2 if hs else 0), fam
        eng.profile(False)
        return [dual, np.float32(loss), eng.forward(b2, 33)["probs"].copy(), eng.forward(b2, 2)["probs"].copy()]
    on, off = both(run, small_tiles=small, options=(("score_overlap", "1"), ("score_dual", "1")))
    same(on, off)
    assert np.array_equal(on[0], on[2]) and not np.array_equal(on[0], on[3])   # the pass scored ITS class, not the training step's


@pytest.mark.parametrize("want", ["all_probs", "pooled", "path_scores"])
def test_every_class_callers_take_the_every_class_head(want):
    idx, labels = paths(5 * 64 + 3, seed=37)

    def run(eng, hs):
        b = eng.batch(idx, labels)
        eng.profile(True)
        out = eng.forward(b, 17, want=("probs", want))
        assert marks(eng) == 0, eng.profile_get()
        assert out[want].shape[1] == 46
        return [out["probs"].copy(), out[want].copy()]
    same(*both(run))


def test_stale_columns_are_rewritten_by_an_every_class_call():
    """a selected-class pass leaves the other columns of S as they were; an every-class call on the same batch for another class id rewrites all of them"""
    idx, labels = paths(5 * 64 + 3, seed=41)
    want = ("probs", "all_probs", "pooled", "path_scores")
    eng = mk(1)
    b = eng.batch(idx, labels)
    eng.profile(True)
    eng.forward(b, 3)
    assert marks(eng) == 1
    after = eng.forward(b, 7, want=want)
    assert marks(eng) == 1
    eng.close()
    fresh_eng = mk(1)
    fresh = fresh_eng.forward(fresh_eng.batch(idx, labels), 7, want=want)
    fresh_eng.close()
    same([after[k] for k in want], [fresh[k] for k in want])


def test_board_and_explain_read_the_selected_column():
    """the other readers of a selected-class pass: kprn_board_put (the pooled probabilities) and kprn_explain_batch (S[:, cid] itself)"""
    idx, labels = synth.make_paths(80, 4, T, Ve=VE, seed=43)

    def run(eng, hs):
        b = eng.batch(idx, labels)
        eng.board_reserve(b.B)
        eng.profile(True)
        eng.forward(b, 16)
        eng.board_put(0, b.B)
        board = eng.board_read(0, b.B).copy()
        ex = eng.explain_batch(b, 3, class_id=16)
        assert marks(eng) == (2 if hs else 0), eng.profile_get()
        ex = ex if isinstance(ex, (tuple, list)) else [ex[k] for k in sorted(ex)]
        return [board] + [np.asarray(v) for v in ex]
    same(*both(run))
