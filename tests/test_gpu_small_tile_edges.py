"""-m gpu: the 16-row-tile route (fused::small_tiles, the NMT = 1 instantiations of k_lstm_fwd / k_lstm_bwd, k_lstm_fwd_dual, k_lstm_bwd_dual and its _det
variant) at every T, grid regime and hand-over edge -- tests/test_gpu_small_tiles.py and its neighbours hold the route to the float64 oracle at T = 6 only.

Regimes of a batch of t tiles (N = 16 t - r paths) on a chip of `cus` compute units, two layers, default options (lstm_fused_bwd.hip backward):
  t = 1              one workgroup per layer, two BPTT launches (the pipeline borrows epoch and fault word from handover_args, which has none below two workgroups)
  2 <= t <= cus / 2  "bwd_pipe": both layers' BPTT in ONE launch, the bottom layer's workgroup of a tile waiting on pipe_flag[tile][step] for the top layer's dx
  cus / 2 < t <= cus two launches, every workgroup one tile
  cus < t <= 2 cus   workgroups b < t - cus own two tiles; "tile_handover" pairs b with b + cus / 2 (mode 2) or cus - 1 - b (mode 1), and a pair whose loads
                     differ moves d steps of the heavy one's first tile through a slot in global memory.
There is no identical-prefix plan in this mode: every tile costs 2 T - 1 half steps, a pair differs by exactly that, and ho_decide (lstm_fused_common.h) gives
  d = the minimiser of max(heavy - 2 d, light + 2 d), clipped to steps - keep = T - 1:
  T = 2: the difference is 3 half steps, below the rule's threshold of 4 (one full step each way) -- NOTHING moves at T = 2, whatever the tile count;
  T = 3: 5 -> d = 1 (3 | 2 left against 4 | 1 with d = 2);   T = 6: 11 -> d = 3 (5 | 6);   T = 16: 31 -> d = 8 (15 | 16); all below T - 1.
Pairs that move at h = t - cus heavy workgroups: min(h, cus - h) in either pairing mode (a pair of two heavy or two light workgroups moves nothing).

Every case proves its regime first -- the profile's families (fused, not the generic pipeline's), the launches recorded for lstm_fused_bwd (1 per backward when
piped, else 2), Batch.handover_stats -- and compares numbers afterwards.  Bars are the project's own: scores 3e-6 of scale, pooled rtol 1e-4 / atol 2e-6,
probabilities rtol 1e-5, loss 1e-5, every gradient tensor 2e-4 of its largest entry (tests/test_gpu_small_tiles.py); on / off comparisons at the bars of the
tests they extend (tests/test_gpu_tail.py, tests/test_gpu_handover.py, tests/test_gpu_loss_stage.py).
Reference semantics: model/OneModel.lua:223-275, optimizer/MyOptimizer.lua:177-221."""
import numpy as np
import pytest

from kprn_amd import _ffi, synth
from oracle.oracle import make_opt
from tests.test_gpu_ragged import check as ragged_check, data as ragged_data, mk as ragged_mk
from tests.test_gpu_small_tiles import SHAPE, mk, rel_inf

pytestmark = pytest.mark.gpu
VE = SHAPE["Ve"]
MAX_PATHS = 8192                        # fused::small_tiles: the mode's last size
MOVED = {2: 0, 3: 1, 6: 3, 16: 8}       # ho_decide's d at a difference of one tile (2 T - 1 half steps), by hand: module docstring
TILES = {"1": lambda c: 1, "2": lambda c: 2, "cus/2": lambda c: c // 2, "cus/2+1": lambda c: c // 2 + 1, "cus": lambda c: c, "cus+1": lambda c: c + 1,
         "3cus/2": lambda c: c + c // 2, "2cus-1": lambda c: 2 * c - 1, "2cus": lambda c: 2 * c}
GENERIC = ("lstm_layer_", "lstm_step_", "lstm_gates_")   # profile families of the generic fp32 pipeline's tiers (generic_pipeline.hip cell_of)


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def n_paths(cus, tiles, r):
    """N = 16 t - r; a case that does not fit the mode on this part is dropped, not clipped"""
    N = 16 * TILES[tiles](cus) - r
    if N > MAX_PATHS:
        pytest.skip(f"{tiles} tiles of 16 rows exceed {MAX_PATHS} paths at {cus} compute units")
    return N


def piped(t, cus):
    return 2 <= t and 2 * t <= cus


def moving_pairs(t, cus, T):
    h = t - cus
    return min(h, cus - h) if h > 0 and MOVED[T] > 0 else 0


def paths(N, T, seed, padded):
    """N pairs of one path (N is exact); padded: the 73 % left-padded mix (T > 4: pads run as ordinary steps here), else every path T real steps"""
    return synth.make_paths(N, 1, T, Ve=VE, seed=seed, real_len=None if padded else T)


def assert_regime(b, fam, cus, T, backwards=1, pipe_on=True, mode=2):
    """fused route; one BPTT launch per backward exactly when piped; the hand-over moves what the rule says"""
    t = (b.n_paths + 15) // 16
    assert "lstm_fused_bwd" in fam and any(k.startswith("lstm_fused_fwd") for k in fam), sorted(fam)
    assert not any(k.startswith(GENERIC) for k in fam), sorted(fam)
    assert fam["lstm_fused_bwd"][1] == backwards * (1 if pipe_on and piped(t, cus) else 2), (t, fam["lstm_fused_bwd"])
    st = b.handover_stats
    want, d, tile = (moving_pairs(t, cus, T) if mode else 0), MOVED[T], 2 * T - 1
    assert st[0] == want and st[1] == want * d, (t, T, st)
    assert st[2] == (2 * tile if t > cus else tile), st      # the longest workgroup, in half steps
    if want > 0 and t - cus <= cus // 2:                     # every two-tile workgroup has a one-tile partner: all of them get shorter
        assert st[0] > 0 and st[3] == max(2 * tile - 2 * d, tile + 2 * d) < st[2], st
    else:
        assert st[3] == st[2], st
    return st


def assert_grads(eng, g, og, bar=2e-4, tag=None):
    for nm, (off, shp) in eng.layout().items():
        n = int(np.prod(shp))
        e = rel_inf(g[off:off + n], og[off:off + n])
        print(f"  {tag} gradient {nm}: {e:.3e}")
        assert e < bar, (tag, nm, e)


def untouched_rows(idx):
    rows = np.setdiff1d(np.arange(VE), np.unique(idx[..., -2]) - 1)   # (ids are 1-based; the entity column is F - 2)
    assert rows.size > 0
    return rows


def entity_grad(eng, g):
    off, shp = eng.layout()["entity_emb"]
    return g[off:off + int(np.prod(shp))].reshape(shp)


def oracle_of(o64, theta, idx, labels):
    ps, pooled, probs = o64.forward(theta, idx)
    ol, og, _ = o64.forward_backward(theta, idx, labels)
    return ps, pooled, probs, ol, og


def forward_backward(eng, b):
    out = eng.forward(b, 1, want=("probs", "all_probs", "pooled", "path_scores"))
    loss = eng.backward(b, 1)
    return out, loss, eng.get_flat_grads()


def assert_oracle(eng, out, loss, g, ref, idx, tag):
    ps, pooled, probs, ol, og = ref
    e = rel_inf(out["path_scores"], ps)
    print(f"  {tag} path scores: {e:.3e}   loss {loss!r} oracle {ol!r}")
    assert out["path_scores"].shape == ps.shape and e < 3e-6, (tag, e)
    np.testing.assert_allclose(out["pooled"], pooled, rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(out["probs"], probs[:, 0], rtol=1e-5)
    np.testing.assert_allclose(out["all_probs"], probs, rtol=1e-4)     # (every class: the bar of tests/test_gpu_ragged.py check)
    assert abs(loss - ol) < 1e-5 * max(1.0, abs(ol)), (tag, loss, ol)
    assert_grads(eng, g, og, tag=tag)
    assert np.all(entity_grad(eng, g)[untouched_rows(idx)] == 0), tag   # exactly: nothing but the batch's own rows is ever added to


# ---- 1. every regime x T against the float64 oracle ------------------------------------------------------------------------------------------------------
# (tiles, r, T, padded).  synth.make_paths draws real lengths from {min(4, T), T}: only at T > 4 does the mix hold pads, so the flag is dealt among those
# twelve cases -- seven padded, five of T real steps; one tile, piped, two launches and hand-over each have both kinds -- and is off where it would change nothing.
REGIMES = [("1", 15, 2, False), ("1", 15, 16, True), ("1", 1, 2, False), ("1", 1, 16, False), ("1", 0, 2, False), ("1", 0, 16, True),   # N = 1, 15, 16
           ("2", 15, 2, False), ("2", 15, 3, False), ("2", 15, 16, False),                             # smallest pipe: N = 17
           ("cus/2", 3, 2, False), ("cus/2", 3, 16, True),                                             # last pipe, ragged
           ("cus/2+1", 15, 2, False), ("cus/2+1", 15, 6, False), ("cus/2+1", 15, 16, True),            # first two-launch, one row in the last tile
           ("cus", 0, 2, False), ("cus", 0, 16, False),                                                # full grid, no hand-over
           ("cus+1", 15, 2, False), ("cus+1", 15, 3, False), ("cus+1", 15, 16, True),                  # one pair moves; workgroup 0's second tile has one row
           ("3cus/2", 5, 2, False), ("3cus/2", 5, 3, False), ("3cus/2", 5, 6, True), ("3cus/2", 5, 16, False),   # every pair moves
           ("2cus-1", 0, 16, True),                                                                    # one light workgroup
           ("2cus", 0, 2, False)]                                                                      # the mode's last size: nothing moves


@pytest.mark.parametrize("tiles,r,T,padded", REGIMES)
def test_every_regime_and_T_against_the_f64_oracle(cus, tiles, r, T, padded):
    """Scores of all 46 classes of every path, pooled values, probabilities, loss and every gradient; then the same batch a SECOND time on the same engine (the
    epochs of pipe_flag and of the hand-over flags move on: a stale flag taken for current shows in the second pass's gradients): scores bit for bit, the loss
    equal, the gradients at the oracle's bars again.  Entity rows the batch does not name keep an exactly zero gradient (the padding rows of a ragged tile).
    T = 2: the hand-over rule moves nothing (module docstring: 3 half steps < 4), asserted as such; 2 cus tiles: nothing can move.
    T = 16 is 32 layer-steps deep against 12 at T = 6 and holds the T = 6 bars as they are: measured on MI355X over all cases, scores at most 1.1e-6 of
    scale (bar 3e-6), gradient tensors at most 2.1e-5 (bar 2e-4)."""
    N = n_paths(cus, tiles, r)
    t = TILES[tiles](cus)
    eng, o64, theta = mk()
    idx, labels = paths(N, T, seed=100 * T + 7 * r + len(tiles) + t % 13, padded=padded)
    ref = oracle_of(o64, theta, idx, labels)
    b = eng.batch(idx, labels)
    assert b.n_paths == N and b.executed_steps == N * T       # 16-row tiles: no identical-prefix plan, pads run as ordinary steps
    eng.profile(True)
    first = None
    for rep in range(2):
        eng.profile_reset()
        out, loss, g = forward_backward(eng, b)
        st = assert_regime(b, eng.profile_get(), cus, T)
        if tiles == "3cus/2":
            assert st[0] == (cus // 2 if T >= 3 else 0), st
        if tiles == "2cus":
            assert N == MAX_PATHS and st[0] == 0 and st[2] == st[3], st
        assert_oracle(eng, out, loss, g, ref, idx, f"{tiles} r={r} T={T} pass {rep}")
        if first is None:
            first = (out["path_scores"].copy(), loss)
    assert np.array_equal(first[0], out["path_scores"]) and first[1] == loss
    eng.close()


def test_one_step_paths_leave_the_fused_route_and_match_the_oracle(cus):
    """T = 1 at N = 17: fwd_supported wants T >= 2, so the batch runs on the generic pipeline -- the route boundary right below the smallest piped batch"""
    eng, o64, theta = mk()
    idx, labels = paths(17, 1, seed=91, padded=False)
    ref = oracle_of(o64, theta, idx, labels)
    b = eng.batch(idx, labels)
    eng.profile(True)
    out, loss, g = forward_backward(eng, b)
    fam = eng.profile_get()
    assert not any(k.startswith("lstm_fused") for k in fam) and any(k.startswith(GENERIC) for k in fam), sorted(fam)
    assert b.handover_stats[0] == 0
    assert_oracle(eng, out, loss, g, ref, idx, "T=1")
    eng.close()


# ---- 2. on against off, same process, same batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labelled", ["ones", "drawn_deterministic"])
@pytest.mark.parametrize("T", [2, 16])
@pytest.mark.parametrize("tiles,r", [("2", 15), ("cus/2", 3), ("cus/2+1", 15)])
def test_bwd_pipe_on_equals_off_at_the_regimes_edges(cus, tiles, r, T, labelled):
    """tests/test_gpu_tail.py::test_both_layers_bptt_in_one_launch_equals_one_launch_per_layer at two tiles (the smallest grid that pipes), at the last piped tile
    count with a ragged last tile, and one tile above it (not piped either way: both sides record two launches); T = 2 (the bottom layer's first flag wait is
    the launch's first action) and T = 16 (the last column of pipe_flag[tile][MAXT_LDS]).  Three backwards each: the flags' epoch moves on.
    The bar is 2e-6 of a tensor's LARGEST entry, and in the default mode the two sides differ, pipe or no pipe, by the order in which a launch's workgroups
    add their head-gradient partials atomically.  With labels drawn 50 / 50 and untrained parameters dS is +-0.5 / B, the one live row of out.weight cancels
    to ~N^-1/2 of its addends, and that order alone then costs as much as the bar: measured on MI355X with drawn labels, out.weight 2.2e-6 (cus / 2 tiles,
    T = 16) and 2.7e-6 (cus / 2 + 1 tiles, T = 2, where NEITHER side pipes: two runs of the same launches), every other tensor below 1.5e-6, and the same cases
    inside the bar on another run.  So the comparison is made twice at the same bar:
      "ones": the default kernels (k_lstm_bwd_dual) with every pair labelled 1 -- one sign of dS leaves nothing to cancel (measured: every tensor at most
              7.7e-7); what the pipe could get wrong (a step index, a stale flag, a padding row) moves the bottom layer's gradients whatever the labels;
      "drawn_deterministic": the drawn labels under option "deterministic" = 1 (k_lstm_bwd_dual_det against two k_lstm_bwd_det launches), where no sum's
              order is left to the hardware (measured: every tensor bit for bit)."""
    N = n_paths(cus, tiles, r)
    idx, labels = paths(N, T, seed=33 + T + r, padded=(T == 16))
    if labelled == "ones":
        labels = np.ones_like(labels)
    res = []
    for pipe in ("1", "0"):
        eng, _, _ = mk(seed=5)
        eng.set_option("bwd_pipe", pipe)
        if labelled == "drawn_deterministic":
            eng.set_option("deterministic", "1")
        b = eng.batch(idx, labels)
        eng.forward(b, 1, want=("probs",))
        eng.profile(True)
        losses = [eng.backward(b, 1) for _ in range(3)]
        assert_regime(b, eng.profile_get(), cus, T, backwards=3, pipe_on=(pipe == "1"))
        res.append((eng.get_flat_grads().astype(np.float64), eng.layout(), losses))
        eng.close()
    (g1, lay, l1), (g0, _, l0) = res
    print(f"  {tiles} T={T} {labelled}: losses on {l1} off {l0}")
    assert l1 == l0
    for nm, (off, shp) in lay.items():
        n = int(np.prod(shp))
        a, c = g1[off:off + n], g0[off:off + n]
        e = float(np.max(np.abs(a - c))) / max(1e-30, float(np.max(np.abs(c))))
        print(f"  {tiles} T={T} {labelled} pipe on - off, {nm}: {e:.3e}")
        assert e <= 2e-6, (nm, e)


@pytest.mark.parametrize("T", [3, 6, 16])
@pytest.mark.parametrize("tiles,r", [("cus+1", 15), ("3cus/2", 5), ("2cus-1", 0)])
def test_hand_over_on_16_row_tiles_equals_off(cus, tiles, r, T):
    """tests/test_gpu_handover.py::test_hand_over_on_equals_off on the 16-row tiles: one pair (the heavy workgroup's second tile has one row), every pair, one
    light workgroup; both pairings.  The forward takes no part: scores, probabilities and loss bit for bit; a row's dx is the same arithmetic whichever
    workgroup runs it, the weight gradients are other partial sums: 1e-5 of each tensor.  Twice per engine (the slots' epochs move on)."""
    N = n_paths(cus, tiles, r)
    t = TILES[tiles](cus)
    idx, labels = paths(N, T, seed=50 + T + r, padded=(T != 6))
    res = {}
    for mode in (2, 1, 0):
        eng, _, _ = mk()
        eng.set_option("small_tiles", "1")
        eng.set_option("tile_handover", str(mode))
        b = eng.batch(idx, labels)
        eng.profile(True)
        runs = []
        for rep in range(2):
            eng.profile_reset()
            out, loss, g = forward_backward(eng, b)
            st = assert_regime(b, eng.profile_get(), cus, T, mode=mode)
            runs.append((out["path_scores"].copy(), out["probs"].copy(), loss, g.astype(np.float64)))
        if mode:
            assert st[0] == {"cus+1": 1, "3cus/2": cus // 2, "2cus-1": 1}[tiles], (mode, st)   # either pairing reaches every heavy workgroup of "3cus/2"
        assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][2] == runs[1][2]
        res[mode] = runs[1] + (eng.layout(),)
        eng.close()
    assert t == (N + 15) // 16
    for mode in (2, 1):
        assert np.array_equal(res[mode][0], res[0][0])
        assert np.array_equal(res[mode][1], res[0][1])
        assert res[mode][2] == res[0][2]
        for nm, (off, shp) in res[mode][4].items():
            n = int(np.prod(shp))
            e = rel_inf(res[mode][3][off:off + n], res[0][3][off:off + n])
            print(f"  {tiles} T={T} hand-over {mode} - off, {nm}: {e:.3e}")
            assert e <= 1e-5, (mode, nm, e)


@pytest.mark.parametrize("T", [2, 16])
@pytest.mark.parametrize("tiles,r", [("2", 15), ("cus/2", 3)])
def test_deterministic_pipe_is_bit_reproducible_and_matches_the_oracle(cus, tiles, r, T):
    """option "deterministic" = 1 in the piped regime (k_lstm_bwd_dual_det): two fresh engines leave bit-identical gradients, at the oracle's bars"""
    N = n_paths(cus, tiles, r)
    idx, labels = paths(N, T, seed=70 + T + r, padded=(T == 16))
    got = []
    for k in range(2):
        eng, o64, theta = mk()
        eng.set_option("deterministic", "1")
        b = eng.batch(idx, labels)
        eng.profile(True)
        out, loss, g = forward_backward(eng, b)
        fam = eng.profile_get()
        assert_regime(b, fam, cus, T)
        assert "det_join" in fam, sorted(fam)
        if k == 0:
            assert_oracle(eng, out, loss, g, oracle_of(o64, theta, idx, labels), idx, f"det {tiles} T={T}")
        got.append((g, loss, out["path_scores"]))
        eng.close()
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1] and np.array_equal(got[0][2], got[1][2])


# ---- 3. one handle walks the regimes ---------------------------------------------------------------------------------------------------------------------
def walk(c):
    """(regime, pairs, P, T, padded) of consecutive Adam steps: every boundary between one tile, piped, two launches, hand-over and the 64-path tiles with their
    plan is crossed in both directions, with T changing (save_frag regrows on cap_N at step 3 and 6, on cap_T at step 4)"""
    h = c // 2
    return [("one", 5, 3, 6, True),                         # 15 paths
            ("pipe", 4 * h, 3, 3, False),                   # 3 h / 4 tiles
            ("handover", 16 * (c + h) - 5, 1, 6, True),     # every pair moves
            ("pipe", 8 * h - 1, 2, 16, True),               # h tiles, the last one ragged: the last piped size, a larger T
            ("two", 8 * h + 1, 2, 6, False),                # h + 1 tiles
            ("big", 2100, 4, 6, True),                      # 8 400 paths: 64-path tiles with their plan
            ("pipe", 17, 1, 2, False),                      # two tiles, T = 2
            ("handover", 16 * (c + 1) - 15, 1, 16, True),   # one pair moves 8 steps
            ("one", 16, 1, 2, False),
            ("handover", 8 * (2 * c - 1), 2, 3, False),     # one light workgroup
            ("pipe", 8, 3, 16, True),                       # two tiles, T = 16
            ("big", 8193, 1, 16, True),                     # one path above the mode, T = 16
            ("one", 1, 1, 16, False),
            ("two", 4 * c, 4, 16, True),                    # every workgroup one tile
            ("handover", 16 * (c + h) - 5, 1, 16, False),
            ("pipe", 8 * h, 2, 6, True),                    # the last piped size, whole tiles
            ("two", 8 * h + 1, 2, 2, False),
            ("handover", 16 * (c + 1) - 15, 1, 6, True),
            ("one", 3, 5, 3, False),
            ("pipe", 128, 3, 6, True)]                      # the reference's minibatch


def test_one_handle_walks_every_regime(cus):
    """tests/test_gpu_small_tiles.py::test_twenty_adam_steps_of_reference_minibatches with the batch size and T changing every step: pipe_flag and the hand-over
    flags are zeroed once and told apart by epoch only, save_frag regrows on cap_N / cap_T -- one handle goes from a piped batch to a hand-over batch to 64-path
    tiles and back.  Loss of every step within 1e-5 of the oracle's, final parameters within 5e-6, then a 512-pair scoring batch at T = 3."""
    eng, o64, th = mk(seed=8)
    opt, oopt, st = _ffi.make_opt(method=1, lr=1e-3), make_opt(method=1, lr=1e-3), o64.new_state()
    eng.profile(True)
    steps = [s for s in walk(cus) if s[0] == "big" or s[1] * s[2] <= MAX_PATHS]
    assert len(steps) <= 20 and (32 * cus > MAX_PATHS or len(steps) == 20)
    for k, (regime, pairs, P, T, padded) in enumerate(steps):
        N, t = pairs * P, (pairs * P + 15) // 16
        idx, labels = synth.make_paths(pairs, P, T, Ve=VE, seed=700 + k, real_len=None if padded else T)
        # what this step's batch does on this chip, from a batch of its own (train_step_host builds and frees its own)
        probe = eng.batch(idx, labels)
        hs, executed = probe.handover_stats, probe.executed_steps
        probe.free()
        if regime == "big":
            assert N > MAX_PATHS and executed < N * T, (k, executed)       # a plan: the 64-path tiles
        else:
            assert executed == N * T
            assert {"one": t == 1, "pipe": piped(t, cus), "two": cus // 2 < t <= cus, "handover": cus < t}[regime], (k, t)
            assert hs[0] == moving_pairs(t, cus, T) and (hs[0] > 0) == (regime == "handover"), (k, hs)
        ol, _ = o64.train_step(th, st, oopt, idx, labels)
        eng.profile_reset()
        gl = eng.train_step_host(idx, labels, opt)
        fam = eng.profile_get()
        assert "lstm_fused_bwd" in fam and "lstm_fused_fwd_train" in fam and not any(f.startswith(GENERIC) for f in fam), (k, sorted(fam))
        assert fam["lstm_fused_bwd"][1] == (1 if regime == "pipe" else 2), (k, regime, fam["lstm_fused_bwd"])
        assert ("prefix_bwd" in fam) == (regime == "big"), (k, sorted(fam))
        print(f"  step {k} {regime} N={N} T={T}: loss {gl!r} oracle {ol!r}")
        assert abs(gl - ol) < 1e-5 * max(1.0, abs(ol)), (k, regime, gl, ol)
    d = float(np.max(np.abs(eng.get_flat_params() - th)))
    print(f"  max |theta - oracle| after {len(steps)} steps: {d:.3e}")
    assert d < 5e-6, d
    idx, _ = synth.make_paths(512, 1, 3, Ve=VE, seed=750)
    probs, _ = eng.forward_host(idx, 1)
    np.testing.assert_allclose(probs, o64.forward(th, idx)[2][:, 0], rtol=1e-5)
    eng.close()


@pytest.mark.parametrize("regime,pairs", [("pipe", 600), ("handover", 3000)])
def test_ragged_batches_in_the_piped_and_the_hand_over_regime(cus, regime, pairs):
    """pairs of 1 .. 28 paths in one batch (tests/test_gpu_ragged.py check: per count group against the oracle) where the BPTT is piped and where tiles change
    hands; T = 6, the only T data() makes"""
    counts = synth.draw_num_paths(np.random.default_rng(9), pairs)
    counts[:2] = (1, 28)
    if counts.sum() % 16 == 0:
        counts[2] += 1
    t = (int(counts.sum()) + 15) // 16
    if not (piped(t, cus) if regime == "pipe" else cus < t <= 2 * cus):
        pytest.skip(f"{t} tiles are not in the {regime} regime at {cus} compute units")
    assert 1 in counts and 28 in counts
    eng, o64, theta = ragged_mk(L=2)
    idx, labels = ragged_data(counts, seed=27)
    b = eng.batch_ragged(idx, counts, labels)
    assert b.executed_steps == b.n_paths * 6
    eng.profile(True)
    ragged_check(eng, o64, theta, idx, counts, labels, batch=b)
    st = assert_regime(b, eng.profile_get(), cus, 6)
    assert (st[0] > 0) == (regime == "handover"), st
    eng.close()


# ---- 4. a scoring pass riding in the training forward, shapes that differ ---------------------------------------------------------------------------------
# (scoring tiles, r, T) against (training tiles, r, T)
@pytest.mark.parametrize("score,train", [(("1", 11, 3), ("cus/2", 3, 6)), (("cus/2+1", 15, 16), ("2", 2, 2))])
def test_a_scoring_pass_of_another_shape_rides_in_the_training_forward(cus, score, train):
    """tests/test_gpu_loss_stage.py::test_a_scoring_pass_rides_in_a_training_step with the two branches of k_lstm_fwd_dual at different T and grid sizes: five
    paths at T = 3 beside cus / 2 tiles at T = 6, and cus / 2 + 1 tiles at T = 16 beside two tiles at T = 2.  The ridden pass's probabilities are the bytes of
    eng.forward of the same batch before the step."""
    eng, o64, theta = mk()
    o64.zero_pad(theta)   # a training step zeroes the pad rows first (MyOptimizer.lua:181): scoring pass and step then see the same parameters
    eng.set_flat_params(theta.astype(np.float32))
    for key, value in (("score_overlap", "1"), ("score_dual", "2")):
        eng.set_option(key, value)
    si, _ = paths(n_paths(cus, *score[:2]), score[2], seed=81, padded=True)
    ti, tl = paths(n_paths(cus, *train[:2]), train[2], seed=82, padded=True)
    sb, tb = eng.batch(si), eng.batch(ti, tl)
    # a parameter change between forward_async and the training forward places the queued pass ahead of it, the usual way: a new engine's first step zeroes
    # the pad rows (hence one step first), and the lazy entity update brings the training batch's rows up to date (hence the dense update)
    opt = _ffi.make_opt(method=1, lr=1e-3, entity_update=1)
    eng.train_step(tb, opt)
    for step in range(2):
        want = eng.forward(sb, 1)["probs"]
        if step == 0:
            np.testing.assert_allclose(want, o64.forward(eng.get_flat_params().astype(np.float64), si)[2][:, 0], rtol=1e-5)
        eng.profile(True)
        eng.profile_reset()
        eng.forward_async(sb, 1)
        loss = eng.train_step(tb, opt)
        got = eng.read_probs(sb.B)
        prof = eng.profile_get()
        eng.profile(False)
        assert np.isfinite(loss)
        assert "lstm_fused_fwd_dual" in prof and "lstm_fused_fwd" not in prof and "lstm_fused_fwd_train" not in prof, sorted(prof)
        assert prof["lstm_fused_bwd"][1] == (1 if piped(TILES[train[0]](cus), cus) else 2), prof["lstm_fused_bwd"]
        print(f"  step {step}: max |riding - forward| = {float(np.max(np.abs(got - want))):.3e}")
        assert got.tobytes() == want.tobytes()
    eng.close()
