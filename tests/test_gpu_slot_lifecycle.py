"""-m gpu: the lifecycle of a feed slot (kprn_amd/csrc/batch_slots.hip) -- the states slots::detach exists for.  A slot is refilled, re-reserved or
freed while the handle still refers to it: as the optimiser's row list (gradients waiting for their update), as the batch of a deferred scoring part, as the
batch of a scoring pass queued on the side stream.  Whatever the handle referred to must come out as if the slot had been a resident batch
(kprn_batch_create) that nobody touched: every comparison is np.array_equal, the trained parameters under option "deterministic" = "1"."""
import ctypes as C
import functools

import numpy as np
import pytest

from kprn_amd import _ffi, synth

pytestmark = pytest.mark.gpu

SHAPE = (6, 5000, 9, 16, 32, 16, 64, 2)   # the engine of tests/test_gpu_feed.py
T, F = 6, 3
SEED = 7
BUILDS = ["host", "device"]
WANT = ("probs", "path_scores")


def _opt():
    return _ffi.make_opt(method=1, lr=1e-2)


@functools.lru_cache(maxsize=None)
def _data(name):
    """rectangular: (idx [B,P,T,F], labels [B]); ragged: (idx [N,T,F], counts [B], labels [B])"""
    if name == "ragged":   # 120 pairs of 1..5 paths, 360 paths: synth.make_paths' paths, cut into pairs of unequal length
        idx, labels = synth.make_paths(360, 1, T, Ve=5000, seed=43)
        counts = np.tile(np.arange(1, 6, dtype=np.int32), 24)
        return idx.reshape(360, T, F), counts, labels[:120].copy()
    pairs, P, seed = {"rect": (200, 3, 41),     # 600 paths
                      "second": (150, 5, 45),   # 750 paths
                      "third": (90, 2, 47),
                      "big": (300, 14, 49)}[name]   # 4 200 paths: 66 tiles of 64 (a split pass needs 64), seven times "rect" (the block must grow)
    return synth.make_paths(pairs, P, T, Ve=5000, seed=seed)


def _engine(build="host", **options):
    eng = _ffi.Engine(*SHAPE, seed=SEED)
    eng.set_option("feed_build", build)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


def _resident(eng, name):
    d = _data(name)
    return eng.batch_ragged(*d) if name == "ragged" else eng.batch(*d)


@functools.lru_cache(maxsize=None)
def _ref_scores(name, small_tiles="1"):
    """probs and path_scores of the untrained engine on a RESIDENT batch of the data (computed once, never written to)"""
    eng = _engine(small_tiles=small_tiles)
    out = eng.forward(_resident(eng, name), 1, want=WANT)
    eng.close()
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_trained(name, one_call):
    """flat parameters after one deterministic step on a RESIDENT batch: kprn_train_step_batch (one_call) or kprn_backward_batch + kprn_apply_update"""
    eng = _engine(deterministic="1")
    b = _resident(eng, name)
    if one_call:
        eng.train_step(b, _opt(), want_loss=False)
    else:
        eng.backward(b, 1, want_loss=False)
        eng.apply_update(_opt())
    theta = eng.get_flat_params()
    eng.close()
    theta.setflags(write=False)
    return theta


def _same(got, want, what):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    print(f"{what}: max |difference| {d.max():.3e}, {int((d != 0).sum())} of {d.size} differ")
    assert np.array_equal(got, want), what


def _reserve_again(eng, slot, max_pairs, max_paths):
    """kprn_batch_slot_reserve on a slot that exists (Batch.reserve makes a new one)"""
    eng._ck(eng.L.kprn_batch_slot_reserve(eng.h, C.byref(slot.ptr), int(max_pairs), C.c_int64(int(max_paths)), T, F, 1))


@pytest.mark.parametrize("build", BUILDS)
def test_reserved_slot_takes_a_rectangular_then_a_ragged_fill(build):
    eng = _engine(build)
    slot = _ffi.Batch.reserve(eng, 200, 600, T, F)
    slot.refill(*_data("rect"))
    got = eng.forward(slot, 1, want=WANT)
    for k in WANT:
        _same(got[k], _ref_scores("rect")[k], f"rectangular fill, {k}")
    slot.refill_ragged(*_data("ragged"))
    got = eng.forward(slot, 1, want=WANT)
    for k in WANT:
        _same(got[k], _ref_scores("ragged")[k], f"ragged fill, {k}")
    eng.close()


@pytest.mark.parametrize("how", ["reserve", "refill"])
@pytest.mark.parametrize("build", BUILDS)
def test_slot_given_up_while_its_gradients_wait_for_the_update(build, how):
    """backward(slot) leaves the optimiser's row list as a view of the slot's distinct rows; a larger reserve (or a larger refill) frees that block before
    the update walks the list"""
    eng = _engine(build, deterministic="1")
    slot = eng.feed(*_data("rect"))
    eng.backward(slot, 1, want_loss=False)
    if how == "reserve":
        _reserve_again(eng, slot, 200, 4 * 600)
    else:
        slot.refill(*_data("big"))
    eng.apply_update(_opt())
    _same(eng.get_flat_params(), _ref_trained("rect", False), f"parameters after {how}")
    eng.close()


@pytest.mark.parametrize("how", ["refill", "free"])
@pytest.mark.parametrize("build", BUILDS)
def test_deferred_scoring_part_reads_the_contents_it_was_queued_for(build, how):
    """score_split: the second half of the pass's tiles is still to be launched when the slot is refilled / freed"""
    eng = _engine(build, small_tiles="0", score_overlap="1", score_split="0.5")   # (64-path tiles: a split needs 64 of them)
    slot = eng.feed(*_data("big"))
    eng.forward_async(slot, 1)
    if how == "refill":
        slot.refill(*_data("rect"))
    else:
        slot.free()
    eng.forward_async_rest()
    _same(eng.read_probs(300), _ref_scores("big", "0")["probs"], f"the old contents' probs after {how}")
    if how == "free":   # the engine stays usable
        _same(eng.forward(_resident(eng, "rect"), 1)["probs"], _ref_scores("rect", "0")["probs"], "another batch after free")
    eng.close()


@pytest.mark.parametrize("build", BUILDS)
def test_refill_grows_the_block_under_a_queued_scoring_pass(build):
    eng = _engine(build, deterministic="1", score_overlap="1")
    slot = eng.feed(*_data("rect"))
    eng.forward_async(slot, 1)
    slot.refill(*_data("big"))   # (no reserve before it: seven times the paths, the old block is freed)
    _same(eng.read_probs(200), _ref_scores("rect")["probs"], "the first pass's probs")
    eng.train_step(slot, _opt(), want_loss=False)
    _same(eng.get_flat_params(), _ref_trained("big", True), "parameters after a step on the refilled slot")
    eng.close()


@functools.lru_cache(maxsize=None)
def _ref_host_entry_points():
    eng = _engine(deterministic="1")
    for name in ("rect", "second"):
        eng.train_step(_resident(eng, name), _opt())
    probs = eng.forward(eng.batch(_data("third")[0]), 1)["probs"]
    theta = eng.get_flat_params()
    eng.close()
    probs.setflags(write=False)
    theta.setflags(write=False)
    return theta, probs


@pytest.mark.parametrize("inline_upload", ["side", "main"])
@pytest.mark.parametrize("build", BUILDS)
def test_host_buffer_entry_points_train_and_score_like_resident_batches(build, inline_upload):
    eng = _engine(build, deterministic="1", inline_upload=inline_upload)
    for name in ("rect", "second"):
        eng.train_step_host(*_data(name), _opt())
    probs, _ = eng.forward_host(_data("third")[0], 1, want_all=False)
    theta, want = _ref_host_entry_points()
    _same(probs, want, "kprn_forward probs")
    _same(eng.get_flat_params(), theta, "parameters after two kprn_train_step calls")
    eng.close()
