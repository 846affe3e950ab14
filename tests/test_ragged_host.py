"""not gpu: the host side of ragged batches (pairs with different path counts in one batch; an extension, the reference has none).

* the library builds for gfx950 and exports the ragged entry points;
* kprn_host_ragged_plan (offsets, loss-stage workgroup table, reducer form) against a numpy restatement, and its refusals;
* BatcherFileList.getMergedGroup: the merged groups, concatenated, are the unmerged batches, concatenated -- pair for pair;
* synth.make_ragged, and dp.shard_pairs refusing ragged input."""
import os
import subprocess

import numpy as np
import pytest

from kprn_amd import _ffi, batcher, build as kbuild, formats, scoring, synth

RAGGED_SYMBOLS = ["kprn_batch_create_ragged", "kprn_batch_feed_ragged_async", "kprn_forward_ragged", "kprn_host_ragged_plan", "kprn_batch_num_paths"]

# the limits the header states (include/kprn.h, 'ragged batches')
MAX_SEG, THREAD_MAX, WG_PATHS, WG_PAIRS = 4096, 28, 448, 16


@pytest.fixture(scope="module")
def so():
    return kbuild.build()


def test_library_exports_the_ragged_entry_points(so):
    syms = subprocess.check_output(["nm", "-D", so]).decode()
    declared = _ffi.declared_symbols()
    for s in RAGGED_SYMBOLS:
        assert s in declared, f"include/kprn.h does not declare {s}"
        assert f" T {s}" in syms, f"libkprn.so does not export {s}"
    assert b"amdgcn-amd-amdhsa--gfx950" in open(so, "rb").read()


def np_plan(counts):
    """the cut restated: consecutive pairs; a workgroup is closed when it holds WG_PAIRS pairs or the next pair would take it past WG_PATHS"""
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    wg, pairs, paths = [], 0, 0
    for b, c in enumerate(counts):
        if pairs == 0 or pairs == WG_PAIRS or paths + c > WG_PATHS:
            wg.append(b)
            pairs, paths = 0, 0
        pairs += 1
        paths += int(c)
    wg.append(len(counts))
    return off, np.asarray(wg), int(counts.max())


COUNT_VECTORS = {
    "ones": np.ones(37, np.int32),
    "one_pair": np.array([5], np.int32),
    "one_long_pair": np.array([MAX_SEG], np.int32),
    "equal_28": np.full(50, 28, np.int32),
    "equal_3": np.full(33, 3, np.int32),
    "drawn": synth.draw_num_paths(np.random.default_rng(3), 1000),
    "edges": np.array([1, 28, 29, 63, 64, 65, 257, MAX_SEG, 1, 1, 447, 1, 448, 449, 2], np.int32),
    "mixed": np.random.default_rng(5).integers(1, 200, size=300).astype(np.int32),
}


@pytest.mark.parametrize("name", sorted(COUNT_VECTORS))
def test_ragged_plan_matches_the_numpy_restatement(so, name):
    counts = COUNT_VECTORS[name]
    B = len(counts)
    p = _ffi.host_ragged_plan(counts)
    off, wg, mx = np_plan(counts)
    assert (p["max_seg"], p["thread_max"], p["wg_paths"], p["wg_pairs"]) == (MAX_SEG, THREAD_MAX, WG_PATHS, WG_PAIRS)
    assert np.array_equal(p["offsets"], off)
    assert p["n_wg"] == len(wg) - 1 and np.array_equal(p["wg_first"], wg)
    assert p["max_count"] == mx and p["wave"] == int(mx > THREAD_MAX)
    # every pair in exactly one workgroup, in order; the bounds hold
    w = p["wg_first"]
    assert w[0] == 0 and w[-1] == B and (np.diff(w) >= 1).all()
    for i in range(p["n_wg"]):
        seg = counts[w[i]:w[i + 1]]
        assert len(seg) <= WG_PAIRS
        assert seg.sum() <= WG_PATHS or len(seg) == 1
    if (counts == counts[0]).all() and counts[0] <= THREAD_MAX:   # the rectangular loss stage's cut: 16 pairs per workgroup
        assert np.array_equal(w[:-1], np.arange(0, B, WG_PAIRS))


def test_ragged_plan_refuses_bad_counts(so):
    ok = np.array([2, 3, 1], np.int32)
    assert _ffi.host_ragged_plan(ok, 6)["n_wg"] == 1
    for counts, N in [(np.array([2, 0, 1], np.int32), 3), (np.array([2, -1, 4], np.int32), 5), (ok, 7), (ok, 5),
                      (np.array([1, MAX_SEG + 1], np.int32), MAX_SEG + 2)]:
        with pytest.raises(_ffi.KprnError) as ei:
            _ffi.host_ragged_plan(counts, N)
        assert ei.value.code == _ffi.E_ARG


def test_make_ragged_is_seeded_and_well_formed():
    idx, counts, labels = synth.make_ragged(200, 6, Ve=300, seed=9)
    idx2, counts2, labels2 = synth.make_ragged(200, 6, Ve=300, seed=9)
    assert np.array_equal(idx, idx2) and np.array_equal(counts, counts2) and np.array_equal(labels, labels2)
    assert idx.shape == (int(counts.sum()), 6, 3) and idx.dtype == np.int32 and labels.shape == (200,)
    assert counts.min() >= 1 and counts.max() <= 28 and len(np.unique(counts)) > 3
    assert idx.min() >= 1 and idx[..., 1].max() <= 300
    given = np.array([1, 40, 2], np.int32)
    idx3, c3, _ = synth.make_ragged(3, 4, Ve=300, seed=1, counts=given)
    assert np.array_equal(c3, given) and idx3.shape == (43, 4, 3)
    # the paths of one pair share the pair's user and item (first real step / last step), as make_paths builds them
    off = np.concatenate([[0], np.cumsum(given)])
    for b in range(3):
        assert len(np.unique(idx3[off[b]:off[b + 1], -1, 1])) == 1


def _write_buckets(root, n_paths=6000, T=6):
    buckets = synth.make_bucketed(n_paths, T, Ve=300, seed=21)
    names = []
    for P in sorted(buckets):
        idx, labels = buckets[P]
        nm = "test_%d.npz" % P
        formats.save_path_file(os.path.join(root, nm), labels, idx, 1)
        names.append(nm)
    with open(os.path.join(root, "test.list"), "w") as f:
        f.write("\n".join(names) + "\n")
    return buckets


@pytest.mark.parametrize("max_paths", [64, 1000, scoring.ENGINE_BATCH_PATHS])
def test_merged_groups_are_the_unmerged_batches_pair_for_pair(tmp_path, max_paths):
    root = str(tmp_path)
    buckets = _write_buckets(root)
    assert len(buckets) > 4
    plain = batcher.BatcherFileList(root, 512, False, 1000, True, "test.list", check_ids=False)
    want_labels, want_paths, want_counts = [], [], []
    while True:
        got = plain.getBatch()
        if got is None:
            break
        labs, data, n, _cid = got
        want_labels.append(labs)
        want_paths.append(data.reshape((-1,) + data.shape[2:]))
        want_counts.append(np.full(n, data.shape[1], np.int32))
    merged = batcher.BatcherFileList(root, 512, False, 1000, True, "test.list", check_ids=False)
    got_labels, got_paths, got_counts, groups = [], [], [], 0
    while True:
        got = merged.getMergedGroup(max_paths)
        if got is None:
            break
        labs, idx, counts, n, cid = got
        assert cid == 1 and n == len(labs) == len(counts) and idx.shape[0] == counts.sum() and idx.dtype == np.int32 and idx.flags.c_contiguous
        assert idx.shape[0] <= max_paths or n == 1
        got_labels.append(labs); got_paths.append(idx); got_counts.append(counts)
        groups += 1
    assert np.array_equal(np.concatenate(got_counts), np.concatenate(want_counts))
    assert np.array_equal(np.concatenate(got_labels), np.concatenate(want_labels))
    assert np.array_equal(np.concatenate(got_paths), np.concatenate(want_paths))
    total = int(np.concatenate(want_counts).sum())
    assert groups >= -(-total // max_paths)
    if max_paths >= total:
        assert groups == 1   # the whole list, 17 path counts or so, in one engine call
    assert merged.getMergedGroup(max_paths) is None
    merged.reset()           # a second pass starts over
    assert merged.getMergedGroup(max_paths)[3] == len(got_labels[0])


def test_merged_mode_refuses_a_shuffled_list(tmp_path):
    root = str(tmp_path)
    _write_buckets(root, 500)
    fl = batcher.BatcherFileList(root, 512, True, 1000, True, "test.list", seed=1, check_ids=False)
    with pytest.raises(ValueError):
        fl.getMergedGroup(1000)


def test_shard_pairs_refuses_ragged_input():
    from kprn_amd import dp
    assert dp.shard_pairs(10, 1, 4) == (3, 6)
    with pytest.raises(TypeError):
        dp.shard_pairs(np.array([1, 2, 3], np.int32), 0, 2)
