#!/usr/bin/env python3
"""What ragged batches (pairs with different path counts in one batch) buy and cost.  One JSON object from one process; every comparison is three
alternating (a, b) pairs after a warm-up, timed with a device synchronise.

1. scoring a make_bucketed set of ~1 M paths (T = 6, D = H = 64, L = 2, headline tables): bucket by bucket through scoring.score_batches
   against merged ragged groups (merge=True): paths/s each;
2. one user's 101 candidate pairs (counts from draw_num_paths): one forward_host per distinct count against one forward_ragged_host: us per user;
3. a training step on a ragged batch whose counts are all equal against the rectangular batch of the same data, 65 536 paths (bench.py's default
   --paths-per-step), P = 2: ms per step.  This isolates the segmented pooling / loss stages; the spread of the three pairs is reported.

usage: gpu_ragged_probe.py [total_paths]"""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kprn_amd import _ffi, formats, scoring, synth  # noqa: E402
from kprn_amd.batcher import BatcherFileList  # noqa: E402

total = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
Vt, Ve, Vr, T = 6, 2851220, 9, 6
eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2, seed=1)
res = {"what": "ragged batches: merged scoring, one-call candidate ranking, segmented stages in a training step", "T": T, "D": 64, "H": 64, "L": 2, "Ve": Ve}


def timed(fn):
    eng.sync()
    t0 = time.perf_counter()
    fn()
    eng.sync()
    return time.perf_counter() - t0


def alternate(a, b, pairs=3):
    a(); b()   # warm-up: allocations, first-launch costs
    ta, tb = [], []
    for _ in range(pairs):
        ta.append(timed(a))
        tb.append(timed(b))
    return ta, tb


# ---- 1: bucket files, unmerged against merged --------------------------------------------------------------------------------------
d = tempfile.mkdtemp(prefix="kprn_ragged_")
buckets = synth.make_bucketed(total, T, Ve=Ve, seed=77)
names, n_paths, n_pairs = [], 0, 0
for P in sorted(buckets):
    idx, labels = buckets[P]
    nm = "test_%d.npz" % P
    formats.save_path_file(os.path.join(d, nm), labels, idx, 1)
    names.append(nm)
    n_paths += idx.shape[0] * P
    n_pairs += idx.shape[0]
with open(os.path.join(d, "test.list"), "w") as f:
    f.write("\n".join(names) + "\n")
fl = BatcherFileList(d, 512, False, 1000, True, "test.list", check_ids=False)   # files read once; reset() between the passes
got = {}


def score(merge):
    def run():
        fl.reset()
        got[merge] = np.concatenate([p for _, p in scoring.score_batches(eng, fl, 1, merge=merge)])
    return run


t_plain, t_merged = alternate(score(False), score(True))
assert got[False].shape == got[True].shape == (n_pairs,)
res["scoring"] = {"paths": n_paths, "pairs": n_pairs, "buckets": {int(P): int(buckets[P][0].shape[0] * P) for P in sorted(buckets)},
                  "bucket_by_bucket_s": [round(x, 4) for x in t_plain], "merged_s": [round(x, 4) for x in t_merged],
                  "bucket_by_bucket_paths_per_s": round(n_paths / min(t_plain)), "merged_paths_per_s": round(n_paths / min(t_merged)),
                  "max_rel_diff": float(np.max(np.abs(got[True] - got[False]) / np.abs(got[False])))}

# ---- 2: one user's candidates ---------------------------------------------------------------------------------------------------------
counts = synth.draw_num_paths(np.random.default_rng(7), 101)
cidx, _, _ = synth.make_ragged(101, T, Ve=Ve, seed=25, counts=counts)
off = np.concatenate([[0], np.cumsum(counts)])
per_count = []
for P in np.unique(counts):
    pairs = np.nonzero(counts == P)[0]
    rows = (off[pairs][:, None] + np.arange(int(P))[None, :]).reshape(-1)
    per_count.append(np.ascontiguousarray(cidx[rows].reshape(len(pairs), int(P), T, 3)))
REP = 200


def per_count_calls():
    for _ in range(REP):
        for a in per_count:
            eng.forward_host(a, 1, want_all=False)


def one_call():
    for _ in range(REP):
        eng.forward_ragged_host(cidx, counts, 1)


t_pc, t_one = alternate(per_count_calls, one_call)
res["candidates"] = {"pairs": 101, "paths": int(counts.sum()), "distinct_counts": len(per_count),
                     "per_count_us_per_user": [round(1e6 * x / REP, 1) for x in t_pc], "one_call_us_per_user": [round(1e6 * x / REP, 1) for x in t_one]}

# ---- 3: the segmented stages inside a training step ----------------------------------------------------------------------------------
P = 2
idx, labels = synth.make_paths(65536 // P, P, T, Ve=Ve, seed=9)
rect = eng.batch(idx, labels)
rag = eng.batch_ragged(idx.reshape((-1, T, 3)), np.full(idx.shape[0], P, np.int32), labels)
opt = _ffi.make_opt(method=1, lr=1e-3)
STEPS = 20


def steps(b):
    def run():
        for _ in range(STEPS):
            eng.train_step(b, opt, 1, want_loss=False)
    return run


t_rect, t_rag = alternate(steps(rect), steps(rag))
res["train_step"] = {"paths": 65536, "P": P, "rectangular_ms_per_step": [round(1e3 * x / STEPS, 4) for x in t_rect],
                     "ragged_equal_counts_ms_per_step": [round(1e3 * x / STEPS, 4) for x in t_rag]}
shutil.rmtree(d, ignore_errors=True)
print(json.dumps(res))
