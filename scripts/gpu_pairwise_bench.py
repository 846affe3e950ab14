"""Times a training step from a graph under the pairwise loss against the same step under BCE, in the setting of scripts/gpu_neg_sample_bench.py
(DESIGN.md 3.14, 3.17): 128 positives (rated user-item edges) x 4 negatives drawn from the items with weight (ratings)^0.75, 2..3 hops, a cap of 28
paths per pair, the fused two-layer D = H = 64 model.

  python scripts/gpu_pairwise_bench.py [--users 80000 --items 20000 --ratings 1000000 --positives 128 --negatives 4 --reps 200 --warmup 20]

Prints one JSON line.  Every repetition finds a fresh minibatch (not timed), then runs one step with "loss" = "bce" and one with "loss" = "bpr" on it,
alternating inside the one loop so that they share whatever else the host and the device are doing.  Whichever step goes first on a fresh minibatch also
pays for the lazy optimiser's catch-up of the batch's entity rows, so the order flips every repetition.  Host clock, milliseconds, median (p10, p90) of
--reps after --warmup:
  bce         kprn_train_step_batch + kprn_sync
  bpr         kprn_batch_set_groups + kprn_train_step_batch + kprn_sync
  set_groups  kprn_batch_set_groups alone (one upload, one counting launch, one wait)
and the profiler's loss_stage / loss_stage_pairwise entries of one step each, with the batch's pairs, groups and terms."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi, graph as kgraph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=80000); ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--ratings", type=int, default=1000000); ap.add_argument("--positives", type=int, default=128)
    ap.add_argument("--negatives", type=int, default=4); ap.add_argument("--attempts", type=int, default=16); ap.add_argument("--cap", type=int, default=28)
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.RandomState(7)
    pop = 1.0 / (np.arange(a.items) + 10.0) ** 0.8
    u = rng.randint(1, a.users + 1, size=a.ratings).astype(np.int32)
    it = (a.users + 1 + rng.choice(a.items, size=a.ratings, p=pop / pop.sum())).astype(np.int32)
    src, dst = np.concatenate([u, it]), np.concatenate([it, u])
    rel = np.concatenate([np.full(a.ratings, 1, np.int32), np.full(a.ratings, 2, np.int32)])
    Ve, Vr, Vt, end_rel = a.users + a.items + 1, 4, 4, 3
    nt = np.ones((Ve, 1), np.int32)
    nt[a.users:] = 2
    items = np.arange(a.users + 1, a.users + a.items + 1, dtype=np.int32)
    weights = (np.bincount(it, minlength=Ve + 1)[items].astype(np.float64) ** 0.75).astype(np.float32)
    pick = rng.choice(a.ratings, size=(a.reps + a.warmup, a.positives))
    positives = np.stack([u[pick], it[pick]], axis=2).astype(np.int32)
    eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2)
    gr = eng.graph(src, dst, rel, nt, end_rel)
    s = eng.sampler(items, weights)
    opt = _ffi.make_opt(method=1, lr=1e-3)
    ts = dict(bce=[], bpr=[], set_groups=[])
    shape = {}

    def step(k, timed):
        batch, _, counts, _ = eng.find_training_paths(gr, s, positives[k], a.negatives, 1, k, 2, 3, a.cap, 4, max_attempts=a.attempts)
        go = kgraph.groups_from_counts(counts, a.negatives)
        eng.sync()
        took = {}

        def bce():
            eng.set_option("loss", "bce")
            t0 = time.perf_counter()
            eng.train_step(batch, opt)
            eng.sync()
            took["bce"] = time.perf_counter() - t0

        def bpr():
            eng.set_option("loss", "bpr")
            t0 = time.perf_counter()
            terms = batch.set_groups(go)
            t1 = time.perf_counter()
            eng.train_step(batch, opt)
            eng.sync()
            took["bpr"], took["set_groups"] = time.perf_counter() - t0, t1 - t0
            shape.update(pairs=batch.B, paths=batch.n_paths, groups=len(go) - 1, n_terms=terms)

        for run in ((bce, bpr) if k % 2 == 0 else (bpr, bce)):
            run()
        batch.free()
        if timed:
            for name, dt in took.items():
                ts[name].append(dt * 1e3)

    for k in range(a.warmup + a.reps):
        step(k, k >= a.warmup)
    out = dict(nodes=Ve - 1, positives=a.positives, negatives=a.negatives, cap=a.cap, reps=a.reps, warmup=a.warmup, last_batch=dict(shape))
    for name, v in ts.items():
        out[name + "_ms"] = [round(float(x), 4) for x in (np.median(v), np.percentile(v, 10), np.percentile(v, 90))]
    out["bpr_over_bce"] = round(float(np.median(ts["bpr"]) / np.median(ts["bce"])), 3)
    eng.profile(True)
    eng.profile_reset()
    step(0, False)
    out["kernels_ms"] = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith("loss_stage")}
    eng.profile(False)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
