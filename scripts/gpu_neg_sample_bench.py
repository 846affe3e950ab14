"""Times kprn_find_training_paths against what it fuses, on the synthetic graph of scripts/gpu_path_find_bench.py: 128 positives
(rated user-item edges) x 4 negatives drawn from the items with weight (ratings)^0.75, 2..3 hops, a cap of 28 paths per pair.

  python scripts/gpu_neg_sample_bench.py [--users 80000 --items 20000 --ratings 1000000 --positives 128 --negatives 4 --reps 200 --warmup 20]

Prints one JSON line.  Host clock around calls that each end in a device wait, in milliseconds: median (p10, p90) of --reps calls after --warmup, the
variants alternating inside one loop so that they share whatever else the host and the device are doing:
  fused     kprn_find_training_paths (+ freeing the batch)
  two_call  kprn_sample_negatives, the pair list formed in numpy, kprn_find_paths with labels (+ freeing the batch)
  sample    kprn_sample_negatives alone
  find      kprn_find_paths alone on the pair list of the first draw (+ freeing the batch)
  twin      kprn_host_sample_negatives on --threads host threads (it sorts the edge arrays into a CSR on every call; median of 3)
and whether the fused call's outputs equalled the composition's on the first draw."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi  # noqa: E402


def pair_list(pos, neg):
    B, n = neg.shape
    prs = np.zeros((B, 1 + n, 2), np.int32)
    prs[:, :, 0] = pos[:, :1]
    prs[:, 0, 1] = pos[:, 1]
    prs[:, 1:, 1] = neg
    prs = prs.reshape(-1, 2)
    labels = np.zeros(len(prs), np.float32)
    labels[::1 + n] = 1
    real = prs[:, 1] != 0
    return prs, labels, real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=80000); ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--ratings", type=int, default=1000000); ap.add_argument("--positives", type=int, default=128)
    ap.add_argument("--negatives", type=int, default=4); ap.add_argument("--attempts", type=int, default=16); ap.add_argument("--cap", type=int, default=28)
    ap.add_argument("--threads", type=int, default=16); ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
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
    positives = np.stack([u[pick], it[pick]], axis=2).astype(np.int32)                    # a fresh minibatch of rated pairs per call
    out = dict(nodes=Ve - 1, edges_in=int(src.shape[0]), positives=a.positives, negatives=a.negatives, attempts=a.attempts, hops="2..3", cap=a.cap,
               reps=a.reps, warmup=a.warmup)
    eng = _ffi.Engine(Vt, Ve, Vr, 16, 32, 16, 64, 2)
    gr = eng.graph(src, dst, rel, nt, end_rel)
    s = eng.sampler(items, weights)
    args = (2, 3, a.cap, 4)

    def fused(pos, draw):
        b, prs, c, f = eng.find_training_paths(gr, s, pos, a.negatives, 1, draw, *args, max_attempts=a.attempts)
        return b, prs, c, f

    def two_call(pos, draw):
        neg, _ = eng.sample_negatives(gr, s, pos[:, 0], a.negatives, 1, draw, max_attempts=a.attempts)
        prs, labels, real = pair_list(pos, neg)
        b, c, f = eng.find_paths(gr, prs[real], *args, labels=labels[real])
        return b, prs, c, f, real

    bf, pf_, cf, ff = fused(positives[0], 0)
    bt, pt, ct, ft, real = two_call(positives[0], 0)
    out["fused_equals_two_call"] = bool(np.array_equal(pf_, pt) and np.array_equal(cf[real], ct) and np.array_equal(ff[real], ft) and not cf[~real].any()
                                        and np.array_equal(bf.read_idx(), bt.read_idx()) and np.array_equal(bf.counts, bt.counts))
    out.update(pairs=int(len(pt)), pairs_with_paths=int((cf > 0).sum()), paths_kept=int(cf.sum()), empty_negative_slots=int((~real).sum()))
    bf.free(); bt.free()
    fixed, fixed_labels, fixed_real = pair_list(positives[0], eng.sample_negatives(gr, s, positives[0][:, 0], a.negatives, 1, 0, max_attempts=a.attempts)[0])
    ts = dict(fused=[], two_call=[], sample=[], find=[])
    for k in range(a.warmup + a.reps):
        pos = positives[k]
        t0 = time.perf_counter()
        b = fused(pos, k)[0]
        if b is not None:
            b.free()
        t1 = time.perf_counter()
        b = two_call(pos, k)[0]
        if b is not None:
            b.free()
        t2 = time.perf_counter()
        eng.sample_negatives(gr, s, pos[:, 0], a.negatives, 1, k, max_attempts=a.attempts)
        t3 = time.perf_counter()
        b = eng.find_paths(gr, fixed[fixed_real], *args, labels=fixed_labels[fixed_real])[0]
        if b is not None:
            b.free()
        t4 = time.perf_counter()
        if k >= a.warmup:
            for name, dt in zip(("fused", "two_call", "sample", "find"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                ts[name].append(dt * 1e3)
    for name, v in ts.items():
        out[name + "_ms"] = [round(float(x), 4) for x in (np.median(v), np.percentile(v, 10), np.percentile(v, 90))]
    out["fused_over_two_call"] = round(float(np.median(ts["fused"]) / np.median(ts["two_call"])), 3)
    eng.profile(True)
    b = fused(positives[0], 0)[0]
    b.free()
    eng.sync()
    out["kernels_ms"] = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith(("find_paths", "sample_negatives"))}
    eng.close()
    tw = []
    for k in range(3):
        t0 = time.perf_counter()
        _ffi.host_sample_negatives(src, dst, rel, Ve, items, weights, positives[k][:, 0], a.negatives, 1, k, max_attempts=a.attempts, threads=a.threads)
        tw.append((time.perf_counter() - t0) * 1e3)
    out["twin_ms"] = round(float(np.median(tw)), 2)
    out["threads"] = a.threads
    print(json.dumps(out))


if __name__ == "__main__":
    main()
