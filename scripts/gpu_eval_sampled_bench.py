"""Times held-out evaluation under the two protocols: every held pair among everything its user reaches (eval_negatives 0) against every
held pair among 100 drawn negatives (eval_negatives 100), on the synthetic graph and model of scripts/gpu_rank_targets_bench.py.

  python scripts/gpu_eval_sampled_bench.py [--reps 5 --chain_users 256 --negatives 100 --users 80000 --items 20000 --ratings 1000000 --out FILE]

One process.  Times are the host clock around graph.evaluate_from_graph, median [min .. max] of --reps calls after a warm-up of two users through every stage,
the two protocols alternating inside one loop.  Per protocol: seconds per call, ms per held pair, the pairs scored (the batches' pairs summed over the
forward passes), and for the sampled protocol the share of the call spent inside Engine.sample_eval_groups (the new stage with its read-back of the cut
list).  The full protocol's result is compared between the reps, the sampled one's too: both are deterministic."""
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
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--chain_users", type=int, default=256); ap.add_argument("--negatives", type=int, default=100)
    ap.add_argument("--users", type=int, default=80000); ap.add_argument("--items", type=int, default=20000); ap.add_argument("--ratings", type=int, default=1000000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.RandomState(7)
    pop = 1.0 / (np.arange(a.items) + 10.0) ** 0.8
    u = rng.randint(1, a.users + 1, size=a.ratings).astype(np.int32)
    it = (a.users + 1 + rng.choice(a.items, size=a.ratings, p=pop / pop.sum())).astype(np.int32)
    src, dst = np.concatenate([u, it]), np.concatenate([it, u])
    rel = np.concatenate([np.full(a.ratings, 1, np.int32), np.full(a.ratings, 2, np.int32)])
    Ve = a.users + a.items + 1
    nt = np.ones((Ve, 1), np.int32)
    nt[a.users:] = 2
    kg = kgraph.KnowledgeGraph(src, dst, rel, nt, 3, 4, 4)
    kg.relation_id = lambda name: 1
    train_kg, held = kg.holdout("rate", 0.8, 1)
    train_kg.relation_id = kg.relation_id
    eng = _ffi.Engine(4, Ve, 4, 16, 32, 16, 64, 2)
    sm = eng.sampler(np.unique(train_kg.interactions("rate")[:, 1]))
    scored, spent = [0], [0.0]
    fwd, stage = eng.forward_async, eng.sample_eval_groups

    def counted(batch, *args, **kw):
        scored[0] += batch.B
        return fwd(batch, *args, **kw)

    def timed(*args, **kw):
        t1 = time.perf_counter()
        r = stage(*args, **kw)
        spent[0] += time.perf_counter() - t1
        return r
    eng.forward_async, eng.sample_eval_groups = counted, timed
    for n in (0, a.negatives):
        kgraph.evaluate_from_graph(eng, train_kg, held, sm, max_users=2, eval_negatives=n)       # warm-up: two users through every stage
    protocols = (("full", 0), ("sampled", a.negatives))
    ts, stage_s, res = {k: [] for k, _ in protocols}, [], {}
    same = {k: True for k, _ in protocols}
    for _ in range(a.reps):
        for name, n in protocols:
            scored[0], spent[0] = 0, 0.0
            t0 = time.perf_counter()
            r = kgraph.evaluate_from_graph(eng, train_kg, held, sm, max_users=a.chain_users, eval_negatives=n)
            ts[name].append(time.perf_counter() - t0)
            if name in res:
                same[name] = same[name] and bool(np.array_equal(res[name][0]["places"], r["places"]))
            res[name] = (r, scored[0])
            if n:
                stage_s.append(spent[0])
    eng.close()
    out = dict(users=a.chain_users, negatives=a.negatives, reps=a.reps, edges_train=int(len(train_kg.src)))
    for name, _ in protocols:
        r, pairs = res[name]
        v = np.array(ts[name])
        out[name] = dict(median_s=round(float(np.median(v)), 4), min_s=round(float(v.min()), 4), max_s=round(float(v.max()), 4), held_pairs=int(r["n"]),
                         ms_per_held_pair=round(1e3 * float(np.median(v)) / max(int(r["n"]), 1), 4), pairs_scored=int(pairs), unreachable=int(r["n_unreachable"]),
                         zero=int(r["n_zero"]), hit_at_10=round(r["hits"][10], 5), same_every_rep=same[name])
    out["sampled"]["short"] = int(res["sampled"][0]["n_short"])
    out["sampled"]["stage_s"] = round(float(np.median(stage_s)), 5)
    out["sampled"]["stage_share"] = round(float(np.median(stage_s)) / out["sampled"]["median_s"], 5)
    out["full_over_sampled"] = round(out["full"]["median_s"] / out["sampled"]["median_s"], 3)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
