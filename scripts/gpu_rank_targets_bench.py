"""Times kprn_rank_targets: against kprn_rank_groups where both apply, as the group and the target count grow, and inside the held-out
evaluation chain on the synthetic graph of scripts/gpu_candidates_top_bench.py.

  python scripts/gpu_rank_targets_bench.py [--reps 30 --groups 10000 --budget_s 420 --chain_users 256 --chain_cap 256 --users 80000 --items 20000
                                            --ratings 1000000 --out FILE --readme FILE]

Every stage starts only while the run is inside --budget_s (a stage that did not start is listed under "skipped"), and with --out the JSON is rewritten after
every stage, so a run cut short leaves what it measured.  Times are the host clock around the synchronous calls -- arguments up, one launch, results down --
as median [p10 .. p90] of --reps calls after one warm-up each, the variants alternating inside one loop; kernel_ms is one profiled call from the engine's
profiler.  Every timed result is compared with the host twin's (or, for the two kernels, with each other).
  against_rank_groups   --groups groups of 101 and of 4096 members, one target each (the positive of kprn_rank_groups)
  scaling               256 groups of 16 384 members with 1, 8 and 64 targets each; one group of 2^20 members with 1 and with 2000 targets
  chain                 graph.evaluate_from_graph over --chain_users held-out users at -max_candidates --chain_cap and uncapped: the whole call, and the
                        share of it spent inside Engine.rank_targets
--readme FILE writes the tables as markdown (profiles/rank_targets/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kprn_amd import _ffi, graph as kgraph  # noqa: E402


def spread(ts):
    """median and p10 .. p90 of the calls after the warm-up, in ms"""
    v = np.array(ts[1:]) * 1e3
    return dict(median_ms=round(float(np.median(v)), 4), p10_ms=round(float(np.percentile(v, 10)), 4), p90_ms=round(float(np.percentile(v, 90)), 4), n=len(v))


def alternate(variants, reps):
    """variants: {name: callable}; -> ({name: spread}, {name: last result})"""
    ts, last = {k: [] for k in variants}, {}
    for _ in range(reps + 1):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            last[name] = fn()
            ts[name].append(time.perf_counter() - t0)
    return {k: spread(v) for k, v in ts.items()}, last


def kernel_ms(eng, fn, prefix):
    eng.sync()
    eng.profile(True)
    fn()
    eng.sync()
    r = {k: round(v[0], 4) for k, v in eng.profile_get().items() if k.startswith(prefix)}
    eng.profile(False)
    return r


def draw(rng, n):
    """scores in [0, 1] whose "%.5f" prints tie often"""
    return (rng.randint(0, 2000, size=n) / 2000.0).astype(np.float32)


def fmt(s):
    return "%.3f [%.3f .. %.3f]" % (s["median_ms"], s["p10_ms"], s["p90_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--groups", type=int, default=10000); ap.add_argument("--budget_s", type=float, default=420)
    ap.add_argument("--chain_users", type=int, default=256); ap.add_argument("--chain_cap", type=int, default=256)
    ap.add_argument("--users", type=int, default=80000); ap.add_argument("--items", type=int, default=20000); ap.add_argument("--ratings", type=int, default=1000000)
    ap.add_argument("--out", default=""); ap.add_argument("--readme", default="")
    a = ap.parse_args()
    t_start = time.perf_counter()
    out = dict(reps=a.reps, skipped=[])

    def note():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(out) + "\n")

    def in_budget(name):
        if time.perf_counter() - t_start < a.budget_s:
            return True
        out["skipped"].append(name)
        return False

    rng = np.random.RandomState(7)
    eng = _ffi.Engine(4, 50, 4, 16, 32, 16, 64, 2)
    # ---- against kprn_rank_groups: one target per group
    out["against_rank_groups"] = {}
    for n in (101, 4096):
        if not in_budget("against_rank_groups_%d" % n):
            continue
        G = a.groups
        scores = draw(rng, G * n)
        eng.board_reserve(len(scores))
        eng.board_write(0, scores)
        goff = np.arange(G + 1, dtype=np.int64) * n
        pos = rng.randint(0, n, size=G).astype(np.int32)
        toff = np.arange(G + 1, dtype=np.int64)
        new = lambda: eng.rank_targets(goff, toff, pos, hist_len=15)
        old = lambda: eng.rank_groups(goff, pos=pos, hist_len=15)
        sp, last = alternate(dict(rank_targets=new, rank_groups=old), a.reps)
        out["against_rank_groups"][str(n)] = dict(groups=G, members=n, calls=sp, ratio=round(sp["rank_targets"]["median_ms"] / sp["rank_groups"]["median_ms"], 3),
                                                  kernel_ms=dict(kernel_ms(eng, new, "rank_"), **kernel_ms(eng, old, "rank_")),
                                                  equal=bool(np.array_equal(last["rank_targets"]["places"], last["rank_groups"]["ranks"])
                                                             and np.array_equal(last["rank_targets"]["hist"], last["rank_groups"]["hist"])))
        note()
    # ---- scaling: long groups, more targets
    out["scaling"] = {}
    shapes = [("256x16384_t%d" % k, 256, 16384, k) for k in (1, 8, 64)] + [("1x1048576_t1", 1, 1 << 20, 1), ("1x1048576_t2000", 1, 1 << 20, 2000)]
    for name, G, n, k in shapes:
        if not in_budget("scaling_" + name):
            continue
        scores = draw(rng, G * n)
        eng.board_reserve(len(scores))
        eng.board_write(0, scores)
        goff = np.arange(G + 1, dtype=np.int64) * n
        toff = np.arange(G + 1, dtype=np.int64) * k
        tg = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for _ in range(G)]).astype(np.int32)
        new = lambda: eng.rank_targets(goff, toff, tg, hist_len=15)
        sp, last = alternate(dict(rank_targets=new), a.reps)
        km = kernel_ms(eng, new, "rank_targets")       # (before the twin: a profiled call after seconds of host work would run on an idle device's clocks)
        host = _ffi.host_rank_targets(scores, goff, toff, tg, hist_len=15)
        out["scaling"][name] = dict(groups=G, members=n, targets=k, calls=sp, kernel_ms=km,
                                    equal=bool(np.array_equal(last["rank_targets"]["places"], host["places"]) and np.array_equal(last["rank_targets"]["hist"], host["hist"])))
        note()
    eng.close()
    # ---- the evaluation chain on the synthetic graph
    if a.chain_users > 0 and in_budget("chain"):
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
        t0 = time.perf_counter()
        train_kg, held = kg.holdout("rate", 0.8, 1)
        train_kg.relation_id = kg.relation_id
        out["chain"] = dict(users=a.chain_users, cap=a.chain_cap, holdout_s=round(time.perf_counter() - t0, 3), held=int(len(held)), edges_train=int(len(train_kg.src)))
        eng = _ffi.Engine(4, Ve, 4, 16, 32, 16, 64, 2)
        sm = eng.sampler(np.unique(train_kg.interactions("rate")[:, 1]))
        inner = eng.rank_targets
        spent = []

        def timed(*args, **kw):
            t1 = time.perf_counter()
            r = inner(*args, **kw)
            spent.append(time.perf_counter() - t1)
            return r
        eng.rank_targets = timed
        kgraph.evaluate_from_graph(eng, train_kg, held, sm, max_users=2, max_candidates=a.chain_cap)      # warm-up: two users through every stage
        for name, cap in (("capped", a.chain_cap), ("uncapped", 0)):
            if not in_budget("chain_" + name):
                continue
            del spent[:]
            t0 = time.perf_counter()
            try:
                r = kgraph.evaluate_from_graph(eng, train_kg, held, sm, max_users=a.chain_users, max_candidates=cap)
                total = time.perf_counter() - t0
                out["chain"][name] = dict(total_s=round(total, 4), rank_targets_s=round(sum(spent), 5), rank_share=round(sum(spent) / total, 5), calls=len(spent),
                                          samples=r["n"], unreachable=r["n_unreachable"], zero=r["n_zero"], hit_at_10=round(r["hits"][10], 5))
            except _ffi.KprnError as ex:
                out["chain"][name] = dict(error=str(ex))
            note()
        eng.close()
    note()
    print(json.dumps(out))
    if a.readme:
        lines = ["# kprn_rank_targets: measurements", "",
                 "Written by `scripts/gpu_rank_targets_bench.py --readme` on one MI355X; host clock around the synchronous call, median [p10 .. p90] ms of %d calls" % a.reps,
                 "after a warm-up, variants alternating inside one loop.  Windows of milliseconds from one run: read ratios, not digits.  Not tuned.", "",
                 "## Against kprn_rank_groups (one target per group)", "", "| groups x members | rank_targets | rank_groups | ratio | kernels (ms) | equal |", "|---|---|---|---|---|---|"]
        for n, r in out["against_rank_groups"].items():
            lines.append("| %d x %s | %s | %s | %.2f | %s | %s |" % (r["groups"], n, fmt(r["calls"]["rank_targets"]), fmt(r["calls"]["rank_groups"]), r["ratio"],
                                                                  json.dumps(r["kernel_ms"]), r["equal"]))
        lines += ["", "## Scaling", "", "| shape | targets per group | call | kernel (ms) | equal to the twin |", "|---|---|---|---|---|"]
        for name, r in out["scaling"].items():
            lines.append("| %d x %d | %d | %s | %s | %s |" % (r["groups"], r["members"], r["targets"], fmt(r["calls"]["rank_targets"]), json.dumps(r["kernel_ms"]), r["equal"]))
        if "chain" in out:
            lines += ["", "## The evaluation chain (graph.evaluate_from_graph, %d users, 64 per call)" % out["chain"]["users"], "",
                      "| variant | whole call | inside rank_targets | share | samples, unreachable, zero |", "|---|---|---|---|---|"]
            for name in ("capped", "uncapped"):
                r = out["chain"].get(name)
                if r and "total_s" in r:
                    lines.append("| %s | %.3f s | %.4f s in %d calls | %.2f %% | %d, %d, %d |" % (name, r["total_s"], r["rank_targets_s"], r["calls"], 100 * r["rank_share"],
                                                                                           r["samples"], r["unreachable"], r["zero"]))
                elif r:
                    lines.append("| %s | %s | | | |" % (name, r["error"]))
        if out["skipped"]:
            lines += ["", "Not measured (the run's time budget ended first): " + ", ".join(out["skipped"])]
        with open(a.readme, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
